// ransac_host.h on the CPU (g++ -ffp-contract=off -fsanitize=address,undefined).
//   ransac_host_test masks   mask_to_bytes over random words against a per-bit loop; both arrays are heap blocks of exactly
//                            the documented length, so that a read or write past either end is an ASan report
//   ransac_host_test table   one line per line of stdin, "n min_inliers <float eps as hex bits> <double probability as hex
//                            bits> max_iterations": prints ransac_max_iterations of it (tests/test_workspace.py compares
//                            the lines with tests/sim3_model.py and tests/pnp_model.py)
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>

#include "ransac_host.h"

static int masks()
{
    std::mt19937_64 rng(7);
    for (int n : {0, 1, 63, 64, 65, 130})
        for (int round = 0; round < 8; round++) {
            const size_t words = ((size_t)n + 63) / 64;
            std::unique_ptr<uint64_t[]> mask(new uint64_t[words]);
            std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)n]);
            for (size_t w = 0; w < words; w++)
                mask[w] = round == 0 ? 0 : round == 1 ? ~(uint64_t)0 : rng();
            std::memset(out.get(), 0xee, (size_t)n);
            orbgpu::mask_to_bytes(mask.get(), n, out.get());
            for (int i = 0; i < n; i++) {
                const uint64_t word = mask[(size_t)(i / 64)];
                const int bit = (int)((word >> (i % 64)) % 2);
                if (out[i] != bit) {
                    std::printf("n %d round %d: byte %d is %d, bit is %d\n", n, round, i, out[i], bit);
                    return 1;
                }
            }
        }
    std::printf("mask_to_bytes ok\n");
    return 0;
}

static int table()
{
    int n, min_inliers, max_iterations;
    unsigned eps_bits;
    unsigned long long p_bits;
    while (std::scanf("%d %d %x %llx %d", &n, &min_inliers, &eps_bits, &p_bits, &max_iterations) == 5) {
        float eps;
        double probability;
        const uint32_t e32 = eps_bits;
        const uint64_t p64 = p_bits;
        std::memcpy(&eps, &e32, sizeof(eps));
        std::memcpy(&probability, &p64, sizeof(probability));
        std::printf("%d\n", orbgpu::ransac_max_iterations(n, min_inliers, eps, probability, max_iterations));
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "masks"))
        return masks();
    if (argc == 2 && !std::strcmp(argv[1], "table"))
        return table();
    std::printf("usage: ransac_host_test masks | table\n");
    return 2;
}

// fast_polarity.h on the CPU: the single-network corner score with the polarity selector (what fast_score_pk computes)
// against the two-network definition.
//   - for c in {0, 1, 128, 254, 255}: every ring over {c-1, c+1} with c itself at up to 4 positions (14.6 M rings per
//     centre), values outside 0..255 skipped; with the argument "full" instead every ring whose pixels are each one
//     of c-1, c, c+1 (3^16 rings per centre: 20 s of CPU time, the reduced set 3 s);
//   - random rings: values in the full range and in narrow ranges round the centre, with planted arcs of length 7..11
//     of both signs.
// Also checked on every ring: at most one of the two terms is positive, a dark arc has H < c, a bright arc H > c.
// Prints "fast_polarity_test ok <rings>" and returns 0, or the first mismatch and 1.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "fast_polarity.h"

using namespace orbgpu_fast;

static std::atomic<int> g_bad{0};

static inline void check(int c, const uint8_t v[16], unsigned long long &n)
{
    n++;
    const TwoTerms t = fast_terms_two_networks(c, v);
    const int ref = t.dark > t.bright ? (t.dark > 0 ? t.dark : 0) : (t.bright > 0 ? t.bright : 0);
    const int got = fast_score_one_network(c, v);
    const int H = fast_selector(v);
    const bool ok = got == ref && !(t.dark > 0 && t.bright > 0) && !(t.dark > 0 && !(H < c)) && !(t.bright > 0 && !(H > c));
    if (!ok && g_bad.fetch_add(1) == 0) {
        std::fprintf(stderr, "mismatch: c %d ring", c);
        for (int k = 0; k < 16; k++)
            std::fprintf(stderr, " %d", v[k]);
        std::fprintf(stderr, ": two networks %d (dark %d bright %d), one network %d, H %d\n", ref, t.dark, t.bright, got, H);
    }
}

// rings over {c-1, c, c+1} whose three leading digits are `chunk` (27 chunks)
static unsigned long long exhaustive_chunk(int c, int chunk)
{
    unsigned long long n = 0;
    int d[16];
    uint8_t v[16];
    for (int k = 0; k < 16; k++)
        d[k] = 0;
    d[13] = chunk % 3, d[14] = chunk / 3 % 3, d[15] = chunk / 9;
    for (int k = 13; k < 16; k++)
        if (c - 1 + d[k] < 0 || c - 1 + d[k] > 255)
            return 0;
    const int lo = c == 0 ? 1 : 0, hi = c == 255 ? 1 : 2;  // digits in range
    for (int k = 0; k < 13; k++)
        d[k] = lo;
    for (;;) {
        for (int k = 0; k < 16; k++)
            v[k] = (uint8_t)(c - 1 + d[k]);
        check(c, v, n);
        int k = 0;
        while (k < 13 && d[k] == hi)
            d[k++] = lo;
        if (k == 13)
            break;
        d[k]++;
    }
    return n;
}

// rings over {c-1, c+1} with c at the positions of zmask, for every zmask of at most 4 bits whose low nibble is `chunk`
static unsigned long long reduced_chunk(int c, int chunk)
{
    unsigned long long n = 0;
    uint8_t v[16];
    for (unsigned zmask = (unsigned)chunk; zmask < 65536u; zmask += 16u) {
        if (__builtin_popcount(zmask) > 4)
            continue;
        const unsigned freeb = ~zmask & 0xFFFFu;
        unsigned bits = 0;
        do {  // bits runs over the subsets of freeb: set = c+1, clear = c-1
            if (!((c == 0 && (~bits & freeb)) || (c == 255 && bits))) {
                for (int k = 0; k < 16; k++)
                    v[k] = (uint8_t)((zmask >> k & 1u) ? c : (bits >> k & 1u) ? c + 1 : c - 1);
                check(c, v, n);
            }
            bits = (bits - freeb) & freeb;
        } while (bits);
    }
    return n;
}

static unsigned long long random_rings(uint64_t seed, int count)
{
    unsigned long long n = 0;
    std::mt19937_64 rng(seed);
    auto below = [&](int m) { return (int)(rng() % (uint64_t)m); };
    uint8_t v[16];
    for (int it = 0; it < count; it++) {
        const int c = below(256);
        const int mode = below(4);
        const int span = mode == 0 ? 256 : mode == 1 ? 3 : mode == 2 ? 9 : 41;  // full range, or c +- 1, 4, 20
        auto clampb = [](int x) { return (uint8_t)(x < 0 ? 0 : x > 255 ? 255 : x); };
        for (int k = 0; k < 16; k++)
            v[k] = span == 256 ? (uint8_t)below(256) : clampb(c - span / 2 + below(span));
        if (below(4) != 0) {  // a planted arc of 7..11 pixels, all above or all below the centre
            const int len = 7 + below(5), start = below(16), sign = below(2) ? 1 : -1, depth = 1 + below(mode == 0 ? 120 : 12);
            for (int k = 0; k < len; k++)
                v[(start + k) & 15] = clampb(c + sign * (depth + below(6)));
        }
        check(c, v, n);
    }
    return n;
}

int main(int argc, char **argv)
{
    const bool full = argc > 1 && std::string(argv[1]) == "full";
    static const int centres[5] = {0, 1, 128, 254, 255};
    const int per = full ? 27 : 16, jobs = 5 * per + 8;
    std::atomic<int> next{0};
    std::atomic<unsigned long long> total{0};
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : nt > 8 ? 8 : nt;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++)
        th.emplace_back([&] {
            for (int j; (j = next.fetch_add(1)) < jobs;)
                total += j >= 5 * per ? random_rings(1000 + (uint64_t)(j - 5 * per), 500000)
                         : full ? exhaustive_chunk(centres[j / per], j % per)
                                : reduced_chunk(centres[j / per], j % per);
        });
    for (auto &t : th)
        t.join();
    if (g_bad.load()) {
        std::fprintf(stderr, "fast_polarity_test: %d rings differ\n", g_bad.load());
        return 1;
    }
    std::printf("fast_polarity_test ok %llu\n", total.load());
    return 0;
}

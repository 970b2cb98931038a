// carve.h on the CPU (g++ -fsanitize=address,undefined): the offsets Carver hands out at both alignments in use, and the
// staging layouts of the three host flavours (orbgpu_sim3_solve*, orbgpu_pnp_solve*, orbgpu_sim3_optimize) against the
// hand-summed formulas those entry points held before they took their offsets from a 16-aligned Carver.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "carve.h"
#include "orbgpu.h"

using orbgpu::Carver;

#define CHECK(c)                                                                \
    do {                                                                        \
        if (!(c)) {                                                             \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c);   \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

static void sequence(Carver c, size_t A)
{
    const size_t sizes[] = {0, 1, 15, 16, 17, 255, 256, 257};
    size_t prev = 0, end_of_last = 0;
    CHECK(c.off == 0);
    for (size_t bytes : sizes) {
        const size_t o = c.take(bytes);
        CHECK(o == prev && o % A == 0);
        CHECK(o >= end_of_last);  // no overlap with the segment before
        CHECK(c.off == ((prev + bytes + A - 1) & ~(A - 1)));
        CHECK(c.off % A == 0 && c.off >= o + bytes && c.off < o + bytes + A);
        end_of_last = o + bytes;
        prev = c.off;
    }
}

static size_t pad(size_t b) { return (b + 15) & ~(size_t)15; }

static void same(const std::vector<size_t> &carved, const std::vector<size_t> &by_hand)
{
    CHECK(carved.size() == by_hand.size());
    for (size_t i = 0; i < carved.size(); i++)
        CHECK(carved[i] == by_hand[i]);
}

// the last element of each list is the block's size
static void sim3_layout(int n1, int H)
{
    const size_t words = (size_t)(n1 + 63) / 64, c1 = (size_t)std::max(n1, 1), cH = (size_t)std::max(H, 1);
    const size_t i_valid = 0, i_x1 = i_valid + pad(c1), i_x2 = i_x1 + pad(12 * c1), i_o1 = i_x2 + pad(12 * c1),
                 i_o2 = i_o1 + pad(4 * c1), i_tr = i_o2 + pad(4 * c1), in_bytes = i_tr + pad(12 * cH);
    const size_t o_res = 0, o_cnt = o_res + pad(sizeof(orbgpu_sim3_result)), o_R = o_cnt + pad(4 * cH), o_t = o_R + pad(36 * cH),
                 o_s = o_t + pad(12 * cH), o_T = o_s + pad(4 * cH), o_m = o_T + pad(64 * cH),
                 out_bytes = o_m + pad(8 * cH * std::max<size_t>(words, 1));
    Carver in(16), out(16);
    const std::vector<size_t> a = {in.take(c1),     in.take(12 * c1), in.take(12 * c1), in.take(4 * c1),
                                   in.take(4 * c1), in.take(12 * cH), in.off};
    same(a, {i_valid, i_x1, i_x2, i_o1, i_o2, i_tr, in_bytes});
    const std::vector<size_t> b = {out.take(sizeof(orbgpu_sim3_result)), out.take(4 * cH), out.take(36 * cH), out.take(12 * cH),
                                   out.take(4 * cH), out.take(64 * cH), out.take(8 * cH * std::max<size_t>(words, 1)), out.off};
    same(b, {o_res, o_cnt, o_R, o_t, o_s, o_T, o_m, out_bytes});
}

static void pnp_layout(int n1, int H, int ms)
{
    const size_t words = (size_t)(n1 + 63) / 64, c1 = (size_t)std::max(n1, 1), cH = (size_t)std::max(H, 1), w1 = std::max<size_t>(words, 1);
    const size_t i_valid = 0, i_x = i_valid + pad(c1), i_kp = i_x + pad(12 * c1), i_o = i_kp + pad(8 * c1), i_s = i_o + pad(4 * c1),
                 in_bytes = i_s + pad(4 * cH * (size_t)ms);
    const size_t o_res = 0, o_cnt = o_res + pad(sizeof(orbgpu_pnp_result)), o_T = o_cnt + pad(4 * cH), o_rm = o_T + pad(64 * cH),
                 o_m = o_rm + pad(8 * w1), out_bytes = o_m + pad(8 * cH * w1);
    Carver in(16), out(16);
    const std::vector<size_t> a = {in.take(c1), in.take(12 * c1), in.take(8 * c1), in.take(4 * c1), in.take(4 * cH * (size_t)ms),
                                   in.off};
    same(a, {i_valid, i_x, i_kp, i_o, i_s, in_bytes});
    const std::vector<size_t> b = {out.take(sizeof(orbgpu_pnp_result)), out.take(4 * cH), out.take(64 * cH), out.take(8 * w1),
                                   out.take(8 * cH * w1), out.off};
    same(b, {o_res, o_cnt, o_T, o_rm, o_m, out_bytes});
}

static void sim3_opt_layout(int n1)
{
    const size_t c1 = (size_t)std::max(n1, 1);
    const size_t i_valid = 0, i_x1 = i_valid + pad(c1), i_x2 = i_x1 + pad(12 * c1), i_o1 = i_x2 + pad(12 * c1),
                 i_o2 = i_o1 + pad(4 * c1), i_k1 = i_o2 + pad(4 * c1), i_k2 = i_k1 + pad(8 * c1), in_bytes = i_k2 + pad(8 * c1);
    const size_t o_res = 0, o_inl = o_res + pad(sizeof(orbgpu_sim3_opt_result)), out_bytes = o_inl + pad(c1);
    Carver in(16), out(16);
    const std::vector<size_t> a = {in.take(c1),     in.take(12 * c1), in.take(12 * c1), in.take(4 * c1),
                                   in.take(4 * c1), in.take(8 * c1),  in.take(8 * c1),  in.off};
    same(a, {i_valid, i_x1, i_x2, i_o1, i_o2, i_k1, i_k2, in_bytes});
    const std::vector<size_t> b = {out.take(sizeof(orbgpu_sim3_opt_result)), out.take(c1), out.off};
    same(b, {o_res, o_inl, out_bytes});
}

int main()
{
    sequence(Carver(), 256);  // the default: the id tables' blocks
    sequence(Carver(256), 256);
    sequence(Carver(16), 16);
    for (int n1 : {0, 1, 15, 16, 17, 64, 65})
        for (int H : {0, 1, 3}) {
            sim3_layout(n1, H);
            for (int ms : {4, 5})
                pnp_layout(n1, H, ms);
            sim3_opt_layout(n1);
        }
    std::printf("carve_test ok\n");
    return 0;
}

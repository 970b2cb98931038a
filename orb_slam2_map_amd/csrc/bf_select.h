// The candidate selection of k_bf_topk (matcher_bf.hip) for one lane and one row block in scalar form, host only: the
// blanking loop the kernel ran before and the order walk it runs now.  tests/bf_select_test.cpp compares the two.
//
// e[0..15] are the lane's tagged accumulator values, e[reg] = dot << 4 | 15 - reg with dot = 256 - 2 * hamming: larger =
// closer, then lower register = lower B row; the 16 values are pairwise distinct.  A value is a hit while dot >= bar
// (bar = acc_min at first, 256 - 2 * (distance of the 4th list entry) once the list is full).  One trip takes the lane's
// largest value not yet taken: the B row of register reg is j0 + (reg & 3) + 8 * (reg >> 2); a row past jlast is skipped
// but still counts as taken.  The key is distance << 12 | j, the list the four smallest keys in ascending order.
#pragma once
#include <climits>
#include <cstdint>

namespace orbgpu_bfsel {

constexpr uint32_t KEY_NONE = 0xFFFFFFFFu;
// 17th operand of the order walk's maximum: below every tagged value (|e| < 2^13) and every bar, and far enough from
// them that SENTINEL - m, taken as unsigned, is smaller than e - m of any value e < m
constexpr int SENTINEL = INT_MIN / 2;

struct Lane {
    uint32_t t[4] = {KEY_NONE, KEY_NONE, KEY_NONE, KEY_NONE};
    int lim;  // bar in units of dot
    explicit Lane(int acc_min) : lim(acc_min) {}
};

inline void top4_insert(uint32_t t[4], uint32_t k)
{
    if (k < t[3]) {
        t[3] = k;
        for (int q = 3; q > 0 && t[q] < t[q - 1]; q--) {
            const uint32_t x = t[q];
            t[q] = t[q - 1];
            t[q - 1] = x;
        }
    }
}

inline int max16(const int e[16])
{
    int m = e[0];
    for (int reg = 1; reg < 16; reg++)
        m = m > e[reg] ? m : e[reg];
    return m;
}

// B row and key of the tagged value m
inline int row_of(int m, int j0)
{
    const int reg = 15 - (m & 15);
    return j0 + (reg & 3) + 8 * (reg >> 2);
}
inline uint32_t key_of(int m, int j) { return (uint32_t)(((256 - (m >> 4)) << 11) + j); }  // (2 ham) << 11 = ham << 12

// Before: the value taken is blanked and the maximum of all 16 formed again.  Returns the lane's trips.
inline int select_blanking(const int acc[16], Lane &L, int j0, int jlast)
{
    int e[16], trips = 0;
    for (int reg = 0; reg < 16; reg++)
        e[reg] = acc[reg];
    for (;;) {
        const int m = max16(e);
        if (!((m >> 4) >= L.lim))
            return trips;
        trips++;
        const int j = row_of(m, j0);
        if (j <= jlast) {
            top4_insert(L.t, key_of(m, j));
            if (L.t[3] != KEY_NONE) {
                const int full = 256 - 2 * (int)(L.t[3] >> 12);
                L.lim = L.lim > full ? L.lim : full;
            }
        }
        for (int reg = 0; reg < 16; reg++)
            e[reg] = e[reg] == m ? INT_MIN : e[reg];
    }
}

// The largest value below m, or SENTINEL if there is none: e - m wraps to a large unsigned number for e < m, the
// closest e the largest, and stays small for the values taken already (e >= m).  *n_out = the maximum without the
// sentinel: a value below m exists iff (int)n < 0.
inline int next_below(const int acc[16], int m, uint32_t *n_out = nullptr)
{
    uint32_t n = 0;
    for (int reg = 0; reg < 16; reg++) {
        const uint32_t d = (uint32_t)acc[reg] - (uint32_t)m;
        n = n > d ? n : d;
    }
    if (n_out)
        *n_out = n;
    const uint32_t s = (uint32_t)SENTINEL - (uint32_t)m;
    n = n > s ? n : s;
    return (int)((uint32_t)m + n);
}

// Now: acc stays as it is; the trips take its values in descending order, and the bar is compared on the tagged value
// (the tag bits lie below the shift: m >= lim << 4 iff m >> 4 >= lim).  The bar of a full list is formed without asking
// whether the list is full: KEY_NONE >> 12 gives a bar far below any acc_min.  Returns the lane's trips.
inline int select_order_walk(const int acc[16], Lane &L, int j0, int jlast)
{
    int trips = 0;
    int lim16 = L.lim * 16;
    int m = max16(acc);
    while (m >= lim16) {
        trips++;
        const int j = row_of(m, j0);
        if (j <= jlast) {
            const uint32_t k = key_of(m, j);
            if (k < L.t[3]) {
                top4_insert(L.t, k);
                const int full16 = (256 - 2 * (int)(L.t[3] >> 12)) * 16;
                lim16 = lim16 > full16 ? lim16 : full16;
            }
        }
        m = next_below(acc, m);
    }
    L.lim = lim16 >> 4;
    return trips;
}

// One bar per A row -- NOT in the kernel: it was built, is exact (the test shows it) and was measured without a gain
// (DESIGN.md 9.35).  The lanes l and l ^ 32 of a wave list disjoint B rows of the same A row; once per tile both would
// take the higher of their two bars.  A bar above acc_min means the partner's list is full, so four B rows are at most
// that far and nothing farther can be among the merged four; equal distances still pass.
inline void share_bar(Lane &a, Lane &b) { a.lim = b.lim = a.lim > b.lim ? a.lim : b.lim; }

// 4 smallest of two sorted 4-lists
inline void top4_merge(uint32_t t[4], const uint32_t o[4])
{
    for (int q = 0; q < 4; q++)
        top4_insert(t, o[q]);
}

}  // namespace orbgpu_bfsel

// The FAST-9/16 corner score in scalar form, host only: the two-network definition and the single-network form with
// the polarity selector that k_fast_detect's fast_score_pk runs on packed pixel pairs (extractor.hip).
// tests/fast_polarity_test.cpp compares the two.
//
// v[0..15] are the ring values in ring order, c is the centre; all are bytes.  The score is
//   max(c - A, B - c, 0),  A = min over the 16 arcs of 9 of the arc maximum,  B = max over the arcs of the arc minimum.
#pragma once
#include <cstdint>

namespace orbgpu_fast {

struct TwoTerms {
    int dark;    // c - A (may be negative)
    int bright;  // B - c (may be negative)
};

// Both networks, straight from the definition.
inline TwoTerms fast_terms_two_networks(int c, const uint8_t v[16])
{
    uint8_t w[24], mx[16], mn[16];
    for (int k = 0; k < 24; k++)
        w[k] = v[k & 15];
    for (int a = 0; a < 16; a++)
        mx[a] = mn[a] = w[a];
    for (int k = 1; k < 9; k++)
        for (int a = 0; a < 16; a++) {
            mx[a] = mx[a] > w[a + k] ? mx[a] : w[a + k];
            mn[a] = mn[a] < w[a + k] ? mn[a] : w[a + k];
        }
    int A = 255, B = 0;
    for (int a = 0; a < 16; a++) {
        A = A < mx[a] ? A : mx[a];
        B = B > mn[a] ? B : mn[a];
    }
    return TwoTerms{c - A, B - c};
}

inline int fast_score_two_networks(int c, const uint8_t v[16])
{
    const TwoTerms t = fast_terms_two_networks(c, v);
    const int s = t.dark > t.bright ? t.dark : t.bright;
    return s > 0 ? s : 0;
}

// H = min over the 8 pairs (2i, 2i+9) of the pair maximum: a bright arc implies H > c, a dark arc H < c.
inline int fast_selector(const uint8_t v[16])
{
    int H = 255;
    for (int i = 0; i < 8; i++) {
        const int a = v[2 * i], b = v[(2 * i + 9) & 15];
        const int e = a > b ? a : b;
        H = H < e ? H : e;
    }
    return H;
}

// One network: the bytes are complemented where the selector says dark (H < c; at H == c the score is 0 either
// way), then the bright network alone -- in the paired-window order of fast_score_pk: M2, M4, E, T, reduction.
inline int fast_score_one_network(int c, const uint8_t v[16])
{
    const int mask = fast_selector(v) < c ? 0xFF : 0;
    int e[16], m2[8], m4[8];
    for (int k = 0; k < 16; k++)
        e[k] = v[k] ^ mask;
    auto mn = [](int a, int b) { return a < b ? a : b; };
    auto mx = [](int a, int b) { return a > b ? a : b; };
    for (int i = 0; i < 8; i++)
        m2[i] = mn(e[2 * i + 1], e[(2 * i + 2) & 15]);
    for (int i = 0; i < 8; i++)
        m4[i] = mn(m2[i], m2[(i + 1) & 7]);
    int B = 0;
    for (int i = 0; i < 8; i++)
        B = mx(B, mn(mn(m4[i], m4[(i + 2) & 7]), mx(e[2 * i], e[(2 * i + 9) & 15])));
    const int s = B - (c ^ mask);
    return s > 0 ? s : 0;
}

}  // namespace orbgpu_fast

// csrc/matcher_common.h on the host: rot_bin and three_maxima against literals worked out from ORBmatcher.cc:238-243 and
// :1601-1642, grid_cell against literals worked out from Frame.cc:382-392.  Built by test_matcher_common.py with AddressSanitizer, UBSan and float-cast-overflow, no recovery: a bin
// that was converted from a float outside int's range, or that indexed the histogram below outside [0, 30), ends the run.
//
// The reference's factor is 1.0f / HISTO_LENGTH = 1 / 30, so angles in [0, 360) use the bins 0..12 only:
// bin = roundf(rot / 30), where 30 folds onto 0 (reached from 885 degrees on) and anything else outside has no bin (-1).
#include <cmath>
#include <cstdio>
#include <limits>

#include "matcher_common.h"

static int g_fail = 0;

static void expect_bin(const char *what, float a, float b, int want)
{
    int histo[ORBGPU_HISTO_LENGTH] = {0};
    const int got = orbgpu::rot_bin(a, b);
    if (got >= 0)
        histo[got]++;  // under ASan: a bin >= 30 is a stack overflow here
    const bool ok = got == want && (got < 0 || histo[got] == 1);
    printf("%s rot_bin %s: %d, expected %d\n", ok ? "ok" : "FAIL", what, got, want);
    g_fail += !ok;
}

static void expect_maxima(const char *what, const int *histo, int w1, int w2, int w3)
{
    int i1 = -7, i2 = -7, i3 = -7;
    orbgpu::three_maxima(histo, ORBGPU_HISTO_LENGTH, i1, i2, i3);
    const bool ok = i1 == w1 && i2 == w2 && i3 == w3;
    printf("%s three_maxima %s: %d %d %d, expected %d %d %d\n", ok ? "ok" : "FAIL", what, i1, i2, i3, w1, w2, w3);
    g_fail += !ok;
}

static void expect_kept(const char *what, int bin, int i1, int i2, int i3, bool want)
{
    const bool got = orbgpu::rot_bin_kept(bin, i1, i2, i3);
    printf("%s rot_bin_kept %s: %d, expected %d\n", got == want ? "ok" : "FAIL", what, (int)got, (int)want);
    g_fail += got != want;
}

// grid_cell on 512 x 384 with bounds = image (cells of 8 x 8 pixels, inv = 0.125 exactly): column * 48 + row, or -1
static void expect_cell(const char *what, float x, float y, int want)
{
    int grid[ORBGPU_GRID_COLS * ORBGPU_GRID_ROWS] = {0};
    const int got = orbgpu::grid_cell(x, y, 0.f, 0.f, 0.125f, 0.125f);
    if (got >= 0)
        grid[got]++;  // under ASan: a cell outside the grid is a stack overflow here
    const bool ok = got == want && (got < 0 || grid[got] == 1);
    printf("%s grid_cell %s: %d, expected %d\n", ok ? "ok" : "FAIL", what, got, want);
    g_fail += !ok;
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // PosInGrid, Frame.cc:382-392: round half away from zero, kept iff 0 <= column < 64 and 0 <= row < 48
    expect_cell("(4, 100)", 4.f, 100.f, 1 * 48 + 13);                       // 0.5 -> 1, 12.5 -> 13
    expect_cell("(4-, 100)", std::nextafter(4.f, 0.f), 100.f, 13);          // 0.49999997 -> 0
    expect_cell("(508-, 380-)", std::nextafter(508.f, 0.f), std::nextafter(380.f, 0.f), 63 * 48 + 47);
    expect_cell("(508, 100)", 508.f, 100.f, -1);                            // 63.5 -> 64
    expect_cell("(100, 380)", 100.f, 380.f, -1);                            // 47.5 -> 48
    expect_cell("(-4, 100)", -4.f, 100.f, -1);                              // -0.5 -> -1
    expect_cell("(-4+, -4+)", std::nextafter(-4.f, 0.f), std::nextafter(-4.f, 0.f), 0);  // -0.49999997 -> -0.0
    expect_cell("(-0, -0)", -0.f, -0.f, 0);
    expect_cell("(NaN, 100)", nan, 100.f, -1);
    expect_cell("(100, NaN)", 100.f, nan, -1);
    expect_cell("(+inf, 100)", inf, 100.f, -1);
    expect_cell("(100, -inf)", 100.f, -inf, -1);
    expect_cell("(1e30, 100)", 1e30f, 100.f, -1);                           // finite, far outside int
    expect_cell("(100, -1e30)", 100.f, -1e30f, -1);
    expect_cell("(3.5e10, 100)", 3.5e10f, 100.f, -1);                       // 4.4e9: wraps to a small int modulo 2^32

    // rot / 30, rounded half away from zero (roundf)
    expect_bin("0", 0.f, 0.f, 0);
    expect_bin("14.99", 14.99f, 0.f, 0);       // 0.4997
    expect_bin("15", 15.f, 0.f, 1);            // 15 * (1.0f / 30) = 0.500000026 rounds to the float 0.5; roundf(0.5) = 1
    expect_bin("344.99", 344.99f, 0.f, 11);    // 11.4997
    expect_bin("345", 345.f, 0.f, 12);         // 11.5
    expect_bin("359.99", 359.99f, 0.f, 12);    // 11.9997: the last bin an angle difference in [0, 360) reaches
    expect_bin("-0.01", 0.f, 0.01f, 12);       // negative: + 360 = 359.99
    expect_bin("10 - 20", 10.f, 20.f, 12);     // 350 / 30 = 11.67
    expect_bin("884.9", 884.9f, 0.f, 29);      // 29.4967
    expect_bin("885", 885.f, 0.f, 0);          // 29.5 -> 30, which the reference folds onto 0 (:241-242)
    expect_bin("914.9", 914.9f, 0.f, 0);       // 30.4967 -> 30
    expect_bin("915", 915.f, 0.f, -1);         // 30.5 -> 31: no bin
    expect_bin("1000", 1000.f, 0.f, -1);       // 33
    expect_bin("-360.01", 0.f, 360.01f, 0);    // -0.01 after + 360: roundf(-0.0003) = -0.0, which is bin 0
    expect_bin("-374.9", 0.f, 374.9f, 0);      // -14.9 -> -0.4967 -> -0.0
    expect_bin("-375", 0.f, 375.f, -1);        // -15 -> -0.5 -> -1: no bin
    expect_bin("-400", 0.f, 400.f, -1);        // -40 -> -1.33 -> -1
    expect_bin("-1000", 0.f, 1000.f, -1);      // -640 -> -21
    expect_bin("3e38 - -3e38", 3e38f, -3e38f, -1);  // the difference overflows to +inf
    expect_bin("1e30", 1e30f, 0.f, -1);        // 3.3e28: finite, far outside int
    expect_bin("NaN a", nan, 0.f, -1);
    expect_bin("NaN b", 0.f, nan, -1);
    expect_bin("+inf", inf, 0.f, -1);
    expect_bin("-inf", -inf, 0.f, -1);         // -inf + 360 = -inf
    expect_bin("inf - inf", inf, inf, -1);     // NaN

    // ComputeThreeMaxima: strict `>` on every rank, so among equal counts the lower bins take the ranks in order and a
    // fourth equal count gets none
    {
        int h[ORBGPU_HISTO_LENGTH] = {0};
        expect_maxima("empty", h, -1, -1, -1);
        h[2] = h[7] = h[9] = h[11] = 5;
        expect_maxima("four equal", h, 2, 7, 9);
    }
    {
        int h[ORBGPU_HISTO_LENGTH] = {0};
        h[0] = 1, h[1] = 2, h[2] = 3;
        expect_maxima("rising", h, 2, 1, 0);  // 1 < 0.1f * 3 is false: all three stay
    }
    {
        int h[ORBGPU_HISTO_LENGTH] = {0};
        h[4] = 5, h[29] = 5, h[12] = 4;
        expect_maxima("tie for first, last bin", h, 4, 29, 12);
    }
    // the 0.1 rule compares in float, strictly: 0.1f * 100.f = 10.00000015 rounds to the float 10, and 10 < 10 is false
    {
        int h[ORBGPU_HISTO_LENGTH] = {0};
        h[3] = 100, h[5] = 10, h[8] = 9;
        expect_maxima("100 10 9", h, 3, 5, -1);
        h[5] = 9, h[8] = 9;
        expect_maxima("100 9 9", h, 3, -1, -1);  // the second falls, and takes the third with it (:1632-1636)
        h[5] = 10, h[8] = 10;
        expect_maxima("100 10 10", h, 3, 5, 8);
        h[3] = 101;  // 0.1f * 101.f = 10.1
        expect_maxima("101 10 10", h, 3, -1, -1);
    }
    {
        int h[ORBGPU_HISTO_LENGTH] = {0};
        h[6] = 1;
        expect_maxima("a single pair", h, 6, -1, -1);  // max2 = 0 < 0.1
    }
    // a pair without a bin is never kept, although three_maxima reports a missing maximum as -1 too
    expect_kept("-1 against (6, -1, -1)", -1, 6, -1, -1, false);
    expect_kept("-1 against (-1, -1, -1)", -1, -1, -1, -1, false);
    expect_kept("6 against (6, -1, -1)", 6, 6, -1, -1, true);
    expect_kept("5 against (3, 5, -1)", 5, 3, 5, -1, true);
    expect_kept("8 against (3, 5, 8)", 8, 3, 5, 8, true);
    expect_kept("0 against (3, 5, 8)", 0, 3, 5, 8, false);

    puts(g_fail ? "FAILED" : "PASSED");
    return g_fail ? 1 : 0;
}

// Helpers shared by the matcher kernels; the rotation check also runs on the host (orbgpu_search_for_initialization),
// so this header compiles without HIP as well (tests/proj_boundary_test.cpp).
#pragma once
#ifdef __HIPCC__
#include "common.h"
#define ORBGPU_HD __host__ __device__
#else
#include <cmath>
#include "orbgpu.h"
#define ORBGPU_HD
#endif

namespace orbgpu {

// ORBmatcher::ComputeThreeMaxima, ORBmatcher.cc:1601-1642
ORBGPU_HD inline void three_maxima(const int *histo, int L, int &ind1, int &ind2, int &ind3)
{
    int max1 = 0, max2 = 0, max3 = 0;
    ind1 = ind2 = ind3 = -1;
    for (int i = 0; i < L; i++) {
        const int s = histo[i];
        if (s > max1) {
            max3 = max2;
            max2 = max1;
            max1 = s;
            ind3 = ind2;
            ind2 = ind1;
            ind1 = i;
        } else if (s > max2) {
            max3 = max2;
            max2 = s;
            ind3 = ind2;
            ind2 = i;
        } else if (s > max3) {
            max3 = s;
            ind3 = i;
        }
    }
    if ((float)max2 < 0.1f * (float)max1) {
        ind2 = -1;
        ind3 = -1;
    } else if ((float)max3 < 0.1f * (float)max1) {
        ind3 = -1;
    }
}

// rotation bin, ORBmatcher.cc:238-243.  The reference asserts bin in [0, HISTO_LENGTH) behind the conversion; angles are
// the caller's, so here the float is tested before it is converted: a pair whose roundf(rot * factor) is not in
// [0, HISTO_LENGTH] (a difference of 915 or more, of -375 or less, NaN, +-inf) has no bin, -1.  Such a pair casts no vote
// and, when the orientation is checked, is removed like a pair outside the three maxima (rot_bin_kept).
ORBGPU_HD inline int rot_bin(float angle_a, float angle_b)
{
    const float factor = 1.0f / ORBGPU_HISTO_LENGTH;
    float rot = angle_a - angle_b;
    if (rot < 0.0f)
        rot += 360.0f;
    const float r = roundf(rot * factor);
    if (!(r >= 0.0f && r <= (float)ORBGPU_HISTO_LENGTH))
        return -1;
    const int bin = (int)r;
    return bin == ORBGPU_HISTO_LENGTH ? 0 : bin;
}

// whether a pair of bin `bin` survives the rotation check; ind1..3 of three_maxima, where -1 stands for "no such maximum"
// and must not keep a pair that has no bin
ORBGPU_HD inline bool rot_bin_kept(int bin, int ind1, int ind2, int ind3)
{
    return bin >= 0 && (bin == ind1 || bin == ind2 || bin == ind3);
}

// Frame::PosInGrid (Frame.cc:382-392) as the CSR cell px * ROWS + py, or -1 where the reference refuses the point.  The
// reference converts round(...) to int before it tests the range; a NaN or a value beyond int has no int (on x86 the
// conversion gives INT_MIN, which the test refuses; on the device it gives 0 for NaN, a cell that would be kept).
// Positions are the caller's, so here the rounded float is tested before it is converted: NaN, +-inf and anything
// beyond the grid have no cell.  For every value the reference defines, the result is the reference's.
ORBGPU_HD inline int grid_cell(float x, float y, float min_x, float min_y, float inv_w, float inv_h)
{
    const float px = roundf((x - min_x) * inv_w), py = roundf((y - min_y) * inv_h);
    if (!(px >= 0.0f && px < (float)ORBGPU_GRID_COLS && py >= 0.0f && py < (float)ORBGPU_GRID_ROWS))
        return -1;
    return (int)px * ORBGPU_GRID_ROWS + (int)py;
}

} // namespace orbgpu

// ORBmatcher::SearchForTriangulation (ORBmatcher.cc:657-823) as device functions.  tri_match_wave is the body of k_tri_match
// (matcher_proj.hip) and of k_np_match (new_points.hip, the neighbour chain of LocalMapping::CreateNewMapPoints), which must
// agree byte for byte.  tri_finish_block is the body of k_tri_finish and of k_np_finish.
#pragma once

#include "common.h"
#include "matcher_common.h"

namespace orbgpu {

struct TriParams {
    float F12[9];
    float ex, ey;  // epipole in the second image (:664-670)
    int only_stereo;
    float sigma2[ORBGPU_MAX_LEVELS], scale[ORBGPU_MAX_LEVELS];  // of key frame 2
};

// One wave per key point of key frame 1 without a map point: its candidates are the key points of key frame 2 under
// the same vocabulary node (node2 == node1 >= 0) without a map point; Hamming <= TH_LOW, the epipole distance test
// for monocular pairs, the epipolar-line test (:140-157), least distance, the LAST among equals in the node's list
// (`dist > bestDist` is the skip, :739), i.e. the largest index.  The reference never sets vbMatched2, so rows do
// not interact.  Rotation histogram: tri_finish_block.
// GUARD_OCTAVE: a candidate whose octave lies outside [0, ORBGPU_MAX_LEVELS) is skipped (callers that cannot check the
// octaves on the host; levels in [nlevels, ORBGPU_MAX_LEVELS) have sigma2 = 0 and fail the epipolar test by themselves).
template <bool GUARD_OCTAVE>
__device__ __forceinline__ void tri_match_wave(int n1, const float *__restrict__ x1, const float *__restrict__ y1,
                                               const float *__restrict__ ur1, const uint8_t *__restrict__ has_mp1,
                                               const int *__restrict__ node1, const uint8_t *__restrict__ desc1, int n2,
                                               const float *__restrict__ x2, const float *__restrict__ y2,
                                               const int *__restrict__ oct2, const float *__restrict__ ur2,
                                               const uint8_t *__restrict__ has_mp2, const int *__restrict__ node2,
                                               const uint8_t *__restrict__ desc2, const TriParams &P,
                                               int *__restrict__ match12)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n1)
        return;
    int best = -1;
    const int nd = node1[i];
    const bool stereo1 = ur1[i] >= 0;
    if (nd >= 0 && !has_mp1[i] && !(P.only_stereo && !stereo1)) {
        const uint64_t *pa = reinterpret_cast<const uint64_t *>(desc1) + (size_t)i * 4;
        const uint64_t a[4] = {pa[0], pa[1], pa[2], pa[3]};
        const float kx = x1[i], ky = y1[i];
        // epipolar line in the second image l = x1' F12 (:143-145)
        const float la = kx * P.F12[0] + ky * P.F12[3] + P.F12[6];
        const float lb = kx * P.F12[1] + ky * P.F12[4] + P.F12[7];
        const float lc = kx * P.F12[2] + ky * P.F12[5] + P.F12[8];
        const float den = la * la + lb * lb;
        uint32_t key = 0xFFFFFFFFu;  // distance << 16 | (65535 - idx2): least distance, then largest index
        for (int j = lane; j < n2; j += 64) {
            if (node2[j] != nd || has_mp2[j])
                continue;
            const bool stereo2 = ur2[j] >= 0;
            if (P.only_stereo && !stereo2)
                continue;
            const uint64_t *pb = reinterpret_cast<const uint64_t *>(desc2) + (size_t)j * 4;
            const uint64_t b[4] = {pb[0], pb[1], pb[2], pb[3]};
            const int dist = hamming256(a, b);
            if (dist > ORBGPU_TH_LOW)
                continue;
            const float px = x2[j], py = y2[j];
            const int o = oct2[j];
            if (GUARD_OCTAVE && (unsigned)o >= (unsigned)ORBGPU_MAX_LEVELS)
                continue;
            if (!stereo1 && !stereo2) {
                const float dex = P.ex - px, dey = P.ey - py;
                if (dex * dex + dey * dey < 100 * P.scale[o])
                    continue;
            }
            const float num = la * px + lb * py + lc;
            if (den == 0)
                continue;
            const float dsqr = num * num / den;
            if (!((double)dsqr < 3.84 * (double)P.sigma2[o]))
                continue;
            key = min(key, ((uint32_t)dist << 16) | (uint32_t)(65535 - j));
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            key = min(key, (uint32_t)__shfl_xor((int)key, off, 64));
        if (key != 0xFFFFFFFFu)
            best = 65535 - (int)(key & 0xFFFFu);
    }
    if (lane == 0)
        match12[i] = best;
}

// rotation consistency of the accepted pairs (:772-795) and the count; one workgroup of 1024
__device__ __forceinline__ void tri_finish_block(int n1, const float *__restrict__ angle1, const float *__restrict__ angle2,
                                                 int check_orientation, int *__restrict__ match12,
                                                 int *__restrict__ nmatches)
{
    __shared__ int histo[ORBGPU_HISTO_LENGTH];
    __shared__ int s_keep[3], s_count;
    const int tid = threadIdx.x;
    if (tid < ORBGPU_HISTO_LENGTH)
        histo[tid] = 0;
    if (tid == 0)
        s_count = 0;
    __syncthreads();
    int cnt = 0;
    for (int i = tid; i < n1; i += 1024) {
        const int j = match12[i];
        if (j < 0)
            continue;
        cnt++;
        if (check_orientation) {
            const int b = rot_bin(angle1[i], angle2[j]);
            if (b >= 0)  // a pair without a bin casts no vote
                atomicAdd(&histo[b], 1);
        }
    }
    __syncthreads();
    if (check_orientation) {
        if (tid == 0) {
            int i1, i2, i3;
            three_maxima(histo, ORBGPU_HISTO_LENGTH, i1, i2, i3);
            s_keep[0] = i1, s_keep[1] = i2, s_keep[2] = i3;
        }
        __syncthreads();
        for (int i = tid; i < n1; i += 1024) {
            const int j = match12[i];
            if (j < 0)
                continue;
            const int b = rot_bin(angle1[i], angle2[j]);
            if (!rot_bin_kept(b, s_keep[0], s_keep[1], s_keep[2])) {
                match12[i] = -1;
                cnt--;
            }
        }
    }
    cnt = wave_reduce_add(cnt);
    if ((tid & 63) == 0)
        atomicAdd(&s_count, cnt);
    __syncthreads();
    if (tid == 0)
        *nmatches = s_count;
}

} // namespace orbgpu

// Frame::ComputeStereoMatches (reference src/Frame.cc:466-638) on the device, for batches of rectified stereo pairs whose
// key points, descriptors and (unblurred) pyramids come from the extractor handles' last calls.
//
//   k_stereo_rows   one workgroup per pair: the right key points as CSR by row floor(y) (counting sort in LDS); a left
//                   key point's candidates are then the contiguous run of rows vL - R .. vL + R, filtered with the
//                   reference's own row-table predicate (Frame.cc:481-489)
//   k_stereo_match  a 16-lane group per left key point, grid (cap / 16, pairs): descriptor search (Frame.cc:509-546),
//                   eleven 11x11 SAD windows, one per lane (:549-595), parabola, disparity and depth (:597-626)
//   k_stereo_cut    one workgroup per pair: the median SAD by a radix select over 16-bit values, the outlier cut
//                   (:629-637) and the per-pair count of matches kept
//
// Conventions where the reference is undefined: minZ = mb = mbf / fx; an empty match list
// cuts nothing; a key point whose row, octave or SAD windows leave the level plane gets no match (and is never read
// outside the plane); a right key point with an octave outside [0, nlevels) is never a candidate.
#include "common.h"
#include "pyramid_view.h"
#include "staging.h"

#include <algorithm>
#include <climits>

namespace orbgpu {

constexpr int ST_GROUP = 16;                      // lanes per left key point
constexpr int ST_KEYS = 256 / ST_GROUP;           // left key points per workgroup
constexpr int ST_W = 5, ST_L = 5;                 // w, L (Frame.cc:557, 566)
constexpr int ST_TH_HIGH = 100;                   // ORBmatcher::TH_HIGH (ORBmatcher.cc:37)
constexpr float ST_MIN_D = -3.0f;                 // minD (Frame.cc:494): this fork's value (upstream has 0)

// Level planes of one handle for the kernels (host-filled from PyramidView; passed by value)
struct StPlanes {
    const uint8_t *pyr;
    size_t frame_pyr;
    const uint8_t *l0;  // direct mode: level 0 from the last call's image
    size_t l0_frame_stride, l0_pitch;
    int direct, frame0, border;
    int pitch[ORBGPU_MAX_LEVELS], plane_off[ORBGPU_MAX_LEVELS];
};

struct StLevels {
    int nlevels, rows0;  // rows0 = mvImagePyramid[0].rows (nRows, Frame.cc:471)
    int w[ORBGPU_MAX_LEVELS], h[ORBGPU_MAX_LEVELS];
    float scale[ORBGPU_MAX_LEVELS], inv_scale[ORBGPU_MAX_LEVELS];
    int row_reach;  // R = ceil(2 * s[nlevels - 1]) + 1: a right key point's rows lie within floor(y) +- R
};

// pixel (x, y) of level l of pair p's frame (x, y inside the level)
__device__ __forceinline__ const uint8_t *st_row(const StPlanes &P, int p, int l, int y)
{
    const int f = P.frame0 + p;
    if (P.direct && l == 0)
        return P.l0 + (size_t)f * P.l0_frame_stride + (size_t)y * P.l0_pitch;
    return P.pyr + (size_t)f * P.frame_pyr + P.plane_off[l] + (size_t)(y + P.border) * P.pitch[l] + P.border;
}

// The right key point's rows, Frame.cc:481-489.  false: the key point is never listed (octave outside the table, or a
// y no row of any image can reach -- NaN included).
__device__ __forceinline__ bool st_right_rows(const orbgpu_keypoint &k, const StLevels &G, int &minr, int &maxr)
{
    if (k.octave < 0 || k.octave >= G.nlevels || !(k.y > -1.0e6f && k.y < 1.0e6f))
        return false;
    const float r = 2.0f * G.scale[k.octave];
    maxr = (int)ceilf(k.y + r);
    minr = (int)floorf(k.y - r);
    return true;
}

// ---- CSR of the right key points by row ------------------------------------------------------------------------------
// Bucket = floor(y) clamped to [0, rows0): the clamp keeps every key point whose listed rows meet the image within
// R rows of its bucket, and the exact predicate is applied by the reader.
// The right key points are written in CSR order as 16-byte records {x, minr, maxr, iR << 4 | octave} with their
// descriptors next to them: a left key point's scan reads consecutive records (no index gather).
__global__ __launch_bounds__(1024) void k_stereo_rows(const orbgpu_keypoint *__restrict__ kps_r,
                                                      const int *__restrict__ n_r, const uint8_t *__restrict__ desc_r,
                                                      int cap, StLevels G, int *__restrict__ row_start,
                                                      int4 *__restrict__ recs, uint4 *__restrict__ sdesc)
{
    extern __shared__ int st_lds[];
    const int rows = G.rows0;
    int *cnt = st_lds;              // [rows + 1]
    int *pos = st_lds + rows + 1;   // [rows]
    __shared__ int s_w[16];
    const int p = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int n = min(max(n_r[p], 0), cap);
    const orbgpu_keypoint *k = kps_r + (size_t)p * cap;
    for (int r = tid; r <= rows; r += nt)
        cnt[r] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += nt) {
        int minr, maxr;
        if (st_right_rows(k[i], G, minr, maxr))
            atomicAdd(&cnt[min(max((int)floorf(k[i].y), 0), rows - 1)], 1);
    }
    __syncthreads();
    {  // exclusive scan of cnt[0..rows)
        const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
        const int per = (rows + nt - 1) / nt;
        const int beg = min(tid * per, rows), end = min(beg + per, rows);
        int sum = 0;
        for (int r = beg; r < end; r++)
            sum += cnt[r];
        int inc = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(inc, off, 64);
            if (lane >= off)
                inc += t;
        }
        if (lane == 63)
            s_w[wave] = inc;
        __syncthreads();
        int woff = 0, total = 0;
        for (int w = 0; w < nw; w++) {
            if (w < wave)
                woff += s_w[w];
            total += s_w[w];
        }
        int run = woff + inc - sum;
        for (int r = beg; r < end; r++) {
            const int t = cnt[r];
            cnt[r] = run;
            pos[r] = run;
            run += t;
        }
        if (tid == 0)
            cnt[rows] = total;
    }
    __syncthreads();
    int *rs = row_start + (size_t)p * (rows + 1);
    for (int r = tid; r <= rows; r += nt)
        rs[r] = cnt[r];
    int4 *rec = recs + (size_t)p * cap;
    uint4 *sd = sdesc + (size_t)p * cap * 2;
    const uint4 *dr = reinterpret_cast<const uint4 *>(desc_r + (size_t)p * cap * 32);
    for (int i = tid; i < n; i += nt) {  // order inside a row is free: the search is min (distance, iR)
        const orbgpu_keypoint kp = k[i];
        int minr, maxr;
        if (st_right_rows(kp, G, minr, maxr)) {
            const int slot = atomicAdd(&pos[min(max((int)floorf(kp.y), 0), rows - 1)], 1);
            rec[slot] = make_int4(__float_as_int(kp.x), minr, maxr, (i << 4) | kp.octave);
            sd[2 * slot] = dr[2 * i];
            sd[2 * slot + 1] = dr[2 * i + 1];
        }
    }
}

// ---- matching ----------------------------------------------------------------------------------------------------------
// Reads: left / right key points and descriptors [pairs][cap], the CSR above, both handles' level planes.
// Writes u_right / depth [pairs][cap] (-1 where there is no match) and the accepted SAD [pairs][cap] (-1: none).
__global__ __launch_bounds__(256) void k_stereo_match(const orbgpu_keypoint *__restrict__ kps_l,
                                                      const int *__restrict__ n_l, const uint8_t *__restrict__ desc_l,
                                                      const orbgpu_keypoint *__restrict__ kps_r,
                                                      const uint8_t *__restrict__ desc_r, int cap,
                                                      const int *__restrict__ row_start,
                                                      const int4 *__restrict__ recs,
                                                      const uint4 *__restrict__ sdesc, StLevels G, StPlanes PL,
                                                      StPlanes PR, float mbf, float maxD,
                                                      float *__restrict__ u_right, float *__restrict__ depth,
                                                      int *__restrict__ sad_out)
{
    const int p = blockIdx.y;
    const int lane = threadIdx.x & (ST_GROUP - 1);
    const int iL = blockIdx.x * ST_KEYS + (threadIdx.x >> 4);
    // (iL >= cap: a group past the end of the last block, go = false below; every branch is uniform across the 16 lanes of
    // a group)
    const size_t o = (size_t)p * cap + min(iL, cap - 1);
    const int n = min(max(n_l[p], 0), cap);
    float ur_out = -1.0f, dz_out = -1.0f;
    int sad_keep = -1;
    const int rows = G.rows0;
    bool go = iL < n;
    orbgpu_keypoint kpL = {};
    int levelL = 0, row = 0;
    if (go) {
        kpL = kps_l[o];
        levelL = kpL.octave;
        // vRowIndices[vL] with vL = (size_t)kpL.pt.y (truncation) -- a row outside the table gets no match
        go = levelL >= 0 && levelL < G.nlevels && kpL.y > -1.0f && kpL.y < (float)rows;
        row = go ? (int)kpL.y : 0;
    }
    const float uL = go ? kpL.x : 0.0f;
    const float minU = uL - maxD;  // Frame.cc:515-516
    const float maxU = uL - ST_MIN_D;
    if (go && maxU < 0)  // :518
        go = false;
    unsigned long long best = ~0ull;
    if (go) {
        const int *rs = row_start + (size_t)p * (rows + 1);
        const int b = rs[max(row - G.row_reach, 0)], e = rs[min(row + G.row_reach, rows - 1) + 1];
        const int4 *rec = recs + (size_t)p * cap;
        const uint4 *sd = sdesc + (size_t)p * cap * 2;
        const uint64_t *dl = reinterpret_cast<const uint64_t *>(desc_l + o * 32);
        const uint64_t a[4] = {dl[0], dl[1], dl[2], dl[3]};
        for (int c = b + lane; c < e; c += ST_GROUP) {
            const int4 r = rec[c];
            if (row < r.y || row > r.z)  // listed in row vL (Frame.cc:481-489)
                continue;
            const int octR = r.w & 15, iR = r.w >> 4;
            if (octR < levelL - 1 || octR > levelL + 1)  // :534-535
                continue;
            const float uR = __int_as_float(r.x);
            if (uR >= minU && uR <= maxU) {  // :539
                const uint4 d0 = sd[2 * c], d1 = sd[2 * c + 1];
                const uint64_t bb[4] = {(uint64_t)d0.x | (uint64_t)d0.y << 32, (uint64_t)d0.z | (uint64_t)d0.w << 32,
                                        (uint64_t)d1.x | (uint64_t)d1.y << 32, (uint64_t)d1.z | (uint64_t)d1.w << 32};
                const int dist = hamming256(a, bb);
                const unsigned long long key = ((unsigned long long)dist << 32) | (unsigned)iR;
                best = key < best ? key : best;
            }
        }
    }
#pragma unroll
    for (int off = ST_GROUP / 2; off > 0; off >>= 1) {
        const unsigned long long t = __shfl_xor(best, off, ST_GROUP);
        best = t < best ? t : best;
    }
    // bestDist starts at TH_HIGH and only a strictly smaller distance replaces it (:524, 544-548, 551)
    go = go && best != ~0ull && (int)(best >> 32) < ST_TH_HIGH;
    float suL = 0.f, svL = 0.f, suR0 = 0.f;
    if (go) {
        const float uR0 = kps_r[(size_t)p * cap + (unsigned)best].x;  // :554
        const float sf = G.inv_scale[levelL];
        suL = roundf(kpL.x * sf);  // std::round: half away from zero
        svL = roundf(kpL.y * sf);
        suR0 = roundf(uR0 * sf);
        const float iniu = suR0 + (float)ST_L - (float)ST_W;  // :572-575, the reference's own bound
        const float endu = suR0 + (float)ST_L + (float)ST_W + 1.0f;
        const int cols = G.w[levelL], lrows = G.h[levelL];
        if (iniu < 0 || endu >= (float)cols)
            go = false;
        // S3: every window inside the plane (the reference asserts in cv::Mat instead)
        else if (!(suL - ST_W >= 0.0f && suL + ST_W < (float)cols && svL - ST_W >= 0.0f && svL + ST_W < (float)lrows &&
                   suR0 - ST_L - ST_W >= 0.0f))
            go = false;
    }
    if (go) {
        const int xl = (int)suL, yl = (int)svL, xr = (int)suR0;  // (inside the planes: checked above)
        // lane j < 11 computes the window of incR = j - L: |(a - ac) - (b - bc)| = |(a + bc) - (b + ac)|, exact
        int sad = INT_MAX;
        if (lane <= 2 * ST_L) {
            const int inc = lane - ST_L;
            const int ac = st_row(PL, p, levelL, yl)[xl];
            const int bc = st_row(PR, p, levelL, yl)[xr + inc];
            int s = 0;
            for (int dy = -ST_W; dy <= ST_W; dy++) {
                const uint8_t *ra = st_row(PL, p, levelL, yl + dy) + xl - ST_W;
                const uint8_t *rb = st_row(PR, p, levelL, yl + dy) + xr + inc - ST_W;
#pragma unroll
                for (int dx = 0; dx < 2 * ST_W + 1; dx++)
                    s += abs(((int)ra[dx] + bc) - ((int)rb[dx] + ac));
            }
            sad = s;
        }
        int d[2 * ST_L + 1];
#pragma unroll
        for (int j = 0; j <= 2 * ST_L; j++)
            d[j] = __shfl(sad, j, ST_GROUP);
        // first strict minimum over incR = -L .. L (:585-589)
        int bestSad = d[0], bestinc = 0;
#pragma unroll
        for (int j = 1; j <= 2 * ST_L; j++)
            if (d[j] < bestSad) {
                bestSad = d[j];
                bestinc = j;
            }
        bestinc -= ST_L;
        if (bestinc == -ST_L || bestinc == ST_L)  // :595-596
            go = false;
        if (go) {
            const float dist1 = (float)d[ST_L + bestinc - 1];  // :599-601
            const float dist2 = (float)d[ST_L + bestinc];
            const float dist3 = (float)d[ST_L + bestinc + 1];
            const float deltaR = (dist1 - dist3) / (2.0f * (dist1 + dist3 - 2.0f * dist2));  // :603
            if (deltaR < -1 || deltaR > 1)  // :605
                go = false;
            if (go) {
                float bestuR = G.scale[levelL] * ((float)suR0 + (float)bestinc + deltaR);  // :609
                float disparity = (uL - bestuR);                                             // :611
                if (disparity >= 0 && disparity < maxD) {                                    // :613
                    if (disparity <= 0) {
                        disparity = 0.01f;                        // (float)0.01
                        bestuR = (float)((double)uL - 0.01);      // uL - 0.01 in double, rounded to float
                    }
                    dz_out = mbf / disparity;
                    ur_out = bestuR;
                    sad_keep = bestSad;  // the inner bestDist (:578), pushed with iL (:622)
                }
            }
        }
    }
    if (lane == 0 && iL < cap) {  // (iL >= cap: a group past the end of the last block)
        u_right[o] = ur_out;
        depth[o] = dz_out;
        sad_out[o] = sad_keep;
    }
}

// ---- outlier cut (Frame.cc:629-637) --------------------------------------------------------------------------------------
// median = the (count / 2)-th smallest accepted SAD (sort of (SAD, iL) pairs: only the first member is read); every
// match with SAD >= 1.5f * 1.4f * median is dropped.  SADs are < 2^16 (121 * 510): a two-pass radix select on bytes.
__global__ __launch_bounds__(256) void k_stereo_cut(const int *__restrict__ n_l, int cap, const int *__restrict__ sad,
                                                    float *__restrict__ u_right, float *__restrict__ depth,
                                                    int *__restrict__ n_stereo)
{
    __shared__ int hist[256];
    __shared__ int s_count, s_sel, s_rank, s_kept;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(n_l[p], 0), cap);
    const int *sp = sad + (size_t)p * cap;
    hist[tid] = 0;
    if (tid == 0) {
        s_count = 0;
        s_kept = 0;
    }
    __syncthreads();
    int cnt = 0;
    for (int i = tid; i < n; i += 256) {
        const int s = sp[i];
        if (s >= 0) {
            cnt++;
            atomicAdd(&hist[s >> 8], 1);
        }
    }
    atomicAdd(&s_count, cnt);
    __syncthreads();
    const int count = s_count;
    if (count == 0) {  // S2: the reference reads vDistIdx[0] of an empty vector; nothing to cut
        if (tid == 0 && n_stereo)
            n_stereo[p] = 0;
        return;
    }
    if (tid == 0) {  // the bin holding rank count / 2
        int rank = count / 2, b = 0;
        while (rank >= hist[b]) {
            rank -= hist[b];
            b++;
        }
        s_sel = b;
        s_rank = rank;
    }
    __syncthreads();
    const int hi = s_sel;
    hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int s = sp[i];
        if (s >= 0 && (s >> 8) == hi)
            atomicAdd(&hist[s & 255], 1);
    }
    __syncthreads();
    if (tid == 0) {
        int rank = s_rank, b = 0;
        while (rank >= hist[b]) {
            rank -= hist[b];
            b++;
        }
        s_sel = (hi << 8) | b;
    }
    __syncthreads();
    const float median = (float)s_sel;
    const float c = 1.5f * 1.4f;  // 1.5f*1.4f*median evaluates left to right
    const float thDist = c * median;
    int kept = 0;
    for (int i = tid; i < n; i += 256) {
        const int s = sp[i];
        if (s < 0)
            continue;
        if ((float)s >= thDist) {
            u_right[(size_t)p * cap + i] = -1.0f;
            depth[(size_t)p * cap + i] = -1.0f;
        } else
            kept++;
    }
    atomicAdd(&s_kept, kept);
    __syncthreads();
    if (tid == 0 && n_stereo)
        n_stereo[p] = s_kept;
}

static void planes_of(const PyramidView &v, int frame0, StPlanes &P)
{
    P.pyr = v.pyr;
    P.frame_pyr = v.frame_pyr;
    P.l0 = v.l0;
    P.l0_frame_stride = v.l0_frame_stride;
    P.l0_pitch = v.l0_pitch;
    P.direct = v.direct;
    P.frame0 = frame0;
    P.border = v.border;
    for (int l = 0; l < ORBGPU_MAX_LEVELS; l++) {
        P.pitch[l] = v.pitch[l];
        P.plane_off[l] = v.plane_off[l];
    }
}

// Host-entry staging: per (thread, device), on the one type of the stateless entry points (staging.h).
enum { KPS_L, KPS_R, DESC_L, DESC_R, COUNTS, UR, DZ, N_BUF };
struct StereoHostWs : Staging<N_BUF> {};

// Everything the entry points check before they touch the device.
static int check_pair(const orbgpu_extractor *left, int lf0, const orbgpu_extractor *right, int rf0, int batch,
                      PyramidView &vl, PyramidView &vr)
{
    int rc = extractor_pyramid_view(left, &vl);
    if (rc == ORBGPU_OK)
        rc = extractor_pyramid_view(right, &vr);
    if (rc != ORBGPU_OK)
        return rc;
    ORBGPU_REQUIRE(vl.nlevels == vr.nlevels && vl.scale_factor == vr.scale_factor,
                   "the handles differ in levels or scale factor");
    ORBGPU_REQUIRE(vl.device_id == vr.device_id, "the handles are on different devices");
    ORBGPU_REQUIRE(vl.last_batch > 0 && vr.last_batch > 0, "a handle has no last call");
    ORBGPU_REQUIRE(vl.w[0] == vr.w[0] && vl.h[0] == vr.h[0], "the image sizes differ (%dx%d against %dx%d)", vl.w[0],
                   vl.h[0], vr.w[0], vr.h[0]);
    ORBGPU_REQUIRE(lf0 >= 0 && (int64_t)lf0 + batch <= vl.last_batch && rf0 >= 0 && (int64_t)rf0 + batch <= vr.last_batch,
                   "frame range outside the last call");
    return ORBGPU_OK;
}

} // namespace orbgpu

using namespace orbgpu;

extern "C" int orbgpu_stereo_matches_batch_device(const orbgpu_extractor *left, int32_t left_frame0,
                                                  const orbgpu_extractor *right, int32_t right_frame0, int32_t batch,
                                                  int32_t cap, const orbgpu_keypoint *d_kps_l, const int32_t *d_n_l,
                                                  const uint8_t *d_desc_l, const orbgpu_keypoint *d_kps_r,
                                                  const int32_t *d_n_r, const uint8_t *d_desc_r, float mbf, float fx,
                                                  float *d_u_right, float *d_depth, int32_t *d_n_stereo,
                                                  void *hip_stream)
{
    ORBGPU_REQUIRE(left && right, "null extractor handle");
    ORBGPU_REQUIRE(batch >= 0 && cap >= 0 && cap < (1 << 27), "bad batch/cap");  // (iR << 4 | octave in 32 bits)
    ORBGPU_REQUIRE(d_kps_l && d_n_l && d_desc_l && d_kps_r && d_n_r && d_desc_r, "null input");
    ORBGPU_REQUIRE(d_u_right && d_depth, "null output");
    PyramidView vl, vr;
    int rc = check_pair(left, left_frame0, right, right_frame0, batch, vl, vr);
    if (rc != ORBGPU_OK)
        return rc;
    if (batch == 0)
        return ORBGPU_OK;
    rc = select_device(vl.device_id);
    if (rc != ORBGPU_OK)
        return rc;
    StLevels G = {};
    G.nlevels = vl.nlevels;
    G.rows0 = vl.h[0];
    for (int l = 0; l < vl.nlevels; l++) {
        G.w[l] = vl.w[l];
        G.h[l] = vl.h[l];
        G.scale[l] = vl.scale[l];
        G.inv_scale[l] = vl.inv_scale[l];
    }
    G.row_reach = (int)ceilf(2.0f * vl.scale[vl.nlevels - 1]) + 1;
    StPlanes PL, PR;
    planes_of(vl, left_frame0, PL);
    planes_of(vr, right_frame0, PR);
    // S1: mb = mbf / fx (Frame.cc:114, assigned only after the call at :90), minZ = mb, maxD = mbf / minZ (:493-495)
    const float mb = mbf / fx;
    const float minZ = mb;
    const float maxD = mbf / minZ;
    // scratch on the left handle: records [batch][cap] (16 B) | descriptors in CSR order [batch][cap][32] |
    // sad [batch][cap] | row_start [batch][rows0 + 1]
    const size_t n_it = (size_t)batch * cap, n_rs = (size_t)batch * (G.rows0 + 1);
    DevBuf &S = *vl.scratch;
    if ((rc = S.reserve(n_it * (16 + 32 + 4) + sizeof(int) * n_rs)) != ORBGPU_OK)
        return rc;
    int4 *recs = S.as<int4>();
    uint4 *sdesc = reinterpret_cast<uint4 *>(recs + n_it);
    int *sad = reinterpret_cast<int *>(sdesc + 2 * n_it), *row_start = sad + n_it;
    const hipStream_t st = (hipStream_t)hip_stream;
    if (cap == 0) {  // no key point slots: nothing to read or write but the counts
        if (d_n_stereo)
            ORBGPU_HIP_TRY(hipMemsetAsync(d_n_stereo, 0, sizeof(int32_t) * batch, st));
        return ORBGPU_OK;
    }
    hipLaunchKernelGGL(k_stereo_rows, dim3(batch), dim3(1024), sizeof(int) * (2 * G.rows0 + 1), st, d_kps_r, d_n_r,
                       d_desc_r, cap, G, row_start, recs, sdesc);
    hipLaunchKernelGGL(k_stereo_match, dim3((cap + ST_KEYS - 1) / ST_KEYS, batch), dim3(256), 0, st, d_kps_l, d_n_l,
                       d_desc_l, d_kps_r, d_desc_r, cap, row_start, recs, sdesc, G, PL, PR, mbf, maxD, d_u_right,
                       d_depth, sad);
    hipLaunchKernelGGL(k_stereo_cut, dim3(batch), dim3(256), 0, st, d_n_l, cap, sad, d_u_right, d_depth, d_n_stereo);
    ORBGPU_HIP_TRY(hipGetLastError());
    return ORBGPU_OK;
}

extern "C" int orbgpu_compute_stereo_matches(const orbgpu_extractor *left, const orbgpu_extractor *right, int32_t n_l,
                                             const orbgpu_keypoint *kps_l, const uint8_t *desc_l, int32_t n_r,
                                             const orbgpu_keypoint *kps_r, const uint8_t *desc_r, float mbf, float fx,
                                             float *u_right, float *depth)
{
    ORBGPU_REQUIRE(left && right, "null extractor handle");
    ORBGPU_REQUIRE(n_l >= 0 && n_r >= 0, "negative key point count");
    ORBGPU_REQUIRE((n_l == 0 || (kps_l && desc_l && u_right && depth)) && (n_r == 0 || (kps_r && desc_r)),
                   "null argument");
    PyramidView vl, vr;
    int rc = check_pair(left, 0, right, 0, 1, vl, vr);
    if (rc != ORBGPU_OK || n_l == 0)
        return rc;
    rc = select_device(vl.device_id);
    if (rc != ORBGPU_OK)
        return rc;
    StereoHostWs &ws = per_device_workspace<StereoHostWs>(vl.device_id);
    if ((rc = ws.bind(vl.device_id, true)) != ORBGPU_OK)
        return rc;
    const size_t cap = (size_t)std::max(std::max(n_l, n_r), 1);
    ws.reserve(KPS_L, sizeof(orbgpu_keypoint) * cap);
    ws.reserve(KPS_R, sizeof(orbgpu_keypoint) * cap);
    ws.reserve(DESC_L, 32 * cap);
    ws.reserve(DESC_R, 32 * cap);
    ws.reserve(COUNTS, sizeof(int) * 2);
    ws.reserve(UR, sizeof(float) * cap);
    ws.reserve(DZ, sizeof(float) * cap);
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    StereoHostWs::FinishOnError on_error{ws};
    const int32_t counts[2] = {n_l, n_r};
    ws.upload(COUNTS, counts, sizeof(counts));
    if (n_l > 0) {
        ws.upload(KPS_L, kps_l, sizeof(orbgpu_keypoint) * n_l);
        ws.upload(DESC_L, desc_l, (size_t)32 * n_l);
    }
    if (n_r > 0) {
        ws.upload(KPS_R, kps_r, sizeof(orbgpu_keypoint) * n_r);
        ws.upload(DESC_R, desc_r, (size_t)32 * n_r);
    }
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    rc = orbgpu_stereo_matches_batch_device(left, 0, right, 0, 1, (int32_t)cap, ws.as<orbgpu_keypoint>(KPS_L), ws.as<int32_t>(COUNTS),
                                            ws.as<uint8_t>(DESC_L), ws.as<orbgpu_keypoint>(KPS_R), ws.as<int32_t>(COUNTS) + 1,
                                            ws.as<uint8_t>(DESC_R), mbf, fx, ws.as<float>(UR), ws.as<float>(DZ), nullptr,
                                            ws.stream);
    if (rc != ORBGPU_OK)
        return rc;
    ws.download(u_right, UR, sizeof(float) * n_l);  // n_l > 0 here
    ws.download(depth, DZ, sizeof(float) * n_l);
    return ws.finish();
}

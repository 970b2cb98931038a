// Sim3Solver (Sim3Solver.cc) on the device: Horn's closed-form alignment of three point pairs per hypothesis, 2 N
// reprojections per hypothesis, the reference's sequential acceptance rule replayed over the counts.  The definition
// (H1-H8, "OpenCV boundary unpinned") is in include/orbgpu.h and tests/sim3_model.py; the arithmetic below is the
// model's operation for operation (-ffp-contract=off), only atan2 / sin / cos come from another libm.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "carve.h"
#include "common.h"
#include "jacobi.h"
#include "ransac_host.h"
#include "staging.h"

namespace orbgpu {

constexpr int S3_THREADS = 256;  // 4 waves, one hypothesis each: a first guess, not a tuned shape
constexpr int S3_WAVES = S3_THREADS / 64;
constexpr int S3_MAX_N1 = 65536, S3_MAX_HYP = 4096;
constexpr int S3_JACOBI_SWEEPS = 16;

struct Sim3Ctl {
    int32_t n, max_its, n_use, pad;
};

struct Sim3ProblemDev {
    const uint8_t *valid;
    const float *Xw1, *Xw2;
    const int32_t *octave1, *octave2, *triples;
    int32_t *counts;
    float *R, *t, *s, *T12;
    unsigned long long *masks;
    int32_t *indices1;
    orbgpu_sim3_result *result;
    float4 *rec;       // [3][n1]: (X1c, maxError1 or NaN) | (X2c, maxError2) | (p1im1, p2im2), by i1
    int32_t *map;      // [n1] compacted -> i1
    Sim3Ctl *ctl;
    int32_t n1, n_hyp, nlevels, fix_scale, min_inliers, start_iteration, best_so_far;
    float T1w[16], T2w[16];
    float K1[4], K2[4];  // fx fy cx cy
    float max_error[ORBGPU_MAX_LEVELS];
};

// H2: cv::gemm's small-matrix path
__device__ inline void rt_apply(const float *T, float x, float y, float z, float out[3])
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float t0 = (T[4 * i] * x + T[4 * i + 1] * y) + T[4 * i + 2] * z;
        out[i] = t0 + T[4 * i + 3];
    }
}

__device__ inline void to_image(const float *K, const float X[3], float &u, float &v)
{
    const float invz = 1.0f / X[2];
    const float x = X[0] * invz, y = X[1] * invz;
    u = K[0] * x + K[2];
    v = K[1] * y + K[3];
}

// row i1 is kept (1), valid with an octave out of range (2), or not valid (0)
__device__ inline int row_kind(const Sim3ProblemDev &P, int i)
{
    if (i >= P.n1 || !P.valid[i])
        return 0;
    const int o1 = P.octave1[i], o2 = P.octave2[i];
    return (o1 < 0 || o1 >= P.nlevels || o2 < 0 || o2 >= P.nlevels) ? 2 : 1;
}

// One workgroup per problem: H1-H3.  Writes a record for EVERY row i1 < n1 (maxError1 = NaN for a row that is not kept,
// so it can never be an inlier), the compacted -> i1 map, N and n_bad_index.
__global__ __launch_bounds__(S3_THREADS) void k_sim3_prepare(const Sim3ProblemDev *__restrict__ problems)
{
    __shared__ int wcount[S3_WAVES][2];
    const Sim3ProblemDev &P = problems[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n1 = P.n1;
    int at = 0, nbad = 0;
    for (int base = 0; base < n1; base += S3_THREADS) {
        const int i = base + tid;
        const int kind = row_kind(P, i);
        const unsigned long long m1 = __ballot(kind == 1), m2 = __ballot(kind == 2);
        __syncthreads();
        if (lane == 0)
            wcount[wave][0] = __popcll(m1), wcount[wave][1] = __popcll(m2);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int wv = 0; wv < S3_WAVES; wv++) {
            before += wv < wave ? wcount[wv][0] : 0;
            total += wcount[wv][0];
            nbad += wcount[wv][1];
        }
        if (i < n1) {
            float4 a, b, c;
            const float qnan = __int_as_float(0x7fc00000);
            a = b = c = make_float4(0.f, 0.f, 0.f, qnan);
            if (kind == 1) {
                const int e = at + before + __popcll(m1 & ((1ull << lane) - 1ull));
                P.map[e] = i;
                if (P.indices1)
                    P.indices1[e] = i;
                float X1[3], X2[3], u1, v1, u2, v2;
                rt_apply(P.T1w, P.Xw1[3 * (size_t)i], P.Xw1[3 * (size_t)i + 1], P.Xw1[3 * (size_t)i + 2], X1);
                rt_apply(P.T2w, P.Xw2[3 * (size_t)i], P.Xw2[3 * (size_t)i + 1], P.Xw2[3 * (size_t)i + 2], X2);
                to_image(P.K1, X1, u1, v1);
                to_image(P.K2, X2, u2, v2);
                a = make_float4(X1[0], X1[1], X1[2], P.max_error[P.octave1[i]]);
                b = make_float4(X2[0], X2[1], X2[2], P.max_error[P.octave2[i]]);
                c = make_float4(u1, v1, u2, v2);
            }
            P.rec[i] = a;
            P.rec[(size_t)n1 + i] = b;
            P.rec[2 * (size_t)n1 + i] = c;
        }
        at += total;
    }
    if (tid == 0) {
        P.ctl->n = at;
        orbgpu_sim3_result *r = P.result;
        r->n = at, r->n_bad_index = nbad, r->n_bad_triple = 0;
    }
}

// ---- H6 (the cyclic Jacobi of the 4 x 4: jacobi.h) ----------------------------------------------------------------------
struct Sim3Hyp {
    float R[9], t[3], s, T12[16], T21[16];
};

// P1[k], P2[k]: the three points in camera 1 / camera 2
__device__ inline void horn(const float P1[3][3], const float P2[3][3], bool fix_scale, Sim3Hyp &h)
{
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        O1[a] = ((P1[0][a] + P1[1][a]) + P1[2][a]) / 3.0f;
        O2[a] = ((P2[0][a] + P2[1][a]) + P2[2][a]) / 3.0f;
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            Pr1[k][a] = P1[k][a] - O1[a];
            Pr2[k][a] = P2[k][a] - O2[a];
        }
    float M[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            M[i][j] = (float)(((double)Pr2[0][i] * (double)Pr1[0][j] + (double)Pr2[1][i] * (double)Pr1[1][j]) +
                              (double)Pr2[2][i] * (double)Pr1[2][j]);
    const double m00 = M[0][0], m01 = M[0][1], m02 = M[0][2], m10 = M[1][0], m11 = M[1][1], m12 = M[1][2], m20 = M[2][0],
                 m21 = M[2][1], m22 = M[2][2];
    const float N11 = (float)((m00 + m11) + m22), N12 = (float)(m12 - m21), N13 = (float)(m20 - m02), N14 = (float)(m01 - m10);
    const float N22 = (float)((m00 - m11) - m22), N23 = (float)(m01 + m10), N24 = (float)(m20 + m02);
    const float N33 = (float)((-m00 + m11) - m22), N34 = (float)(m12 + m21), N44 = (float)((-m00 - m11) + m22);
    double A[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34}, {N14, N24, N34, N44}};
    double V[4][4];
    jacobi4_lane<S3_JACOBI_SWEEPS>(A, V);
    double best = A[0][0], q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int k = 1; k < 4; k++)
        if (A[k][k] > best) {
            best = A[k][k];
#pragma unroll
            for (int r = 0; r < 4; r++)
                q[r] = V[r][k];
        }
    const double nv = sqrt((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3]);
    const double ang = atan2(nv, q[0]);
    double vec[3], r[3];
#pragma unroll
    for (int a = 0; a < 3; a++)
        vec[a] = ((2.0 * ang) * q[1 + a]) / nv;
    const double theta = sqrt((vec[0] * vec[0] + vec[1] * vec[1]) + vec[2] * vec[2]);
    const double cs = cos(theta), sn = sin(theta), c1 = 1.0 - cs;
#pragma unroll
    for (int a = 0; a < 3; a++)
        r[a] = vec[a] / theta;
    const double Kx[9] = {0.0, -r[2], r[1], r[2], 0.0, -r[0], -r[1], r[0], 0.0};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            h.R[3 * i + j] = (float)((cs * (i == j ? 1.0 : 0.0) + c1 * (r[i] * r[j])) + sn * Kx[3 * i + j]);
    const float *R = h.R;
    float s = 1.0f;
    if (!fix_scale) {
        float P3[3][3];  // [k][i]
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int i = 0; i < 3; i++)
                P3[k][i] = (R[3 * i] * Pr2[k][0] + R[3 * i + 1] * Pr2[k][1]) + R[3 * i + 2] * Pr2[k][2];
        double nom = 0.0, den = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) {
                nom += (double)Pr1[k][i] * (double)P3[k][i];
                den += (double)(P3[k][i] * P3[k][i]);
            }
        s = (float)(nom / den);
    }
    h.s = s;
    const float inv_s = 1.0f / s;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float u = (R[3 * i] * O2[0] + R[3 * i + 1] * O2[1]) + R[3 * i + 2] * O2[2];
        h.t[i] = O1[i] - s * u;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            h.T12[4 * i + j] = s * R[3 * i + j];
            h.T21[4 * i + j] = inv_s * R[3 * j + i];
        }
        h.T12[4 * i + 3] = h.t[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
        h.T21[4 * i + 3] = -((h.T21[4 * i] * h.t[0] + h.T21[4 * i + 1] * h.t[1]) + h.T21[4 * i + 2] * h.t[2]);
#pragma unroll
    for (int j = 0; j < 4; j++)
        h.T12[12 + j] = h.T21[12 + j] = j == 3 ? 1.0f : 0.0f;
}

// grid (ceil(max n_hyp / 4), problems), one wave per hypothesis.  Every lane computes the Horn step from the same three
// records (same bits in every lane), then the 64 lanes stride over the rows i1: one ballot is one word of the mask.
// There is no barrier in this kernel, so a wave may leave early.
__global__ __launch_bounds__(S3_THREADS) void k_sim3_hypotheses(const Sim3ProblemDev *__restrict__ problems)
{
    const Sim3ProblemDev &P = problems[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = blockIdx.x * S3_WAVES + wave;
    if (h >= P.n_hyp)
        return;
    const int N = P.ctl->n, n_use = P.ctl->n_use, n1 = P.n1;
    if (h >= n_use) {
        if (lane == 0)
            P.counts[h] = 0;
        return;
    }
    const int words = (n1 + 63) >> 6;
    int tr[3];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        tr[k] = P.triples[3 * (size_t)h + k];
        if (tr[k] < 0 || tr[k] >= N) {
            bad = true;
            tr[k] = 0;
        }
    }
    if (bad || N == 0) {  // never read through; N == 0 cannot hold a valid index
        const float qnan = __int_as_float(0x7fc00000);
        if (lane == 0) {
            P.counts[h] = 0;
            P.s[h] = qnan;
            atomicAdd(&P.result->n_bad_triple, 1);
        }
        if (lane < 9)
            P.R[9 * (size_t)h + lane] = qnan;
        if (lane < 3)
            P.t[3 * (size_t)h + lane] = qnan;
        if (lane < 16)
            P.T12[16 * (size_t)h + lane] = qnan;
        for (int w = lane; w < words; w += 64)
            P.masks[(size_t)h * words + w] = 0ull;
        return;
    }
    float P1[3][3], P2[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int i = P.map[tr[k]];
        const float4 a = P.rec[i], b = P.rec[(size_t)n1 + i];
        P1[k][0] = a.x, P1[k][1] = a.y, P1[k][2] = a.z;
        P2[k][0] = b.x, P2[k][1] = b.y, P2[k][2] = b.z;
    }
    Sim3Hyp H;
    horn(P1, P2, P.fix_scale != 0, H);
    if (lane == 0) {  // constant indices only: H stays in registers
        P.s[h] = H.s;
#pragma unroll
        for (int k = 0; k < 9; k++)
            P.R[9 * (size_t)h + k] = H.R[k];
#pragma unroll
        for (int k = 0; k < 3; k++)
            P.t[3 * (size_t)h + k] = H.t[k];
#pragma unroll
        for (int k = 0; k < 16; k++)
            P.T12[16 * (size_t)h + k] = H.T12[k];
    }
    int count = 0;
    for (int base = 0; base < n1; base += 64) {
        const int i = base + lane;
        bool inl = false;
        if (i < n1) {
            const float4 a = P.rec[i], b = P.rec[(size_t)n1 + i], c = P.rec[2 * (size_t)n1 + i];
            float Q[3], W[3], u, v;
            rt_apply(H.T12, b.x, b.y, b.z, Q);
            to_image(P.K1, Q, u, v);
            const float d1x = c.x - u, d1y = c.y - v;
            const float err1 = (float)((double)d1x * (double)d1x + (double)d1y * (double)d1y);
            rt_apply(H.T21, a.x, a.y, a.z, W);
            to_image(P.K2, W, u, v);
            const float d2x = u - c.z, d2y = v - c.w;
            const float err2 = (float)((double)d2x * (double)d2x + (double)d2y * (double)d2y);
            inl = err1 < a.w && err2 < b.w;
        }
        const unsigned long long word = __ballot(inl);
        if (lane == 0)
            P.masks[(size_t)h * words + (base >> 6)] = word;
        count += __popcll(word);
    }
    if (lane == 0)
        P.counts[h] = count;
}

// H8, one thread per problem: the reference's loop over the counts
__global__ void k_sim3_select(const Sim3ProblemDev *__restrict__ problems, int n)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n)
        return;
    const Sim3ProblemDev &P = problems[k];
    const Sim3Ctl c = *P.ctl;
    orbgpu_sim3_result *r = P.result;
    int it = P.start_iteration, best = P.best_so_far, best_it = -1, accepted = -1, n_inl = 0, no_more = 0;
    if (c.n < P.min_inliers) {
        no_more = 1;
    } else {
        while (it < c.n_use) {
            const int cnt = P.counts[it];
            const int cur = it++;
            if (cnt >= best) {
                best = cnt, best_it = cur;
                if (cnt > P.min_inliers) {
                    accepted = cur, n_inl = cnt;
                    break;
                }
            }
        }
        if (accepted < 0 && it >= c.max_its)
            no_more = 1;
    }
    r->max_its = c.max_its;
    r->accepted = accepted, r->n_inliers = n_inl, r->best_inliers = best, r->best_iteration = best_it;
    r->iterations = it, r->no_more = no_more;
}

// Per (thread, device) staging of the entry points (staging.h); the stream and the two H_* blocks (the uploaded
// problem and its outputs) are the host flavour's.
enum { PROBLEMS, REC, MAP, CTL, H_IN, H_OUT, N_BUF };
struct Sim3Ws : Staging<N_BUF> {
    std::vector<Sim3ProblemDev> h_problems;  // sources of asynchronous uploads: they outlive the call
    std::vector<Sim3Ctl> h_ctl;
    ~Sim3Ws() { release(); }  // the stream is waited for while the vectors are still there
};

static int ransac_iterations(int n, double probability, int min_inliers, int max_iterations)
{
    return ransac_max_iterations(n, min_inliers, (float)min_inliers / (float)n, probability, max_iterations);
}

static int check_common(const orbgpu_sim3_problem &p, int k)
{
    ORBGPU_REQUIRE(p.n1 >= 0 && p.n1 <= S3_MAX_N1, "problem %d: n1 outside [0, %d]", k, S3_MAX_N1);
    ORBGPU_REQUIRE(p.n_hyp >= 0 && p.n_hyp <= S3_MAX_HYP, "problem %d: n_hyp outside [0, %d]", k, S3_MAX_HYP);
    ORBGPU_REQUIRE(p.nlevels >= 1 && p.nlevels <= ORBGPU_MAX_LEVELS, "problem %d: nlevels outside [1, %d]", k,
                   ORBGPU_MAX_LEVELS);
    ORBGPU_REQUIRE(p.min_inliers >= 0 && p.max_iterations >= 0 && p.start_iteration >= 0 && p.best_so_far >= 0,
                   "problem %d: negative min_inliers / max_iterations / start_iteration / best_so_far", k);
    ORBGPU_REQUIRE(p.n1 == 0 || (p.valid && p.Xw1 && p.Xw2 && p.octave1 && p.octave2), "problem %d: null input arrays", k);
    ORBGPU_REQUIRE(p.n_hyp == 0 || p.triples, "problem %d: null triples", k);
    return ORBGPU_OK;
}

static int check_device_problem(const orbgpu_sim3_problem &p, int k)
{
    int rc = check_common(p, k);
    if (rc != ORBGPU_OK)
        return rc;
    ORBGPU_REQUIRE(p.result, "problem %d: null result", k);
    ORBGPU_REQUIRE(p.n_hyp == 0 || (p.counts && p.R && p.t && p.s && p.T12 && (p.n1 == 0 || p.masks)),
                   "problem %d: null output arrays", k);
    return ORBGPU_OK;
}

} // namespace orbgpu

using namespace orbgpu;

extern "C" int orbgpu_sim3_ransac_iterations(int32_t n, double probability, int32_t min_inliers, int32_t max_iterations,
                                             int32_t *max_its)
{
    ORBGPU_REQUIRE(max_its && n >= 0 && min_inliers >= 0 && max_iterations >= 0, "bad arguments");
    *max_its = ransac_iterations(n, probability, min_inliers, max_iterations);
    return ORBGPU_OK;
}

extern "C" int orbgpu_sim3_solve_batch_device(int32_t n, const orbgpu_sim3_problem *problems, int32_t device_id,
                                              void *hip_stream)
{
    Sim3Ws *wsp;
    int rc = batch_begin(n, problems, check_device_problem, device_id, wsp);
    if (rc != ORBGPU_OK || !wsp)
        return rc;
    Sim3Ws &ws = *wsp;
    size_t rows = 0;
    int max_hyp = 0;
    for (int k = 0; k < n; k++) {
        rows += (size_t)problems[k].n1;
        max_hyp = std::max(max_hyp, (int)problems[k].n_hyp);
    }
    ws.reserve(PROBLEMS, sizeof(Sim3ProblemDev) * (size_t)n);
    ws.reserve(REC, 3 * sizeof(float4) * std::max<size_t>(rows, 1));
    ws.reserve(MAP, sizeof(int32_t) * std::max<size_t>(rows, 1));
    ws.reserve(CTL, sizeof(Sim3Ctl) * (size_t)n);
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    std::vector<Sim3ProblemDev> &hp = ws.h_problems;
    std::vector<Sim3Ctl> &ctl = ws.h_ctl;
    ORBGPU_HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));  // an earlier call's uploads have left hp / ctl
    hp.resize((size_t)n), ctl.resize((size_t)n);
    size_t ro = 0;
    for (int k = 0; k < n; k++) {
        const orbgpu_sim3_problem &p = problems[k];
        Sim3ProblemDev &D = hp[k];
        memset(&D, 0, sizeof(D));
        D.valid = p.valid, D.Xw1 = p.Xw1, D.Xw2 = p.Xw2, D.octave1 = p.octave1, D.octave2 = p.octave2, D.triples = p.triples;
        D.counts = p.counts, D.R = p.R, D.t = p.t, D.s = p.s, D.T12 = p.T12;
        D.masks = reinterpret_cast<unsigned long long *>(p.masks);
        D.indices1 = p.indices1, D.result = p.result;
        D.rec = ws.as<float4>(REC) + 3 * ro, D.map = ws.as<int32_t>(MAP) + ro, D.ctl = ws.as<Sim3Ctl>(CTL) + k;
        ro += (size_t)p.n1;
        D.n1 = p.n1, D.n_hyp = p.n_hyp, D.nlevels = p.nlevels, D.fix_scale = p.fix_scale, D.min_inliers = p.min_inliers;
        D.start_iteration = p.start_iteration, D.best_so_far = p.best_so_far;
        memcpy(D.T1w, p.T1w, sizeof(D.T1w));
        memcpy(D.T2w, p.T2w, sizeof(D.T2w));
        D.K1[0] = p.fx1, D.K1[1] = p.fy1, D.K1[2] = p.cx1, D.K1[3] = p.cy1;
        D.K2[0] = p.fx2, D.K2[1] = p.fy2, D.K2[2] = p.cx2, D.K2[3] = p.cy2;
        for (int l = 0; l < p.nlevels; l++) {  // H3
            const double e = 9.210 * (double)p.level_sigma2[l];
            D.max_error[l] = e >= 0.0 ? (float)std::trunc(e) : 0.0f;
        }
    }
    const hipStream_t st = (hipStream_t)hip_stream;
    ORBGPU_HIP_TRY(hipMemcpyAsync(ws.buf[PROBLEMS].p, hp.data(), sizeof(Sim3ProblemDev) * (size_t)n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_sim3_prepare, dim3(n), dim3(S3_THREADS), 0, st, ws.as<Sim3ProblemDev>(PROBLEMS));
    ORBGPU_HIP_TRY(hipGetLastError());
    ORBGPU_HIP_TRY(hipMemcpyAsync(ctl.data(), ws.buf[CTL].p, sizeof(Sim3Ctl) * (size_t)n, hipMemcpyDeviceToHost, st));
    ORBGPU_HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < n; k++) {
        const orbgpu_sim3_problem &p = problems[k];
        Sim3Ctl &c = ctl[k];
        c.max_its = ransac_iterations(c.n, p.probability, p.min_inliers, p.max_iterations);
        c.n_use = c.n < p.min_inliers ? 0 : std::min((int)p.n_hyp, c.max_its);
        c.pad = 0;
    }
    ORBGPU_HIP_TRY(hipMemcpyAsync(ws.buf[CTL].p, ctl.data(), sizeof(Sim3Ctl) * (size_t)n, hipMemcpyHostToDevice, st));
    if (max_hyp > 0) {
        hipLaunchKernelGGL(k_sim3_hypotheses, dim3((max_hyp + S3_WAVES - 1) / S3_WAVES, n), dim3(S3_THREADS), 0, st,
                           ws.as<Sim3ProblemDev>(PROBLEMS));
        ORBGPU_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_sim3_select, dim3((n + 63) / 64), dim3(64), 0, st, ws.as<Sim3ProblemDev>(PROBLEMS), n);
    ORBGPU_HIP_TRY(hipGetLastError());
    return ORBGPU_OK;
}

extern "C" int orbgpu_sim3_solve_device(const orbgpu_sim3_problem *p, int32_t device_id, void *hip_stream)
{
    ORBGPU_REQUIRE(p, "null argument");
    return orbgpu_sim3_solve_batch_device(1, p, device_id, hip_stream);
}

// The host flavours.  all = false: R / t / s / T12 of the best iteration and the accepted iteration's inlier bytes;
// all = true: R [H][9], t [H][3], s [H], T12 [H][16] and masks [H][words] of every hypothesis.
static int solve_host(const orbgpu_sim3_problem *p, int32_t *counts, float *R, float *t, float *s, float *T12, uint8_t *inliers,
                      uint64_t *masks, bool all, orbgpu_sim3_result *result, int32_t device_id)
{
    ORBGPU_REQUIRE(p && result, "null argument");
    int rc = check_common(*p, 0);
    if (rc != ORBGPU_OK)
        return rc;
    const int n1 = p->n1, H = p->n_hyp;
    // H1 and H4 on the host, to refuse a triple index outside [0, N) before anything is launched
    int N = 0;
    for (int i = 0; i < n1; i++)
        if (p->valid[i] && p->octave1[i] >= 0 && p->octave1[i] < p->nlevels && p->octave2[i] >= 0 && p->octave2[i] < p->nlevels)
            N++;
    const int max_its = ransac_iterations(N, p->probability, p->min_inliers, p->max_iterations);
    const int n_use = N < p->min_inliers ? 0 : std::min(H, max_its);
    for (int h = 0; h < n_use; h++)
        for (int k = 0; k < 3; k++)
            ORBGPU_REQUIRE(p->triples[3 * h + k] >= 0 && p->triples[3 * h + k] < N, "triple %d: index %d outside [0, %d)", h,
                           p->triples[3 * h + k], N);
    // one staging block each way; all = false fetches its rows of R / t / s / T12 / masks after the launch, below
    const size_t words = (size_t)(n1 + 63) / 64;
    orbgpu_sim3_result r;
    HostPlan<N_BUF> plan;
    const auto i_valid = plan.in(H_IN, p->valid, n1);
    const auto i_x1 = plan.in(H_IN, p->Xw1, n1, 3), i_x2 = plan.in(H_IN, p->Xw2, n1, 3);
    const auto i_o1 = plan.in(H_IN, p->octave1, n1), i_o2 = plan.in(H_IN, p->octave2, n1);
    const auto i_tr = plan.in(H_IN, p->triples, H, 3);
    const auto o_res = plan.out(H_OUT, &r, 1);
    const auto o_cnt = plan.out(H_OUT, counts, H);
    const auto o_R = plan.out(H_OUT, all ? R : nullptr, H, 9), o_t = plan.out(H_OUT, all ? t : nullptr, H, 3);
    const auto o_s = plan.out(H_OUT, all ? s : nullptr, H), o_T = plan.out(H_OUT, all ? T12 : nullptr, H, 16);
    const auto o_m = plan.out(H_OUT, masks, H, words);
    Sim3Ws *wsp;
    if ((rc = host_begin(device_id, plan, wsp)) != ORBGPU_OK)
        return rc;
    Sim3Ws &ws = *wsp;
    Sim3Ws::FinishOnError on_error{ws};
    plan.upload(ws);
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    if (all)  // hypotheses beyond n_use are not written by the kernels: they come back as zeros
        ORBGPU_HIP_TRY(hipMemsetAsync(ws.as<char>(H_OUT), 0, plan.bytes(H_OUT), ws.stream));
    orbgpu_sim3_problem d = *p;
    d.valid = ws.at(i_valid), d.Xw1 = ws.at(i_x1), d.Xw2 = ws.at(i_x2);
    d.octave1 = ws.at(i_o1), d.octave2 = ws.at(i_o2), d.triples = ws.at(i_tr);
    d.result = ws.at(o_res), d.counts = ws.at(o_cnt);
    d.R = ws.at(o_R), d.t = ws.at(o_t), d.s = ws.at(o_s);
    d.T12 = ws.at(o_T), d.masks = ws.at(o_m);
    d.indices1 = nullptr;
    if ((rc = orbgpu_sim3_solve_batch_device(1, &d, device_id, ws.stream)) != ORBGPU_OK)
        return rc;
    plan.download(ws);
    if ((rc = ws.finish()) != ORBGPU_OK)
        return rc;
    if (all) {
        *result = r;
        return ORBGPU_OK;
    }
    const int b = r.best_iteration;
    if (b >= 0 && b < H) {
        if (R)
            ws.download(R, H_OUT, 36, o_R.off + 36 * (size_t)b);
        if (t)
            ws.download(t, H_OUT, 12, o_t.off + 12 * (size_t)b);
        if (s)
            ws.download(s, H_OUT, 4, o_s.off + 4 * (size_t)b);
        if (T12)
            ws.download(T12, H_OUT, 64, o_T.off + 64 * (size_t)b);
    }
    std::vector<uint64_t> mask(std::max<size_t>(words, 1), 0);
    if (r.accepted >= 0 && words > 0)
        ws.download(mask.data(), H_OUT, 8 * words, o_m.off + 8 * words * (size_t)r.accepted);
    if ((rc = ws.finish()) != ORBGPU_OK)
        return rc;
    if (inliers)
        mask_to_bytes(mask.data(), n1, inliers);
    *result = r;
    return ORBGPU_OK;
}

extern "C" int orbgpu_sim3_solve(const orbgpu_sim3_problem *p, int32_t *counts, float *R, float *t, float *s, float *T12,
                                 uint8_t *inliers, orbgpu_sim3_result *result, int32_t device_id)
{
    return solve_host(p, counts, R, t, s, T12, inliers, nullptr, false, result, device_id);
}

extern "C" int orbgpu_sim3_solve_all(const orbgpu_sim3_problem *p, int32_t *counts, float *R, float *t, float *s, float *T12,
                                     uint64_t *masks, orbgpu_sim3_result *result, int32_t device_id)
{
    return solve_host(p, counts, R, t, s, T12, nullptr, masks, true, result, device_id);
}

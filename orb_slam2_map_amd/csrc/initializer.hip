// Initializer (Initializer.cc) on the device: 8-point homography and fundamental-matrix hypotheses over host-drawn minimal
// sets, the reference's checks over all matches, its scans and branch, the 8 (Faugeras) or 4 (DecomposeE) motions, CheckRT
// with a triangulation per lane, and its accept rule.  The definition (I1-I10, "OpenCV boundary unpinned") is in
// include/orbgpu.h and tests/init_model.py; the arithmetic below is the model's operation for operation
// (-ffp-contract=off): FP64 where OpenCV's SVD stood, float where the reference computes in float, only +, -, *, /, sqrt
// and comparisons on the device (float / and sqrt go through the correctly rounded FP64 ones), no libm.
//
// Five kernels per call: k_init_prepare (one wave per problem), k_init_hypotheses (one wave per hypothesis and model),
// k_init_select (one wave per problem), k_init_checkrt (one wave per motion), k_init_finish (one wave per problem).
// The Jacobi of the wave-wide steps is jacobi.h's jacobi_wave (matrices in LDS, the rows of a rotation spread over the lanes);
// the 4x4 of a triangulation runs in the registers of the lane that owns the pair.
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
namespace {

constexpr int INIT_MAX_N = 16384, INIT_MAX_HYP = 4096;
constexpr int INIT_JACOBI_SWEEPS = 30;
constexpr int ILD = 12;  // row stride of the LDS matrices (jacobi.h)

struct InitCtl {
    int32_t n, best_h, best_f, use_h, n_motions, n_inliers;
    float T1[4], T2[4];  // sX sY -meanX*sX -meanY*sY
    float R[8][9], t[8][3];
    int32_t n_good[8];
    float cosp[8];
};

struct InitProblemDev {
    const float *kp1, *kp2;
    const int32_t *matches12, *sets;
    float *scores_h, *scores_f;
    unsigned long long *masks_h, *masks_f;
    float *R21, *t21, *P3D;
    uint8_t *triangulated;
    orbgpu_init_result *result;
    float4 *pts;      // [n1] compacted: u1 v1 u2 v2
    float4 *pn;       // [n1] compacted, normalised
    int32_t *first;   // [n1] compacted -> i
    float *mats;      // [n_hyp][2][9]
    float *p3d;       // [8][n1][3], zeroed by the entry point
    uint8_t *good;    // [8][n1], zeroed by the entry point
    float *cosv;      // [8][n1]: the cosines of a motion's good pairs
    InitCtl *ctl;
    int32_t n1, n2, n_hyp, min_triangulated;
    float K[4], sigma, cos_limit_f, cos_limit_h;
};

// ---- float steps with one rounding each --------------------------------------------------------------------------------
__device__ inline float fdiv(float a, float b) { return (float)((double)a / (double)b); }
__device__ inline float fsqrt(float a) { return (float)sqrt((double)a); }
__device__ inline float finv(float x) { return (float)(1.0 / (double)x); }
__device__ inline float fdot3(float a, float b, float c, float d, float e, float f) { return (a * b + c * d) + e * f; }

// C = A B, FP64, (a b + c d) + e f per entry
__device__ inline void mul3(const double *A, const double *B, double *C)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

// C = A B in float
__device__ inline void fmul3(const float *A, const float *B, float *C)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

// float(A B C) of three matrices of float entries
__device__ inline void triple3(const double *A, const float *Bf, const double *C, float *out)
{
    double B[9], AB[9], ABC[9];
#pragma unroll
    for (int e = 0; e < 9; e++)
        B[e] = (double)Bf[e];
    mul3(A, B, AB);
    mul3(AB, C, ABC);
#pragma unroll
    for (int e = 0; e < 9; e++)
        out[e] = (float)ABC[e];
}

// cv::determinant's expression in double over float entries
__device__ inline double det3d(const float *m)
{
    const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
    return (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g);
}

__device__ inline void tmat(const float *T, double *M)  // [sX 0 tx; 0 sY ty; 0 0 1]
{
    M[0] = (double)T[0], M[1] = 0.0, M[2] = (double)T[2];
    M[3] = 0.0, M[4] = (double)T[1], M[5] = (double)T[3];
    M[6] = 0.0, M[7] = 0.0, M[8] = 1.0;
}

__device__ inline unsigned cos_key(float c)
{
    const unsigned u = __float_as_uint(c);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ inline float key_cos(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ---- the LDS of the wave-wide Jacobi (jacobi.h) --------------------------------------------------------------------------
struct InitLds {
    double A[ILD * ILD], V[ILD * ILD], Ut[ILD * ILD], w[ILD];
    float rows[16 * 9];
    float terms[128];
};

// I4: A = U diag(d) V' of a 3x3 of float entries.  U[3 i + k] = component i of u_k, Vt[3 k + j] = component j of v_k.
// proper: u_2 takes the sign of A v_2; otherwise the sign rule.  Every lane returns the same values.
__device__ void svd3_wave(InitLds &S, const float *Af, int lane, bool proper, double *U, double *d, double *Vt)
{
    double A[9];
#pragma unroll
    for (int e = 0; e < 9; e++)
        A[e] = (double)Af[e];
    __syncthreads();
    if (lane < 9) {
        const int a = lane / 3, b = lane % 3;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 3; j++)
            s = s + A[3 * j + a] * A[3 * j + b];
        S.A[a * ILD + b] = s;
    }
    __syncthreads();
    sorted_eig_wave<ILD, INIT_JACOBI_SWEEPS>(S, 3, lane);
    double av[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int j = 0; j < 3; j++)
            Vt[3 * k + j] = S.Ut[k * ILD + j];
#pragma unroll
        for (int i = 0; i < 3; i++)
            av[k][i] = (A[3 * i] * Vt[3 * k] + A[3 * i + 1] * Vt[3 * k + 1]) + A[3 * i + 2] * Vt[3 * k + 2];
        d[k] = sqrt((av[k][0] * av[k][0] + av[k][1] * av[k][1]) + av[k][2] * av[k][2]);
    }
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
        for (int i = 0; i < 3; i++)
            U[3 * i + k] = av[k][i] / d[k];
    double c[3];
    c[0] = U[3] * U[7] - U[6] * U[4];
    c[1] = U[6] * U[1] - U[0] * U[7];
    c[2] = U[0] * U[4] - U[3] * U[1];
    const double nc = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
#pragma unroll
    for (int i = 0; i < 3; i++)
        c[i] = c[i] / nc;
    bool flip;
    if (proper) {
        flip = (c[0] * av[2][0] + c[1] * av[2][1]) + c[2] * av[2][2] < 0.0;
    } else {
        double big = fabs(c[0]), lead = c[0];
        if (fabs(c[1]) > big)
            big = fabs(c[1]), lead = c[1];
        if (fabs(c[2]) > big)
            big = fabs(c[2]), lead = c[2];
        flip = lead < 0.0;
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
        U[3 * i + 2] = flip ? -c[i] : c[i];
}

// ---- I1, I3 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_init_prepare(const InitProblemDev *__restrict__ problems)
{
    const InitProblemDev &P = problems[blockIdx.x];
    const int lane = threadIdx.x, n1 = P.n1, n2 = P.n2;
    // Normalize: lane 0 / 1 the x / y of frame 1, lane 2 / 3 of frame 2; the reference's running sums in index order
    float mean = 0.f, sc = 0.f;
    if (lane < 4) {
        const float *kp = lane < 2 ? P.kp1 : P.kp2;
        const int n = lane < 2 ? n1 : n2, c = lane & 1;
        float s = 0.f;
        for (int i = 0; i < n; i++)
            s = s + kp[2 * (size_t)i + c];
        mean = fdiv(s, (float)n);
        float dv = 0.f;
        for (int i = 0; i < n; i++)
            dv = dv + fabsf(kp[2 * (size_t)i + c] - mean);
        sc = finv(fdiv(dv, (float)n));
    }
    const float mx1 = __shfl(mean, 0, 64), my1 = __shfl(mean, 1, 64), mx2 = __shfl(mean, 2, 64), my2 = __shfl(mean, 3, 64);
    const float sx1 = __shfl(sc, 0, 64), sy1 = __shfl(sc, 1, 64), sx2 = __shfl(sc, 2, 64), sy2 = __shfl(sc, 3, 64);
    int at = 0, nbad = 0;
    for (int base = 0; base < n1; base += 64) {
        const int i = base + lane;
        const int m = i < n1 ? P.matches12[i] : -1;
        const bool kept = m >= 0 && m < n2;
        const unsigned long long mk = __ballot(kept), mb = __ballot(i < n1 && m >= n2);
        if (kept) {
            const int e = at + __popcll(mk & ((1ull << lane) - 1ull));
            const float u1 = P.kp1[2 * (size_t)i], v1 = P.kp1[2 * (size_t)i + 1];
            const float u2 = P.kp2[2 * (size_t)m], v2 = P.kp2[2 * (size_t)m + 1];
            P.pts[e] = make_float4(u1, v1, u2, v2);
            P.pn[e] = make_float4((u1 - mx1) * sx1, (v1 - my1) * sy1, (u2 - mx2) * sx2, (v2 - my2) * sy2);
            P.first[e] = i;
        }
        if (i < n1) {
            P.P3D[3 * (size_t)i] = P.P3D[3 * (size_t)i + 1] = P.P3D[3 * (size_t)i + 2] = 0.f;
            P.triangulated[i] = 0;
        }
        at += __popcll(mk);
        nbad += __popcll(mb);
    }
    if (lane == 0) {
        InitCtl &c = *P.ctl;
        c.n = at;
        c.T1[0] = sx1, c.T1[1] = sy1, c.T1[2] = -mx1 * sx1, c.T1[3] = -my1 * sy1;
        c.T2[0] = sx2, c.T2[1] = sy2, c.T2[2] = -mx2 * sx2, c.T2[3] = -my2 * sy2;
        orbgpu_init_result *r = P.result;
        r->n = at, r->n_bad_index = nbad, r->n_bad_set = 0;
    }
}

// ---- I4, I5: grid (max n_hyp, 2, problems), one wave per hypothesis and model (y = 0: H, 1: F) ---------------------------
__global__ __launch_bounds__(64) void k_init_hypotheses(const InitProblemDev *__restrict__ problems)
{
    __shared__ InitLds S;
    const InitProblemDev &P = problems[blockIdx.z];
    const int lane = threadIdx.x, h = blockIdx.x, model = blockIdx.y;
    if (h >= P.n_hyp)
        return;
    const InitCtl &ctl = *P.ctl;
    const int N = ctl.n, words = (P.n1 + 63) >> 6;
    float *score_out = (model ? P.scores_f : P.scores_h) + h;
    unsigned long long *mask = (model ? P.masks_f : P.masks_h) + (size_t)h * words;
    float *mat = P.mats + ((size_t)h * 2 + model) * 9;
    const int e8 = (lane < 8 && N >= 8) ? P.sets[(size_t)h * 8 + lane] : 0;
    const bool bad = __ballot(e8 < 0 || e8 >= N) != 0ull;
    if (N < 8 || bad) {  // never read through
        if (lane == 0) {
            *score_out = 0.f;
            if (N >= 8 && model == 0)
                atomicAdd(&P.result->n_bad_set, 1);
        }
        if (lane < 9)
            mat[lane] = 0.f;
        for (int w = lane; w < words; w += 64)
            mask[w] = 0ull;
        return;
    }
    // the DLT's rows
    if (lane < 8) {
        const float4 q = P.pn[e8];
        const float u1 = q.x, v1 = q.y, u2 = q.z, v2 = q.w;
        if (model == 0) {
            float *r0 = S.rows + 18 * lane, *r1 = r0 + 9;
            r0[0] = 0.f, r0[1] = 0.f, r0[2] = 0.f, r0[3] = -u1, r0[4] = -v1, r0[5] = -1.f;
            r0[6] = v2 * u1, r0[7] = v2 * v1, r0[8] = v2;
            r1[0] = u1, r1[1] = v1, r1[2] = 1.f, r1[3] = 0.f, r1[4] = 0.f, r1[5] = 0.f;
            r1[6] = -u2 * u1, r1[7] = -u2 * v1, r1[8] = -u2;
        } else {
            float *r0 = S.rows + 9 * lane;
            r0[0] = u2 * u1, r0[1] = u2 * v1, r0[2] = u2, r0[3] = v2 * u1, r0[4] = v2 * v1, r0[5] = v2;
            r0[6] = u1, r0[7] = v1, r0[8] = 1.f;
        }
    }
    __syncthreads();
    const int nrows = model ? 8 : 16;
    for (int e = lane; e < 81; e += 64) {
        const int a = e / 9, b = e % 9;
        double s = 0.0;
        for (int r = 0; r < nrows; r++)
            s = s + (double)S.rows[9 * r + a] * (double)S.rows[9 * r + b];
        S.A[a * ILD + b] = s;
    }
    __syncthreads();
    sorted_eig_wave<ILD, INIT_JACOBI_SWEEPS>(S, 9, lane);
    float nv[9];
#pragma unroll
    for (int k = 0; k < 9; k++)
        nv[k] = (float)S.Ut[8 * ILD + k];
    double T1[9], T2[9];
    tmat(ctl.T1, T1);
    tmat(ctl.T2, T2);
    float M21[9], M12[9];  // H21 / H12, or F21
    if (model == 0) {
        double T2i[9];  // inv(T2) written out
        T2i[0] = 1.0 / T2[0], T2i[1] = 0.0, T2i[2] = -T2[2] / T2[0];
        T2i[3] = 0.0, T2i[4] = 1.0 / T2[4], T2i[5] = -T2[5] / T2[4];
        T2i[6] = 0.0, T2i[7] = 0.0, T2i[8] = 1.0;
        triple3(T2i, nv, T1, M21);
        const double a = M21[0], b = M21[1], c = M21[2], d = M21[3], e = M21[4], f = M21[5], g = M21[6], hh = M21[7], i = M21[8];
        const double det = (a * (e * i - f * hh) - b * (d * i - f * g)) + c * (d * hh - e * g);
        M12[0] = (float)((e * i - f * hh) / det), M12[1] = (float)((c * hh - b * i) / det), M12[2] = (float)((b * f - c * e) / det);
        M12[3] = (float)((f * g - d * i) / det), M12[4] = (float)((a * i - c * g) / det), M12[5] = (float)((c * d - a * f) / det);
        M12[6] = (float)((d * hh - e * g) / det), M12[7] = (float)((b * g - a * hh) / det), M12[8] = (float)((a * e - b * d) / det);
    } else {
        double U[9], d[3], Vt[9];
        svd3_wave(S, nv, lane, false, U, d, Vt);
        float Fn[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                Fn[3 * i + j] = (float)((d[0] * U[3 * i]) * Vt[j] + (d[1] * U[3 * i + 1]) * Vt[3 + j]);
        const double T2t[9] = {T2[0], 0.0, 0.0, 0.0, T2[4], 0.0, T2[2], T2[5], 1.0};
        triple3(T2t, Fn, T1, M21);
#pragma unroll
        for (int e = 0; e < 9; e++)
            M12[e] = 0.f;
    }
    if (lane < 9)
        mat[lane] = M21[lane];
    // the check over all pairs, 64 at a time; the score is the running sum in index order
    const float inv_sigma2 = finv(P.sigma * P.sigma);
    const float th_h = 5.991f, th_f = 3.841f;
    float score = 0.f;
    for (int base = 0; base < N; base += 64) {
        const int e = base + lane;
        float t1 = 0.f, t2 = 0.f;
        bool in = false;
        if (e < N) {
            const float4 q = P.pts[e];
            const float u1 = q.x, v1 = q.y, u2 = q.z, v2 = q.w;
            in = true;
            if (model == 0) {
                const float w2 = finv((M12[6] * u2 + M12[7] * v2) + M12[8]);
                const float u2in1 = ((M12[0] * u2 + M12[1] * v2) + M12[2]) * w2;
                const float v2in1 = ((M12[3] * u2 + M12[4] * v2) + M12[5]) * w2;
                const float sq1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
                const float chi1 = sq1 * inv_sigma2;
                if (chi1 <= th_h)
                    t1 = th_h - chi1;
                else
                    in = false;
                const float w1 = finv((M21[6] * u1 + M21[7] * v1) + M21[8]);
                const float u1in2 = ((M21[0] * u1 + M21[1] * v1) + M21[2]) * w1;
                const float v1in2 = ((M21[3] * u1 + M21[4] * v1) + M21[5]) * w1;
                const float sq2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
                const float chi2 = sq2 * inv_sigma2;
                if (chi2 <= th_h)
                    t2 = th_h - chi2;
                else
                    in = false;
            } else {
                const float a2 = (M21[0] * u1 + M21[1] * v1) + M21[2];
                const float b2 = (M21[3] * u1 + M21[4] * v1) + M21[5];
                const float c2 = (M21[6] * u1 + M21[7] * v1) + M21[8];
                const float num2 = (a2 * u2 + b2 * v2) + c2;
                const float chi1 = fdiv(num2 * num2, a2 * a2 + b2 * b2) * inv_sigma2;
                if (chi1 <= th_f)
                    t1 = th_h - chi1;
                else
                    in = false;
                const float a1 = (M21[0] * u2 + M21[3] * v2) + M21[6];
                const float b1 = (M21[1] * u2 + M21[4] * v2) + M21[7];
                const float c1 = (M21[2] * u2 + M21[5] * v2) + M21[8];
                const float num1 = (a1 * u1 + b1 * v1) + c1;
                const float chi2 = fdiv(num1 * num1, a1 * a1 + b1 * b1) * inv_sigma2;
                if (chi2 <= th_f)
                    t2 = th_h - chi2;
                else
                    in = false;
            }
        }
        const unsigned long long word = __ballot(in);
        if (lane == 0)
            mask[base >> 6] = word;
        __syncthreads();
        S.terms[2 * lane] = t1, S.terms[2 * lane + 1] = t2;
        __syncthreads();
        for (int k = 0; k < 128; k++)
            score = score + S.terms[k];
    }
    for (int w = ((N + 63) >> 6) + lane; w < words; w += 64)
        mask[w] = 0ull;
    if (lane == 0)
        *score_out = score;
}

// ---- I6, I7, I8: one wave per problem -------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_init_select(const InitProblemDev *__restrict__ problems)
{
    __shared__ InitLds S;
    const InitProblemDev &P = problems[blockIdx.x];
    const int lane = threadIdx.x, words = (P.n1 + 63) >> 6;
    InitCtl &ctl = *P.ctl;
    const int N = ctl.n;
    float SH = 0.f, SF = 0.f;
    int bh = -1, bf = -1;
    if (N >= 8) {
        for (int h = 0; h < P.n_hyp; h++) {
            const float s = P.scores_h[h];
            if (s > SH)
                SH = s, bh = h;
        }
        for (int h = 0; h < P.n_hyp; h++) {
            const float s = P.scores_f[h];
            if (s > SF)
                SF = s, bf = h;
        }
    }
    const float RH = fdiv(SH, SH + SF);
    const bool useH = (double)RH > 0.40;
    float H21[9], F21[9];
#pragma unroll
    for (int e = 0; e < 9; e++) {
        H21[e] = bh >= 0 ? P.mats[((size_t)bh * 2) * 9 + e] : 0.f;
        F21[e] = bf >= 0 ? P.mats[((size_t)bf * 2 + 1) * 9 + e] : 0.f;
    }
    const int sel = useH ? bh : bf;
    int n_inl = 0;
    if (sel >= 0) {
        const unsigned long long *mask = (useH ? P.masks_h : P.masks_f) + (size_t)sel * words;
        int c = 0;
        for (int w = lane; w < words; w += 64)
            c += __popcll(mask[w]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            c += __shfl_down(c, off, 64);
        n_inl = __shfl(c, 0, 64);
    }
    const float fx = P.K[0], fy = P.K[1], cx = P.K[2], cy = P.K[3];
    const double Kd[9] = {(double)fx, 0.0, (double)cx, 0.0, (double)fy, (double)cy, 0.0, 0.0, 1.0};
    float R[8][9], t[8][3];
#pragma unroll
    for (int m = 0; m < 8; m++) {
#pragma unroll
        for (int e = 0; e < 9; e++)
            R[m][e] = 0.f;
        t[m][0] = t[m][1] = t[m][2] = 0.f;
    }
    int n_motions = 0;
    if (sel >= 0 && useH) {
        const double Ki[9] = {1.0 / Kd[0], 0.0, -Kd[2] / Kd[0], 0.0, 1.0 / Kd[4], -Kd[5] / Kd[4], 0.0, 0.0, 1.0};
        float A[9];
        triple3(Ki, H21, Kd, A);
        double Ud[9], dd[3], Vd[9];
        svd3_wave(S, A, lane, true, Ud, dd, Vd);
        float U[9], Vt[9];
#pragma unroll
        for (int e = 0; e < 9; e++)
            U[e] = (float)Ud[e], Vt[e] = (float)Vd[e];
        const float s = (float)(det3d(U) * det3d(Vt));
        const float d1 = (float)dd[0], d2 = (float)dd[1], d3 = (float)dd[2];
        if (!((double)fdiv(d1, d2) < 1.00001 || (double)fdiv(d2, d3) < 1.00001)) {
            n_motions = 8;
            const float q1 = d1 * d1, q2 = d2 * d2, q3 = d3 * d3;
            const float aux1 = fsqrt(fdiv(q1 - q2, q1 - q3)), aux3 = fsqrt(fdiv(q2 - q3, q1 - q3));
            const float x1[4] = {aux1, aux1, -aux1, -aux1}, x3[4] = {aux3, -aux3, aux3, -aux3};
            const float root = fsqrt((q1 - q2) * (q2 - q3));
            const float aux_st = fdiv(root, (d1 + d3) * d2), ctheta = fdiv(q2 + d1 * d3, (d1 + d3) * d2);
            const float aux_sp = fdiv(root, (d1 - d3) * d2), cphi = fdiv(d1 * d3 - q2, (d1 - d3) * d2);
            const float sgn[4] = {1.f, -1.f, -1.f, 1.f};
            float sU[9];
#pragma unroll
            for (int e = 0; e < 9; e++)
                sU[e] = s * U[e];
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const int i = m & 3;
                const bool second = m >= 4;
                const float sn = sgn[i] > 0.f ? (second ? aux_sp : aux_st) : (second ? -aux_sp : -aux_st);
                float Rp[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (!second)
                    Rp[0] = ctheta, Rp[2] = -sn, Rp[4] = 1.f, Rp[6] = sn, Rp[8] = ctheta;
                else
                    Rp[0] = cphi, Rp[2] = sn, Rp[4] = -1.f, Rp[6] = sn, Rp[8] = -cphi;
                float UR[9];
                fmul3(sU, Rp, UR);
                fmul3(UR, Vt, R[m]);
                const float scale = second ? d1 + d3 : d1 - d3;
                const float tp0 = x1[i] * scale, tp1 = 0.f * scale, tp2 = (second ? x3[i] : -x3[i]) * scale;
                float tv[3];
#pragma unroll
                for (int r = 0; r < 3; r++)
                    tv[r] = fdot3(U[3 * r], tp0, U[3 * r + 1], tp1, U[3 * r + 2], tp2);
                const float nrm = (float)sqrt(((double)tv[0] * (double)tv[0] + (double)tv[1] * (double)tv[1]) + (double)tv[2] * (double)tv[2]);
#pragma unroll
                for (int r = 0; r < 3; r++)
                    t[m][r] = fdiv(tv[r], nrm);
            }
        }
    } else if (sel >= 0) {
        const double Kt[9] = {Kd[0], 0.0, 0.0, 0.0, Kd[4], 0.0, Kd[2], Kd[5], 1.0};
        float E[9];
        triple3(Kt, F21, Kd, E);
        double Ud[9], dd[3], Vd[9];
        svd3_wave(S, E, lane, false, Ud, dd, Vd);
        float U[9], Vt[9];
#pragma unroll
        for (int e = 0; e < 9; e++)
            U[e] = (float)Ud[e], Vt[e] = (float)Vd[e];
        n_motions = 4;
        const float tv[3] = {U[2], U[5], U[8]};
        const float nrm = (float)sqrt(((double)tv[0] * (double)tv[0] + (double)tv[1] * (double)tv[1]) + (double)tv[2] * (double)tv[2]);
        const float W[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f}, Wt[9] = {0.f, 1.f, 0.f, -1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
        float UW[9], R1[9], R2[9];
        fmul3(U, W, UW);
        fmul3(UW, Vt, R1);
        fmul3(U, Wt, UW);
        fmul3(UW, Vt, R2);
        const bool n1f = det3d(R1) < 0.0, n2f = det3d(R2) < 0.0;
#pragma unroll
        for (int e = 0; e < 9; e++) {
            const float a = n1f ? -R1[e] : R1[e], b = n2f ? -R2[e] : R2[e];
            R[0][e] = R[2][e] = a, R[1][e] = R[3][e] = b;
        }
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const float v = fdiv(tv[r], nrm);
            t[0][r] = t[1][r] = v, t[2][r] = t[3][r] = -v;
        }
    }
    if (lane == 0) {
        ctl.best_h = bh, ctl.best_f = bf, ctl.use_h = useH ? 1 : 0, ctl.n_motions = n_motions, ctl.n_inliers = n_inl;
#pragma unroll
        for (int m = 0; m < 8; m++) {
#pragma unroll
            for (int e = 0; e < 9; e++)
                ctl.R[m][e] = R[m][e];
            ctl.t[m][0] = t[m][0], ctl.t[m][1] = t[m][1], ctl.t[m][2] = t[m][2];
        }
        orbgpu_init_result *r = P.result;
        r->best_h = bh, r->best_f = bf, r->SH = SH, r->SF = SF, r->RH = RH, r->used_homography = useH ? 1 : 0;
        r->n_inliers = n_inl;
#pragma unroll
        for (int e = 0; e < 9; e++)
            r->H21[e] = H21[e], r->F21[e] = F21[e];
    }
}

// ---- I9 ---------------------------------------------------------------------------------------------------------------------
// the triangulation of a pair is null_vector4 (jacobi.h), shared with new_points.hip
// grid (8, problems), one wave per motion
__global__ __launch_bounds__(64) void k_init_checkrt(const InitProblemDev *__restrict__ problems)
{
    const InitProblemDev &P = problems[blockIdx.y];
    const int lane = threadIdx.x, mo = blockIdx.x, n1 = P.n1;
    InitCtl &ctl = *P.ctl;
    if (mo >= ctl.n_motions) {
        if (lane == 0)
            ctl.n_good[mo] = 0, ctl.cosp[mo] = 0.f;
        return;
    }
    const int N = ctl.n, words = (n1 + 63) >> 6;
    const unsigned long long *mask = ctl.use_h ? P.masks_h + (size_t)ctl.best_h * words : P.masks_f + (size_t)ctl.best_f * words;
    float R[9], t[3];
#pragma unroll
    for (int e = 0; e < 9; e++)
        R[e] = ctl.R[mo][e];
    t[0] = ctl.t[mo][0], t[1] = ctl.t[mo][1], t[2] = ctl.t[mo][2];
    const float fx = P.K[0], fy = P.K[1], cx = P.K[2], cy = P.K[3];
    const float Kf[9] = {fx, 0.f, cx, 0.f, fy, cy, 0.f, 0.f, 1.f};
    const float P1[3][4] = {{fx, 0.f, cx, 0.f}, {0.f, fy, cy, 0.f}, {0.f, 0.f, 1.f, 0.f}};
    float P2[3][4];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const float m0 = c < 3 ? R[c] : t[0], m1 = c < 3 ? R[3 + c] : t[1], m2 = c < 3 ? R[6 + c] : t[2];
            P2[r][c] = (Kf[3 * r] * m0 + Kf[3 * r + 1] * m1) + Kf[3 * r + 2] * m2;
        }
    float O2[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
        O2[i] = ((-R[i]) * t[0] + (-R[3 + i]) * t[1]) + (-R[6 + i]) * t[2];
    const float th2 = (float)(4.0 * (double)(P.sigma * P.sigma));
    float *p3d = P.p3d + (size_t)mo * n1 * 3;
    uint8_t *good = P.good + (size_t)mo * n1;
    float *cosv = P.cosv + (size_t)mo * n1;
    int n_good = 0;
    for (int base = 0; base < N; base += 64) {
        const int e = base + lane;
        bool pass = false;
        float cosp = 0.f, x = 0.f, y = 0.f, z = 0.f;
        if (e < N && ((mask[e >> 6] >> (e & 63)) & 1ull)) {
            const float4 q = P.pts[e];
            float Af[4][4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                Af[0][c] = q.x * P1[2][c] - P1[0][c];
                Af[1][c] = q.y * P1[2][c] - P1[1][c];
                Af[2][c] = q.z * P2[2][c] - P2[0][c];
                Af[3][c] = q.w * P2[2][c] - P2[1][c];
            }
            float x4[4];
            null_vector4(Af, x4);
            x = fdiv(x4[0], x4[3]), y = fdiv(x4[1], x4[3]), z = fdiv(x4[2], x4[3]);
            const bool finite = (x - x == 0.f) && (y - y == 0.f) && (z - z == 0.f);
            if (finite) {
                const float dist1 = (float)sqrt(((double)x * (double)x + (double)y * (double)y) + (double)z * (double)z);
                const float nx = x - O2[0], ny = y - O2[1], nz = z - O2[2];
                const float dist2 = (float)sqrt(((double)nx * (double)nx + (double)ny * (double)ny) + (double)nz * (double)nz);
                const double dot = ((double)x * (double)nx + (double)y * (double)ny) + (double)z * (double)nz;
                cosp = (float)(dot / (double)(dist1 * dist2));
                const bool low = (double)cosp < 0.99998;
                const float x2 = ((R[0] * x + R[1] * y) + R[2] * z) + t[0];
                const float y2 = ((R[3] * x + R[4] * y) + R[5] * z) + t[1];
                const float z2 = ((R[6] * x + R[7] * y) + R[8] * z) + t[2];
                pass = !(z <= 0.f && low) && !(z2 <= 0.f && low);
                const float iz1 = finv(z);
                const float im1x = (fx * x) * iz1 + cx, im1y = (fy * y) * iz1 + cy;
                const float e1 = (im1x - q.x) * (im1x - q.x) + (im1y - q.y) * (im1y - q.y);
                pass = pass && !(e1 > th2);
                const float iz2 = finv(z2);
                const float im2x = (fx * x2) * iz2 + cx, im2y = (fy * y2) * iz2 + cy;
                const float e2 = (im2x - q.z) * (im2x - q.z) + (im2y - q.w) * (im2y - q.w);
                pass = pass && !(e2 > th2);
            }
        }
        const unsigned long long word = __ballot(pass);
        if (pass) {
            const int i = P.first[e];
            p3d[3 * (size_t)i] = x, p3d[3 * (size_t)i + 1] = y, p3d[3 * (size_t)i + 2] = z;
            good[i] = (double)cosp < 0.99998 ? 1 : 0;
            cosv[n_good + __popcll(word & ((1ull << lane) - 1ull))] = cosp;
        }
        n_good += __popcll(word);
    }
    __syncthreads();
    // the element of rank min(50, nGood - 1): a radix select over the ordered keys
    float sel = 1.0f;
    if (n_good > 0) {
        int kk = min(50, n_good - 1);
        unsigned prefix = 0u;
        for (int bit = 31; bit >= 0; bit--) {
            const unsigned hi = bit == 31 ? 0u : (~0u << (bit + 1));
            int cnt0 = 0;
            for (int base = 0; base < n_good; base += 64) {
                const int j = base + lane;
                bool zero = false;
                if (j < n_good) {
                    const unsigned k = cos_key(cosv[j]);
                    zero = (k & hi) == prefix && !((k >> bit) & 1u);
                }
                cnt0 += __popcll(__ballot(zero));
            }
            if (kk >= cnt0)
                prefix |= 1u << bit, kk -= cnt0;
        }
        sel = key_cos(prefix);
    }
    if (lane == 0)
        ctl.n_good[mo] = n_good, ctl.cosp[mo] = sel;
}

// ---- the accept rules of ReconstructH / ReconstructF, one wave per problem ---------------------------------------------------
__global__ __launch_bounds__(64) void k_init_finish(const InitProblemDev *__restrict__ problems)
{
    const InitProblemDev &P = problems[blockIdx.x];
    const int lane = threadIdx.x, n1 = P.n1;
    const InitCtl &ctl = *P.ctl;
    const int Ni = ctl.n_inliers;
    int best = -1, second = 0, success = 0;
    if (ctl.n_motions == 8) {
        int best_good = 0;
        for (int i = 0; i < 8; i++) {
            const int g = ctl.n_good[i];
            if (g > best_good)
                second = best_good, best_good = g, best = i;
            else if (g > second)
                second = g;
        }
        success = best >= 0 && (double)second < 0.75 * (double)best_good && ctl.cosp[best] <= P.cos_limit_h &&
                  best_good > P.min_triangulated && (double)best_good > 0.9 * (double)Ni;
    } else if (ctl.n_motions == 4) {
        int max_good = 0;
        for (int i = 0; i < 4; i++)
            max_good = max(max_good, ctl.n_good[i]);
        const int n_min_good = max((int)(0.9 * (double)Ni), P.min_triangulated);
        for (int i = 0; i < 4; i++)
            second += (double)ctl.n_good[i] > 0.7 * (double)max_good ? 1 : 0;  // nsimilar
        for (int i = 3; i >= 0; i--)
            if (ctl.n_good[i] == max_good)
                best = i;
        success = !(max_good < n_min_good || second > 1) && ctl.cosp[best] <= P.cos_limit_f;
    }
    if (success) {
        const float *p3d = P.p3d + (size_t)best * n1 * 3;
        const uint8_t *good = P.good + (size_t)best * n1;
        for (int i = lane; i < n1; i += 64) {
            P.P3D[3 * (size_t)i] = p3d[3 * (size_t)i], P.P3D[3 * (size_t)i + 1] = p3d[3 * (size_t)i + 1];
            P.P3D[3 * (size_t)i + 2] = p3d[3 * (size_t)i + 2];
            P.triangulated[i] = good[i];
        }
    }
    if (lane < 12) {
        const float v = success ? (lane < 9 ? ctl.R[best][lane] : ctl.t[best][lane - 9]) : 0.f;
        if (lane < 9) {
            P.result->R21[lane] = v;
            if (P.R21)
                P.R21[lane] = v;
        } else {
            P.result->t21[lane - 9] = v;
            if (P.t21)
                P.t21[lane - 9] = v;
        }
    }
    if (lane == 0) {
        orbgpu_init_result *r = P.result;
        for (int i = 0; i < 8; i++)
            r->n_good[i] = ctl.n_good[i], r->cos_parallax[i] = ctl.cosp[i];
        r->best_motion = best, r->second_best_good = second, r->success = success, r->parallax_deg = 0.f;
    }
}

enum { PROBLEMS, PTS, PN, FIRST, MATS, P3DW, GOODW, COSV, CTL, H_IN, H_OUT, N_BUF };
struct InitWs : Staging<N_BUF> {
    std::vector<InitProblemDev> h_problems;  // source of an asynchronous upload: it outlives the call
    ~InitWs() { release(); }
};

// I10: the reference's parallax of a cosine
float parallax_of(float c) { return (float)((double)(acosf(c) * 180.0f) / 3.1415926535897932384626433832795); }

unsigned host_key(float c)
{
    uint32_t u;
    memcpy(&u, &c, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

float host_cos(unsigned k)
{
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float c;
    memcpy(&c, &u, 4);
    return c;
}

// the largest float c in [-1, 1] for which parallax_of(c) > mp (strict) or >= mp holds; NaN if none
float cos_limit(float mp, bool strict)
{
    auto holds = [&](float c) { return strict ? parallax_of(c) > mp : parallax_of(c) >= mp; };
    if (!holds(-1.0f))
        return std::nanf("");
    if (holds(1.0f))
        return 1.0f;
    unsigned lo = host_key(-1.0f), hi = host_key(1.0f);
    while (hi - lo > 1u) {
        const unsigned mid = lo + (hi - lo) / 2u;
        if (holds(host_cos(mid)))
            lo = mid;
        else
            hi = mid;
    }
    return host_cos(lo);
}

int check_common(const orbgpu_init_problem &p, int k)
{
    ORBGPU_REQUIRE(p.n1 >= 0 && p.n1 <= INIT_MAX_N && p.n2 >= 0 && p.n2 <= INIT_MAX_N, "problem %d: n1 or n2 outside [0, %d]", k,
                   INIT_MAX_N);
    ORBGPU_REQUIRE(p.n_hyp >= 0 && p.n_hyp <= INIT_MAX_HYP, "problem %d: n_hyp outside [0, %d]", k, INIT_MAX_HYP);
    ORBGPU_REQUIRE(p.sigma > 0.0f, "problem %d: sigma must be positive", k);
    ORBGPU_REQUIRE(p.min_triangulated >= 0, "problem %d: negative min_triangulated", k);
    ORBGPU_REQUIRE(p.n1 == 0 || (p.kp1 && p.matches12), "problem %d: null kp1 / matches12", k);
    ORBGPU_REQUIRE(p.n2 == 0 || p.kp2, "problem %d: null kp2", k);
    ORBGPU_REQUIRE(p.n_hyp == 0 || p.sets, "problem %d: null sets", k);
    return ORBGPU_OK;
}

int check_device_problem(const orbgpu_init_problem &p, int k)
{
    int rc = check_common(p, k);
    if (rc != ORBGPU_OK)
        return rc;
    ORBGPU_REQUIRE(p.result, "problem %d: null result", k);
    ORBGPU_REQUIRE(p.n1 == 0 || (p.P3D && p.triangulated), "problem %d: null P3D / triangulated", k);
    ORBGPU_REQUIRE(p.n_hyp == 0 || (p.scores_h && p.scores_f && (p.n1 == 0 || (p.masks_h && p.masks_f))),
                   "problem %d: null scores / masks", k);
    return ORBGPU_OK;
}

} // namespace
} // namespace orbgpu

using namespace orbgpu;

extern "C" int orbgpu_initializer_cos_limits(float min_parallax, float *limit_f, float *limit_h)
{
    ORBGPU_REQUIRE(limit_f && limit_h, "null argument");
    *limit_f = cos_limit(min_parallax, true), *limit_h = cos_limit(min_parallax, false);
    return ORBGPU_OK;
}

extern "C" int orbgpu_initializer_batch_device(int32_t n, const orbgpu_init_problem *problems, int32_t device_id, void *hip_stream)
{
    InitWs *wsp;
    int rc = batch_begin(n, problems, check_device_problem, device_id, wsp);
    if (rc != ORBGPU_OK || !wsp)
        return rc;
    InitWs &ws = *wsp;
    size_t rows = 0, hyps = 0;
    int max_hyp = 0;
    for (int k = 0; k < n; k++) {
        rows += (size_t)problems[k].n1;
        hyps += (size_t)problems[k].n_hyp;
        max_hyp = std::max(max_hyp, (int)problems[k].n_hyp);
    }
    const size_t r1 = std::max<size_t>(rows, 1), h1 = std::max<size_t>(hyps, 1);
    ws.reserve(PROBLEMS, sizeof(InitProblemDev) * (size_t)n);
    ws.reserve(PTS, sizeof(float4) * r1);
    ws.reserve(PN, sizeof(float4) * r1);
    ws.reserve(FIRST, sizeof(int32_t) * r1);
    ws.reserve(MATS, sizeof(float) * 18 * h1);
    ws.reserve(P3DW, sizeof(float) * 24 * r1);
    ws.reserve(GOODW, 8 * r1);
    ws.reserve(COSV, sizeof(float) * 8 * r1);
    ws.reserve(CTL, sizeof(InitCtl) * (size_t)n);
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    std::vector<InitProblemDev> &hp = ws.h_problems;
    const hipStream_t st = (hipStream_t)hip_stream;
    ORBGPU_HIP_TRY(hipStreamSynchronize(st));  // an earlier call's upload has left hp
    hp.resize((size_t)n);
    size_t ro = 0, ho = 0;
    for (int k = 0; k < n; k++) {
        const orbgpu_init_problem &p = problems[k];
        InitProblemDev &D = hp[k];
        memset(&D, 0, sizeof(D));
        D.kp1 = p.kp1, D.kp2 = p.kp2, D.matches12 = p.matches12, D.sets = p.sets;
        D.scores_h = p.scores_h, D.scores_f = p.scores_f;
        D.masks_h = reinterpret_cast<unsigned long long *>(p.masks_h);
        D.masks_f = reinterpret_cast<unsigned long long *>(p.masks_f);
        D.R21 = p.R21, D.t21 = p.t21, D.P3D = p.P3D, D.triangulated = p.triangulated, D.result = p.result;
        D.pts = ws.as<float4>(PTS) + ro, D.pn = ws.as<float4>(PN) + ro, D.first = ws.as<int32_t>(FIRST) + ro;
        D.mats = ws.as<float>(MATS) + 18 * ho;
        D.p3d = ws.as<float>(P3DW) + 24 * ro, D.good = ws.as<uint8_t>(GOODW) + 8 * ro, D.cosv = ws.as<float>(COSV) + 8 * ro;
        D.ctl = ws.as<InitCtl>(CTL) + k;
        ro += (size_t)p.n1, ho += (size_t)p.n_hyp;
        D.n1 = p.n1, D.n2 = p.n2, D.n_hyp = p.n_hyp, D.min_triangulated = p.min_triangulated;
        D.K[0] = p.fx, D.K[1] = p.fy, D.K[2] = p.cx, D.K[3] = p.cy, D.sigma = p.sigma;
        D.cos_limit_f = cos_limit(p.min_parallax, true), D.cos_limit_h = cos_limit(p.min_parallax, false);
    }
    ORBGPU_HIP_TRY(hipMemcpyAsync(ws.buf[PROBLEMS].p, hp.data(), sizeof(InitProblemDev) * (size_t)n, hipMemcpyHostToDevice, st));
    ORBGPU_HIP_TRY(hipMemsetAsync(ws.buf[P3DW].p, 0, sizeof(float) * 24 * r1, st));
    ORBGPU_HIP_TRY(hipMemsetAsync(ws.buf[GOODW].p, 0, 8 * r1, st));
    const InitProblemDev *dp = ws.as<InitProblemDev>(PROBLEMS);
    hipLaunchKernelGGL(k_init_prepare, dim3(n), dim3(64), 0, st, dp);
    ORBGPU_HIP_TRY(hipGetLastError());
    if (max_hyp > 0) {
        hipLaunchKernelGGL(k_init_hypotheses, dim3(max_hyp, 2, n), dim3(64), 0, st, dp);
        ORBGPU_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_init_select, dim3(n), dim3(64), 0, st, dp);
    ORBGPU_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_init_checkrt, dim3(8, n), dim3(64), 0, st, dp);
    ORBGPU_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_init_finish, dim3(n), dim3(64), 0, st, dp);
    ORBGPU_HIP_TRY(hipGetLastError());
    return ORBGPU_OK;
}

extern "C" int orbgpu_initializer_device(const orbgpu_init_problem *p, int32_t device_id, void *hip_stream)
{
    ORBGPU_REQUIRE(p, "null argument");
    return orbgpu_initializer_batch_device(1, p, device_id, hip_stream);
}

// The host flavours.  all: the per-hypothesis scores and masks come back as well.
static int init_host(const orbgpu_init_problem *p, float *scores_h, float *scores_f, uint64_t *masks_h, uint64_t *masks_f,
                     float *P3D, uint8_t *triangulated, bool all, orbgpu_init_result *result, int32_t device_id)
{
    ORBGPU_REQUIRE(p && result, "null argument");
    int rc = check_common(*p, 0);
    if (rc != ORBGPU_OK)
        return rc;
    const int n1 = p->n1, n2 = p->n2, H = p->n_hyp;
    // I1 on the host, to refuse a set index outside [0, N) before anything is launched
    int N = 0;
    for (int i = 0; i < n1; i++)
        if (p->matches12[i] >= 0 && p->matches12[i] < n2)
            N++;
    if (N >= 8)
        for (int h = 0; h < H; h++)
            for (int k = 0; k < 8; k++)
                ORBGPU_REQUIRE(p->sets[(size_t)h * 8 + k] >= 0 && p->sets[(size_t)h * 8 + k] < N, "set %d: index %d outside [0, %d)", h,
                               p->sets[(size_t)h * 8 + k], N);
    // one staging block each way
    const size_t words = (size_t)(n1 + 63) / 64;
    orbgpu_init_result r;
    HostPlan<N_BUF> plan;
    const auto i_k1 = plan.in(H_IN, p->kp1, n1, 2), i_k2 = plan.in(H_IN, p->kp2, n2, 2);
    const auto i_m = plan.in(H_IN, p->matches12, n1), i_s = plan.in(H_IN, p->sets, H, 8);
    const auto o_res = plan.out(H_OUT, &r, 1);
    const auto o_p = plan.out(H_OUT, P3D, n1, 3);
    const auto o_t = plan.out(H_OUT, triangulated, n1);
    const auto o_sh = plan.out(H_OUT, all ? scores_h : nullptr, H), o_sf = plan.out(H_OUT, all ? scores_f : nullptr, H);
    const auto o_mh = plan.out(H_OUT, all ? masks_h : nullptr, H, words), o_mf = plan.out(H_OUT, all ? masks_f : nullptr, H, words);
    InitWs *wsp;
    if ((rc = host_begin(device_id, plan, wsp)) != ORBGPU_OK)
        return rc;
    InitWs &ws = *wsp;
    InitWs::FinishOnError on_error{ws};
    plan.upload(ws);
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    ORBGPU_HIP_TRY(hipMemsetAsync(ws.as<char>(H_OUT), 0, plan.bytes(H_OUT), ws.stream));
    orbgpu_init_problem d = *p;
    d.kp1 = ws.at(i_k1), d.kp2 = ws.at(i_k2), d.matches12 = ws.at(i_m);
    d.sets = ws.at(i_s);
    d.result = ws.at(o_res), d.P3D = ws.at(o_p), d.triangulated = ws.at(o_t);
    d.scores_h = ws.at(o_sh), d.scores_f = ws.at(o_sf);
    d.masks_h = ws.at(o_mh), d.masks_f = ws.at(o_mf);
    d.R21 = d.t21 = nullptr;
    if ((rc = orbgpu_initializer_batch_device(1, &d, device_id, ws.stream)) != ORBGPU_OK)
        return rc;
    plan.download(ws);
    if ((rc = ws.finish()) != ORBGPU_OK)
        return rc;
    if (r.best_motion >= 0 && r.n_good[r.best_motion] > 0)
        r.parallax_deg = parallax_of(r.cos_parallax[r.best_motion]);
    *result = r;
    return ORBGPU_OK;
}

extern "C" int orbgpu_initializer(const orbgpu_init_problem *p, float *P3D, uint8_t *triangulated, orbgpu_init_result *result,
                                  int32_t device_id)
{
    return init_host(p, nullptr, nullptr, nullptr, nullptr, P3D, triangulated, false, result, device_id);
}

extern "C" int orbgpu_initializer_all(const orbgpu_init_problem *p, float *scores_h, float *scores_f, uint64_t *masks_h,
                                      uint64_t *masks_f, float *P3D, uint8_t *triangulated, orbgpu_init_result *result,
                                      int32_t device_id)
{
    return init_host(p, scores_h, scores_f, masks_h, masks_f, P3D, triangulated, true, result, device_id);
}

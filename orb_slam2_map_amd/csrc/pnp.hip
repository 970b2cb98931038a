// PnPsolver (PnPsolver.cc) on the device: EPnP on a minimal set per hypothesis, N reprojections per hypothesis, the
// reference's sequential acceptance rule with its Refine replayed over the counts.  The definition (P1-P10, "OpenCV
// boundary unpinned") is in include/orbgpu.h and tests/pnp_model.py; the arithmetic below is the model's operation for
// operation in FP64 (-ffp-contract=off): only +, -, *, /, sqrt and comparisons, no libm.
//
// One wave works on one EPnP problem (k_pnp_hypotheses: the minimal set of a hypothesis; k_pnp_select: the inlier set of
// a record).  Sums over the points of a set are wave sums (lane l adds the terms l, l + 64, ... from +0.0, then the 64
// partial sums are folded by halves); the small dense steps run in every lane on the same values, with the matrices of
// the Jacobi in LDS and the independent row / column updates of a rotation spread over the lanes.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "carve.h"
#include "common.h"
#include "jacobi.h"
#include "ransac_host.h"
#include "staging.h"

namespace orbgpu {

constexpr int PNP_MAX_N1 = 16384, PNP_MAX_HYP = 4096, PNP_MIN_SET_LO = 4, PNP_MIN_SET_HI = 64;
constexpr int PNP_JACOBI_SWEEPS = 30;
constexpr double PNP_CC_REL = 1e-6, PNP_LS_REL = 1e-12;
constexpr int LD = 12;  // row stride of the LDS matrices (jacobi.h)

struct PnpCtl {
    int32_t n, min_inliers, max_its, n_use;
};

struct PnpProblemDev {
    const uint8_t *valid;
    const float *Xw, *kp;
    const int32_t *octave, *sets;
    int32_t *counts;
    float *Tcw;
    unsigned long long *masks, *refined_mask;
    int32_t *indices;
    orbgpu_pnp_result *result;
    float4 *rec;    // [n1]: (Xw, maxError or NaN for a row that is not kept), by i
    float2 *uv;     // [n1]
    int32_t *map;   // [n1] compacted -> i
    int32_t *list;  // [n1] the rows of the set being refined
    PnpCtl *ctl;
    int32_t n1, n_hyp, nlevels, min_set, start_iteration, best_so_far, n_iterations;
    float K[4];  // fx fy cx cy
    float max_error[ORBGPU_MAX_LEVELS];
};

__device__ inline int pnp_row_kind(const PnpProblemDev &P, int i)
{
    if (i >= P.n1 || !P.valid[i])
        return 0;
    const int o = P.octave[i];
    return (o < 0 || o >= P.nlevels) ? 2 : 1;
}

// One wave per problem: P1 / P2.  A record for EVERY row i < n1 (maxError = NaN for a row that is not kept, so it can
// never be an inlier), the compacted -> i map, N and n_bad_index.
__global__ __launch_bounds__(64) void k_pnp_prepare(const PnpProblemDev *__restrict__ problems)
{
    const PnpProblemDev &P = problems[blockIdx.x];
    const int lane = threadIdx.x, n1 = P.n1;
    int at = 0, nbad = 0;
    for (int base = 0; base < n1; base += 64) {
        const int i = base + lane;
        const int kind = pnp_row_kind(P, i);
        const unsigned long long m1 = __ballot(kind == 1), m2 = __ballot(kind == 2);
        if (i < n1) {
            float4 a = make_float4(0.f, 0.f, 0.f, __int_as_float(0x7fc00000));
            float2 b = make_float2(0.f, 0.f);
            if (kind == 1) {
                const int e = at + __popcll(m1 & ((1ull << lane) - 1ull));
                P.map[e] = i;
                if (P.indices)
                    P.indices[e] = i;
                a = make_float4(P.Xw[3 * (size_t)i], P.Xw[3 * (size_t)i + 1], P.Xw[3 * (size_t)i + 2], P.max_error[P.octave[i]]);
                b = make_float2(P.kp[2 * (size_t)i], P.kp[2 * (size_t)i + 1]);
            }
            P.rec[i] = a;
            P.uv[i] = b;
        }
        at += __popcll(m1);
        nbad += __popcll(m2);
    }
    if (lane == 0) {
        P.ctl->n = at;
        orbgpu_pnp_result *r = P.result;
        r->n = at, r->n_bad_index = nbad, r->n_bad_set = 0;
    }
}

// ---- wave helpers --------------------------------------------------------------------------------------------------------
__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = v + __shfl_down(v, off, 64);
    return __shfl(v, 0, 64);
}

struct EpnpLds {
    double A[LD * LD], V[LD * LD], Ut[LD * LD], w[LD];
    double vs[4 * 12];   // v[0] (smallest eigenvalue) ... v[3]
    double L[6 * 10], rho[6], g[8], n2[LD];
};

struct PnpPoint {
    double x[3], u, v;
};

__device__ inline PnpPoint pnp_point(const PnpProblemDev &P, int i)
{
    const float4 a = P.rec[i];
    const float2 b = P.uv[i];
    PnpPoint p;
    p.x[0] = (double)a.x, p.x[1] = (double)a.y, p.x[2] = (double)a.z, p.u = (double)b.x, p.v = (double)b.y;
    return p;
}

__device__ inline double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

struct EpnpFrame {
    double c0[3], ci[3][3];  // centroid; rows of the inverse of CC
};

__device__ inline void alphas_of(const EpnpFrame &F, const PnpPoint &p, double al[4])
{
    const double d[3] = {p.x[0] - F.c0[0], p.x[1] - F.c0[1], p.x[2] - F.c0[2]};
#pragma unroll
    for (int j = 0; j < 3; j++)
        al[1 + j] = (F.ci[j][0] * d[0] + F.ci[j][1] * d[1]) + F.ci[j][2] * d[2];
    al[0] = ((1.0 - al[1]) - al[2]) - al[3];
}

// x minimising |L[:, cols] x - rho| with the least norm, through the Jacobi of the normal matrix (P5)
template <int KK> __device__ void lstsq_wave(EpnpLds &S, const int (&cols)[KK], int lane, double x[KK])
{
    __syncthreads();
    if (lane < KK * KK) {
        const int a = lane / KK, b = lane % KK;
        double s = 0.0;
        for (int i = 0; i < 6; i++)
            s = s + S.L[i * 10 + cols[a]] * S.L[i * 10 + cols[b]];
        S.A[a * LD + b] = s;
    } else if (lane >= 32 && lane < 32 + KK) {
        const int a = lane - 32;
        double s = 0.0;
        for (int i = 0; i < 6; i++)
            s = s + S.L[i * 10 + cols[a]] * S.rho[i];
        S.g[a] = s;
    }
    __syncthreads();
    jacobi_wave<LD, PNP_JACOBI_SWEEPS>(S, KK, lane);
    double wmax = S.A[0];
#pragma unroll
    for (int i = 1; i < KK; i++) {
        const double wi = S.A[i * LD + i];
        if (wi > wmax)
            wmax = wi;
    }
    const double thr = PNP_LS_REL * wmax;
#pragma unroll
    for (int a = 0; a < KK; a++)
        x[a] = 0.0;
#pragma unroll
    for (int i = 0; i < KK; i++) {
        double pr = 0.0;
#pragma unroll
        for (int a = 0; a < KK; a++)
            pr = pr + S.V[a * LD + i] * S.g[a];
        const double wi = S.A[i * LD + i];
        const double coef = wi <= thr ? 0.0 : pr / wi;
#pragma unroll
        for (int a = 0; a < KK; a++)
            x[a] = x[a] + coef * S.V[a * LD + i];
    }
}

// Householder QR of the 6 x 4 system; a zero pivot column gives x = 0
__device__ inline void qr_solve(double (&A)[6][4], double (&b)[6], double (&x)[4])
{
    double A1[4], A2[4];
    bool sing = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        double eta = fabs(A[k][k]);
#pragma unroll
        for (int i = k + 1; i < 6; i++) {
            const double elt = fabs(A[i][k]);
            if (eta < elt)
                eta = elt;
        }
        sing = sing || eta == 0.0;
        const double inv_eta = 1.0 / eta;
        double sum = 0.0;
#pragma unroll
        for (int i = k; i < 6; i++) {
            A[i][k] = A[i][k] * inv_eta;
            sum = sum + A[i][k] * A[i][k];
        }
        double sigma = sqrt(sum);
        if (A[k][k] < 0.0)
            sigma = -sigma;
        A[k][k] = A[k][k] + sigma;
        A1[k] = sigma * A[k][k];
        A2[k] = -eta * sigma;
#pragma unroll
        for (int j = k + 1; j < 4; j++) {
            double s2 = 0.0;
#pragma unroll
            for (int i = k; i < 6; i++)
                s2 = s2 + A[i][k] * A[i][j];
            const double tau = s2 / A1[k];
#pragma unroll
            for (int i = k; i < 6; i++)
                A[i][j] = A[i][j] - tau * A[i][k];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double tau = 0.0;
#pragma unroll
        for (int i = j; i < 6; i++)
            tau = tau + A[i][j] * b[i];
        tau = tau / A1[j];
#pragma unroll
        for (int i = j; i < 6; i++)
            b[i] = b[i] - tau * A[i][j];
    }
    x[3] = b[3] / A2[3];
#pragma unroll
    for (int i = 2; i >= 0; i--) {
        double sum = 0.0;
#pragma unroll
        for (int j = i + 1; j < 4; j++)
            sum = sum + A[i][j] * x[j];
        x[i] = (b[i] - sum) / A2[i];
    }
    if (sing)
        x[0] = x[1] = x[2] = x[3] = 0.0;
}

__device__ void gauss_newton(const EpnpLds &S, double (&be)[4])
{
    for (int it = 0; it < 5; it++) {
        double A[6][4], r[6], x[4];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const double *l = S.L + i * 10;
            A[i][0] = (((2.0 * l[0]) * be[0] + l[1] * be[1]) + l[3] * be[2]) + l[6] * be[3];
            A[i][1] = ((l[1] * be[0] + (2.0 * l[2]) * be[1]) + l[4] * be[2]) + l[7] * be[3];
            A[i][2] = ((l[3] * be[0] + l[4] * be[1]) + (2.0 * l[5]) * be[2]) + l[8] * be[3];
            A[i][3] = ((l[6] * be[0] + l[7] * be[1]) + l[8] * be[2]) + (2.0 * l[9]) * be[3];
            double s = (l[0] * be[0]) * be[0];
            s = s + (l[1] * be[0]) * be[1];
            s = s + (l[2] * be[1]) * be[1];
            s = s + (l[3] * be[0]) * be[2];
            s = s + (l[4] * be[1]) * be[2];
            s = s + (l[5] * be[2]) * be[2];
            s = s + (l[6] * be[0]) * be[3];
            s = s + (l[7] * be[1]) * be[3];
            s = s + (l[8] * be[2]) * be[3];
            s = s + (l[9] * be[3]) * be[3];
            r[i] = S.rho[i] - s;
        }
        qr_solve(A, r, x);
#pragma unroll
        for (int i = 0; i < 4; i++)
            be[i] = be[i] + x[i];
    }
}

// compute_R_and_t: the pose of one beta vector and its mean reprojection error
__device__ double pose_from_betas(const PnpProblemDev &P, const int32_t *list, int n, EpnpLds &S, const EpnpFrame &F,
                                  const double (&be)[4], int lane, double (&R)[9], double (&t)[3])
{
    const double fu = (double)P.K[0], fv = (double)P.K[1], uc = (double)P.K[2], vc = (double)P.K[3];
    double ccs[12];
#pragma unroll
    for (int e = 0; e < 12; e++) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 4; i++)
            s = s + be[i] * S.vs[i * 12 + e];
        ccs[e] = s;
    }
    {
        double al[4];
        alphas_of(F, pnp_point(P, list[0]), al);
        const double z = ((al[0] * ccs[2] + al[1] * ccs[5]) + al[2] * ccs[8]) + al[3] * ccs[11];
        if (z < 0.0) {
#pragma unroll
            for (int e = 0; e < 12; e++)
                ccs[e] = -ccs[e];
        }
    }
    double pc0[3] = {0.0, 0.0, 0.0};
    for (int k = lane; k < n; k += 64) {
        double al[4];
        alphas_of(F, pnp_point(P, list[k]), al);
#pragma unroll
        for (int j = 0; j < 3; j++)
            pc0[j] = pc0[j] + (((al[0] * ccs[j] + al[1] * ccs[3 + j]) + al[2] * ccs[6 + j]) + al[3] * ccs[9 + j]);
    }
#pragma unroll
    for (int j = 0; j < 3; j++)
        pc0[j] = wave_sum(pc0[j]) / (double)n;
    double abt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = lane; k < n; k += 64) {
        const PnpPoint p = pnp_point(P, list[k]);
        double al[4];
        alphas_of(F, p, al);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double pc = ((al[0] * ccs[j] + al[1] * ccs[3 + j]) + al[2] * ccs[6 + j]) + al[3] * ccs[9 + j];
            const double dc = pc - pc0[j];
#pragma unroll
            for (int m = 0; m < 3; m++)
                abt[3 * j + m] = abt[3 * j + m] + dc * (p.x[m] - F.c0[m]);
        }
    }
#pragma unroll
    for (int e = 0; e < 9; e++)
        abt[e] = wave_sum(abt[e]);
    // R = U V' of abt = U S V' through the Jacobi of abt' abt: u_k = abt v_k / |abt v_k|
    __syncthreads();
    if (lane < 9) {
        const int a = lane / 3, b = lane % 3;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 3; j++)
            s = s + abt[3 * j + a] * abt[3 * j + b];
        S.A[a * LD + b] = s;
    }
    __syncthreads();
    jacobi_wave<LD, PNP_JACOBI_SWEEPS>(S, 3, lane);
#pragma unroll
    for (int e = 0; e < 9; e++)
        R[e] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double v0 = S.V[k], v1 = S.V[LD + k], v2 = S.V[2 * LD + k];
        double u[3];
#pragma unroll
        for (int i = 0; i < 3; i++)
            u[i] = (abt[3 * i] * v0 + abt[3 * i + 1] * v1) + abt[3 * i + 2] * v2;
        const double nrm = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
        const double vk[3] = {v0, v1, v2};
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double ui = u[i] / nrm;
#pragma unroll
            for (int j = 0; j < 3; j++)
                R[3 * i + j] = R[3 * i + j] + ui * vk[j];
        }
    }
    double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6];
    det = det + R[2] * R[3] * R[7];
    det = det - R[2] * R[4] * R[6];
    det = det - R[1] * R[3] * R[8];
    det = det - R[0] * R[5] * R[7];
    if (det < 0.0)
        R[6] = -R[6], R[7] = -R[7], R[8] = -R[8];
#pragma unroll
    for (int i = 0; i < 3; i++)
        t[i] = pc0[i] - dot3(R + 3 * i, F.c0);
    double err = 0.0;
    for (int k = lane; k < n; k += 64) {
        const PnpPoint p = pnp_point(P, list[k]);
        const double Xc = dot3(R, p.x) + t[0], Yc = dot3(R + 3, p.x) + t[1];
        const double iz = 1.0 / (dot3(R + 6, p.x) + t[2]);
        const double du = p.u - (uc + (fu * Xc) * iz), dv = p.v - (vc + (fv * Yc) * iz);
        err = err + sqrt(du * du + dv * dv);
    }
    return wave_sum(err) / (double)n;
}

// compute_pose (P5) over the rows list[0 .. n); every lane returns the same R, t
__device__ void epnp_wave(const PnpProblemDev &P, const int32_t *list, int n, EpnpLds &S, int lane, double (&Rb)[9], double (&tb)[3])
{
    const double fu = (double)P.K[0], fv = (double)P.K[1], uc = (double)P.K[2], vc = (double)P.K[3];
    EpnpFrame F;
    {
        double c[3] = {0.0, 0.0, 0.0};
        for (int k = lane; k < n; k += 64) {
            const PnpPoint p = pnp_point(P, list[k]);
#pragma unroll
            for (int j = 0; j < 3; j++)
                c[j] = c[j] + p.x[j];
        }
#pragma unroll
        for (int j = 0; j < 3; j++)
            F.c0[j] = wave_sum(c[j]) / (double)n;
    }
    {
        double c[6] = {0, 0, 0, 0, 0, 0};  // 00 01 02 11 12 22
        for (int k = lane; k < n; k += 64) {
            const PnpPoint p = pnp_point(P, list[k]);
            const double d[3] = {p.x[0] - F.c0[0], p.x[1] - F.c0[1], p.x[2] - F.c0[2]};
            c[0] = c[0] + d[0] * d[0], c[1] = c[1] + d[0] * d[1], c[2] = c[2] + d[0] * d[2];
            c[3] = c[3] + d[1] * d[1], c[4] = c[4] + d[1] * d[2], c[5] = c[5] + d[2] * d[2];
        }
#pragma unroll
        for (int e = 0; e < 6; e++)
            c[e] = wave_sum(c[e]);
        __syncthreads();
        if (lane == 0) {
            S.A[0] = c[0], S.A[1] = S.A[LD] = c[1], S.A[2] = S.A[2 * LD] = c[2];
            S.A[LD + 1] = c[3], S.A[LD + 2] = S.A[2 * LD + 1] = c[4], S.A[2 * LD + 2] = c[5];
        }
        __syncthreads();
    }
    sorted_eig_wave<LD, PNP_JACOBI_SWEEPS>(S, 3, lane);
    double cws[4][3];
    {
        double kk[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double w = S.w[i];
            kk[i] = sqrt((w < 0.0 ? 0.0 : w) / (double)n);
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double inv_k = kk[i] <= PNP_CC_REL * kk[0] ? 0.0 : 1.0 / kk[i];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double u = S.Ut[i * LD + j];
                F.ci[i][j] = inv_k * u;
                cws[1 + i][j] = F.c0[j] + kk[i] * u;
            }
        }
#pragma unroll
        for (int j = 0; j < 3; j++)
            cws[0][j] = F.c0[j];
    }
    // M'M: per point two rows of M; the upper triangle's 78 sums
    {
        double acc[78];
#pragma unroll
        for (int e = 0; e < 78; e++)
            acc[e] = 0.0;
        for (int k = lane; k < n; k += 64) {
            const PnpPoint p = pnp_point(P, list[k]);
            double al[4], m1[12], m2[12];
            alphas_of(F, p, al);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                m1[3 * i] = al[i] * fu, m1[3 * i + 1] = 0.0, m1[3 * i + 2] = al[i] * (uc - p.u);
                m2[3 * i] = 0.0, m2[3 * i + 1] = al[i] * fv, m2[3 * i + 2] = al[i] * (vc - p.v);
            }
            int e = 0;
#pragma unroll
            for (int r = 0; r < 12; r++)
#pragma unroll
                for (int c = r; c < 12; c++, e++)
                    acc[e] = acc[e] + (m1[r] * m1[c] + m2[r] * m2[c]);
        }
        __syncthreads();
        int e = 0;
#pragma unroll
        for (int r = 0; r < 12; r++)
#pragma unroll
            for (int c = r; c < 12; c++, e++) {
                const double s = wave_sum(acc[e]);
                if (lane == 0)
                    S.A[r * LD + c] = S.A[c * LD + r] = s;
            }
        __syncthreads();
    }
    sorted_eig_wave<LD, PNP_JACOBI_SWEEPS>(S, 12, lane);
    if (lane < 48)
        S.vs[lane] = S.Ut[(11 - lane / 12) * LD + lane % 12];
    __syncthreads();
    // the canonical basis of the structurally singular part (k = 12 - 2 n vectors)
    const int kn = max(0, 12 - 2 * n);
    if (kn > 0) {
        if (lane < 12) {
            for (int r = 0; r < 12; r++) {
                double s = 0.0;
                for (int j = 0; j < kn; j++)
                    s = s + S.vs[j * 12 + r] * S.vs[j * 12 + lane];
                S.A[r * LD + lane] = s;
            }
        }
        __syncthreads();
        for (int st = 0; st < kn; st++) {
            if (lane < 12) {
                double s = 0.0;
                for (int r = 0; r < 12; r++)
                    s = s + S.A[r * LD + lane] * S.A[r * LD + lane];
                S.n2[lane] = s;
            }
            __syncthreads();
            int piv = 0;
            double best = S.n2[0];
            for (int c = 1; c < 12; c++)
                if (S.n2[c] > best)
                    best = S.n2[c], piv = c;
            const double nrm = sqrt(best);
            double b[12];
            double big = 0.0, lead = 0.0;
#pragma unroll
            for (int r = 0; r < 12; r++) {
                b[r] = S.A[r * LD + piv] / nrm;
                if (r == 0 || fabs(b[r]) > big)
                    big = fabs(b[r]), lead = b[r];
            }
            if (lead < 0.0) {
#pragma unroll
                for (int r = 0; r < 12; r++)
                    b[r] = -b[r];
            }
            __syncthreads();
            if (lane < 12) {
                double d = 0.0;
#pragma unroll
                for (int r = 0; r < 12; r++)
                    d = d + b[r] * S.A[r * LD + lane];
#pragma unroll
                for (int r = 0; r < 12; r++)
                    S.A[r * LD + lane] = S.A[r * LD + lane] - d * b[r];
            } else if (lane == 32) {
#pragma unroll
                for (int r = 0; r < 12; r++)
                    S.vs[st * 12 + r] = b[r];
            }
            __syncthreads();
        }
    }
    // L (6 x 10) and rho
    if (lane < 6) {
        const int a = lane < 3 ? 0 : (lane < 5 ? 1 : 2), b = lane < 3 ? lane + 1 : (lane < 5 ? lane - 1 : 3);
        double dv[4][3];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                dv[i][j] = S.vs[i * 12 + 3 * a + j] - S.vs[i * 12 + 3 * b + j];
        double *row = S.L + 10 * lane;
        row[0] = dot3(dv[0], dv[0]);
        row[1] = 2.0 * dot3(dv[0], dv[1]);
        row[2] = dot3(dv[1], dv[1]);
        row[3] = 2.0 * dot3(dv[0], dv[2]);
        row[4] = 2.0 * dot3(dv[1], dv[2]);
        row[5] = dot3(dv[2], dv[2]);
        row[6] = 2.0 * dot3(dv[0], dv[3]);
        row[7] = 2.0 * dot3(dv[1], dv[3]);
        row[8] = 2.0 * dot3(dv[2], dv[3]);
        row[9] = dot3(dv[3], dv[3]);
        double dd[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double ca = cws[0][j], cb = cws[1][j];  // selected without dynamic indexing
            ca = a == 1 ? cws[1][j] : (a == 2 ? cws[2][j] : ca);
            cb = b == 2 ? cws[2][j] : (b == 3 ? cws[3][j] : cb);
            dd[j] = ca - cb;
        }
        S.rho[lane] = dot3(dd, dd);
    }
    __syncthreads();
    double best_err = 0.0;
#pragma unroll 1
    for (int kind = 1; kind <= 3; kind++) {
        double be[4] = {0.0, 0.0, 0.0, 0.0};
        if (kind == 1) {
            const int cols[4] = {0, 1, 3, 6};
            double x[4];
            lstsq_wave<4>(S, cols, lane, x);
            const bool neg = x[0] < 0.0;
            be[0] = neg ? sqrt(-x[0]) : sqrt(x[0]);
#pragma unroll
            for (int i = 1; i < 4; i++)
                be[i] = (neg ? -x[i] : x[i]) / be[0];
        } else {
            double x[5] = {0, 0, 0, 0, 0};
            if (kind == 2) {
                const int cols[3] = {0, 1, 2};
                double x3[3];
                lstsq_wave<3>(S, cols, lane, x3);
                x[0] = x3[0], x[1] = x3[1], x[2] = x3[2];
            } else {
                const int cols[5] = {0, 1, 2, 3, 4};
                lstsq_wave<5>(S, cols, lane, x);
            }
            const bool neg = x[0] < 0.0;
            double b0 = neg ? sqrt(-x[0]) : sqrt(x[0]);
            const double b1 = neg ? (x[2] < 0.0 ? sqrt(-x[2]) : 0.0) : (x[2] > 0.0 ? sqrt(x[2]) : 0.0);
            if (x[1] < 0.0)
                b0 = -b0;
            be[0] = b0, be[1] = b1;
            if (kind == 3)
                be[2] = x[3] / b0;
        }
        gauss_newton(S, be);
        double R[9], t[3];
        const double err = pose_from_betas(P, list, n, S, F, be, lane, R, t);
        if (kind == 1 || err < best_err) {
            best_err = err;
#pragma unroll
            for (int e = 0; e < 9; e++)
                Rb[e] = R[e];
#pragma unroll
            for (int e = 0; e < 3; e++)
                tb[e] = t[e];
        }
    }
}

// P6 for row i of the records
__device__ inline bool pnp_inlier(const PnpProblemDev &P, const double (&R)[9], const double (&t)[3], int i)
{
    const float4 a = P.rec[i];
    const float2 b = P.uv[i];
    const double x = (double)a.x, y = (double)a.y, z = (double)a.z;
    const float Xc = (float)(((R[0] * x + R[1] * y) + R[2] * z) + t[0]);
    const float Yc = (float)(((R[3] * x + R[4] * y) + R[5] * z) + t[1]);
    const float invZc = (float)(1.0 / (((R[6] * x + R[7] * y) + R[8] * z) + t[2]));
    const double ue = (double)P.K[2] + ((double)P.K[0] * (double)Xc) * (double)invZc;
    const double ve = (double)P.K[3] + ((double)P.K[1] * (double)Yc) * (double)invZc;
    const float distX = (float)((double)b.x - ue), distY = (float)((double)b.y - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < a.w;
}

// the inliers of a pose over all rows: mask words out, returns the count
__device__ int pnp_check_inliers(const PnpProblemDev &P, const double (&R)[9], const double (&t)[3], int lane,
                                 unsigned long long *mask)
{
    int count = 0;
    for (int base = 0; base < P.n1; base += 64) {
        const int i = base + lane;
        const bool inl = i < P.n1 && pnp_inlier(P, R, t, i);
        const unsigned long long word = __ballot(inl);
        if (lane == 0)
            mask[base >> 6] = word;
        count += __popcll(word);
    }
    return count;
}

__device__ inline void pnp_write_tcw(float *T, const double (&R)[9], const double (&t)[3], int lane)
{
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++)
                T[4 * i + j] = (float)R[3 * i + j];
            T[4 * i + 3] = (float)t[i];
        }
        T[12] = T[13] = T[14] = 0.0f, T[15] = 1.0f;
    }
}

// grid (max n_hyp, problems), one wave per hypothesis
__global__ __launch_bounds__(64) void k_pnp_hypotheses(const PnpProblemDev *__restrict__ problems)
{
    __shared__ EpnpLds S;
    __shared__ int32_t list[PNP_MIN_SET_HI];
    const PnpProblemDev &P = problems[blockIdx.y];
    const int lane = threadIdx.x, h = blockIdx.x;
    if (h >= P.n_hyp)
        return;
    const int N = P.ctl->n, n_use = P.ctl->n_use, n1 = P.n1, ms = P.min_set;
    if (h >= n_use) {
        if (lane == 0)
            P.counts[h] = 0;
        return;
    }
    const int words = (n1 + 63) >> 6;
    int e = lane < ms ? P.sets[(size_t)h * ms + lane] : 0;
    const bool bad = __ballot(e < 0 || e >= N) != 0ull || N == 0;
    if (bad) {  // never read through
        if (lane == 0) {
            P.counts[h] = 0;
            atomicAdd(&P.result->n_bad_set, 1);
        }
        if (lane < 16)
            P.Tcw[16 * (size_t)h + lane] = __int_as_float(0x7fc00000);
        for (int w = lane; w < words; w += 64)
            P.masks[(size_t)h * words + w] = 0ull;
        return;
    }
    if (lane < ms)
        list[lane] = P.map[e];
    __syncthreads();
    double R[9], t[3];
    epnp_wave(P, list, ms, S, lane, R, t);
    pnp_write_tcw(P.Tcw + 16 * (size_t)h, R, t, lane);
    const int count = pnp_check_inliers(P, R, t, lane, P.masks + (size_t)h * words);
    if (lane == 0)
        P.counts[h] = count;
}

// P7 / P8, one wave per problem: the reference's loop over the counts, a Refine per record
__global__ __launch_bounds__(64) void k_pnp_select(const PnpProblemDev *__restrict__ problems)
{
    __shared__ EpnpLds S;
    const PnpProblemDev &P = problems[blockIdx.x];
    const int lane = threadIdx.x, n1 = P.n1, words = (n1 + 63) >> 6;
    const PnpCtl c = *P.ctl;
    orbgpu_pnp_result *r = P.result;
    int it = P.start_iteration, best = P.best_so_far, best_it = -1, accepted = -1, n_inl = 0, no_more = 0;
    if (c.n < c.min_inliers) {
        no_more = 1;
    } else {
        int cur = 0;
        while ((it < c.max_its || cur < P.n_iterations) && it < c.n_use) {
            cur++;
            const int h = it++;
            const int cnt = P.counts[h];
            if (cnt >= c.min_inliers && cnt > best) {
                best = cnt, best_it = h;
                // Refine: EPnP over the record's inliers in index order, then P6
                int m = 0;
                for (int base = 0; base < n1; base += 64) {
                    const unsigned long long word = P.masks[(size_t)h * words + (base >> 6)];
                    if ((word >> lane) & 1ull)
                        P.list[m + __popcll(word & ((1ull << lane) - 1ull))] = base + lane;
                    m += __popcll(word);
                }
                __syncthreads();
                double R[9], t[3];
                epnp_wave(P, P.list, m, S, lane, R, t);
                const int rc = pnp_check_inliers(P, R, t, lane, P.refined_mask);
                __syncthreads();
                if (rc > c.min_inliers) {
                    accepted = h, n_inl = rc;
                    pnp_write_tcw(r->Tcw, R, t, lane);
                    break;
                }
            }
        }
        if (accepted < 0 && !(it < c.max_its || cur < P.n_iterations))
            no_more = 1;
    }
    if (accepted < 0) {  // the fallback of a finished search: the best record's own pose and mask; zeros otherwise
        const bool fb = no_more && best_it >= 0 && best >= c.min_inliers;
        if (fb)
            n_inl = best;
        if (lane < 16)
            r->Tcw[lane] = fb ? P.Tcw[16 * (size_t)best_it + lane] : 0.0f;
        for (int w = lane; w < words; w += 64)
            P.refined_mask[w] = fb ? P.masks[(size_t)best_it * words + w] : 0ull;
    }
    if (lane == 0) {
        r->min_inliers = c.min_inliers, r->max_its = c.max_its, r->pad_ = 0;
        r->accepted = accepted, r->n_inliers = n_inl, r->best_inliers = best, r->best_iteration = best_it;
        r->iterations = it, r->no_more = no_more;
    }
}

enum { PROBLEMS, REC, UV, MAP, LIST, CTL, H_IN, H_OUT, N_BUF };
struct PnpWs : Staging<N_BUF> {
    std::vector<PnpProblemDev> h_problems;  // sources of asynchronous uploads: they outlive the call
    std::vector<PnpCtl> h_ctl;
    ~PnpWs() { release(); }
};

// P3
static void ransac_parameters(int n, double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                              int &mi, int &max_its)
{
    const float v = (float)n * epsilon;
    mi = (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : INT_MAX;
    mi = std::max(mi, std::max(min_inliers, min_set));
    const float ratio = (float)mi / (float)n;  // n == 0: not used
    const float eps = epsilon < ratio ? ratio : epsilon;
    max_its = ransac_max_iterations(n, mi, eps, probability, max_iterations);
}

static int n_use_of(const orbgpu_pnp_problem &p, int N, int mi, int max_its)
{
    if (N < mi)
        return 0;
    const long long reach = std::max<long long>(max_its, (long long)p.start_iteration + p.n_iterations);
    return (int)std::min<long long>(p.n_hyp, reach);
}

static int check_common(const orbgpu_pnp_problem &p, int k)
{
    ORBGPU_REQUIRE(p.n1 >= 0 && p.n1 <= PNP_MAX_N1, "problem %d: n1 outside [0, %d]", k, PNP_MAX_N1);
    ORBGPU_REQUIRE(p.n_hyp >= 0 && p.n_hyp <= PNP_MAX_HYP, "problem %d: n_hyp outside [0, %d]", k, PNP_MAX_HYP);
    ORBGPU_REQUIRE(p.min_set >= PNP_MIN_SET_LO && p.min_set <= PNP_MIN_SET_HI, "problem %d: min_set outside [%d, %d]", k,
                   PNP_MIN_SET_LO, PNP_MIN_SET_HI);
    ORBGPU_REQUIRE(p.nlevels >= 1 && p.nlevels <= ORBGPU_MAX_LEVELS, "problem %d: nlevels outside [1, %d]", k, ORBGPU_MAX_LEVELS);
    ORBGPU_REQUIRE(p.min_inliers >= 0 && p.max_iterations >= 0 && p.start_iteration >= 0 && p.best_so_far >= 0 && p.n_iterations >= 0,
                   "problem %d: negative min_inliers / max_iterations / start_iteration / best_so_far / n_iterations", k);
    ORBGPU_REQUIRE(p.n1 == 0 || (p.valid && p.Xw && p.kp && p.octave), "problem %d: null input arrays", k);
    ORBGPU_REQUIRE(p.n_hyp == 0 || p.sets, "problem %d: null sets", k);
    return ORBGPU_OK;
}

// for orbgpu_pnp_solve_table (map_table.hip), which builds the arrays itself
int pnp_check_host_problem(const orbgpu_pnp_problem &p)
{
    orbgpu_pnp_problem q = p;
    static const uint8_t some = 0;  // stands for the arrays the caller is about to make
    q.valid = &some, q.Xw = q.kp = reinterpret_cast<const float *>(&some), q.octave = reinterpret_cast<const int32_t *>(&some);
    return check_common(q, 0);
}

static int check_device_problem(const orbgpu_pnp_problem &p, int k)
{
    int rc = check_common(p, k);
    if (rc != ORBGPU_OK)
        return rc;
    ORBGPU_REQUIRE(p.result, "problem %d: null result", k);
    ORBGPU_REQUIRE(p.n1 == 0 || p.refined_mask, "problem %d: null refined_mask", k);
    ORBGPU_REQUIRE(p.n_hyp == 0 || (p.counts && p.Tcw && (p.n1 == 0 || p.masks)), "problem %d: null output arrays", k);
    return ORBGPU_OK;
}

} // namespace orbgpu

using namespace orbgpu;

extern "C" int orbgpu_pnp_ransac_parameters(int32_t n, double probability, int32_t min_inliers, int32_t max_iterations,
                                            int32_t min_set, float epsilon, int32_t *adjusted_min_inliers, int32_t *max_its)
{
    ORBGPU_REQUIRE(adjusted_min_inliers && max_its && n >= 0 && min_inliers >= 0 && max_iterations >= 0 && min_set >= 0,
                   "bad arguments");
    int mi, its;
    ransac_parameters(n, probability, min_inliers, max_iterations, min_set, epsilon, mi, its);
    *adjusted_min_inliers = mi, *max_its = its;
    return ORBGPU_OK;
}

extern "C" int orbgpu_pnp_solve_batch_device(int32_t n, const orbgpu_pnp_problem *problems, int32_t device_id, void *hip_stream)
{
    PnpWs *wsp;
    int rc = batch_begin(n, problems, check_device_problem, device_id, wsp);
    if (rc != ORBGPU_OK || !wsp)
        return rc;
    PnpWs &ws = *wsp;
    size_t rows = 0;
    int max_hyp = 0;
    for (int k = 0; k < n; k++) {
        rows += (size_t)problems[k].n1;
        max_hyp = std::max(max_hyp, (int)problems[k].n_hyp);
    }
    const size_t r1 = std::max<size_t>(rows, 1);
    ws.reserve(PROBLEMS, sizeof(PnpProblemDev) * (size_t)n);
    ws.reserve(REC, sizeof(float4) * r1);
    ws.reserve(UV, sizeof(float2) * r1);
    ws.reserve(MAP, sizeof(int32_t) * r1);
    ws.reserve(LIST, sizeof(int32_t) * r1);
    ws.reserve(CTL, sizeof(PnpCtl) * (size_t)n);
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    std::vector<PnpProblemDev> &hp = ws.h_problems;
    std::vector<PnpCtl> &ctl = ws.h_ctl;
    ORBGPU_HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));  // an earlier call's uploads have left hp / ctl
    hp.resize((size_t)n), ctl.resize((size_t)n);
    size_t ro = 0;
    for (int k = 0; k < n; k++) {
        const orbgpu_pnp_problem &p = problems[k];
        PnpProblemDev &D = hp[k];
        memset(&D, 0, sizeof(D));
        D.valid = p.valid, D.Xw = p.Xw, D.kp = p.kp, D.octave = p.octave, D.sets = p.sets;
        D.counts = p.counts, D.Tcw = p.Tcw;
        D.masks = reinterpret_cast<unsigned long long *>(p.masks);
        D.refined_mask = reinterpret_cast<unsigned long long *>(p.refined_mask);
        D.indices = p.indices, D.result = p.result;
        D.rec = ws.as<float4>(REC) + ro, D.uv = ws.as<float2>(UV) + ro, D.map = ws.as<int32_t>(MAP) + ro;
        D.list = ws.as<int32_t>(LIST) + ro, D.ctl = ws.as<PnpCtl>(CTL) + k;
        ro += (size_t)p.n1;
        D.n1 = p.n1, D.n_hyp = p.n_hyp, D.nlevels = p.nlevels, D.min_set = p.min_set;
        D.start_iteration = p.start_iteration, D.best_so_far = p.best_so_far, D.n_iterations = p.n_iterations;
        D.K[0] = p.fx, D.K[1] = p.fy, D.K[2] = p.cx, D.K[3] = p.cy;
        for (int l = 0; l < p.nlevels; l++)  // P2
            D.max_error[l] = p.level_sigma2[l] * p.th2;
    }
    const hipStream_t st = (hipStream_t)hip_stream;
    ORBGPU_HIP_TRY(hipMemcpyAsync(ws.buf[PROBLEMS].p, hp.data(), sizeof(PnpProblemDev) * (size_t)n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pnp_prepare, dim3(n), dim3(64), 0, st, ws.as<PnpProblemDev>(PROBLEMS));
    ORBGPU_HIP_TRY(hipGetLastError());
    ORBGPU_HIP_TRY(hipMemcpyAsync(ctl.data(), ws.buf[CTL].p, sizeof(PnpCtl) * (size_t)n, hipMemcpyDeviceToHost, st));
    ORBGPU_HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < n; k++) {
        const orbgpu_pnp_problem &p = problems[k];
        PnpCtl &c = ctl[k];
        int mi, its;
        ransac_parameters(c.n, p.probability, p.min_inliers, p.max_iterations, p.min_set, p.epsilon, mi, its);
        c.min_inliers = mi, c.max_its = its;
        c.n_use = n_use_of(p, c.n, mi, its);
    }
    ORBGPU_HIP_TRY(hipMemcpyAsync(ws.buf[CTL].p, ctl.data(), sizeof(PnpCtl) * (size_t)n, hipMemcpyHostToDevice, st));
    if (max_hyp > 0) {
        hipLaunchKernelGGL(k_pnp_hypotheses, dim3(max_hyp, n), dim3(64), 0, st, ws.as<PnpProblemDev>(PROBLEMS));
        ORBGPU_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_pnp_select, dim3(n), dim3(64), 0, st, ws.as<PnpProblemDev>(PROBLEMS));
    ORBGPU_HIP_TRY(hipGetLastError());
    return ORBGPU_OK;
}

extern "C" int orbgpu_pnp_solve_device(const orbgpu_pnp_problem *p, int32_t device_id, void *hip_stream)
{
    ORBGPU_REQUIRE(p, "null argument");
    return orbgpu_pnp_solve_batch_device(1, p, device_id, hip_stream);
}

// The host flavours.  all = false: the returned Tcw and the inlier bytes of the result; all = true: Tcw [H][16] and
// masks [H][words] of every hypothesis and the words of the returned mask.
static int solve_host(const orbgpu_pnp_problem *p, int32_t *counts, float *Tcw, uint8_t *inliers, uint64_t *masks,
                      uint64_t *refined_mask, bool all, orbgpu_pnp_result *result, int32_t device_id)
{
    ORBGPU_REQUIRE(p && result, "null argument");
    int rc = check_common(*p, 0);
    if (rc != ORBGPU_OK)
        return rc;
    const int n1 = p->n1, H = p->n_hyp, ms = p->min_set;
    // P1 and P3 on the host, to refuse a set index outside [0, N) before anything is launched
    int N = 0;
    for (int i = 0; i < n1; i++)
        if (p->valid[i] && p->octave[i] >= 0 && p->octave[i] < p->nlevels)
            N++;
    int mi, max_its;
    ransac_parameters(N, p->probability, p->min_inliers, p->max_iterations, ms, p->epsilon, mi, max_its);
    const int n_use = n_use_of(*p, N, mi, max_its);
    for (int h = 0; h < n_use; h++)
        for (int k = 0; k < ms; k++)
            ORBGPU_REQUIRE(p->sets[(size_t)h * ms + k] >= 0 && p->sets[(size_t)h * ms + k] < N, "set %d: index %d outside [0, %d)", h,
                           p->sets[(size_t)h * ms + k], N);
    // one staging block each way; the words of the returned mask land in `mask` in either flavour
    const size_t words = (size_t)(n1 + 63) / 64;
    orbgpu_pnp_result r;
    std::vector<uint64_t> mask(std::max<size_t>(words, 1), 0);
    HostPlan<N_BUF> plan;
    const auto i_valid = plan.in(H_IN, p->valid, n1);
    const auto i_x = plan.in(H_IN, p->Xw, n1, 3), i_kp = plan.in(H_IN, p->kp, n1, 2);
    const auto i_o = plan.in(H_IN, p->octave, n1), i_s = plan.in(H_IN, p->sets, H, ms);
    const auto o_res = plan.out(H_OUT, &r, 1);
    const auto o_cnt = plan.out(H_OUT, counts, H);
    const auto o_T = plan.out(H_OUT, all ? Tcw : nullptr, H, 16);
    const auto o_rm = plan.out(H_OUT, mask.data(), 1, words), o_m = plan.out(H_OUT, masks, H, words);
    PnpWs *wsp;
    if ((rc = host_begin(device_id, plan, wsp)) != ORBGPU_OK)
        return rc;
    PnpWs &ws = *wsp;
    PnpWs::FinishOnError on_error{ws};
    plan.upload(ws);
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    // hypotheses beyond n_use come back as zeros
    ORBGPU_HIP_TRY(hipMemsetAsync(ws.as<char>(H_OUT), 0, plan.bytes(H_OUT), ws.stream));
    orbgpu_pnp_problem d = *p;
    d.valid = ws.at(i_valid), d.Xw = ws.at(i_x), d.kp = ws.at(i_kp);
    d.octave = ws.at(i_o), d.sets = ws.at(i_s);
    d.result = ws.at(o_res), d.counts = ws.at(o_cnt), d.Tcw = ws.at(o_T);
    d.refined_mask = ws.at(o_rm), d.masks = ws.at(o_m);
    d.indices = nullptr;
    if ((rc = orbgpu_pnp_solve_batch_device(1, &d, device_id, ws.stream)) != ORBGPU_OK)
        return rc;
    plan.download(ws);
    if ((rc = ws.finish()) != ORBGPU_OK)
        return rc;
    if (all) {
        if (refined_mask)
            for (size_t w = 0; w < words; w++)
                refined_mask[w] = mask[w];
    } else {
        if (Tcw)
            memcpy(Tcw, r.Tcw, sizeof(r.Tcw));
        if (inliers)
            mask_to_bytes(mask.data(), n1, inliers);
    }
    *result = r;
    return ORBGPU_OK;
}

extern "C" int orbgpu_pnp_solve(const orbgpu_pnp_problem *p, int32_t *counts, float *Tcw, uint8_t *inliers,
                                orbgpu_pnp_result *result, int32_t device_id)
{
    return solve_host(p, counts, Tcw, inliers, nullptr, nullptr, false, result, device_id);
}

extern "C" int orbgpu_pnp_solve_all(const orbgpu_pnp_problem *p, int32_t *counts, float *Tcw, uint64_t *masks,
                                    uint64_t *refined_mask, orbgpu_pnp_result *result, int32_t device_id)
{
    return solve_host(p, counts, Tcw, nullptr, masks, refined_mask, true, result, device_id);
}

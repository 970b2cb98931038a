// The FP64 Sim3 arithmetic of the device optimisers, written once: the group operations on 8-double states (q[4] as x, y, z,
// w, not normalised; t[3]; s), the logarithm and the edge error of the pose graph (essential_graph.hip, G2-G4), and the
// exponential update S' = exp(x) * S of both Sim3 optimisers (sim3_opt.hip O4, O5; essential_graph.hip G5).  The definition
// of every function is its namesake in tests/eg_model.py (s_mul, s_inv, s_map, lu_solve3, s_log, s_update) and
// tests/sim3opt_model.py (sim3_update), operation for operation; tests/sim3_math_test.cpp builds this header with g++ and
// tests/test_sim3_math.py compares the two bit for bit.  The rules are opt_math.h's: host + device, no HIP header, no fused
// multiply-add, and no expression may be re-associated.
#pragma once

#include "opt_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif  // gcc: build with -ffp-contract=off

namespace orbgpu {

ORBGPU_HD inline void load8(const double *p, double o[8])
{
    ORBGPU_UNROLL
    for (int k = 0; k < 8; k++)
        o[k] = p[k];
}

// ---- G2 ------------------------------------------------------------------------------------------------------------------
ORBGPU_HD inline void mat_vec3(const double R[9], const double v[3], double o[3])
{
    ORBGPU_UNROLL
    for (int r = 0; r < 3; r++)
        o[r] = (R[3 * r] * v[0] + R[3 * r + 1] * v[1]) + R[3 * r + 2] * v[2];
}

ORBGPU_HD inline void sim3_mul(const double A[8], const double B[8], double o[8])
{
    double R[9], Rt[3];
    quat_mul(A, B, o);
    quat_to_matrix(A, R);
    mat_vec3(R, B + 4, Rt);
    ORBGPU_UNROLL
    for (int r = 0; r < 3; r++)
        o[4 + r] = A[7] * Rt[r] + A[4 + r];
    o[7] = A[7] * B[7];
}

ORBGPU_HD inline void sim3_inv(const double S[8], double o[8])
{
    double R[9];
    quat_to_matrix(S, R);
    const double is = 1.0 / S[7];
    const double u0 = -is * S[4], u1 = -is * S[5], u2 = -is * S[6];
    o[0] = -S[0], o[1] = -S[1], o[2] = -S[2], o[3] = S[3];
    ORBGPU_UNROLL
    for (int r = 0; r < 3; r++)
        o[4 + r] = (R[r] * u0 + R[3 + r] * u1) + R[6 + r] * u2;
    o[7] = is;
}

ORBGPU_HD inline void sim3_map(const double S[8], const double X[3], double o[3])
{
    double R[9], RX[3];
    quat_to_matrix(S, R);
    mat_vec3(R, X, RX);
    ORBGPU_UNROLL
    for (int r = 0; r < 3; r++)
        o[r] = S[7] * RX[r] + S[4 + r];
}

// W x = t by LU with partial pivoting (G3); the swaps are selects, so that everything stays in registers
ORBGPU_HD inline void lu_solve3(const double W[9], const double t[3], double x[3])
{
    double a00 = W[0], a01 = W[1], a02 = W[2], a10 = W[3], a11 = W[4], a12 = W[5], a20 = W[6], a21 = W[7], a22 = W[8];
    double b0 = t[0], b1 = t[1], b2 = t[2];
#define ORBGPU_SIM3_SWAP(p, q)          \
    {                                   \
        const double tp = m ? q : p;    \
        q = m ? p : q;                  \
        p = tp;                         \
    }
    {
        const bool m = fabs(a10) > fabs(a00);
        ORBGPU_SIM3_SWAP(a00, a10) ORBGPU_SIM3_SWAP(a01, a11) ORBGPU_SIM3_SWAP(a02, a12) ORBGPU_SIM3_SWAP(b0, b1)
    }
    {
        const bool m = fabs(a20) > fabs(a00);
        ORBGPU_SIM3_SWAP(a00, a20) ORBGPU_SIM3_SWAP(a01, a21) ORBGPU_SIM3_SWAP(a02, a22) ORBGPU_SIM3_SWAP(b0, b2)
    }
    const double m1 = a10 / a00;
    a11 = a11 - m1 * a01, a12 = a12 - m1 * a02, b1 = b1 - m1 * b0;
    const double m2 = a20 / a00;
    a21 = a21 - m2 * a01, a22 = a22 - m2 * a02, b2 = b2 - m2 * b0;
    {
        const bool m = fabs(a21) > fabs(a11);
        ORBGPU_SIM3_SWAP(a11, a21) ORBGPU_SIM3_SWAP(a12, a22) ORBGPU_SIM3_SWAP(b1, b2)
    }
#undef ORBGPU_SIM3_SWAP
    const double m3 = a21 / a11;
    a22 = a22 - m3 * a12, b2 = b2 - m3 * b1;
    x[2] = b2 / a22;
    x[1] = (b1 - a12 * x[2]) / a11;
    x[0] = ((b0 - a01 * x[1]) - a02 * x[2]) / a00;
}

// G3
ORBGPU_HD inline void sim3_log(const double S[8], double e[7])
{
    const double s = S[7];
    const double sigma = log(s);
    double R[9];
    quat_to_matrix(S, R);
    const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const double eps = 1e-5;
    const bool small_th = d > 1.0 - eps, small_sigma = fabs(sigma) < eps;
    double w[3], th = 0.0;
    if (small_th) {
        ORBGPU_UNROLL
        for (int r = 0; r < 3; r++)
            w[r] = 0.5 * dR[r];
    } else {
        th = acos(d);
        const double f = th / (2.0 * sqrt(1.0 - d * d));
        ORBGPU_UNROLL
        for (int r = 0; r < 3; r++)
            w[r] = f * dR[r];
    }
    double A, B, C;
    if (small_sigma) {
        C = 1.0;
        if (small_th) {
            A = 0.5;
            B = 1.0 / 6.0;
        } else {
            const double sn = sin(th), cs = cos(th), th2 = th * th;
            A = (1.0 - cs) / th2;
            B = (th - sn) / (th2 * th);
        }
    } else {
        C = (s - 1.0) / sigma;
        const double sigma2 = sigma * sigma;
        if (small_th) {
            A = ((sigma - 1.0) * s + 1.0) / sigma2;
            B = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma);  // as published (G3)
        } else {
            const double sn = sin(th), cs = cos(th), th2 = th * th;
            const double a = s * sn, b = s * cs, c = th2 + sigma2;
            A = (a * sigma + (1.0 - b) * th) / (th * c);
            B = (C - ((b - 1.0) * sigma + a * th) / c) / th2;
        }
    }
    const double O[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    double W[9];
    ORBGPU_UNROLL
    for (int r = 0; r < 3; r++)
        ORBGPU_UNROLL
        for (int c = 0; c < 3; c++) {
            const double o2 = (O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c]) + O[3 * r + 2] * O[6 + c];
            W[3 * r + c] = (A * O[3 * r + c] + B * o2) + (r == c ? C : 0.0);
        }
    lu_solve3(W, S + 4, e + 3);
    e[0] = w[0], e[1] = w[1], e[2] = w[2];
    e[6] = sigma;
}

// G4: e = log((M * S_i) * S_j^-1), the error of a pose-graph edge
ORBGPU_HD inline void sim3_edge_error(const double M[8], const double Si[8], const double Sj[8], double e[7])
{
    double A[8], Bi[8], C[8];
    sim3_mul(M, Si, A);
    sim3_inv(Sj, Bi);
    sim3_mul(A, Bi, C);
    sim3_log(C, e);
}

ORBGPU_HD inline double chi2_of(const double e[7])
{
    double c = e[0] * e[0];
    ORBGPU_UNROLL
    for (int r = 1; r < 7; r++)
        c = c + e[r] * e[r];
    return c;
}

// S' = exp(x) * S (O4, O5) on (q, t, s); nothing is renormalised.  The four cases of A, B, C (small / large angle x
// small / large |sigma|, threshold 1e-5) are written here and nowhere else.
ORBGPU_HD inline void sim3_update(const double q[4], const double t[3], double s, const double x[7], bool fix_scale,
                                  double qn[4], double tn[3], double &sn)
{
    const double w0 = x[0], w1 = x[1], w2 = x[2];
    const double sigma = fix_scale ? 0.0 : x[6];
    const double th = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
    const double sx = exp(sigma);
    const double O[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    double O2[9];
    ORBGPU_UNROLL
    for (int r = 0; r < 3; r++)
        ORBGPU_UNROLL
        for (int c = 0; c < 3; c++)
            O2[3 * r + c] = (O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c]) + O[3 * r + 2] * O[6 + c];
    const double eps = 1e-5;
    const bool small_th = th < eps, small_sigma = fabs(sigma) < eps;
    double A, B, C, ra = 1.0, rb = 1.0;  // R = (I + ra Om) + rb Om Om
    if (small_sigma) {
        C = 1.0;
        if (small_th) {
            A = 0.5;
            B = 1.0 / 6.0;
        } else {
            const double sn_ = sin(th), cs = cos(th);
            A = (1.0 - cs) / (th * th);
            B = (th - sn_) / ((th * th) * th);
            ra = sn_ / th;
            rb = (1.0 - cs) / (th * th);
        }
    } else {
        C = (sx - 1.0) / sigma;
        if (small_th) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1.0) * sx + 1.0) / sigma2;
            B = (((0.5 * sigma2 - sigma) + 1.0) * sx) / (sigma2 * sigma);
        } else {
            const double sn_ = sin(th), cs = cos(th);
            ra = sn_ / th;
            rb = (1.0 - cs) / (th * th);
            const double a = sx * sn_, b = sx * cs, th2 = th * th, c = th2 + sigma * sigma;
            A = (a * sigma + (1.0 - b) * th) / (th * c);
            B = (C - ((b - 1.0) * sigma + a * th) / c) / th2;
        }
    }
    double R[9], W[9];
    ORBGPU_UNROLL
    for (int i = 0; i < 9; i++) {
        const bool diag = i % 4 == 0;
        R[i] = small_th ? ((diag ? 1.0 : 0.0) + O[i]) + O2[i] : ((diag ? 1.0 : 0.0) + ra * O[i]) + rb * O2[i];
        W[i] = (A * O[i] + B * O2[i]) + (diag ? C : 0.0);
    }
    double qx[4], Rx[9];
    quat_from_matrix(R, qx);
    quat_to_matrix(qx, Rx);
    quat_mul(qx, q, qn);
    ORBGPU_UNROLL
    for (int r = 0; r < 3; r++) {
        const double tx = (W[3 * r] * x[3] + W[3 * r + 1] * x[4]) + W[3 * r + 2] * x[5];
        tn[r] = sx * ((Rx[3 * r] * t[0] + Rx[3 * r + 1] * t[1]) + Rx[3 * r + 2] * t[2]) + tx;
    }
    sn = sx * s;
}

// the same on 8-double states
ORBGPU_HD inline void sim3_update(const double S[8], const double x[7], bool fix_scale, double Sn[8])
{
    sim3_update(S, S + 4, S[7], x, fix_scale, Sn, Sn + 4, Sn[7]);
}

} // namespace orbgpu

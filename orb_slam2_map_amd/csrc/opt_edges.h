// The reprojection edge and the SE3 vertex update the bundle adjustments share (pose_opt.hip, local_ba.hip): g2o's
// EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ error and its Jacobians, and SE3Quat's exp(x) * T.  The definition of every
// function is its namesake in tests/pose_model.py (point_jacobian: tests/lba_model.py), operation for operation, under the
// arithmetic rules of opt_math.h.
#pragma once

#include "common.h"
#include "opt_math.h"

namespace orbgpu {

struct Cam {
    double fx, fy, cx, cy, bf;
};

// T' = exp(x) * T with x = (omega, upsilon): SE3Quat::exp (its small-angle branch kept as is) and operator*
__device__ inline void pose_update(const double q[4], const double t[3], const double x[6], double qn[4], double tn[3])
{
    const double w0 = x[0], w1 = x[1], w2 = x[2];
    const double th = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
    const double O[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    double O2[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++)
            O2[3 * r + c] = (O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c]) + O[3 * r + 2] * O[6 + c];
    double R[9], V[9];
    if (th < 1e-5) {
#pragma unroll
        for (int i = 0; i < 9; i++) {
            R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + O[i]) + O2[i];
            V[i] = R[i];
        }
    } else {
        const double sn = sin(th), cs = cos(th);
        const double a = sn / th, b = (1.0 - cs) / (th * th), c = (th - sn) / ((th * th) * th);
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const double I = i % 4 == 0 ? 1.0 : 0.0;
            R[i] = (I + a * O[i]) + b * O2[i];
            V[i] = (I + b * O[i]) + c * O2[i];
        }
    }
    double dq[4], dR[9];
    quat_from_matrix(R, dq);
    quat_normalize(dq);
    quat_mul(dq, q, qn);
    quat_normalize(qn);
    quat_to_matrix(dq, dR);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double dt = (V[3 * r] * x[3] + V[3 * r + 1] * x[4]) + V[3 * r + 2] * x[5];
        tn[r] = ((dR[3 * r] * t[0] + dR[3 * r + 1] * t[1]) + dR[3 * r + 2] * t[2]) + dt;
    }
}

// ---- one edge ----------------------------------------------------------------------------------------------------
// e = obs - projection (third component 0 for a mono edge), P = R Xw + t, returns chi2 = invSigma2 * e'e
__device__ inline double edge_error(const double R[9], const double t[3], const Cam &C, double X0, double X1, double X2,
                                    double w, double ox, double oy, double our, bool stereo, double e[3], double P[3])
{
#pragma unroll
    for (int r = 0; r < 3; r++)
        P[r] = ((R[3 * r] * X0 + R[3 * r + 1] * X1) + R[3 * r + 2] * X2) + t[r];
    const double iz = 1.0 / P[2];
    const double u = (C.fx * P[0]) * iz + C.cx;
    e[0] = ox - u;
    e[1] = oy - ((C.fy * P[1]) * iz + C.cy);
    e[2] = stereo ? our - (u - C.bf * iz) : 0.0;
    return w * ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
}

// the same over a packed edge record: a = (float Xw, invSigma2), b = (kp x, kp y, u_right, -)
__device__ inline double edge_error(const double R[9], const double t[3], const Cam &C, const float4 a, const float4 b,
                                    bool stereo, double e[3], double P[3])
{
    return edge_error(R, t, C, (double)a.x, (double)a.y, (double)a.z, (double)a.w, (double)b.x, (double)b.y, (double)b.z,
                      stereo, e, P);
}

// d e / d (omega, upsilon) of the left update exp(omega, upsilon) * T at zero, P = the camera point; row 2 is 0 for a mono
// edge
__device__ inline void pose_jacobian(const double P[3], const Cam &C, bool stereo, double J[3][6])
{
    const double x = P[0], y = P[1], z = P[2];
    const double iz = 1.0 / z, iz2 = iz * iz;
    J[0][0] = ((x * y) * iz2) * C.fx;
    J[0][1] = -(1.0 + (x * x) * iz2) * C.fx;
    J[0][2] = (y * iz) * C.fx;
    J[0][3] = -iz * C.fx;
    J[0][4] = 0.0;
    J[0][5] = (x * iz2) * C.fx;
    J[1][0] = (1.0 + (y * y) * iz2) * C.fy;
    J[1][1] = -((x * y) * iz2) * C.fy;
    J[1][2] = -(x * iz) * C.fy;
    J[1][3] = 0.0;
    J[1][4] = -iz * C.fy;
    J[1][5] = (y * iz2) * C.fy;
    if (stereo) {
        J[2][0] = J[0][0] - (C.bf * y) * iz2;
        J[2][1] = J[0][1] + (C.bf * x) * iz2;
        J[2][2] = J[0][2];
        J[2][3] = J[0][3];
        J[2][4] = 0.0;
        J[2][5] = J[0][5] - C.bf * iz2;
    } else {
#pragma unroll
        for (int a = 0; a < 6; a++)
            J[2][a] = 0.0;
    }
}

// d e / d Xw = -(d proj / d Pc) R (EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ::linearizeOplus, the point's side)
__device__ inline void point_jacobian(const double P[3], const double R[9], const Cam &C, bool stereo, double J[3][3])
{
    const double x = P[0], y = P[1], z = P[2];
    const double iz = 1.0 / z, iz2 = iz * iz;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        J[0][c] = -(C.fx * R[c]) * iz + ((C.fx * x) * R[6 + c]) * iz2;
        J[1][c] = -(C.fy * R[3 + c]) * iz + ((C.fy * y) * R[6 + c]) * iz2;
        J[2][c] = stereo ? J[0][c] - (C.bf * R[6 + c]) * iz2 : 0.0;
    }
}

} // namespace orbgpu

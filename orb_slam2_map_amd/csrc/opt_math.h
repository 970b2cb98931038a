// The FP64 arithmetic the device optimisers share (pose_opt.hip, sim3_opt.hip, local_ba.hip, essential_graph.hip): quaternions
// as g2o's SE3Quat / Sim3 use them, the Huber weights, the dense LL^T solve of the damped normal equation, its initial
// damping, the decision on a Levenberg-Marquardt trial and the fixed-order workgroup reductions.  The definition of every
// function is its namesake in tests/pose_model.py, operation for operation; tests/opt_math_test.cpp builds this header with
// g++ and tests/test_opt_math.py compares the two bit for bit.  No fused multiply-add (-ffp-contract=off), and no
// expression may be re-associated: parity of the optimisers with their models rests on the order written here.  Pure C++
// except the part under __HIPCC__ (the workgroup reductions, the barrier and the stop flag), which needs the device.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define ORBGPU_HD __host__ __device__
#define ORBGPU_UNROLL _Pragma("unroll")
#else
#define ORBGPU_HD
#define ORBGPU_UNROLL
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif  // gcc: build with -ffp-contract=off

namespace orbgpu {

// ---- quaternions (x, y, z, w) ------------------------------------------------------------------------------------------
// Eigen's Quaterniond(Matrix3d)
ORBGPU_HD inline void quat_from_matrix(const double m[9], double q[4])
{
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t;
        q[1] = (m[2] - m[6]) * t;
        q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0])
            i = 1;
        if (m[8] > m[4 * i])
            i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t;
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t;
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t;
    }
}

// SE3Quat::normalizeRotation: w >= 0, unit norm
ORBGPU_HD inline void quat_normalize(double q[4])
{
    if (q[3] < 0)
        for (int i = 0; i < 4; i++)
            q[i] = -q[i];
    const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    for (int i = 0; i < 4; i++)
        q[i] = q[i] / n;
}

ORBGPU_HD inline void quat_to_matrix(const double q[4], double R[9])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1.0 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
    R[3] = txy + twz, R[4] = 1.0 - (txx + tzz), R[5] = tyz - twx;
    R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1.0 - (txx + tyy);
}

ORBGPU_HD inline void quat_mul(const double a[4], const double b[4], double o[4])
{
    o[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
    o[1] = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2];
    o[2] = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0];
    o[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
}

// The entry state of an optimiser (Converter::toSE3Quat, Converter.cc:37-47): the float 3x3 at the head of rows of
// `stride` floats -> double -> unit quaternion
inline void unit_quat_from_floats(const float *m, int stride, double q[4])
{
    double R[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++)
            R[3 * r + c] = (double)m[stride * r + c];
    quat_from_matrix(R, q);
    quat_normalize(q);
}

// RobustKernelHuber without the second-order term; an edge without kernel keeps chi2
ORBGPU_HD inline void huber(double chi2, double delta, double delta2, double &rho0, double &rho1, bool use_kernel = true)
{
    if (chi2 <= delta2 || !use_kernel) {
        rho0 = chi2;
        rho1 = 1.0;
    } else {
        const double s = sqrt(chi2);
        rho0 = (2.0 * s) * delta - delta2;
        rho1 = delta / s;
    }
}

// (H + lam I) x = b by LL^T, H as its upper triangle packed row by row; not positive definite (a pivot that is not > 0,
// NaN included): false and x = 0
template <int N>
ORBGPU_HD inline bool cholesky_solve(const double (&Hu)[N * (N + 1) / 2], double lam, const double (&b)[N], double (&x)[N])
{
    double A[N][N], L[N][N];
    {
        int k = 0;
        ORBGPU_UNROLL
        for (int a = 0; a < N; a++)
            ORBGPU_UNROLL
            for (int c = a; c < N; c++, k++)
                A[a][c] = A[c][a] = Hu[k];
    }
    ORBGPU_UNROLL
    for (int i = 0; i < N; i++) {
        A[i][i] = A[i][i] + lam;
        ORBGPU_UNROLL
        for (int j = 0; j < N; j++)
            L[i][j] = 0.0;
        x[i] = 0.0;
    }
    bool ok = true;
    ORBGPU_UNROLL
    for (int j = 0; j < N; j++) {
        double d = A[j][j];
        ORBGPU_UNROLL
        for (int k = 0; k < j; k++)
            d = d - L[j][k] * L[j][k];
        if (!(d > 0.0))
            ok = false;
        d = sqrt(d);
        L[j][j] = d;
        ORBGPU_UNROLL
        for (int i = j + 1; i < N; i++) {
            double s = A[j][i];
            ORBGPU_UNROLL
            for (int k = 0; k < j; k++)
                s = s - L[i][k] * L[j][k];
            L[i][j] = s / d;
        }
    }
    if (!ok)
        return false;
    double y[N];
    ORBGPU_UNROLL
    for (int i = 0; i < N; i++) {
        double s = b[i];
        ORBGPU_UNROLL
        for (int k = 0; k < i; k++)
            s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
    ORBGPU_UNROLL
    for (int i = N - 1; i >= 0; i--) {
        double s = y[i];
        ORBGPU_UNROLL
        for (int k = i + 1; k < N; k++)
            s = s - L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
    return true;
}

// ---- Levenberg-Marquardt bookkeeping (g2o's OptimizationAlgorithmLevenberg) ----------------------------------------------
// the first iteration's damping: 1e-5 * max |diag H|
template <int N> ORBGPU_HD inline double lm_initial_lambda(const double (&Hu)[N * (N + 1) / 2])
{
    double m = 0.0;
    ORBGPU_UNROLL
    for (int a = 0, k = 0; a < N; k += N - a, a++)
        if (fabs(Hu[k]) > m)
            m = fabs(Hu[k]);
    return 1e-5 * m;
}

// The decision on one trial: the robust chi2 went from cur to tmp under a step whose x'(lambda x + b) + 1e-3 is `scale`.
// Accepted (true): lambda shrinks by max(1/3, min(1 - (2 rho - 1)^3, 2/3)) and nu restarts at 2; the caller keeps the
// trial's state and sets cur = tmp.  Refused: lambda grows by nu, nu doubles, and a lambda that is no longer finite sets
// stop.  The callers loop while (!stop && rho < 0 && trial < 10).
ORBGPU_HD inline bool lm_trial(double cur, double tmp, double scale, double &lam, double &nu, double &rho, bool &stop)
{
    using std::isfinite;  // g++ declares it nowhere else
    rho = (cur - tmp) / scale;
    if (rho > 0 && isfinite(tmp)) {
        const double c3 = 2.0 * rho - 1.0;
        const double alpha = fmin(1.0 - (c3 * c3) * c3, 2.0 / 3.0);
        lam = lam * fmax(1.0 / 3.0, alpha);
        nu = 2.0;
        return true;
    }
    lam = lam * nu;
    nu = nu * 2.0;
    if (!isfinite(lam))
        stop = true;
    return false;
}

// ---- what the bundle adjustment with free points adds (local_ba.hip; definitions in tests/lba_model.py, host test
// tests/opt_math_lba_test.cpp) ---------------------------------------------------------------------------------------------
// Inverse of the symmetric 3x3 with upper triangle h = (00, 01, 02, 11, 12, 22) and lam added to its diagonal, by cofactors
// as Eigen's 3x3 inverse: the determinant from the first column's cofactors, one reciprocal.  inv row-major, all 9 entries.
ORBGPU_HD inline void inv3_sym(const double h[6], double lam, double inv[9])
{
    const double m[3][3] = {{h[0] + lam, h[1], h[2]}, {h[1], h[3] + lam, h[4]}, {h[2], h[4], h[5] + lam}};
    double c[3][3];
    ORBGPU_UNROLL
    for (int i = 0; i < 3; i++)
        ORBGPU_UNROLL
        for (int j = 0; j < 3; j++) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            c[i][j] = m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
        }
    const double det = (c[0][0] * m[0][0] + c[1][0] * m[1][0]) + c[2][0] * m[2][0];
    const double invdet = 1.0 / det;
    ORBGPU_UNROLL
    for (int i = 0; i < 3; i++)
        ORBGPU_UNROLL
        for (int j = 0; j < 3; j++)
            inv[3 * i + j] = c[j][i] * invdet;
}

// VertexSBAPointXYZ::oplusImpl
ORBGPU_HD inline void point_update(const double X[3], const double x[3], double Xn[3])
{
    ORBGPU_UNROLL
    for (int i = 0; i < 3; i++)
        Xn[i] = X[i] + x[i];
}

// position of (i, j), i >= j, in a lower triangle packed row by row
ORBGPU_HD inline size_t tri_at(int i, int j)
{
    return (size_t)i * (size_t)(i + 1) / 2 + (size_t)j;
}

// A x = b by LL^T for a symmetric A of runtime size n.  A: its lower triangle packed row by row (tri_at), overwritten with
// L below the diagonal (the diagonal keeps the pivots before their root); v: b on entry, x on return; work: 2 n doubles.
// Written for `nt` cooperating threads (this one is `tid`) that call `barrier()` together -- a workgroup with
// __syncthreads, or one host thread with nothing -- and every entry is computed by the same operations in the same order
// whatever nt is: column j left-looking (k ascending), forward substitution with k ascending and back substitution with k
// DESCENDING per row.  A, v and work are shared by the threads.  A pivot that is not > 0 (NaN included): false and x = 0;
// the return value is the same in every thread.
template <typename Barrier>
ORBGPU_HD inline bool llt_solve(int n, double *A, double *v, double *work, int tid, int nt, Barrier barrier)
{
    double *dg = work, *y = work + n;
    for (int j = 0; j < n; j++) {
        const double *Lj = A + tri_at(j, 0);
        for (int i = j + tid; i < n; i += nt) {
            double *Li = A + tri_at(i, 0);
            double s = Li[j];
            for (int k = 0; k < j; k++)
                s = s - Li[k] * Lj[k];
            Li[j] = s;
        }
        barrier();
        const double d = Lj[j];
        if (!(d > 0.0)) {
            barrier();  // every thread has read its pivot before v changes hands
            for (int i = tid; i < n; i += nt)
                v[i] = 0.0;
            barrier();
            return false;
        }
        const double sd = sqrt(d);
        if (tid == 0)
            dg[j] = sd;
        for (int i = j + 1 + tid; i < n; i += nt)
            A[tri_at(i, j)] = A[tri_at(i, j)] / sd;
        barrier();
    }
    for (int i = tid; i < n; i += nt)
        y[i] = v[i];
    barrier();
    for (int k = 0; k < n; k++) {
        const double yk = y[k] / dg[k];
        barrier();  // y[k] is read by all before its owner replaces it
        if (tid == 0)
            y[k] = yk;
        for (int i = k + 1 + tid; i < n; i += nt)
            y[i] = y[i] - A[tri_at(i, k)] * yk;
        barrier();
    }
    for (int k = n - 1; k >= 0; k--) {
        const double xk = y[k] / dg[k];
        const double *Lk = A + tri_at(k, 0);
        barrier();
        if (tid == 0)
            v[k] = xk;
        for (int i = tid; i < k; i += nt)
            y[i] = y[i] - Lk[i] * xk;
        barrier();
    }
    return true;
}

struct NoBarrier {
    ORBGPU_HD void operator()() const {}
};

#if defined(__HIPCC__)
// Fixed-order sum over a workgroup of WAVES waves: shuffle tree inside each wave, then wave 0 + 1 + ... in every lane.
// The result is the same bits in every lane, so control flow that branches on it stays workgroup-uniform.
// red: WAVES * K doubles of LDS.
template <int WAVES, int K> __device__ inline void block_sum(double (&v)[K], double *red)
{
#pragma unroll
    for (int k = 0; k < K; k++)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            v[k] += __shfl_down(v[k], off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();  // the previous sum's readers are done with `red`
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; k++)
            red[wave * K + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        double s = red[k];
#pragma unroll
        for (int wv = 1; wv < WAVES; wv++)
            s += red[wv * K + k];
        v[k] = s;
    }
}

// max over a workgroup of WAVES waves, the same in every lane; NaN never wins.  red: WAVES doubles of LDS.
template <int WAVES> __device__ inline double block_max(double m, double *red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(m, off, 64);
        if (o > m)
            m = o;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0)
        red[wave] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int wv = 1; wv < WAVES; wv++)
        if (red[wv] > m)
            m = red[wv];
    return m;
}

// the shuffle tree alone: the sums of one wave, in its lane 0
template <int K> __device__ inline void wave_sum(double (&v)[K])
{
#pragma unroll
    for (int k = 0; k < K; k++)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            v[k] += __shfl_down(v[k], off, 64);
}

// the barrier llt_solve and skyline_llt_solve take when a workgroup runs them
struct WorkgroupBarrier {
    __device__ void operator()() const { __syncthreads(); }
};

// the stop flag of an optimiser (L9, G9), read by one lane and broadcast through *flag in LDS
__device__ inline bool stop_requested(const int32_t *stop, int *flag)
{
    if (!stop)
        return false;
    __syncthreads();
    if (threadIdx.x == 0)
        *flag = __hip_atomic_load(stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __syncthreads();
    return *flag != 0;
}
#endif

} // namespace orbgpu

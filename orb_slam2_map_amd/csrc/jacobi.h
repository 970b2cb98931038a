// The cyclic Jacobi eigen-solver of the solvers (H6 of Sim3Solver, P5 of PnPsolver, I4 / I9 of the Initializer, N5 of
// CreateNewMapPoints): pairs row by row, one rotation per pair with a non-zero entry, and a sweep starts only while
// off > JACOBI_STOP * (diag + 2 off).  Parity of those entry points with their models rests on the order written here; the
// definition of every function is its namesake in tests/jacobi_model.py (null_vector4: tests/newpts_model.py), operation for
// operation.  tests/jacobi_test.cpp builds the per-lane half with g++ and tests/test_jacobi.py compares the two bit for bit.
// No fused multiply-add (-ffp-contract=off), and no expression may be re-associated.  Pure C++ except the wave-wide form,
// which needs LDS and the workgroup barrier.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define ORBGPU_JACOBI_HD __host__ __device__
#define ORBGPU_JACOBI_UNROLL _Pragma("unroll")
#define ORBGPU_JACOBI_NO_UNROLL _Pragma("unroll 1")
#else
#define ORBGPU_JACOBI_HD
#define ORBGPU_JACOBI_UNROLL
#define ORBGPU_JACOBI_NO_UNROLL
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif  // gcc: build with -ffp-contract=off

namespace orbgpu {

constexpr double JACOBI_STOP = 1e-32;
constexpr int NULL_VECTOR4_SWEEPS = 30;

// Cyclic Jacobi of a symmetric 4 x 4 in the registers of one lane, at most SWEEPS sweeps: eigenvalues stay on A's diagonal,
// eigenvectors in the columns of V.  The same pairs, rotations and stopping rule as jacobi_wave; lanes diverge only in how
// many sweeps they need.
template <int SWEEPS> ORBGPU_JACOBI_HD inline void jacobi4_lane(double (&A)[4][4], double (&V)[4][4])
{
    ORBGPU_JACOBI_UNROLL
    for (int i = 0; i < 4; i++)
        ORBGPU_JACOBI_UNROLL
        for (int j = 0; j < 4; j++)
            V[i][j] = i == j ? 1.0 : 0.0;
    ORBGPU_JACOBI_NO_UNROLL
    for (int sweep = 0; sweep < SWEEPS; sweep++) {
        double off = 0.0, diag = 0.0;
        ORBGPU_JACOBI_UNROLL
        for (int p = 0; p < 4; p++)
            ORBGPU_JACOBI_UNROLL
            for (int q = p + 1; q < 4; q++)
                off = off + A[p][q] * A[p][q];
        ORBGPU_JACOBI_UNROLL
        for (int i = 0; i < 4; i++)
            diag = diag + A[i][i] * A[i][i];
        if (off <= JACOBI_STOP * (diag + 2.0 * off))
            break;
        ORBGPU_JACOBI_UNROLL
        for (int p = 0; p < 4; p++)
            ORBGPU_JACOBI_UNROLL
            for (int q = p + 1; q < 4; q++) {
                const double apq = A[p][q];
                if (!(apq == 0.0)) {
                    const double app = A[p][p], aqq = A[q][q];
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double den = fabs(theta) + sqrt(theta * theta + 1.0);
                    const double t = theta >= 0.0 ? 1.0 / den : -1.0 / den;
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                    ORBGPU_JACOBI_UNROLL
                    for (int r = 0; r < 4; r++) {
                        if (r != p && r != q) {
                            const double arp = A[r][p], arq = A[r][q];
                            const double np = c * arp - s * arq, nq = s * arp + c * arq;
                            A[r][p] = A[p][r] = np;
                            A[r][q] = A[q][r] = nq;
                        }
                        const double vrp = V[r][p], vrq = V[r][q];
                        V[r][p] = c * vrp - s * vrq;
                        V[r][q] = s * vrp + c * vrq;
                    }
                    A[p][p] = app - t * apq, A[q][q] = aqq + t * apq;
                    A[p][q] = A[q][p] = 0.0;
                }
            }
    }
}

// A'A of the float 4 x 4 A, accumulated in FP64 in row order, and after jacobi4_lane the eigenvector of the least
// eigenvalue: the last of the stable descending order, with the sign rule (the entry of largest magnitude, the first
// among equals, is positive), rounded to float.  The triangulation of k_init_checkrt (I9) and of new_points.hip (N5).
ORBGPU_JACOBI_HD inline void null_vector4(const float (&Af)[4][4], float (&x4)[4])
{
    double A[4][4], V[4][4];
    ORBGPU_JACOBI_UNROLL
    for (int a = 0; a < 4; a++)
        ORBGPU_JACOBI_UNROLL
        for (int b = 0; b < 4; b++) {
            double s = 0.0;
            ORBGPU_JACOBI_UNROLL
            for (int r = 0; r < 4; r++)
                s = s + (double)Af[r][a] * (double)Af[r][b];
            A[a][b] = s;
        }
    jacobi4_lane<NULL_VECTOR4_SWEEPS>(A, V);
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    ORBGPU_JACOBI_UNROLL
    for (int i = 0; i < 4; i++) {
        int rank = 0;
        ORBGPU_JACOBI_UNROLL
        for (int j = 0; j < 4; j++)
            rank += j < i ? !(A[j][j] < A[i][i]) : (j > i ? A[j][j] > A[i][i] : 0);
        if (rank >= 3)
            v[0] = V[0][i], v[1] = V[1][i], v[2] = V[2][i], v[3] = V[3][i];
    }
    double big = fabs(v[0]), lead = v[0];
    ORBGPU_JACOBI_UNROLL
    for (int r = 1; r < 4; r++)
        if (fabs(v[r]) > big)
            big = fabs(v[r]), lead = v[r];
    const bool flip = lead < 0.0;
    x4[0] = (float)(flip ? -v[0] : v[0]), x4[1] = (float)(flip ? -v[1] : v[1]);
    x4[2] = (float)(flip ? -v[2] : v[2]), x4[3] = (float)(flip ? -v[3] : v[3]);
}

#if defined(__HIPCC__)
// The wave-wide form, one wave per workgroup.  Lds has double A[], V[], Ut[] (m x m, row stride LD) and w[] in LDS.
// Cyclic Jacobi on the symmetric m x m in S.A, at most SWEEPS sweeps; eigenvalues stay on its diagonal, eigenvectors in the
// columns of S.V.  Every lane computes the rotation's c, s, t from the same three entries; lane r < m updates row r of A (and
// the mirrored column entries), lane 16 + r row r of V: the entries of one rotation do not depend on each other.
template <int LD, int SWEEPS, class Lds> __device__ void jacobi_wave(Lds &S, int m, int lane)
{
    for (int e = lane; e < m * m; e += 64)
        S.V[(e / m) * LD + e % m] = (e / m == e % m) ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < SWEEPS; sweep++) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < m; p++)
            for (int q = p + 1; q < m; q++)
                off = off + S.A[p * LD + q] * S.A[p * LD + q];
        for (int i = 0; i < m; i++)
            diag = diag + S.A[i * LD + i] * S.A[i * LD + i];
        if (off <= JACOBI_STOP * (diag + 2.0 * off))
            break;
        for (int p = 0; p < m; p++)
            for (int q = p + 1; q < m; q++) {
                const double apq = S.A[p * LD + q];
                if (apq == 0.0)
                    continue;
                const double app = S.A[p * LD + p], aqq = S.A[q * LD + q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double den = fabs(theta) + sqrt(theta * theta + 1.0);
                const double t = theta >= 0.0 ? 1.0 / den : -1.0 / den;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                __syncthreads();
                if (lane < m) {
                    const int r = lane;
                    if (r == p) {
                        S.A[p * LD + p] = app - t * apq;
                        S.A[p * LD + q] = 0.0;
                    } else if (r == q) {
                        S.A[q * LD + q] = aqq + t * apq;
                        S.A[q * LD + p] = 0.0;
                    } else {
                        const double arp = S.A[r * LD + p], arq = S.A[r * LD + q];
                        const double np = c * arp - s * arq, nq = s * arp + c * arq;
                        S.A[r * LD + p] = S.A[p * LD + r] = np;
                        S.A[r * LD + q] = S.A[q * LD + r] = nq;
                    }
                } else if (lane >= 16 && lane < 16 + m) {
                    const int r = lane - 16;
                    const double vrp = S.V[r * LD + p], vrq = S.V[r * LD + q];
                    S.V[r * LD + p] = c * vrp - s * vrq;
                    S.V[r * LD + q] = s * vrp + c * vrq;
                }
                __syncthreads();
            }
    }
    __syncthreads();
}

// Eigenvalues descending (stable) into S.w, eigenvectors as rows of S.Ut, each flipped so that its component of largest
// magnitude (lowest index on ties) is positive.
template <int LD, int SWEEPS, class Lds> __device__ void sorted_eig_wave(Lds &S, int m, int lane)
{
    jacobi_wave<LD, SWEEPS>(S, m, lane);
    if (lane < m) {
        const double wi = S.A[lane * LD + lane];
        int rank = 0;
        for (int j = 0; j < m; j++) {
            const double wj = S.A[j * LD + j];
            rank += j < lane ? !(wj < wi) : (j > lane ? wj > wi : 0);
        }
        rank = min(rank, m - 1);
        double big = fabs(S.V[lane]), lead = S.V[lane];
        for (int r = 1; r < m; r++) {
            const double v = S.V[r * LD + lane];
            if (fabs(v) > big)
                big = fabs(v), lead = v;
        }
        const bool flip = lead < 0.0;
        for (int r = 0; r < m; r++) {
            const double v = S.V[r * LD + lane];
            S.Ut[rank * LD + r] = flip ? -v : v;
        }
        S.w[rank] = wi;
    }
    __syncthreads();
}
#endif  // __HIPCC__

} // namespace orbgpu

// The per-lane 4 x 4 symmetric eigen-solver of the triangulations (convention I9 of the Initializer, N5 of
// CreateNewMapPoints): initializer.hip and new_points.hip must give the same null vector for the same A'A.  jacobi4_lane is
// shared; null_vector4 is new_points.hip's, and restates the steps k_init_checkrt has inline around its jacobi4_lane call
// (calling it from there changed that kernel's register allocation).
#pragma once

#include "common.h"

namespace orbgpu {

constexpr int INIT_JACOBI_SWEEPS = 30;
constexpr double INIT_JACOBI_STOP = 1e-32;

// Cyclic Jacobi of a symmetric 4 x 4 in the registers of one lane: the same pairs, rotations and stopping rule as
// jacobi_wave.  Lanes diverge only in how many sweeps they need.
__device__ inline void jacobi4_lane(double (&A)[4][4], double (&V)[4][4])
{
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
            V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < INIT_JACOBI_SWEEPS; sweep++) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++)
                off = off + A[p][q] * A[p][q];
#pragma unroll
        for (int i = 0; i < 4; i++)
            diag = diag + A[i][i] * A[i][i];
        if (off <= INIT_JACOBI_STOP * (diag + 2.0 * off))
            break;
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                const double apq = A[p][q];
                if (!(apq == 0.0)) {
                    const double app = A[p][p], aqq = A[q][q];
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double den = fabs(theta) + sqrt(theta * theta + 1.0);
                    const double t = theta >= 0.0 ? 1.0 / den : -1.0 / den;
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
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
// among equals, is positive), rounded to float.
__device__ inline void null_vector4(const float (&Af)[4][4], float (&x4)[4])
{
    double A[4][4], V[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            double s = 0.0;
#pragma unroll
            for (int r = 0; r < 4; r++)
                s = s + (double)Af[r][a] * (double)Af[r][b];
            A[a][b] = s;
        }
    jacobi4_lane(A, V);
    double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < 4; j++)
            rank += j < i ? !(A[j][j] < A[i][i]) : (j > i ? A[j][j] > A[i][i] : 0);
        if (rank >= 3)
            v[0] = V[0][i], v[1] = V[1][i], v[2] = V[2][i], v[3] = V[3][i];
    }
    double big = fabs(v[0]), lead = v[0];
#pragma unroll
    for (int r = 1; r < 4; r++)
        if (fabs(v[r]) > big)
            big = fabs(v[r]), lead = v[r];
    const bool flip = lead < 0.0;
    x4[0] = (float)(flip ? -v[0] : v[0]), x4[1] = (float)(flip ? -v[1] : v[1]);
    x4[2] = (float)(flip ? -v[2] : v[2]), x4[3] = (float)(flip ? -v[3] : v[3]);
}

} // namespace orbgpu

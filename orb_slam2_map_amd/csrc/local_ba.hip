// Optimizer::LocalBundleAdjustment (Optimizer.cc:453-778) on the device: the poses of the local key frames and the points
// they see, over every observation of those points, by Levenberg-Marquardt on the Schur complement (g2o's BlockSolver_6_3
// restated, "g2o unpinned").  One workgroup per problem runs both rounds and every trial without returning to the host; the
// definition (L1-L12) is in include/orbgpu.h and tests/lba_model.py.  FP64 throughout, no fused multiply-add
// (-ffp-contract=off): the per-edge, per-pair and per-vertex arithmetic is the model's operation for operation; the sums per
// point run edge by edge as the model's do, the sums per pose, per block of the reduced system and over the workgroup as
// per-lane partial sums and a fixed tree.
//
// Optimizer::BundleAdjustment / GlobalBundleAdjustemnt (Optimizer.cc:41-237; B1-B7, tests/ba_model.py) is the same loop in
// another round structure -- one optimize(n_iterations) over every key frame and point of a map, no classification -- and
// shares this file's kernel text (lm_problem<FULL>) and host side; DESIGN.md 9.27.
//
// Memory: everything of a problem whose size follows its edges or points (the sorted edges, both copies of the state, Hll,
// bl, Hll^-1, Hpl, the index lists) lives in the call's global workspace; only the reduced camera system S (lower triangle,
// packed) with its three vectors lives in LDS, when the problem has at most LBA_LDS_POSES free poses.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "carve.h"
#include "common.h"
#include "opt_edges.h"
#include "opt_math.h"
#include "staging.h"

namespace orbgpu {

// First guesses, not tuned shapes: the only timing so far is the first run of tools/bench_lba.py
// (profiles/lba_times.json); no alternative has been measured against them.
// 8 waves: the passes over points and edges are one thread each, the passes over poses and blocks of S one wave each.
constexpr int LBA_THREADS = 512;
constexpr int LBA_WAVES = LBA_THREADS / 64;
// S of 6 * 28 = 168 rows is 14196 doubles, with 3 * 168 of vectors 115 KiB of the 160 KiB a gfx950 workgroup has; the rest
// (reduction scratch) is under 1 KiB
constexpr int LBA_LDS_POSES = 28;
constexpr int LBA_LDS_ROWS = 6 * LBA_LDS_POSES;
constexpr int LBA_LDS_TRI = LBA_LDS_ROWS * (LBA_LDS_ROWS + 1) / 2;
constexpr unsigned LBA_STEREO = 1u, LBA_LEVEL1 = 2u;
constexpr int LBA_POSE_STRIDE = 16;  // q[4], t[3], R[9]

struct LbaEdge {  // sorted by point row, then in the caller's order
    int32_t point, pose, orig;
    uint32_t flags;
    float x, y, ur, w;
};

struct LbaProblemDev {
    LbaEdge *edges;              // [ne]
    const int32_t *point_start;  // [M + 1] into edges
    const int32_t *free_of;      // [P] slot in the reduced system, or -1
    const int32_t *free_row;     // [nf] pose row of a slot
    const int32_t *pose_start;   // [nf + 1] into pose_edges
    const int32_t *pose_edges;   // edges that end at a free pose, by slot, then in edge order
    const int32_t *blk_start;    // [nf (nf + 1) / 2 + 1] into pairs; block (f1, f2), f1 >= f2, is f1 (f1 + 1) / 2 + f2
    const int2 *pairs;           // (e1, e2): same point, slot(e1) = f1, slot(e2) = f2; by point, e1, e2
    const double *cam;           // [P][5]
    double *pose[2];             // [P][LBA_POSE_STRIDE]: the kept state and the trial's; q and t of [0] uploaded
    double *X[2];                // [M][3]
    double *Hll, *bl, *inv;      // [M][6], [M][3], [M][9]
    double *Hpp, *bp;            // [nf][21], [nf][6]
    double *Hpl;                 // [ne][18]
    double *S, *vec;             // the reduced system outside LDS: [tri(6 nf)], [18 nf]
    uint8_t *pt_on, *fr_on;      // [M], [nf]: the vertex has a level-0 edge
    const int32_t *stop;
    double *Tcw_d, *pos_d;
    float *Tcw, *pos;
    uint8_t *erase;
    orbgpu_local_ba_result *result;
    int32_t *spill_count;
    int32_t P, nl, M, ne, nf, n_bad_index, in_lds;
    double delta[2], delta2[2];
    // Optimizer::BundleAdjustment only (k_bundle_adjustment): nl = P there, erase and result are null
    uint8_t *not_included;  // [M]
    orbgpu_bundle_adjustment_result *ba_result;
    int32_t n_iterations, robust, n_not_included;
};

// error of edge E at a state; returns chi2, C and R of its pose
__device__ inline double eval_edge(const LbaProblemDev &P, const LbaEdge &E, const double *poses, const double *X, Cam &C,
                                   const double *&R, double er[3], double Pc[3])
{
    const double *ps = poses + (size_t)E.pose * LBA_POSE_STRIDE, *c = P.cam + 5 * (size_t)E.pose, *x = X + 3 * (size_t)E.point;
    C = Cam{c[0], c[1], c[2], c[3], c[4]};
    R = ps + 7;
    return edge_error(R, ps + 4, C, x[0], x[1], x[2], (double)E.w, (double)E.x, (double)E.y, (double)E.ur,
                      (E.flags & LBA_STEREO) != 0, er, Pc);
}

// robust chi2 of the level-0 edges at a state
__device__ inline double robust_chi(const LbaProblemDev &P, const double *poses, const double *X, bool use_kernel, double *red)
{
    double part[1] = {0.0};
    for (int e = threadIdx.x; e < P.ne; e += LBA_THREADS) {
        const LbaEdge E = P.edges[e];
        if (E.flags & LBA_LEVEL1)
            continue;
        Cam C;
        const double *R;
        double er[3], Pc[3], rho0, rho1;
        const double chi2 = eval_edge(P, E, poses, X, C, R, er, Pc);
        const int st = E.flags & LBA_STEREO;
        huber(chi2, P.delta[st], P.delta2[st], rho0, rho1, use_kernel);
        part[0] += rho0;
    }
    block_sum<LBA_WAVES>(part, red);
    return part[0];
}

// L7 / L8: chi2 over the threshold or depth not positive, for every edge at a state; to_level: set the edges' level,
// else write erase.  Returns the number of edges that failed.
__device__ inline int classify(const LbaProblemDev &P, const double *poses, const double *X, bool to_level, int *icount)
{
    __syncthreads();
    if (threadIdx.x == 0)
        *icount = 0;
    __syncthreads();
    int mine = 0;
    for (int e = threadIdx.x; e < P.ne; e += LBA_THREADS) {
        LbaEdge E = P.edges[e];
        Cam C;
        const double *R;
        double er[3], Pc[3];
        const double chi2 = eval_edge(P, E, poses, X, C, R, er, Pc);
        const bool bad = chi2 > ((E.flags & LBA_STEREO) ? 7.815 : 5.991) || !(Pc[2] > 0.0);
        if (to_level)
            P.edges[e].flags = bad ? (E.flags | LBA_LEVEL1) : (E.flags & ~LBA_LEVEL1);
        else
            P.erase[E.orig] = bad ? 1 : 0;
        mine += bad ? 1 : 0;
    }
    mine = wave_reduce_add(mine);
    if ((threadIdx.x & 63) == 0 && mine)
        atomicAdd(icount, mine);
    __syncthreads();
    return *icount;
}

// The one text of the Levenberg-Marquardt loop.  What the two optimisers differ in is a template argument, so that each
// kernel compiles its round structure from constants:
//   FULL = false  Optimizer::LocalBundleAdjustment (L1-L12): optimize(5) with Huber, classify, optimize(10) without, erase
//   FULL = true   Optimizer::BundleAdjustment (B1-B7): ONE optimize(P.n_iterations), Huber iff P.robust, no classification;
//                 not_included per point and the poses of every row (P.nl = P.P) out
template <bool FULL>
__device__ __forceinline__ void lm_problem(const LbaProblemDev &P)
{
    __shared__ double S_lds[LBA_LDS_TRI];
    __shared__ double vec_lds[3 * LBA_LDS_ROWS];
    __shared__ double red[LBA_WAVES];
    __shared__ int flag, icount;
    constexpr int N_ROUNDS = FULL ? 1 : 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = 6 * P.nf, nblk = P.nf * (P.nf + 1) / 2;
    double *S = P.in_lds ? S_lds : P.S;
    double *vec = P.in_lds ? vec_lds : P.vec;  // [n] right-hand side / solution, [2 n] work of the solve

    // Everything below that steers control flow (the flag, lam, nu, rho, the counters, which copy of the state is kept) is
    // the same in every lane -- broadcast through LDS or computed from block_sum / block_max results -- so the barriers
    // inside the loops are reached by all lanes.  Trip counts are bounded by the constants of the definition: 5 + 10
    // iterations (FULL: n_iterations <= ORBGPU_BA_MAX_ITERATIONS, checked on the host) of at most 10 trials.
    if (stop_requested(P.stop, &flag)) {  // Optimizer.cc:655
        if (tid == 0) {
            if constexpr (FULL) {
                orbgpu_bundle_adjustment_result r{};
                r.n_edges = P.ne, r.n_bad_index = P.n_bad_index, r.stopped = 1, r.reduced_in_lds = P.in_lds;
                r.n_not_included = P.n_not_included;
                *P.ba_result = r;
            } else {
                orbgpu_local_ba_result r{};
                r.n_edges = P.ne, r.n_bad_index = P.n_bad_index, r.stopped = 1, r.reduced_in_lds = P.in_lds;
                *P.result = r;
            }
        }
        return;
    }
    if (tid == 0 && !P.in_lds)
        atomicAdd(P.spill_count, 1);
    for (int i = tid; i < P.P; i += LBA_THREADS)
        quat_to_matrix(P.pose[0] + (size_t)i * LBA_POSE_STRIDE, P.pose[0] + (size_t)i * LBA_POSE_STRIDE + 7);
    __syncthreads();

    int kept = 0;  // P.pose[kept], P.X[kept]: the state
    int rounds = 0, stopped = 0, iterations[2] = {0, 0}, trials[2] = {0, 0};
    double chi_start[2] = {0.0, 0.0}, chi_end[2] = {0.0, 0.0};
    bool use_kernel = FULL ? P.robust != 0 : true;
    for (int rnd = 0; rnd < N_ROUNDS && !stopped; rnd++) {
        if (!FULL && rnd == 1) {
            if (stop_requested(P.stop, &flag)) {  // Optimizer.cc:664: bDoMore = false
                stopped = 1;
                break;
            }
            (void)classify(P, P.pose[kept], P.X[kept], true, &icount);
            use_kernel = false;
        }
        // the active vertices of this round (g2o's initializeOptimization(0))
        for (int p = tid; p < P.M; p += LBA_THREADS) {
            uint8_t on = 0;
            for (int e = P.point_start[p]; e < P.point_start[p + 1]; e++)
                on |= (P.edges[e].flags & LBA_LEVEL1) ? 0 : 1;
            P.pt_on[p] = on;
        }
        for (int f = tid; f < P.nf; f += LBA_THREADS) {
            uint8_t on = 0;
            for (int k = P.pose_start[f]; k < P.pose_start[f + 1]; k++)
                on |= (P.edges[P.pose_edges[k]].flags & LBA_LEVEL1) ? 0 : 1;
            P.fr_on[f] = on;
        }
        __syncthreads();

        double lam = 0.0, nu = 2.0, cur = 0.0;
        const int n_it = FULL ? P.n_iterations : (rnd == 0 ? 5 : 10);
        if (FULL && n_it == 0)  // B4: nothing runs; both chi2 members are the input's
            chi_start[rnd] = cur = robust_chi(P, P.pose[kept], P.X[kept], use_kernel, red);
        for (int it = 0; it < n_it; it++) {
            if (stop_requested(P.stop, &flag)) {
                stopped = 1;
                break;
            }
            const double *poses = P.pose[kept], *X = P.X[kept];
            // ---- L4: the blocks of the normal equation at the kept state ----
            for (int p = tid; p < P.M; p += LBA_THREADS) {
                if (!P.pt_on[p])
                    continue;
                double h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
                for (int e = P.point_start[p]; e < P.point_start[p + 1]; e++) {
                    const LbaEdge E = P.edges[e];
                    if (E.flags & LBA_LEVEL1)
                        continue;
                    Cam C;
                    const double *R;
                    double er[3], Pc[3], rho0, rho1, Jp[3][3];
                    const bool stereo = E.flags & LBA_STEREO;
                    const double chi2 = eval_edge(P, E, poses, X, C, R, er, Pc);
                    huber(chi2, P.delta[stereo], P.delta2[stereo], rho0, rho1, use_kernel);
                    const double s = (double)E.w * rho1;
                    point_jacobian(Pc, R, C, stereo, Jp);
                    double Jpw[3][3];
#pragma unroll
                    for (int r = 0; r < 3; r++)
#pragma unroll
                        for (int a = 0; a < 3; a++)
                            Jpw[r][a] = Jp[r][a] * s;
                    int k = 0;
#pragma unroll
                    for (int a = 0; a < 3; a++)
#pragma unroll
                        for (int c = a; c < 3; c++, k++)
                            h[k] = h[k] + ((Jpw[0][a] * Jp[0][c] + Jpw[1][a] * Jp[1][c]) + Jpw[2][a] * Jp[2][c]);
#pragma unroll
                    for (int a = 0; a < 3; a++)
                        b[a] = b[a] + -((Jpw[0][a] * er[0] + Jpw[1][a] * er[1]) + Jpw[2][a] * er[2]);
                    if (P.free_of[E.pose] >= 0) {
                        double Jc[3][6];
                        pose_jacobian(Pc, C, stereo, Jc);
                        double *W = P.Hpl + 18 * (size_t)e;
#pragma unroll
                        for (int a = 0; a < 6; a++) {
                            const double w0 = Jc[0][a] * s, w1 = Jc[1][a] * s, w2 = Jc[2][a] * s;
#pragma unroll
                            for (int c = 0; c < 3; c++)
                                W[3 * a + c] = (w0 * Jp[0][c] + w1 * Jp[1][c]) + w2 * Jp[2][c];
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < 6; k++)
                    P.Hll[6 * (size_t)p + k] = h[k];
#pragma unroll
                for (int a = 0; a < 3; a++)
                    P.bl[3 * (size_t)p + a] = b[a];
            }
            for (int f = wave; f < P.nf; f += LBA_WAVES) {
                if (!P.fr_on[f])
                    continue;
                double acc[27];
#pragma unroll
                for (int k = 0; k < 27; k++)
                    acc[k] = 0.0;
                for (int k = P.pose_start[f] + lane; k < P.pose_start[f + 1]; k += 64) {
                    const LbaEdge E = P.edges[P.pose_edges[k]];
                    if (E.flags & LBA_LEVEL1)
                        continue;
                    Cam C;
                    const double *R;
                    double er[3], Pc[3], rho0, rho1, J[3][6], Jw[3][6];
                    const bool stereo = E.flags & LBA_STEREO;
                    const double chi2 = eval_edge(P, E, poses, X, C, R, er, Pc);
                    huber(chi2, P.delta[stereo], P.delta2[stereo], rho0, rho1, use_kernel);
                    const double s = (double)E.w * rho1;
                    pose_jacobian(Pc, C, stereo, J);
#pragma unroll
                    for (int r = 0; r < 3; r++)
#pragma unroll
                        for (int a = 0; a < 6; a++)
                            Jw[r][a] = J[r][a] * s;
                    int q = 0;
#pragma unroll
                    for (int a = 0; a < 6; a++)
#pragma unroll
                        for (int c = a; c < 6; c++, q++)
                            acc[q] += (Jw[0][a] * J[0][c] + Jw[1][a] * J[1][c]) + Jw[2][a] * J[2][c];
#pragma unroll
                    for (int a = 0; a < 6; a++)
                        acc[21 + a] += -((Jw[0][a] * er[0] + Jw[1][a] * er[1]) + Jw[2][a] * er[2]);
                }
                wave_sum(acc);
                if (lane == 0) {
#pragma unroll
                    for (int k = 0; k < 21; k++)
                        P.Hpp[21 * (size_t)f + k] = acc[k];
#pragma unroll
                    for (int a = 0; a < 6; a++)
                        P.bp[6 * (size_t)f + a] = acc[21 + a];
                }
            }
            __syncthreads();
            if (it == 0) {  // lambda0 = 1e-5 max |diag| over Hpp and Hll of the active vertices
                double m = 0.0;
                for (int f = tid; f < P.nf; f += LBA_THREADS)
                    if (P.fr_on[f])
                        for (int a = 0, k = 0; a < 6; k += 6 - a, a++) {
                            const double d = fabs(P.Hpp[21 * (size_t)f + k]);
                            if (d > m)
                                m = d;
                        }
                for (int p = tid; p < P.M; p += LBA_THREADS)
                    if (P.pt_on[p])
                        for (int a = 0, k = 0; a < 3; k += 3 - a, a++) {
                            const double d = fabs(P.Hll[6 * (size_t)p + k]);
                            if (d > m)
                                m = d;
                        }
                lam = 1e-5 * block_max<LBA_WAVES>(m, red);
                nu = 2.0;
            }
            cur = robust_chi(P, poses, X, use_kernel, red);
            if (it == 0)
                chi_start[rnd] = cur;
            double rho = 0.0;
            int trial = 0;
            bool stop = false;
            iterations[rnd]++;
            do {
                if (stop_requested(P.stop, &flag)) {
                    stopped = 1;
                    break;
                }
                double *poses_n = P.pose[kept ^ 1], *X_n = P.X[kept ^ 1];
                // ---- L5: Hll^-1, then the reduced system ----
                for (int p = tid; p < P.M; p += LBA_THREADS)
                    if (P.pt_on[p])
                        inv3_sym(P.Hll + 6 * (size_t)p, lam, P.inv + 9 * (size_t)p);
                __syncthreads();
                for (int blk = wave; blk < nblk; blk += LBA_WAVES) {
                    int f1 = (int)((sqrt(8.0 * (double)blk + 1.0) - 1.0) * 0.5);
                    while ((f1 + 1) * (f1 + 2) / 2 <= blk)
                        f1++;
                    while (f1 * (f1 + 1) / 2 > blk)
                        f1--;
                    const int f2 = blk - f1 * (f1 + 1) / 2;
                    double T[36];
#pragma unroll
                    for (int k = 0; k < 36; k++)
                        T[k] = 0.0;
                    for (int k = P.blk_start[blk] + lane; k < P.blk_start[blk + 1]; k += 64) {
                        const int2 pr = P.pairs[k];
                        const LbaEdge E1 = P.edges[pr.x];
                        if ((E1.flags | P.edges[pr.y].flags) & LBA_LEVEL1)
                            continue;
                        const double *W1 = P.Hpl + 18 * (size_t)pr.x, *W2 = P.Hpl + 18 * (size_t)pr.y;
                        const double *iv = P.inv + 9 * (size_t)E1.point;
                        double w2[18];
#pragma unroll
                        for (int i = 0; i < 18; i++)
                            w2[i] = W2[i];
#pragma unroll
                        for (int a = 0; a < 6; a++) {
                            double Y[3];
#pragma unroll
                            for (int c = 0; c < 3; c++)
                                Y[c] = (W1[3 * a] * iv[c] + W1[3 * a + 1] * iv[3 + c]) + W1[3 * a + 2] * iv[6 + c];
#pragma unroll
                            for (int c = 0; c < 6; c++)
                                T[6 * a + c] += (Y[0] * w2[3 * c] + Y[1] * w2[3 * c + 1]) + Y[2] * w2[3 * c + 2];
                        }
                    }
                    wave_sum(T);
                    if (lane == 0) {
                        if (f1 != f2) {
#pragma unroll
                            for (int a = 0; a < 6; a++)
#pragma unroll
                                for (int c = 0; c < 6; c++)
                                    S[tri_at(6 * f1 + a, 6 * f2 + c)] = 0.0 - T[6 * a + c];
                        } else if (P.fr_on[f1]) {
                            const double *H = P.Hpp + 21 * (size_t)f1;
#pragma unroll
                            for (int a = 0; a < 6; a++)
#pragma unroll
                                for (int c = 0; c <= a; c++) {
                                    double A = H[c * 6 - c * (c - 1) / 2 + (a - c)];
                                    if (a == c)
                                        A = A + lam;
                                    S[tri_at(6 * f1 + a, 6 * f1 + c)] = A - T[6 * a + c];
                                }
                        } else {  // a free pose without a level-0 edge: x = 0, coupled to nothing
#pragma unroll
                            for (int a = 0; a < 6; a++)
#pragma unroll
                                for (int c = 0; c <= a; c++)
                                    S[tri_at(6 * f1 + a, 6 * f1 + c)] = a == c ? 1.0 : 0.0;
                        }
                    }
                }
                for (int f = wave; f < P.nf; f += LBA_WAVES) {
                    double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                    const bool on = P.fr_on[f];
                    for (int k = P.pose_start[f] + lane; on && k < P.pose_start[f + 1]; k += 64) {
                        const int e = P.pose_edges[k];
                        const LbaEdge E = P.edges[e];
                        if (E.flags & LBA_LEVEL1)
                            continue;
                        const double *W = P.Hpl + 18 * (size_t)e, *iv = P.inv + 9 * (size_t)E.point;
                        const double *b = P.bl + 3 * (size_t)E.point;
#pragma unroll
                        for (int a = 0; a < 6; a++) {
                            double Y[3];
#pragma unroll
                            for (int c = 0; c < 3; c++)
                                Y[c] = (W[3 * a] * iv[c] + W[3 * a + 1] * iv[3 + c]) + W[3 * a + 2] * iv[6 + c];
                            g[a] += (Y[0] * b[0] + Y[1] * b[1]) + Y[2] * b[2];
                        }
                    }
                    wave_sum(g);
                    if (lane == 0)
#pragma unroll
                        for (int a = 0; a < 6; a++)
                            vec[6 * f + a] = on ? P.bp[6 * (size_t)f + a] - g[a] : 0.0;
                }
                __syncthreads();
                const bool ok = llt_solve(n, S, vec, vec + n, tid, LBA_THREADS, WorkgroupBarrier());
                __syncthreads();
                // ---- the increments, the trial state and x'(lambda x + b) ----
                double part[1] = {0.0};
                for (int i = tid; i < P.P; i += LBA_THREADS) {
                    const double *ps = poses + (size_t)i * LBA_POSE_STRIDE;
                    double *pn = poses_n + (size_t)i * LBA_POSE_STRIDE;
                    const int f = P.free_of[i];
                    if (f >= 0 && P.fr_on[f]) {
                        double x[6];
#pragma unroll
                        for (int a = 0; a < 6; a++) {
                            x[a] = vec[6 * f + a];
                            part[0] = part[0] + x[a] * (lam * x[a] + P.bp[6 * (size_t)f + a]);
                        }
                        pose_update(ps, ps + 4, x, pn, pn + 4);
                        quat_to_matrix(pn, pn + 7);
                    } else {
#pragma unroll
                        for (int k = 0; k < LBA_POSE_STRIDE; k++)
                            pn[k] = ps[k];
                    }
                }
                for (int p = tid; p < P.M; p += LBA_THREADS) {
                    const double *x0 = X + 3 * (size_t)p;
                    double *xn = X_n + 3 * (size_t)p;
                    if (!P.pt_on[p]) {
                        xn[0] = x0[0], xn[1] = x0[1], xn[2] = x0[2];
                        continue;
                    }
                    double t[3] = {0.0, 0.0, 0.0};
                    for (int e = P.point_start[p]; e < P.point_start[p + 1]; e++) {
                        const LbaEdge E = P.edges[e];
                        const int f = P.free_of[E.pose];
                        if ((E.flags & LBA_LEVEL1) || f < 0)
                            continue;
                        const double *W = P.Hpl + 18 * (size_t)e;
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            double v = W[c] * vec[6 * f];
#pragma unroll
                            for (int a = 1; a < 6; a++)
                                v = v + W[3 * a + c] * vec[6 * f + a];
                            t[c] = t[c] + v;
                        }
                    }
                    const double *b = P.bl + 3 * (size_t)p, *iv = P.inv + 9 * (size_t)p;
                    const double r[3] = {b[0] - t[0], b[1] - t[1], b[2] - t[2]};
                    double xl[3];
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        xl[c] = ok ? (iv[3 * c] * r[0] + iv[3 * c + 1] * r[1]) + iv[3 * c + 2] * r[2] : 0.0;
                        part[0] = part[0] + xl[c] * (lam * xl[c] + b[c]);
                    }
                    point_update(x0, xl, xn);
                }
                __syncthreads();
                block_sum<LBA_WAVES>(part, red);
                const double chi_n = robust_chi(P, poses_n, X_n, use_kernel, red);
                const double tmp = ok ? chi_n : DBL_MAX;
                const double scale = part[0] + 1e-3;
                trials[rnd]++;
                if (lm_trial(cur, tmp, scale, lam, nu, rho, stop)) {
                    kept ^= 1;
                    cur = tmp;
                }
                trial++;
            } while (!stop && rho < 0 && trial < 10);
            if (stopped || trial == 10 || rho == 0 || stop)
                break;
        }
        chi_end[rnd] = cur;
        rounds = rnd + 1;
    }

    // ---- L8, L12 ----
    int n_erased = 0;
    if constexpr (FULL) {
        for (int p = tid; p < P.M; p += LBA_THREADS)  // B4: vbNotIncludedMP
            P.not_included[p] = P.pt_on[p] ? 0 : 1;
    } else {
        n_erased = classify(P, P.pose[kept], P.X[kept], false, &icount);
    }
    for (int i = tid; i < P.nl; i += LBA_THREADS) {
        const double *ps = P.pose[kept] + (size_t)i * LBA_POSE_STRIDE, *R = ps + 7, *t = ps + 4;
        const double T[16] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0.0, 0.0, 0.0, 1.0};
        for (int k = 0; k < 16; k++) {
            P.Tcw_d[16 * (size_t)i + k] = T[k];
            P.Tcw[16 * (size_t)i + k] = (float)T[k];
        }
    }
    for (int k = tid; k < 3 * P.M; k += LBA_THREADS) {
        const double v = P.X[kept][k];
        P.pos_d[k] = v;
        P.pos[k] = (float)v;
    }
    if (tid == 0) {
        if constexpr (FULL) {
            orbgpu_bundle_adjustment_result r{};
            r.chi2_start = chi_start[0], r.chi2_end = chi_end[0];
            r.n_edges = P.ne, r.iterations = iterations[0], r.trials = trials[0], r.stopped = stopped;
            r.n_bad_index = P.n_bad_index, r.n_not_included = P.n_not_included, r.reduced_in_lds = P.in_lds;
            *P.ba_result = r;
        } else {
            orbgpu_local_ba_result r{};
            for (int k = 0; k < 2; k++) {
                r.chi2_start[k] = chi_start[k], r.chi2_end[k] = chi_end[k];
                r.iterations[k] = iterations[k], r.trials[k] = trials[k];
            }
            r.n_edges = P.ne, r.n_erased = n_erased, r.rounds = rounds, r.stopped = stopped, r.n_bad_index = P.n_bad_index;
            r.reduced_in_lds = P.in_lds;
            *P.result = r;
        }
    }
}

__global__ __launch_bounds__(LBA_THREADS) void k_local_ba(const LbaProblemDev *__restrict__ problems)
{
    lm_problem<false>(problems[blockIdx.x]);
}

__global__ __launch_bounds__(LBA_THREADS) void k_bundle_adjustment(const LbaProblemDev *__restrict__ problems)
{
    lm_problem<true>(problems[blockIdx.x]);
}

// Per (thread, device) staging of the entry points (staging.h): PROBLEMS and WORK are the device flavours' (the problem
// records; the uploaded index structure and state followed by the kernel's scratch), the stream and the H_* buffers the
// host flavour's.
enum { PROBLEMS, WORK, SPILL_COUNT, H_OUT, H_STOP, N_BUF };
struct LbaWs : Staging<N_BUF> {
    // what the device flavours upload: kept until the thread's next call, which is ordered after this one on its stream
    std::vector<char> blob;
    std::vector<LbaProblemDev> records;
};
struct BaWs : LbaWs {};  // Optimizer::BundleAdjustment's: its calls and its spill count are its own

// The host side takes either optimiser's problem as an orbgpu_local_ba_problem (BundleAdjustment: every row local, no erase)
// with the capacities of its entry point; what only BundleAdjustment has is read from its own structure.
struct LbaCaps {
    int poses, free, points, edges;
};
constexpr LbaCaps LBA_CAPS{ORBGPU_LBA_MAX_POSES, ORBGPU_LBA_MAX_FREE, ORBGPU_LBA_MAX_POINTS, ORBGPU_LBA_MAX_EDGES};
constexpr LbaCaps BA_CAPS{ORBGPU_BA_MAX_POSES, ORBGPU_BA_MAX_FREE, ORBGPU_BA_MAX_POINTS, ORBGPU_BA_MAX_EDGES};

static orbgpu_local_ba_problem as_local(const orbgpu_bundle_adjustment_problem &b)
{
    orbgpu_local_ba_problem p{};
    p.n_poses = p.n_local = b.n_poses, p.n_points = b.n_points, p.n_edges = b.n_edges, p.nlevels = b.nlevels;
    p.Tcw = b.Tcw, p.fixed = b.fixed, p.cam = b.cam, p.inv_level_sigma2 = b.inv_level_sigma2, p.world_pos = b.world_pos;
    p.edge_point = b.edge_point, p.edge_pose = b.edge_pose, p.edge_octave = b.edge_octave;
    p.edge_xy = b.edge_xy, p.edge_u_right = b.edge_u_right;
    p.d_stop = b.d_stop, p.d_Tcw_d = b.d_Tcw_d, p.d_Tcw = b.d_Tcw, p.d_pos_d = b.d_pos_d, p.d_pos = b.d_pos;
    return p;
}

static int check_problem(const orbgpu_local_ba_problem &p, int k, const LbaCaps &caps = LBA_CAPS)
{
    ORBGPU_REQUIRE(p.n_poses >= 0 && p.n_local >= 0 && p.n_points >= 0 && p.n_edges >= 0, "problem %d: negative count", k);
    ORBGPU_REQUIRE(p.n_local <= p.n_poses, "problem %d: more local key frames than pose rows", k);
    ORBGPU_REQUIRE(p.nlevels >= 1 && p.nlevels <= ORBGPU_MAX_LEVELS, "problem %d: nlevels outside [1, %d]", k,
                   ORBGPU_MAX_LEVELS);
    ORBGPU_REQUIRE(p.n_poses <= caps.poses, "problem %d: more than %d pose rows", k, caps.poses);
    ORBGPU_REQUIRE(p.n_points <= caps.points, "problem %d: more than %d points", k, caps.points);
    ORBGPU_REQUIRE(p.n_edges <= caps.edges, "problem %d: more than %d edges", k, caps.edges);
    ORBGPU_REQUIRE(p.n_poses == 0 || (p.Tcw && p.cam && p.inv_level_sigma2), "problem %d: null pose arrays", k);
    ORBGPU_REQUIRE(p.n_local == 0 || p.fixed, "problem %d: null fixed array", k);
    ORBGPU_REQUIRE(p.n_points == 0 || p.world_pos, "problem %d: null point array", k);
    ORBGPU_REQUIRE(p.n_edges == 0 || (p.edge_point && p.edge_pose && p.edge_octave && p.edge_xy && p.edge_u_right),
                   "problem %d: null edge arrays", k);
    int nf = 0;
    for (int i = 0; i < p.n_local; i++)
        nf += p.fixed[i] ? 0 : 1;
    ORBGPU_REQUIRE(nf <= caps.free, "problem %d: %d free poses, more than %d", k, nf, caps.free);
    return ORBGPU_OK;
}

static int check_problem(const orbgpu_bundle_adjustment_problem &b, int k)
{
    ORBGPU_REQUIRE(b.n_iterations >= 0 && b.n_iterations <= ORBGPU_BA_MAX_ITERATIONS, "problem %d: n_iterations outside [0, %d]",
                   k, ORBGPU_BA_MAX_ITERATIONS);
    return check_problem(as_local(b), k, BA_CAPS);
}

static int check_device_outputs(const orbgpu_local_ba_problem &p, int k)
{
    int rc = check_problem(p, k);
    if (rc != ORBGPU_OK)
        return rc;
    ORBGPU_REQUIRE(p.d_result && (p.n_local == 0 || (p.d_Tcw_d && p.d_Tcw)) && (p.n_points == 0 || (p.d_pos_d && p.d_pos)) &&
                       (p.n_edges == 0 || p.d_erase),
                   "problem %d: null output", k);
    return ORBGPU_OK;
}

static int check_device_outputs(const orbgpu_bundle_adjustment_problem &b, int k)
{
    int rc = check_problem(b, k);
    if (rc != ORBGPU_OK)
        return rc;
    ORBGPU_REQUIRE(b.d_result && (b.n_poses == 0 || (b.d_Tcw_d && b.d_Tcw)) &&
                       (b.n_points == 0 || (b.d_pos_d && b.d_pos && b.d_not_included)),
                   "problem %d: null output", k);
    return ORBGPU_OK;
}

// The index structure of one problem (L10's fixed orders), built on the host
struct LbaIndex {
    std::vector<LbaEdge> edges;
    std::vector<int32_t> point_start, free_of, free_row, pose_start, pose_edges, blk_start;
    std::vector<int2> pairs;
    int n_bad_index = 0;
};

static int build_index(const orbgpu_local_ba_problem &p, int k, LbaIndex &ix)
{
    const int M = p.n_points, Pn = p.n_poses;
    ix.free_of.assign((size_t)Pn, -1);
    ix.free_row.clear();
    for (int i = 0; i < p.n_local; i++)
        if (!p.fixed[i]) {
            ix.free_of[i] = (int32_t)ix.free_row.size();
            ix.free_row.push_back(i);
        }
    const int nf = (int)ix.free_row.size();
    // edges by point, the caller's order within a point (counting sort)
    ix.point_start.assign((size_t)M + 1, 0);
    ix.n_bad_index = 0;
    auto taken = [&](int e) {
        const int pt = p.edge_point[e], ps = p.edge_pose[e], o = p.edge_octave[e];
        return pt >= 0 && pt < M && ps >= 0 && ps < Pn && o >= 0 && o < p.nlevels;
    };
    for (int e = 0; e < p.n_edges; e++) {
        if (taken(e))
            ix.point_start[(size_t)p.edge_point[e] + 1]++;
        else
            ix.n_bad_index++;
    }
    for (int i = 0; i < M; i++)
        ix.point_start[i + 1] += ix.point_start[i];
    const int ne = ix.point_start[M];
    ix.edges.assign((size_t)ne, LbaEdge{});
    {
        std::vector<int32_t> at(ix.point_start.begin(), ix.point_start.end() - 1);
        for (int e = 0; e < p.n_edges; e++) {
            if (!taken(e))
                continue;
            LbaEdge E{};
            E.point = p.edge_point[e], E.pose = p.edge_pose[e], E.orig = e;
            E.x = p.edge_xy[2 * (size_t)e], E.y = p.edge_xy[2 * (size_t)e + 1], E.ur = p.edge_u_right[e];
            E.flags = E.ur < 0.f ? 0u : LBA_STEREO;
            E.w = p.inv_level_sigma2[(size_t)E.pose * p.nlevels + p.edge_octave[e]];
            ix.edges[(size_t)at[E.point]++] = E;
        }
    }
    // per free pose, its edges in sorted order
    ix.pose_start.assign((size_t)nf + 1, 0);
    for (const LbaEdge &E : ix.edges)
        if (ix.free_of[E.pose] >= 0)
            ix.pose_start[(size_t)ix.free_of[E.pose] + 1]++;
    for (int f = 0; f < nf; f++)
        ix.pose_start[f + 1] += ix.pose_start[f];
    ix.pose_edges.assign((size_t)ix.pose_start[nf], 0);
    {
        std::vector<int32_t> at(ix.pose_start.begin(), ix.pose_start.end() - 1);
        for (int e = 0; e < ne; e++) {
            const int f = ix.free_of[ix.edges[e].pose];
            if (f >= 0)
                ix.pose_edges[(size_t)at[f]++] = e;
        }
    }
    // per block (f1 >= f2) of the reduced system, the pairs of edges that share a point: by point, e1, e2
    const int nblk = nf * (nf + 1) / 2;
    std::vector<int64_t> count((size_t)nblk + 1, 0);
    auto for_each_pair = [&](auto &&fn) {
        for (int pt = 0; pt < M; pt++)
            for (int e1 = ix.point_start[pt]; e1 < ix.point_start[pt + 1]; e1++) {
                const int f1 = ix.free_of[ix.edges[e1].pose];
                if (f1 < 0)
                    continue;
                for (int e2 = ix.point_start[pt]; e2 < ix.point_start[pt + 1]; e2++) {
                    const int f2 = ix.free_of[ix.edges[e2].pose];
                    if (f2 >= 0 && f1 >= f2)
                        fn(f1 * (f1 + 1) / 2 + f2, e1, e2);
                }
            }
    };
    for_each_pair([&](int blk, int, int) { count[(size_t)blk + 1]++; });
    for (int b = 0; b < nblk; b++)
        count[b + 1] += count[b];
    ORBGPU_REQUIRE(count[nblk] <= (int64_t)ORBGPU_LBA_MAX_PAIRS, "problem %d: %lld edge pairs between free poses, more than %d",
                   k, (long long)count[nblk], ORBGPU_LBA_MAX_PAIRS);
    ix.blk_start.assign(count.begin(), count.end());
    ix.pairs.assign((size_t)count[nblk], int2{0, 0});
    {
        std::vector<int32_t> at(ix.blk_start.begin(), ix.blk_start.end() - 1);
        for_each_pair([&](int blk, int e1, int e2) { ix.pairs[(size_t)at[blk]++] = int2{e1, e2}; });
    }
    return ORBGPU_OK;
}

// Both *_batch_device entry points after their checks: n > 0 problems on the bound workspace ws; full: the
// BundleAdjustment structures the problems were taken from, or null for LocalBundleAdjustment.
static int enqueue(int32_t n, const orbgpu_local_ba_problem *problems, const orbgpu_bundle_adjustment_problem *full, LbaWs &ws,
                   void *hip_stream)
{
    int rc = ORBGPU_OK;
    // ORBGPU_DEBUG_LBA_LDS_POSES=<k> (tests): problems with more than k free poses keep the reduced system in global memory
    const int lds_poses = debug_limit("ORBGPU_DEBUG_LBA_LDS_POSES", LBA_LDS_POSES);
    std::vector<LbaIndex> ix((size_t)n);
    for (int k = 0; k < n; k++)
        if ((rc = build_index(problems[k], k, ix[k])) != ORBGPU_OK)
            return rc;
    // The workspace (carve.h's WorkPlan): every buffer of problem k is named here, once
    auto describe = [&](int k, WorkPlan &plan, LbaProblemDev &D) {
        const orbgpu_local_ba_problem &p = problems[k];
        const LbaIndex &I = ix[k];
        const size_t Pn = (size_t)p.n_poses, M = (size_t)p.n_points, nf = I.free_row.size(), ne = I.edges.size(), rows = 6 * nf;
        const bool in_lds = (int)nf <= lds_poses;
        double *cam, *pose, *X;  // filled in place below; null while the plan only measures
        D.edges = plan.seg(ne, I.edges.data());
        D.point_start = plan.seg(I.point_start.size(), I.point_start.data());
        D.free_of = plan.seg(I.free_of.size(), I.free_of.data());
        D.free_row = plan.seg(nf, I.free_row.data());
        D.pose_start = plan.seg(I.pose_start.size(), I.pose_start.data());
        D.pose_edges = plan.seg(I.pose_edges.size(), I.pose_edges.data());
        D.blk_start = plan.seg(I.blk_start.size(), I.blk_start.data());
        D.pairs = plan.seg(I.pairs.size(), I.pairs.data());
        D.cam = plan.seg_in_place(5 * Pn, cam);
        D.pose[0] = plan.seg_in_place(LBA_POSE_STRIDE * Pn, pose);
        D.X[0] = plan.seg_in_place(3 * M, X);
        D.pose[1] = plan.seg<double>(LBA_POSE_STRIDE * Pn);
        D.X[1] = plan.seg<double>(3 * M);
        D.Hll = plan.seg<double>(6 * M);
        D.bl = plan.seg<double>(3 * M);
        D.inv = plan.seg<double>(9 * M);
        D.Hpp = plan.seg<double>(21 * nf);
        D.bp = plan.seg<double>(6 * nf);
        D.Hpl = plan.seg<double>(18 * ne);
        D.S = plan.seg<double>(in_lds ? 0 : rows * (rows + 1) / 2);
        D.vec = plan.seg<double>(in_lds ? 0 : 3 * rows);
        D.pt_on = plan.seg<uint8_t>(M);
        D.fr_on = plan.seg<uint8_t>(nf);
        if (!cam)
            return;
        for (int i = 0; i < p.n_poses; i++) {
            for (int c = 0; c < 5; c++)
                cam[5 * (size_t)i + c] = (double)p.cam[5 * (size_t)i + c];
            // Converter::toSE3Quat (Converter.cc:37-47): float 3x3 -> double -> unit quaternion, float t -> double
            double *q = pose + (size_t)i * LBA_POSE_STRIDE;
            unit_quat_from_floats(p.Tcw + 16 * (size_t)i, 4, q);
            for (int r = 0; r < 3; r++)
                q[4 + r] = (double)p.Tcw[16 * (size_t)i + 4 * r + 3];
        }
        for (size_t i = 0; i < 3 * M; i++)
            X[i] = (double)p.world_pos[i];
    };
    WorkPlan measured;
    for (int k = 0; k < n; k++) {
        LbaProblemDev unused{};
        describe(k, measured, unused);
    }
    ws.reserve(PROBLEMS, sizeof(LbaProblemDev) * (size_t)n);
    ws.reserve(WORK, measured.total());
    ws.reserve(SPILL_COUNT, sizeof(int32_t));
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    std::vector<char> &blob = ws.blob;
    std::vector<LbaProblemDev> &hp = ws.records;
    const size_t upload_bytes = measured.upload_bytes();
    blob.assign(upload_bytes, 0);
    hp.assign((size_t)n, LbaProblemDev{});
    char *dev = ws.as<char>(WORK);
    WorkPlan plan(measured, dev, blob.data());
    for (int k = 0; k < n; k++) {
        const orbgpu_local_ba_problem &p = problems[k];
        const LbaIndex &I = ix[k];
        LbaProblemDev &D = hp[k];
        describe(k, plan, D);
        D.stop = p.d_stop;
        D.Tcw_d = p.d_Tcw_d, D.Tcw = p.d_Tcw, D.pos_d = p.d_pos_d, D.pos = p.d_pos, D.erase = p.d_erase, D.result = p.d_result;
        D.spill_count = ws.as<int32_t>(SPILL_COUNT);
        D.P = p.n_poses, D.nl = p.n_local, D.M = p.n_points, D.ne = (int32_t)I.edges.size(), D.nf = (int32_t)I.free_row.size();
        D.n_bad_index = I.n_bad_index;
        D.in_lds = D.nf <= lds_poses ? 1 : 0;
        D.delta[0] = (double)(float)std::sqrt(full ? 5.99 : 5.991), D.delta[1] = (double)(float)std::sqrt(7.815);
        if (full) {
            D.not_included = full[k].d_not_included, D.ba_result = full[k].d_result;
            D.n_iterations = full[k].n_iterations, D.robust = full[k].robust;
            for (int i = 0; i < p.n_points; i++)
                D.n_not_included += I.point_start[i + 1] == I.point_start[i] ? 1 : 0;
        }
        D.delta2[0] = D.delta[0] * D.delta[0], D.delta2[1] = D.delta[1] * D.delta[1];
    }
    const hipStream_t st = (hipStream_t)hip_stream;
    ORBGPU_HIP_TRY(hipMemsetAsync(ws.buf[SPILL_COUNT].p, 0, sizeof(int32_t), st));
    ORBGPU_HIP_TRY(hipMemcpyAsync(ws.buf[PROBLEMS].p, hp.data(), sizeof(LbaProblemDev) * (size_t)n, hipMemcpyHostToDevice, st));
    if (upload_bytes)
        ORBGPU_HIP_TRY(hipMemcpyAsync(dev, blob.data(), upload_bytes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(full ? k_bundle_adjustment : k_local_ba, dim3(n), dim3(LBA_THREADS), 0, st,
                       ws.as<LbaProblemDev>(PROBLEMS));
    ORBGPU_HIP_TRY(hipGetLastError());
    return ORBGPU_OK;
}

} // namespace orbgpu

using namespace orbgpu;

extern "C" int orbgpu_local_ba_batch_device(int32_t n, const orbgpu_local_ba_problem *problems, int32_t device_id,
                                            void *hip_stream)
{
    LbaWs *wsp;
    int rc = batch_begin(n, problems, static_cast<int (*)(const orbgpu_local_ba_problem &, int)>(check_device_outputs), device_id,
                         wsp);
    if (rc != ORBGPU_OK || !wsp)
        return rc;
    return enqueue(n, problems, nullptr, *wsp, hip_stream);
}

extern "C" int orbgpu_local_ba_device(const orbgpu_local_ba_problem *p, int32_t device_id, void *hip_stream)
{
    ORBGPU_REQUIRE(p, "null argument");
    return orbgpu_local_ba_batch_device(1, p, device_id, hip_stream);
}

extern "C" int orbgpu_local_ba_last_spills(int32_t device_id, int32_t *problems_spilled)
{
    return last_spills<LbaWs>(device_id, SPILL_COUNT, "no local bundle adjustment recorded on this thread", problems_spilled);
}

// The host flavour of either bundle adjustment: the stop flag as sampled now, and one staging block for the outputs -- all
// in/out, so that what a stopped call or a skipped edge leaves alone goes back as it came.  `flag` is erase [n_edges] or
// not_included [n_points], at the problem's member d_flag; `batch` the family's *_batch_device.
template <typename Ws, typename Problem, typename Result>
static int ba_host(const Problem &p, size_t n_rows, uint8_t *flag, size_t n_flag, uint8_t *Problem::*d_flag,
                   int (*batch)(int32_t, const Problem *, int32_t, void *), const int32_t *stop, double *Tcw_d, float *Tcw,
                   double *pos_d, float *pos, Result *result, int32_t device_id)
{
    const int32_t stop_now = stop ? *stop : 0;
    Result r;
    HostPlan<N_BUF> plan;
    const auto i_stop = plan.in(H_STOP, &stop_now, 1);
    const auto o_res = plan.out(H_OUT, &r, 1);
    const auto o_Td = plan.inout(H_OUT, Tcw_d, n_rows, 16);
    const auto o_T = plan.inout(H_OUT, Tcw, n_rows, 16);
    const auto o_Xd = plan.inout(H_OUT, pos_d, (size_t)p.n_points, 3);
    const auto o_X = plan.inout(H_OUT, pos, (size_t)p.n_points, 3);
    const auto o_flag = plan.inout(H_OUT, flag, n_flag);
    Ws *wsp;
    int rc = host_begin(device_id, plan, wsp);
    if (rc != ORBGPU_OK)
        return rc;
    Ws &ws = *wsp;
    typename Ws::FinishOnError on_error{ws};
    plan.upload(ws);
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    Problem d = p;
    d.d_stop = stop ? ws.at(i_stop) : nullptr;
    d.d_Tcw_d = ws.at(o_Td), d.d_Tcw = ws.at(o_T), d.d_pos_d = ws.at(o_Xd), d.d_pos = ws.at(o_X);
    d.*d_flag = ws.at(o_flag), d.d_result = ws.at(o_res);
    if ((rc = batch(1, &d, device_id, ws.stream)) != ORBGPU_OK)
        return rc;
    plan.download(ws);
    if ((rc = ws.finish()) != ORBGPU_OK)
        return rc;
    if (result)
        *result = r;
    return ORBGPU_OK;
}

extern "C" int orbgpu_local_ba(const orbgpu_local_ba_problem *p, const int32_t *stop, double *Tcw_d, float *Tcw, double *pos_d,
                               float *pos, uint8_t *erase, orbgpu_local_ba_result *result, int32_t device_id)
{
    ORBGPU_REQUIRE(p, "null argument");
    int rc = check_problem(*p, 0);
    if (rc != ORBGPU_OK)
        return rc;
    ORBGPU_REQUIRE((p->n_local == 0 || Tcw) && (p->n_points == 0 || pos) && (p->n_edges == 0 || erase), "null output");
    return ba_host<LbaWs>(*p, (size_t)p->n_local, erase, (size_t)p->n_edges, &orbgpu_local_ba_problem::d_erase,
                          orbgpu_local_ba_batch_device, stop, Tcw_d, Tcw, pos_d, pos, result, device_id);
}

// ---- Optimizer::BundleAdjustment / GlobalBundleAdjustemnt (B1-B7): the same host side over the other kernel ----------------
extern "C" int orbgpu_bundle_adjustment_batch_device(int32_t n, const orbgpu_bundle_adjustment_problem *problems, int32_t device_id,
                                                     void *hip_stream)
{
    BaWs *wsp;
    int rc = batch_begin(n, problems, static_cast<int (*)(const orbgpu_bundle_adjustment_problem &, int)>(check_device_outputs),
                         device_id, wsp);
    if (rc != ORBGPU_OK || !wsp)
        return rc;
    std::vector<orbgpu_local_ba_problem> local((size_t)n);
    for (int k = 0; k < n; k++)
        local[k] = as_local(problems[k]);
    return enqueue(n, local.data(), problems, *wsp, hip_stream);
}

extern "C" int orbgpu_bundle_adjustment_device(const orbgpu_bundle_adjustment_problem *p, int32_t device_id, void *hip_stream)
{
    ORBGPU_REQUIRE(p, "null argument");
    return orbgpu_bundle_adjustment_batch_device(1, p, device_id, hip_stream);
}

extern "C" int orbgpu_bundle_adjustment_last_spills(int32_t device_id, int32_t *problems_spilled)
{
    return last_spills<BaWs>(device_id, SPILL_COUNT, "no bundle adjustment recorded on this thread", problems_spilled);
}

extern "C" int orbgpu_bundle_adjustment(const orbgpu_bundle_adjustment_problem *p, const int32_t *stop, double *Tcw_d, float *Tcw,
                                        double *pos_d, float *pos, uint8_t *not_included,
                                        orbgpu_bundle_adjustment_result *result, int32_t device_id)
{
    ORBGPU_REQUIRE(p, "null argument");
    int rc = check_problem(*p, 0);
    if (rc != ORBGPU_OK)
        return rc;
    ORBGPU_REQUIRE((p->n_poses == 0 || Tcw) && (p->n_points == 0 || (pos && not_included)), "null output");
    return ba_host<BaWs>(*p, (size_t)p->n_poses, not_included, (size_t)p->n_points,
                         &orbgpu_bundle_adjustment_problem::d_not_included, orbgpu_bundle_adjustment_batch_device, stop, Tcw_d, Tcw,
                         pos_d, pos, result, device_id);
}

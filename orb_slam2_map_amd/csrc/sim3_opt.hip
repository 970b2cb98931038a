// Optimizer::OptimizeSim3 (Optimizer.cc:1079-1236) on the device: 7-DoF refinement of ONE Sim3 over N correspondences, two
// reprojection edges each.  One workgroup per loop candidate runs both stages and every Levenberg-Marquardt trial without
// returning to the host; the definition (g2o restated, "g2o unpinned", conventions O1-O9) is in include/orbgpu.h and
// tests/sim3opt_model.py.  FP64 throughout, no fused multiply-add (-ffp-contract=off): the per-edge arithmetic is the
// model's operation for operation, only the order of the sums over edges differs (fixed tree here, sequential there).
// The quaternions, the Huber weights, the Cholesky solve, the initial damping and the reduction tree are opt_math.h's,
// shared with pose_opt.hip; exp(x) * S (O4, O5) is sim3_math.h's, shared with essential_graph.hip.  make_xf, pair_errors
// and write_result keep their own inverse and map, on the Xf form the edges read, and the decision on a trial is
// opt_math.h's lm_trial written out: calling it cost one row of tools/bench_sim3opt.py more than the parent's spread
// (DESIGN.md 9.29).  The two compaction passes are written out here and in pose_opt.hip, because moving them changed the
// generated code.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "carve.h"
#include "common.h"
#include "opt_math.h"
#include "sim3_math.h"
#include "staging.h"

namespace orbgpu {
namespace sim3opt {

constexpr int SO_THREADS = 256;               // 4 waves, the shape of k_pose_opt: a first guess, not a tuned one
constexpr int SO_WAVES = SO_THREADS / 64;
constexpr int SO_LDS_PAIRS = 768;             // 64 B per correspondence -> 48 KiB of LDS; more go through the global spill
constexpr int SO_REC = 4;                     // float4 per correspondence
constexpr int SO_SUMS = 36;                   // 28 of symmetric H, 7 of b, 1 robust chi2
constexpr int SO_STATES = 15;                 // the state and exp(+-d 1_k) * state, k = 0..6
constexpr int SO_XF = 17;                     // doubles per transform: R, t, s, 1 / s, t of the inverse
constexpr int SO_MAX_N1 = 65536;
constexpr double SO_DELTA = 1e-9;             // O6

struct Sim3OptProblemDev {
    const uint8_t *valid;
    const float *Xw1, *Xw2;
    const int32_t *octave1, *octave2;
    const float *kp1, *kp2;
    uint8_t *inlier;
    orbgpu_sim3_opt_result *result;
    float4 *spill;        // [SO_REC * n1], or nullptr when n1 <= lds_pairs
    int32_t *spill_count; // problems of this call that took the spill path (diagnostic)
    int32_t n1, nlevels, lds_pairs, fix_scale;
    float T1w[12], T2w[12];
    float inv_sigma2[ORBGPU_MAX_LEVELS];
    double K1[4], K2[4];  // fx, fy, cx, cy
    double q0[4], t0[3], s0;  // the entry state (O4)
    double qmw[4], tmw[3];    // Smw (O9)
    double th2, delta, delta2;
};

// a Sim3 and its inverse in the form the edges use them
struct Xf {
    double R[9], t[3], s, is, ti[3];
};

__device__ inline void make_xf(const double q[4], const double t[3], double s, Xf &F)
{
    quat_to_matrix(q, F.R);
    F.s = s;
    F.is = 1.0 / s;
    const double u0 = -F.is * t[0], u1 = -F.is * t[1], u2 = -F.is * t[2];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        F.t[r] = t[r];
        F.ti[r] = (F.R[r] * u0 + F.R[3 + r] * u1) + F.R[6 + r] * u2;
    }
}

__device__ inline void store_xf(const Xf &F, double *o)
{
#pragma unroll
    for (int i = 0; i < 9; i++)
        o[i] = F.R[i];
#pragma unroll
    for (int i = 0; i < 3; i++)
        o[9 + i] = F.t[i], o[14 + i] = F.ti[i];
    o[12] = F.s, o[13] = F.is;
}

__device__ inline void load_xf(const double *o, Xf &F)
{
#pragma unroll
    for (int i = 0; i < 9; i++)
        F.R[i] = o[i];
#pragma unroll
    for (int i = 0; i < 3; i++)
        F.t[i] = o[9 + i], F.ti[i] = o[14 + i];
    F.s = o[12], F.is = o[13];
}

// ---- one correspondence ------------------------------------------------------------------------------------------------
struct Pair {
    double X1[3], X2[3], o1[2], o2[2], w1, w2;
};

__device__ inline void load_pair(const float4 *E, int c, Pair &p)
{
    const float4 a = E[SO_REC * c], b = E[SO_REC * c + 1], o = E[SO_REC * c + 2];
    p.X1[0] = (double)a.x, p.X1[1] = (double)a.y, p.X1[2] = (double)a.z, p.w1 = (double)a.w;
    p.X2[0] = (double)b.x, p.X2[1] = (double)b.y, p.X2[2] = (double)b.z, p.w2 = (double)b.w;
    p.o1[0] = (double)o.x, p.o1[1] = (double)o.y, p.o2[0] = (double)o.z, p.o2[1] = (double)o.w;
}

// e12 = obs1 - cam1(S X2c), e21 = obs2 - cam2(S^-1 X1c)  (O3)
__device__ inline void pair_errors(const Xf &F, const double K1[4], const double K2[4], const Pair &p, double e12[2],
                                   double e21[2])
{
    double P[3], Q[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double a = (F.R[3 * r] * p.X2[0] + F.R[3 * r + 1] * p.X2[1]) + F.R[3 * r + 2] * p.X2[2];
        P[r] = F.s * a + F.t[r];
        const double b = (F.R[r] * p.X1[0] + F.R[3 + r] * p.X1[1]) + F.R[6 + r] * p.X1[2];
        Q[r] = F.is * b + F.ti[r];
    }
    e12[0] = p.o1[0] - ((P[0] / P[2]) * K1[0] + K1[2]);
    e12[1] = p.o1[1] - ((P[1] / P[2]) * K1[1] + K1[3]);
    e21[0] = p.o2[0] - ((Q[0] / Q[2]) * K2[0] + K2[2]);
    e21[1] = p.o2[1] - ((Q[1] / Q[2]) * K2[1] + K2[3]);
}

// one edge's share of H (upper triangle, row-major), b and the robust chi2
__device__ inline void accumulate(double (&acc)[SO_SUMS], const double J[2][7], const double e[2], double w, double delta,
                                  double delta2)
{
    const double chi2 = w * (e[0] * e[0] + e[1] * e[1]);
    double rho0, rho1;
    huber(chi2, delta, delta2, rho0, rho1);
    const double s = w * rho1;
    double Jw[2][7];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int a = 0; a < 7; a++)
            Jw[r][a] = J[r][a] * s;
    int k = 0;
#pragma unroll
    for (int a = 0; a < 7; a++)
#pragma unroll
        for (int c = a; c < 7; c++, k++)
            acc[k] += Jw[0][a] * J[0][c] + Jw[1][a] * J[1][c];
#pragma unroll
    for (int a = 0; a < 7; a++)
        acc[28 + a] += -(Jw[0][a] * e[0] + Jw[1][a] * e[1]);
    acc[35] += rho0;
}

// row i is a correspondence (1), a valid row with an octave out of range (2), or nothing (0)  (O1)
__device__ inline int pair_kind(const Sim3OptProblemDev &P, int i)
{
    if (i >= P.n1 || !P.valid[i])
        return 0;
    const int o1 = P.octave1[i], o2 = P.octave2[i];
    return (o1 < 0 || o1 >= P.nlevels || o2 < 0 || o2 >= P.nlevels) ? 2 : 1;
}

// O9, by one lane
__device__ inline void write_result(const Sim3OptProblemDev &P, const double q[4], const double t[3], double s, int n,
                                    int n_bad, int n_inliers, int stages, int iterations, int trials, int nbadidx)
{
    orbgpu_sim3_opt_result *r = P.result;
    double R[9], qc[4], Rc[9];
    quat_to_matrix(q, R);
    quat_mul(q, P.qmw, qc);
    quat_to_matrix(qc, Rc);
    for (int i = 0; i < 9; i++) {
        r->R12_d[i] = R[i];
        r->R12[i] = (float)R[i];
    }
    r->s12_d = s;
    r->s12 = (float)s;
    for (int a = 0; a < 3; a++) {
        r->t12_d[a] = t[a];
        r->t12[a] = (float)t[a];
        const double tc = s * ((R[3 * a] * P.tmw[0] + R[3 * a + 1] * P.tmw[1]) + R[3 * a + 2] * P.tmw[2]) + t[a];
        for (int c = 0; c < 3; c++) {
            r->T12[4 * a + c] = (float)(s * R[3 * a + c]);
            r->Scw[4 * a + c] = (float)((s * 1.0) * Rc[3 * a + c]);
        }
        r->T12[4 * a + 3] = (float)t[a];
        r->Scw[4 * a + 3] = (float)tc;
        r->T12[12 + a] = 0.f;
        r->Scw[12 + a] = 0.f;
    }
    r->T12[15] = 1.f;
    r->Scw[15] = 1.f;
    r->n_correspondences = n, r->n_bad = n_bad, r->n_inliers = n_inliers, r->stages = stages;
    r->iterations = iterations, r->trials = trials, r->n_bad_index = nbadidx;
}

__global__ __launch_bounds__(SO_THREADS) void k_sim3_opt(const Sim3OptProblemDev *__restrict__ problems)
{
    __shared__ float4 lds_rec[SO_REC * SO_LDS_PAIRS];
    __shared__ double red[SO_WAVES * SO_SUMS];
    __shared__ double xf[SO_STATES][SO_XF];
    __shared__ int wcount[SO_WAVES][2];
    __shared__ int icount;
    const Sim3OptProblemDev &P = problems[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n1 = P.n1;

    // pass 1: count the correspondences (decides LDS or spill) and the skipped rows
    int N = 0, nbadidx = 0;
    for (int base = 0; base < n1; base += SO_THREADS) {
        const int kind = pair_kind(P, base + tid);
        const unsigned long long m1 = __ballot(kind == 1), m2 = __ballot(kind == 2);
        __syncthreads();
        if (lane == 0)
            wcount[wave][0] = __popcll(m1), wcount[wave][1] = __popcll(m2);
        __syncthreads();
#pragma unroll
        for (int wv = 0; wv < SO_WAVES; wv++)
            N += wcount[wv][0], nbadidx += wcount[wv][1];
    }
    // N <= n1, and the host gives every problem with n1 > lds_pairs a spill block of SO_REC * n1 records
    const bool spilled = N > P.lds_pairs;
    float4 *E = spilled ? P.spill : lds_rec;

    // pass 2: compact the correspondences in index order (O1, O2); each starts as an inlier
    {
        int at = 0;
        for (int base = 0; base < n1; base += SO_THREADS) {
            const int i = base + tid;
            const bool is_pair = pair_kind(P, i) == 1;
            const unsigned long long m1 = __ballot(is_pair);
            __syncthreads();
            if (lane == 0)
                wcount[wave][0] = __popcll(m1);
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int wv = 0; wv < SO_WAVES; wv++) {
                before += wv < wave ? wcount[wv][0] : 0;
                total += wcount[wv][0];
            }
            if (is_pair) {
                const int e = at + before + __popcll(m1 & ((1ull << lane) - 1ull));
                const float *A = P.Xw1 + 3 * (size_t)i, *B = P.Xw2 + 3 * (size_t)i;
                float x1[3], x2[3];
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    x1[r] = ((P.T1w[4 * r] * A[0] + P.T1w[4 * r + 1] * A[1]) + P.T1w[4 * r + 2] * A[2]) + P.T1w[4 * r + 3];
                    x2[r] = ((P.T2w[4 * r] * B[0] + P.T2w[4 * r + 1] * B[1]) + P.T2w[4 * r + 2] * B[2]) + P.T2w[4 * r + 3];
                }
                E[SO_REC * e] = make_float4(x1[0], x1[1], x1[2], P.inv_sigma2[P.octave1[i]]);
                E[SO_REC * e + 1] = make_float4(x2[0], x2[1], x2[2], P.inv_sigma2[P.octave2[i]]);
                E[SO_REC * e + 2] = make_float4(P.kp1[2 * (size_t)i], P.kp1[2 * (size_t)i + 1], P.kp2[2 * (size_t)i],
                                                P.kp2[2 * (size_t)i + 1]);
                E[SO_REC * e + 3] = make_float4(__int_as_float(i), __int_as_float(1), 0.f, 0.f);
                P.inlier[i] = 1;
            }
            at += total;
        }
    }
    __syncthreads();

    double q[4], t[3], s = P.s0;
#pragma unroll
    for (int i = 0; i < 4; i++)
        q[i] = P.q0[i];
#pragma unroll
    for (int i = 0; i < 3; i++)
        t[i] = P.t0[i];
    if (N == 0) {  // O8: returns 0, nothing written to inlier[]
        if (tid == 0)
            write_result(P, q, t, s, 0, 0, 0, 0, 0, 0, nbadidx);
        return;
    }
    if (tid == 0 && spilled)
        atomicAdd(P.spill_count, 1);

    // Everything below that steers control flow (lam, nu, rho, the state, the counters) is computed redundantly by every
    // lane from block_sum results or read from LDS after a barrier, hence workgroup-uniform: the barriers inside the loops
    // are reached by all lanes.  Trip counts are bounded by the constants of the definition: 2 stages x <= 10 iterations x
    // <= 10 trials.
    const double delta = P.delta, delta2 = P.delta2, th2 = P.th2;
    const bool fix_scale = P.fix_scale != 0;
    const double inv2d = 1.0 / (2.0 * SO_DELTA);
    int iterations = 0, trials = 0, n_bad = 0, n_in = 0;
    for (int stage = 0; stage < 2; stage++) {
        const int budget = stage == 0 ? 5 : (n_bad > 0 ? 10 : 5);
        double lam = 0.0, nu = 2.0;
        for (int it = 0; it < budget; it++) {
            // the state and the 14 perturbed states of the numeric Jacobian (O6), one lane each, shared through LDS
            __syncthreads();  // the previous linearisation's readers are done with `xf`
            if (tid < SO_STATES) {
                Xf F;
                if (tid == 0) {
                    make_xf(q, t, s, F);
                } else {
                    const int k = (tid - 1) >> 1;
                    const double d = (tid - 1) & 1 ? -SO_DELTA : SO_DELTA;
                    double x[7], qn[4], tn[3], sn;
#pragma unroll
                    for (int a = 0; a < 7; a++)
                        x[a] = a == k ? d : 0.0;
                    sim3_update(q, t, s, x, fix_scale, qn, tn, sn);
                    make_xf(qn, tn, sn, F);
                }
                store_xf(F, xf[tid]);
            }
            __syncthreads();
            double acc[SO_SUMS];
#pragma unroll
            for (int k = 0; k < SO_SUMS; k++)
                acc[k] = 0.0;
            for (int c = tid; c < N; c += SO_THREADS) {
                if (__float_as_int(E[SO_REC * c + 3].y) == 0)
                    continue;
                Pair pr;
                load_pair(E, c, pr);
                Xf F;
                double e12[2], e21[2], J12[2][7] = {}, J21[2][7] = {};
                load_xf(xf[0], F);
                pair_errors(F, P.K1, P.K2, pr, e12, e21);
                // one column per trip, kept rolled: the two transforms of a column are live only inside it, and the column
                // is put in place by selects so that J stays in registers
#pragma unroll 1
                for (int k = 0; k < 7; k++) {
                    double p12[2], p21[2], m12[2], m21[2];
                    load_xf(xf[1 + 2 * k], F);
                    pair_errors(F, P.K1, P.K2, pr, p12, p21);
                    load_xf(xf[2 + 2 * k], F);
                    pair_errors(F, P.K1, P.K2, pr, m12, m21);
#pragma unroll
                    for (int r = 0; r < 2; r++) {
                        const double d12 = (p12[r] - m12[r]) * inv2d, d21 = (p21[r] - m21[r]) * inv2d;
#pragma unroll
                        for (int a = 0; a < 7; a++) {
                            J12[r][a] = a == k ? d12 : J12[r][a];
                            J21[r][a] = a == k ? d21 : J21[r][a];
                        }
                    }
                }
                accumulate(acc, J12, e12, pr.w1, delta, delta2);
                accumulate(acc, J21, e21, pr.w2, delta, delta2);
            }
            block_sum<SO_WAVES>(acc, red);
            double Hu[28], b[7];
#pragma unroll
            for (int k = 0; k < 28; k++)
                Hu[k] = acc[k];
#pragma unroll
            for (int a = 0; a < 7; a++)
                b[a] = acc[28 + a];
            if (it == 0) {
                lam = lm_initial_lambda<7>(Hu);
                nu = 2.0;
            }
            double cur = acc[35], rho = 0.0;
            int trial = 0;
            bool stop = false;
            iterations++;
            do {
                double x[7], qn[4], tn[3], sn;
                const bool ok = cholesky_solve<7>(Hu, lam, b, x);
                sim3_update(q, t, s, x, fix_scale, qn, tn, sn);
                Xf F;
                make_xf(qn, tn, sn, F);
                double part[1] = {0.0};
                for (int c = tid; c < N; c += SO_THREADS) {
                    if (__float_as_int(E[SO_REC * c + 3].y) == 0)
                        continue;
                    Pair pr;
                    load_pair(E, c, pr);
                    double e12[2], e21[2], rho0, rho1;
                    pair_errors(F, P.K1, P.K2, pr, e12, e21);
                    huber(pr.w1 * (e12[0] * e12[0] + e12[1] * e12[1]), delta, delta2, rho0, rho1);
                    part[0] += rho0;
                    huber(pr.w2 * (e21[0] * e21[0] + e21[1] * e21[1]), delta, delta2, rho0, rho1);
                    part[0] += rho0;
                }
                block_sum<SO_WAVES>(part, red);
                const double tmp = ok ? part[0] : DBL_MAX;
                double scale = 0.0;
#pragma unroll
                for (int a = 0; a < 7; a++)
                    scale = scale + x[a] * (lam * x[a] + b[a]);
                scale = scale + 1e-3;
                rho = (cur - tmp) / scale;
                trials++;
                if (rho > 0 && isfinite(tmp)) {
                    const double c3 = 2.0 * rho - 1.0;
                    const double alpha = fmin(1.0 - (c3 * c3) * c3, 2.0 / 3.0);
                    lam = lam * fmax(1.0 / 3.0, alpha);
                    nu = 2.0;
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        q[i] = qn[i];
#pragma unroll
                    for (int i = 0; i < 3; i++)
                        t[i] = tn[i];
                    s = sn;
                    cur = tmp;
                } else {
                    lam = lam * nu;
                    nu = nu * 2.0;
                    if (!isfinite(lam))
                        stop = true;
                }
                trial++;
            } while (!stop && rho < 0 && trial < 10);
            if (trial == 10 || rho == 0 || stop)
                break;
        }
        // classification at the stage's final, kept state (O8)
        Xf F;
        make_xf(q, t, s, F);
        __syncthreads();
        if (tid == 0)
            icount = 0;
        __syncthreads();
        int mine = 0;
        for (int c = tid; c < N; c += SO_THREADS) {
            float4 meta = E[SO_REC * c + 3];
            if (__float_as_int(meta.y) == 0)
                continue;
            Pair pr;
            load_pair(E, c, pr);
            double e12[2], e21[2];
            pair_errors(F, P.K1, P.K2, pr, e12, e21);
            const double c12 = pr.w1 * (e12[0] * e12[0] + e12[1] * e12[1]);
            const double c21 = pr.w2 * (e21[0] * e21[0] + e21[1] * e21[1]);
            if (c12 > th2 || c21 > th2) {
                meta.y = __int_as_float(0);
                E[SO_REC * c + 3] = meta;
                P.inlier[__float_as_int(meta.x)] = 0;
                mine++;
            }
        }
        mine = wave_reduce_add(mine);
        if (lane == 0 && mine)
            atomicAdd(&icount, mine);
        __syncthreads();
        const int cleared = icount;
        if (stage == 0) {
            n_bad = cleared;
            if (N - n_bad < 10) {  // returns 0, S12 untouched: the entry state goes out
                if (tid == 0)
                    write_result(P, P.q0, P.t0, P.s0, N, n_bad, 0, 1, iterations, trials, nbadidx);
                return;
            }
        } else {
            n_in = N - n_bad - cleared;
        }
    }
    if (tid == 0)
        write_result(P, q, t, s, N, n_bad, n_in, 2, iterations, trials, nbadidx);
}

// Per (thread, device) staging of the entry points (staging.h); the stream and the H_* blocks (the uploaded problem and
// its outputs) are the host flavour's.
enum { PROBLEMS, SPILL, SPILL_COUNT, H_IN, H_OUT, N_BUF };
struct Sim3OptWs : Staging<N_BUF> {};

static int check_common(const orbgpu_sim3_opt_problem &p, int k)
{
    ORBGPU_REQUIRE(p.n1 >= 0 && p.n1 <= SO_MAX_N1, "problem %d: n1 outside [0, %d]", k, SO_MAX_N1);
    ORBGPU_REQUIRE(p.nlevels >= 1 && p.nlevels <= ORBGPU_MAX_LEVELS, "problem %d: nlevels outside [1, %d]", k,
                   ORBGPU_MAX_LEVELS);
    ORBGPU_REQUIRE(p.n1 == 0 || (p.valid && p.Xw1 && p.Xw2 && p.octave1 && p.octave2 && p.kp1_xy && p.kp2_xy),
                   "problem %d: null input arrays", k);
    return ORBGPU_OK;
}

static int check_device_problem(const orbgpu_sim3_opt_problem &p, int k)
{
    int rc = check_common(p, k);
    if (rc != ORBGPU_OK)
        return rc;
    ORBGPU_REQUIRE(p.result && (p.n1 == 0 || p.inlier), "problem %d: null output", k);
    return ORBGPU_OK;
}

} // namespace sim3opt
} // namespace orbgpu

using namespace orbgpu;
using namespace orbgpu::sim3opt;

extern "C" int orbgpu_sim3_optimize_batch_device(int32_t n, const orbgpu_sim3_opt_problem *problems, int32_t device_id,
                                                 void *hip_stream)
{
    Sim3OptWs *wsp;
    int rc = batch_begin(n, problems, check_device_problem, device_id, wsp);
    if (rc != ORBGPU_OK || !wsp)
        return rc;
    Sim3OptWs &ws = *wsp;
    // ORBGPU_DEBUG_SIM3OPT_LDS_PAIRS=<k> (tests): problems with more than k correspondences take the global spill path
    const int lds_pairs = debug_limit("ORBGPU_DEBUG_SIM3OPT_LDS_PAIRS", SO_LDS_PAIRS);
    size_t spill_rows = 0;
    for (int k = 0; k < n; k++)
        if (problems[k].n1 > lds_pairs)
            spill_rows += (size_t)problems[k].n1;
    ws.reserve(PROBLEMS, sizeof(Sim3OptProblemDev) * (size_t)n);
    ws.reserve(SPILL, SO_REC * sizeof(float4) * std::max<size_t>(spill_rows, 1));
    ws.reserve(SPILL_COUNT, sizeof(int32_t));
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    std::vector<Sim3OptProblemDev> hp((size_t)n);
    size_t so = 0;
    for (int k = 0; k < n; k++) {
        const orbgpu_sim3_opt_problem &p = problems[k];
        Sim3OptProblemDev &D = hp[k];
        memset(&D, 0, sizeof(D));
        D.valid = p.valid, D.Xw1 = p.Xw1, D.Xw2 = p.Xw2, D.octave1 = p.octave1, D.octave2 = p.octave2;
        D.kp1 = p.kp1_xy, D.kp2 = p.kp2_xy, D.inlier = p.inlier, D.result = p.result;
        D.n1 = p.n1, D.nlevels = p.nlevels, D.lds_pairs = lds_pairs, D.fix_scale = p.fix_scale;
        D.spill_count = ws.as<int32_t>(SPILL_COUNT);
        if (p.n1 > lds_pairs) {
            D.spill = ws.as<float4>(SPILL) + SO_REC * so;
            so += (size_t)p.n1;
        }
        memcpy(D.T1w, p.T1w, sizeof(D.T1w));
        memcpy(D.T2w, p.T2w, sizeof(D.T2w));
        for (int l = 0; l < p.nlevels; l++)
            D.inv_sigma2[l] = p.inv_level_sigma2[l];
        D.K1[0] = (double)p.fx1, D.K1[1] = (double)p.fy1, D.K1[2] = (double)p.cx1, D.K1[3] = (double)p.cy1;
        D.K2[0] = (double)p.fx2, D.K2[1] = (double)p.fy2, D.K2[2] = (double)p.cx2, D.K2[3] = (double)p.cy2;
        // O4: float R12 -> double -> unit quaternion; O9: Smw from the float pose of key frame 2
        unit_quat_from_floats(p.R12, 3, D.q0);
        unit_quat_from_floats(p.T2w, 4, D.qmw);
        for (int r = 0; r < 3; r++) {
            D.t0[r] = (double)p.t12[r];
            D.tmw[r] = (double)p.T2w[4 * r + 3];
        }
        D.s0 = (double)p.s12;
        D.th2 = (double)p.th2;
        D.delta = (double)std::sqrt(p.th2);  // sqrt of the float (Optimizer.cc:1095)
        D.delta2 = D.delta * D.delta;
    }
    const hipStream_t st = (hipStream_t)hip_stream;
    ORBGPU_HIP_TRY(hipMemsetAsync(ws.buf[SPILL_COUNT].p, 0, sizeof(int32_t), st));
    ORBGPU_HIP_TRY(hipMemcpyAsync(ws.buf[PROBLEMS].p, hp.data(), sizeof(Sim3OptProblemDev) * (size_t)n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_sim3_opt, dim3(n), dim3(SO_THREADS), 0, st, ws.as<Sim3OptProblemDev>(PROBLEMS));
    ORBGPU_HIP_TRY(hipGetLastError());
    return ORBGPU_OK;
}

extern "C" int orbgpu_sim3_optimize_device(const orbgpu_sim3_opt_problem *p, int32_t device_id, void *hip_stream)
{
    ORBGPU_REQUIRE(p, "null argument");
    return orbgpu_sim3_optimize_batch_device(1, p, device_id, hip_stream);
}

extern "C" int orbgpu_sim3_opt_last_spills(int32_t device_id, int32_t *problems_spilled)
{
    return last_spills<Sim3OptWs>(device_id, SPILL_COUNT, "no Sim3 optimisation recorded on this thread", problems_spilled);
}

extern "C" int orbgpu_sim3_optimize(const orbgpu_sim3_opt_problem *p, uint8_t *inlier, int32_t *n_inliers,
                                    orbgpu_sim3_opt_result *result, int32_t device_id)
{
    ORBGPU_REQUIRE(p && n_inliers, "null argument");
    int rc = check_common(*p, 0);
    if (rc != ORBGPU_OK)
        return rc;
    ORBGPU_REQUIRE(p->n1 == 0 || inlier, "null inlier array");
    // one staging block each way
    const int n1 = p->n1;
    orbgpu_sim3_opt_result r;
    HostPlan<N_BUF> plan;
    const auto i_valid = plan.in(H_IN, p->valid, n1);
    const auto i_x1 = plan.in(H_IN, p->Xw1, n1, 3), i_x2 = plan.in(H_IN, p->Xw2, n1, 3);
    const auto i_o1 = plan.in(H_IN, p->octave1, n1), i_o2 = plan.in(H_IN, p->octave2, n1);
    const auto i_k1 = plan.in(H_IN, p->kp1_xy, n1, 2), i_k2 = plan.in(H_IN, p->kp2_xy, n1, 2);
    const auto o_res = plan.out(H_OUT, &r, 1);
    const auto o_inl = plan.inout(H_OUT, inlier, n1);
    Sim3OptWs *wsp;
    if ((rc = host_begin(device_id, plan, wsp)) != ORBGPU_OK)
        return rc;
    Sim3OptWs &ws = *wsp;
    Sim3OptWs::FinishOnError on_error{ws};
    plan.upload(ws);
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    orbgpu_sim3_opt_problem d = *p;
    d.valid = ws.at(i_valid), d.Xw1 = ws.at(i_x1), d.Xw2 = ws.at(i_x2);
    d.octave1 = ws.at(i_o1), d.octave2 = ws.at(i_o2);
    d.kp1_xy = ws.at(i_k1), d.kp2_xy = ws.at(i_k2);
    d.inlier = ws.at(o_inl), d.result = ws.at(o_res);
    if ((rc = orbgpu_sim3_optimize_batch_device(1, &d, device_id, ws.stream)) != ORBGPU_OK)
        return rc;
    plan.download(ws);
    if ((rc = ws.finish()) != ORBGPU_OK)
        return rc;
    *n_inliers = r.n_inliers;
    if (result)
        *result = r;
    return ORBGPU_OK;
}

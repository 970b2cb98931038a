// Optimizer::PoseOptimization (Optimizer.cc:239-451) on the device: motion-only bundle adjustment of ONE pose over
// N unary reprojection edges.  One workgroup per problem runs all four rounds and every Levenberg-Marquardt trial
// without returning to the host; the definition (g2o restated, "g2o unpinned") is in include/orbgpu.h and
// tests/pose_model.py.  FP64 throughout, no fused multiply-add (-ffp-contract=off): the per-edge arithmetic is the
// model's operation for operation, only the order of the sums over edges differs (fixed tree here, sequential there).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "opt_edges.h"
#include "opt_math.h"
#include "staging.h"

namespace orbgpu {

constexpr int PO_THREADS = 256;               // 4 waves: a first guess (DESIGN.md "Pose optimisation"), not a tuned shape
constexpr int PO_WAVES = PO_THREADS / 64;
constexpr int PO_LDS_EDGES = 1536;            // 32 B per edge -> 48 KiB of LDS; more edges go through the global spill
constexpr int PO_SUMS = 28;                   // 21 of symmetric H, 6 of b, 1 robust chi2
constexpr unsigned PO_STEREO = 1u << 30, PO_LEVEL1 = 1u << 31, PO_KP_MASK = (1u << 24) - 1;

struct PoseProblemDev {
    const int32_t *n;
    const orbgpu_keypoint *kps;
    const float *u_right;
    const int32_t *kp_to_mp;
    const float *world_pos;
    uint8_t *outlier;
    orbgpu_pose_result *result;
    float4 *spill;        // [2 * cap], or nullptr when cap <= lds_edges
    int32_t *spill_count; // problems of this call that took the spill path (diagnostic)
    int32_t cap, rows, nlevels, lds_edges;
    float inv_sigma2[ORBGPU_MAX_LEVELS];
    float Tcw[16];
    double q0[4], t0[3];  // Converter::toSE3Quat(mTcw)
    double fx, fy, cx, cy, bf;
    double delta[2], delta2[2];  // Huber delta (mono, stereo) and its square
};

// key point i is an edge (1), has an out-of-range row / octave (2), or holds no map point (0)
__device__ inline int edge_kind(const PoseProblemDev &P, int i, int n)
{
    if (i >= n)
        return 0;
    const int r = P.kp_to_mp[i];
    if (r < 0)
        return 0;
    const int o = P.kps[i].octave;
    return (r >= P.rows || o < 0 || o >= P.nlevels) ? 2 : 1;
}

__global__ __launch_bounds__(PO_THREADS) void k_pose_opt(const PoseProblemDev *__restrict__ problems)
{
    __shared__ float4 lds_edges[2 * PO_LDS_EDGES];
    __shared__ double red[PO_WAVES * PO_SUMS];
    __shared__ int wcount[PO_WAVES][2];
    __shared__ int icount;
    const PoseProblemDev &P = problems[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(*P.n, 0), P.cap);
    const Cam C{P.fx, P.fy, P.cx, P.cy, P.bf};

    // pass 1: count the edges (decides LDS or spill) and the skipped ones
    int ne = 0, nbadidx = 0;
    for (int base = 0; base < n; base += PO_THREADS) {
        const int kind = edge_kind(P, base + tid, n);
        const unsigned long long m1 = __ballot(kind == 1), m2 = __ballot(kind == 2);
        __syncthreads();
        if (lane == 0)
            wcount[wave][0] = __popcll(m1), wcount[wave][1] = __popcll(m2);
        __syncthreads();
#pragma unroll
        for (int wv = 0; wv < PO_WAVES; wv++)
            ne += wcount[wv][0], nbadidx += wcount[wv][1];
    }
    orbgpu_pose_result *res = P.result;
    // ne <= cap, and the host gives every problem with cap > lds_edges a spill block of 2 * cap records
    const bool spilled = ne > P.lds_edges;
    float4 *E = spilled ? P.spill : lds_edges;

    // pass 2: compact the edges in key-point order; all edges get mvbOutlier = false (Optimizer.cc:281, :318)
    {
        int at = 0;
        for (int base = 0; base < n; base += PO_THREADS) {
            const int i = base + tid;
            const bool is_edge = edge_kind(P, i, n) == 1;
            const unsigned long long m1 = __ballot(is_edge);
            __syncthreads();
            if (lane == 0)
                wcount[wave][0] = __popcll(m1);
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int wv = 0; wv < PO_WAVES; wv++) {
                before += wv < wave ? wcount[wv][0] : 0;
                total += wcount[wv][0];
            }
            if (is_edge) {
                const int e = at + before + __popcll(m1 & ((1ull << lane) - 1ull));
                const orbgpu_keypoint kp = P.kps[i];
                const float *X = P.world_pos + 3 * (size_t)P.kp_to_mp[i];
                const float ur = P.u_right[i];
                const unsigned bits = (unsigned)i | (ur < 0.f ? 0u : PO_STEREO);
                E[2 * e] = make_float4(X[0], X[1], X[2], P.inv_sigma2[kp.octave]);
                E[2 * e + 1] = make_float4(kp.x, kp.y, ur, __uint_as_float(bits));
                P.outlier[i] = 0;
            }
            at += total;
        }
    }
    __syncthreads();

    if (ne < 3) {  // Optimizer.cc:365-366: return 0, pose untouched
        if (tid == 0) {
            for (int i = 0; i < 16; i++) {
                res->Tcw[i] = P.Tcw[i];
                res->Tcw_d[i] = (double)P.Tcw[i];
            }
            res->n_initial = ne, res->n_inliers = 0, res->rounds = 0, res->iterations = 0, res->trials = 0;
            res->n_bad_index = nbadidx;
        }
        return;
    }
    if (tid == 0 && spilled)
        atomicAdd(P.spill_count, 1);

    // Everything below that steers control flow (lam, nu, rho, the pose, the counters) is computed redundantly by every
    // lane from block_sum results, hence workgroup-uniform: the barriers inside the loops are reached by all lanes.
    // Trip counts are bounded by the constants of the definition: 4 rounds x 10 iterations x 10 trials.
    double q[4], t[3], R[9];
    int rounds = 0, iterations = 0, trials = 0, n_bad = 0;
    bool use_kernel = true;
    for (int rnd = 0; rnd < 4; rnd++) {
#pragma unroll
        for (int i = 0; i < 4; i++)
            q[i] = P.q0[i];
#pragma unroll
        for (int i = 0; i < 3; i++)
            t[i] = P.t0[i];  // Optimizer.cc:377: every round restarts from the input pose
        double lam = 0.0, nu = 2.0;
        for (int it = 0; it < 10; it++) {
            // errors, robust chi2 and the normal equation at the current pose
            quat_to_matrix(q, R);
            double acc[PO_SUMS];
#pragma unroll
            for (int k = 0; k < PO_SUMS; k++)
                acc[k] = 0.0;
            for (int e = tid; e < ne; e += PO_THREADS) {
                const float4 ea = E[2 * e], eb = E[2 * e + 1];
                const unsigned bits = __float_as_uint(eb.w);
                if (bits & PO_LEVEL1)
                    continue;
                const bool stereo = bits & PO_STEREO;
                double er[3], Pc[3];
                const double chi2 = edge_error(R, t, C, ea, eb, stereo, er, Pc);
                double rho0, rho1;
                huber(chi2, P.delta[stereo], P.delta2[stereo], rho0, rho1, use_kernel);
                double J[3][6];
                pose_jacobian(Pc, C, stereo, J);
                const double s = (double)ea.w * rho1;
                double Jw[3][6];
#pragma unroll
                for (int r = 0; r < 3; r++)
#pragma unroll
                    for (int a = 0; a < 6; a++)
                        Jw[r][a] = J[r][a] * s;
                int k = 0;
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int c = a; c < 6; c++, k++)
                        acc[k] += (Jw[0][a] * J[0][c] + Jw[1][a] * J[1][c]) + Jw[2][a] * J[2][c];
#pragma unroll
                for (int a = 0; a < 6; a++)
                    acc[21 + a] += -((Jw[0][a] * er[0] + Jw[1][a] * er[1]) + Jw[2][a] * er[2]);
                acc[27] += rho0;
            }
            block_sum<PO_WAVES>(acc, red);
            double Hu[21], b[6];
#pragma unroll
            for (int k = 0; k < 21; k++)
                Hu[k] = acc[k];
#pragma unroll
            for (int a = 0; a < 6; a++)
                b[a] = acc[21 + a];
            if (it == 0) {
                lam = lm_initial_lambda<6>(Hu);
                nu = 2.0;
            }
            double cur = acc[27], rho = 0.0;
            int trial = 0;
            bool stop = false;
            iterations++;
            do {
                double x[6], qn[4], tn[3], Rn[9];
                const bool ok = cholesky_solve<6>(Hu, lam, b, x);
                pose_update(q, t, x, qn, tn);
                quat_to_matrix(qn, Rn);
                double part[1] = {0.0};
                for (int e = tid; e < ne; e += PO_THREADS) {
                    const float4 ea = E[2 * e], eb = E[2 * e + 1];
                    const unsigned bits = __float_as_uint(eb.w);
                    if (bits & PO_LEVEL1)
                        continue;
                    const bool stereo = bits & PO_STEREO;
                    double er[3], Pc[3], rho0, rho1;
                    const double chi2 = edge_error(Rn, tn, C, ea, eb, stereo, er, Pc);
                    huber(chi2, P.delta[stereo], P.delta2[stereo], rho0, rho1, use_kernel);
                    part[0] += rho0;
                }
                block_sum<PO_WAVES>(part, red);
                const double tmp = ok ? part[0] : DBL_MAX;
                double scale = 0.0;
#pragma unroll
                for (int a = 0; a < 6; a++)
                    scale = scale + x[a] * (lam * x[a] + b[a]);
                scale = scale + 1e-3;
                trials++;
                if (lm_trial(cur, tmp, scale, lam, nu, rho, stop)) {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        q[i] = qn[i];
#pragma unroll
                    for (int i = 0; i < 3; i++)
                        t[i] = tn[i];
                    cur = tmp;
                }
                trial++;
            } while (!stop && rho < 0 && trial < 10);
            if (trial == 10 || rho == 0 || stop)
                break;
        }
        // classification at the round's final pose (Optimizer.cc:384-437)
        quat_to_matrix(q, R);
        __syncthreads();
        if (tid == 0)
            icount = 0;
        __syncthreads();
        int mine = 0;
        for (int e = tid; e < ne; e += PO_THREADS) {
            const float4 ea = E[2 * e];
            float4 eb = E[2 * e + 1];
            unsigned bits = __float_as_uint(eb.w);
            const bool stereo = bits & PO_STEREO;
            double er[3], Pc[3];
            const double chi2 = edge_error(R, t, C, ea, eb, stereo, er, Pc);
            const bool out = (float)chi2 > (stereo ? 7.815f : 5.991f);
            bits = out ? (bits | PO_LEVEL1) : (bits & ~PO_LEVEL1);
            eb.w = __uint_as_float(bits);
            E[2 * e + 1] = eb;
            P.outlier[bits & PO_KP_MASK] = out ? 1 : 0;
            mine += out ? 1 : 0;
        }
        mine = wave_reduce_add(mine);
        if (lane == 0 && mine)
            atomicAdd(&icount, mine);
        __syncthreads();
        n_bad = icount;
        rounds = rnd + 1;
        if (rnd == 2)
            use_kernel = false;
        if (ne < 10)  // optimizer.edges().size() < 10: the total, not the active ones (Optimizer.cc:439)
            break;
    }
    if (tid == 0) {
        quat_to_matrix(q, R);
        const double T[16] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0.0, 0.0, 0.0, 1.0};
        for (int i = 0; i < 16; i++) {
            res->Tcw_d[i] = T[i];
            res->Tcw[i] = (float)T[i];
        }
        res->n_initial = ne, res->n_inliers = ne - n_bad, res->rounds = rounds, res->iterations = iterations;
        res->trials = trials, res->n_bad_index = nbadidx;
    }
}

// Per (thread, device) staging of the entry points (staging.h); the stream and the H_* buffers (the uploaded problem)
// are the host flavour's.
enum { PROBLEMS, SPILL, SPILL_COUNT, H_KPS, H_UR, H_K2M, H_WP, H_N, H_OUT, H_RES, N_BUF };
struct PoseWs : Staging<N_BUF> {};

static int check_problem(const orbgpu_pose_problem &p, int k)
{
    ORBGPU_REQUIRE(p.frame && p.d_kp_to_mp && p.Tcw && p.inv_level_sigma2 && p.d_outlier && p.d_result,
                   "problem %d: null argument", k);
    const orbgpu_device_frame_view *f = p.frame;
    ORBGPU_REQUIRE(f->cap >= 0 && f->cap <= 16384, "problem %d: frame capacity out of range (max 16384)", k);
    ORBGPU_REQUIRE(f->nlevels >= 1 && f->nlevels <= ORBGPU_MAX_LEVELS, "problem %d: nlevels outside [1, %d]", k,
                   ORBGPU_MAX_LEVELS);
    ORBGPU_REQUIRE(f->n && (f->cap == 0 || (f->kps && f->u_right)), "problem %d: null frame arrays", k);
    ORBGPU_REQUIRE(p.rows >= 0 && (p.rows == 0 || p.d_world_pos), "problem %d: bad map point rows", k);
    return ORBGPU_OK;
}

} // namespace orbgpu

using namespace orbgpu;

extern "C" int orbgpu_pose_optimization_batch_device(int32_t n, const orbgpu_pose_problem *problems, int32_t device_id,
                                                     void *hip_stream)
{
    PoseWs *wsp;
    int rc = batch_begin(n, problems, check_problem, device_id, wsp);
    if (rc != ORBGPU_OK || !wsp)
        return rc;
    PoseWs &ws = *wsp;
    // ORBGPU_DEBUG_POSE_LDS_EDGES=<k> (tests): problems with more than k edges take the global spill path
    const int lds_edges = debug_limit("ORBGPU_DEBUG_POSE_LDS_EDGES", PO_LDS_EDGES);
    size_t spill_edges = 0;
    for (int k = 0; k < n; k++)
        if (problems[k].frame->cap > lds_edges)
            spill_edges += (size_t)problems[k].frame->cap;
    ws.reserve(PROBLEMS, sizeof(PoseProblemDev) * (size_t)n);
    ws.reserve(SPILL, 2 * sizeof(float4) * std::max<size_t>(spill_edges, 1));
    ws.reserve(SPILL_COUNT, sizeof(int32_t));
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    std::vector<PoseProblemDev> hp((size_t)n);
    size_t so = 0;
    for (int k = 0; k < n; k++) {
        const orbgpu_pose_problem &p = problems[k];
        const orbgpu_device_frame_view *f = p.frame;
        PoseProblemDev &D = hp[k];
        memset(&D, 0, sizeof(D));
        D.n = f->n, D.kps = f->kps, D.u_right = f->u_right, D.kp_to_mp = p.d_kp_to_mp, D.world_pos = p.d_world_pos;
        D.outlier = p.d_outlier, D.result = p.d_result;
        D.cap = f->cap, D.rows = p.rows, D.nlevels = f->nlevels, D.lds_edges = lds_edges;
        D.spill_count = ws.as<int32_t>(SPILL_COUNT);
        if (f->cap > lds_edges) {
            D.spill = ws.as<float4>(SPILL) + 2 * so;
            so += (size_t)f->cap;
        }
        for (int l = 0; l < f->nlevels; l++)
            D.inv_sigma2[l] = p.inv_level_sigma2[l];
        // Converter::toSE3Quat (Converter.cc:37-47): float 3x3 -> double -> unit quaternion, float t -> double
        unit_quat_from_floats(p.Tcw, 4, D.q0);
        for (int r = 0; r < 3; r++)
            D.t0[r] = (double)p.Tcw[4 * r + 3];
        for (int i = 0; i < 16; i++)
            D.Tcw[i] = p.Tcw[i];
        D.fx = (double)p.fx, D.fy = (double)p.fy, D.cx = (double)p.cx, D.cy = (double)p.cy, D.bf = (double)p.mbf;
        D.delta[0] = (double)(float)std::sqrt(5.991), D.delta[1] = (double)(float)std::sqrt(7.815);
        D.delta2[0] = D.delta[0] * D.delta[0], D.delta2[1] = D.delta[1] * D.delta[1];
    }
    const hipStream_t st = (hipStream_t)hip_stream;
    ORBGPU_HIP_TRY(hipMemsetAsync(ws.buf[SPILL_COUNT].p, 0, sizeof(int32_t), st));
    ORBGPU_HIP_TRY(hipMemcpyAsync(ws.buf[PROBLEMS].p, hp.data(), sizeof(PoseProblemDev) * (size_t)n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pose_opt, dim3(n), dim3(PO_THREADS), 0, st, ws.as<PoseProblemDev>(PROBLEMS));
    ORBGPU_HIP_TRY(hipGetLastError());
    return ORBGPU_OK;
}

extern "C" int orbgpu_pose_optimization_device(const orbgpu_pose_problem *p, int32_t device_id, void *hip_stream)
{
    ORBGPU_REQUIRE(p, "null argument");
    return orbgpu_pose_optimization_batch_device(1, p, device_id, hip_stream);
}

extern "C" int orbgpu_pose_last_spills(int32_t device_id, int32_t *problems_spilled)
{
    return last_spills<PoseWs>(device_id, SPILL_COUNT, "no pose optimisation recorded on this thread", problems_spilled);
}

extern "C" int orbgpu_pose_optimization(const orbgpu_frame_view *f, const uint8_t *has_mp, const float *world_pos,
                                        float *Tcw, const float *inv_level_sigma2, float fx, float fy, float cx, float cy,
                                        float mbf, uint8_t *outlier, int32_t *n_inliers, orbgpu_pose_result *result,
                                        int32_t device_id)
{
    ORBGPU_REQUIRE(f && Tcw && inv_level_sigma2 && n_inliers, "null argument");
    ORBGPU_REQUIRE(f->n >= 0 && f->n <= 16384, "key point count out of range (max 16384)");
    ORBGPU_REQUIRE(f->nlevels >= 1 && f->nlevels <= ORBGPU_MAX_LEVELS, "nlevels outside [1, %d]", ORBGPU_MAX_LEVELS);
    ORBGPU_REQUIRE(f->n == 0 || (f->kp_x && f->kp_y && f->kp_octave && f->u_right && has_mp && world_pos && outlier),
                   "null arrays");
    int rc = select_device(device_id);
    if (rc != ORBGPU_OK)
        return rc;
    PoseWs &ws = per_device_workspace<PoseWs>(device_id);
    if ((rc = ws.bind(device_id, true)) != ORBGPU_OK)
        return rc;
    const int n = f->n;
    const size_t cap = (size_t)std::max(n, 1);
    ws.reserve(H_KPS, sizeof(orbgpu_keypoint) * cap);
    ws.reserve(H_UR, sizeof(float) * cap);
    ws.reserve(H_K2M, sizeof(int32_t) * cap);
    ws.reserve(H_WP, 3 * sizeof(float) * cap);
    ws.reserve(H_N, sizeof(int32_t));
    ws.reserve(H_OUT, cap);
    ws.reserve(H_RES, sizeof(orbgpu_pose_result));
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    std::vector<orbgpu_keypoint> kps(cap);
    std::vector<int32_t> k2m(cap);
    for (int i = 0; i < n; i++) {
        orbgpu_keypoint k{};
        k.x = f->kp_x[i], k.y = f->kp_y[i], k.octave = f->kp_octave[i], k.class_id = -1;
        kps[i] = k;
        k2m[i] = has_mp[i] ? i : -1;
    }
    PoseWs::FinishOnError on_error{ws};
    const int32_t n32 = n;
    ws.upload(H_N, &n32, sizeof(n32));
    if (n > 0) {
        ws.upload(H_KPS, kps.data(), sizeof(orbgpu_keypoint) * n);
        ws.upload(H_K2M, k2m.data(), sizeof(int32_t) * n);
        ws.upload(H_UR, f->u_right, sizeof(float) * n);
        ws.upload(H_WP, world_pos, 3 * sizeof(float) * n);
        ws.upload(H_OUT, outlier, n);
    }
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    orbgpu_device_frame_view dv{};
    dv.cap = n, dv.n = ws.as<int32_t>(H_N), dv.kps = ws.as<orbgpu_keypoint>(H_KPS), dv.u_right = ws.as<float>(H_UR);
    dv.nlevels = f->nlevels;
    orbgpu_pose_problem p{};
    p.frame = &dv, p.d_kp_to_mp = ws.as<int32_t>(H_K2M), p.d_world_pos = ws.as<float>(H_WP), p.rows = n;
    p.Tcw = Tcw, p.inv_level_sigma2 = inv_level_sigma2;
    p.fx = fx, p.fy = fy, p.cx = cx, p.cy = cy, p.mbf = mbf;
    p.d_outlier = ws.as<uint8_t>(H_OUT), p.d_result = ws.as<orbgpu_pose_result>(H_RES);
    if ((rc = orbgpu_pose_optimization_batch_device(1, &p, device_id, ws.stream)) != ORBGPU_OK)
        return rc;
    orbgpu_pose_result r;
    ws.download(&r, H_RES, sizeof(r));
    if (n > 0)
        ws.download(outlier, H_OUT, n);
    if ((rc = ws.finish()) != ORBGPU_OK)
        return rc;
    memcpy(Tcw, r.Tcw, sizeof(r.Tcw));
    *n_inliers = r.n_inliers;
    if (result)
        *result = r;
    return ORBGPU_OK;
}

// Optimizer::OptimizeEssentialGraph (Optimizer.cc:780-1045) on the device: the Sim3 pose graph of a loop closure, one 7-DoF
// vertex per key frame, one EdgeSim3 per essential-graph edge, Levenberg-Marquardt over a sparse system of 7 rows per key
// frame (g2o's BlockSolver_7_3 restated, "g2o unpinned").  One workgroup per problem runs every iteration and every trial
// without returning to the host; the definition (G1-G12) is in include/orbgpu.h and tests/eg_model.py.  FP64 throughout, no
// fused multiply-add (-ffp-contract=off): the per-edge and per-vertex arithmetic is the model's operation for operation;
// the sums per block of H run edge by edge in edge order as the model's do, the sums over the workgroup (chi2, the scale of
// rho) as per-lane partial sums and a fixed tree.
//
// Per iteration: (1) one lane per (vertex, k, sign) forms the 14 perturbed states of G5; (2) one lane per (edge, column)
// evaluates the edge's error or one column of one of its two numeric Jacobians -- 1 + 28 error evaluations per edge; (3) one
// lane per (block of H, row) sums J'J over the block's edge list; then per trial (4) the blocks are scattered into the
// envelope with lambda on the diagonal, (5) skyline_llt_solve (skyline.h) runs over the whole workgroup with __syncthreads,
// (6) one lane per vertex applies exp(x_v), (7) one lane per edge evaluates the trial's chi2.
//
// Memory: everything lives in the call's global workspace -- the envelope of the factor is far larger than LDS for the maps
// this is for (an LDS-resident variant for small graphs is not written); LDS holds the reduction scratch only.
//
// The Sim3 arithmetic (G2-G5: product, inverse, map, logarithm, edge error, exp(x) * S) is sim3_math.h's, which k_sim3_opt
// shares; the barrier and the stop flag are opt_math.h's.  The decision on a trial is opt_math.h's lm_trial written out:
// calling it here cost one row of tools/bench_eg.py more than the parent's spread.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "carve.h"
#include "common.h"
#include "opt_math.h"
#include "sim3_math.h"
#include "skyline.h"
#include "staging.h"

namespace orbgpu {
namespace eg {

// First guesses, not tuned shapes: the width is k_bundle_adjustment's, nothing has been measured against it.
constexpr int EG_THREADS = 512;
constexpr int EG_WAVES = EG_THREADS / 64;
constexpr int EG_POINT_THREADS = 256;
constexpr double EG_DELTA = 1e-9;     // G5
constexpr double EG_LAMBDA0 = 1e-16;  // G8
constexpr int EG_COLS = 15;           // work items per edge: its error, 7 columns of Ji, 7 columns of Jj

struct EgEdge {  // a taken edge, in the caller's order
    int32_t i, j, kind, orig;
};

struct EgProblemDev {
    const EgEdge *edges;        // [ne]
    const double *Snc;          // [V][8]
    double *state[2];           // [V][8]: the kept state and the trial's; [0] uploaded as Scw
    const int32_t *slot;        // [V]: position among the free active vertices in the solver's order, or -1
    const int32_t *row_of;      // [nf]: vertex of a position
    double *meas;               // [ne][8]
    double *pert;               // [V][14][8]: exp(+-d 1_k) * state, k-major, + before -
    double *J;                  // [ne][2][7 error rows][7 parameters]
    double *err;                // [ne][7]
    const int32_t *diag_start;  // [nf + 1] into diag_items
    const int32_t *diag_items;  // 2 * edge + end, per position, in edge order
    const int32_t *blk_start;   // [nblk + 1] into blk_items
    const int32_t *blk_items;   // 2 * edge + (end of the edge that is the block's row vertex), in edge order
    const int2 *blk_pos;        // [nblk]: (a, b), a > b: positions of the block's row and column vertex
    double *Hd, *Ho, *b;        // [nf][49], [nblk][49], [7 nf]
    const int32_t *first, *last;  // skyline.h, [7 nf]
    const int64_t *off;
    double *A;                  // the envelope
    double *vec;                // [3 * 7 nf]: right-hand side / x, then the solve's work
    const int32_t *stop;
    double *Siw_d;
    float *Tiw;
    orbgpu_essential_graph_result *result;
    int64_t envelope;
    int32_t V, ne, nf, nblk, n_bad_index, n_iterations, fix_scale, bandwidth;
};

// errors of every edge at `states` into P.err, and their sum (the same bits in every lane)
__device__ __noinline__ double chi2_at(const EgProblemDev &P, const double *states, double *red)
{
    double part[1] = {0.0};
    for (int e = threadIdx.x; e < P.ne; e += EG_THREADS) {
        const EgEdge E = P.edges[e];
        double M[8], Si[8], Sj[8], er[7];
        load8(P.meas + 8 * (size_t)e, M);
        load8(states + 8 * (size_t)E.i, Si);
        load8(states + 8 * (size_t)E.j, Sj);
        sim3_edge_error(M, Si, Sj, er);
#pragma unroll
        for (int r = 0; r < 7; r++)
            P.err[7 * (size_t)e + r] = er[r];
        part[0] = part[0] + chi2_of(er);
    }
    block_sum<EG_WAVES>(part, red);
    return part[0];
}

__global__ __launch_bounds__(EG_THREADS) void k_essential_graph(const EgProblemDev *__restrict__ problems)
{
    __shared__ double red[EG_WAVES];
    __shared__ int flag;
    const EgProblemDev &P = problems[blockIdx.x];
    const int tid = threadIdx.x;
    const int n = 7 * P.nf;
    const bool fix_scale = P.fix_scale != 0;

    // Everything below that steers control flow (the flag, lam, nu, rho, the counters, which copy of the state is kept) is
    // the same in every lane -- broadcast through LDS or computed from block_sum results -- so the barriers inside the
    // loops are reached by all lanes.  Trip counts are bounded by the definition: n_iterations <=
    // ORBGPU_EG_MAX_ITERATIONS (checked on the host) of at most 10 trials.
    orbgpu_essential_graph_result res{};
    res.n_edges = P.ne, res.n_bad_index = P.n_bad_index, res.n_free_active = P.nf;
    res.envelope = (int32_t)P.envelope, res.bandwidth = P.bandwidth;
    if (stop_requested(P.stop, &flag)) {
        if (tid == 0) {
            res.stopped = 1;
            *P.result = res;
        }
        return;
    }
    // G1: the measurements, from the entry states
    for (int e = tid; e < P.ne; e += EG_THREADS) {
        const EgEdge E = P.edges[e];
        const double *src = E.kind == 0 ? P.state[0] : P.Snc;
        double Si[8], Sj[8], Ii[8], M[8];
        load8(src + 8 * (size_t)E.i, Si);
        load8(src + 8 * (size_t)E.j, Sj);
        sim3_inv(Si, Ii);
        sim3_mul(Sj, Ii, M);
#pragma unroll
        for (int k = 0; k < 8; k++)
            P.meas[8 * (size_t)e + k] = M[k];
    }
    __syncthreads();

    int kept = 0, stopped = 0, iterations = 0, trials = 0;
    double lam = 0.0, nu = 2.0, cur = 0.0, chi_start = 0.0;
    const double inv2d = 1.0 / (2.0 * EG_DELTA);
    if (P.n_iterations == 0)
        chi_start = cur = chi2_at(P, P.state[0], red);
    for (int it = 0; it < P.n_iterations; it++) {
        if (stop_requested(P.stop, &flag)) {
            stopped = 1;
            break;
        }
        const double *St = P.state[kept];
        double *Sn = P.state[kept ^ 1];
        // ---- G5 (1): the perturbed states of the free active vertices ----
        for (int idx = tid; idx < 14 * P.nf; idx += EG_THREADS) {
            const int v = P.row_of[idx / 14], c = idx % 14, k = c >> 1;
            const double d = c & 1 ? -EG_DELTA : EG_DELTA;
            double S[8], x[7], Sp[8];
            load8(St + 8 * (size_t)v, S);
#pragma unroll
            for (int a = 0; a < 7; a++)
                x[a] = a == k ? d : 0.0;
            sim3_update(S, x, fix_scale, Sp);
#pragma unroll
            for (int a = 0; a < 8; a++)
                P.pert[(14 * (size_t)v + c) * 8 + a] = Sp[a];
        }
        __syncthreads();
        // ---- G4, G5 (2): per edge its error and the 14 columns of its two Jacobians ----
        for (long long idx = tid; idx < (long long)EG_COLS * P.ne; idx += EG_THREADS) {
            const int e = (int)(idx / EG_COLS), c = (int)(idx % EG_COLS);
            const EgEdge E = P.edges[e];
            const int end = c > 7 ? 1 : 0, k = c == 0 ? 0 : (c - 1) % 7;
            const int v = end ? E.j : E.i;
            if (c > 0 && P.slot[v] < 0)  // a fixed vertex has no Jacobian
                continue;
            double M[8], Si[8], Sj[8], dif[7];
            load8(P.meas + 8 * (size_t)e, M);
            load8(St + 8 * (size_t)E.i, Si);
            load8(St + 8 * (size_t)E.j, Sj);
            // One text of the error for all three uses, kept rolled: the error itself (one trip, nothing replaced), or
            // e(+) then e(-) with the perturbed state in the place of its end -- by selects, so that both states stay in
            // registers and only one evaluation is live at a time.
            const double *pp = P.pert + (14 * (size_t)v + 2 * k) * 8;
#pragma unroll 1
            for (int sgn = 0; sgn < (c == 0 ? 1 : 2); sgn++) {
                double Sa[8], Sb[8], er[7];
#pragma unroll
                for (int a = 0; a < 8; a++) {
                    const double pv = c == 0 ? 0.0 : pp[8 * sgn + a];
                    Sa[a] = c == 0 || end ? Si[a] : pv;
                    Sb[a] = c == 0 || !end ? Sj[a] : pv;
                }
                sim3_edge_error(M, Sa, Sb, er);
#pragma unroll
                for (int r = 0; r < 7; r++)
                    dif[r] = sgn == 0 ? er[r] : (dif[r] - er[r]) * inv2d;
            }
            double *o = c == 0 ? P.err + 7 * (size_t)e : P.J + ((size_t)e * 2 + end) * 49 + k;
            const int stride = c == 0 ? 1 : 7;
#pragma unroll
            for (int r = 0; r < 7; r++)
                o[stride * r] = dif[r];
        }
        __syncthreads();
        {
            double part[1] = {0.0};
            for (int e = tid; e < P.ne; e += EG_THREADS) {
                double er[7];
#pragma unroll
                for (int r = 0; r < 7; r++)
                    er[r] = P.err[7 * (size_t)e + r];
                part[0] = part[0] + chi2_of(er);
            }
            block_sum<EG_WAVES>(part, red);
            cur = part[0];
        }
        if (it == 0) {
            chi_start = cur;
            lam = EG_LAMBDA0;
            nu = 2.0;
        }
        // ---- G6 (3): one lane per (block, row) sums its edges in edge order ----
        for (int idx = tid; idx < 7 * (P.nf + P.nblk); idx += EG_THREADS) {
            const int blk = idx / 7, x = idx % 7;
            const bool diag = blk < P.nf;
            const int o = diag ? blk : blk - P.nf;
            const int32_t *items = diag ? P.diag_items : P.blk_items;
            const int k0 = diag ? P.diag_start[o] : P.blk_start[o], k1 = diag ? P.diag_start[o + 1] : P.blk_start[o + 1];
            double h[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, bx = 0.0;
            for (int k = k0; k < k1; k++) {
                const int item = items[k], e = item >> 1, end = item & 1;
                const double *Ja = P.J + ((size_t)e * 2 + end) * 49;
                const double *Jb = diag ? Ja : P.J + ((size_t)e * 2 + (end ^ 1)) * 49;
#pragma unroll
                for (int r = 0; r < 7; r++) {
                    const double a = Ja[7 * r + x];
#pragma unroll
                    for (int y = 0; y < 7; y++)
                        h[y] = h[y] + a * Jb[7 * r + y];
                }
                if (diag) {
                    const double *er = P.err + 7 * (size_t)e;
                    double g = Ja[x] * er[0];
#pragma unroll
                    for (int r = 1; r < 7; r++)
                        g = g + Ja[7 * r + x] * er[r];
                    bx = bx - g;
                }
            }
            double *H = (diag ? P.Hd : P.Ho) + 49 * (size_t)o + 7 * x;
#pragma unroll
            for (int y = 0; y < 7; y++)
                H[y] = h[y];
            if (diag)
                P.b[7 * (size_t)o + x] = bx;
        }
        __syncthreads();

        double rho = 0.0;
        int trial = 0;
        bool stop = false;
        iterations++;
        do {
            if (stop_requested(P.stop, &flag)) {
                stopped = 1;
                break;
            }
            // ---- G7 (4): the blocks into the envelope, lambda on the diagonal ----
            for (long long k = tid; k < P.envelope; k += EG_THREADS)
                P.A[k] = 0.0;
            __syncthreads();
            for (int idx = tid; idx < 7 * (P.nf + P.nblk); idx += EG_THREADS) {
                const int blk = idx / 7, x = idx % 7;
                if (blk < P.nf) {
                    const double *H = P.Hd + 49 * (size_t)blk + 7 * x;
                    const int row = 7 * blk + x;
                    double *Ar = P.A + P.off[row] + 7 * blk;
                    for (int y = 0; y <= x; y++)
                        Ar[y] = y == x ? H[y] + lam : H[y];
                    P.vec[row] = P.b[row];
                } else {
                    const int2 ab = P.blk_pos[blk - P.nf];
                    const double *H = P.Ho + 49 * (size_t)(blk - P.nf) + 7 * x;
                    double *Ar = P.A + P.off[7 * ab.x + x] + 7 * ab.y;
#pragma unroll
                    for (int y = 0; y < 7; y++)
                        Ar[y] = H[y];
                }
            }
            __syncthreads();
            // ---- (5) ----
            const bool ok = skyline_llt_solve(n, P.first, P.off, P.last, P.A, P.vec, P.vec + n, tid, EG_THREADS, WorkgroupBarrier());
            __syncthreads();
            // ---- (6): the trial state and x'(lambda x + b) ----
            double part[1] = {0.0};
            for (int v = tid; v < P.V; v += EG_THREADS) {
                const int f = P.slot[v];
                double S[8], Sv[8];
                load8(St + 8 * (size_t)v, S);
                if (f >= 0) {
                    double x[7];
#pragma unroll
                    for (int a = 0; a < 7; a++) {
                        x[a] = P.vec[7 * f + a];
                        part[0] = part[0] + x[a] * (lam * x[a] + P.b[7 * f + a]);
                    }
                    sim3_update(S, x, fix_scale, Sv);
                } else {
#pragma unroll
                    for (int a = 0; a < 8; a++)
                        Sv[a] = S[a];
                }
#pragma unroll
                for (int a = 0; a < 8; a++)
                    Sn[8 * (size_t)v + a] = Sv[a];
            }
            __syncthreads();
            block_sum<EG_WAVES>(part, red);
            // ---- (7) ----
            const double chi_n = chi2_at(P, Sn, red);
            const double tmp = ok ? chi_n : DBL_MAX;
            const double scale = part[0] + 1e-3;
            rho = (cur - tmp) / scale;
            trials++;
            if (rho > 0 && isfinite(tmp)) {
                const double c3 = 2.0 * rho - 1.0;
                const double alpha = fmin(1.0 - (c3 * c3) * c3, 2.0 / 3.0);
                lam = lam * fmax(1.0 / 3.0, alpha);
                nu = 2.0;
                kept ^= 1;
                cur = tmp;
            } else {
                lam = lam * nu;
                nu = nu * 2.0;
                if (!isfinite(lam))
                    stop = true;
            }
            trial++;
            // an accepted trial ends the loop (rho > 0): St and Sn above stay the iteration's
        } while (!stop && rho < 0 && trial < 10);
        if (stopped || trial == 10 || rho == 0 || stop)
            break;
    }

    // ---- G10 ----
    __syncthreads();
    for (int v = tid; v < P.V; v += EG_THREADS) {
        double S[8], R[9];
        load8(P.state[kept] + 8 * (size_t)v, S);
        quat_to_matrix(S, R);
        const double is = 1.0 / S[7];
        double *od = P.Siw_d + 8 * (size_t)v;
        float *T = P.Tiw + 16 * (size_t)v;
#pragma unroll
        for (int k = 0; k < 8; k++)
            od[k] = S[k];
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++)
                T[4 * r + c] = (float)R[3 * r + c];
            T[4 * r + 3] = (float)(S[4 + r] * is);
            T[12 + r] = 0.f;
        }
        T[15] = 1.f;
    }
    if (tid == 0) {
        res.chi2_start = chi_start, res.chi2_end = cur;
        res.iterations = iterations, res.trials = trials, res.stopped = stopped;
        *P.result = res;
    }
}

// G11: one point per lane, the two states of its row read from global memory
__global__ __launch_bounds__(EG_POINT_THREADS) void k_eg_correct_points(int V, const double *__restrict__ Scw,
                                                                      const double *__restrict__ Siw, int M, const float *pos_in,
                                                                      const int32_t *__restrict__ ref, float *pos_out,
                                                                      int32_t *n_bad_ref)
{
    const int m = blockIdx.x * EG_POINT_THREADS + threadIdx.x;
    if (m >= M)
        return;
    const float px = pos_in[3 * (size_t)m], py = pos_in[3 * (size_t)m + 1], pz = pos_in[3 * (size_t)m + 2];
    const int r = ref[m];
    if (r < 0 || r >= V) {
        pos_out[3 * (size_t)m] = px, pos_out[3 * (size_t)m + 1] = py, pos_out[3 * (size_t)m + 2] = pz;
        if (n_bad_ref)
            atomicAdd(n_bad_ref, 1);
        return;
    }
    double A[8], B[8], Bi[8], Pc[3], Pw[3];
    load8(Scw + 8 * (size_t)r, A);
    load8(Siw + 8 * (size_t)r, B);
    const double X[3] = {(double)px, (double)py, (double)pz};
    sim3_map(A, X, Pc);
    sim3_inv(B, Bi);
    sim3_map(Bi, Pc, Pw);
    pos_out[3 * (size_t)m] = (float)Pw[0], pos_out[3 * (size_t)m + 1] = (float)Pw[1], pos_out[3 * (size_t)m + 2] = (float)Pw[2];
}

// Per (thread, device) staging of the entry points (staging.h): PROBLEMS and WORK are the device flavours' (the problem
// records; the uploaded index structure and states followed by the kernel's scratch), the stream and the H_* buffers the
// host flavour's.
enum { PROBLEMS, WORK, H_IN, H_OUT, H_STOP, N_BUF };
struct EgWs : Staging<N_BUF> {
    // what the device flavours upload: kept until the thread's next call, which is ordered after this one on its stream
    std::vector<char> blob;
    std::vector<EgProblemDev> records;
};

// The index structure of one problem (G12's fixed orders), built on the host before a device is touched
struct EgIndex {
    std::vector<EgEdge> edges;
    std::vector<int32_t> slot, row_of, diag_start, diag_items, blk_start, blk_items, first, last;
    std::vector<int2> blk_pos;
    std::vector<int64_t> off;
    int64_t envelope = 0;
    int n_bad_index = 0, bandwidth = 0;
};

static int check_problem(const orbgpu_essential_graph_problem &p, int k)
{
    ORBGPU_REQUIRE(p.n_vertices >= 0 && p.n_edges >= 0, "problem %d: negative count", k);
    ORBGPU_REQUIRE(p.n_iterations >= 0 && p.n_iterations <= ORBGPU_EG_MAX_ITERATIONS, "problem %d: n_iterations outside [0, %d]",
                   k, ORBGPU_EG_MAX_ITERATIONS);
    ORBGPU_REQUIRE(p.n_vertices <= ORBGPU_EG_MAX_VERTICES, "problem %d: more than %d vertices", k, ORBGPU_EG_MAX_VERTICES);
    ORBGPU_REQUIRE(p.n_edges <= ORBGPU_EG_MAX_EDGES, "problem %d: more than %d edges", k, ORBGPU_EG_MAX_EDGES);
    ORBGPU_REQUIRE(p.n_vertices == 0 || (p.Scw && p.Snc && p.fixed), "problem %d: null vertex arrays", k);
    ORBGPU_REQUIRE(p.n_edges == 0 || (p.edge_i && p.edge_j && p.edge_kind), "problem %d: null edge arrays", k);
    return ORBGPU_OK;
}

static int build_index(const orbgpu_essential_graph_problem &p, int k, EgIndex &ix)
{
    const int V = p.n_vertices;
    std::vector<uint8_t> active((size_t)V, 0);
    ix.edges.clear();
    ix.n_bad_index = 0;
    for (int e = 0; e < p.n_edges; e++) {
        const int i = p.edge_i[e], j = p.edge_j[e];
        if (i < 0 || i >= V || j < 0 || j >= V || i == j) {
            ix.n_bad_index++;
            continue;
        }
        ix.edges.push_back(EgEdge{i, j, p.edge_kind[e] == 0 ? 0 : 1, e});
        active[i] = active[j] = 1;
    }
    // the free active vertices in row order, their graph (each neighbour once), the solver's order
    std::vector<int32_t> fa_of((size_t)V, -1), fa_row;
    for (int v = 0; v < V; v++)
        if (active[v] && !p.fixed[v]) {
            fa_of[v] = (int32_t)fa_row.size();
            fa_row.push_back(v);
        }
    const int nf = (int)fa_row.size();
    std::vector<std::pair<int32_t, int32_t>> links;
    for (const EgEdge &E : ix.edges) {
        const int a = fa_of[E.i], b = fa_of[E.j];
        if (a >= 0 && b >= 0) {
            links.push_back({a, b});
            links.push_back({b, a});
        }
    }
    std::sort(links.begin(), links.end());
    links.erase(std::unique(links.begin(), links.end()), links.end());
    std::vector<int32_t> adj_start((size_t)nf + 1, 0), adj(links.size());
    for (size_t l = 0; l < links.size(); l++) {
        adj_start[(size_t)links[l].first + 1]++;
        adj[l] = links[l].second;
    }
    for (int f = 0; f < nf; f++)
        adj_start[f + 1] += adj_start[f];
    std::vector<int32_t> order((size_t)nf), pos((size_t)nf);
    rcm_order(nf, adj_start.data(), adj.data(), order.data());
    ix.slot.assign((size_t)std::max(V, 1), -1);
    ix.row_of.assign((size_t)std::max(nf, 1), 0);
    for (int q = 0; q < nf; q++) {
        pos[order[q]] = q;
        ix.row_of[q] = fa_row[order[q]];
        ix.slot[fa_row[order[q]]] = q;
    }
    // the envelope
    std::vector<int32_t> first_block((size_t)nf);
    for (int f = 0; f < nf; f++) {
        int lo = pos[f];
        for (int a = adj_start[f]; a < adj_start[f + 1]; a++)
            lo = std::min(lo, (int)pos[adj[a]]);
        first_block[pos[f]] = lo;
    }
    int64_t env = 0;
    ix.bandwidth = 0;
    for (int q = 0; q < nf; q++) {
        for (int x = 0; x < 7; x++)
            env += 7 * (int64_t)(q - first_block[q]) + x + 1;
        ix.bandwidth = std::max(ix.bandwidth, 7 * (q - first_block[q]) + 7);
    }
    ORBGPU_REQUIRE(env <= (int64_t)ORBGPU_EG_MAX_ENVELOPE, "problem %d: an envelope of %lld doubles, more than %d", k, (long long)env,
                   ORBGPU_EG_MAX_ENVELOPE);
    ix.first.assign((size_t)std::max(7 * nf, 1), 0), ix.last.assign((size_t)std::max(7 * nf, 1), 0);
    ix.off.assign((size_t)std::max(7 * nf, 1), 0);
    ix.envelope = skyline_layout(nf, 7, first_block.data(), ix.first.data(), ix.off.data(), ix.last.data());
    // per position the (edge, end) items of its diagonal block; per linked pair of positions those of its block: edge order
    ix.diag_start.assign((size_t)nf + 1, 0);
    std::vector<std::pair<int64_t, int32_t>> keyed;  // (a * nf + b, item), a > b
    for (size_t e = 0; e < ix.edges.size(); e++) {
        const int a = ix.slot[ix.edges[e].i], b = ix.slot[ix.edges[e].j];
        if (a >= 0)
            ix.diag_start[(size_t)a + 1]++;
        if (b >= 0)
            ix.diag_start[(size_t)b + 1]++;
        if (a >= 0 && b >= 0)
            keyed.push_back(a > b ? std::make_pair((int64_t)a * nf + b, (int32_t)(2 * e)) : std::make_pair((int64_t)b * nf + a, (int32_t)(2 * e + 1)));
    }
    for (int q = 0; q < nf; q++)
        ix.diag_start[q + 1] += ix.diag_start[q];
    ix.diag_items.assign((size_t)std::max(ix.diag_start[nf], 1), 0);
    {
        std::vector<int32_t> at(ix.diag_start.begin(), ix.diag_start.end() - 1);
        for (size_t e = 0; e < ix.edges.size(); e++) {
            const int a = ix.slot[ix.edges[e].i], b = ix.slot[ix.edges[e].j];
            if (a >= 0)
                ix.diag_items[(size_t)at[a]++] = (int32_t)(2 * e);
            if (b >= 0)
                ix.diag_items[(size_t)at[b]++] = (int32_t)(2 * e + 1);
        }
    }
    std::stable_sort(keyed.begin(), keyed.end(), [](const auto &l, const auto &r) { return l.first < r.first; });
    ix.blk_start.assign(1, 0);
    ix.blk_pos.clear();
    ix.blk_items.clear();
    for (size_t l = 0; l < keyed.size(); l++) {
        if (l == 0 || keyed[l].first != keyed[l - 1].first) {
            if (l)
                ix.blk_start.push_back((int32_t)l);
            ix.blk_pos.push_back(int2{(int)(keyed[l].first / nf), (int)(keyed[l].first % nf)});
        }
        ix.blk_items.push_back(keyed[l].second);
    }
    if (!keyed.empty())
        ix.blk_start.push_back((int32_t)keyed.size());
    return ORBGPU_OK;
}

static int enqueue(int32_t n, const orbgpu_essential_graph_problem *problems, std::vector<EgIndex> &ix, EgWs &ws, void *hip_stream)
{
    int rc = ORBGPU_OK;
    // The record of problem k: every buffer of its workspace named once (carve.h's WorkPlan), then its scalars
    auto describe = [&](int k, WorkPlan &plan, EgProblemDev &D) {
        const orbgpu_essential_graph_problem &p = problems[k];
        const EgIndex &I = ix[k];
        const size_t V = (size_t)p.n_vertices, ne = I.edges.size(), nf = I.diag_start.size() - 1, nblk = I.blk_pos.size();
        D.edges = plan.seg(ne, I.edges.data());
        D.Snc = plan.seg(8 * V, p.Snc);
        D.state[0] = plan.seg(8 * V, p.Scw);
        D.slot = plan.seg(I.slot.size(), I.slot.data());
        D.row_of = plan.seg(I.row_of.size(), I.row_of.data());
        D.diag_start = plan.seg(I.diag_start.size(), I.diag_start.data());
        D.diag_items = plan.seg(I.diag_items.size(), I.diag_items.data());
        D.blk_start = plan.seg(I.blk_start.size(), I.blk_start.data());
        D.blk_items = plan.seg(I.blk_items.size(), I.blk_items.data());
        D.blk_pos = plan.seg(nblk, I.blk_pos.data());
        D.first = plan.seg(I.first.size(), I.first.data());
        D.last = plan.seg(I.last.size(), I.last.data());
        D.off = plan.seg(I.off.size(), I.off.data());
        D.state[1] = plan.seg<double>(8 * V);
        D.meas = plan.seg<double>(8 * ne);
        D.pert = plan.seg<double>(14 * 8 * V);
        D.J = plan.seg<double>(98 * ne);
        D.err = plan.seg<double>(7 * ne);
        D.Hd = plan.seg<double>(49 * nf);
        D.Ho = plan.seg<double>(49 * nblk);
        D.b = plan.seg<double>(7 * nf);
        D.A = plan.seg<double>((size_t)I.envelope);
        D.vec = plan.seg<double>(21 * nf);
        D.stop = p.d_stop;
        D.Siw_d = p.d_Siw_d, D.Tiw = p.d_Tiw, D.result = p.d_result;
        D.envelope = I.envelope;
        D.V = p.n_vertices, D.ne = (int32_t)ne, D.nf = (int32_t)nf;
        D.nblk = (int32_t)nblk, D.n_bad_index = I.n_bad_index, D.n_iterations = p.n_iterations;
        D.fix_scale = p.fix_scale ? 1 : 0, D.bandwidth = I.bandwidth;
    };
    WorkPlan measured;
    for (int k = 0; k < n; k++) {
        EgProblemDev unused{};
        describe(k, measured, unused);
    }
    ws.reserve(PROBLEMS, sizeof(EgProblemDev) * (size_t)n);
    ws.reserve(WORK, measured.total());
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    std::vector<char> &blob = ws.blob;
    std::vector<EgProblemDev> &hp = ws.records;
    const size_t upload_bytes = measured.upload_bytes();
    blob.assign(upload_bytes, 0);
    hp.assign((size_t)n, EgProblemDev{});
    char *dev = ws.as<char>(WORK);
    WorkPlan plan(measured, dev, blob.data());
    for (int k = 0; k < n; k++)
        describe(k, plan, hp[k]);
    const hipStream_t st = (hipStream_t)hip_stream;
    ORBGPU_HIP_TRY(hipMemcpyAsync(ws.buf[PROBLEMS].p, hp.data(), sizeof(EgProblemDev) * (size_t)n, hipMemcpyHostToDevice, st));
    if (upload_bytes)
        ORBGPU_HIP_TRY(hipMemcpyAsync(dev, blob.data(), upload_bytes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_essential_graph, dim3(n), dim3(EG_THREADS), 0, st, ws.as<EgProblemDev>(PROBLEMS));
    ORBGPU_HIP_TRY(hipGetLastError());
    return ORBGPU_OK;
}

// checks and index structure of problem k: everything that can be refused is refused here, before a device is touched
static int check_and_index(const orbgpu_essential_graph_problem &p, int k, bool device_outputs, EgIndex &ix)
{
    int rc = check_problem(p, k);
    if (rc != ORBGPU_OK)
        return rc;
    ORBGPU_REQUIRE(!device_outputs || (p.d_result && (p.n_vertices == 0 || (p.d_Siw_d && p.d_Tiw))), "problem %d: null output", k);
    return build_index(p, k, ix);
}

static int check_points(int32_t n_vertices, int32_t n_points)
{
    ORBGPU_REQUIRE(n_vertices >= 0 && n_points >= 0, "negative count");
    ORBGPU_REQUIRE(n_vertices <= ORBGPU_EG_MAX_VERTICES, "more than %d vertices", ORBGPU_EG_MAX_VERTICES);
    ORBGPU_REQUIRE(n_points <= ORBGPU_EG_MAX_POINTS, "more than %d points", ORBGPU_EG_MAX_POINTS);
    return ORBGPU_OK;
}

} // namespace eg
} // namespace orbgpu

using namespace orbgpu;
using namespace orbgpu::eg;

extern "C" int orbgpu_sim3_from_pose(const float *Tcw, double *out)
{
    ORBGPU_REQUIRE(Tcw && out, "null argument");
    unit_quat_from_floats(Tcw, 4, out);
    for (int r = 0; r < 3; r++)
        out[4 + r] = (double)Tcw[4 * r + 3];
    out[7] = 1.0;
    return ORBGPU_OK;
}

extern "C" int orbgpu_essential_graph_batch_device(int32_t n, const orbgpu_essential_graph_problem *problems, int32_t device_id,
                                                   void *hip_stream)
{
    std::vector<EgIndex> ix;
    EgWs *wsp;
    int rc = batch_begin(
        n, problems,
        [&ix](const orbgpu_essential_graph_problem &p, int k) {
            ix.emplace_back();
            return check_and_index(p, k, true, ix.back());
        },
        device_id, wsp);
    if (rc != ORBGPU_OK || !wsp)
        return rc;
    return enqueue(n, problems, ix, *wsp, hip_stream);
}

extern "C" int orbgpu_essential_graph_device(const orbgpu_essential_graph_problem *p, int32_t device_id, void *hip_stream)
{
    ORBGPU_REQUIRE(p, "null argument");
    return orbgpu_essential_graph_batch_device(1, p, device_id, hip_stream);
}

extern "C" int orbgpu_essential_graph_correct_points_device(int32_t n_vertices, const double *d_Scw, const double *d_Siw,
                                                            int32_t n_points, const float *d_pos_in, const int32_t *d_ref,
                                                            float *d_pos_out, int32_t *d_n_bad_ref, int32_t device_id,
                                                            void *hip_stream)
{
    int rc = check_points(n_vertices, n_points);
    if (rc != ORBGPU_OK)
        return rc;
    ORBGPU_REQUIRE((n_vertices == 0 || (d_Scw && d_Siw)) && (n_points == 0 || (d_pos_in && d_ref && d_pos_out)), "null argument");
    if ((rc = select_device(device_id)) != ORBGPU_OK || n_points == 0)
        return rc;
    hipLaunchKernelGGL(k_eg_correct_points, dim3((n_points + EG_POINT_THREADS - 1) / EG_POINT_THREADS), dim3(EG_POINT_THREADS), 0,
                       (hipStream_t)hip_stream, n_vertices, d_Scw, d_Siw, n_points, d_pos_in, d_ref, d_pos_out, d_n_bad_ref);
    ORBGPU_HIP_TRY(hipGetLastError());
    return ORBGPU_OK;
}

extern "C" int orbgpu_essential_graph(const orbgpu_essential_graph_problem *p, const int32_t *stop, double *Siw_d, float *Tiw,
                                      int32_t n_points, const float *world_pos, const int32_t *point_ref, float *pos_out,
                                      orbgpu_essential_graph_result *result, int32_t device_id)
{
    ORBGPU_REQUIRE(p, "null argument");
    std::vector<EgIndex> ix(1);
    int rc = check_and_index(*p, 0, false, ix[0]);
    if (rc != ORBGPU_OK || (rc = check_points(p->n_vertices, n_points)) != ORBGPU_OK)
        return rc;
    ORBGPU_REQUIRE((p->n_vertices == 0 || Tiw) && (n_points == 0 || (world_pos && point_ref && pos_out)), "null argument");
    // the stop flag as sampled now and one staging block each way; the outputs are in/out: what a call stopped at once leaves
    // alone goes back as it came
    const size_t V = (size_t)p->n_vertices, M = (size_t)n_points;
    const int32_t stop_now = stop ? *stop : 0;
    orbgpu_essential_graph_result r;
    HostPlan<N_BUF> plan;
    const auto i_stop = plan.in(H_STOP, &stop_now, 1);
    const auto i_scw = plan.in(H_IN, p->Scw, V, 8);
    const auto i_pos = plan.in(H_IN, world_pos, M, 3);
    const auto i_ref = plan.in(H_IN, point_ref, M);
    const auto o_res = plan.out(H_OUT, &r, 1);
    const auto o_Sd = plan.inout(H_OUT, Siw_d, V, 8);
    const auto o_T = plan.inout(H_OUT, Tiw, V, 16), o_X = plan.inout(H_OUT, pos_out, M, 3);
    EgWs *wsp;
    if ((rc = host_begin(device_id, plan, wsp)) != ORBGPU_OK)
        return rc;
    EgWs &ws = *wsp;
    EgWs::FinishOnError on_error{ws};
    plan.upload(ws);
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    orbgpu_essential_graph_problem d = *p;
    d.d_stop = stop ? ws.at(i_stop) : nullptr;
    d.d_Siw_d = ws.at(o_Sd), d.d_Tiw = ws.at(o_T);
    d.d_result = ws.at(o_res);
    if ((rc = enqueue(1, &d, ix, ws, ws.stream)) != ORBGPU_OK)
        return rc;
    // the sampled flag is the one the kernel reads first: a call stopped at once has written no state to correct with
    if (M && !stop_now &&
        (rc = orbgpu_essential_graph_correct_points_device(p->n_vertices, ws.at(i_scw), d.d_Siw_d, n_points, ws.at(i_pos),
                                                           ws.at(i_ref), ws.at(o_X), &d.d_result->n_bad_ref, device_id,
                                                           ws.stream)) != ORBGPU_OK)
        return rc;
    plan.download(ws);
    if ((rc = ws.finish()) != ORBGPU_OK)
        return rc;
    if (result)
        *result = r;
    return ORBGPU_OK;
}

// The sparse solver of the Sim3 pose graph (essential_graph.hip): a symmetric positive definite system of BLOCK x BLOCK blocks,
// one block row per vertex, kept as an ENVELOPE (skyline) and solved by LL^T without fill outside it.  Pure C++ like
// opt_math.h; tests/skyline_test.cpp builds it with g++ and holds it to the dense llt_solve bit for bit.
//
// Ordering, on the host (rcm_order): reverse Cuthill-McKee over the graph of the vertices.
//   1. the degree of a vertex is the length of its neighbour list (the caller gives each neighbour once, no self loops);
//   2. while a vertex is unvisited: the component's start is the unvisited vertex of least degree, ties to the lowest row;
//      it is appended to the order, and then, for each vertex of the order in turn from the start on, its unvisited
//      neighbours are appended by ascending (degree, row);
//   3. the whole order is reversed.
// order[position] = row.  Nothing in it depends on anything but the lists, so the same graph gives the same order.  A
// closed loop is a ring: breadth-first levels from any start hold the two arcs side by side, which costs about twice the
// local bandwidth, where the caller's own order (key frames by age) would stretch the loop edges across the whole matrix.
//
// Storage (skyline_layout): per block row a, in permuted position, first_block[a] = the least block column with a
// non-zero (at most a: the diagonal is always kept).  The BLOCK scalar rows of a block row share it: scalar row i is kept
// from first[i] = BLOCK * first_block[i / BLOCK] up to i, in one piece, and entry (i, k) lives at A[off[i] + k].
// last[k] is the largest row that keeps column k, which bounds the column sweeps.
//
// skyline_llt_solve is llt_solve's algorithm (opt_math.h) entry for entry: column j left-looking with k ascending in every
// dot product, forward substitution with k ascending, back substitution with k descending, for `nt` cooperating threads
// that call `barrier()` together.  A term with a factor outside the envelope is skipped.  In the dense factorisation that
// factor is an exact zero (no fill leaves the envelope: L(i, k) with k < first[i] is 0 - sum of products with zeros), and
// s - 0 * x = s for finite x, so for finite input every kept entry and every x[i] has the bits llt_solve gives on the
// permuted dense matrix.  (The one exception IEEE allows is the sign of a zero: -0 - (-0) is +0.  The pose graph's H starts
// its sums at +0 and never holds a -0.)  A pivot that is not > 0 (NaN included): false and x = 0, the same in every thread.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "opt_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace orbgpu {

// adj_start [n + 1], adj [adj_start[n]]: the neighbour lists.  order [n] out.
inline void rcm_order(int n, const int32_t *adj_start, const int32_t *adj, int32_t *order)
{
    std::vector<uint8_t> seen((size_t)n, 0);
    auto degree = [&](int v) { return adj_start[v + 1] - adj_start[v]; };
    auto before = [&](int a, int b) { return degree(a) != degree(b) ? degree(a) < degree(b) : a < b; };
    int count = 0;
    std::vector<int32_t> next;
    while (count < n) {
        int start = -1;
        for (int v = 0; v < n; v++)
            if (!seen[v] && (start < 0 || before(v, start)))
                start = v;
        seen[start] = 1;
        order[count++] = start;
        for (int head = count - 1; head < count; head++) {
            const int v = order[head];
            next.clear();
            for (int a = adj_start[v]; a < adj_start[v + 1]; a++)
                if (!seen[adj[a]]) {
                    seen[adj[a]] = 1;
                    next.push_back(adj[a]);
                }
            std::sort(next.begin(), next.end(), before);
            for (int32_t w : next)
                order[count++] = w;
        }
    }
    std::reverse(order, order + n);
}

// first_block [nb] -> first, off, last [BLOCK * nb]; returns the envelope: the doubles A needs.
inline int64_t skyline_layout(int nb, int block, const int32_t *first_block, int32_t *first, int64_t *off, int32_t *last)
{
    int64_t at = 0;
    const int n = block * nb;
    for (int i = 0; i < n; i++) {
        first[i] = block * first_block[i / block];
        off[i] = at - first[i];
        at += i - first[i] + 1;
    }
    // block column b is kept by block rows up to the largest a with first_block[a] <= b
    std::vector<int32_t> last_block((size_t)nb);
    for (int a = 0; a < nb; a++) {
        last_block[a] = a;
        for (int b = first_block[a]; b < a; b++)
            last_block[b] = a;
    }
    for (int i = 0; i < n; i++)
        last[i] = block * last_block[i / block] + block - 1;
    return at;
}

// A x = b by LL^T.  A: the envelope, overwritten with L below the diagonal (the diagonal keeps the pivots before their
// root); v: b on entry, x on return; work: 2 n doubles.  A, v, work and the three index arrays are shared by the threads.
template <typename Barrier>
ORBGPU_HD inline bool skyline_llt_solve(int n, const int32_t *first, const int64_t *off, const int32_t *last, double *A,
                                        double *v, double *work, int tid, int nt, Barrier barrier)
{
    double *dg = work, *y = work + n;
    for (int j = 0; j < n; j++) {
        const double *Lj = A + off[j];
        const int fj = first[j], lj = last[j];
        for (int i = j + tid; i <= lj; i += nt) {
            const int fi = first[i];
            if (fi > j)
                continue;
            double *Li = A + off[i];
            double s = Li[j];
            for (int k = fi > fj ? fi : fj; k < j; k++)
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
        for (int i = j + 1 + tid; i <= lj; i += nt)
            if (first[i] <= j)
                A[off[i] + j] = A[off[i] + j] / sd;
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
        const int lk = last[k];
        for (int i = k + 1 + tid; i <= lk; i += nt)
            if (first[i] <= k)
                y[i] = y[i] - A[off[i] + k] * yk;
        barrier();
    }
    for (int k = n - 1; k >= 0; k--) {
        const double xk = y[k] / dg[k];
        const double *Lk = A + off[k];
        barrier();
        if (tid == 0)
            v[k] = xk;
        for (int i = first[k] + tid; i < k; i += nt)
            y[i] = y[i] - Lk[i] * xk;
        barrier();
    }
    return true;
}

} // namespace orbgpu

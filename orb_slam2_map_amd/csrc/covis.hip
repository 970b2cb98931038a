// Device-resident observation graph: the relation between key frames and map points, and the two votes over it.
//
// Tracking::UpdateLocalMap (Tracking.cc:1499-1643) lets every map point of the frame vote for the key frames that observe
// it (std::map copies taken under a mutex), extends the voted key frames by neighbours, children and parents, and gathers
// the map points of all of them; KeyFrame::UpdateConnections (KeyFrame.cc:327-417) is the same vote with the key frame's own
// points as the query.  Here a key frame is a row keyed by KeyFrame::mnId (id_table.h); its slots -- the id of the map
// point at every key-point index, -1 for none -- lie in one pool, key-frame-major, one int64 per slot.  That one relation
// stands for both KeyFrame::mvpMapPoints and MapPoint::mObservations (V2), and a vote streams the pool once, 8 bytes per
// slot, instead of chasing per-point maps:
//   k_covis_vote     one wave per row: a lane takes a slot and binary-searches the query's distinct ids (sorted, with
//                    multiplicities; staged in LDS, or read from global memory when the query is longer than the staging);
//                    the wave adds up the multiplicities (V5).  Integers only.
//   k_covis_list     one workgroup: the voted rows compacted in ascending id (through the id-order column), the row with
//                    the strictly greatest count (V6), the <= 80-step extension with its candidate tests spread over the
//                    lanes, and the slot prefix of the final list.
//   k_covis_insert / k_covis_count / k_covis_scan / k_covis_emit / k_covis_unhash
//                    the point gather: every slot of the list enters a device hash of 64-bit ids (integer atomicCAS on
//                    the key, atomicMin on the position in the gather order); a slot whose position is the minimum is the
//                    id's first occurrence; chunk counts, one scan and an order-preserving write follow.  The last kernel
//                    empties exactly the hash slots the call used.  The result does not depend on scheduling.
// No host decision lies between the vote and the points; a query waits twice (sizes, then lists).  Every call returns
// synchronised; the caller serialises (CovisibilityGraphT does).  Refusals are answered before any device is touched.
//
// LocalMapping::KeyFrameCulling (LocalMapping.cc:632-698) runs over the same pool and a second column beside it, one byte
// per slot: the key point's octave and its STEREO / FAR flags (V1).  The query is the distinct points of the candidates'
// slots (built from the host mirror, as orbgpu_covis_connections builds its own):
//   k_covis_cull_count    k_covis_vote's shape: one wave per row, a lane takes a slot and binary-searches the query; a hit
//                         adds the slot's weight to obs[q] and 1 to cnt[q][octave] (integer atomics).  With one level it is
//                         orbgpu_covis_observations.
//   k_covis_cull_resolve  one workgroup walks the candidates in the caller's order (V8): the row's own slots leave cnt, the
//                         lanes evaluate the slots, the verdict goes through LDS to every lane, and the slots either come
//                         back or stay out while obs drops and points at <= 2 die.  Every barrier is reached by the whole
//                         workgroup.
//   k_covis_cull_emit     the dead points in query order, which is ascending id.
// One wait per call; the graph is not modified.
//
// MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth (MapPoint.cc:242-307, :330-371) for a batch of points
// (R1-R8) run over the same pool, a third pool column (the key frames' descriptors, 32 bytes per slot, allocated by the first
// orbgpu_covis_graph_set_descriptors), a row column (the camera centres) and the scale-factor table the host hands over
// by value:
//   k_covis_cull_count    with one level: the observations per query point.
//   k_covis_refresh_scan  one workgroup: each point's start in the entry buffer (points without observations, over the cap
//                         or excluded by the table take no space), the list of points with <= 64 observations and the list
//                         of those with more, the status of every point that is not refreshed.
//   k_covis_refresh_fill  the vote's shape again: a hit takes atomicAdd(cursor[q], 1) and stores (row, slot index).
//   k_covis_refresh       two launches over the two lists: one wave per point (a 64-thread workgroup), or 256 threads per
//                         point with four entries each.  A thread ranks its (key-frame id, slot index) among the point's
//                         entries through LDS (R1's order, whatever order the atomics left), puts its descriptor and its
//                         normal term into LDS at its rank, finds the median of its distance row by bisection on the value
//                         (or from a stored row: ORBGPU_DEBUG_REFRESH_SELECT=rows, wave path), the least (median, rank) is
//                         reduced over the wave and the workgroup, and thread 0 sums the normal terms in rank order.  Every
//                         barrier stands under workgroup-uniform control flow; all global writes are plain vector stores.
// The entry buffer is as long as the pool slots in use -- a slot holds one id and the query's ids are distinct, so no call
// needs more -- which spares the wait for the total: one wait per call.  The graph is not modified.
#include "common.h"
#include "compact_kernels.h"
#include "compact_plan.h"
#include "id_table.h"
#include "refresh_internal.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <unordered_map>
#include <vector>

namespace orbgpu {

constexpr int CV_MAX_NB = ORBGPU_COVIS_MAX_COVISIBLES;  // GetBestCovisibilityKeyFrames(10)
constexpr int CV_MAX_SLOTS = ORBGPU_COVIS_MAX_SLOTS;    // slots of a row, key points of a query
constexpr int CV_MAX_ROWS = 1 << 20;                    // first choices, as local BA's caps were
constexpr int64_t CV_MAX_POOL = (int64_t)1 << 30;
constexpr int CV_MAX_CALL = 1 << 20;                    // entries of a batched edit, ids of a previous list
constexpr int CV_MAX_POINTS = 1 << 22;                  // local map points of one query
constexpr int CV_MAX_LOCAL_KFS = 80;                    // Tracking.cc:1589
constexpr int CV_LDS_IDS = 4096;                        // distinct query ids staged per block (8 + 4 bytes each: 48 KiB)
constexpr int CV_BLOCK = 256;
constexpr int CV_WAVES = CV_BLOCK / 64;
constexpr int CV_LIST_BLOCK = 1024;
constexpr int CV_CHUNK = 1024;  // gather positions per chunk: four steps of a 256-thread block
constexpr int32_t CV_POS_NONE = 0x7F7F7F7F;  // (hipMemset's byte pattern) above every gather position (< 2^30)
constexpr int CV_LEVELS = ORBGPU_COVIS_MAX_LEVELS;
constexpr int CV_MAX_CANDIDATES = 1 << 16;      // key frames of one culling call
constexpr int64_t CV_OFF_NONE = INT64_MIN / 2;  // CvRow::off of a bad row a compaction kept (C3): off + idx < 0 for every slot index
constexpr int CV_MAX_QUERY_POINTS = 1 << 20;    // distinct points of their slots (64 bytes of counters each); a first choice
static_assert(CV_LEVELS == 16 && (ORBGPU_COVIS_KP_STEREO | ORBGPU_COVIS_KP_FAR) == 0xC0, "the attribute byte of V1");

struct CvRow {  // 120 bytes; the host keeps a mirror and uploads the part an edit changes
    int64_t id;
    int64_t parent;  // -1: none; need not be a row
    int64_t off;     // the row's slots in the pool
    int32_t n_slots, bad;
    int32_t nn, has_desc;  // has_desc: orbgpu_covis_graph_set_descriptors has filled the row's part of the third pool column
    int64_t nb[CV_MAX_NB];
};

// header of a query, written by the kernels and downloaded with the first wait
enum { CH_LIST = 0, CH_VOTED, CH_REF, CH_MAX, CH_KEPT, CH_SLOTS, CH_POINTS, CH_USED, CH_OVERFLOW, CH_RANGE, CH_WORDS };

// exclusive prefix of v over the block in thread order, and the block's total; every thread of the block calls it
__device__ __forceinline__ int block_scan_excl(int v, int *s_w, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off, 64);
        if (lane >= off)
            incl += o;
    }
    __syncthreads();  // the previous call's reads of s_w are over
    if (lane == 63)
        s_w[wave] = incl;
    __syncthreads();
    int base = 0, all = 0;
    for (int i = 0; i < nw; i++) {
        if (i < wave)
            base += s_w[i];
        all += s_w[i];
    }
    total = all;
    return base + incl - v;
}

__global__ __launch_bounds__(256) void k_covis_scatter(int n, const int64_t *__restrict__ addr, const int64_t *__restrict__ val,
                                                       int64_t pool_used, int64_t *__restrict__ pool)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && addr[i] >= 0 && addr[i] < pool_used)  // (addresses are distinct: the host keeps the last entry of each)
        pool[addr[i]] = val[i];
}

// count[row] = sum over the row's slots of the multiplicity of the slot's id in the query (V5); 0 for a bad row and for
// `exclude_row` (orbgpu_covis_connections: the key frame itself).  Saturates at INT_MAX.
template <bool LDS>
__global__ __launch_bounds__(CV_BLOCK) void k_covis_vote(int n_rows, const CvRow *__restrict__ rows, const int64_t *__restrict__ pool,
                                                         int64_t pool_used, int nq, const int64_t *__restrict__ q_ids,
                                                         const int32_t *__restrict__ q_mult, int exclude_row,
                                                         int32_t *__restrict__ count)
{
    extern __shared__ int64_t s_cv[];
    const int64_t *q = q_ids;
    const int32_t *m = q_mult;
    if (LDS) {  // a template constant: the barrier is under workgroup-uniform control flow
        int32_t *s_m = reinterpret_cast<int32_t *>(s_cv + nq);
        for (int i = threadIdx.x; i < nq; i += CV_BLOCK) {
            s_cv[i] = q_ids[i];
            s_m[i] = q_mult[i];
        }
        __syncthreads();
        q = s_cv;
        m = s_m;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int row = blockIdx.x * CV_WAVES + wave; row < n_rows; row += gridDim.x * CV_WAVES) {  // wave-uniform
        const int64_t off = rows[row].off;
        const int len = rows[row].n_slots;
        const bool live = !rows[row].bad && row != exclude_row && off >= 0 && len >= 0 && off + len <= pool_used;
        unsigned sum = 0;  // per lane at most 2^10 slots of multiplicity 2^16
        if (live && nq > 0) {
            for (int e = lane; e < len; e += 64) {
                const int64_t id = pool[off + e];
                if (id < 0)
                    continue;
                int lo = 0, hi = nq;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (q[mid] < id)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                if (lo < nq && q[lo] == id)
                    sum += (unsigned)m[lo];
            }
        }
        long long total = sum;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            total += __shfl_down(total, o, 64);
        if (lane == 0)
            count[row] = (int32_t)(total > INT_MAX ? INT_MAX : total);
    }
}

struct CvList {  // the list a query builds, in the call's staging
    int cap;
    int32_t *rows;
    int64_t *ids;
    int32_t *counts;
    int32_t *prefix;  // cap + 1: slots before every entry, then their total
};

__device__ __forceinline__ void covis_append(const CvList &l, int k, int r, const CvRow *rows, const int32_t *count, int32_t *stamp,
                                             int cur)
{
    if (k < l.cap) {
        l.rows[k] = r;
        l.ids[k] = rows[r].id;
        l.counts[k] = count[r];
    }
    stamp[r] = cur;
}

// mode 0: orbgpu_covis_local_map (V6).  mode 1: orbgpu_covis_connections (V7): the counter only, nothing stamped.
__global__ __launch_bounds__(CV_LIST_BLOCK) void k_covis_list(int mode, int n_rows, const CvRow *__restrict__ rows,
                                                              const int32_t *__restrict__ order, const int32_t *__restrict__ count,
                                                              int32_t *stamp, int cur, const int64_t *__restrict__ hkeys,
                                                              const int32_t *__restrict__ hvals, int log2cap, int n_prev,
                                                              const int32_t *__restrict__ prev_rows, CvList l, long long *hdr)
{
    __shared__ int s_w[CV_LIST_BLOCK / 64];
    __shared__ unsigned long long s_best[CV_LIST_BLOCK / 64];
    __shared__ int s_cand, s_nb[CV_MAX_NB];
    const int tid = threadIdx.x;
    // K1: the not-bad rows with a vote, in ascending id; the first of them with the strictly greatest count
    int n = 0;
    unsigned long long best = 0;
    for (int base = 0; base < n_rows; base += CV_LIST_BLOCK) {
        const int p = base + tid;
        int r = -1;
        if (p < n_rows) {
            const int o = order[p];
            if (o >= 0 && o < n_rows && !rows[o].bad && count[o] > 0)
                r = o;
        }
        int total;
        const int k = n + block_scan_excl(r >= 0, s_w, total);
        if (r >= 0) {
            if (k < l.cap) {
                l.rows[k] = r;
                l.ids[k] = rows[r].id;
                l.counts[k] = count[r];
            }
            if (mode == 0)
                stamp[r] = cur;
            const unsigned long long key = ((unsigned long long)(unsigned)count[r] << 32) | (0xFFFFFFFFu - (unsigned)k);
            best = key > best ? key : best;
        }
        n += total;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(best, off, 64);
        best = o > best ? o : best;
    }
    if ((tid & 63) == 0)
        s_best[tid >> 6] = best;
    __syncthreads();  // (also: the list and the stamps written above are visible to the whole workgroup)
    best = s_best[0];
    for (int i = 1; i < CV_LIST_BLOCK / 64; i++)
        best = s_best[i] > best ? s_best[i] : best;
    n = min(n, l.cap);
    int L = n, kept = 0;
    if (mode == 0 && n == 0) {  // Tracking.cc:1557-1558: no vote, the previous list stays
        kept = 1;
        L = min(n_prev, l.cap);
        for (int i = tid; i < L; i += CV_LIST_BLOCK) {
            const int r = min(max(prev_rows[i], 0), n_rows - 1);
            l.rows[i] = r;
            l.ids[i] = rows[r].id;
            l.counts[i] = 0;
        }
    } else if (mode == 0) {
        // Tracking.cc:1586-1636 over the positions of K1 only; the list grows behind them
        for (int pos = 0; pos < n && pos <= CV_MAX_LOCAL_KFS; pos++) {
            if (L > CV_MAX_LOCAL_KFS)
                break;
            __syncthreads();
            const int r = l.rows[pos];
            // (a) the first stored covisible that is known, not bad and not stamped
            if (tid == 0)
                s_cand = INT_MAX;
            __syncthreads();
            if (tid < CV_MAX_NB && tid < rows[r].nn) {
                const int r2 = id_hash_lookup(hkeys, hvals, log2cap, rows[r].nb[tid]);
                s_nb[tid] = r2;
                if (r2 >= 0 && r2 < n_rows && !rows[r2].bad && stamp[r2] != cur)
                    atomicMin(&s_cand, tid);
            }
            __syncthreads();
            if (s_cand != INT_MAX) {
                if (tid == 0)
                    covis_append(l, L, s_nb[s_cand], rows, count, stamp, cur);
                L++;
            }
            __syncthreads();
            // (b) the first child (V3: rows whose parent is this one, ascending id) that is not bad and not stamped
            if (tid == 0)
                s_cand = INT_MAX;
            __syncthreads();
            const int64_t id = rows[r].id;
            for (int p = tid; p < n_rows; p += CV_LIST_BLOCK) {
                const int r2 = order[p];
                if (r2 >= 0 && r2 < n_rows && rows[r2].parent == id && !rows[r2].bad && stamp[r2] != cur) {
                    atomicMin(&s_cand, p);
                    break;  // a thread's positions ascend
                }
            }
            __syncthreads();
            if (s_cand != INT_MAX) {
                if (tid == 0)
                    covis_append(l, L, order[s_cand], rows, count, stamp, cur);
                L++;
            }
            __syncthreads();
            // (c) the parent, with no bad test; the `break` of Tracking.cc:1632 leaves the OUTER loop
            if (tid == 0) {
                const int r2 = id_hash_lookup(hkeys, hvals, log2cap, rows[r].parent);
                s_cand = r2 >= 0 && r2 < n_rows && stamp[r2] != cur ? r2 : -1;
            }
            __syncthreads();
            if (s_cand >= 0) {
                if (tid == 0)
                    covis_append(l, L, s_cand, rows, count, stamp, cur);
                L++;
                break;
            }
        }
        L = min(L, l.cap);
    }
    __syncthreads();
    // slots before every entry of the final list (the gather order of the points)
    int run = 0;
    if (mode == 0)
        for (int base = 0; base < L; base += CV_LIST_BLOCK) {
            const int i = base + tid;
            int v = 0;
            if (i < L) {
                const int r = l.rows[i];
                v = r >= 0 && r < n_rows ? min(max(rows[r].n_slots, 0), CV_MAX_SLOTS) : 0;
            }
            int total;
            const int ex = block_scan_excl(v, s_w, total);
            if (i < L)
                l.prefix[i] = run + ex;
            if (total > (1 << 30) - run) {  // (the host bounds the sum; an overflow would be a bug, not a fault)
                total = 0;
                if (tid == 0)
                    hdr[CH_RANGE] = 1;
            }
            run += total;
        }
    if (tid == 0) {
        if (mode == 0)
            l.prefix[L] = run;
        const int kb = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull));
        hdr[CH_LIST] = L;
        hdr[CH_VOTED] = n;
        hdr[CH_REF] = n > 0 && kb >= 0 && kb < n ? l.ids[kb] : -1;
        hdr[CH_MAX] = n > 0 ? (long long)(best >> 32) : 0;
        hdr[CH_KEPT] = kept;
        hdr[CH_SLOTS] = run;
    }
}

// gather position p -> the id in that slot; false for an empty slot (and for an index outside its range)
__device__ __forceinline__ bool covis_slot_at(int p, int L, const CvList &l, int n_rows, const CvRow *__restrict__ rows,
                                              const int64_t *__restrict__ pool, int64_t pool_used, int64_t &id)
{
    int lo = 0, hi = L;  // prefix[lo] <= p < prefix[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (l.prefix[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    const int r = l.rows[lo];
    if (r < 0 || r >= n_rows)
        return false;
    const int idx = p - l.prefix[lo];
    const int64_t a = rows[r].off + idx;
    if (idx < 0 || idx >= rows[r].n_slots || a < 0 || a >= pool_used)
        return false;
    id = pool[a];
    return id >= 0;
}

struct CvPointHash {
    int log2cap;
    int limit;  // entries the call may make (<= capacity / 2)
    int64_t *keys;
    int32_t *pos;
    int32_t *used;  // the slots the call filled, in any order: k_covis_unhash empties them
};

__global__ __launch_bounds__(CV_BLOCK) void k_covis_insert(CvList l, int n_rows, const CvRow *__restrict__ rows,
                                                           const int64_t *__restrict__ pool, int64_t pool_used, CvPointHash h,
                                                           long long *hdr)
{
    const int L = (int)hdr[CH_LIST], T = (int)hdr[CH_SLOTS];
    const uint32_t mask = (1u << h.log2cap) - 1u;
    for (int p = blockIdx.x * CV_BLOCK + threadIdx.x; p < T; p += gridDim.x * CV_BLOCK) {
        int64_t id;
        if (!covis_slot_at(p, L, l, n_rows, rows, pool, pool_used, id))
            continue;
        uint32_t s = id_hash_slot(id, h.log2cap);
        bool placed = false;
        for (uint32_t probe = 0; probe <= mask && !placed; probe++, s = (s + 1) & mask) {
            const unsigned long long was = atomicCAS(reinterpret_cast<unsigned long long *>(h.keys + s),
                                                     (unsigned long long)ID_HASH_EMPTY, (unsigned long long)id);
            if (was == (unsigned long long)ID_HASH_EMPTY) {
                const unsigned long long k = atomicAdd(reinterpret_cast<unsigned long long *>(hdr + CH_USED), 1ull);
                if (k < (unsigned long long)h.limit)
                    h.used[k] = (int32_t)s;
                else
                    hdr[CH_OVERFLOW] = 1;
            }
            if (was == (unsigned long long)ID_HASH_EMPTY || was == (unsigned long long)id) {
                atomicMin(h.pos + s, p);
                placed = true;
            }
        }
        if (!placed)
            hdr[CH_OVERFLOW] = 1;
    }
}

// is gather position p the first occurrence of its id?
__device__ __forceinline__ bool covis_first_at(int p, int L, const CvList &l, int n_rows, const CvRow *__restrict__ rows,
                                               const int64_t *__restrict__ pool, int64_t pool_used, const CvPointHash &h, int64_t &id)
{
    if (!covis_slot_at(p, L, l, n_rows, rows, pool, pool_used, id))
        return false;
    const uint32_t mask = (1u << h.log2cap) - 1u;
    uint32_t s = id_hash_slot(id, h.log2cap);
    for (uint32_t probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {
        const int64_t k = h.keys[s];
        if (k == id)
            return h.pos[s] == p;
        if (k == ID_HASH_EMPTY)
            return false;
    }
    return false;
}

__global__ __launch_bounds__(CV_BLOCK) void k_covis_count(CvList l, int n_rows, const CvRow *__restrict__ rows,
                                                          const int64_t *__restrict__ pool, int64_t pool_used, CvPointHash h,
                                                          const long long *__restrict__ hdr, int n_chunks_cap,
                                                          int32_t *__restrict__ chunks)
{
    __shared__ int s_n;
    const int L = (int)hdr[CH_LIST], T = (int)hdr[CH_SLOTS];
    const int n_chunks = min((T + CV_CHUNK - 1) / CV_CHUNK, n_chunks_cap);
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {  // workgroup-uniform
        if (threadIdx.x == 0)
            s_n = 0;
        __syncthreads();
        int mine = 0;
        for (int p = c * CV_CHUNK + threadIdx.x; p < min((c + 1) * CV_CHUNK, T); p += CV_BLOCK) {
            int64_t id;
            mine += covis_first_at(p, L, l, n_rows, rows, pool, pool_used, h, id);
        }
        mine = wave_reduce_add(mine);
        if ((threadIdx.x & 63) == 0)
            atomicAdd(&s_n, mine);  // an integer sum: the same in any order
        __syncthreads();
        if (threadIdx.x == 0)
            chunks[c] = s_n;
        __syncthreads();
    }
}

__global__ __launch_bounds__(CV_LIST_BLOCK) void k_covis_scan(int n_chunks_cap, int32_t *chunks, long long *hdr)
{
    __shared__ int s_w[CV_LIST_BLOCK / 64];
    const int T = (int)hdr[CH_SLOTS];
    const int n_chunks = min((T + CV_CHUNK - 1) / CV_CHUNK, n_chunks_cap);
    int run = 0;
    for (int base = 0; base < n_chunks; base += CV_LIST_BLOCK) {
        const int c = base + threadIdx.x;
        const int v = c < n_chunks ? chunks[c] : 0;
        int total;
        const int ex = block_scan_excl(v, s_w, total);
        if (c < n_chunks)
            chunks[c] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0)
        hdr[CH_POINTS] = run;
}

__global__ __launch_bounds__(CV_BLOCK) void k_covis_emit(CvList l, int n_rows, const CvRow *__restrict__ rows,
                                                         const int64_t *__restrict__ pool, int64_t pool_used, CvPointHash h,
                                                         const long long *__restrict__ hdr, int n_chunks_cap,
                                                         const int32_t *__restrict__ chunks, int out_cap, int64_t *__restrict__ out)
{
    __shared__ int s_w[CV_WAVES];
    const int L = (int)hdr[CH_LIST], T = (int)hdr[CH_SLOTS];
    const int n_chunks = min((T + CV_CHUNK - 1) / CV_CHUNK, n_chunks_cap);
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {  // workgroup-uniform
        int run = chunks[c];
        for (int step = 0; step < CV_CHUNK / CV_BLOCK; step++) {
            const int p = c * CV_CHUNK + step * CV_BLOCK + threadIdx.x;
            int64_t id = -1;
            const bool first = p < T && covis_first_at(p, L, l, n_rows, rows, pool, pool_used, h, id);
            int total;
            const int k = run + block_scan_excl(first, s_w, total);
            if (first && k >= 0 && k < out_cap)
                out[k] = id;
            run += total;
        }
    }
}

__global__ __launch_bounds__(256) void k_covis_unhash(CvPointHash h, const long long *__restrict__ hdr)
{
    const int n = (int)min(hdr[CH_USED], (long long)h.limit);
    const uint32_t mask = (1u << h.log2cap) - 1u;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        const uint32_t s = (uint32_t)h.used[k] & mask;
        h.keys[s] = ID_HASH_EMPTY;
        h.pos[s] = CV_POS_NONE;
    }
}

// header of a culling call
enum { CU_CULLED = 0, CU_TO_BE_ERASED, CU_SKIPPED, CU_BAD, CU_WORDS };
static_assert(CU_WORDS <= CH_WORDS, "the culling header lies in the query header's buffer");

// the position of id in the sorted distinct ids q[0..nq), -1 if it is not there
__device__ __forceinline__ int covis_find(const int64_t *q, int nq, int64_t id)
{
    int lo = 0, hi = nq;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (q[mid] < id)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < nq && q[lo] == id ? lo : -1;
}

// Over every slot of every row that is not bad and holds a query point q: obs[q] += the slot's weight (2 if STEREO),
// cnt[q * levels + (octave & (levels - 1))] += 1.  levels is 16 (culling) or 1 (orbgpu_covis_observations: the number of
// slots).  obs and cnt start at zero; integer atomics, so the sums do not depend on the order.
template <bool LDS>
__global__ __launch_bounds__(CV_BLOCK) void k_covis_cull_count(int n_rows, const CvRow *__restrict__ rows, const int64_t *__restrict__ pool,
                                                               const uint8_t *__restrict__ kp, int64_t pool_used, int nq,
                                                               const int64_t *__restrict__ q_ids, int levels, int32_t *obs, int32_t *cnt)
{
    extern __shared__ int64_t s_cv[];
    const int64_t *q = q_ids;
    if (LDS) {  // a template constant: the barrier is under workgroup-uniform control flow
        for (int i = threadIdx.x; i < nq; i += CV_BLOCK)
            s_cv[i] = q_ids[i];
        __syncthreads();
        q = s_cv;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int row = blockIdx.x * CV_WAVES + wave; row < n_rows; row += gridDim.x * CV_WAVES) {  // wave-uniform
        const int64_t off = rows[row].off;
        const int len = rows[row].n_slots;
        if (rows[row].bad || off < 0 || len < 0 || off + len > pool_used)
            continue;
        for (int e = lane; e < len; e += 64) {
            const int64_t id = pool[off + e];
            if (id < 0)
                continue;
            const int k = covis_find(q, nq, id);
            if (k < 0)
                continue;
            const unsigned a = kp[off + e];
            atomicAdd(obs + k, (a & ORBGPU_COVIS_KP_STEREO) ? 2 : 1);
            atomicAdd(cnt + (size_t)k * levels + (a & (unsigned)(levels - 1)), 1);
        }
    }
}

struct CvCull {  // a culling call's arrays, in the handle's staging
    int n, nq, th;
    const int64_t *q;         // the query: sorted distinct point ids
    const int32_t *cand_row;  // per candidate: its row, -1 for one the host knows to be skipped (id 0, no row, a bad row)
    const int32_t *first;     // per candidate: the first position that names the same row
    const uint8_t *not_erase;
    int32_t *obs, *cnt;       // Obs_S(q); slots of S that hold q, per octave
    uint8_t *dead, *culled;   // per query point; per candidate position (indexed by `first`)
    int8_t *verdict;
    int32_t *n_mps, *n_red;
    int slot_cap;             // the longest candidate row
    int32_t *slot_q;          // the current candidate's slots as query positions, -1 for none
};

// V8: the candidates in order, one workgroup.  s_row / s_verdict carry the two decisions to every lane, so that every
// barrier below stands under workgroup-uniform control flow.
__global__ __launch_bounds__(CV_LIST_BLOCK) void k_covis_cull_resolve(CvCull c, int n_rows, const CvRow *__restrict__ rows,
                                                                      const int64_t *__restrict__ pool, const uint8_t *__restrict__ kp,
                                                                      int64_t pool_used, long long *hdr)
{
    __shared__ int s_row, s_verdict, s_mps, s_red;
    const int tid = threadIdx.x;
    int n_culled = 0, n_keep = 0, n_skip = 0;  // thread 0's
    for (int k = 0; k < c.n; k++) {
        if (tid == 0) {
            int r = c.cand_row[k];
            const int f = c.first[k];
            if (r < 0 || r >= n_rows || f < 0 || f > k || c.culled[f])
                r = -1;
            else if (rows[r].bad || rows[r].off < 0 || rows[r].n_slots < 0 || rows[r].n_slots > c.slot_cap ||
                     rows[r].off + rows[r].n_slots > pool_used)
                r = -1;
            s_row = r;
            s_mps = s_red = 0;
        }
        __syncthreads();
        const int r = s_row;
        if (r < 0) {  // workgroup-uniform
            if (tid == 0) {
                c.verdict[k] = -1;
                c.n_mps[k] = c.n_red[k] = 0;
                n_skip++;
            }
            __syncthreads();  // s_row has been read
            continue;
        }
        const int64_t off = rows[r].off;
        const int len = rows[r].n_slots;
        // A lane looks its slots up once; in every phase below it takes the same slots, so it reads back its own stores.
        // The row's own slots leave the counts (pKFi == pKF).
        for (int e = tid; e < len; e += CV_LIST_BLOCK) {
            const int64_t id = pool[off + e];
            const int qi = id >= 0 ? covis_find(c.q, c.nq, id) : -1;
            c.slot_q[e] = qi;
            if (qi >= 0)
                atomicSub(c.cnt + (size_t)qi * CV_LEVELS + (kp[off + e] & (CV_LEVELS - 1)), 1);
        }
        __syncthreads();
        int mps = 0, red = 0;
        for (int e = tid; e < len; e += CV_LIST_BLOCK) {
            const int qi = c.slot_q[e];
            const unsigned a = kp[off + e];
            if (qi < 0 || c.dead[qi] || (a & ORBGPU_COVIS_KP_FAR))
                continue;
            mps++;
            if (c.obs[qi] > c.th) {
                const int top = min((int)(a & (CV_LEVELS - 1)) + 1, CV_LEVELS - 1);
                int others = 0;
                for (int l = 0; l <= top; l++)
                    others += c.cnt[(size_t)qi * CV_LEVELS + l];
                red += others >= c.th;
            }
        }
        mps = wave_reduce_add(mps);
        red = wave_reduce_add(red);
        if ((tid & 63) == 0) {
            atomicAdd(&s_mps, mps);  // integer sums: the same in any order
            atomicAdd(&s_red, red);
        }
        __syncthreads();
        if (tid == 0) {
            int v = (double)s_red > 0.9 * (double)s_mps ? 1 : 0;  // LocalMapping.cc:695, in FP64 as written
            if (v && c.not_erase[k])
                v = 2;
            if (v == 1) {
                c.culled[c.first[k]] = 1;
                n_culled++;
            }
            n_keep += v == 2;
            c.verdict[k] = (int8_t)v;
            c.n_mps[k] = s_mps;
            c.n_red[k] = s_red;
            s_verdict = v;
        }
        __syncthreads();
        const bool gone = s_verdict == 1;  // read by every lane before the branch
        for (int e = tid; e < len; e += CV_LIST_BLOCK) {
            const int qi = c.slot_q[e];
            if (qi < 0)
                continue;
            const unsigned a = kp[off + e];
            if (gone)
                atomicSub(c.obs + qi, (a & ORBGPU_COVIS_KP_STEREO) ? 2 : 1);  // the slot has left S
            else
                atomicAdd(c.cnt + (size_t)qi * CV_LEVELS + (a & (CV_LEVELS - 1)), 1);
        }
        __syncthreads();
        if (gone)
            for (int e = tid; e < len; e += CV_LIST_BLOCK) {
                const int qi = c.slot_q[e];
                if (qi >= 0 && !c.dead[qi] && c.obs[qi] <= 2)
                    c.dead[qi] = 1;  // MapPoint.cc:130 (lanes that meet in one point write the same value)
            }
        __syncthreads();
    }
    if (tid == 0) {
        hdr[CU_CULLED] = n_culled;
        hdr[CU_TO_BE_ERASED] = n_keep;
        hdr[CU_SKIPPED] = n_skip;
    }
}

// the dead points in query order (ascending id); at most out_cap are written, the count is full
__global__ __launch_bounds__(CV_LIST_BLOCK) void k_covis_cull_emit(int nq, const int64_t *__restrict__ q, const uint8_t *__restrict__ dead,
                                                                   int out_cap, int64_t *__restrict__ out, long long *hdr)
{
    __shared__ int s_w[CV_LIST_BLOCK / 64];
    int run = 0;
    for (int base = 0; base < nq; base += CV_LIST_BLOCK) {
        const int i = base + threadIdx.x;
        const bool d = i < nq && dead[i];
        int total;
        const int k = run + block_scan_excl(d, s_w, total);
        if (d && k < out_cap)
            out[k] = q[i];
        run += total;
    }
    if (threadIdx.x == 0)
        hdr[CU_BAD] = run;
}

// ---- the refresh of descriptor, normal and depth (R1-R8) ------------------------------------------------------------------
constexpr int CV_REFRESH_MAX_OBS = ORBGPU_COVIS_REFRESH_MAX_OBS;
constexpr int CV_REFRESH_MAX_POINTS = 1 << 20;  // ids of one call; a first choice, like CV_MAX_QUERY_POINTS
constexpr int CV_REFRESH_WAVE = 64;             // observations the one-wave path takes
constexpr unsigned CV_REFRESH_HALVES = ORBGPU_REFRESH_DESCRIPTOR | ORBGPU_REFRESH_NORMAL_DEPTH;
enum { RH_ENTRIES = 0, RH_WAVE, RH_GROUP, RH_RANGE, RH_WORDS };  // header of a refresh (the first words of d_hdr)
static_assert(RH_WORDS <= CH_WORDS, "the refresh header lies in d_hdr");
static_assert(CV_MAX_POOL <= INT_MAX, "entry positions (CvRefresh::start, and its sums with a cursor) are 32-bit");

struct CvCentre {  // the row column: KeyFrame::GetCameraCenter()
    float x, y, z;
    int32_t has;
};

struct CvScale {  // KeyFrame::mvScaleFactors, by value
    int32_t n_levels;  // 0: not set
    float sf[CV_LEVELS];
};

struct CvEntry {  // an observation: the row and the slot index
    int32_t row, idx;
};

struct CvRefresh {  // a refresh call's arrays, in the handle's staging
    int nq;
    unsigned what;
    const int64_t *q;        // the query: sorted distinct point ids
    const int32_t *perm;     // sorted position -> the caller's index; every array below `cursor` goes by the caller's index
    const int32_t *ref_row;  // the row of mpRefKF, -1 for an unknown or bad one
    const float *pos;        // [n][3]
    const uint8_t *pre;      // table form: ORBGPU_REFRESH_UNKNOWN / ORBGPU_REFRESH_BAD; nullptr otherwise
    const int32_t *t_row;    // table form: the table row that takes the results
    float *t_normal, *t_min, *t_max;
    uint8_t *t_desc;
    int32_t *obs, *cnt, *cursor, *start;  // per sorted position: k_covis_cull_count's two sums, entries stored, first entry
    int32_t *list_w, *list_g;             // sorted positions with <= 64 observations, with more
    float *normal, *min_dist, *max_dist;  // the results, by the caller's index
    uint8_t *desc;
    int64_t *desc_kf;
    int32_t *desc_idx, *n_slots;
    uint8_t *status;
    int64_t ent_cap;
    CvEntry *ents;
};

__global__ __launch_bounds__(CV_LIST_BLOCK) void k_covis_refresh_scan(CvRefresh c, long long *hdr)
{
    __shared__ int s_w[CV_LIST_BLOCK / 64];
    long long run_e = 0;
    int run_w = 0, run_g = 0;
    for (int base = 0; base < c.nq; base += CV_LIST_BLOCK) {
        const int k = base + threadIdx.x;
        int n = 0, st = 0, ci = 0;
        if (k < c.nq) {
            ci = c.perm[k];
            n = c.cnt[k];
            const int pre = c.pre ? c.pre[ci] : 0;
            st = pre ? pre : n == 0 ? ORBGPU_REFRESH_NO_OBS : n > CV_REFRESH_MAX_OBS ? ORBGPU_REFRESH_OVERFLOW : 0;
        }
        const bool live = k < c.nq && st == 0;
        const bool wave = live && n <= CV_REFRESH_WAVE, group = live && n > CV_REFRESH_WAVE;
        int te, tw, tg;
        const int xe = block_scan_excl(live ? n : 0, s_w, te);  // (at most 2^10 points of 2^10 entries per step)
        const int xw = block_scan_excl(wave, s_w, tw);
        const int xg = block_scan_excl(group, s_w, tg);
        if (k < c.nq) {
            c.start[k] = live ? (int)(run_e + xe) : -1;  // (below ent_cap <= CV_MAX_POOL, which fits: see the assertion)
            if (wave)
                c.list_w[run_w + xw] = k;
            if (group)
                c.list_g[run_g + xg] = k;
            c.status[ci] = (uint8_t)st;  // (k_covis_refresh writes a refreshed point's again)
            c.n_slots[ci] = n;
            c.desc_kf[ci] = -1;
            c.desc_idx[ci] = -1;
        }
        run_e += te;
        run_w += tw;
        run_g += tg;
    }
    if (threadIdx.x == 0) {
        hdr[RH_ENTRIES] = run_e;
        hdr[RH_WAVE] = run_w;
        hdr[RH_GROUP] = run_g;
        if (run_e > c.ent_cap)
            hdr[RH_RANGE] = 1;
    }
}

// Every slot of a row that is not bad and holds a point with a list: (row, slot index) goes to the point's next free entry.
template <bool LDS>
__global__ __launch_bounds__(CV_BLOCK) void k_covis_refresh_fill(int n_rows, const CvRow *__restrict__ rows, const int64_t *__restrict__ pool,
                                                                 int64_t pool_used, CvRefresh c, long long *hdr)
{
    extern __shared__ int64_t s_cv[];
    const int64_t *q = c.q;
    if (LDS) {  // a template constant: the barrier is under workgroup-uniform control flow
        for (int i = threadIdx.x; i < c.nq; i += CV_BLOCK)
            s_cv[i] = c.q[i];
        __syncthreads();
        q = s_cv;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int row = blockIdx.x * CV_WAVES + wave; row < n_rows; row += gridDim.x * CV_WAVES) {  // wave-uniform
        const int64_t off = rows[row].off;
        const int len = rows[row].n_slots;
        if (rows[row].bad || off < 0 || len < 0 || off + len > pool_used)
            continue;
        for (int e = lane; e < len; e += 64) {
            const int64_t id = pool[off + e];
            if (id < 0)
                continue;
            const int k = covis_find(q, c.nq, id);
            if (k < 0)
                continue;
            const int s = c.start[k];
            if (s < 0)
                continue;
            const int p = atomicAdd(c.cursor + k, 1);  // R8: where the entry lands; k_covis_refresh orders the list itself
            if (p >= c.cnt[k] || (int64_t)s + p >= c.ent_cap) {
                hdr[RH_RANGE] = 1;
                continue;
            }
            c.ents[s + p] = CvEntry{row, e};
        }
    }
}

// the k-th smallest of the n distances of a to the descriptors sd[0..n) (a is one of them), k = (n - 1) >> 1: the smallest
// v with #{j : d_j <= v} >= k + 1, by bisection on [0, 256] (k_distinctive's).  dist != nullptr: the row was stored there.
__device__ __forceinline__ int refresh_median(const uint64_t a[4], const uint64_t *sd, int n, const uint16_t *dist)
{
    const int k = (n - 1) >> 1;
    int lo = 0, hi = 256;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int cnt = 0;
        for (int j = 0; j < n; j++) {
            int d;
            if (dist)
                d = dist[j];
            else {
                const uint64_t b[4] = {sd[j * 4], sd[j * 4 + 1], sd[j * 4 + 2], sd[j * 4 + 3]};
                d = hamming256(a, b);
            }
            cnt += d <= mid ? 1 : 0;
        }
        if (cnt >= k + 1)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// One workgroup of BLOCK threads per point of the list (`group`: list_g, otherwise list_w), PER entries per thread; the
// scan put a point on a list whose BLOCK * PER holds its observations.  ROWS (one wave, one entry per thread): the distance
// row is stored in LDS once and the bisection counts over it.
template <int BLOCK, int PER, bool ROWS>
__global__ __launch_bounds__(BLOCK) void k_covis_refresh(int group, const CvRow *__restrict__ rows, const uint8_t *__restrict__ kp,
                                                         const uint8_t *__restrict__ descs, const CvCentre *__restrict__ centres,
                                                         CvScale sc, CvRefresh c, const long long *__restrict__ hdr)
{
    constexpr int CAP = BLOCK * PER;
    constexpr int DSTRIDE = CAP + 2;  // halfwords: an odd number of words, so that the lanes' rows fall into distinct banks
    static_assert(!ROWS || (BLOCK == 64 && PER == 1), "the stored distance row is the one-wave path's");
    __shared__ int64_t s_kf[CAP];
    __shared__ int32_t s_e[CAP];
    __shared__ __align__(16) uint64_t s_d[CAP * 4];
    __shared__ float s_t[CAP * 3];
    __shared__ uint16_t s_dist[ROWS ? CAP * DSTRIDE : 1];
    __shared__ unsigned long long s_best;
    __shared__ int s_flags, s_ref_e, s_ref_level;
    __shared__ float s_ref_dist;
    const int tid = threadIdx.x;
    if (hdr[RH_RANGE])  // an index left its range in the scan or the fill: the host reports it, nothing is read
        return;
    const int n_list = (int)hdr[group ? RH_GROUP : RH_WAVE];
    const int32_t *list = group ? c.list_g : c.list_w;
    for (int li = blockIdx.x; li < n_list; li += gridDim.x) {  // workgroup-uniform, as is everything a barrier stands under
        const int k = list[li];
        const int n = min(c.cnt[k], CAP), base = c.start[k], ci = c.perm[k];
        const int ref = c.ref_row[ci];
        const float px = c.pos[3 * (size_t)ci], py = c.pos[3 * (size_t)ci + 1], pz = c.pos[3 * (size_t)ci + 2];
        if (tid == 0) {
            s_best = ~0ull;
            s_flags = 0;
            s_ref_e = INT_MAX;
        }
        int row[PER], e[PER], rank[PER];
        int64_t kf[PER], off[PER];
        float tx[PER], ty[PER], tz[PER], dist[PER];
        int flags = 0;
#pragma unroll
        for (int m = 0; m < PER; m++) {
            const int t = tid + m * BLOCK;
            row[m] = -1;
            if (t < n) {
                const CvEntry en = c.ents[base + t];
                row[m] = en.row;
                e[m] = en.idx;
                kf[m] = rows[en.row].id;
                off[m] = rows[en.row].off;
                s_kf[t] = kf[m];
                s_e[t] = en.idx;
                if (!rows[en.row].has_desc)
                    flags |= 1;
                const CvCentre ce = centres[en.row];
                if (!ce.has)
                    flags |= 2;
                // R5: d = P - Ow in float, the norm in FP64, its inverse rounded to float, the term rounded again
                const float dx = px - ce.x, dy = py - ce.y, dz = pz - ce.z;
                const double nrm = sqrt((double)dx * (double)dx + (double)dy * (double)dy + (double)dz * (double)dz);
                const float inv = (float)(1.0 / nrm);
                tx[m] = dx * inv;
                ty[m] = dy * inv;
                tz[m] = dz * inv;
                dist[m] = (float)nrm;
            }
        }
        __syncthreads();  // the keys; s_best, s_flags, s_ref_e
        if (flags)
            atomicOr(&s_flags, flags);
#pragma unroll
        for (int m = 0; m < PER; m++) {
            if (row[m] < 0)
                continue;
            int r = 0;  // R1: the entries before this one in (key-frame id, slot index); the keys are distinct
            for (int j = 0; j < n; j++)
                r += s_kf[j] < kf[m] || (s_kf[j] == kf[m] && s_e[j] < e[m]) ? 1 : 0;
            rank[m] = r;
            if (row[m] == ref)
                atomicMin(&s_ref_e, e[m]);  // R6: the lowest slot of the reference row
        }
        __syncthreads();
        const int fl = s_flags, ref_e = s_ref_e;
        if ((c.what & ORBGPU_REFRESH_DESCRIPTOR) && !(fl & 1)) {  // R4
#pragma unroll
            for (int m = 0; m < PER; m++)
                if (row[m] >= 0) {
                    const uint4 *src = reinterpret_cast<const uint4 *>(descs + 32 * (size_t)(off[m] + e[m]));
                    uint4 *dst = reinterpret_cast<uint4 *>(s_d + 4 * rank[m]);
                    dst[0] = src[0];
                    dst[1] = src[1];
                }
            __syncthreads();
            unsigned long long mine = ~0ull;
#pragma unroll
            for (int m = 0; m < PER; m++)
                if (row[m] >= 0) {
                    const uint64_t *own = s_d + 4 * rank[m];
                    const uint64_t a[4] = {own[0], own[1], own[2], own[3]};
                    const uint16_t *stored = nullptr;
                    if (ROWS) {
                        uint16_t *dr = s_dist + tid * DSTRIDE;
                        for (int j = 0; j < n; j++) {
                            const uint64_t b[4] = {s_d[j * 4], s_d[j * 4 + 1], s_d[j * 4 + 2], s_d[j * 4 + 3]};
                            dr[j] = (uint16_t)hamming256(a, b);
                        }
                        stored = dr;
                    }
                    const unsigned long long key =
                        ((unsigned long long)refresh_median(a, s_d, n, stored) << 32) | (unsigned)rank[m];  // least median, then R1's order
                    mine = key < mine ? key : mine;
                }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long other = __shfl_xor(mine, o, 64);
                mine = other < mine ? other : mine;
            }
            if ((tid & 63) == 0)
                atomicMin(&s_best, mine);
            __syncthreads();
            const int best = (int)(s_best & 0xFFFFFFFFull);
#pragma unroll
            for (int m = 0; m < PER; m++)
                if (row[m] >= 0 && rank[m] == best) {
                    const uint4 *own = reinterpret_cast<const uint4 *>(s_d + 4 * best);
                    uint4 *out = reinterpret_cast<uint4 *>(c.desc + 32 * (size_t)ci);
                    out[0] = own[0];
                    out[1] = own[1];
                    if (c.t_row) {
                        uint4 *tout = reinterpret_cast<uint4 *>(c.t_desc + 32 * (size_t)c.t_row[ci]);
                        tout[0] = own[0];
                        tout[1] = own[1];
                    }
                    c.desc_kf[ci] = kf[m];
                    c.desc_idx[ci] = e[m];
                }
        }
        if (c.what & ORBGPU_REFRESH_NORMAL_DEPTH) {
#pragma unroll
            for (int m = 0; m < PER; m++)
                if (row[m] >= 0) {
                    s_t[3 * rank[m]] = tx[m];
                    s_t[3 * rank[m] + 1] = ty[m];
                    s_t[3 * rank[m] + 2] = tz[m];
                    if (row[m] == ref && e[m] == ref_e) {
                        s_ref_dist = dist[m];
                        s_ref_level = kp[off[m] + e[m]] & (CV_LEVELS - 1);
                    }
                }
        }
        __syncthreads();
        if (tid == 0) {
            int st = 0;
            if ((c.what & ORBGPU_REFRESH_DESCRIPTOR) && (fl & 1))
                st |= ORBGPU_REFRESH_NO_DESC;
            if (c.what & ORBGPU_REFRESH_NORMAL_DEPTH) {
                const bool ref_ok = ref_e != INT_MAX && s_ref_level < sc.n_levels;  // (n_levels = 0: no table)
                if (fl & 2)
                    st |= ORBGPU_REFRESH_NO_CENTRE;
                if (!ref_ok)
                    st |= ORBGPU_REFRESH_NO_REF;
                if (!(fl & 2) && ref_ok) {
                    float ax = 0.f, ay = 0.f, az = 0.f;  // R5: in R1's order
                    for (int j = 0; j < n; j++) {
                        ax = ax + s_t[3 * j];
                        ay = ay + s_t[3 * j + 1];
                        az = az + s_t[3 * j + 2];
                    }
                    const float inv_n = (float)(1.0 / (double)n);
                    const float nx = ax * inv_n, ny = ay * inv_n, nz = az * inv_n;
                    const float mx = s_ref_dist * sc.sf[s_ref_level];  // R6
                    const float mn = mx / sc.sf[sc.n_levels - 1];
                    c.normal[3 * (size_t)ci] = nx;
                    c.normal[3 * (size_t)ci + 1] = ny;
                    c.normal[3 * (size_t)ci + 2] = nz;
                    c.min_dist[ci] = mn;
                    c.max_dist[ci] = mx;
                    if (c.t_row) {
                        const size_t tr = (size_t)c.t_row[ci];
                        c.t_normal[3 * tr] = nx;
                        c.t_normal[3 * tr + 1] = ny;
                        c.t_normal[3 * tr + 2] = nz;
                        c.t_min[tr] = mn;
                        c.t_max[tr] = mx;
                    }
                }
            }
            c.status[ci] = (uint8_t)st;
        }
        __syncthreads();  // the next point takes the arrays over
    }
}

constexpr int CV_ROW_COLS = 5;  // the per-row arrays of orbgpu_covis_graph

} // namespace orbgpu

using namespace orbgpu;

struct orbgpu_covis_graph {
    int device_id = 0, initial_rows = 0;
    int64_t initial_slots = 0;
    bool bound = false;  // device selected, stream created, first buffers allocated
    hipStream_t stream = nullptr;
    int rows = 0, row_cap = 0, n_bad = 0;
    int64_t pool_used = 0, pool_cap = 0;
    // per row, all carried over by a growth: the row, its vote, its query stamp (mnTrackReferenceForFrame), and the rows in
    // ascending id (position p holds the row of the p-th smallest id)
    DevBuf d_rows, d_count, d_stamp, d_order, d_centre;  // d_centre: the camera centres (R5), zero until set_centres
    const IdColumn<DevBuf> row_cols[CV_ROW_COLS] = {
        {&d_rows, sizeof(CvRow)}, {&d_count, 4}, {&d_stamp, 4}, {&d_order, 4}, {&d_centre, sizeof(CvCentre)}};
    orbgpu_covis_graph() = default;
    orbgpu_covis_graph(const orbgpu_covis_graph &) = delete;
    DevBuf d_pool, d_kp, d_hkeys, d_hvals, d_stage, d_hdr, d_pkeys, d_ppos, d_used, d_chunks, d_points;
    IdHash hash;  // id -> row (bad rows included); the device holds a byte-identical copy
    std::vector<CvRow> h_rows;
    std::vector<int64_t> h_pool;   // the slots, as the device holds them
    std::vector<uint8_t> h_kp;     // the key-point attribute of every slot (V1), as the device holds it
    std::vector<int32_t> h_order;  // rows in ascending id
    std::unordered_map<int64_t, std::vector<int64_t>> covis;  // lists set for ids that are not rows yet
    std::unordered_map<int64_t, int64_t> parents;             // parents set for ids that are not rows yet
    std::vector<char> stage;
    int stamp = 0;
    int lds_ids = CV_LDS_IDS;    // ORBGPU_DEBUG_COVIS_LDS_IDS, read at creation
    int point_log2 = 0;          // the point hash as allocated
    bool point_dirty = true;     // it may hold entries: emptied as a whole before its next use
    int64_t global_queries = 0;  // vote and culling-count launches that read the query from global memory (tests)
    // the refresh (R1-R8)
    DevBuf d_desc;                   // the third pool column, 32 bytes per slot; empty until the first set_descriptors
    bool has_desc_col = false;       // d_desc is as long as the pool and grows with it
    DevBuf d_ents;                   // a call's observation lists
    std::vector<CvCentre> h_centre;  // the centre column, as the device holds it
    bool centres_set = false;        // the column may hold something other than zeros
    CvScale scale = {};
    bool refresh_rows = false;       // ORBGPU_DEBUG_REFRESH_SELECT=rows, read at creation
};

namespace orbgpu {

static int cv_grow_rows(orbgpu_covis_graph *g, int want)
{
    if (want <= g->row_cap)
        return ORBGPU_OK;
    int ncap = std::max(g->row_cap, 1);
    while (ncap < want)
        ncap *= 2;
    TableStreamOps ops{g->stream, "growing the covisibility graph"};
    const IdTableParts<DevBuf> parts{g->row_cols, CV_ROW_COLS, CV_ROW_COLS, &g->d_hkeys, &g->d_hvals, &g->hash, &g->row_cap};
    return id_table_grow(parts, g->rows, ncap, ops);
}

static int cv_grow_pool(orbgpu_covis_graph *g, int64_t want)
{
    if (want <= g->pool_cap)
        return ORBGPU_OK;
    int64_t ncap = std::max<int64_t>(g->pool_cap, 1024);
    while (ncap < want)
        ncap *= 2;
    DevBuf np, nk, nd;  // every column or none: nothing is swapped before all copies have arrived (the descriptor column
                        // takes part once it exists)
    int rc = np.reserve(8 * (size_t)ncap);
    if (rc == ORBGPU_OK)
        rc = nk.reserve((size_t)ncap);
    if (rc == ORBGPU_OK && g->has_desc_col)
        rc = nd.reserve(32 * (size_t)ncap);
    if (rc == ORBGPU_OK && g->pool_used > 0) {
        hipError_t he = hipMemcpyAsync(np.p, g->d_pool.p, 8 * (size_t)g->pool_used, hipMemcpyDeviceToDevice, g->stream);
        if (he == hipSuccess)
            he = hipMemcpyAsync(nk.p, g->d_kp.p, (size_t)g->pool_used, hipMemcpyDeviceToDevice, g->stream);
        if (he == hipSuccess && g->has_desc_col)
            he = hipMemcpyAsync(nd.p, g->d_desc.p, 32 * (size_t)g->pool_used, hipMemcpyDeviceToDevice, g->stream);
        if (he == hipSuccess)
            he = hipStreamSynchronize(g->stream);
        if (he != hipSuccess) {
            set_error("growing the slot pool: %s", hipGetErrorString(he));
            rc = ORBGPU_EHIP;
        }
    }
    if (rc != ORBGPU_OK) {
        (void)hipStreamSynchronize(g->stream);
        np.release();
        nk.release();
        nd.release();
        return rc;
    }
    std::swap(g->d_pool, np);
    std::swap(g->d_kp, nk);
    if (g->has_desc_col)
        std::swap(g->d_desc, nd);
    np.release();
    nk.release();
    nd.release();
    g->pool_cap = ncap;
    return ORBGPU_OK;
}

// Growth after the first call: under the lifecycle lock, on the growing branch only (id_table.h).
static int cv_grow_locked(orbgpu_covis_graph *g, int rows, int64_t pool)
{
    return lifecycle_locked_unless(rows <= g->row_cap && pool <= g->pool_cap, lifecycle_mutex(), [&] {
        const int rc = cv_grow_rows(g, rows);
        return rc != ORBGPU_OK ? rc : cv_grow_pool(g, pool);
    });
}
static int cv_reserve_locked(DevBuf &b, size_t bytes)
{
    return lifecycle_locked_unless(bytes <= b.bytes, lifecycle_mutex(), [&] { return b.reserve(bytes); });
}

// what the first call allocates for (the creation arguments, or their defaults); orbgpu_covis_graph_compact returns to it (C5)
static int cv_initial_rows(const orbgpu_covis_graph *g) { return g->initial_rows > 0 ? g->initial_rows : 1024; }
static int64_t cv_initial_slots(const orbgpu_covis_graph *g)
{
    return g->initial_slots > 0 ? g->initial_slots : std::min<int64_t>((int64_t)cv_initial_rows(g) * 1024, 1 << 22);
}

// first call that needs the device: select it, create the stream, allocate for initial_rows / initial_slots
static int cv_bind(orbgpu_covis_graph *g)
{
    int rc = select_device(g->device_id);
    if (rc != ORBGPU_OK || g->bound)
        return rc;
    std::lock_guard<std::mutex> lifecycle(lifecycle_mutex());
    if (!g->stream) {
        hipError_t he = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
        if (he != hipSuccess) {
            g->stream = nullptr;
            set_error("hipStreamCreate: %s", hipGetErrorString(he));
            return ORBGPU_EHIP;
        }
    }
    const int rows0 = cv_initial_rows(g);
    const int64_t slots0 = cv_initial_slots(g);
    if ((rc = cv_grow_rows(g, rows0)) != ORBGPU_OK || (rc = cv_grow_pool(g, slots0)) != ORBGPU_OK)
        return rc;
    if ((rc = g->d_hdr.reserve(8 * CH_WORDS)) != ORBGPU_OK)
        return rc;
    g->bound = true;
    return ORBGPU_OK;
}

static int cv_sync_or_fail(orbgpu_covis_graph *g, hipError_t he, const char *what)
{
    const hipError_t se = hipStreamSynchronize(g->stream);  // also after a failed enqueue: copies read the caller's arrays
    if (he == hipSuccess)
        he = se;
    if (he != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(he));
        return ORBGPU_EHIP;
    }
    return ORBGPU_OK;
}

// the distinct ids >= 0 of a query in ascending order, with their multiplicities
static void cv_query(int n, const int64_t *ids, std::vector<int64_t> &q, std::vector<int32_t> &mult)
{
    std::vector<int64_t> s;
    for (int i = 0; i < n; i++)
        if (ids[i] >= 0)
            s.push_back(ids[i]);
    std::sort(s.begin(), s.end());
    q.clear();
    mult.clear();
    for (size_t i = 0; i < s.size(); i++) {
        if (i == 0 || s[i] != s[i - 1]) {
            q.push_back(s[i]);
            mult.push_back(0);
        }
        mult.back()++;
    }
}

static void cv_launch_vote(orbgpu_covis_graph *g, int nq, const int64_t *q_ids, const int32_t *q_mult, int exclude_row)
{
    const int grid = std::min((g->rows + CV_WAVES - 1) / CV_WAVES, 4096);
    const CvRow *rows = g->d_rows.as<CvRow>();
    if (nq <= g->lds_ids)
        hipLaunchKernelGGL(k_covis_vote<true>, dim3(grid), dim3(CV_BLOCK), 12 * (size_t)std::max(nq, 1), g->stream, g->rows, rows,
                           g->d_pool.as<int64_t>(), g->pool_used, nq, q_ids, q_mult, exclude_row, g->d_count.as<int32_t>());
    else {
        g->global_queries++;
        hipLaunchKernelGGL(k_covis_vote<false>, dim3(grid), dim3(CV_BLOCK), 0, g->stream, g->rows, rows, g->d_pool.as<int64_t>(),
                           g->pool_used, nq, q_ids, q_mult, exclude_row, g->d_count.as<int32_t>());
    }
}

// obs and cnt (levels per query point) are zero; the query goes through LDS or global memory as the vote's does
static void cv_launch_cull_count(orbgpu_covis_graph *g, int nq, const int64_t *q_ids, int levels, int32_t *obs, int32_t *cnt)
{
    const int grid = std::min((g->rows + CV_WAVES - 1) / CV_WAVES, 4096);
    const CvRow *rows = g->d_rows.as<CvRow>();
    if (nq <= g->lds_ids)
        hipLaunchKernelGGL(k_covis_cull_count<true>, dim3(grid), dim3(CV_BLOCK), 8 * (size_t)std::max(nq, 1), g->stream, g->rows, rows,
                           g->d_pool.as<int64_t>(), g->d_kp.as<uint8_t>(), g->pool_used, nq, q_ids, levels, obs, cnt);
    else {
        g->global_queries++;
        hipLaunchKernelGGL(k_covis_cull_count<false>, dim3(grid), dim3(CV_BLOCK), 0, g->stream, g->rows, rows, g->d_pool.as<int64_t>(),
                           g->d_kp.as<uint8_t>(), g->pool_used, nq, q_ids, levels, obs, cnt);
    }
}

// A query: stage the inputs, vote, build the list and -- local map only -- gather the points; first wait: the header.
struct CvStaged {
    size_t o_q = 0, o_mult = 0, o_prev = 0, in_bytes = 0, o_rows = 0, o_ids = 0, o_counts = 0, o_prefix = 0;
    int list_cap = 0, point_cap = 0;
    long long hdr[CH_WORDS] = {};
};

static int cv_run(orbgpu_covis_graph *g, int mode, const std::vector<int64_t> &q, const std::vector<int32_t> &mult, int exclude_row,
                  const std::vector<int32_t> &prev_rows, int64_t prev_slots, CvStaged &s)
{
    const int nq = (int)q.size(), np = (int)prev_rows.size();
    s.list_cap = std::max(g->rows, np) + 1;
    Carver c;
    s.o_q = c.take(8 * (size_t)std::max(nq, 1));
    s.o_mult = c.take(4 * (size_t)std::max(nq, 1));
    s.o_prev = c.take(4 * (size_t)std::max(np, 1));
    s.in_bytes = c.off;
    s.o_rows = c.take(4 * (size_t)s.list_cap);
    s.o_ids = c.take(8 * (size_t)s.list_cap);
    s.o_counts = c.take(4 * (size_t)s.list_cap);
    s.o_prefix = c.take(4 * ((size_t)s.list_cap + 1));
    int rc = cv_reserve_locked(g->d_stage, c.off);
    if (rc != ORBGPU_OK)
        return rc;
    // the gather: at most `bound` slots (every row once, or the previous list), at most CV_MAX_POINTS distinct ids
    const int64_t bound = std::max<int64_t>(std::max(g->pool_used, prev_slots), 1);
    const int n_chunks = (int)((bound + CV_CHUNK - 1) / CV_CHUNK) + 1;
    CvPointHash h{};
    if (mode == 0) {
        s.point_cap = (int)std::min<int64_t>(bound, CV_MAX_POINTS);
        const int l2 = id_hash_log2cap(std::max(s.point_cap, 512));
        if (l2 > g->point_log2) {
            if ((rc = cv_reserve_locked(g->d_pkeys, sizeof(int64_t) << l2)) != ORBGPU_OK)
                return rc;
            g->point_dirty = true;  // (one of the two may be new)
            if ((rc = cv_reserve_locked(g->d_ppos, sizeof(int32_t) << l2)) != ORBGPU_OK)
                return rc;
            g->point_log2 = l2;
        }
        if ((rc = cv_reserve_locked(g->d_used, 4 * (size_t)s.point_cap)) != ORBGPU_OK ||
            (rc = cv_reserve_locked(g->d_points, 8 * (size_t)s.point_cap)) != ORBGPU_OK ||
            (rc = cv_reserve_locked(g->d_chunks, 4 * (size_t)n_chunks)) != ORBGPU_OK)
            return rc;
        h = CvPointHash{g->point_log2, s.point_cap, g->d_pkeys.as<int64_t>(), g->d_ppos.as<int32_t>(), g->d_used.as<int32_t>()};
    }
    g->stage.resize(s.in_bytes);
    if (nq) {
        memcpy(g->stage.data() + s.o_q, q.data(), 8 * (size_t)nq);
        memcpy(g->stage.data() + s.o_mult, mult.data(), 4 * (size_t)nq);
    }
    if (np)
        memcpy(g->stage.data() + s.o_prev, prev_rows.data(), 4 * (size_t)np);
    hipError_t he = hipSuccess;
    if (mode == 0) {
        if (g->stamp == INT_MAX) {  // the stamps of 2^31 queries are used up: start again
            he = hipMemsetAsync(g->d_stamp.p, 0, 4 * (size_t)g->row_cap, g->stream);
            g->stamp = 0;
        }
        g->stamp++;
        if (he == hipSuccess && g->point_dirty) {
            he = hipMemsetAsync(g->d_pkeys.p, 0xFF, sizeof(int64_t) << g->point_log2, g->stream);  // ID_HASH_EMPTY
            if (he == hipSuccess)
                he = hipMemsetAsync(g->d_ppos.p, 0x7F, sizeof(int32_t) << g->point_log2, g->stream);  // CV_POS_NONE
        }
        g->point_dirty = true;  // until this call has emptied what it filled
    }
    char *st = g->d_stage.as<char>();
    long long *hdr = g->d_hdr.as<long long>();
    if (he == hipSuccess)
        he = hipMemcpyAsync(st, g->stage.data(), s.in_bytes, hipMemcpyHostToDevice, g->stream);
    if (he == hipSuccess)
        he = hipMemsetAsync(hdr, 0, 8 * CH_WORDS, g->stream);
    if (he == hipSuccess) {
        const CvRow *rows = g->d_rows.as<CvRow>();
        const int64_t *pool = g->d_pool.as<int64_t>();
        const CvList l{s.list_cap, reinterpret_cast<int32_t *>(st + s.o_rows), reinterpret_cast<int64_t *>(st + s.o_ids),
                       reinterpret_cast<int32_t *>(st + s.o_counts), reinterpret_cast<int32_t *>(st + s.o_prefix)};
        cv_launch_vote(g, nq, reinterpret_cast<const int64_t *>(st + s.o_q), reinterpret_cast<const int32_t *>(st + s.o_mult),
                       exclude_row);
        hipLaunchKernelGGL(k_covis_list, dim3(1), dim3(CV_LIST_BLOCK), 0, g->stream, mode, g->rows, rows, g->d_order.as<int32_t>(),
                           g->d_count.as<int32_t>(), g->d_stamp.as<int32_t>(), g->stamp, g->d_hkeys.as<int64_t>(),
                           g->d_hvals.as<int32_t>(), g->hash.log2cap, np, reinterpret_cast<const int32_t *>(st + s.o_prev), l, hdr);
        if (mode == 0) {
            const int grid = (int)std::min<int64_t>((bound + CV_CHUNK - 1) / CV_CHUNK, 2048);
            hipLaunchKernelGGL(k_covis_insert, dim3(grid), dim3(CV_BLOCK), 0, g->stream, l, g->rows, rows, pool, g->pool_used, h, hdr);
            hipLaunchKernelGGL(k_covis_count, dim3(grid), dim3(CV_BLOCK), 0, g->stream, l, g->rows, rows, pool, g->pool_used, h, hdr,
                               n_chunks, g->d_chunks.as<int32_t>());
            hipLaunchKernelGGL(k_covis_scan, dim3(1), dim3(CV_LIST_BLOCK), 0, g->stream, n_chunks, g->d_chunks.as<int32_t>(), hdr);
            hipLaunchKernelGGL(k_covis_emit, dim3(grid), dim3(CV_BLOCK), 0, g->stream, l, g->rows, rows, pool, g->pool_used, h, hdr,
                               n_chunks, g->d_chunks.as<int32_t>(), s.point_cap, g->d_points.as<int64_t>());
            hipLaunchKernelGGL(k_covis_unhash, dim3(std::min((s.point_cap + 255) / 256, 1024)), dim3(256), 0, g->stream, h, hdr);
        }
        he = hipGetLastError();
        if (he == hipSuccess)
            he = hipMemcpyAsync(s.hdr, hdr, 8 * CH_WORDS, hipMemcpyDeviceToHost, g->stream);
    }
    if ((rc = cv_sync_or_fail(g, he, mode == 0 ? "local map query" : "connections query")) != ORBGPU_OK)
        return rc;
    if (s.hdr[CH_RANGE] || s.hdr[CH_LIST] < 0 || s.hdr[CH_LIST] > s.list_cap) {
        set_error("covisibility graph: an index left its range on the device");
        return ORBGPU_EHIP;
    }
    if (mode == 0 && !s.hdr[CH_OVERFLOW])
        g->point_dirty = false;
    return ORBGPU_OK;
}

static int cv_destroy(orbgpu_covis_graph *g)
{
    if (!g)
        return ORBGPU_OK;
    if (g->bound || g->stream) {
        (void)hipSetDevice(g->device_id);
        if (g->stream) {
            (void)hipStreamSynchronize(g->stream);
            (void)hipStreamDestroy(g->stream);
        }
        for (const IdColumn<DevBuf> &c : g->row_cols)
            c.buf->release();
        for (DevBuf *b : {&g->d_pool, &g->d_kp, &g->d_hkeys, &g->d_hvals, &g->d_stage, &g->d_hdr, &g->d_pkeys, &g->d_ppos, &g->d_used,
                          &g->d_chunks, &g->d_points, &g->d_desc, &g->d_ents})
            b->release();
    }
    delete g;
    return ORBGPU_OK;
}

} // namespace orbgpu

extern "C" {

int orbgpu_covis_graph_create(int32_t device_id, int32_t initial_rows, int64_t initial_slots, orbgpu_covis_graph **out)
{
    ORBGPU_REQUIRE(out, "null argument");
    ORBGPU_REQUIRE(device_id >= 0, "device_id = %d", device_id);
    ORBGPU_REQUIRE(initial_rows >= 0 && initial_rows <= CV_MAX_ROWS, "initial_rows = %d (at most %d)", initial_rows, CV_MAX_ROWS);
    ORBGPU_REQUIRE(initial_slots >= 0 && initial_slots <= CV_MAX_POOL, "initial_slots = %lld (at most %lld)",
                   (long long)initial_slots, (long long)CV_MAX_POOL);
    orbgpu_covis_graph *g = new (std::nothrow) orbgpu_covis_graph();
    if (!g) {
        set_error("out of host memory");
        return ORBGPU_ENOMEM;
    }
    g->device_id = device_id;
    g->initial_rows = initial_rows;
    g->initial_slots = initial_slots;
    // ORBGPU_DEBUG_COVIS_LDS_IDS=<k> (tests): a query of more than k distinct ids takes the global-memory path
    if (const char *e = getenv("ORBGPU_DEBUG_COVIS_LDS_IDS"))
        g->lds_ids = std::min(std::max(atoi(e), 0), CV_LDS_IDS);
    // ORBGPU_DEBUG_REFRESH_SELECT=rows (measurements): the one-wave refresh keeps its distance rows in LDS
    if (const char *e = getenv("ORBGPU_DEBUG_REFRESH_SELECT"))
        g->refresh_rows = !strcmp(e, "rows");
    *out = g;
    return ORBGPU_OK;
}

int orbgpu_covis_graph_destroy(orbgpu_covis_graph *g)
{
    std::lock_guard<std::mutex> lifecycle(orbgpu::lifecycle_mutex());
    return cv_destroy(g);
}

int orbgpu_covis_graph_clear(orbgpu_covis_graph *g)
{
    ORBGPU_REQUIRE(g, "null argument");
    if (g->bound) {
        int rc = select_device(g->device_id);
        if (rc != ORBGPU_OK)
            return rc;
        hipError_t he = hipMemsetAsync(g->d_hkeys.p, 0xFF, sizeof(int64_t) << g->hash.log2cap, g->stream);  // ID_HASH_EMPTY
        if (he == hipSuccess && g->centres_set)  // a row added later starts without a centre
            he = hipMemsetAsync(g->d_centre.p, 0, sizeof(CvCentre) * (size_t)g->row_cap, g->stream);
        if ((rc = cv_sync_or_fail(g, he, "clearing the covisibility graph")) != ORBGPU_OK)
            return rc;
    }
    g->hash.clear();
    g->h_rows.clear();
    g->h_pool.clear();
    g->h_kp.clear();
    g->h_order.clear();
    g->h_centre.clear();  // (descriptors go with the rows' flags)
    g->centres_set = false;
    g->scale = CvScale{};
    g->covis.clear();
    g->parents.clear();
    g->rows = g->n_bad = 0;
    g->pool_used = 0;
    return ORBGPU_OK;
}

int orbgpu_covis_graph_size(const orbgpu_covis_graph *g, int32_t *alive, int32_t *bad)
{
    ORBGPU_REQUIRE(g && alive && bad, "null argument");
    *alive = g->rows - g->n_bad;
    *bad = g->n_bad;
    return ORBGPU_OK;
}

int orbgpu_covis_graph_add_keyframe(orbgpu_covis_graph *g, int64_t id, int32_t n_slots, const int64_t *mp_ids)
{
    ORBGPU_REQUIRE(g, "null argument");
    ORBGPU_REQUIRE(id >= 0, "key frame id %lld", (long long)id);
    ORBGPU_REQUIRE(n_slots >= 0 && n_slots <= CV_MAX_SLOTS, "n_slots = %d (at most %d)", n_slots, CV_MAX_SLOTS);
    for (int i = 0; mp_ids && i < n_slots; i++)
        ORBGPU_REQUIRE(mp_ids[i] >= -1, "map point id %lld at slot %d", (long long)mp_ids[i], i);
    ORBGPU_REQUIRE(g->hash.find(id) < 0, "key frame %lld is in the graph", (long long)id);
    ORBGPU_REQUIRE(g->rows < CV_MAX_ROWS, "more than %d rows", CV_MAX_ROWS);
    ORBGPU_REQUIRE(g->pool_used + n_slots <= CV_MAX_POOL, "more than %lld pool slots", (long long)CV_MAX_POOL);
    int rc = cv_bind(g);
    if (rc != ORBGPU_OK || (rc = cv_grow_locked(g, g->rows + 1, g->pool_used + n_slots)) != ORBGPU_OK)
        return rc;
    CvRow row{};
    row.id = id;
    row.parent = -1;
    row.off = g->pool_used;
    row.n_slots = n_slots;
    for (int k = 0; k < CV_MAX_NB; k++)
        row.nb[k] = -1;
    const auto ic = g->covis.find(id);
    if (ic != g->covis.end()) {
        row.nn = (int32_t)ic->second.size();
        std::copy(ic->second.begin(), ic->second.end(), row.nb);
    }
    const auto ip = g->parents.find(id);
    if (ip != g->parents.end())
        row.parent = ip->second;
    const int r = g->rows;
    const uint32_t slot = g->hash.slot_for(id);
    // the rows in ascending id: the new one usually goes last
    const size_t at = (size_t)(std::lower_bound(g->h_order.begin(), g->h_order.end(), id,
                                                [g](int32_t a, int64_t v) { return g->h_rows[(size_t)a].id < v; }) -
                               g->h_order.begin());
    std::vector<int32_t> tail;
    tail.push_back(r);
    tail.insert(tail.end(), g->h_order.begin() + (ptrdiff_t)at, g->h_order.end());
    std::vector<int64_t> slots((size_t)n_slots, -1);
    if (mp_ids && n_slots)
        memcpy(slots.data(), mp_ids, 8 * (size_t)n_slots);
    hipError_t he = hipSuccess;
    if (n_slots > 0)
        he = hipMemcpyAsync(g->d_pool.as<int64_t>() + g->pool_used, slots.data(), 8 * (size_t)n_slots, hipMemcpyHostToDevice, g->stream);
    if (he == hipSuccess && n_slots > 0)
        he = hipMemsetAsync(g->d_kp.as<uint8_t>() + g->pool_used, 0, (size_t)n_slots, g->stream);  // octave 0, monocular, close
    if (he == hipSuccess)
        he = hipMemcpyAsync(g->d_order.as<int32_t>() + at, tail.data(), 4 * tail.size(), hipMemcpyHostToDevice, g->stream);
    if (he == hipSuccess)
        he = hipMemcpyAsync(g->d_rows.as<CvRow>() + r, &row, sizeof(row), hipMemcpyHostToDevice, g->stream);
    if (he == hipSuccess)
        he = hipMemcpyAsync(g->d_hvals.as<int32_t>() + slot, &r, 4, hipMemcpyHostToDevice, g->stream);
    if (he == hipSuccess)
        he = hipMemcpyAsync(g->d_hkeys.as<int64_t>() + slot, &id, 8, hipMemcpyHostToDevice, g->stream);
    if ((rc = cv_sync_or_fail(g, he, "adding a key frame")) != ORBGPU_OK) {
        if (at < g->h_order.size())  // the order column as it was (best effort: the failure is reported either way)
            (void)hipMemcpy(g->d_order.as<int32_t>() + at, g->h_order.data() + at, 4 * (g->h_order.size() - at), hipMemcpyHostToDevice);
        return rc;
    }
    g->hash.keys[slot] = id;
    g->hash.vals[slot] = r;
    g->h_rows.push_back(row);
    g->h_order.insert(g->h_order.begin() + (ptrdiff_t)at, r);
    g->h_pool.insert(g->h_pool.end(), slots.begin(), slots.end());
    g->h_kp.insert(g->h_kp.end(), (size_t)n_slots, (uint8_t)0);
    g->h_centre.push_back(CvCentre{});
    g->covis.erase(id);
    g->parents.erase(id);
    g->pool_used += n_slots;
    g->rows++;
    return ORBGPU_OK;
}

int orbgpu_covis_graph_set_slots(orbgpu_covis_graph *g, int32_t n, const int64_t *kf_ids, const int32_t *idx, const int64_t *mp_ids,
                                 int32_t *known)
{
    ORBGPU_REQUIRE(g && n >= 0 && n <= CV_MAX_CALL && (n == 0 || (kf_ids && idx && mp_ids)), "bad argument");
    std::vector<int64_t> addr;
    int n_known = 0;
    for (int i = 0; i < n; i++) {
        ORBGPU_REQUIRE(mp_ids[i] >= -1, "map point id %lld (entry %d)", (long long)mp_ids[i], i);
        const int r = g->hash.find(kf_ids[i]);
        if (r < 0) {
            addr.push_back(-1);
            continue;  // an unknown key frame: ignored
        }
        const CvRow &row = g->h_rows[(size_t)r];
        ORBGPU_REQUIRE(idx[i] >= 0 && idx[i] < row.n_slots, "slot %d outside key frame %lld (%d slots, entry %d)", idx[i],
                       (long long)row.id, row.n_slots, i);
        n_known++;
        addr.push_back(row.bad ? -1 : row.off + idx[i]);  // V2: a bad key frame holds no slot
    }
    if (known)
        *known = n_known;
    // applied in order to the mirror (later entries win); the device gets the final value of every slot touched
    std::vector<std::pair<int64_t, int64_t>> undo;
    for (int i = 0; i < n; i++)
        if (addr[(size_t)i] >= 0) {
            undo.emplace_back(addr[(size_t)i], g->h_pool[(size_t)addr[(size_t)i]]);
            g->h_pool[(size_t)addr[(size_t)i]] = mp_ids[i];
        }
    if (undo.empty())
        return ORBGPU_OK;
    std::vector<int64_t> a;
    for (const auto &u : undo)
        a.push_back(u.first);
    std::sort(a.begin(), a.end());
    a.erase(std::unique(a.begin(), a.end()), a.end());
    const int m = (int)a.size();
    auto fail = [&](int rc) {
        for (size_t k = undo.size(); k-- > 0;)
            g->h_pool[(size_t)undo[k].first] = undo[k].second;
        return rc;
    };
    int rc = cv_bind(g);
    if (rc != ORBGPU_OK)
        return fail(rc);
    Carver c;
    const size_t o_a = c.take(8 * (size_t)m), o_v = c.take(8 * (size_t)m);
    if ((rc = cv_reserve_locked(g->d_stage, c.off)) != ORBGPU_OK)
        return fail(rc);
    g->stage.resize(c.off);
    memcpy(g->stage.data() + o_a, a.data(), 8 * (size_t)m);
    int64_t *v = reinterpret_cast<int64_t *>(g->stage.data() + o_v);
    for (int k = 0; k < m; k++)
        v[k] = g->h_pool[(size_t)a[(size_t)k]];
    char *st = g->d_stage.as<char>();
    hipError_t he = hipMemcpyAsync(st, g->stage.data(), c.off, hipMemcpyHostToDevice, g->stream);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(k_covis_scatter, dim3((m + 255) / 256), dim3(256), 0, g->stream, m, reinterpret_cast<const int64_t *>(st + o_a),
                           reinterpret_cast<const int64_t *>(st + o_v), g->pool_used, g->d_pool.as<int64_t>());
        he = hipGetLastError();
    }
    if ((rc = cv_sync_or_fail(g, he, "setting slots")) != ORBGPU_OK)
        return fail(rc);
    return ORBGPU_OK;
}

int orbgpu_covis_graph_set_bad(orbgpu_covis_graph *g, int32_t n, const int64_t *kf_ids, int32_t *known)
{
    ORBGPU_REQUIRE(g && n >= 0 && n <= CV_MAX_CALL && (n == 0 || kf_ids), "bad argument");
    if (known)
        *known = 0;
    std::vector<int> todo;
    int n_known = 0;
    for (int i = 0; i < n; i++) {
        const int r = g->hash.find(kf_ids[i]);
        if (r < 0)
            continue;
        n_known++;
        if (!g->h_rows[(size_t)r].bad && std::find(todo.begin(), todo.end(), r) == todo.end())
            todo.push_back(r);
    }
    if (!todo.empty()) {
        int rc = cv_bind(g);
        if (rc != ORBGPU_OK)
            return rc;
        std::vector<CvRow> nr;
        for (int r : todo) {
            CvRow row = g->h_rows[(size_t)r];
            row.bad = 1;
            row.nn = 0;
            for (int k = 0; k < CV_MAX_NB; k++)
                row.nb[k] = -1;
            nr.push_back(row);
        }
        hipError_t he = hipSuccess;
        for (size_t k = 0; k < todo.size() && he == hipSuccess; k++) {
            he = hipMemcpyAsync(g->d_rows.as<CvRow>() + todo[k], &nr[k], sizeof(CvRow), hipMemcpyHostToDevice, g->stream);
            if (he == hipSuccess && nr[k].n_slots > 0)
                he = hipMemsetAsync(g->d_pool.as<int64_t>() + nr[k].off, 0xFF, 8 * (size_t)nr[k].n_slots, g->stream);  // -1
        }
        if ((rc = cv_sync_or_fail(g, he, "setting key frames bad")) != ORBGPU_OK) {
            // put back what may have been written: rows and slots as the mirror has them
            for (size_t k = 0; k < todo.size(); k++) {
                const CvRow &row = g->h_rows[(size_t)todo[k]];
                (void)hipMemcpy(g->d_rows.as<CvRow>() + todo[k], &row, sizeof(CvRow), hipMemcpyHostToDevice);
                if (row.n_slots > 0)
                    (void)hipMemcpy(g->d_pool.as<int64_t>() + row.off, g->h_pool.data() + row.off, 8 * (size_t)row.n_slots,
                                    hipMemcpyHostToDevice);
            }
            return rc;
        }
        for (size_t k = 0; k < todo.size(); k++) {
            g->h_rows[(size_t)todo[k]] = nr[k];
            std::fill(g->h_pool.begin() + (ptrdiff_t)nr[k].off, g->h_pool.begin() + (ptrdiff_t)(nr[k].off + nr[k].n_slots), (int64_t)-1);
        }
        g->n_bad += (int)todo.size();
    }
    if (known)
        *known = n_known;
    return ORBGPU_OK;
}

int orbgpu_covis_graph_set_parent(orbgpu_covis_graph *g, int64_t kf_id, int64_t parent_id)
{
    ORBGPU_REQUIRE(g, "null argument");
    ORBGPU_REQUIRE(kf_id >= 0 && parent_id >= -1, "key frame %lld, parent %lld", (long long)kf_id, (long long)parent_id);
    const int r = g->hash.find(kf_id);
    if (r < 0) {
        g->parents[kf_id] = parent_id;  // kept for when the key frame is added
        return ORBGPU_OK;
    }
    int rc = cv_bind(g);
    if (rc != ORBGPU_OK)
        return rc;
    hipError_t he = hipMemcpyAsync(reinterpret_cast<char *>(g->d_rows.as<CvRow>() + r) + offsetof(CvRow, parent), &parent_id, 8,
                                   hipMemcpyHostToDevice, g->stream);
    if ((rc = cv_sync_or_fail(g, he, "setting a parent")) != ORBGPU_OK)
        return rc;
    g->h_rows[(size_t)r].parent = parent_id;
    return ORBGPU_OK;
}

int orbgpu_covis_graph_set_covisibles(orbgpu_covis_graph *g, int64_t kf_id, int32_t n, const int64_t *ids)
{
    ORBGPU_REQUIRE(g, "null argument");
    ORBGPU_REQUIRE(kf_id >= 0, "key frame id %lld", (long long)kf_id);
    ORBGPU_REQUIRE(n >= 0 && n <= CV_MAX_NB && (n == 0 || ids), "%d covisibles (at most %d)", n, CV_MAX_NB);
    for (int k = 0; k < n; k++)
        ORBGPU_REQUIRE(ids[k] >= 0, "covisible id %lld", (long long)ids[k]);
    const int r = g->hash.find(kf_id);
    if (r < 0) {
        g->covis[kf_id].assign(ids, ids + n);  // kept for when the key frame is added
        return ORBGPU_OK;
    }
    if (g->h_rows[(size_t)r].bad)
        return ORBGPU_OK;  // a bad key frame has forgotten its covisibles and learns no new ones
    int rc = cv_bind(g);
    if (rc != ORBGPU_OK)
        return rc;
    CvRow row = g->h_rows[(size_t)r];
    row.nn = n;
    for (int k = 0; k < CV_MAX_NB; k++)
        row.nb[k] = k < n ? ids[k] : -1;
    const size_t o = offsetof(CvRow, nn);
    hipError_t he = hipMemcpyAsync(reinterpret_cast<char *>(g->d_rows.as<CvRow>() + r) + o, reinterpret_cast<const char *>(&row) + o,
                                   sizeof(CvRow) - o, hipMemcpyHostToDevice, g->stream);
    if ((rc = cv_sync_or_fail(g, he, "setting covisible key frames")) != ORBGPU_OK)
        return rc;
    g->h_rows[(size_t)r] = row;
    return ORBGPU_OK;
}

int orbgpu_covis_graph_debug_global_queries(const orbgpu_covis_graph *g, int64_t *n)
{
    ORBGPU_REQUIRE(g && n, "null argument");
    *n = g->global_queries;
    return ORBGPU_OK;
}

// C1-C7 (orbgpu.h).  The plan is host work over the mirror (compact_plan.h); the copies run inside the transaction of
// id_table.h, which swaps rows, hash and pool columns only after everything has arrived.
int orbgpu_covis_graph_compact(orbgpu_covis_graph *g, orbgpu_compact_result *res)
{
    ORBGPU_REQUIRE(g, "null argument");
    const int n = g->rows;
    std::vector<int32_t> bad((size_t)n), len((size_t)n);
    std::vector<int64_t> ids((size_t)n), par((size_t)n);
    std::vector<uint8_t> owns((size_t)n);
    for (int r = 0; r < n; r++) {
        const CvRow &row = g->h_rows[(size_t)r];
        bad[(size_t)r] = row.bad;
        len[(size_t)r] = row.n_slots;
        ids[(size_t)r] = row.id;
        par[(size_t)r] = row.parent;
        owns[(size_t)r] = !row.bad;
    }
    const std::vector<uint8_t> keep = compact_keep_graph(n, bad.data(), ids.data(), par.data());
    const CompactPlan plan = compact_plan(n, len.data(), keep.data(), owns.data(), g->pool_used, CV_OFF_NONE);
    const int m = (int)plan.src.size();
    orbgpu_compact_result out{};
    out.rows_before = out.rows_after = n;
    out.rows_bad_kept = g->n_bad;
    out.row_capacity = g->row_cap;
    out.slots_before = out.slots_after = g->pool_used;
    out.slot_capacity = g->pool_cap;
    if (!plan.needed) {  // C6
        if (res)
            *res = out;
        return ORBGPU_OK;
    }
    int rc = cv_bind(g);  // (a graph with rows is bound: this selects the device)
    if (rc != ORBGPU_OK)
        return rc;
    const int ncap = (int)compact_capacity(1, cv_initial_rows(g), m);
    const int64_t pcap = compact_capacity(1024, cv_initial_slots(g), plan.pool_after);
    // the mirrors as they will be, built before anything is touched
    std::vector<CvRow> n_rows((size_t)m);
    std::vector<CvCentre> n_centre((size_t)m);
    std::vector<int64_t> n_pool((size_t)plan.pool_after), old_off((size_t)m);
    std::vector<uint8_t> n_kp((size_t)plan.pool_after);
    std::vector<int32_t> n_order, new_of((size_t)n, -1);
    int n_bad = 0;
    for (int i = 0; i < m; i++) {
        const size_t r = (size_t)plan.src[(size_t)i];
        const int64_t off = plan.off[(size_t)i];
        const int32_t l = plan.len[(size_t)i];
        n_rows[(size_t)i] = g->h_rows[r];
        n_rows[(size_t)i].off = off;
        n_centre[(size_t)i] = g->h_centre[r];
        old_off[(size_t)i] = g->h_rows[r].off;
        new_of[r] = i;
        n_bad += g->h_rows[r].bad != 0;
        if (l > 0) {
            std::copy_n(g->h_pool.begin() + (ptrdiff_t)g->h_rows[r].off, l, n_pool.begin() + (ptrdiff_t)off);
            std::copy_n(g->h_kp.begin() + (ptrdiff_t)g->h_rows[r].off, l, n_kp.begin() + (ptrdiff_t)off);
        }
    }
    n_order.reserve((size_t)m);
    for (int32_t r : g->h_order)  // ascending id stays ascending id
        if (new_of[(size_t)r] >= 0)
            n_order.push_back(new_of[(size_t)r]);
    Carver c;
    const size_t o_old = c.take(8 * (size_t)std::max(m, 1)), o_new = c.take(8 * (size_t)std::max(m, 1)),
                 o_src = c.take(4 * (size_t)std::max(m, 1)), o_len = c.take(4 * (size_t)std::max(m, 1));
    std::vector<char> stage(c.off);
    if (m > 0) {
        memcpy(stage.data() + o_old, old_off.data(), 8 * (size_t)m);
        memcpy(stage.data() + o_new, plan.off.data(), 8 * (size_t)m);
        memcpy(stage.data() + o_src, plan.src.data(), 4 * (size_t)m);
        memcpy(stage.data() + o_len, plan.len.data(), 4 * (size_t)m);
    }
    TableStreamOps ops{g->stream, "compacting the covisibility graph"};
    const IdColumn<DevBuf> pool_cols[3] = {{&g->d_pool, 8}, {&g->d_kp, 1}, {&g->d_desc, 32}};
    const int n_pool_cols = g->has_desc_col ? 3 : 2;
    // d_stage, which carries the plan, is per-call scratch outside the transaction (as in orbgpu_mappoint_table_retain)
    auto fill = [&](const DevBuf *nb, const DevBuf *np, int l2, IdHash &nh) -> int {
        if (m > 0) {
            const int rr = g->d_stage.reserve(c.off);
            if (rr != ORBGPU_OK)
                return rr;
            char *st = g->d_stage.as<char>();
            if (ops.upload(st, stage.data(), c.off) || ops.upload(nb[3].p, n_order.data(), 4 * (size_t)m))
                return ORBGPU_EHIP;
            const int32_t *src = reinterpret_cast<const int32_t *>(st + o_src);
            const int64_t *noff = reinterpret_cast<const int64_t *>(st + o_new);
            const dim3 grid((unsigned)((m + 255) / 256)), block(256);
            hipLaunchKernelGGL(k_compact_rows<CvRow>, grid, block, 0, g->stream, m, src, noff, n, g->d_rows.as<CvRow>(),
                               static_cast<CvRow *>(nb[0].p));
            hipLaunchKernelGGL(k_compact_gather<int32_t>, grid, block, 0, g->stream, m, src, n, g->d_count.as<int32_t>(),
                               static_cast<int32_t *>(nb[1].p));
            hipLaunchKernelGGL(k_compact_gather<int32_t>, grid, block, 0, g->stream, m, src, n, g->d_stamp.as<int32_t>(),
                               static_cast<int32_t *>(nb[2].p));
            hipLaunchKernelGGL(k_compact_gather<CvCentre>, grid, block, 0, g->stream, m, src, n, g->d_centre.as<CvCentre>(),
                               static_cast<CvCentre *>(nb[4].p));
            if (plan.pool_after > 0) {
                CompactPool<3> p{};
                for (int k = 0; k < n_pool_cols; k++) {
                    p.src[k] = static_cast<const uint8_t *>(pool_cols[k].buf->p);
                    p.dst[k] = static_cast<uint8_t *>(np[k].p);
                }
                hipLaunchKernelGGL((k_compact_pool<8, 1, 32>), dim3((unsigned)compact_pool_grid(m)), dim3(COMPACT_BLOCK), 0, g->stream, m,
                                   reinterpret_cast<const int64_t *>(st + o_old), noff, reinterpret_cast<const int32_t *>(st + o_len),
                                   g->pool_used, pcap, p);
            }
            if (ops.done(hipGetLastError()))
                return ORBGPU_EHIP;
        }
        nh.rebuild(l2);
        for (int i = 0; i < m; i++)
            nh.insert(n_rows[(size_t)i].id, i);
        return ORBGPU_OK;
    };
    {
        std::lock_guard<std::mutex> lifecycle(lifecycle_mutex());
        const IdTableParts<DevBuf> parts{g->row_cols, CV_ROW_COLS, CV_ROW_COLS, &g->d_hkeys, &g->d_hvals, &g->hash, &g->row_cap};
        if ((rc = id_table_compact(parts, ncap, pool_cols, n_pool_cols, (size_t)pcap, ops, fill)) != ORBGPU_OK)
            return rc;
    }
    g->h_rows.swap(n_rows);
    g->h_centre.swap(n_centre);
    g->h_pool.swap(n_pool);
    g->h_kp.swap(n_kp);
    g->h_order.swap(n_order);
    g->rows = m;
    g->n_bad = n_bad;
    g->pool_used = plan.pool_after;
    g->pool_cap = pcap;
    out.compacted = 1;
    out.rows_after = m;
    out.rows_bad_kept = n_bad;
    out.row_capacity = g->row_cap;
    out.slots_after = g->pool_used;
    out.slot_capacity = g->pool_cap;
    if (res)
        *res = out;
    return ORBGPU_OK;
}

int orbgpu_covis_local_map(orbgpu_covis_graph *g, int32_t n_kp, const int64_t *kp_ids, int32_t n_prev, const int64_t *prev_kf_ids,
                           int32_t kf_capacity, int64_t *kf_ids, int32_t point_capacity, int64_t *point_ids,
                           orbgpu_covis_local_map_result *res)
{
    ORBGPU_REQUIRE(g && res, "null argument");
    ORBGPU_REQUIRE(n_kp >= 0 && n_kp <= CV_MAX_SLOTS && (n_kp == 0 || kp_ids), "n_kp = %d (at most %d)", n_kp, CV_MAX_SLOTS);
    ORBGPU_REQUIRE(n_prev >= 0 && n_prev <= CV_MAX_CALL && (n_prev == 0 || prev_kf_ids), "n_prev = %d (at most %d)", n_prev, CV_MAX_CALL);
    ORBGPU_REQUIRE(kf_capacity >= 0 && (kf_capacity == 0 || kf_ids) && point_capacity >= 0 && (point_capacity == 0 || point_ids),
                   "bad output capacity");
    std::vector<int32_t> prev_rows;
    int64_t prev_slots = 0;
    for (int i = 0; i < n_prev; i++) {
        const int r = g->hash.find(prev_kf_ids[i]);
        if (r < 0)
            continue;
        prev_rows.push_back(r);
        prev_slots += g->h_rows[(size_t)r].n_slots;
    }
    ORBGPU_REQUIRE(prev_slots <= CV_MAX_POOL, "the previous list holds more than %lld slots", (long long)CV_MAX_POOL);
    memset(res, 0, sizeof(*res));
    res->ref_kf = -1;
    res->kept_previous = 1;
    res->n_unknown_previous = n_prev - (int32_t)prev_rows.size();
    if (g->rows == 0)
        return ORBGPU_OK;  // every previous id is unknown: an empty list, no device needed
    std::vector<int64_t> q;
    std::vector<int32_t> mult;
    cv_query(n_kp, kp_ids, q, mult);
    int rc = cv_bind(g);
    if (rc != ORBGPU_OK)
        return rc;
    CvStaged s;
    if ((rc = cv_run(g, 0, q, mult, -1, prev_rows, prev_slots, s)) != ORBGPU_OK)
        return rc;
    if (s.hdr[CH_OVERFLOW] || s.hdr[CH_POINTS] > CV_MAX_POINTS) {
        set_error("a local map of more than %d points", CV_MAX_POINTS);
        return ORBGPU_ECAPACITY;
    }
    res->n_kfs = (int32_t)s.hdr[CH_LIST];
    res->n_voted = (int32_t)s.hdr[CH_VOTED];
    res->ref_kf = s.hdr[CH_REF];
    res->max_votes = (int32_t)s.hdr[CH_MAX];
    res->kept_previous = (int32_t)s.hdr[CH_KEPT];
    res->n_points = (int32_t)std::min<long long>(s.hdr[CH_POINTS], s.point_cap);
    // second wait: the lists, as long as the caller's arrays
    const int nk = std::min(res->n_kfs, kf_capacity), npt = std::min(res->n_points, point_capacity);
    if (nk > 0 || npt > 0) {
        hipError_t he = hipSuccess;
        if (nk > 0)
            he = hipMemcpyAsync(kf_ids, g->d_stage.as<char>() + s.o_ids, 8 * (size_t)nk, hipMemcpyDeviceToHost, g->stream);
        if (he == hipSuccess && npt > 0)
            he = hipMemcpyAsync(point_ids, g->d_points.p, 8 * (size_t)npt, hipMemcpyDeviceToHost, g->stream);
        if ((rc = cv_sync_or_fail(g, he, "local map query (lists)")) != ORBGPU_OK)
            return rc;
    }
    return ORBGPU_OK;
}

int orbgpu_covis_connections(orbgpu_covis_graph *g, int64_t kf_id, int32_t th, int32_t capacity, int64_t *ids, int32_t *counts,
                             int32_t *n, int32_t ordered_capacity, int64_t *ordered_ids, int32_t *ordered_weights, int32_t *n_ordered)
{
    ORBGPU_REQUIRE(g && n && n_ordered, "null argument");
    ORBGPU_REQUIRE(capacity >= 0 && (capacity == 0 || (ids && counts)) && ordered_capacity >= 0 &&
                       (ordered_capacity == 0 || (ordered_ids && ordered_weights)),
                   "bad output capacity");
    *n = *n_ordered = 0;
    const int r = g->hash.find(kf_id);
    if (r < 0 || g->h_rows[(size_t)r].bad)
        return ORBGPU_OK;
    const CvRow &row = g->h_rows[(size_t)r];
    std::vector<int64_t> q;
    std::vector<int32_t> mult;
    cv_query(row.n_slots, g->h_pool.data() + row.off, q, mult);
    if (q.empty())
        return ORBGPU_OK;
    int rc = cv_bind(g);
    if (rc != ORBGPU_OK)
        return rc;
    CvStaged s;
    if ((rc = cv_run(g, 1, q, mult, r, std::vector<int32_t>(), 0, s)) != ORBGPU_OK)
        return rc;
    const int nc = (int)s.hdr[CH_LIST];
    if (nc == 0)
        return ORBGPU_OK;
    std::vector<int64_t> c_ids((size_t)nc);
    std::vector<int32_t> c_n((size_t)nc);
    hipError_t he = hipMemcpyAsync(c_ids.data(), g->d_stage.as<char>() + s.o_ids, 8 * (size_t)nc, hipMemcpyDeviceToHost, g->stream);
    if (he == hipSuccess)
        he = hipMemcpyAsync(c_n.data(), g->d_stage.as<char>() + s.o_counts, 4 * (size_t)nc, hipMemcpyDeviceToHost, g->stream);
    if ((rc = cv_sync_or_fail(g, he, "connections query (lists)")) != ORBGPU_OK)
        return rc;
    *n = nc;
    for (int k = 0; k < nc && k < capacity; k++) {
        ids[k] = c_ids[(size_t)k];
        counts[k] = c_n[(size_t)k];
    }
    // KeyFrame.cc:364-399: the entries at the threshold, or the single first-strictly-greatest one; descending (weight, id)
    std::vector<std::pair<int32_t, int64_t>> pairs;
    for (int k = 0; k < nc; k++)
        if (c_n[(size_t)k] >= th)
            pairs.emplace_back(c_n[(size_t)k], c_ids[(size_t)k]);
    if (pairs.empty())
        pairs.emplace_back((int32_t)s.hdr[CH_MAX], (int64_t)s.hdr[CH_REF]);
    std::sort(pairs.begin(), pairs.end());
    std::reverse(pairs.begin(), pairs.end());
    *n_ordered = (int32_t)pairs.size();
    for (int k = 0; k < (int)pairs.size() && k < ordered_capacity; k++) {
        ordered_ids[k] = pairs[(size_t)k].second;
        ordered_weights[k] = pairs[(size_t)k].first;
    }
    return ORBGPU_OK;
}

int orbgpu_covis_graph_set_keypoints(orbgpu_covis_graph *g, int64_t kf_id, int32_t n_slots, const uint8_t *kp)
{
    ORBGPU_REQUIRE(g, "null argument");
    const int r = g->hash.find(kf_id);
    ORBGPU_REQUIRE(r >= 0, "key frame %lld is not in the graph", (long long)kf_id);
    const CvRow &row = g->h_rows[(size_t)r];
    ORBGPU_REQUIRE(n_slots == row.n_slots, "n_slots = %d, key frame %lld has %d", n_slots, (long long)kf_id, row.n_slots);
    ORBGPU_REQUIRE(n_slots == 0 || kp, "null argument");
    for (int i = 0; i < n_slots; i++)
        ORBGPU_REQUIRE(!(kp[i] & 0x30), "key-point attribute 0x%02x at slot %d (bits 4-5 are reserved)", kp[i], i);
    if (row.bad || n_slots == 0)
        return ORBGPU_OK;  // a bad key frame holds no slot (V2)
    int rc = cv_bind(g);
    if (rc != ORBGPU_OK)
        return rc;
    hipError_t he = hipMemcpyAsync(g->d_kp.as<uint8_t>() + row.off, kp, (size_t)n_slots, hipMemcpyHostToDevice, g->stream);
    if ((rc = cv_sync_or_fail(g, he, "setting key-point attributes")) != ORBGPU_OK) {
        (void)hipMemcpy(g->d_kp.as<uint8_t>() + row.off, g->h_kp.data() + row.off, (size_t)n_slots, hipMemcpyHostToDevice);
        return rc;
    }
    memcpy(g->h_kp.data() + row.off, kp, (size_t)n_slots);
    return ORBGPU_OK;
}

int orbgpu_covis_observations(orbgpu_covis_graph *g, int32_t n, const int64_t *mp_ids, int32_t *n_obs, int32_t *n_slots)
{
    ORBGPU_REQUIRE(g && n >= 0 && n <= CV_MAX_CALL && (n == 0 || (mp_ids && n_obs && n_slots)), "bad argument");
    for (int i = 0; i < n; i++)
        ORBGPU_REQUIRE(mp_ids[i] >= -1, "map point id %lld (entry %d)", (long long)mp_ids[i], i);
    std::vector<int64_t> q;
    std::vector<int32_t> mult;
    cv_query(n, mp_ids, q, mult);
    const int nq = (int)q.size();
    for (int i = 0; i < n; i++)
        n_obs[i] = n_slots[i] = 0;
    if (nq == 0 || g->rows == g->n_bad)
        return ORBGPU_OK;  // nothing is held anywhere: no device needed
    int rc = cv_bind(g);
    if (rc != ORBGPU_OK)
        return rc;
    Carver c;
    const size_t o_q = c.take(8 * (size_t)nq), o_obs = c.take(4 * (size_t)nq), o_cnt = c.take(4 * (size_t)nq);
    if ((rc = cv_reserve_locked(g->d_stage, c.off)) != ORBGPU_OK)
        return rc;
    char *st = g->d_stage.as<char>();
    std::vector<int32_t> obs((size_t)nq), cnt((size_t)nq);
    hipError_t he = hipMemcpyAsync(st + o_q, q.data(), 8 * (size_t)nq, hipMemcpyHostToDevice, g->stream);
    if (he == hipSuccess)
        he = hipMemsetAsync(st + o_obs, 0, c.off - o_obs, g->stream);
    if (he == hipSuccess) {
        cv_launch_cull_count(g, nq, reinterpret_cast<const int64_t *>(st + o_q), 1, reinterpret_cast<int32_t *>(st + o_obs),
                             reinterpret_cast<int32_t *>(st + o_cnt));
        he = hipGetLastError();
    }
    if (he == hipSuccess)
        he = hipMemcpyAsync(obs.data(), st + o_obs, 4 * (size_t)nq, hipMemcpyDeviceToHost, g->stream);
    if (he == hipSuccess)
        he = hipMemcpyAsync(cnt.data(), st + o_cnt, 4 * (size_t)nq, hipMemcpyDeviceToHost, g->stream);
    if ((rc = cv_sync_or_fail(g, he, "observations query")) != ORBGPU_OK)
        return rc;
    for (int i = 0; i < n; i++) {
        if (mp_ids[i] < 0)
            continue;
        const size_t k = (size_t)(std::lower_bound(q.begin(), q.end(), mp_ids[i]) - q.begin());
        n_obs[i] = obs[k];
        n_slots[i] = cnt[k];
    }
    return ORBGPU_OK;
}

int orbgpu_covis_keyframe_culling(orbgpu_covis_graph *g, int32_t n, const int64_t *kf_ids, const uint8_t *not_erase, int32_t th_obs,
                                  int8_t *verdict, int32_t *n_mps, int32_t *n_redundant, int32_t point_capacity,
                                  int64_t *bad_point_ids, orbgpu_covis_culling_result *res)
{
    ORBGPU_REQUIRE(g && res, "null argument");
    ORBGPU_REQUIRE(n >= 0 && n <= CV_MAX_CANDIDATES, "n = %d (at most %d)", n, CV_MAX_CANDIDATES);
    ORBGPU_REQUIRE(n == 0 || (kf_ids && verdict && n_mps && n_redundant), "null argument");
    ORBGPU_REQUIRE(th_obs >= 1 && th_obs <= 255, "th_obs = %d (1 to 255)", th_obs);
    ORBGPU_REQUIRE(point_capacity >= 0 && (point_capacity == 0 || bad_point_ids), "bad output capacity");
    for (int k = 0; k < n; k++)
        ORBGPU_REQUIRE(kf_ids[k] >= 0, "key frame id %lld (entry %d)", (long long)kf_ids[k], k);
    // what the host knows of a candidate: its row, unless LocalMapping.cc:643 or V8 skips it whatever came before; and the
    // first position that names the same row, where the device records a verdict 1
    std::vector<int32_t> cand((size_t)n, -1), first((size_t)n, 0);
    std::unordered_map<int, int> seen;
    std::vector<int64_t> slots;
    int slot_cap = 1;
    for (int k = 0; k < n; k++) {
        const int r = kf_ids[k] == 0 ? -1 : g->hash.find(kf_ids[k]);
        first[(size_t)k] = k;
        if (r < 0 || g->h_rows[(size_t)r].bad)
            continue;
        cand[(size_t)k] = r;
        const auto it = seen.find(r);
        if (it != seen.end()) {
            first[(size_t)k] = it->second;
            continue;
        }
        seen.emplace(r, k);
        const CvRow &row = g->h_rows[(size_t)r];
        slot_cap = std::max(slot_cap, row.n_slots);
        for (int e = 0; e < row.n_slots; e++)
            if (g->h_pool[(size_t)(row.off + e)] >= 0)
                slots.push_back(g->h_pool[(size_t)(row.off + e)]);
    }
    std::sort(slots.begin(), slots.end());
    slots.erase(std::unique(slots.begin(), slots.end()), slots.end());
    if (slots.size() > (size_t)CV_MAX_QUERY_POINTS) {
        set_error("the candidates hold %zu distinct map points (at most %d)", slots.size(), CV_MAX_QUERY_POINTS);
        return ORBGPU_ECAPACITY;
    }
    const int nq = (int)slots.size();
    memset(res, 0, sizeof(*res));
    res->n_query_points = nq;
    if (seen.empty()) {  // every candidate is skipped: no device needed
        for (int k = 0; k < n; k++) {
            verdict[k] = -1;
            n_mps[k] = n_redundant[k] = 0;
        }
        res->n_skipped = n;
        return ORBGPU_OK;
    }
    int rc = cv_bind(g);
    if (rc != ORBGPU_OK)
        return rc;
    // uploaded | zeroed | written by the kernels
    Carver c;
    const size_t nq1 = (size_t)std::max(nq, 1);
    const size_t o_q = c.take(8 * nq1), o_cand = c.take(4 * (size_t)n), o_first = c.take(4 * (size_t)n), o_ne = c.take((size_t)n);
    const size_t in_bytes = c.off;
    const size_t o_obs = c.take(4 * nq1), o_cnt = c.take(4 * nq1 * CV_LEVELS), o_dead = c.take(nq1), o_culled = c.take((size_t)n);
    const size_t zero_end = c.off;
    const size_t o_verdict = c.take((size_t)n), o_mps = c.take(4 * (size_t)n), o_red = c.take(4 * (size_t)n), o_bad = c.take(8 * nq1);
    const size_t o_slotq = c.take(4 * (size_t)slot_cap);
    if ((rc = cv_reserve_locked(g->d_stage, c.off)) != ORBGPU_OK)
        return rc;
    g->stage.assign(in_bytes, 0);
    if (nq)
        memcpy(g->stage.data() + o_q, slots.data(), 8 * (size_t)nq);
    memcpy(g->stage.data() + o_cand, cand.data(), 4 * (size_t)n);
    memcpy(g->stage.data() + o_first, first.data(), 4 * (size_t)n);
    for (int k = 0; not_erase && k < n; k++)
        g->stage[o_ne + (size_t)k] = not_erase[k] != 0;
    char *st = g->d_stage.as<char>();
    long long *hdr = g->d_hdr.as<long long>();
    long long h[CU_WORDS] = {};
    hipError_t he = hipMemcpyAsync(st, g->stage.data(), in_bytes, hipMemcpyHostToDevice, g->stream);
    if (he == hipSuccess)
        he = hipMemsetAsync(st + o_obs, 0, zero_end - o_obs, g->stream);
    if (he == hipSuccess)
        he = hipMemsetAsync(hdr, 0, 8 * CH_WORDS, g->stream);
    if (he == hipSuccess) {
        const int64_t *q = reinterpret_cast<const int64_t *>(st + o_q);
        const CvCull cu{n, nq, th_obs, q, reinterpret_cast<const int32_t *>(st + o_cand), reinterpret_cast<const int32_t *>(st + o_first),
                        reinterpret_cast<const uint8_t *>(st + o_ne), reinterpret_cast<int32_t *>(st + o_obs),
                        reinterpret_cast<int32_t *>(st + o_cnt), reinterpret_cast<uint8_t *>(st + o_dead),
                        reinterpret_cast<uint8_t *>(st + o_culled), reinterpret_cast<int8_t *>(st + o_verdict),
                        reinterpret_cast<int32_t *>(st + o_mps), reinterpret_cast<int32_t *>(st + o_red), slot_cap,
                        reinterpret_cast<int32_t *>(st + o_slotq)};
        cv_launch_cull_count(g, nq, q, CV_LEVELS, cu.obs, cu.cnt);
        hipLaunchKernelGGL(k_covis_cull_resolve, dim3(1), dim3(CV_LIST_BLOCK), 0, g->stream, cu, g->rows, g->d_rows.as<CvRow>(),
                           g->d_pool.as<int64_t>(), g->d_kp.as<uint8_t>(), g->pool_used, hdr);
        hipLaunchKernelGGL(k_covis_cull_emit, dim3(1), dim3(CV_LIST_BLOCK), 0, g->stream, nq, q, cu.dead, nq,
                           reinterpret_cast<int64_t *>(st + o_bad), hdr);
        he = hipGetLastError();
    }
    // first wait: the header and the per-candidate outputs
    if (he == hipSuccess)
        he = hipMemcpyAsync(h, hdr, 8 * CU_WORDS, hipMemcpyDeviceToHost, g->stream);
    if (he == hipSuccess)
        he = hipMemcpyAsync(verdict, st + o_verdict, (size_t)n, hipMemcpyDeviceToHost, g->stream);
    if (he == hipSuccess)
        he = hipMemcpyAsync(n_mps, st + o_mps, 4 * (size_t)n, hipMemcpyDeviceToHost, g->stream);
    if (he == hipSuccess)
        he = hipMemcpyAsync(n_redundant, st + o_red, 4 * (size_t)n, hipMemcpyDeviceToHost, g->stream);
    if ((rc = cv_sync_or_fail(g, he, "key frame culling")) != ORBGPU_OK)
        return rc;
    if (h[CU_BAD] < 0 || h[CU_BAD] > nq) {
        set_error("covisibility graph: an index left its range on the device");
        return ORBGPU_EHIP;
    }
    res->n_culled = (int32_t)h[CU_CULLED];
    res->n_to_be_erased = (int32_t)h[CU_TO_BE_ERASED];
    res->n_skipped = (int32_t)h[CU_SKIPPED];
    res->n_points_bad = (int32_t)h[CU_BAD];
    // second wait: the bad points, as long as the caller's array
    const int nb = std::min(res->n_points_bad, point_capacity);
    if (nb > 0) {
        he = hipMemcpyAsync(bad_point_ids, st + o_bad, 8 * (size_t)nb, hipMemcpyDeviceToHost, g->stream);
        if ((rc = cv_sync_or_fail(g, he, "key frame culling (bad points)")) != ORBGPU_OK)
            return rc;
    }
    return ORBGPU_OK;
}

int orbgpu_covis_graph_set_scale_factors(orbgpu_covis_graph *g, int32_t n_levels, const float *scale_factors)
{
    ORBGPU_REQUIRE(g, "null argument");
    ORBGPU_REQUIRE(n_levels >= 1 && n_levels <= CV_LEVELS, "n_levels = %d (1 to %d)", n_levels, CV_LEVELS);
    ORBGPU_REQUIRE(scale_factors, "null argument");
    for (int l = 0; l < n_levels; l++)
        ORBGPU_REQUIRE(std::isfinite(scale_factors[l]) && scale_factors[l] > 0.f, "scale factor %g at level %d", (double)scale_factors[l], l);
    g->scale = CvScale{};  // host only: the kernels take the table by value
    g->scale.n_levels = n_levels;
    std::copy(scale_factors, scale_factors + n_levels, g->scale.sf);
    return ORBGPU_OK;
}

int orbgpu_covis_graph_set_descriptors(orbgpu_covis_graph *g, int64_t kf_id, int32_t n_slots, const uint8_t *desc)
{
    ORBGPU_REQUIRE(g, "null argument");
    const int r = g->hash.find(kf_id);
    ORBGPU_REQUIRE(r >= 0, "key frame %lld is not in the graph", (long long)kf_id);
    const CvRow &row = g->h_rows[(size_t)r];
    ORBGPU_REQUIRE(n_slots == row.n_slots, "n_slots = %d, key frame %lld has %d", n_slots, (long long)kf_id, row.n_slots);
    ORBGPU_REQUIRE(n_slots == 0 || desc, "null argument");
    if (row.bad || n_slots == 0)
        return ORBGPU_OK;  // a bad key frame holds no slot (V2)
    int rc = cv_bind(g);
    if (rc != ORBGPU_OK)
        return rc;
    // the column comes with its first use; until then cv_grow_pool carries two columns
    rc = lifecycle_locked_unless(g->has_desc_col, lifecycle_mutex(), [&] {
        const int rr = g->d_desc.reserve(32 * (size_t)g->pool_cap);
        g->has_desc_col = rr == ORBGPU_OK;
        return rr;
    });
    if (rc != ORBGPU_OK)
        return rc;
    CvRow nr = row;
    nr.has_desc = 1;
    hipError_t he = hipMemcpyAsync(g->d_desc.as<uint8_t>() + 32 * (size_t)row.off, desc, 32 * (size_t)n_slots, hipMemcpyHostToDevice, g->stream);
    if (he == hipSuccess)
        he = hipMemcpyAsync(g->d_rows.as<CvRow>() + r, &nr, sizeof(CvRow), hipMemcpyHostToDevice, g->stream);
    if ((rc = cv_sync_or_fail(g, he, "setting descriptors")) != ORBGPU_OK) {
        (void)hipMemcpy(g->d_rows.as<CvRow>() + r, &row, sizeof(CvRow), hipMemcpyHostToDevice);  // the flag as it was
        return rc;
    }
    g->h_rows[(size_t)r] = nr;
    return ORBGPU_OK;
}

int orbgpu_covis_graph_set_centres(orbgpu_covis_graph *g, int32_t n, const int64_t *kf_ids, const float *centres, int32_t *known)
{
    ORBGPU_REQUIRE(g && n >= 0 && n <= CV_MAX_CALL && (n == 0 || (kf_ids && centres)), "bad argument");
    if (known)
        *known = 0;
    // applied in order to the mirror (later entries win); the device gets the rows from the first to the last one touched
    std::vector<std::pair<int, CvCentre>> undo;
    int n_known = 0, lo = INT_MAX, hi = -1;
    for (int i = 0; i < n; i++) {
        const int r = g->hash.find(kf_ids[i]);
        if (r < 0)
            continue;  // an unknown key frame: ignored
        n_known++;
        if (g->h_rows[(size_t)r].bad)
            continue;
        undo.emplace_back(r, g->h_centre[(size_t)r]);
        g->h_centre[(size_t)r] = CvCentre{centres[3 * (size_t)i], centres[3 * (size_t)i + 1], centres[3 * (size_t)i + 2], 1};
        lo = std::min(lo, r);
        hi = std::max(hi, r);
    }
    if (!undo.empty()) {
        auto fail = [&](int rc) {
            for (size_t k = undo.size(); k-- > 0;)
                g->h_centre[(size_t)undo[k].first] = undo[k].second;
            return rc;
        };
        int rc = cv_bind(g);
        if (rc != ORBGPU_OK)
            return fail(rc);
        const hipError_t he = hipMemcpyAsync(g->d_centre.as<CvCentre>() + lo, g->h_centre.data() + lo, sizeof(CvCentre) * (size_t)(hi - lo + 1),
                                             hipMemcpyHostToDevice, g->stream);
        if ((rc = cv_sync_or_fail(g, he, "setting camera centres")) != ORBGPU_OK) {
            fail(rc);
            (void)hipMemcpy(g->d_centre.as<CvCentre>() + lo, g->h_centre.data() + lo, sizeof(CvCentre) * (size_t)(hi - lo + 1), hipMemcpyHostToDevice);
            return rc;
        }
        g->centres_set = true;
    }
    if (known)
        *known = n_known;
    return ORBGPU_OK;
}

int orbgpu_covis_refresh_points(orbgpu_covis_graph *g, int32_t n, const int64_t *mp_ids, const int64_t *ref_kf_ids,
                                const float *world_pos, uint32_t what, float *normal, float *min_dist, float *max_dist,
                                uint8_t *desc, int64_t *desc_kf, int32_t *desc_idx, int32_t *n_slots, uint8_t *status,
                                orbgpu_covis_refresh_result *res)
{
    std::vector<int32_t> perm;
    const int rc = covis_refresh_check(g, n, mp_ids, ref_kf_ids, what, n_slots, status, res, perm);
    if (rc != ORBGPU_OK)
        return rc;
    ORBGPU_REQUIRE(n == 0 || world_pos, "null argument");
    return covis_refresh_run(g, n, mp_ids, ref_kf_ids, world_pos, what, normal, min_dist, max_dist, desc, desc_kf, desc_idx, n_slots,
                             status, res, perm, nullptr);
}

} // extern "C"

namespace orbgpu {

int covis_refresh_device_id(const orbgpu_covis_graph *g) { return g->device_id; }

int covis_refresh_check(const orbgpu_covis_graph *g, int32_t n, const int64_t *mp_ids, const int64_t *ref_kf_ids, uint32_t what,
                        const int32_t *n_slots, const uint8_t *status, const orbgpu_covis_refresh_result *res, std::vector<int32_t> &perm)
{
    ORBGPU_REQUIRE(g && res, "null argument");
    ORBGPU_REQUIRE(n >= 0 && n <= CV_REFRESH_MAX_POINTS, "n = %d (at most %d)", n, CV_REFRESH_MAX_POINTS);
    ORBGPU_REQUIRE(what != 0 && !(what & ~CV_REFRESH_HALVES), "what = 0x%x (ORBGPU_REFRESH_DESCRIPTOR | ORBGPU_REFRESH_NORMAL_DEPTH)", what);
    ORBGPU_REQUIRE(n == 0 || (mp_ids && ref_kf_ids && n_slots && status), "null argument");
    for (int i = 0; i < n; i++)
        ORBGPU_REQUIRE(mp_ids[i] >= 0, "map point id %lld (entry %d)", (long long)mp_ids[i], i);
    // the one sort of the call: the query in ascending id, as positions in the caller's arrays; equal ids end up adjacent
    std::vector<int32_t> p((size_t)n);
    for (int i = 0; i < n; i++)
        p[(size_t)i] = i;
    std::sort(p.begin(), p.end(), [mp_ids](int32_t a, int32_t b) { return mp_ids[a] < mp_ids[b]; });
    const auto dup = std::adjacent_find(p.begin(), p.end(), [mp_ids](int32_t a, int32_t b) { return mp_ids[a] == mp_ids[b]; });
    ORBGPU_REQUIRE(dup == p.end(), "map point id %lld appears twice in one refresh call", (long long)mp_ids[*dup]);
    perm.swap(p);
    return ORBGPU_OK;
}

int covis_refresh_run(orbgpu_covis_graph *g, int32_t n, const int64_t *mp_ids, const int64_t *ref_kf_ids, const float *world_pos,
                      uint32_t what, float *normal, float *min_dist, float *max_dist, uint8_t *desc, int64_t *desc_kf,
                      int32_t *desc_idx, int32_t *n_slots, uint8_t *status, orbgpu_covis_refresh_result *res,
                      const std::vector<int32_t> &perm, const RefreshTableIO *tio)
{
    memset(res, 0, sizeof(*res));
    if (n == 0)
        return ORBGPU_OK;
    const size_t nn = (size_t)n;
    if (!tio && g->rows == g->n_bad) {  // nothing is held anywhere (R2): no device needed
        for (int i = 0; i < n; i++) {
            status[i] = ORBGPU_REFRESH_NO_OBS;
            n_slots[i] = 0;
            if (desc_kf)
                desc_kf[i] = -1;
            if (desc_idx)
                desc_idx[i] = -1;
        }
        res->n_no_obs = n;
        return ORBGPU_OK;
    }
    int rc = cv_bind(g);
    if (rc != ORBGPU_OK)
        return rc;
    // the query in ascending id: the permutation is covis_refresh_check's; the results come back in the caller's order
    // uploaded | zeroed | written by the kernels
    Carver c;
    const size_t o_q = c.take(8 * nn), o_perm = c.take(4 * nn), o_ref = c.take(4 * nn), o_pos = c.take(tio ? 0 : 12 * nn);
    const size_t in_bytes = c.off;
    const size_t o_obs = c.take(4 * nn), o_cnt = c.take(4 * nn), o_cursor = c.take(4 * nn);
    const size_t zero_end = c.off;
    const size_t o_start = c.take(4 * nn), o_lw = c.take(4 * nn), o_lg = c.take(4 * nn);
    const size_t o_status = c.take(nn), o_ns = c.take(4 * nn), o_dkf = c.take(8 * nn), o_didx = c.take(4 * nn);
    const size_t o_nr = c.take(12 * nn), o_mn = c.take(4 * nn), o_mx = c.take(4 * nn), o_ds = c.take(32 * nn);
    const int64_t ent_cap = std::max<int64_t>(g->pool_used, 1);  // a slot holds one id, the query's ids are distinct
    if ((rc = cv_reserve_locked(g->d_stage, c.off)) != ORBGPU_OK ||
        (rc = cv_reserve_locked(g->d_ents, sizeof(CvEntry) * (size_t)ent_cap)) != ORBGPU_OK)
        return rc;
    g->stage.assign(in_bytes, 0);
    int64_t *h_q = reinterpret_cast<int64_t *>(g->stage.data() + o_q);
    int32_t *h_ref = reinterpret_cast<int32_t *>(g->stage.data() + o_ref);
    for (int k = 0; k < n; k++)
        h_q[k] = mp_ids[perm[(size_t)k]];
    memcpy(g->stage.data() + o_perm, perm.data(), 4 * nn);
    for (int i = 0; i < n; i++) {
        const int r = g->hash.find(ref_kf_ids[i]);
        h_ref[i] = r >= 0 && !g->h_rows[(size_t)r].bad ? r : -1;
    }
    if (!tio)
        memcpy(g->stage.data() + o_pos, world_pos, 12 * nn);
    char *st = g->d_stage.as<char>();
    long long *hdr = g->d_hdr.as<long long>();
    long long h[RH_WORDS] = {};
    std::vector<uint8_t> h_status(nn), h_desc;
    std::vector<int32_t> h_ns(nn), h_didx;
    std::vector<int64_t> h_dkf;
    std::vector<float> h_nr, h_mn, h_mx;
    hipError_t he = hipMemcpyAsync(st, g->stage.data(), in_bytes, hipMemcpyHostToDevice, g->stream);
    if (he == hipSuccess)
        he = hipMemsetAsync(st + o_obs, 0, zero_end - o_obs, g->stream);
    if (he == hipSuccess)
        he = hipMemsetAsync(hdr, 0, 8 * CH_WORDS, g->stream);
    if (he == hipSuccess) {
        CvRefresh cr{};
        cr.nq = n;
        cr.what = what;
        cr.q = reinterpret_cast<const int64_t *>(st + o_q);
        cr.perm = reinterpret_cast<const int32_t *>(st + o_perm);
        cr.ref_row = reinterpret_cast<const int32_t *>(st + o_ref);
        cr.pos = tio ? tio->pos : reinterpret_cast<const float *>(st + o_pos);
        if (tio) {
            cr.pre = tio->pre;
            cr.t_row = tio->row;
            cr.t_normal = tio->normal;
            cr.t_min = tio->min_dist;
            cr.t_max = tio->max_dist;
            cr.t_desc = tio->desc;
        }
        cr.obs = reinterpret_cast<int32_t *>(st + o_obs);
        cr.cnt = reinterpret_cast<int32_t *>(st + o_cnt);
        cr.cursor = reinterpret_cast<int32_t *>(st + o_cursor);
        cr.start = reinterpret_cast<int32_t *>(st + o_start);
        cr.list_w = reinterpret_cast<int32_t *>(st + o_lw);
        cr.list_g = reinterpret_cast<int32_t *>(st + o_lg);
        cr.normal = reinterpret_cast<float *>(st + o_nr);
        cr.min_dist = reinterpret_cast<float *>(st + o_mn);
        cr.max_dist = reinterpret_cast<float *>(st + o_mx);
        cr.desc = reinterpret_cast<uint8_t *>(st + o_ds);
        cr.desc_kf = reinterpret_cast<int64_t *>(st + o_dkf);
        cr.desc_idx = reinterpret_cast<int32_t *>(st + o_didx);
        cr.n_slots = reinterpret_cast<int32_t *>(st + o_ns);
        cr.status = reinterpret_cast<uint8_t *>(st + o_status);
        cr.ent_cap = ent_cap;
        cr.ents = g->d_ents.as<CvEntry>();
        const CvRow *rows = g->d_rows.as<CvRow>();
        if (g->rows > 0)
            cv_launch_cull_count(g, n, cr.q, 1, cr.obs, cr.cnt);
        hipLaunchKernelGGL(k_covis_refresh_scan, dim3(1), dim3(CV_LIST_BLOCK), 0, g->stream, cr, hdr);
        if (g->rows > 0) {
            const int grid = std::min((g->rows + CV_WAVES - 1) / CV_WAVES, 4096);
            if (n <= g->lds_ids)
                hipLaunchKernelGGL(k_covis_refresh_fill<true>, dim3(grid), dim3(CV_BLOCK), 8 * nn, g->stream, g->rows, rows,
                                   g->d_pool.as<int64_t>(), g->pool_used, cr, hdr);
            else {
                g->global_queries++;
                hipLaunchKernelGGL(k_covis_refresh_fill<false>, dim3(grid), dim3(CV_BLOCK), 0, g->stream, g->rows, rows,
                                   g->d_pool.as<int64_t>(), g->pool_used, cr, hdr);
            }
            // the lists' lengths stay on the device: grids by their bounds, a workgroup past the end returns at once
            const int grid_w = std::min(n, 16384);
            const int grid_g = (int)std::min<int64_t>(std::min<int64_t>(n, g->pool_used / (CV_REFRESH_WAVE + 1) + 1), 4096);
            const uint8_t *kp = g->d_kp.as<uint8_t>(), *descs = g->d_desc.as<uint8_t>();
            const CvCentre *centres = g->d_centre.as<CvCentre>();
            if (g->refresh_rows)
                hipLaunchKernelGGL((k_covis_refresh<64, 1, true>), dim3(grid_w), dim3(64), 0, g->stream, 0, rows, kp, descs, centres,
                                   g->scale, cr, hdr);
            else
                hipLaunchKernelGGL((k_covis_refresh<64, 1, false>), dim3(grid_w), dim3(64), 0, g->stream, 0, rows, kp, descs, centres,
                                   g->scale, cr, hdr);
            hipLaunchKernelGGL((k_covis_refresh<256, 4, false>), dim3(grid_g), dim3(256), 0, g->stream, 1, rows, kp, descs, centres,
                               g->scale, cr, hdr);
        }
        he = hipGetLastError();
    }
    // the one wait: the header, status and n_slots, and what the caller asked for
    auto fetch = [&](void *dst, size_t off, size_t bytes) {
        if (he == hipSuccess)
            he = hipMemcpyAsync(dst, st + off, bytes, hipMemcpyDeviceToHost, g->stream);
    };
    if (he == hipSuccess)
        he = hipMemcpyAsync(h, hdr, 8 * RH_WORDS, hipMemcpyDeviceToHost, g->stream);
    fetch(h_status.data(), o_status, nn);
    fetch(h_ns.data(), o_ns, 4 * nn);
    if (desc_kf) {
        h_dkf.resize(nn);
        fetch(h_dkf.data(), o_dkf, 8 * nn);
    }
    if (desc_idx) {
        h_didx.resize(nn);
        fetch(h_didx.data(), o_didx, 4 * nn);
    }
    if (normal && (what & ORBGPU_REFRESH_NORMAL_DEPTH)) {
        h_nr.resize(3 * nn);
        fetch(h_nr.data(), o_nr, 12 * nn);
    }
    if (min_dist && (what & ORBGPU_REFRESH_NORMAL_DEPTH)) {
        h_mn.resize(nn);
        fetch(h_mn.data(), o_mn, 4 * nn);
    }
    if (max_dist && (what & ORBGPU_REFRESH_NORMAL_DEPTH)) {
        h_mx.resize(nn);
        fetch(h_mx.data(), o_mx, 4 * nn);
    }
    if (desc && (what & ORBGPU_REFRESH_DESCRIPTOR)) {
        h_desc.resize(32 * nn);
        fetch(h_desc.data(), o_ds, 32 * nn);
    }
    if ((rc = cv_sync_or_fail(g, he, "refresh query")) != ORBGPU_OK)
        return rc;
    if (h[RH_RANGE] || h[RH_ENTRIES] < 0 || h[RH_ENTRIES] > ent_cap) {
        set_error("covisibility graph: an index left its range on the device");
        return ORBGPU_EHIP;
    }
    // in/out: an entry the rules leave untouched keeps the caller's bytes
    const unsigned no_point = ORBGPU_REFRESH_NO_OBS | ORBGPU_REFRESH_OVERFLOW | ORBGPU_REFRESH_UNKNOWN | ORBGPU_REFRESH_BAD;
    res->n_entries = h[RH_ENTRIES];
    for (int i = 0; i < n; i++) {
        const unsigned s = h_status[(size_t)i];
        status[i] = (uint8_t)s;
        n_slots[i] = h_ns[(size_t)i];
        res->max_obs = std::max(res->max_obs, n_slots[i]);
        res->n_no_obs += (s & ORBGPU_REFRESH_NO_OBS) != 0;
        res->n_overflow += (s & ORBGPU_REFRESH_OVERFLOW) != 0;
        res->n_no_desc += (s & ORBGPU_REFRESH_NO_DESC) != 0;
        res->n_no_centre += (s & ORBGPU_REFRESH_NO_CENTRE) != 0;
        res->n_no_ref += (s & ORBGPU_REFRESH_NO_REF) != 0;
        res->n_unknown += (s & ORBGPU_REFRESH_UNKNOWN) != 0;
        res->n_bad += (s & ORBGPU_REFRESH_BAD) != 0;
        const bool wrote_desc = (what & ORBGPU_REFRESH_DESCRIPTOR) && !(s & (no_point | ORBGPU_REFRESH_NO_DESC));
        const bool wrote_nd = (what & ORBGPU_REFRESH_NORMAL_DEPTH) && !(s & (no_point | ORBGPU_REFRESH_NO_CENTRE | ORBGPU_REFRESH_NO_REF));
        res->n_descriptors += wrote_desc;
        res->n_normals += wrote_nd;
        if (desc_kf)
            desc_kf[i] = h_dkf[(size_t)i];
        if (desc_idx)
            desc_idx[i] = h_didx[(size_t)i];
        if (wrote_desc && desc)
            memcpy(desc + 32 * (size_t)i, h_desc.data() + 32 * (size_t)i, 32);
        if (wrote_nd && normal)
            memcpy(normal + 3 * (size_t)i, h_nr.data() + 3 * (size_t)i, 12);
        if (wrote_nd && min_dist)
            min_dist[i] = h_mn[(size_t)i];
        if (wrote_nd && max_dist)
            max_dist[i] = h_mx[(size_t)i];
    }
    return ORBGPU_OK;
}

} // namespace orbgpu

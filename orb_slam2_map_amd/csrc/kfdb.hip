// Device-resident KeyFrameDatabase: the BoW candidate search that starts relocalisation and loop detection.
//
// The reference keeps an inverted file -- one std::list<KeyFrame*> per vocabulary word (KeyFrameDatabase.cc:36) -- and a
// query walks the list of every query word, stamps and counts the key frames it meets (:86-104, :207-222), then runs
// L1Scoring::score on the ones that share enough words (:125-139, :242-253), sums the scores over each one's ten best
// covisible key frames (:148-173, :262-287) and keeps the best neighbours of the groups above 0.75 of the best sum.
// Here a key frame is a row keyed by KeyFrame::mnId; its BoW vector lies in one pool (word ids int32, values double),
// key-frame-major, and a query streams that pool once, 12 bytes per entry, instead of chasing per-word lists:
//   k_kfdb_score   one wave per row: every lane takes an entry of the row and binary-searches the query's word ids (staged
//                  in LDS, or read from global memory when the query is longer than the staging); hits are counted with
//                  __ballot / popcount and their terms added to the running double IN WORD ORDER, so the
//                  score has the reference's bits.  Yields words, first common word and score of every row, and the
//                  integer maximum of `words` (order-free).
//   k_kfdb_acc     one thread per row of the sharing list: threshold (K3), neighbours resolved through the device copy of
//                  the id hash (K7), float sum in list order (K6).
//   k_kfdb_select  one block: float max by reduction (no floating-point atomics), survivors compacted, and -- last -- the
//                  relocalisation score register of the scored rows (K5).
// The few survivor records are ordered (first common word, add sequence: K1) and de-duplicated on the host inside the
// entry point.  Every call returns synchronised; the caller serialises (KeyFrameDatabaseT does).  The device is bound at
// the first call that needs it, so that refusals (K8) are answered without one.
#include "common.h"
#include "compact_kernels.h"
#include "compact_plan.h"
#include "id_table.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <unordered_map>
#include <vector>

namespace orbgpu {

constexpr int KF_MAX_NB = 10;             // GetBestCovisibilityKeyFrames(10)
constexpr int KF_MAX_ROWS = 1 << 24;      // rows of a database between two clears or compactions
constexpr int KF_MAX_BOW = 1 << 24;       // entries of one BoW vector
constexpr int64_t KF_MAX_POOL = 1 << 30;  // entries of the pool
constexpr int KF_MAX_CALL = 1 << 24;      // ids per call
constexpr int KF_LDS_WORDS = 12288;       // query word ids staged per block (48 KiB)
constexpr int64_t KF_INITIAL_POOL = 1 << 22;  // entries allocated at most before the first add asks for more (48 MiB)
constexpr int KF_BLOCK = 256;
constexpr int KF_WAVES = KF_BLOCK / 64;
constexpr int KF_SELECT_BLOCK = 1024;

enum { KF_SHARING = 1, KF_SCORED = 2, KF_RETAINED = 4 };

struct KfRow {  // 112 bytes; the host keeps a mirror and uploads the part an edit changes
    int64_t id;
    int32_t off, len;  // the row's entries in the pool
    int32_t alive;
    float reg;         // mRelocScore: written by every reloc query that scores the row (K5)
    int32_t nn, pad;
    int64_t nb[KF_MAX_NB];
};

struct KfSurvivor {
    int32_t row, first;
    float acc;
    int32_t pad;
    int64_t best_id;
};

__global__ __launch_bounds__(256) void k_kfdb_mark(int n, const int32_t *__restrict__ list, int n_rows,
                                                   int32_t *__restrict__ excl, int stamp)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && list[i] >= 0 && list[i] < n_rows)
        excl[list[i]] = stamp;
}

// Item i is row sel[i] (orbgpu_keyframe_db_score; -1: unknown id) or row i (the detect calls, where dead rows and the
// rows of connected key frames -- excl[row] == stamp -- count no words).
template <bool LDS>
__global__ __launch_bounds__(KF_BLOCK) void k_kfdb_score(int n_items, const int32_t *__restrict__ sel, int n_rows,
                                                         const KfRow *__restrict__ rows, const int32_t *__restrict__ pool_ids,
                                                         const double *__restrict__ pool_vals, int nq,
                                                         const int32_t *__restrict__ q_ids, const double *__restrict__ q_vals,
                                                         const int32_t *__restrict__ excl, int stamp, int32_t *__restrict__ words,
                                                         int32_t *__restrict__ first, float *__restrict__ score,
                                                         int32_t *__restrict__ max_words)
{
    extern __shared__ int32_t s_q[];
    const int32_t *q = q_ids;
    if (LDS) {  // a template constant: the barrier is under workgroup-uniform control flow
        for (int i = threadIdx.x; i < nq; i += KF_BLOCK)
            s_q[i] = q_ids[i];
        __syncthreads();
        q = s_q;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int item = blockIdx.x * KF_WAVES + wave; item < n_items; item += gridDim.x * KF_WAVES) {  // wave-uniform
        const int row = sel ? sel[item] : item;
        bool live = row >= 0 && row < n_rows;
        int off = 0, len = 0;
        if (live) {
            live = rows[row].alive != 0 && (sel || excl[row] != stamp);
            off = rows[row].off;
            len = rows[row].len;
        }
        int n_common = 0, fw = -1;
        double s = 0.0;
        if (live) {
            for (int base = 0; base < len; base += 64) {
                const int e = base + lane;
                bool hit = false;
                int w = 0;
                double term = 0.0;
                if (e < len) {
                    w = pool_ids[off + e];
                    int lo = 0, hi = nq;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (q[mid] < w)
                            lo = mid + 1;
                        else
                            hi = mid;
                    }
                    if (lo < nq && q[lo] == w) {
                        hit = true;
                        const double vi = q_vals[lo], wi = pool_vals[off + e];
                        term = fabs(vi - wi) - fabs(vi) - fabs(wi);  // ScoringObject.cpp:41
                    }
                }
                unsigned long long m = __ballot(hit);  // the same mask in every lane
                if (m) {
                    if (fw < 0)
                        fw = __shfl(w, __ffsll((long long)m) - 1, 64);
                    n_common += __popcll(m);
                    while (m) {  // K2: the chunk's terms join the sum in ascending word id
                        s += __shfl(term, __ffsll((long long)m) - 1, 64);
                        m &= m - 1;
                    }
                }
            }
        }
        if (lane == 0) {
            words[item] = n_common;
            first[item] = fw;
            score[item] = live ? (float)(-s / 2.0) : __builtin_nanf("");
            if (!sel && n_common > 0)
                atomicMax(max_words, n_common);
        }
    }
}

__global__ __launch_bounds__(256) void k_kfdb_acc(int n_rows, const KfRow *__restrict__ rows, const int64_t *__restrict__ hkeys,
                                                  const int32_t *__restrict__ hvals, int log2cap,
                                                  const int32_t *__restrict__ words, const float *__restrict__ score,
                                                  const int32_t *__restrict__ max_words, int reloc, float min_score,
                                                  float *__restrict__ acc, int64_t *__restrict__ best, uint8_t *__restrict__ flag)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows)
        return;
    const int min_common = (int)((float)max_words[0] * 0.8f);  // K3
    const int w = words[r];
    uint8_t f = 0;
    float a = __builtin_nanf("");
    int64_t b = -1;
    if (w > 0) {
        f = KF_SHARING;
        if (w > min_common) {
            f |= KF_SCORED;
            const float si = score[r];
            if (reloc || si >= min_score) {
                f |= KF_RETAINED;
                float best_score = si;
                a = si;
                b = rows[r].id;
                const int nn = min(max(rows[r].nn, 0), KF_MAX_NB);
                for (int k = 0; k < nn; k++) {
                    const int r2 = id_hash_lookup(hkeys, hvals, log2cap, rows[r].nb[k]);
                    if (r2 < 0 || r2 >= n_rows || !rows[r2].alive || words[r2] <= 0)
                        continue;  // not in the database (K7) or not in the sharing list
                    float s2;
                    if (words[r2] > min_common)
                        s2 = score[r2];
                    else if (reloc)
                        s2 = rows[r2].reg;  // KeyFrameDatabase.cc:273-276: what an earlier query left (K5)
                    else
                        continue;  // :159
                    a += s2;
                    if (s2 > best_score) {
                        b = rows[r2].id;
                        best_score = s2;
                    }
                }
            }
        }
    }
    acc[r] = a;
    best[r] = b;
    flag[r] = f;
}

__global__ __launch_bounds__(KF_SELECT_BLOCK) void k_kfdb_select(int n_rows, KfRow *__restrict__ rows,
                                                                 const uint8_t *__restrict__ flag, const float *__restrict__ acc,
                                                                 const int64_t *__restrict__ best, const int32_t *__restrict__ first,
                                                                 const float *__restrict__ score, int reloc, float start, int cap,
                                                                 KfSurvivor *__restrict__ out, int32_t *__restrict__ n_out)
{
    __shared__ float s_red[KF_SELECT_BLOCK / 64];
    float m = start;  // bestAccScore: minScore (:145) or 0 (:259)
    for (int r = threadIdx.x; r < n_rows; r += KF_SELECT_BLOCK)
        if ((flag[r] & KF_RETAINED) && acc[r] > m)
            m = acc[r];
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_down(m, off, 64);
        if (o > m)
            m = o;
    }
    if ((threadIdx.x & 63) == 0)
        s_red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = s_red[0];
    for (int i = 1; i < KF_SELECT_BLOCK / 64; i++)
        if (s_red[i] > m)
            m = s_red[i];
    const float keep = 0.75f * m;  // :176, :290
    for (int r = threadIdx.x; r < n_rows; r += KF_SELECT_BLOCK) {
        const uint8_t f = flag[r];
        if ((f & KF_RETAINED) && acc[r] > keep) {
            const int k = atomicAdd(n_out, 1);
            if (k < cap)
                out[k] = KfSurvivor{r, first[r], acc[r], 0, best[r]};
        }
        if (reloc && (f & KF_SCORED))
            rows[r].reg = score[r];  // K5: after every read of the register by this query
    }
}

constexpr int KF_ROW_COLS = 9;  // the per-row arrays of orbgpu_keyframe_db

} // namespace orbgpu

using namespace orbgpu;

struct orbgpu_keyframe_db {
    int device_id = 0, n_words = 0, initial_rows = 0;
    bool bound = false;  // device selected, stream created, first buffers allocated
    hipStream_t stream = nullptr;
    int rows = 0, row_cap = 0, alive = 0;
    int64_t pool_used = 0, pool_cap = 0, next_seq = 0;
    // per row: named once with their bytes per row (growth carries all of them over: the last query's columns are read
    // afterwards).  The list points into the handle, which is therefore never copied.
    DevBuf d_rows, d_words, d_first, d_score, d_acc, d_best, d_flag, d_excl, d_surv;
    const IdColumn<DevBuf> row_cols[KF_ROW_COLS] = {{&d_rows, sizeof(KfRow)}, {&d_words, 4}, {&d_first, 4},
                                                    {&d_score, 4},            {&d_acc, 4},   {&d_best, 8},
                                                    {&d_flag, 1},             {&d_excl, 4},  {&d_surv, sizeof(KfSurvivor)}};
    orbgpu_keyframe_db() = default;
    orbgpu_keyframe_db(const orbgpu_keyframe_db &) = delete;
    DevBuf d_pool_ids, d_pool_vals, d_hkeys, d_hvals, d_stage, d_ctr;
    IdHash hash;  // id -> most recent row of the id (dead or alive); the device holds a byte-identical copy
    std::vector<KfRow> h_rows;
    std::vector<int64_t> h_seq;
    std::unordered_map<int64_t, std::vector<int64_t>> covis;  // K7: the lists as set, also of ids that are not rows
    std::vector<char> stage;
    int stamp = 0;
    int last_rows = 0;  // rows of the most recent detect call (0: none)
    int64_t global_queries = 0;  // score launches that read the query from global memory (tests)
};

namespace orbgpu {

static int lds_word_limit()
{
    // ORBGPU_DEBUG_KFDB_LDS_WORDS=<k> (tests): a query of more than k words takes the global-memory path
    const char *s = getenv("ORBGPU_DEBUG_KFDB_LDS_WORDS");
    if (!s)
        return KF_LDS_WORDS;
    return std::min(std::max(atoi(s), 0), KF_LDS_WORDS);
}

static int check_vector(int n_words, int32_t n, const int32_t *ids, const double *vals)
{
    ORBGPU_REQUIRE(n >= 0 && n <= KF_MAX_BOW && (n == 0 || (ids && vals)), "bad BoW vector (n = %d)", n);
    for (int i = 0; i < n; i++) {
        ORBGPU_REQUIRE(ids[i] >= 0 && ids[i] < n_words, "word id %d outside [0, %d)", ids[i], n_words);
        ORBGPU_REQUIRE(i == 0 || ids[i] > ids[i - 1], "word ids are not strictly ascending (entry %d)", i);
        ORBGPU_REQUIRE(std::isfinite(vals[i]), "value %d is not finite", i);
    }
    return ORBGPU_OK;
}

static int alive_row(const orbgpu_keyframe_db *db, int64_t id)
{
    const int r = db->hash.find(id);
    return r >= 0 && db->h_rows[(size_t)r].alive ? r : -1;
}

// Row capacity `want`: every per-row array and the hash are re-allocated, contents carried over -- the transaction of
// id_table.h: either everything has grown or nothing has.
static int grow_rows(orbgpu_keyframe_db *db, int want)
{
    if (want <= db->row_cap)
        return ORBGPU_OK;
    ORBGPU_REQUIRE(want <= KF_MAX_ROWS, "more than %d rows", KF_MAX_ROWS);
    int ncap = std::max(db->row_cap, 1);
    while (ncap < want)
        ncap *= 2;
    TableStreamOps ops{db->stream, "growing the key-frame database"};
    const IdTableParts<DevBuf> parts{db->row_cols, KF_ROW_COLS, KF_ROW_COLS, &db->d_hkeys, &db->d_hvals, &db->hash, &db->row_cap};
    return id_table_grow(parts, db->rows, ncap, ops);
}

static int grow_pool(orbgpu_keyframe_db *db, int64_t want)
{
    if (want <= db->pool_cap)
        return ORBGPU_OK;
    ORBGPU_REQUIRE(want <= KF_MAX_POOL, "more than %lld pool entries", (long long)KF_MAX_POOL);
    int64_t ncap = std::max<int64_t>(db->pool_cap, 1024);
    while (ncap < want)
        ncap *= 2;
    DevBuf ni, nv;
    int rc = ni.reserve(4 * (size_t)ncap);
    if (rc == ORBGPU_OK)
        rc = nv.reserve(8 * (size_t)ncap);
    hipError_t he = hipSuccess;
    if (rc == ORBGPU_OK && db->pool_used > 0) {
        he = hipMemcpyAsync(ni.p, db->d_pool_ids.p, 4 * (size_t)db->pool_used, hipMemcpyDeviceToDevice, db->stream);
        if (he == hipSuccess)
            he = hipMemcpyAsync(nv.p, db->d_pool_vals.p, 8 * (size_t)db->pool_used, hipMemcpyDeviceToDevice, db->stream);
        if (he == hipSuccess)
            he = hipStreamSynchronize(db->stream);
        if (he != hipSuccess) {
            set_error("growing the key-frame pool: %s", hipGetErrorString(he));
            rc = ORBGPU_EHIP;
        }
    }
    if (rc != ORBGPU_OK) {
        (void)hipStreamSynchronize(db->stream);
        ni.release();
        nv.release();
        return rc;
    }
    std::swap(db->d_pool_ids, ni);
    std::swap(db->d_pool_vals, nv);
    ni.release();
    nv.release();
    db->pool_cap = ncap;
    return ORBGPU_OK;
}

// Growth after the first call: under the lifecycle lock, on the growing branch only (id_table.h).
static int grow_locked(orbgpu_keyframe_db *db, int rows, int64_t pool)
{
    return lifecycle_locked_unless(rows <= db->row_cap && pool <= db->pool_cap, lifecycle_mutex(), [&] {
        const int rc = grow_rows(db, rows);
        return rc != ORBGPU_OK ? rc : grow_pool(db, pool);
    });
}
static int reserve_locked(DevBuf &b, size_t bytes)
{
    return lifecycle_locked_unless(bytes <= b.bytes, lifecycle_mutex(), [&] { return b.reserve(bytes); });
}

// what the first call allocates for (the creation argument, or its default); orbgpu_keyframe_db_compact returns to it (D3)
static int initial_rows(const orbgpu_keyframe_db *db) { return db->initial_rows > 0 ? db->initial_rows : 1024; }
static int64_t initial_pool(const orbgpu_keyframe_db *db) { return std::min<int64_t>((int64_t)initial_rows(db) * 512, KF_INITIAL_POOL); }

// first call that needs the device: select it, create the stream, allocate for initial_rows
static int bind(orbgpu_keyframe_db *db)
{
    int rc = select_device(db->device_id);
    if (rc != ORBGPU_OK || db->bound)
        return rc;
    std::lock_guard<std::mutex> lifecycle(lifecycle_mutex());
    if (!db->stream) {
        hipError_t he = hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking);
        if (he != hipSuccess) {
            db->stream = nullptr;
            set_error("hipStreamCreate: %s", hipGetErrorString(he));
            return ORBGPU_EHIP;
        }
    }
    if ((rc = grow_rows(db, initial_rows(db))) != ORBGPU_OK)
        return rc;
    if ((rc = grow_pool(db, initial_pool(db))) != ORBGPU_OK)
        return rc;
    if ((rc = db->d_ctr.reserve(64)) != ORBGPU_OK)
        return rc;
    db->bound = true;
    return ORBGPU_OK;
}

static int sync_or_fail(orbgpu_keyframe_db *db, hipError_t he, const char *what)
{
    const hipError_t se = hipStreamSynchronize(db->stream);  // also after a failed enqueue: copies read the caller's arrays
    if (he == hipSuccess)
        he = se;
    if (he != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(he));
        return ORBGPU_EHIP;
    }
    return ORBGPU_OK;
}

static void launch_score(orbgpu_keyframe_db *db, int n_items, const int32_t *sel, int nq, const int32_t *q_ids,
                         const double *q_vals, int32_t *words, int32_t *first, float *score, int32_t *max_words)
{
    const int grid = std::min((n_items + KF_WAVES - 1) / KF_WAVES, 4096);
    const KfRow *rows = db->d_rows.as<KfRow>();
    if (nq <= lds_word_limit())
        hipLaunchKernelGGL(k_kfdb_score<true>, dim3(grid), dim3(KF_BLOCK), sizeof(int32_t) * (size_t)std::max(nq, 1), db->stream,
                           n_items, sel, db->rows, rows, db->d_pool_ids.as<int32_t>(), db->d_pool_vals.as<double>(), nq, q_ids,
                           q_vals, db->d_excl.as<int32_t>(), db->stamp, words, first, score, max_words);
    else {
        db->global_queries++;
        hipLaunchKernelGGL(k_kfdb_score<false>, dim3(grid), dim3(KF_BLOCK), 0, db->stream, n_items, sel, db->rows, rows,
                           db->d_pool_ids.as<int32_t>(), db->d_pool_vals.as<double>(), nq, q_ids, q_vals,
                           db->d_excl.as<int32_t>(), db->stamp, words, first, score, max_words);
    }
}

static int detect(orbgpu_keyframe_db *db, bool reloc, int32_t nq, const int32_t *q_ids, const double *q_vals, int32_t n_conn,
                  const int64_t *conn, float min_score, int32_t capacity, int64_t *cand, int32_t *n_cand)
{
    ORBGPU_REQUIRE(db && n_cand && capacity >= 0 && (capacity == 0 || cand), "bad argument");
    ORBGPU_REQUIRE(n_conn >= 0 && n_conn <= KF_MAX_CALL && (n_conn == 0 || conn), "bad connected list");
    ORBGPU_REQUIRE(std::isfinite(min_score), "min_score is not finite");
    int rc = check_vector(db->n_words, nq, q_ids, q_vals);
    if (rc != ORBGPU_OK || (rc = bind(db)) != ORBGPU_OK)
        return rc;
    *n_cand = 0;
    db->last_rows = 0;
    if (nq == 0 || db->rows == 0 || db->alive == 0)
        return ORBGPU_OK;  // K9
    // stage: query values, query word ids, rows of the connected key frames
    std::vector<int32_t> conn_rows;
    for (int i = 0; i < n_conn; i++) {
        const int r = alive_row(db, conn[i]);
        if (r >= 0)
            conn_rows.push_back(r);
    }
    const int nc = (int)conn_rows.size();
    Carver c;
    const size_t o_vals = c.take(8 * (size_t)nq), o_ids = c.take(4 * (size_t)nq), o_conn = c.take(4 * (size_t)std::max(nc, 1));
    if ((rc = reserve_locked(db->d_stage, c.off)) != ORBGPU_OK)
        return rc;
    db->stage.resize(c.off);
    memcpy(db->stage.data() + o_vals, q_vals, 8 * (size_t)nq);
    memcpy(db->stage.data() + o_ids, q_ids, 4 * (size_t)nq);
    if (nc)
        memcpy(db->stage.data() + o_conn, conn_rows.data(), 4 * (size_t)nc);
    if (db->stamp == INT_MAX) {  // the stamps of 2^31 queries are used up: start again
        ORBGPU_HIP_TRY(hipMemsetAsync(db->d_excl.p, 0, 4 * (size_t)db->row_cap, db->stream));
        db->stamp = 0;
    }
    db->stamp++;
    char *st = db->d_stage.as<char>();
    int32_t *ctr = db->d_ctr.as<int32_t>();  // [0] maxCommonWords, [1] survivors
    hipError_t he = hipMemcpyAsync(st, db->stage.data(), c.off, hipMemcpyHostToDevice, db->stream);
    if (he == hipSuccess)
        he = hipMemsetAsync(ctr, 0, 64, db->stream);
    int32_t h_ctr[2] = {0, 0};
    std::vector<KfSurvivor> surv;
    if (he == hipSuccess) {
        const int n = db->rows;
        if (nc)
            hipLaunchKernelGGL(k_kfdb_mark, dim3((nc + 255) / 256), dim3(256), 0, db->stream, nc,
                               reinterpret_cast<const int32_t *>(st + o_conn), n, db->d_excl.as<int32_t>(), db->stamp);
        launch_score(db, n, nullptr, nq, reinterpret_cast<const int32_t *>(st + o_ids), reinterpret_cast<const double *>(st + o_vals),
                     db->d_words.as<int32_t>(), db->d_first.as<int32_t>(), db->d_score.as<float>(), ctr);
        hipLaunchKernelGGL(k_kfdb_acc, dim3((n + 255) / 256), dim3(256), 0, db->stream, n, db->d_rows.as<KfRow>(),
                           db->d_hkeys.as<int64_t>(), db->d_hvals.as<int32_t>(), db->hash.log2cap, db->d_words.as<int32_t>(),
                           db->d_score.as<float>(), ctr, reloc ? 1 : 0, min_score, db->d_acc.as<float>(), db->d_best.as<int64_t>(),
                           db->d_flag.as<uint8_t>());
        hipLaunchKernelGGL(k_kfdb_select, dim3(1), dim3(KF_SELECT_BLOCK), 0, db->stream, n, db->d_rows.as<KfRow>(),
                           db->d_flag.as<uint8_t>(), db->d_acc.as<float>(), db->d_best.as<int64_t>(), db->d_first.as<int32_t>(),
                           db->d_score.as<float>(), reloc ? 1 : 0, reloc ? 0.f : min_score, db->row_cap,
                           db->d_surv.as<KfSurvivor>(), ctr + 1);
        he = hipGetLastError();
        if (he == hipSuccess)
            he = hipMemcpyAsync(h_ctr, ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, db->stream);
    }
    if ((rc = sync_or_fail(db, he, "key-frame database query")) != ORBGPU_OK)
        return rc;
    const int ns = std::min(std::max(h_ctr[1], 0), db->rows);
    if (ns > 0) {
        surv.resize((size_t)ns);
        he = hipMemcpyAsync(surv.data(), db->d_surv.p, sizeof(KfSurvivor) * (size_t)ns, hipMemcpyDeviceToHost, db->stream);
        if ((rc = sync_or_fail(db, he, "key-frame database query (survivors)")) != ORBGPU_OK)
            return rc;
    }
    db->last_rows = db->rows;
    // K1 order of the scored rows, K6 first occurrence of every best neighbour
    for (const KfSurvivor &s : surv)
        ORBGPU_REQUIRE(s.row >= 0 && s.row < db->rows, "survivor row %d outside the table", s.row);
    std::sort(surv.begin(), surv.end(), [db](const KfSurvivor &a, const KfSurvivor &b) {
        return a.first != b.first ? a.first < b.first : db->h_seq[(size_t)a.row] < db->h_seq[(size_t)b.row];
    });
    std::vector<int64_t> seen;
    int32_t n_out = 0;
    for (const KfSurvivor &s : surv) {
        if (std::find(seen.begin(), seen.end(), s.best_id) != seen.end())
            continue;
        seen.push_back(s.best_id);
        if (n_out < capacity)
            cand[n_out] = s.best_id;
        n_out++;
    }
    *n_cand = n_out;
    return ORBGPU_OK;
}

static int destroy_impl(orbgpu_keyframe_db *db)
{
    if (!db)
        return ORBGPU_OK;
    if (db->bound || db->stream) {
        (void)hipSetDevice(db->device_id);
        if (db->stream) {
            (void)hipStreamSynchronize(db->stream);
            (void)hipStreamDestroy(db->stream);
        }
        for (const IdColumn<DevBuf> &c : db->row_cols)
            c.buf->release();
        for (DevBuf *b : {&db->d_pool_ids, &db->d_pool_vals, &db->d_hkeys, &db->d_hvals, &db->d_stage, &db->d_ctr})
            b->release();
    }
    delete db;
    return ORBGPU_OK;
}

} // namespace orbgpu

extern "C" {

int orbgpu_keyframe_db_create(int32_t n_words, int32_t scoring, int32_t device_id, int32_t initial_rows,
                              orbgpu_keyframe_db **out)
{
    ORBGPU_REQUIRE(out, "null argument");
    ORBGPU_REQUIRE(n_words > 0, "n_words = %d", n_words);
    ORBGPU_REQUIRE(scoring == 0, "scoring type %d: the key-frame database scores with L1_NORM (0) only", scoring);
    ORBGPU_REQUIRE(device_id >= 0 && initial_rows >= 0 && initial_rows <= KF_MAX_ROWS, "bad argument");
    orbgpu_keyframe_db *db = new (std::nothrow) orbgpu_keyframe_db();
    if (!db) {
        set_error("out of host memory");
        return ORBGPU_ENOMEM;
    }
    db->n_words = n_words;
    db->device_id = device_id;
    db->initial_rows = initial_rows;
    *out = db;
    return ORBGPU_OK;
}

int orbgpu_keyframe_db_destroy(orbgpu_keyframe_db *db)
{
    std::lock_guard<std::mutex> lifecycle(orbgpu::lifecycle_mutex());
    return destroy_impl(db);
}

int orbgpu_keyframe_db_clear(orbgpu_keyframe_db *db)
{
    ORBGPU_REQUIRE(db, "null argument");
    if (db->bound) {
        int rc = select_device(db->device_id);
        if (rc != ORBGPU_OK)
            return rc;
        hipError_t he = hipMemsetAsync(db->d_hkeys.p, 0xFF, sizeof(int64_t) << db->hash.log2cap, db->stream);  // ID_HASH_EMPTY
        if ((rc = sync_or_fail(db, he, "clearing the key-frame database")) != ORBGPU_OK)
            return rc;
    }
    db->hash.clear();
    db->h_rows.clear();
    db->h_seq.clear();
    db->covis.clear();
    db->rows = db->alive = db->last_rows = 0;
    db->pool_used = db->next_seq = 0;
    return ORBGPU_OK;
}

int orbgpu_keyframe_db_size(const orbgpu_keyframe_db *db, int32_t *alive)
{
    ORBGPU_REQUIRE(db && alive, "null argument");
    *alive = db->alive;
    return ORBGPU_OK;
}

int orbgpu_keyframe_db_add(orbgpu_keyframe_db *db, int64_t id, int32_t n_bow, const int32_t *bow_ids, const double *bow_vals)
{
    ORBGPU_REQUIRE(db && id >= 0, "bad argument");
    int rc = check_vector(db->n_words, n_bow, bow_ids, bow_vals);
    if (rc != ORBGPU_OK)
        return rc;
    ORBGPU_REQUIRE(alive_row(db, id) < 0, "key frame %lld is in the database", (long long)id);
    if ((rc = bind(db)) != ORBGPU_OK || (rc = grow_locked(db, db->rows + 1, db->pool_used + n_bow)) != ORBGPU_OK)
        return rc;
    KfRow row{};
    row.id = id;
    row.off = (int32_t)db->pool_used;
    row.len = n_bow;
    row.alive = 1;
    row.reg = 0.f;
    for (int k = 0; k < KF_MAX_NB; k++)
        row.nb[k] = -1;
    const auto it = db->covis.find(id);
    if (it != db->covis.end()) {
        row.nn = (int32_t)it->second.size();
        std::copy(it->second.begin(), it->second.end(), row.nb);
    }
    const int r = db->rows;
    const uint32_t slot = db->hash.slot_for(id);
    hipError_t he = hipSuccess;
    if (n_bow > 0) {
        he = hipMemcpyAsync(db->d_pool_ids.as<int32_t>() + db->pool_used, bow_ids, 4 * (size_t)n_bow, hipMemcpyHostToDevice,
                            db->stream);
        if (he == hipSuccess)
            he = hipMemcpyAsync(db->d_pool_vals.as<double>() + db->pool_used, bow_vals, 8 * (size_t)n_bow, hipMemcpyHostToDevice,
                                db->stream);
    }
    if (he == hipSuccess)
        he = hipMemcpyAsync(db->d_rows.as<KfRow>() + r, &row, sizeof(row), hipMemcpyHostToDevice, db->stream);
    if (he == hipSuccess)
        he = hipMemcpyAsync(db->d_hvals.as<int32_t>() + slot, &r, 4, hipMemcpyHostToDevice, db->stream);
    if (he == hipSuccess)
        he = hipMemcpyAsync(db->d_hkeys.as<int64_t>() + slot, &id, 8, hipMemcpyHostToDevice, db->stream);
    if ((rc = sync_or_fail(db, he, "adding a key frame")) != ORBGPU_OK)
        return rc;
    db->hash.keys[slot] = id;
    db->hash.vals[slot] = r;
    db->h_rows.push_back(row);
    db->h_seq.push_back(db->next_seq++);
    db->pool_used += n_bow;
    db->rows++;
    db->alive++;
    return ORBGPU_OK;
}

int orbgpu_keyframe_db_erase(orbgpu_keyframe_db *db, int32_t n, const int64_t *ids, int32_t *known)
{
    ORBGPU_REQUIRE(db && n >= 0 && n <= KF_MAX_CALL && (n == 0 || ids), "bad argument");
    if (known)
        *known = 0;
    if (n == 0 || db->alive == 0)
        return ORBGPU_OK;
    int rc = bind(db);
    if (rc != ORBGPU_OK)
        return rc;
    hipError_t he = hipSuccess;
    const int32_t dead = 0;
    std::vector<int> done;
    for (int i = 0; i < n && he == hipSuccess; i++) {
        const int r = alive_row(db, ids[i]);
        if (r < 0)
            continue;  // unknown, or named twice in this call
        db->h_rows[(size_t)r].alive = 0;
        done.push_back(r);
        he = hipMemcpyAsync(reinterpret_cast<char *>(db->d_rows.as<KfRow>() + r) + offsetof(KfRow, alive), &dead, 4,
                            hipMemcpyHostToDevice, db->stream);
    }
    if ((rc = sync_or_fail(db, he, "erasing key frames")) != ORBGPU_OK) {
        for (int r : done)
            db->h_rows[(size_t)r].alive = 1;
        return rc;
    }
    db->alive -= (int)done.size();
    for (int r : done)
        db->covis.erase(db->h_rows[(size_t)r].id);  // K7: an erased key frame's list goes with it
    if (known)
        *known = (int32_t)done.size();
    return ORBGPU_OK;
}

int orbgpu_keyframe_db_set_covisibles(orbgpu_keyframe_db *db, int64_t id, int32_t n, const int64_t *neighbour_ids)
{
    ORBGPU_REQUIRE(db && id >= 0, "bad argument");
    ORBGPU_REQUIRE(n >= 0 && n <= KF_MAX_NB && (n == 0 || neighbour_ids), "%d neighbours (at most %d)", n, KF_MAX_NB);
    for (int k = 0; k < n; k++)
        ORBGPU_REQUIRE(neighbour_ids[k] >= 0, "neighbour id %lld", (long long)neighbour_ids[k]);
    const int r = alive_row(db, id);
    if (r >= 0) {
        int rc = bind(db);
        if (rc != ORBGPU_OK)
            return rc;
        KfRow row = db->h_rows[(size_t)r];
        row.nn = n;
        for (int k = 0; k < KF_MAX_NB; k++)
            row.nb[k] = k < n ? neighbour_ids[k] : -1;
        const size_t o = offsetof(KfRow, nn);
        hipError_t he = hipMemcpyAsync(reinterpret_cast<char *>(db->d_rows.as<KfRow>() + r) + o,
                                       reinterpret_cast<const char *>(&row) + o, sizeof(KfRow) - o, hipMemcpyHostToDevice, db->stream);
        if ((rc = sync_or_fail(db, he, "setting covisible key frames")) != ORBGPU_OK)
            return rc;
        db->h_rows[(size_t)r] = row;
    }
    db->covis[id].assign(neighbour_ids, neighbour_ids + n);
    return ORBGPU_OK;
}

int orbgpu_keyframe_db_debug_global_queries(const orbgpu_keyframe_db *db, int64_t *n)
{
    ORBGPU_REQUIRE(db && n, "null argument");
    *n = db->global_queries;
    return ORBGPU_OK;
}

// D1-D4 (orbgpu.h).  The rows are gathered on the device: the relocalisation score register of K5 lives there only.
int orbgpu_keyframe_db_compact(orbgpu_keyframe_db *db, orbgpu_compact_result *res)
{
    ORBGPU_REQUIRE(db, "null argument");
    const int n = db->rows;
    std::vector<int32_t> len((size_t)n);
    std::vector<uint8_t> keep((size_t)n);
    for (int r = 0; r < n; r++) {
        len[(size_t)r] = db->h_rows[(size_t)r].len;
        keep[(size_t)r] = db->h_rows[(size_t)r].alive != 0;
    }
    const CompactPlan plan = compact_plan(n, len.data(), keep.data(), keep.data(), db->pool_used, -1);
    const int m = (int)plan.src.size();
    orbgpu_compact_result out{};
    out.rows_before = out.rows_after = n;
    out.row_capacity = db->row_cap;
    out.slots_before = out.slots_after = db->pool_used;
    out.slot_capacity = db->pool_cap;
    if (!plan.needed) {  // D4
        db->last_rows = 0;  // D2: last_query starts over with every compact call that succeeds, as tests/compact_model.py has it
        if (res)
            *res = out;
        return ORBGPU_OK;
    }
    int rc = bind(db);  // (a database with rows is bound: this selects the device)
    if (rc != ORBGPU_OK)
        return rc;
    const int ncap = (int)compact_capacity(1, initial_rows(db), m);
    const int64_t pcap = compact_capacity(1024, initial_pool(db), plan.pool_after);
    std::vector<KfRow> n_rows((size_t)m);
    std::vector<int64_t> n_seq((size_t)m), old_off((size_t)m);
    for (int i = 0; i < m; i++) {
        const size_t r = (size_t)plan.src[(size_t)i];
        n_rows[(size_t)i] = db->h_rows[r];
        n_rows[(size_t)i].off = (int32_t)plan.off[(size_t)i];
        n_seq[(size_t)i] = db->h_seq[r];
        old_off[(size_t)i] = db->h_rows[r].off;
    }
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
    TableStreamOps ops{db->stream, "compacting the key-frame database"};
    const IdColumn<DevBuf> pool_cols[2] = {{&db->d_pool_ids, 4}, {&db->d_pool_vals, 8}};
    // d_stage, which carries the plan, is per-call scratch outside the transaction.  Of the row columns only the rows
    // are carried: the others describe the last query, which last_query no longer reports (D2), and start as zeros -- no
    // stamp of d_excl is 0 when a query reads it.
    auto fill = [&](const DevBuf *nb, const DevBuf *np, int l2, IdHash &nh) -> int {
        if (m > 0) {
            const int rr = db->d_stage.reserve(c.off);
            if (rr != ORBGPU_OK)
                return rr;
            char *st = db->d_stage.as<char>();
            if (ops.upload(st, stage.data(), c.off))
                return ORBGPU_EHIP;
            const int64_t *noff = reinterpret_cast<const int64_t *>(st + o_new);
            hipLaunchKernelGGL(k_compact_rows<KfRow>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, db->stream, m,
                               reinterpret_cast<const int32_t *>(st + o_src), noff, n, db->d_rows.as<KfRow>(),
                               static_cast<KfRow *>(nb[0].p));
            if (plan.pool_after > 0) {
                CompactPool<2> p{};
                for (int k = 0; k < 2; k++) {
                    p.src[k] = static_cast<const uint8_t *>(pool_cols[k].buf->p);
                    p.dst[k] = static_cast<uint8_t *>(np[k].p);
                }
                hipLaunchKernelGGL((k_compact_pool<4, 8>), dim3((unsigned)compact_pool_grid(m)), dim3(COMPACT_BLOCK), 0, db->stream, m,
                                   reinterpret_cast<const int64_t *>(st + o_old), noff, reinterpret_cast<const int32_t *>(st + o_len),
                                   db->pool_used, pcap, p);
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
        const IdTableParts<DevBuf> parts{db->row_cols, KF_ROW_COLS, KF_ROW_COLS, &db->d_hkeys, &db->d_hvals, &db->hash, &db->row_cap};
        if ((rc = id_table_compact(parts, ncap, pool_cols, 2, (size_t)pcap, ops, fill)) != ORBGPU_OK)
            return rc;
    }
    db->h_rows.swap(n_rows);
    db->h_seq.swap(n_seq);
    db->rows = m;
    db->pool_used = plan.pool_after;
    db->pool_cap = pcap;
    db->last_rows = 0;
    out.compacted = 1;
    out.rows_after = m;
    out.row_capacity = db->row_cap;
    out.slots_after = db->pool_used;
    out.slot_capacity = db->pool_cap;
    if (res)
        *res = out;
    return ORBGPU_OK;
}

int orbgpu_keyframe_db_score(orbgpu_keyframe_db *db, int32_t n_bow, const int32_t *bow_ids, const double *bow_vals, int32_t n,
                             const int64_t *ids, float *scores)
{
    ORBGPU_REQUIRE(db && n >= 0 && n <= KF_MAX_CALL && (n == 0 || (ids && scores)), "bad argument");
    int rc = check_vector(db->n_words, n_bow, bow_ids, bow_vals);
    if (rc != ORBGPU_OK || (rc = bind(db)) != ORBGPU_OK)
        return rc;
    if (n == 0)
        return ORBGPU_OK;
    Carver c;
    const size_t o_vals = c.take(8 * (size_t)std::max(n_bow, 1)), o_ids = c.take(4 * (size_t)std::max(n_bow, 1)),
                 o_sel = c.take(4 * (size_t)n), in_bytes = c.off, o_words = c.take(4 * (size_t)n), o_first = c.take(4 * (size_t)n),
                 o_score = c.take(4 * (size_t)n);
    if ((rc = reserve_locked(db->d_stage, c.off)) != ORBGPU_OK)
        return rc;
    db->stage.resize(in_bytes);
    if (n_bow) {
        memcpy(db->stage.data() + o_vals, bow_vals, 8 * (size_t)n_bow);
        memcpy(db->stage.data() + o_ids, bow_ids, 4 * (size_t)n_bow);
    }
    int32_t *sel = reinterpret_cast<int32_t *>(db->stage.data() + o_sel);
    for (int i = 0; i < n; i++)
        sel[i] = alive_row(db, ids[i]);
    char *st = db->d_stage.as<char>();
    hipError_t he = hipMemcpyAsync(st, db->stage.data(), in_bytes, hipMemcpyHostToDevice, db->stream);
    if (he == hipSuccess) {
        launch_score(db, n, reinterpret_cast<const int32_t *>(st + o_sel), n_bow, reinterpret_cast<const int32_t *>(st + o_ids),
                     reinterpret_cast<const double *>(st + o_vals), reinterpret_cast<int32_t *>(st + o_words),
                     reinterpret_cast<int32_t *>(st + o_first), reinterpret_cast<float *>(st + o_score),
                     db->d_ctr.as<int32_t>() + 2);
        he = hipGetLastError();
    }
    if (he == hipSuccess)
        he = hipMemcpyAsync(scores, st + o_score, 4 * (size_t)n, hipMemcpyDeviceToHost, db->stream);
    return sync_or_fail(db, he, "scoring key frames");
}

int orbgpu_keyframe_db_detect_loop(orbgpu_keyframe_db *db, int32_t n_bow, const int32_t *bow_ids, const double *bow_vals,
                                   int32_t n_connected, const int64_t *connected_ids, float min_score, int32_t capacity,
                                   int64_t *candidate_ids, int32_t *n_candidates)
{
    return detect(db, false, n_bow, bow_ids, bow_vals, n_connected, connected_ids, min_score, capacity, candidate_ids,
                  n_candidates);
}

int orbgpu_keyframe_db_detect_reloc(orbgpu_keyframe_db *db, int32_t n_bow, const int32_t *bow_ids, const double *bow_vals,
                                    int32_t capacity, int64_t *candidate_ids, int32_t *n_candidates)
{
    return detect(db, true, n_bow, bow_ids, bow_vals, 0, nullptr, 0.f, capacity, candidate_ids, n_candidates);
}

int orbgpu_keyframe_db_last_query(orbgpu_keyframe_db *db, int32_t capacity, int64_t *ids, int32_t *words, int32_t *first_word,
                                  float *score, float *acc, int64_t *best_id, int32_t *n)
{
    ORBGPU_REQUIRE(db && n && capacity >= 0, "bad argument");
    *n = 0;
    const int nr = db->last_rows;
    if (nr == 0)
        return ORBGPU_OK;
    int rc = bind(db);
    if (rc != ORBGPU_OK)
        return rc;
    std::vector<int32_t> h_words((size_t)nr), h_first((size_t)nr);
    std::vector<float> h_score((size_t)nr), h_acc((size_t)nr);
    std::vector<int64_t> h_best((size_t)nr);
    std::vector<uint8_t> h_flag((size_t)nr);
    struct {
        void *dst;
        const DevBuf *src;
        size_t elt;
    } copies[] = {{h_words.data(), &db->d_words, 4}, {h_first.data(), &db->d_first, 4}, {h_score.data(), &db->d_score, 4},
                  {h_acc.data(), &db->d_acc, 4},     {h_best.data(), &db->d_best, 8},   {h_flag.data(), &db->d_flag, 1}};
    hipError_t he = hipSuccess;
    for (const auto &cp : copies)
        if (he == hipSuccess)
            he = hipMemcpyAsync(cp.dst, cp.src->p, cp.elt * (size_t)nr, hipMemcpyDeviceToHost, db->stream);
    if ((rc = sync_or_fail(db, he, "reading the last query")) != ORBGPU_OK)
        return rc;
    std::vector<int> order;
    for (int r = 0; r < nr; r++)
        if (h_flag[(size_t)r] & KF_SHARING)
            order.push_back(r);
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        return h_first[(size_t)a] != h_first[(size_t)b] ? h_first[(size_t)a] < h_first[(size_t)b]
                                                        : db->h_seq[(size_t)a] < db->h_seq[(size_t)b];
    });
    *n = (int32_t)order.size();
    const float nan = std::nanf("");
    for (int k = 0; k < (int)order.size() && k < capacity; k++) {
        const size_t r = (size_t)order[(size_t)k];
        if (ids)
            ids[k] = db->h_rows[r].id;
        if (words)
            words[k] = h_words[r];
        if (first_word)
            first_word[k] = h_first[r];
        if (score)
            score[k] = (h_flag[r] & KF_SCORED) ? h_score[r] : nan;
        if (acc)
            acc[k] = (h_flag[r] & KF_RETAINED) ? h_acc[r] : nan;
        if (best_id)
            best_id[k] = (h_flag[r] & KF_RETAINED) ? h_best[r] : -1;
    }
    return ORBGPU_OK;
}

} // extern "C"

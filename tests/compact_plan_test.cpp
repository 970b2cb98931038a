// CPU unit test of a compaction's host-only parts: the plan (orb_slam2_map_amd/csrc/compact_plan.h) and the transaction it
// runs in (id_table_compact, orb_slam2_map_amd/csrc/id_table.h).  Plain g++ with the sanitizers, no HIP.  The plan is
// checked against a restatement on hand cases and on every keep mask of a small table; the capacity rule against a
// simulation of the doubling; the transaction over malloc-backed buffers with a recording Ops, in the manner of
// tests/id_table_test.cpp: every allocation and every operation failed once, then none.
#include "compact_plan.h"
#include "id_table.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);   \
            return 1;                                             \
        }                                                         \
    } while (0)

using namespace orbgpu;

constexpr int64_t NONE = -77;

// ---- the plan ----------------------------------------------------------------------------------

static int check_plan(const std::vector<int32_t> &len, const std::vector<uint8_t> &keep, const std::vector<uint8_t> &owns,
                      const std::vector<uint8_t> &holds)
{
    const int n = (int)len.size();
    int64_t before = 0;
    for (int r = 0; r < n; r++)
        before += holds[(size_t)r] ? len[(size_t)r] : 0;
    const CompactPlan p = compact_plan(n, len.data(), keep.data(), owns.data(), before, NONE);
    // the restatement
    int64_t run = 0;
    size_t i = 0;
    bool dropped = false, frees = false;
    for (int r = 0; r < n; r++) {
        if (!keep[(size_t)r]) {
            dropped = true;
            continue;
        }
        CHECK(i < p.src.size() && p.src[i] == r);
        if (owns[(size_t)r]) {
            CHECK(p.off[i] == run && p.len[i] == len[(size_t)r]);
            run += len[(size_t)r];
        } else {
            CHECK(p.off[i] == NONE && p.len[i] == 0);
            frees = frees || (holds[(size_t)r] && len[(size_t)r] > 0);
        }
        i++;
    }
    CHECK(i == p.src.size() && p.off.size() == i && p.len.size() == i);
    CHECK(p.pool_after == run);
    CHECK(p.dropped == n - (int)i);
    // C6: needed iff a row is dropped or a kept row that owns nothing afterwards holds entries now.  (A dropped row of
    // length 0 that holds nothing is still a dropped row.)
    bool holds_consistent = true;  // every row that owns afterwards holds now: the tables never hand pool space out in a compaction
    for (int r = 0; r < n; r++)
        holds_consistent = holds_consistent && (!keep[(size_t)r] || !owns[(size_t)r] || holds[(size_t)r]);
    CHECK(holds_consistent);
    CHECK(p.needed == (dropped || frees));
    return 0;
}

static int test_plan()
{
    const std::vector<int32_t> lens = {0, 1, 63, 64, 65, 130, 4097};
    const int n = (int)lens.size();
    // 0 rows
    {
        const CompactPlan p = compact_plan(0, nullptr, nullptr, nullptr, 0, NONE);
        CHECK(p.src.empty() && p.off.empty() && p.pool_after == 0 && p.dropped == 0 && !p.needed);
    }
    const std::vector<uint8_t> all((size_t)n, 1), none((size_t)n, 0);
    std::vector<uint8_t> first = all, last = all, alt = all;
    first[0] = 0;
    last[(size_t)n - 1] = 0;
    for (int r = 0; r < n; r += 2)
        alt[(size_t)r] = 0;
    for (const std::vector<uint8_t> &keep : {all, none, first, last, alt})
        if (check_plan(lens, keep, all, all))
            return 1;
    {  // all kept, everything owned: nothing to do
        const CompactPlan p = compact_plan(n, lens.data(), all.data(), all.data(), 0 + 1 + 63 + 64 + 65 + 130 + 4097, NONE);
        CHECK(!p.needed && p.pool_after == 4420 && (int)p.src.size() == n);
        CHECK(p.off[0] == 0 && p.off[1] == 0 && p.off[2] == 1 && p.off[3] == 64 && p.off[4] == 128 && p.off[5] == 193 && p.off[6] == 323);
    }
    // every keep mask of the seven rows x two ownership patterns: kept rows that own no pool, holding space or not
    for (int mask = 0; mask < (1 << n); mask++) {
        std::vector<uint8_t> keep((size_t)n), owns((size_t)n), holds_all((size_t)n, 1), holds_own((size_t)n);
        for (int r = 0; r < n; r++) {
            keep[(size_t)r] = (mask >> r) & 1;
            owns[(size_t)r] = r % 3 != 1;
            holds_own[(size_t)r] = owns[(size_t)r] || !keep[(size_t)r];
        }
        if (check_plan(lens, keep, owns, holds_all) || check_plan(lens, keep, owns, holds_own))
            return 1;
    }
    {  // a second compaction right after one: the kept not-owning rows hold nothing any more
        const std::vector<int32_t> l = {5, 7, 0, 3};
        const std::vector<uint8_t> keep = {1, 1, 1, 1}, owns = {1, 0, 0, 1};
        const CompactPlan a = compact_plan(4, l.data(), keep.data(), owns.data(), 15, NONE);
        CHECK(a.needed && a.pool_after == 8 && a.off[1] == NONE && a.off[3] == 5);
        const CompactPlan b = compact_plan(4, l.data(), keep.data(), owns.data(), a.pool_after, NONE);
        CHECK(!b.needed && b.pool_after == 8);
    }
    return 0;
}

// ---- C1 ------------------------------------------------------------------------------------------

static int test_keep()
{
    // ids 10..17; parents: 11 -> 10 (bad parent of a live row: kept), 13 -> 12 (bad parent of a bad row: dropped),
    // 14 -> 99 (no row: ignored), 15 -> 15's parent 16 is live, 17 names 10 too
    const int64_t id[] = {10, 11, 12, 13, 14, 15, 16, 17};
    const int64_t parent[] = {-1, 10, 16, 12, 99, 16, -1, 10};
    const int32_t bad[] = {1, 0, 1, 1, 0, 0, 0, 1};
    const std::vector<uint8_t> k = compact_keep_graph(8, bad, id, parent);
    const uint8_t want[] = {1, 1, 0, 0, 1, 1, 1, 0};
    for (int r = 0; r < 8; r++)
        CHECK(k[(size_t)r] == want[r]);
    // a chain 20 <- 21 <- 22, all bad but the last: only 22 and its parent 21 stay; once 22 is bad too, nothing stays
    const int64_t cid[] = {20, 21, 22}, cpar[] = {-1, 20, 21};
    const int32_t cbad[] = {1, 1, 0}, call[] = {1, 1, 1}, cnone[] = {0, 0, 0};
    std::vector<uint8_t> c = compact_keep_graph(3, cbad, cid, cpar);
    CHECK(!c[0] && c[1] && c[2]);
    c = compact_keep_graph(3, call, cid, cpar);
    CHECK(!c[0] && !c[1] && !c[2]);
    c = compact_keep_graph(3, cnone, cid, cpar);
    CHECK(c[0] && c[1] && c[2]);
    // a bad row that names itself is not kept by that; no rows
    const int64_t sid[] = {5}, spar[] = {5};
    const int32_t sbad[] = {1};
    CHECK(!compact_keep_graph(1, sbad, sid, spar)[0]);
    CHECK(compact_keep_graph(0, nullptr, nullptr, nullptr).empty());
    return 0;
}

// ---- C5 / D3 ---------------------------------------------------------------------------------------

// a fresh handle: the first call grows to `initial`, later ones one row (or `step` entries) at a time
static int64_t simulate(int64_t base, int64_t initial, int64_t want, int64_t step)
{
    int64_t cap = 0;
    auto grow = [&](int64_t w) {
        if (w <= cap)
            return;
        int64_t ncap = std::max(cap, base);
        while (ncap < w)
            ncap *= 2;
        cap = ncap;
    };
    grow(initial);
    for (int64_t have = 0; have < want; have += step)
        grow(std::min(have + step, want));
    return cap;
}

static int test_capacity()
{
    for (int64_t base : {1, 1024})
        for (int64_t initial : {1, 2, 3, 8, 1000, 1024, 1025, 4096})
            for (int64_t want : {0, 1, 2, 3, 5, 8, 9, 1023, 1024, 1025, 4420, 70000})
                for (int64_t step : {1, 7, 4097})
                    CHECK(compact_capacity(base, initial, want) == simulate(base, initial, want, step));
    CHECK(compact_capacity(1, 2, 0) == 2 && compact_capacity(1, 2, 13) == 16 && compact_capacity(1024, 8, 4420) == 8192);
    return 0;
}

// ---- the transaction -------------------------------------------------------------------------------

static std::vector<std::string> g_log;  // "alloc", "free", "zero", "copy", "upload", "kernel", "sync"; a failed step ends in '!'
static std::vector<void *> g_freed;
static int g_countdown = 0;  // the step that fails (1 = the next one, 0 = none)
static int g_live = 0;       // buffers allocated and not freed

static bool step(const char *what)
{
    const bool fail = g_countdown > 0 && --g_countdown == 0;
    g_log.push_back(std::string(what) + (fail ? "!" : ""));
    return fail;
}

struct FakeBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int reserve(size_t n)
    {
        if (n <= bytes)
            return ORBGPU_OK;
        release();
        if (step("alloc"))
            return ORBGPU_ENOMEM;
        p = std::malloc(n);
        bytes = n;
        g_live++;
        return ORBGPU_OK;
    }
    void release()
    {
        if (p) {
            std::free(p);
            g_log.push_back("free");
            g_freed.push_back(p);
            g_live--;
        }
        p = nullptr;
        bytes = 0;
    }
};

struct FakeOps {
    int zero(void *p, size_t n) { return step("zero") ? 1 : (std::memset(p, 0, n), 0); }
    int copy(void *d, const void *s, size_t n) { return step("copy") ? 1 : (std::memcpy(d, s, n), 0); }
    int upload(void *d, const void *s, size_t n) { return step("upload") ? 1 : (std::memcpy(d, s, n), 0); }
    int sync() { return step("sync") ? 1 : 0; }
    void drain() { g_log.push_back("sync"); }
};

// a table of two row columns (a 24-byte row {id, off, len} and a 4-byte one), three pool columns of 8 / 1 / 32 bytes
constexpr int N_COLS = 2, N_POOL = 3, ROWS = 6, CAP = 8;
constexpr size_t POOL_CAP = 1024;
static const size_t ELT[N_COLS] = {24, 4}, PELT[N_POOL] = {8, 1, 32};
struct Row {
    int64_t id, off, len;
};
static const int64_t IDS[ROWS] = {7, 1ll << 40, 0, 123456789, 3, 55};
static const int32_t LEN[ROWS] = {3, 0, 65, 1, 4, 2};
static const uint8_t KEEP[ROWS] = {0, 1, 1, 0, 1, 1}, OWNS[ROWS] = {1, 1, 1, 1, 0, 1};

struct Table {
    FakeBuf col[N_COLS], pool[N_POOL], hkeys, hvals;
    IdColumn<FakeBuf> cols[N_COLS] = {{&col[0], ELT[0]}, {&col[1], ELT[1]}};
    IdColumn<FakeBuf> pcols[N_POOL] = {{&pool[0], PELT[0]}, {&pool[1], PELT[1]}, {&pool[2], PELT[2]}};
    IdHash hash;
    int rows = 0, cap = 0;
    int64_t pool_used = 0, pool_cap = 0;
    IdTableParts<FakeBuf> parts() { return {cols, N_COLS, N_COLS, &hkeys, &hvals, &hash, &cap}; }
    std::vector<FakeBuf *> all() { return {&col[0], &col[1], &pool[0], &pool[1], &pool[2], &hkeys, &hvals}; }
    void release()
    {
        for (FakeBuf *b : all())
            b->release();
    }
};

struct Snapshot {
    std::vector<void *> p;
    std::vector<size_t> bytes;
    std::vector<std::vector<unsigned char>> content;
    int rows, cap, log2cap;
    int64_t pool_used, pool_cap;
    std::vector<int64_t> keys;
    std::vector<int32_t> vals;
};

static Snapshot snapshot(Table &t)
{
    Snapshot s;
    for (FakeBuf *b : t.all()) {
        s.p.push_back(b->p);
        s.bytes.push_back(b->bytes);
        s.content.emplace_back((unsigned char *)b->p, (unsigned char *)b->p + b->bytes);
    }
    s.rows = t.rows, s.cap = t.cap, s.log2cap = t.hash.log2cap, s.pool_used = t.pool_used, s.pool_cap = t.pool_cap;
    s.keys = t.hash.keys, s.vals = t.hash.vals;
    return s;
}

static bool same(Table &t, const Snapshot &s)
{
    const Snapshot n = snapshot(t);
    return n.p == s.p && n.bytes == s.bytes && n.content == s.content && n.rows == s.rows && n.cap == s.cap && n.log2cap == s.log2cap &&
           n.pool_used == s.pool_used && n.pool_cap == s.pool_cap && n.keys == s.keys && n.vals == s.vals;
}

static unsigned char pool_byte(int c, int64_t entry, size_t b) { return (unsigned char)(1 + 60 * c + 7 * entry + b); }

static int make_table(Table &t)
{
    FakeOps ops;
    g_countdown = 0;
    CHECK(id_table_grow(t.parts(), 0, CAP, ops) == ORBGPU_OK && t.cap == CAP);
    for (int c = 0; c < N_POOL; c++) {
        CHECK(t.pool[c].reserve(PELT[c] * POOL_CAP) == ORBGPU_OK);
        std::memset(t.pool[c].p, 0xEE, t.pool[c].bytes);
    }
    t.pool_cap = (int64_t)POOL_CAP;
    for (int r = 0; r < ROWS; r++) {
        ((Row *)t.col[0].p)[r] = Row{IDS[r], t.pool_used, LEN[r]};
        ((int32_t *)t.col[1].p)[r] = 1000 + r;
        for (int c = 0; c < N_POOL; c++)
            for (int64_t e = t.pool_used; e < t.pool_used + LEN[r]; e++)
                for (size_t b = 0; b < PELT[c]; b++)
                    ((unsigned char *)t.pool[c].p)[PELT[c] * (size_t)e + b] = pool_byte(c, e, b);
        t.pool_used += LEN[r];
        t.hash.insert(IDS[r], r);
    }
    t.rows = ROWS;
    std::memcpy(t.hkeys.p, t.hash.keys.data(), 8 * t.hash.capacity());
    std::memcpy(t.hvals.p, t.hash.vals.data(), 4 * t.hash.capacity());
    return 0;
}

// what the tables' compact calls do: plan, new capacities, the fill (one upload of the plan, one "kernel" for the rows and
// one for the pool), and the bookkeeping after a success
static int run(Table &t, FakeOps &ops, FakeBuf &stage)
{
    const CompactPlan plan = compact_plan(ROWS, LEN, KEEP, OWNS, t.pool_used, NONE);
    if (!plan.needed)
        return -1;
    const int m = (int)plan.src.size();
    const int ncap = (int)compact_capacity(1, 2, m);
    const size_t pcap = (size_t)compact_capacity(512, 8, plan.pool_after);
    auto fill = [&](const FakeBuf *nb, const FakeBuf *np, int l2, IdHash &nh) -> int {
        const int rc = stage.reserve(4 * (size_t)m);
        if (rc != ORBGPU_OK)
            return rc;
        if (ops.upload(stage.p, plan.src.data(), 4 * (size_t)m) || step("kernel"))
            return ORBGPU_EHIP;
        const int32_t *src = (const int32_t *)stage.p;
        const Row *old = (const Row *)t.col[0].p;
        for (int i = 0; i < m; i++) {
            Row r = old[src[i]];
            r.off = plan.off[(size_t)i];
            ((Row *)nb[0].p)[i] = r;
            ((int32_t *)nb[1].p)[i] = ((const int32_t *)t.col[1].p)[src[i]];
        }
        if (step("kernel"))
            return ORBGPU_EHIP;
        for (int i = 0; i < m; i++)
            for (int c = 0; c < N_POOL; c++)
                std::memcpy((char *)np[c].p + PELT[c] * (size_t)std::max<int64_t>(plan.off[(size_t)i], 0),
                            (const char *)t.pool[c].p + PELT[c] * (size_t)old[src[i]].off, PELT[c] * (size_t)plan.len[(size_t)i]);
        nh.rebuild(l2);
        for (int i = 0; i < m; i++)
            nh.insert(old[src[i]].id, i);
        return ORBGPU_OK;
    };
    const int rc = id_table_compact(t.parts(), ncap, t.pcols, N_POOL, pcap, ops, fill);
    if (rc == ORBGPU_OK) {
        t.rows = m;
        t.pool_used = plan.pool_after;
        t.pool_cap = (int64_t)pcap;
    }
    return rc;
}

static int test_transaction()
{
    int n_steps = 0;
    {
        Table t;
        FakeOps ops;
        FakeBuf stage;
        if (make_table(t))
            return 1;
        g_log.clear();
        CHECK(run(t, ops, stage) == ORBGPU_OK);
        for (const std::string &e : g_log)
            n_steps += e != "free";
        // pool allocations, row and hash allocations, zeroes, the fill (stage, upload, two kernels), two uploads and the sync
        CHECK(n_steps == N_POOL + (N_COLS + 2) + N_COLS + 4 + 3);
        t.release();
        stage.release();
        CHECK(g_live == 0);
    }
    for (int k = 1; k <= n_steps; k++) {
        Table t;
        FakeOps ops;
        FakeBuf stage;
        if (make_table(t))
            return 1;
        const Snapshot before = snapshot(t);
        g_log.clear();
        g_freed.clear();
        g_countdown = k;
        const int rc = run(t, ops, stage);
        CHECK(g_countdown == 0);
        size_t failed = 0;
        while (failed < g_log.size() && g_log[failed].back() != '!')
            failed++;
        CHECK(failed < g_log.size());
        CHECK(rc == (g_log[failed] == "alloc!" ? ORBGPU_ENOMEM : ORBGPU_EHIP));
        CHECK(same(t, before));
        // after the failed step: nothing but a sync (once anything may be enqueued) and the frees of new buffers
        for (size_t i = failed + 1; i < g_log.size(); i++)
            CHECK(g_log[i] == "free" || (g_log[i] == "sync" && i == failed + 1));
        if ((int)failed >= N_POOL)  // inside id_table_replace
            CHECK(failed + 1 < g_log.size() && g_log[failed + 1] == "sync");
        for (void *p : g_freed)
            for (void *q : before.p)
                CHECK(p != q);
        // ... and the table still works: the same call, unfailed
        CHECK(run(t, ops, stage) == ORBGPU_OK);
        t.release();
        stage.release();
        CHECK(g_live == 0);  // nothing leaked (and ASan would say so)
    }
    // unfailed: what the plan promises, every id found or not through the uploaded hash, the old buffers freed exactly once
    Table t;
    FakeOps ops;
    FakeBuf stage;
    if (make_table(t))
        return 1;
    const Snapshot before = snapshot(t);
    g_log.clear();
    g_freed.clear();
    CHECK(run(t, ops, stage) == ORBGPU_OK);
    CHECK(t.rows == 4 && t.cap == 4 && t.hash.log2cap == 3 && t.hkeys.bytes == 8u << 3 && t.hvals.bytes == 4u << 3);
    CHECK(t.pool_used == 67 && t.pool_cap == 512);
    for (int c = 0; c < N_COLS; c++)
        CHECK(t.col[c].bytes == ELT[c] * 4);
    for (int c = 0; c < N_POOL; c++)
        CHECK(t.pool[c].bytes == PELT[c] * 512);
    const int want_src[] = {1, 2, 4, 5};
    const int64_t want_off[] = {0, 0, NONE, 65};
    int64_t old_off[ROWS], run_off = 0;
    for (int r = 0; r < ROWS; r++) {
        old_off[r] = run_off;
        run_off += LEN[r];
    }
    for (int i = 0; i < 4; i++) {
        const Row &r = ((const Row *)t.col[0].p)[i];
        CHECK(r.id == IDS[want_src[i]] && r.len == LEN[want_src[i]] && r.off == want_off[i]);
        CHECK(((const int32_t *)t.col[1].p)[i] == 1000 + want_src[i]);
        if (want_off[i] != NONE)
            for (int c = 0; c < N_POOL; c++)
                for (int64_t e = 0; e < r.len; e++)
                    for (size_t b = 0; b < PELT[c]; b++)
                        CHECK(((const unsigned char *)t.pool[c].p)[PELT[c] * (size_t)(r.off + e) + b] ==
                              pool_byte(c, old_off[want_src[i]] + e, b));
    }
    CHECK(std::memcmp(t.hkeys.p, t.hash.keys.data(), t.hkeys.bytes) == 0 && std::memcmp(t.hvals.p, t.hash.vals.data(), t.hvals.bytes) == 0);
    for (int r = 0; r < ROWS; r++) {
        int want = -1;
        for (int i = 0; i < 4; i++)
            if (want_src[i] == r)
                want = i;
        CHECK(id_hash_lookup((const int64_t *)t.hkeys.p, (const int32_t *)t.hvals.p, t.hash.log2cap, IDS[r]) == want);
        CHECK(t.hash.find(IDS[r]) == want);
    }
    for (void *q : before.p) {
        int n = 0;
        for (void *p : g_freed)
            n += p == q;
        CHECK(n == 1);
    }
    CHECK(g_freed.size() == before.p.size());
    // the second call in a row has nothing to do
    const int32_t len2[] = {0, 65, 4, 2};
    const uint8_t keep2[] = {1, 1, 1, 1}, owns2[] = {1, 1, 0, 1};
    CHECK(!compact_plan(4, len2, keep2, owns2, t.pool_used, NONE).needed);
    t.release();
    stage.release();
    CHECK(g_live == 0);
    return 0;
}

int main()
{
    if (test_plan() || test_keep() || test_capacity() || test_transaction())
        return 1;
    std::printf("compact_plan_test ok\n");
    return 0;
}

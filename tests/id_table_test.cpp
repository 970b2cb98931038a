// CPU unit test of the id tables' growth transaction (orb_slam2_map_amd/csrc/id_table.h): plain g++ with the sanitizers,
// no HIP.  Buffers are malloc-backed, the Ops record what they are asked to do, and a countdown makes the k-th step (an
// allocation or an operation) of a call fail.  A table of 3 carried columns (1, 12 and 8 bytes per row) and one scratch
// column, 5 rows, capacity 8 -> 16, is grown and -- retain-style -- compacted: every step failed once, then none.
#include "id_table.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);   \
            return 1;                                             \
        }                                                         \
    } while (0)

using namespace orbgpu;

static std::vector<std::string> g_log;  // "alloc", "free", "zero", "copy", "upload", "kernel", "sync"; a failed step ends in '!'
static std::vector<void *> g_freed;
static int g_countdown = 0;  // the step that fails (1 = the next one, 0 = none)

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
        return ORBGPU_OK;
    }
    void release()
    {
        if (p) {
            std::free(p);
            g_log.push_back("free");
            g_freed.push_back(p);
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

constexpr int N_COLS = 4, N_CARRIED = 3, ROWS = 5;
static const size_t ELT[N_COLS] = {1, 12, 8, 4};
static const int64_t IDS[ROWS] = {7, 1ll << 40, 0, 123456789, 3};

struct Table {
    FakeBuf col[N_COLS], hkeys, hvals;
    IdColumn<FakeBuf> cols[N_COLS] = {{&col[0], ELT[0]}, {&col[1], ELT[1]}, {&col[2], ELT[2]}, {&col[3], ELT[3]}};
    IdHash hash;
    int rows = 0, cap = 0;
    IdTableParts<FakeBuf> parts() { return {cols, N_CARRIED, N_COLS, &hkeys, &hvals, &hash, &cap}; }
    void release()
    {
        for (FakeBuf &b : col)
            b.release();
        hkeys.release();
        hvals.release();
    }
};

struct Snapshot {
    void *p[N_COLS + 2];
    size_t bytes[N_COLS + 2];
    std::vector<unsigned char> content[N_COLS];
    int rows, cap, log2cap;
    std::vector<int64_t> keys;
    std::vector<int32_t> vals;
};

static Snapshot snapshot(Table &t)
{
    Snapshot s;
    FakeBuf *all[N_COLS + 2] = {&t.col[0], &t.col[1], &t.col[2], &t.col[3], &t.hkeys, &t.hvals};
    for (int i = 0; i < N_COLS + 2; i++)
        s.p[i] = all[i]->p, s.bytes[i] = all[i]->bytes;
    for (int i = 0; i < N_COLS; i++)
        s.content[i].assign((unsigned char *)t.col[i].p, (unsigned char *)t.col[i].p + t.col[i].bytes);
    s.rows = t.rows, s.cap = t.cap, s.log2cap = t.hash.log2cap, s.keys = t.hash.keys, s.vals = t.hash.vals;
    return s;
}

static bool same(Table &t, const Snapshot &s)
{
    const Snapshot n = snapshot(t);
    bool ok = n.rows == s.rows && n.cap == s.cap && n.log2cap == s.log2cap && n.keys == s.keys && n.vals == s.vals;
    for (int i = 0; i < N_COLS + 2; i++)
        ok = ok && n.p[i] == s.p[i] && n.bytes[i] == s.bytes[i];
    for (int i = 0; i < N_COLS; i++)
        ok = ok && n.content[i] == s.content[i];
    return ok;
}

// a table of capacity 8 with ROWS rows: column bytes that name their column, row and byte; the hash uploaded
static int make_table(Table &t)
{
    FakeOps ops;
    g_countdown = 0;
    CHECK(id_table_grow(t.parts(), 0, 8, ops) == ORBGPU_OK && t.cap == 8 && t.hash.log2cap == 4);
    for (int c = 0; c < N_COLS; c++)
        for (size_t b = 0; b < ELT[c] * ROWS; b++)
            ((unsigned char *)t.col[c].p)[b] = (unsigned char)(1 + 50 * c + b);
    for (int r = 0; r < ROWS; r++)
        t.hash.insert(IDS[r], r);
    t.rows = ROWS;
    std::memcpy(t.hkeys.p, t.hash.keys.data(), 8 * t.hash.capacity());
    std::memcpy(t.hvals.p, t.hash.vals.data(), 4 * t.hash.capacity());
    return 0;
}

// retain-style fill: rows SRC of the old columns become rows 0.. of the new ones (one upload of the list, one "kernel")
static const int32_t SRC[] = {4, 0, 2};
constexpr int KEPT = 3;
struct RetainFill {
    Table &t;
    FakeOps &ops;
    FakeBuf &stage;
    int operator()(const FakeBuf *nb, int l2, IdHash &nh) const
    {
        int rc = stage.reserve(sizeof(SRC));
        if (rc != ORBGPU_OK)
            return rc;
        if (ops.upload(stage.p, SRC, sizeof(SRC)) || step("kernel"))
            return ORBGPU_EHIP;
        const int32_t *src = (const int32_t *)stage.p;
        for (int c = 0; c < N_CARRIED; c++)
            for (int i = 0; i < KEPT; i++)
                std::memcpy((char *)nb[c].p + ELT[c] * (size_t)i, (const char *)t.col[c].p + ELT[c] * (size_t)src[i], ELT[c]);
        nh.rebuild(l2);
        for (int i = 0; i < KEPT; i++)
            nh.insert(IDS[SRC[i]], i);
        return ORBGPU_OK;
    }
};

static int run(Table &t, bool retain, FakeOps &ops, FakeBuf &stage)
{
    if (!retain)
        return id_table_grow(t.parts(), t.rows, 16, ops);
    const int rc = id_table_replace(t.parts(), 16, ops, RetainFill{t, ops, stage});
    if (rc == ORBGPU_OK)
        t.rows = KEPT;
    return rc;
}

static int test_transaction(bool retain)
{
    // the steps of a successful run
    int n_steps = 0;
    {
        Table t;
        FakeOps ops;
        FakeBuf stage;
        if (make_table(t))
            return 1;
        g_log.clear();
        CHECK(run(t, retain, ops, stage) == ORBGPU_OK);
        for (const std::string &e : g_log)
            n_steps += e != "free";
        CHECK(n_steps == (retain ? 6 + 1 + 4 + 2 + 3 : 6 + 4 + 3 + 3));  // allocations, zeroes, the fill, two uploads and the sync
        t.release();
        stage.release();
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
        const int rc = run(t, retain, ops, stage);
        CHECK(g_countdown == 0);
        size_t failed = 0;
        while (failed < g_log.size() && g_log[failed].back() != '!')
            failed++;
        CHECK(failed < g_log.size());
        CHECK(rc == (g_log[failed] == "alloc!" ? ORBGPU_ENOMEM : ORBGPU_EHIP));
        CHECK(same(t, before));
        // after the failed step: a sync, then the frees of the new buffers (none of the table's own) and nothing else
        size_t first_free = failed + 1;
        while (first_free < g_log.size() && g_log[first_free] != "free")
            first_free++;
        CHECK(failed + 1 < g_log.size() && g_log[failed + 1] == "sync" && first_free == failed + 2);
        for (size_t i = first_free; i < g_log.size(); i++)
            CHECK(g_log[i] == "free");
        for (void *p : g_freed)
            for (int i = 0; i < N_COLS + 2; i++)
                CHECK(p != before.p[i]);
        // ... and the table still works: the same call, unfailed
        CHECK(run(t, retain, ops, stage) == ORBGPU_OK && t.cap == 16);
        t.release();
        stage.release();
    }
    // unfailed: contents carried over, every id found through the uploaded copy, the old buffers freed exactly once
    Table t;
    FakeOps ops;
    FakeBuf stage;
    if (make_table(t))
        return 1;
    const Snapshot before = snapshot(t);
    g_log.clear();
    g_freed.clear();
    CHECK(run(t, retain, ops, stage) == ORBGPU_OK);
    CHECK(t.cap == 16 && t.hash.log2cap == 5 && t.hkeys.bytes == 8u << 5 && t.hvals.bytes == 4u << 5);
    const int rows = retain ? KEPT : ROWS;
    CHECK(t.rows == rows);
    for (int c = 0; c < N_COLS; c++) {
        CHECK(t.col[c].bytes == ELT[c] * 16);
        const unsigned char *now = (const unsigned char *)t.col[c].p;
        for (int r = 0; r < 16; r++)
            for (size_t b = 0; b < ELT[c]; b++) {
                const int from = retain ? SRC[r < KEPT ? r : 0] : r;
                const unsigned char want = c < N_CARRIED && r < rows ? before.content[c][ELT[c] * (size_t)from + b] : 0;
                CHECK(now[ELT[c] * (size_t)r + b] == want);
            }
    }
    CHECK(std::memcmp(t.hkeys.p, t.hash.keys.data(), t.hkeys.bytes) == 0 && std::memcmp(t.hvals.p, t.hash.vals.data(), t.hvals.bytes) == 0);
    for (int r = 0; r < ROWS; r++) {
        int want = r;
        if (retain) {
            want = -1;
            for (int i = 0; i < KEPT; i++)
                if (SRC[i] == r)
                    want = i;
        }
        CHECK(id_hash_lookup((const int64_t *)t.hkeys.p, (const int32_t *)t.hvals.p, t.hash.log2cap, IDS[r]) == want);
        CHECK(t.hash.find(IDS[r]) == want);
    }
    CHECK(id_hash_lookup((const int64_t *)t.hkeys.p, (const int32_t *)t.hvals.p, t.hash.log2cap, 99) == -1);
    for (int i = 0; i < N_COLS + 2; i++) {
        int n = 0;
        for (void *p : g_freed)
            n += p == before.p[i];
        CHECK(n == 1);
    }
    CHECK(g_freed.size() == (size_t)N_COLS + 2);
    t.release();
    stage.release();
    return 0;
}

static int test_lock_rule()
{
    std::mutex m;
    int calls = 0;
    auto grow = [&] {  // 1 if another thread finds the lock taken while this one grows
        calls++;
        bool held = false;
        std::thread([&] { held = !m.try_lock() || (m.unlock(), false); }).join();
        return held ? 1 : 0;
    };
    CHECK(lifecycle_locked_unless(true, m, grow) == ORBGPU_OK && calls == 0);  // enough capacity: neither lock nor growth
    CHECK(lifecycle_locked_unless(false, m, grow) == 1 && calls == 1);
    CHECK(m.try_lock());  // released afterwards
    m.unlock();
    return 0;
}

int main()
{
    if (test_transaction(false) || test_transaction(true) || test_lock_rule())
        return 1;
    std::printf("id_table_test ok\n");
    return 0;
}

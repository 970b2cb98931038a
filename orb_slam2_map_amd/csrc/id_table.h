// The core of a device table keyed by a 64-bit id (MapPoint table, key-frame database): rows in per-attribute device
// arrays ("columns"), a host IdHash (id_hash.h) that hands out rows, a byte-identical device copy of it that the kernels
// probe -- and the one way such a table changes its capacity.  No HIP types here: tests/id_table_test.cpp runs the
// transaction with plain g++ over malloc-backed buffers and a recording Ops.
//
// The growth transaction (id_table_replace) replaces the columns and the hash of a table:
//   1. every new buffer is allocated at the new capacity: the columns, then hash keys and hash values;
//   2. the columns are zeroed;
//   3. the caller's `fill` writes them and builds the new host hash (growth: the first `rows` rows of the carried columns
//      device-to-device and a rebuilt copy of the hash; MapPoint retain: a compaction kernel and the kept ids);
//   4. keys and values are uploaded, and the stream is synchronised once;
//   5. only now the table is switched over: buffers swapped in, the old ones released, host hash and capacity set.
// A failure at any step synchronises the stream (nothing enqueued may still write into what is freed), releases every
// new buffer and returns the first failure's code (ORBGPU_ENOMEM: an allocation, ORBGPU_EHIP: an operation); the table is
// then bit for bit what it was -- pointers, sizes, capacity, rows, host hash.
//
// id_table_compact is the same transaction for a table whose rows own ranges of a pool (observation graph, key-frame
// database; compact_plan.h plans it): the pool columns are replaced with the rows, all or nothing.
//
// The lifecycle lock (common.h) guards what allocates and frees device memory.  A call that may grow a table takes it
// on the growing branch only (lifecycle_locked_unless); creation, which holds it already, calls the unlocked form.
#pragma once

#include "carve.h"
#include "id_hash.h"
#include "orbgpu.h"

#include <mutex>
#include <utility>
#include <vector>

namespace orbgpu {

template <typename Grow> int lifecycle_locked_unless(bool enough, std::mutex &lifecycle, Grow grow)
{
    if (enough)
        return ORBGPU_OK;
    std::lock_guard<std::mutex> lock(lifecycle);
    return grow();
}

// A column of a table: its buffer and its bytes per row.  Buf: p, bytes, int reserve(size_t) (ORBGPU_OK / ORBGPU_ENOMEM),
// release().
template <typename Buf> struct IdColumn {
    Buf *buf;
    size_t elt;
};

// What a transaction replaces.  A table names its columns once, carried ones first; columns [n_carried, n_cols) are
// scratch that needs no carry-over.
template <typename Buf> struct IdTableParts {
    const IdColumn<Buf> *cols;
    int n_carried, n_cols;
    Buf *hkeys, *hvals;
    IdHash *hash;
    int *cap;
};

// Ops: zero(p, bytes), copy(dst, src, bytes) (device to device), upload(dst, src, bytes), sync(); each enqueues on the
// table's stream and returns 0, or non-zero after leaving its message; drain() waits for the stream and reports nothing
// (the failure path: the first failure's message stays).  fill(new columns, log2cap, new hash) -> ORBGPU_*.
template <typename Buf, typename Ops, typename Fill> int id_table_replace(const IdTableParts<Buf> &t, int ncap, Ops &ops, Fill fill)
{
    const int l2 = id_hash_log2cap(ncap);
    std::vector<Buf> nb((size_t)t.n_cols + 2);
    Buf &nk = nb[(size_t)t.n_cols], &nv = nb[(size_t)t.n_cols + 1];
    IdHash nh;
    auto build = [&]() -> int {
        int rc;
        for (int i = 0; i < t.n_cols; i++)
            if ((rc = nb[(size_t)i].reserve(t.cols[i].elt * (size_t)ncap)) != ORBGPU_OK)
                return rc;
        if ((rc = nk.reserve(sizeof(int64_t) << l2)) != ORBGPU_OK || (rc = nv.reserve(sizeof(int32_t) << l2)) != ORBGPU_OK)
            return rc;
        for (int i = 0; i < t.n_cols; i++)
            if (ops.zero(nb[(size_t)i].p, t.cols[i].elt * (size_t)ncap))
                return ORBGPU_EHIP;
        if ((rc = fill(nb.data(), l2, nh)) != ORBGPU_OK)
            return rc;
        if (ops.upload(nk.p, nh.keys.data(), sizeof(int64_t) << l2) || ops.upload(nv.p, nh.vals.data(), sizeof(int32_t) << l2) ||
            ops.sync())
            return ORBGPU_EHIP;
        return ORBGPU_OK;
    };
    const int rc = build();
    if (rc != ORBGPU_OK)
        ops.drain();
    else {
        for (int i = 0; i < t.n_cols; i++)
            std::swap(*t.cols[i].buf, nb[(size_t)i]);
        std::swap(*t.hkeys, nk);
        std::swap(*t.hvals, nv);
        std::swap(*t.hash, nh);
        *t.cap = ncap;
    }
    for (Buf &b : nb)  // the new buffers of a failure, the old ones of a success
        b.release();
    return rc;
}

// Capacity `ncap` (> *t.cap), the `rows` rows in use carried over.
template <typename Buf, typename Ops> int id_table_grow(const IdTableParts<Buf> &t, int rows, int ncap, Ops &ops)
{
    return id_table_replace(t, ncap, ops, [&](const Buf *nb, int l2, IdHash &nh) {
        for (int i = 0; i < t.n_carried && rows > 0; i++)
            if (ops.copy(nb[i].p, t.cols[i].buf->p, t.cols[i].elt * (size_t)rows))
                return (int)ORBGPU_EHIP;
        nh = *t.hash;
        nh.rebuild(l2);
        return (int)ORBGPU_OK;
    });
}

// Compaction of a table whose rows own ranges of a pool (observation graph, key-frame database): the row columns and the
// hash are replaced at capacity `ncap` as above, and with them the pool columns at `pool_cap` entries.  The new pool
// buffers are allocated first; fill(new columns, new pool columns, log2cap, new hash) writes rows, pool and hash; the
// pool columns are swapped in only after the row swap has succeeded (id_table_replace has synchronised by then, so every
// copy has arrived) and released on every failure path.  A failure leaves table and pool bit for bit as they were.
template <typename Buf, typename Ops, typename Fill>
int id_table_compact(const IdTableParts<Buf> &t, int ncap, const IdColumn<Buf> *pool, int n_pool, size_t pool_cap, Ops &ops, Fill fill)
{
    std::vector<Buf> np((size_t)n_pool);
    int rc = ORBGPU_OK;
    for (int i = 0; i < n_pool && rc == ORBGPU_OK; i++)
        rc = np[(size_t)i].reserve(pool[i].elt * pool_cap);
    if (rc == ORBGPU_OK)
        rc = id_table_replace(t, ncap, ops, [&](const Buf *nb, int l2, IdHash &nh) { return fill(nb, np.data(), l2, nh); });
    if (rc == ORBGPU_OK)
        for (int i = 0; i < n_pool; i++)
            std::swap(*pool[i].buf, np[(size_t)i]);
    for (Buf &b : np)  // the new buffers of a failure, the old ones of a success
        b.release();
    return rc;
}

} // namespace orbgpu

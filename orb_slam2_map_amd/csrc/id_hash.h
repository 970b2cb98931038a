// id -> row hash of the id-keyed device tables (MapPoint table, key-frame database; id_table.h grows them).  Pure C++
// (tests/id_hash_test.cpp builds it with g++ and the sanitizers); the device kernels probe a byte-identical copy of
// `keys` / `vals` with id_hash_lookup, the function IdHash::find runs on the host.
//
// Open addressing, linear probing, capacity 2^log2cap with a load factor <= 1/2 (the owner grows it before it fills up),
// multiplicative hash.  Entries are never removed -- except the ones a refused call has just inserted, which are taken
// out again in one go (`rollback`): nothing was inserted after them, so clearing their slots cannot cut a probe chain
// that an older entry depends on.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace orbgpu {

constexpr int64_t ID_HASH_EMPTY = -1;

#if defined(__HIPCC__)
#define ORBGPU_HD __host__ __device__
#else
#define ORBGPU_HD
#endif
ORBGPU_HD inline uint32_t id_hash_slot(int64_t id, int log2cap)
{
    return (uint32_t)(((uint64_t)id * 0x9E3779B97F4A7C15ull) >> (64 - log2cap));
}

// row of `id` in a hash of capacity 2^log2cap, -1 if absent (ids are >= 0; log2cap 0: no hash yet)
ORBGPU_HD inline int id_hash_lookup(const int64_t *__restrict__ hkeys, const int32_t *__restrict__ hvals, int log2cap, int64_t id)
{
    if (id < 0 || log2cap <= 0)
        return -1;
    const uint32_t mask = (1u << log2cap) - 1u;
    uint32_t s = id_hash_slot(id, log2cap);
    for (uint32_t probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {  // (load <= 1/2: an empty slot ends every chain)
        const int64_t k = hkeys[s];
        if (k == id)
            return hvals[s];
        if (k == ID_HASH_EMPTY)
            return -1;
    }
    return -1;
}

// hash capacity for `rows` rows: the smallest l2 >= 1 with 2^l2 >= 2 * rows (load factor <= 1/2)
inline int id_hash_log2cap(int64_t rows)
{
    int l2 = 1;
    while (((int64_t)1 << l2) < 2 * rows)
        l2++;
    return l2;
}

struct IdHash {
    std::vector<int64_t> keys;  // ID_HASH_EMPTY = free slot
    std::vector<int32_t> vals;
    int log2cap = 0;

    size_t capacity() const { return keys.size(); }

    // row of `id`, -1 if absent
    int find(int64_t id) const { return id_hash_lookup(keys.data(), vals.data(), log2cap, id); }
    // slot that holds `id`, or the free slot an insertion of it would take; the table must have a free slot (load factor)
    uint32_t slot_for(int64_t id) const
    {
        const uint32_t mask = (1u << log2cap) - 1u;
        uint32_t s = id_hash_slot(id, log2cap);
        while (keys[s] != id && keys[s] != ID_HASH_EMPTY)
            s = (s + 1) & mask;
        return s;
    }
    // inserts an id that is NOT in the table (the caller has looked it up) and returns its slot
    uint32_t insert(int64_t id, int32_t row)
    {
        const uint32_t s = slot_for(id);
        keys[s] = id;
        vals[s] = row;
        return s;
    }
    // every slot empty, the capacity as it is
    void clear()
    {
        std::fill(keys.begin(), keys.end(), ID_HASH_EMPTY);
        std::fill(vals.begin(), vals.end(), -1);
    }
    // undoes the n most recent insertions (their slots, in any order)
    void rollback(const int32_t *slots, int n)
    {
        for (int k = 0; k < n; k++) {
            keys[(size_t)slots[k]] = ID_HASH_EMPTY;
            vals[(size_t)slots[k]] = -1;
        }
    }
    // capacity 2^l2 (>= twice the rows it must hold), existing entries re-inserted
    void rebuild(int l2)
    {
        std::vector<int64_t> old_keys;
        std::vector<int32_t> old_vals;
        old_keys.swap(keys);
        old_vals.swap(vals);
        log2cap = l2;
        keys.assign((size_t)1 << l2, ID_HASH_EMPTY);
        vals.assign((size_t)1 << l2, -1);
        for (size_t s = 0; s < old_keys.size(); s++)
            if (old_keys[s] != ID_HASH_EMPTY)
                insert(old_keys[s], old_vals[s]);
    }
};

} // namespace orbgpu

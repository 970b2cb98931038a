// The host-only plan of a compaction (orbgpu_covis_graph_compact, orbgpu_keyframe_db_compact): which rows of an id-keyed
// table stay, where their pool ranges go, how large the table is afterwards -- and whether there is anything to do.  No HIP
// types: tests/compact_plan_test.cpp runs it with plain g++ and the sanitizers.
//
// A table hands over, per row in add order, the length of its pool range, whether the row is kept and whether a kept row
// owns pool space afterwards (a kept bad row of the observation graph does not: C3).  The pool of both tables is
// append-only between two compactions, so the entries in use are the sum of the lengths of the rows that hold a range;
// the plan compares its own total with that number instead of asking every row where it lies.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace orbgpu {

struct CompactPlan {
    std::vector<int32_t> src;  // new row i is old row src[i]; ascending, so kept rows keep their add order
    std::vector<int64_t> off;  // new row i's range in the new pool: the exclusive prefix sum of the owned lengths, or
                               // `no_off` for a kept row that owns none
    std::vector<int32_t> len;  // entries new row i moves (0 for a row that owns none)
    int64_t pool_after = 0;    // entries in use afterwards
    int dropped = 0;
    bool needed = false;       // C6 / D4: false -- nothing is dropped and no space comes back -- means "do not touch the handle"
};

// keep / owns: one byte per row, non-zero for yes.  pool_before: the entries in use now.
inline CompactPlan compact_plan(int n, const int32_t *len, const uint8_t *keep, const uint8_t *owns, int64_t pool_before, int64_t no_off)
{
    CompactPlan p;
    for (int r = 0; r < n; r++) {
        if (!keep[r]) {
            p.dropped++;
            continue;
        }
        const bool own = owns[r] != 0;
        const int32_t l = own ? std::max(len[r], 0) : 0;
        p.src.push_back(r);
        p.off.push_back(own ? p.pool_after : no_off);
        p.len.push_back(l);
        p.pool_after += l;
    }
    p.needed = p.dropped > 0 || p.pool_after != pool_before;
    return p;
}

// C5 / D3: the capacity the doubling rules (start at `base`, double until enough) give a fresh handle that was created
// for `initial` and has since been asked for `want`.  Doubling from one base is monotone, so the two requests fold into
// their maximum.
inline int64_t compact_capacity(int64_t base, int64_t initial, int64_t want)
{
    int64_t cap = std::max<int64_t>(base, 1);
    while (cap < std::max(initial, want))
        cap *= 2;
    return cap;
}

// C1: every row that is not bad is kept; a bad row is kept if and only if a not-bad row names its id as parent.  (A
// parent value that is no row's id, or only a bad row's parent, keeps nothing.)
inline std::vector<uint8_t> compact_keep_graph(int n, const int32_t *bad, const int64_t *id, const int64_t *parent)
{
    std::vector<int64_t> named;
    for (int r = 0; r < n; r++)
        if (!bad[r] && parent[r] >= 0)
            named.push_back(parent[r]);
    std::sort(named.begin(), named.end());
    std::vector<uint8_t> keep((size_t)n, 0);
    for (int r = 0; r < n; r++)
        keep[(size_t)r] = !bad[r] || std::binary_search(named.begin(), named.end(), id[r]);
    return keep;
}

} // namespace orbgpu

// CovisibilityGraphT::Compact / KeyFrameDatabaseT::Compact (orbgpu_shim.hpp) and INTEGRATION.md's compaction block (2p,
// included as compact_block.inc) against tests/integration/compact_standin.hpp.  `run`: what needs no device -- handles
// that hold nothing answer all zeros (C6 / D4), the block's policy returns before any compaction, a null handle is
// refused.  `gpu`: the block over a graph and a database in which most key frames are bad / erased.
// tests/test_compact_shim.py builds it with -Wall -Wextra -Werror, and again with -fsanitize=address,undefined.
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "compact_standin.hpp"

#include "compact_block.inc"

using ORB_SLAM2::CovisibilityGraph;
using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::KeyFrameDatabase;

void KeyFrame::SetBadFlag() { mbBad = true; }

static_assert(sizeof(orbgpu_compact_result) == 48 && offsetof(orbgpu_compact_result, row_capacity) == 16 &&
                  offsetof(orbgpu_compact_result, slots_before) == 24 && offsetof(orbgpu_compact_result, slot_capacity) == 40,
              "orbgpu_compact_result as lib.py mirrors it");

#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            return 1;                                                          \
        }                                                                      \
    } while (0)

static bool all_zero(const orbgpu_compact_result &r)
{
    return r.compacted == 0 && r.rows_before == 0 && r.rows_after == 0 && r.rows_bad_kept == 0 && r.row_capacity == 0 &&
           r.slots_before == 0 && r.slots_after == 0 && r.slot_capacity == 0;
}

static int run()
{
    CovisibilityGraph graph(0, 2, 8);
    KeyFrameDatabase db(100, 0, 0, 2);
    REQUIRE(all_zero(graph.Compact()) && all_zero(graph.Compact()));  // never bound: no device needed
    REQUIRE(all_zero(db.Compact()));
    REQUIRE(orbgpu_covis_graph_compact(graph.handle(), nullptr) == ORBGPU_OK);  // res may be NULL
    REQUIRE(orbgpu_keyframe_db_compact(db.handle(), nullptr) == ORBGPU_OK);
    ORB_SLAM2::CompactAfterCulling(&graph, &db);  // nothing bad: the policy returns first
    REQUIRE(graph.KeyFrames() == 0 && db.size() == 0);
    bool refused = false;
    try {
        orbgpu_compact_result res;
        orbgpu_shim::check(orbgpu_covis_graph_compact(nullptr, &res), "compact");
    } catch (const std::exception &e) {
        refused = std::strstr(e.what(), "null argument") != nullptr;
    }
    REQUIRE(refused);
    REQUIRE(orbgpu_keyframe_db_compact(nullptr, nullptr) == ORBGPU_EINVAL);
    std::printf("compact shim ok\n");
    return 0;
}

static int gpu()
{
    CovisibilityGraph graph(0, 2, 8);
    KeyFrameDatabase db(100, 0, 0, 2);
    const int32_t words[3] = {1, 5, 9};
    const double vals[3] = {0.5, 0.25, 0.25};
    for (int64_t id = 1; id <= 9; id++) {
        const int64_t slots[4] = {100 + id, 101 + id, -1, 7};
        orbgpu_shim::check(orbgpu_covis_graph_add_keyframe(graph.handle(), id, 4, slots), "add_keyframe");
        orbgpu_shim::check(orbgpu_keyframe_db_add(db.handle(), id, 3, words, vals), "add");
    }
    int32_t alive = 0, bad = 0, known = 0;
    const int64_t few[3] = {2, 3, 4}, more[3] = {5, 6, 7};
    orbgpu_shim::check(orbgpu_covis_graph_set_bad(graph.handle(), 3, few, &known), "set_bad");
    orbgpu_shim::check(orbgpu_keyframe_db_erase(db.handle(), 3, few, &known), "erase");
    ORB_SLAM2::CompactAfterCulling(&graph, &db);  // 3 bad, 6 alive: the example policy waits
    orbgpu_shim::check(orbgpu_covis_graph_size(graph.handle(), &alive, &bad), "size");
    REQUIRE(alive == 6 && bad == 3);
    orbgpu_shim::check(orbgpu_covis_graph_set_bad(graph.handle(), 3, more, &known), "set_bad");
    orbgpu_shim::check(orbgpu_keyframe_db_erase(db.handle(), 3, more, &known), "erase");
    ORB_SLAM2::CompactAfterCulling(&graph, &db);  // 6 bad, 3 alive
    orbgpu_shim::check(orbgpu_covis_graph_size(graph.handle(), &alive, &bad), "size");
    REQUIRE(alive == 3 && bad == 0 && db.size() == 3);
    const orbgpu_compact_result g2 = graph.Compact(), d2 = db.Compact();
    REQUIRE(g2.compacted == 0 && g2.rows_before == 3 && g2.rows_after == 3 && g2.slots_after == 12 && g2.row_capacity == 4 &&
            g2.slot_capacity == 1024);
    REQUIRE(d2.compacted == 0 && d2.rows_before == 3 && d2.rows_after == 3 && d2.slots_after == 9 && d2.row_capacity == 4 &&
            d2.slot_capacity == 1024);
    orbgpu_shim::check(orbgpu_covis_graph_set_bad(graph.handle(), 3, few, &known), "set_bad");
    REQUIRE(known == 0);  // C2: a dropped id is an unknown id
    std::printf("compact shim ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    const bool on_gpu = argc == 2 && std::strcmp(argv[1], "gpu") == 0;
    if (argc != 2 || (std::strcmp(argv[1], "run") != 0 && !on_gpu)) {
        std::fprintf(stderr, "usage: compact_shim_test run|gpu\n");
        return 2;
    }
    try {
        return on_gpu ? gpu() : run();
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}

// CovisibilityGraphT's SetKeyPoints / Observations / KeyFrameCulling (orbgpu_shim.hpp) and INTEGRATION.md's key-frame
// culling block (2p, included as cull_block.inc) against tests/integration/cull_standin.hpp: the host-only parts -- the
// attribute packing, the marshalling, what a graph that holds nothing answers without a device -- as a stand-alone
// program.  tests/test_cull_shim.py builds it with -Wall -Wextra -Werror, and again with -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>

#include "cull_standin.hpp"

#include "cull_block.inc"

using ORB_SLAM2::CovisibilityGraph;
using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;

static std::vector<KeyFrame *> g_set_bad;
void KeyFrame::SetBadFlag()
{
    g_set_bad.push_back(this);
    if (mbNotErase)
        mbToBeErased = true;
    else
        mbBad = true;
}

#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            return 1;                                                          \
        }                                                                      \
    } while (0)

static int run()
{
    // V1's attribute byte: octave | STEREO | FAR
    std::vector<cv::KeyPoint> keys(5);
    const int octaves[5] = {0, 7, 3, 15, 40};  // (40: clamped to the last level, never into the flag bits)
    for (int i = 0; i < 5; i++)
        keys[(size_t)i].octave = octaves[i];
    const std::vector<float> uRight = {-1.f, 10.f, 0.f, 12.f, -1.f};
    const std::vector<float> depth = {-1.f, 5.f, 41.f, 40.f, -1.f};
    KeyFrame a(7, keys, uRight, depth, 40.f);
    const std::vector<uint8_t> stereo = CovisibilityGraph::KeyPointBytes(a, false);
    REQUIRE(stereo == (std::vector<uint8_t>{0x80, 0x47, 0xC3, 0x4F, 0x8F}));  // depth < 0 and depth > mThDepth are far; == is close
    const std::vector<uint8_t> mono = CovisibilityGraph::KeyPointBytes(a, true);
    REQUIRE(mono == (std::vector<uint8_t>{0x00, 0x47, 0x43, 0x4F, 0x0F}));  // LocalMapping.cc:660: no depth test
    for (uint8_t b : stereo)
        REQUIRE(!(b & 0x30));
    KeyFrame none(9, 0);
    REQUIRE(CovisibilityGraph::KeyPointBytes(none, false).empty());

    // a graph that holds nothing needs no device
    CovisibilityGraph graph(0, 2, 8);
    MapPoint p(100), bad(9);
    bad.mbBad = true;
    REQUIRE(graph.Observations({&p, nullptr, &bad, &p}) == (std::vector<int>{0, 0, 0, 0}));
    REQUIRE(graph.Observations({}).empty());
    KeyFrame b(8, 3), cur(12, 1);
    b.mbNotErase = true;
    cur.mvpOrderedConnectedKeyFrames = {&a, &b, &a};
    REQUIRE(graph.KeyFrameCulling(&cur, [](KeyFrame *k) { return k->GetNotErase(); }).empty() && g_set_bad.empty());  // all skipped
    REQUIRE(graph.KeyFrameCulling(&none, [](KeyFrame *) { return false; }).empty());  // no covisibles
    bool refused = false;
    try {
        graph.SetKeyPoints(&a, false);  // no row yet: the hook follows AddKeyFrame
    } catch (const std::exception &e) {
        refused = std::strstr(e.what(), "key frame 7 is not in the graph") != nullptr;
    }
    REQUIRE(refused);
    refused = false;
    try {
        const int64_t id = 3;
        int8_t v = 0;
        int32_t m = 0, r = 0;
        orbgpu_covis_culling_result res;
        orbgpu_shim::check(orbgpu_covis_keyframe_culling(graph.handle(), 1, &id, nullptr, 0, &v, &m, &r, 0, nullptr, &res), "culling");
    } catch (const std::exception &e) {
        refused = std::strstr(e.what(), "th_obs = 0") != nullptr;
    }
    REQUIRE(refused);

    // the block: LocalMapping::KeyFrameCulling goes through the current key frame's covisibles
    ORB_SLAM2::LocalMapping lm;
    lm.mpCovisibilityGraph = &graph;
    lm.mpCurrentKeyFrame = &cur;
    lm.KeyFrameCulling();
    REQUIRE(g_set_bad.empty() && !a.isBad() && !b.mbToBeErased);
    std::printf("cull shim ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2 || std::strcmp(argv[1], "run") != 0) {
        std::fprintf(stderr, "usage: cull_shim_test run\n");
        return 2;
    }
    try {
        return run();
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}

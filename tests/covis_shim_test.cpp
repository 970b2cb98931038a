// The host-only parts of CovisibilityGraphT (orbgpu_shim.hpp) as a stand-alone program: id <-> pointer maps, the
// marshalling of slot edits, the host half of UpdateConnections, and what a graph that holds nothing answers without a
// device.  tests/test_covis_shim.py builds it with -Wall -Wextra -Werror, and again with -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>

#include "covis_standin.hpp"

using ORB_SLAM2::CovisibilityGraph;
using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;

static std::vector<std::pair<KeyFrame *, std::pair<KeyFrame *, int>>> g_added;  // (on, (of, weight))
void KeyFrame::AddConnection(KeyFrame *pKF, const int &weight)
{
    mConnectedKeyFrameWeights[pKF] = weight;
    g_added.push_back({this, {pKF, weight}});
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
    KeyFrame a(7, 4), b(1ul << 33, 2), c(3, 0);
    MapPoint p(100), q((1ul << 40) + 5), bad(9);
    bad.mbBad = true;

    // id -> pointer: order kept, unknown ids skipped
    orbgpu_shim::IdPtrMap<KeyFrame> kfs;
    kfs.put(7, &a), kfs.put((int64_t)b.mnId, &b), kfs.put(3, &c);
    const int64_t ask[5] = {(int64_t)b.mnId, 55, 3, 7, 3};
    const std::vector<KeyFrame *> got = kfs.Resolve(ask, 5);
    REQUIRE(got.size() == 4 && got[0] == &b && got[1] == &c && got[2] == &a && got[3] == &c);
    kfs.erase(3);
    REQUIRE(kfs.Resolve(ask, 5).size() == 2 && kfs.size() == 2);

    // slots of a key frame: empty and bad points are -1
    a.mvpMapPoints = {&p, nullptr, &bad, &q};
    const std::vector<int64_t> ids = CovisibilityGraph::SlotIds(a.GetMapPointMatches());
    REQUIRE(ids.size() == 4 && ids[0] == 100 && ids[1] == -1 && ids[2] == -1 && ids[3] == (int64_t)q.mnId);
    REQUIRE(CovisibilityGraph::SlotIds(c.GetMapPointMatches()).empty());

    // a batch of edits, in order
    std::vector<int64_t> kf_ids, mp_ids;
    std::vector<int32_t> idx;
    CovisibilityGraph::MarshalSlots({{&a, 3, &q}, {&b, 1, nullptr}, {&a, 3, &p}}, kf_ids, idx, mp_ids);
    REQUIRE(kf_ids == (std::vector<int64_t>{7, (int64_t)b.mnId, 7}) && idx == (std::vector<int32_t>{3, 1, 3}));
    REQUIRE(mp_ids == (std::vector<int64_t>{(int64_t)q.mnId, -1, 100}));

    // the host half of UpdateConnections from the call's lists
    kfs.put(3, &c);
    const int64_t c_ids[4] = {3, 7, 999, (int64_t)b.mnId}, o_ids[3] = {(int64_t)b.mnId, 999, 3};
    const int32_t c_n[4] = {20, 4, 50, 31}, o_w[3] = {31, 50, 20};
    const CovisibilityGraph::Connections con = CovisibilityGraph::MakeConnections(kfs, c_ids, c_n, 4, o_ids, o_w, 3);
    REQUIRE(con.counter.size() == 3 && con.counter[0] == std::make_pair(&c, 20) && con.counter[2] == std::make_pair(&b, 31));
    REQUIRE(con.ordered == (std::vector<KeyFrame *>{&b, &c}) && con.weights == (std::vector<int>{31, 20}));
    KeyFrame cur(12, 1);
    int applied = 0;
    KeyFrame *parent = CovisibilityGraph::HostHalf(&cur, con, [&](const CovisibilityGraph::Connections &k) -> KeyFrame * {
        applied++;
        cur.mvpOrderedConnectedKeyFrames = k.ordered;
        return k.ordered.front();
    });
    REQUIRE(applied == 1 && parent == &b && g_added.size() == 2);
    REQUIRE(g_added[0].first == &b && g_added[0].second == std::make_pair(&cur, 31));
    REQUIRE(g_added[1].first == &c && g_added[1].second == std::make_pair(&cur, 20));

    // a graph that holds nothing needs no device
    CovisibilityGraph graph(0, 2, 8);
    REQUIRE(graph.KeyFrames() == 0);
    graph.SetSlots({{&a, 0, &p}, {&b, 1, &q}});  // unknown key frames: ignored
    graph.SetKeyFrameBad(&a);
    graph.SetParent(&a, &b);
    graph.SetParent(&a, nullptr);
    graph.UpdateCovisibles(&a, {&b, &c});
    ORB_SLAM2::Frame F;
    F.mnId = 77, F.N = 3, F.mvpMapPoints = {&p, &bad, nullptr};
    std::vector<KeyFrame *> local_kfs = {&a, &c};
    std::vector<MapPoint *> local_mps = {&p, &q};
    KeyFrame *ref = &c;
    graph.UpdateLocalMap(F, local_kfs, local_mps, ref);
    REQUIRE(F.mvpMapPoints[0] == &p && F.mvpMapPoints[1] == nullptr);  // Tracking.cc:1552
    REQUIRE(local_kfs.size() == 2 && local_kfs[0] == &a && ref == &c && F.mpReferenceKF == nullptr);  // :1557-1558
    REQUIRE(local_mps.empty() && a.mnTrackReferenceForFrame == 77 && c.mnTrackReferenceForFrame == 77);
    REQUIRE(!graph.UpdateConnections(&a, [](const CovisibilityGraph::Connections &) -> KeyFrame * { return nullptr; }));
    bool refused = false;
    try {
        orbgpu_covis_graph_set_covisibles(graph.handle(), 7, 11, nullptr);
        graph.SetSlots({{&a, 0, nullptr}});
        const int64_t neg = -2, kf = 7;
        const int32_t i0 = 0;
        orbgpu_shim::check(orbgpu_covis_graph_set_slots(graph.handle(), 1, &kf, &i0, &neg, nullptr), "set_slots");
    } catch (const std::exception &e) {
        refused = std::strstr(e.what(), "map point id -2") != nullptr;
    }
    REQUIRE(refused);
    graph.clear();
    std::printf("covis shim ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2 || std::strcmp(argv[1], "run") != 0) {
        std::fprintf(stderr, "usage: covis_shim_test run\n");
        return 2;
    }
    try {
        return run();
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}

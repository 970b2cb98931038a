// CovisibilityGraphT::RefreshMapPoints on the device through INTEGRATION.md's refresh block (2q, refresh_block.inc) and the
// stand-ins of tests/integration/refresh_standin.hpp: a small map built through Map::AddKeyFrame and SetSlots, refreshed
// without a table and with one.  Checked here: a case whose answer is known by hand (one observer on the z axis), that the
// two forms agree bit for bit, that the table's rows hold what the objects got, and that set_refreshed runs exactly for the
// points and the halves the status allows.  (tests/test_gpu_refresh.py compares the library with the model entry for entry.)
#include <cstdio>
#include <cstring>

#include "refresh_standin.hpp"

#include "refresh_block.inc"

using ORB_SLAM2::CovisibilityGraph;
using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;
using ORB_SLAM2::MapPointTable;

void KeyFrame::ComputePose(const cv::Mat &Tcw)
{
    for (int c = 0; c < 3; c++)  // (pure translations: Ow = -tcw)
        Ow.at<float>(c, 0) = -Tcw.ptr<float>(c)[3];
}

#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            return 1;                                                          \
        }                                                                      \
    } while (0)

struct Got {
    bool normal = false, desc = false;
};

struct RecordingAccess : ORB_SLAM2::RefreshAccess {
    void set_refreshed(MapPoint *pMP, const float *normal, float mn, float mx, const unsigned char *d)
    {
        got[pMP].normal = normal != nullptr;
        got[pMP].desc = d != nullptr;
        pMP->nSetRefreshed++;
        ORB_SLAM2::RefreshAccess::set_refreshed(pMP, normal, mn, mx, d);
    }
    std::map<MapPoint *, Got> got;
};

static void place(KeyFrame &kf, float x, float y, float z)
{
    cv::Mat Tcw(4, 4, CV_32F);
    std::memset(Tcw.data, 0, 64);
    Tcw.at<float>(0, 3) = -x, Tcw.at<float>(1, 3) = -y, Tcw.at<float>(2, 3) = -z;
    kf.SetPose(Tcw);
}

static bool same(const MapPoint &a, const MapPoint &b)
{
    return !std::memcmp(a.mNormalVector.data, b.mNormalVector.data, 12) && !std::memcmp(&a.mfMinDistance, &b.mfMinDistance, 4) &&
           !std::memcmp(&a.mfMaxDistance, &b.mfMaxDistance, 4) && !std::memcmp(a.mDescriptor.data, b.mDescriptor.data, 32);
}

static int run()
{
    CovisibilityGraph graph(0, 2, 8);
    KeyFrame::mpCovisibilityGraph = &graph;
    ORB_SLAM2::Map map;
    map.mpCovisibilityGraph = &graph;
    // four key frames of four key points; kf 30 enters first, so rows are not in id order; kf 40 stays at the origin
    KeyFrame k30(30, 4), k10(10, 4), k20(20, 4), k40(40, 4);
    KeyFrame *kfs[4] = {&k30, &k10, &k20, &k40};
    for (KeyFrame *k : kfs) {
        for (int i = 0; i < 4; i++) {
            k->mvKeysUn[(size_t)i].octave = i % 3;
            std::memset(k->mDescriptors.ptr<unsigned char>(i), (int)(k->mnId + (unsigned)i), 32);
        }
    }
    place(k30, 0.f, 0.f, 0.f);  // (before AddKeyFrame: SetPose's hook finds no row and is ignored; AddKeyFrame reads Ow)
    place(k10, 1.f, 0.f, 0.f);
    place(k20, 0.f, 1.f, 0.f);
    for (KeyFrame *k : kfs)
        map.AddKeyFrame(k);
    // two sets of the same points: one refreshed without a table, one with
    MapPoint a(1, 0.f, 0.f, 2.f), b(2, 1.f, 2.f, 3.f), c(3, 3.f, 2.f, 1.f), lonely(4, 1.f, 1.f, 1.f), far(5, 2.f, 2.f, 2.f), gone(6, 1.f, 1.f, 5.f);
    MapPoint a2(1, 0.f, 0.f, 2.f), b2(2, 1.f, 2.f, 3.f), c2(3, 3.f, 2.f, 1.f), lonely2(4, 1.f, 1.f, 1.f), far2(5, 2.f, 2.f, 2.f), gone2(6, 1.f, 1.f, 5.f);
    MapPoint *one[6] = {&a, &b, &c, &lonely, &far, &gone}, *two[6] = {&a2, &b2, &c2, &lonely2, &far2, &gone2};
    gone.mbBad = gone2.mbBad = true;
    for (MapPoint **set : {one, two}) {
        set[0]->mpRefKF = &k30;  // a: kf 30 alone, key point 0 (octave 0)
        set[1]->mpRefKF = &k10;  // b: all three with a centre
        set[2]->mpRefKF = &k40;  // c: kf 20 and kf 40, whose centre is the origin too -- every row has one
        set[3]->mpRefKF = &k30;  // lonely: observed nowhere
        set[4]->mpRefKF = &k10;  // far: observed by kf 20 only, the reference is not an observer
        set[5]->mpRefKF = &k30;
    }
    graph.SetSlots({{&k30, 0, &a}, {&k30, 1, &b}, {&k10, 2, &b}, {&k20, 0, &b}, {&k20, 1, &c}, {&k40, 3, &c}, {&k20, 2, &far}});

    RecordingAccess host;
    const std::vector<MapPoint *> first = {&gone, &b, &a, nullptr, &lonely, &c, &far, &a};
    orbgpu_covis_refresh_result res = graph.RefreshMapPoints(first, ORBGPU_REFRESH_DESCRIPTOR | ORBGPU_REFRESH_NORMAL_DEPTH, host);
    REQUIRE(res.n_no_obs == 1 && res.n_no_ref == 1 && res.n_descriptors == 4 && res.n_normals == 3 && res.max_obs == 3 && res.n_entries == 7);
    REQUIRE(host.got.size() == 4 && a.nSetRefreshed == 1 && b.nSetRefreshed == 1 && c.nSetRefreshed == 1 && far.nSetRefreshed == 1);
    REQUIRE(lonely.nSetRefreshed == 0 && gone.nSetRefreshed == 0);
    REQUIRE(host.got[&a].normal && host.got[&a].desc && host.got[&far].desc && !host.got[&far].normal);
    // a: one observer at the origin, the point on the z axis at 2, octave 0 of (1, 1.2, 1.44)
    REQUIRE(a.mNormalVector.at<float>(0, 0) == 0.f && a.mNormalVector.at<float>(1, 0) == 0.f && a.mNormalVector.at<float>(2, 0) == 1.f);
    REQUIRE(a.mfMaxDistance == 2.f && a.mfMinDistance == 2.f / 1.44f && a.mDescriptor.data[5] == 30);
    // b: the rows of kf 10, 20, 30 hold 12 = 01100b, 20 = 10100b, 31 = 11111b in every byte: distances 12-20: 64, 12-31: 96,
    // 20-31: 96, so the medians (index 1 of 3) are 64, 64 and 96 and the first minimum in id order is kf 10's row
    REQUIRE(b.mDescriptor.data[0] == 12 && b.mDescriptor.data[31] == 12);
    REQUIRE(far.mDescriptor.data[0] == 22 && far.mfMaxDistance == 0.f);

    // the same through a table: positions from its rows, results into its rows, and into the second set of objects
    MapPointTable table(0, 4);
    ORB_SLAM2::RefreshAccess acc;
    const std::vector<MapPoint *> known = {&a2, &b2, &c2, &far2, &gone2};  // lonely2 stays unknown to the table
    std::vector<cv::Mat> keep;
    table.Upsert(known, [&](MapPoint *p) { keep.push_back(p->GetWorldPos()); return keep.back().ptr<float>(); },
                 [](MapPoint *p) { return p->mNormalVector.ptr<float>(); }, [](MapPoint *p) { return p->mfMinDistance; },
                 [](MapPoint *p) { return p->mfMaxDistance; }, [](MapPoint *p) { return p->mDescriptor.ptr<unsigned char>(); });
    RecordingAccess dev;
    const std::vector<MapPoint *> second = {&far2, &lonely2, &c2, &gone2, &a2, &b2};
    res = graph.RefreshMapPoints(second, ORBGPU_REFRESH_DESCRIPTOR | ORBGPU_REFRESH_NORMAL_DEPTH, dev, &table);
    REQUIRE(res.n_unknown == 1 && res.n_bad == 0 && res.n_no_ref == 1 && res.n_descriptors == 4 && res.n_normals == 3);
    REQUIRE(dev.got.size() == 4 && lonely2.nSetRefreshed == 0 && gone2.nSetRefreshed == 0);
    for (int i = 0; i < 6; i++)
        REQUIRE(same(*one[i], *two[i]));
    for (MapPoint *p : {&a2, &b2, &c2, &far2}) {
        float nr[3], mn = -1.f, mx = -1.f;
        uint8_t ds[32];
        REQUIRE(orbgpu_mappoint_table_read(table.handle(), (int64_t)p->mnId, nullptr, nr, &mn, &mx, ds, nullptr, nullptr) == ORBGPU_OK);
        REQUIRE(!std::memcmp(nr, p->mNormalVector.data, 12) && !std::memcmp(ds, p->mDescriptor.data, 32));
        REQUIRE(!std::memcmp(&mn, &p->mfMinDistance, 4) && !std::memcmp(&mx, &p->mfMaxDistance, 4));
    }
    // each half alone; a moved key frame changes the normal through SetPose's hook
    RecordingAccess half;
    res = graph.RefreshMapPoints({&a, &far}, ORBGPU_REFRESH_NORMAL_DEPTH, half);
    REQUIRE(res.n_normals == 1 && res.n_descriptors == 0 && half.got.size() == 1 && half.got[&a].normal && !half.got[&a].desc);
    place(k30, 0.f, 0.f, 1.f);
    res = graph.RefreshMapPoints({&a}, ORBGPU_REFRESH_NORMAL_DEPTH, half);
    REQUIRE(a.mfMaxDistance == 1.f && a.mNormalVector.at<float>(2, 0) == 1.f);
    KeyFrame::mpCovisibilityGraph = nullptr;
    std::printf("refresh shim gpu ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2 || std::strcmp(argv[1], "run") != 0) {
        std::fprintf(stderr, "usage: refresh_shim_gpu_test run\n");
        return 2;
    }
    try {
        return run();
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}

// CovisibilityGraphT's SetScaleFactors / SetDescriptors / SetCentres / RefreshMapPoints (orbgpu_shim.hpp) and
// INTEGRATION.md's refresh block (2q, included as refresh_block.inc) against tests/integration/refresh_standin.hpp: the
// host-only parts -- what a graph that holds nothing answers without a device, the refusals, the setter the block adds --
// as a stand-alone program.  tests/test_refresh_shim.py builds it with -Wall -Wextra -Werror, and again with
// -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>

#include "refresh_standin.hpp"

#include "refresh_block.inc"

using ORB_SLAM2::CovisibilityGraph;
using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;

void KeyFrame::ComputePose(const cv::Mat &Tcw)
{
    for (int c = 0; c < 3; c++)  // (the test's poses are pure translations: Ow = -tcw)
        Ow.at<float>(c, 0) = -Tcw.ptr<float>(c)[3];
}

#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            return 1;                                                          \
        }                                                                      \
    } while (0)

template <typename Call> static bool refused(Call call, const char *text)
{
    try {
        call();
    } catch (const std::exception &e) {
        return std::strstr(e.what(), text) != nullptr;
    }
    return false;
}

struct CountingAccess : ORB_SLAM2::RefreshAccess {
    void set_refreshed(MapPoint *pMP, const float *normal, float mn, float mx, const unsigned char *d)
    {
        calls++;
        ORB_SLAM2::RefreshAccess::set_refreshed(pMP, normal, mn, mx, d);
    }
    int calls = 0;
};

static int run()
{
    // the setter the block adds: each half alone leaves the other as it was
    MapPoint p(100, 1.f, 2.f, 3.f), q(101, 0.f, 0.f, 2.f), bad(9, 0.f, 0.f, 1.f);
    bad.mbBad = true;
    const float normal[3] = {0.f, 0.6f, 0.8f};
    unsigned char d[32];
    std::memset(d, 0x5A, 32);
    p.SetRefreshed(normal, 1.5f, 2.5f, nullptr);
    REQUIRE(p.mNormalVector.at<float>(2, 0) == 0.8f && p.mfMinDistance == 1.5f && p.mfMaxDistance == 2.5f && p.mDescriptor.data[0] == 0);
    p.SetRefreshed(nullptr, 9.f, 9.f, d);
    REQUIRE(p.mfMinDistance == 1.5f && p.mfMaxDistance == 2.5f && p.mDescriptor.data[31] == 0x5A);

    // a graph that holds nothing needs no device: every point is NO_OBS and no setter runs
    CovisibilityGraph graph(0, 2, 8);
    KeyFrame a(7, 3);
    p.mpRefKF = &a;
    CountingAccess access;
    orbgpu_covis_refresh_result res = graph.RefreshMapPoints({&p, nullptr, &bad, &q, &p}, ORBGPU_REFRESH_DESCRIPTOR | ORBGPU_REFRESH_NORMAL_DEPTH, access);
    REQUIRE(res.n_no_obs == 2 && res.n_descriptors == 0 && res.n_normals == 0 && access.calls == 0);  // null, bad and repeated: passed over
    res = graph.RefreshMapPoints({}, ORBGPU_REFRESH_DESCRIPTOR, access);
    REQUIRE(res.n_no_obs == 0 && access.calls == 0);
    REQUIRE(refused([&] { graph.RefreshMapPoints({&p}, 0, access); }, "what = 0x0"));
    REQUIRE(refused([&] { graph.RefreshMapPoints({&p}, 4, access); }, "what = 0x4"));

    // the columns: the scale table is host memory; descriptors need a row; centres of unknown key frames are ignored
    graph.SetScaleFactors(a.mvScaleFactors);
    REQUIRE(refused([&] { graph.SetScaleFactors({}); }, "n_levels = 0"));
    REQUIRE(refused([&] { graph.SetScaleFactors({1.f, -1.f}); }, "at level 1"));
    REQUIRE(refused([&] { graph.SetDescriptors(&a, [](KeyFrame *k, size_t i) { return k->mDescriptors.ptr<unsigned char>((int)i); }); },
                    "key frame 7 is not in the graph"));
    graph.SetCentres({&a}, ORB_SLAM2::CameraCentre);
    graph.SetCentres({}, ORB_SLAM2::CameraCentre);

    // the block: KeyFrame::SetPose moves Ow and tells the graph (no row: ignored); the end of SearchInNeighbors
    KeyFrame::mpCovisibilityGraph = &graph;
    cv::Mat Tcw(4, 4, CV_32F);
    std::memset(Tcw.data, 0, 64);
    Tcw.at<float>(0, 3) = -1.f, Tcw.at<float>(1, 3) = -2.f, Tcw.at<float>(2, 3) = 4.f;
    a.SetPose(Tcw);
    float ow[3];
    ORB_SLAM2::CameraCentre(&a, ow);
    REQUIRE(ow[0] == 1.f && ow[1] == 2.f && ow[2] == -4.f);
    a.mvpMapPoints = {&p, nullptr, &bad};
    ORB_SLAM2::LocalMapping lm;
    lm.mpCovisibilityGraph = &graph;
    lm.mpCurrentKeyFrame = &a;
    lm.RefreshFusedPoints();
    REQUIRE(p.mfMinDistance == 1.5f && p.mDescriptor.data[0] == 0x5A);  // nothing observed in the graph: untouched
    KeyFrame::mpCovisibilityGraph = nullptr;
    std::printf("refresh shim ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2 || std::strcmp(argv[1], "run") != 0) {
        std::fprintf(stderr, "usage: refresh_shim_test run\n");
        return 2;
    }
    try {
        return run();
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}

// OptimizerT::OptimizeEssentialGraph (orbgpu_shim.hpp) end to end on the device over stand-in key frames and map points from
// the file of tests/test_eg_shim.py, with a MapPoint table attached.  Arguments: in.txt out.bin (format of in.txt:
// tests/integration/eg_standin.hpp).  out.bin: the orbgpu_essential_graph_result record; per key frame (all of them, in file
// order) float Tcw[16], int32 calls of SetPose; per map point float pos[3], int32 calls of UpdateNormalAndDepth; then the
// table's world_pos of every map point (float [3]).
#include <cmath>
#include <iostream>

#define ORBGPU_EG_SCENE
#include "eg_standin.hpp"

using namespace ORB_SLAM2;

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::cerr << "usage: eg_shim_gpu_test in.txt out.bin\n";
        return 2;
    }
    try {
        EgScene sc(argv[1]);
        MapPointTable table(0);
        {
            std::vector<MapPoint *> all;
            for (MapPoint &m : sc.mps)
                all.push_back(&m);
            std::vector<uint8_t> zeros(32, 0);
            table.Upsert(all, [](MapPoint *m) { return m->mWorldPos.ptr<float>(); }, [](MapPoint *m) { return m->mNormalVector.ptr<float>(); },
                         [](MapPoint *m) { return m->GetMinDistanceInvariance(); }, [](MapPoint *m) { return m->GetMaxDistanceInvariance(); },
                         [&zeros](MapPoint *) { return zeros.data(); });
        }
        orbgpu_essential_graph_result res;
        Optimizer::OptimizeEssentialGraph(&sc.map, sc.pLoopKF, sc.pCurKF, sc.NonCorrectedSim3, sc.CorrectedSim3, sc.LoopConnections,
                                          sc.bFixScale, EssentialGraphAccess(), &table, 0, &res);
        std::ofstream o(argv[2], std::ios::binary);
        auto put = [&o](const void *v, size_t n) { o.write(reinterpret_cast<const char *>(v), (std::streamsize)n); };
        auto put_i = [&put](int32_t v) { put(&v, 4); };
        put(&res, sizeof(res));
        for (KeyFrame &k : sc.kfs)
            put(k.Tcw.ptr<float>(), 64), put_i(k.nSetPose);
        for (MapPoint &m : sc.mps)
            put(m.mWorldPos.ptr<float>(), 12), put_i(m.nUpdates);
        for (MapPoint &m : sc.mps) {
            float w[3] = {NAN, NAN, NAN};
            orbgpu_shim::check(orbgpu_mappoint_table_read(table.handle(), (int64_t)m.mnId, w, NULL, NULL, NULL, NULL, NULL, NULL),
                               "orbgpu_mappoint_table_read");
            put(w, 12);
        }
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    std::cout << "eg shim ok\n";
    return 0;
}

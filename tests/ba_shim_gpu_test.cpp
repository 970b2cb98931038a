// OptimizerT::GlobalBundleAdjustemnt (orbgpu_shim.hpp) end to end on the device over stand-in key frames and map points
// from the files of tests/test_ba_shim.py, with a MapPoint table attached.  Arguments: in.bin rows.bin out.bin stop
// nLoopKF robust (formats: tests/integration/ba_standin.hpp; stop: the value of *pbStopFlag, or -1 for a null pointer).
// out.bin: the orbgpu_bundle_adjustment_result record; per key frame (all of them, in file order) float Tcw[16], float
// mTcwGBA[16] (NaN when empty), int32 mnBAGlobalForKF; per map point float pos[3], float mPosGBA[3] (NaN when empty), int32
// mnBAGlobalForKF, int32 calls of UpdateNormalAndDepth; then the table's world_pos of every map point (float [3]).
#include <cmath>
#include <iostream>

#define ORBGPU_BA_SCENE
#include "ba_standin.hpp"

using namespace ORB_SLAM2;

int main(int argc, char **argv)
{
    if (argc != 7) {
        std::cerr << "usage: ba_shim_gpu_test in.bin rows.bin out.bin stop nLoopKF robust\n";
        return 2;
    }
    try {
        BaScene sc(argv[1], argv[2]);
        const int stop_arg = atoi(argv[4]);
        bool stop = stop_arg > 0;
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
        orbgpu_bundle_adjustment_result res;
        Optimizer::GlobalBundleAdjustemnt(&sc.map, 20, stop_arg < 0 ? static_cast<bool *>(NULL) : &stop,
                                          (unsigned long)atol(argv[5]), atoi(argv[6]) != 0, FullBAAccess(), &table, 0, &res);
        std::ofstream o(argv[3], std::ios::binary);
        auto put = [&o](const void *v, size_t n) { o.write(reinterpret_cast<const char *>(v), (std::streamsize)n); };
        auto put_i = [&put](int32_t v) { put(&v, 4); };
        auto put_mat = [&put](const cv::Mat &m, int n) {
            for (int i = 0; i < n; i++) {
                const float v = m.empty() ? NAN : m.ptr<float>()[i];
                put(&v, 4);
            }
        };
        put(&res, sizeof(res));
        for (KeyFrame &k : sc.kfs)
            put_mat(k.Tcw, 16), put_mat(k.mTcwGBA, 16), put_i((int32_t)k.mnBAGlobalForKF);
        for (MapPoint &m : sc.mps)
            put_mat(m.mWorldPos, 3), put_mat(m.mPosGBA, 3), put_i((int32_t)m.mnBAGlobalForKF), put_i(m.nUpdates);
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
    std::cout << "ba shim ok\n";
    return 0;
}

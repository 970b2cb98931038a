// OptimizerT::LocalBundleAdjustment (orbgpu_shim.hpp) end to end on the device over stand-in key frames and map points from
// a file of tests/test_lba_shim.py, with a MapPoint table attached.  Arguments: in.bin out.bin stop (format of in.bin:
// tests/integration/lba_scene.hpp; stop: the value of *pbStopFlag, or -1 for a null pointer).  out.bin: the
// orbgpu_local_ba_result record; per key frame (all of them, in file order) float Tcw[16] and int32 mvpMapPoints[nkp]
// (map-point index or -1); per map point float pos[3], int32 calls of UpdateNormalAndDepth, int32 nobs and the key-frame
// indices of its observations; then the table's world_pos of every map point it knows (float [3], NaN if unknown).
#include <cmath>
#include <iostream>

#include "lba_scene.hpp"

using namespace ORB_SLAM2;

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::cerr << "usage: lba_shim_gpu_test in.bin out.bin stop\n";
        return 2;
    }
    try {
        LbaScene sc(argv[1]);
        const int stop_arg = atoi(argv[3]);
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
        orbgpu_local_ba_result res;
        Optimizer::LocalBundleAdjustment(&sc.kfs[(size_t)sc.cur], stop_arg < 0 ? static_cast<bool *>(NULL) : &stop, &sc.map,
                                         LocalBAAccess(), &table, 0, &res);
        std::ofstream o(argv[2], std::ios::binary);
        auto put = [&o](const void *v, size_t n) { o.write(reinterpret_cast<const char *>(v), (std::streamsize)n); };
        auto put_i = [&put](int32_t v) { put(&v, 4); };
        put(&res, sizeof(res));
        for (KeyFrame &k : sc.kfs) {
            put(k.Tcw.ptr<float>(), 64);
            for (MapPoint *m : k.mvpMapPoints)
                put_i(sc.mp_index(m));
        }
        for (MapPoint &m : sc.mps) {
            put(m.mWorldPos.ptr<float>(), 12);
            put_i(m.nUpdates), put_i((int32_t)m.mObservations.size());
            for (const auto &ob : m.mObservations)
                put_i(sc.kf_index(ob.first));
        }
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
    std::cout << "lba shim ok\n";
    return 0;
}

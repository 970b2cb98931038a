// The graph of OptimizerT::BundleAdjustment (orbgpu_shim.hpp: FullBAGraph) over stand-in key frames and map points from the
// files of tests/test_ba_shim.py; needs no device.  Arguments: in.bin rows.bin out.bin (formats:
// tests/integration/ba_standin.hpp).  out.bin, int32 unless named: n_poses n_points n_edges nlevels maxKFid n_iterations
// robust; rows[] (key-frame indices), points[] (map-point indices); fixed_flag[n_poses]; edge_point[], edge_pose[],
// edge_octave[]; float edge_xy[2 E], edge_ur[E], Tcw[16 P], cam[5 P], inv_sigma2[nlevels P], world_pos[3 M].
#include <iostream>

#define ORBGPU_BA_SCENE
#include "ba_standin.hpp"

using namespace ORB_SLAM2;

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::cerr << "usage: ba_shim_test in.bin rows.bin out.bin\n";
        return 2;
    }
    try {
        BaScene sc(argv[1], argv[2]);
        FullBAAccess access;
        const orbgpu_shim::FullBAGraph<KeyFrame, MapPoint> g(sc.map.GetAllKeyFrames(), sc.map.GetAllMapPoints(), access);
        const orbgpu_bundle_adjustment_problem p = g.Problem(20, false);
        std::ofstream o(argv[3], std::ios::binary);
        auto put = [&o](const void *v, size_t n) { o.write(reinterpret_cast<const char *>(v), (std::streamsize)n); };
        auto put_i = [&put](int32_t v) { put(&v, 4); };
        put_i(p.n_poses), put_i(p.n_points), put_i(p.n_edges), put_i(p.nlevels), put_i((int32_t)g.maxKFid);
        put_i(p.n_iterations), put_i(p.robust);
        for (KeyFrame *k : g.rows)
            put_i(sc.kf_index(k));
        for (MapPoint *m : g.points)
            put_i(sc.mp_index(m));
        for (int i = 0; i < p.n_poses; i++)
            put_i(p.fixed[i]);
        put(p.edge_point, 4 * (size_t)p.n_edges), put(p.edge_pose, 4 * (size_t)p.n_edges), put(p.edge_octave, 4 * (size_t)p.n_edges);
        put(p.edge_xy, 8 * (size_t)p.n_edges), put(p.edge_u_right, 4 * (size_t)p.n_edges);
        put(p.Tcw, 64 * (size_t)p.n_poses), put(p.cam, 20 * (size_t)p.n_poses);
        put(p.inv_level_sigma2, 4 * (size_t)p.nlevels * (size_t)p.n_poses), put(p.world_pos, 12 * (size_t)p.n_points);
        for (size_t e = 0; e < g.edge_kf.size(); e++)
            if (g.edge_kf[e]->isBad() || g.edge_kf[e]->mnId > g.maxKFid || g.edge_mp[e] != g.points[(size_t)g.edge_point[e]]) {
                std::cerr << "edge " << e << " should have been skipped\n";
                return 1;
            }
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    std::cout << "ba shim ok\n";
    return 0;
}

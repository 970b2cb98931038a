// The graph gathering of OptimizerT::LocalBundleAdjustment (orbgpu_shim.hpp: LocalBAGraph) over stand-in key frames and map
// points from a file of tests/test_lba_shim.py; needs no device.  Arguments: in.bin out.bin (format of in.bin:
// tests/integration/lba_scene.hpp).  out.bin, int32 unless named: n_local n_fixed n_points n_edges nlevels; local[],
// fixed[] (key-frame indices), points[] (map-point indices); fixed_flag[n_local]; edge_point[], edge_pose[], edge_octave[];
// float edge_xy[2 E], edge_ur[E], Tcw[16 P], cam[5 P], inv_sigma2[nlevels P], world_pos[3 M].
#include <iostream>

#include "lba_scene.hpp"

using namespace ORB_SLAM2;

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::cerr << "usage: lba_shim_test in.bin out.bin\n";
        return 2;
    }
    try {
        LbaScene sc(argv[1]);
        LocalBAAccess access;
        const orbgpu_shim::LocalBAGraph<KeyFrame, MapPoint> g(&sc.kfs[(size_t)sc.cur], access);
        const orbgpu_local_ba_problem p = g.Problem();
        std::ofstream o(argv[2], std::ios::binary);
        auto put = [&o](const void *v, size_t n) { o.write(reinterpret_cast<const char *>(v), (std::streamsize)n); };
        auto put_i = [&put](int32_t v) { put(&v, 4); };
        put_i(p.n_local), put_i(p.n_poses - p.n_local), put_i(p.n_points), put_i(p.n_edges), put_i(p.nlevels);
        for (KeyFrame *k : g.local)
            put_i(sc.kf_index(k));
        for (KeyFrame *k : g.fixed)
            put_i(sc.kf_index(k));
        for (MapPoint *m : g.points)
            put_i(sc.mp_index(m));
        for (uint8_t f : g.fixed_flag)
            put_i(f);
        put(p.edge_point, 4 * (size_t)p.n_edges), put(p.edge_pose, 4 * (size_t)p.n_edges), put(p.edge_octave, 4 * (size_t)p.n_edges);
        put(p.edge_xy, 8 * (size_t)p.n_edges), put(p.edge_u_right, 4 * (size_t)p.n_edges);
        put(p.Tcw, 64 * (size_t)p.n_poses), put(p.cam, 20 * (size_t)p.n_poses);
        put(p.inv_level_sigma2, 4 * (size_t)p.nlevels * (size_t)p.n_poses), put(p.world_pos, 12 * (size_t)p.n_points);
        // the marks the reference leaves behind
        const long unsigned int id = sc.kfs[(size_t)sc.cur].mnId;
        for (size_t e = 0; e < g.edge_kf.size(); e++)
            if (g.edge_mp[e]->mnBALocalForKF != id || (g.edge_kf[e]->mnBALocalForKF != id && g.edge_kf[e]->mnBAFixedForKF != id)) {
                std::cerr << "edge " << e << " joins unmarked vertices\n";
                return 1;
            }
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    std::cout << "lba shim ok\n";
    return 0;
}

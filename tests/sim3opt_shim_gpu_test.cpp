// OptimizerT::OptimizeSim3 (orbgpu_shim.hpp) end to end on the device over stand-in key frames and map points from a file
// of tests/test_sim3opt_shim.py.  Arguments: in.bin out.bin (format of in.bin: tests/integration/sim3opt_scene.hpp).
// out.bin: int32 nInliers; uint8 is_null[n1] (vpMatches1 after the call); double r[4], t[3], s of S12 after the call; the
// orbgpu_sim3_opt_result record.
#include <iostream>

#include "sim3opt_scene.hpp"

using namespace ORB_SLAM2;

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::cerr << "usage: sim3opt_shim_gpu_test in.bin out.bin\n";
        return 2;
    }
    Sim3OptScene sc(argv[1]);
    try {
        orbgpu_shim::Sim3 S12(sc.R12, sc.t12, sc.s12);
        orbgpu_sim3_opt_result res;
        const int n_inliers = Optimizer::OptimizeSim3(
            &sc.kf1, &sc.kf2, sc.matches, S12, sc.th2, sc.fix_scale != 0, [](KeyFrame *kf) { return kf->Tcw.ptr<float>(); },
            [](MapPoint *mp) { return mp->mWorldPos.ptr<float>(); }, 0, &res, sc.R12);
        std::ofstream o(argv[2], std::ios::binary);
        auto put = [&o](const void *v, size_t n) { o.write(reinterpret_cast<const char *>(v), (std::streamsize)n); };
        const int32_t ni = n_inliers;
        put(&ni, 4);
        for (MapPoint *m : sc.matches) {
            const char c = m == nullptr;
            put(&c, 1);
        }
        put(S12.r, 32), put(S12.t, 24), put(&S12.s, 8), put(&res, sizeof(res));
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    std::cout << "sim3opt shim ok\n";
    return 0;
}

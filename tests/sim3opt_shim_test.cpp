// OptimizerT::OptimizeSim3's row construction (orbgpu_shim::Sim3OptRows) and the Sim3 stand-in without a device: stand-in
// key frames and map points from a file of tests/test_sim3opt_shim.py.  Arguments: in.bin out.bin (format of in.bin:
// tests/integration/sim3opt_scene.hpp).
// out.bin: uint8 valid[n1], in_range[n1]; int32 o1[n1], o2[n1]; float x1[n1][3], x2[n1][3], k1[n1][2], k2[n1][2];
// double r[4], t[3], s of Sim3(R12, t12, s12); double R[9] of its RotationMatrix.
#include <iostream>

#include "sim3opt_scene.hpp"

using namespace ORB_SLAM2;

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::cerr << "usage: sim3opt_shim_test in.bin out.bin\n";
        return 2;
    }
    Sim3OptScene sc(argv[1]);
    const orbgpu_shim::Sim3OptRows<KeyFrame, MapPoint> rows(&sc.kf1, &sc.kf2, sc.matches,
                                                            [](MapPoint *mp) { return mp->mWorldPos.ptr<float>(); });
    std::ofstream o(argv[2], std::ios::binary);
    auto put = [&o](const void *v, size_t n) { o.write(reinterpret_cast<const char *>(v), (std::streamsize)n); };
    const size_t n = (size_t)sc.n1;
    if (rows.valid.size() != n || rows.in_range.size() != n)
        return 1;
    put(rows.valid.data(), n), put(rows.in_range.data(), n), put(rows.o1.data(), 4 * n), put(rows.o2.data(), 4 * n);
    put(rows.x1.data(), 12 * n), put(rows.x2.data(), 12 * n), put(rows.k1.data(), 8 * n), put(rows.k2.data(), 8 * n);
    const orbgpu_shim::Sim3 S(sc.R12, sc.t12, sc.s12);
    double R[9];
    S.RotationMatrix(R);
    put(S.r, 32), put(S.t, 24), put(&S.s, 8), put(R, 72);
    std::cout << "sim3opt shim ok\n";
    return 0;
}

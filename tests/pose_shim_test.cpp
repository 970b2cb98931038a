// Optimizer::PoseOptimization through the C++ shim (OptimizerT) on a stand-in Frame that carries the members the
// reference's function reads and writes.  Arguments: in.bin out.bin.  in.bin: int32 n, nlevels; float K[5] (fx fy cx cy
// mbf); float Tcw[16]; float inv_sigma2[nlevels]; per key point float x, y, u_right, int32 octave, int32 has, float
// world[3].  out.bin: int32 inliers, float Tcw[16], uint8 outlier[n] -- for tests/test_pose_shim.py to compare with
// the host entry point.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>

#include "orbgpu_shim.hpp"

struct Point2f { float x, y; };
struct KeyPoint { Point2f pt; float size, angle, response; int octave, class_id; };
struct MapPoint { unsigned long mnId; float w[3]; };

struct PoseFrame {
    int N = 0;
    std::vector<KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    float mTcw[16];
    static float fx, fy, cx, cy;
    float mbf = 0;
};
float PoseFrame::fx = 0, PoseFrame::fy = 0, PoseFrame::cx = 0, PoseFrame::cy = 0;

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::cerr << "usage: pose_shim_test in.bin out.bin\n";
        return 2;
    }
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const char *p = buf.data();
    auto take = [&p](void *dst, size_t n) { std::memcpy(dst, p, n), p += n; };
    int32_t n = 0, nl = 0;
    float K[5];
    take(&n, 4), take(&nl, 4), take(K, 20);
    PoseFrame F;
    F.N = n;
    PoseFrame::fx = K[0], PoseFrame::fy = K[1], PoseFrame::cx = K[2], PoseFrame::cy = K[3], F.mbf = K[4];
    take(F.mTcw, 64);
    F.mvInvLevelSigma2.resize(nl);
    take(F.mvInvLevelSigma2.data(), 4 * (size_t)nl);
    std::vector<MapPoint> pts(n);
    F.mvKeysUn.resize(n), F.mvuRight.resize(n), F.mvpMapPoints.assign(n, nullptr), F.mvbOutlier.assign(n, true);
    for (int i = 0; i < n; i++) {
        int32_t has = 0;
        take(&F.mvKeysUn[i].pt.x, 4), take(&F.mvKeysUn[i].pt.y, 4), take(&F.mvuRight[i], 4), take(&F.mvKeysUn[i].octave, 4);
        take(&has, 4), take(pts[i].w, 12);
        pts[i].mnId = (unsigned long)i;
        F.mvpMapPoints[i] = has ? &pts[i] : nullptr;
    }
    try {
        const int inliers = orbgpu_shim::OptimizerT<PoseFrame, MapPoint>::PoseOptimization(
            &F, [](PoseFrame &fr) { return (const float *)fr.mTcw; }, [](MapPoint *mp) { return (const float *)mp->w; },
            [](PoseFrame &fr, const float *T) { std::memcpy(fr.mTcw, T, 64); });
        std::ofstream o(argv[2], std::ios::binary);
        const int32_t ni = inliers;
        o.write(reinterpret_cast<const char *>(&ni), 4);
        o.write(reinterpret_cast<const char *>(F.mTcw), 64);
        for (int i = 0; i < n; i++) {
            const char b = F.mvbOutlier[i] ? 1 : 0;
            o.write(&b, 1);
        }
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    std::cout << "pose shim ok\n";
    return 0;
}

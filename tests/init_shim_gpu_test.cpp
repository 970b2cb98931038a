// InitializerT (orbgpu_shim.hpp) end to end on the device.  Arguments: in.bin out.bin.  in.bin: int32 n1, n2, iterations, K;
// float fx, fy, cx, cy; float kp1[n1][2]; float kp2[n2][2]; int32 matches[n1]; int32 rand[K].  out.bin: int32 returned; the
// orbgpu_init_result of the call; if returned, float R21[9], t21[3], P3D[n1][3] and n1 bytes of vbTriangulated; then the
// number of sets drawn and the sets.  For tests/test_init_shim.py.
#include <fstream>
#include <iostream>
#include <iterator>

#include "init_standin.hpp"

using namespace ORB_SLAM2;

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::cerr << "usage: init_shim_gpu_test in.bin out.bin\n";
        return 2;
    }
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const int32_t *p = reinterpret_cast<const int32_t *>(buf.data());
    const int n1 = p[0], n2 = p[1], iterations = p[2], K = p[3];
    const float *cam = reinterpret_cast<const float *>(p + 4), *kp1 = cam + 4, *kp2 = kp1 + 2 * (size_t)n1;
    const int32_t *matches = reinterpret_cast<const int32_t *>(kp2 + 2 * (size_t)n2), *rnd = matches + n1;
    Frame F1, F2;
    F1.mvKeysUn.resize(n1), F2.mvKeysUn.resize(n2);
    for (int i = 0; i < n1; i++)
        F1.mvKeysUn[i].pt.x = kp1[2 * (size_t)i], F1.mvKeysUn[i].pt.y = kp1[2 * (size_t)i + 1];
    for (int i = 0; i < n2; i++)
        F2.mvKeysUn[i].pt.x = kp2[2 * (size_t)i], F2.mvKeysUn[i].pt.y = kp2[2 * (size_t)i + 1];
    F1.fx = F2.fx = cam[0], F1.fy = F2.fy = cam[1], F1.cx = F2.cx = cam[2], F1.cy = F2.cy = cam[3];
    int at = 0;
    try {
        Initializer init(F1, 1.0f, iterations, [&](int, int) { return at < K ? rnd[at++] : 0; });
        std::ofstream o(argv[2], std::ios::binary);
        auto put = [&o](int32_t v) { o.write(reinterpret_cast<const char *>(&v), 4); };
        cv::Mat R21, t21;
        std::vector<cv::Point3f> P;
        std::vector<bool> tri;
        const bool got = init.Initialize(F2, std::vector<int>(matches, matches + n1), R21, t21, P, tri);
        put(got);
        o.write(reinterpret_cast<const char *>(&init.Result()), sizeof(orbgpu_init_result));
        if (got) {
            for (int i = 0; i < 3; i++)
                o.write(reinterpret_cast<const char *>(R21.ptr<float>(i)), 12);
            for (int i = 0; i < 3; i++)
                o.write(reinterpret_cast<const char *>(t21.ptr<float>(i)), 4);
            for (int i = 0; i < n1; i++)
                o.write(reinterpret_cast<const char *>(&P[i]), 12);
            for (int i = 0; i < n1; i++) {
                const char b = tri[i];
                o.write(&b, 1);
            }
        }
        put((int32_t)(init.Sets().size() / 8));
        for (int32_t v : init.Sets())
            put(v);
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    std::cout << "init shim ok\n";
    return 0;
}

// PnPsolverT (orbgpu_shim.hpp) end to end on the device.  Arguments: in.bin out.bin.  in.bin: int32 n1, min_inliers,
// max_iterations, chunk (0: find()), K, calls; float fx, fy, cx, cy; float sigma2[8]; int32 valid[n1]; int32 octave[n1];
// float Xw[n1][3]; float kp[n1][2]; int32 rand[K].  out.bin: int32 N, adjusted min_inliers, max_its; per call, `calls` of
// them or until bNoMore: int32 returned (1 / 0), nInliers, bNoMore, iterations and, if a pose was returned, its 16 floats and
// n1 bytes of vbInliers; then int32 -1, the number of sets drawn, and the sets.  For tests/test_pnp_shim.py.
#include <fstream>
#include <iostream>
#include <iterator>

#include "pnp_standin.hpp"

using namespace ORB_SLAM2;

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::cerr << "usage: pnp_shim_gpu_test in.bin out.bin\n";
        return 2;
    }
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const int32_t *p = reinterpret_cast<const int32_t *>(buf.data());
    const int n1 = p[0], min_inliers = p[1], max_iterations = p[2], chunk = p[3], K = p[4], calls = p[5];
    const float *cam = reinterpret_cast<const float *>(p + 6), *sigma2 = cam + 4;
    const int32_t *valid = reinterpret_cast<const int32_t *>(sigma2 + 8), *octave = valid + n1;
    const float *Xw = reinterpret_cast<const float *>(octave + n1), *kp = Xw + 3 * (size_t)n1;
    const int32_t *rnd = reinterpret_cast<const int32_t *>(kp + 2 * (size_t)n1);
    Frame F;
    F.mvKeysUn.resize(n1);
    F.mvLevelSigma2.assign(sigma2, sigma2 + 8);
    F.fx = cam[0], F.fy = cam[1], F.cx = cam[2], F.cy = cam[3];
    std::vector<MapPoint> mps(n1);
    std::vector<MapPoint *> matches(n1, nullptr);
    for (int i = 0; i < n1; i++) {
        mps[i].mWorldPos.create(3, 1, CV_32F);
        std::memcpy(mps[i].mWorldPos.data, Xw + 3 * (size_t)i, 12);
        F.mvKeysUn[i].octave = octave[i];
        F.mvKeysUn[i].pt.x = kp[2 * (size_t)i], F.mvKeysUn[i].pt.y = kp[2 * (size_t)i + 1];
        if (valid[i])
            matches[i] = &mps[i];
        else if (i % 2)
            matches[i] = &mps[i], mps[i].mbBad = true;
    }
    int at = 0;
    try {
        PnPsolver solver(
            F, matches, [](MapPoint *mp) { return mp->mWorldPos.ptr<float>(); }, [&](int, int) { return at < K ? rnd[at++] : 0; });
        solver.SetRansacParameters(0.99, min_inliers, max_iterations, 4, 0.5f, 5.991f);
        std::ofstream o(argv[2], std::ios::binary);
        auto put = [&o](int32_t v) { o.write(reinterpret_cast<const char *>(&v), 4); };
        put(solver.NumCorrespondences()), put(solver.MinInliers()), put(solver.MaxIterations());
        bool no_more = false;
        for (int call = 0; call < calls && !no_more; call++) {
            std::vector<bool> inl;
            int n_inl = 0;
            const float *T = chunk > 0 ? solver.iterate(chunk, no_more, inl, n_inl) : solver.find(inl, n_inl);
            put(T != nullptr), put(n_inl), put(no_more), put(solver.Iterations());
            if (T) {
                o.write(reinterpret_cast<const char *>(T), 64);
                for (int i = 0; i < n1; i++) {
                    const char b = (size_t)i < inl.size() && inl[i];
                    o.write(&b, 1);
                }
            }
            if (chunk == 0)
                break;
        }
        put(-1), put((int32_t)(solver.Sets().size() / 4));
        for (int32_t v : solver.Sets())
            put(v);
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    std::cout << "pnp shim ok\n";
    return 0;
}

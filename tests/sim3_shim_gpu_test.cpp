// Sim3SolverT (orbgpu_shim.hpp) end to end on the device: stand-in key frames and map points built from a scene of
// tests/sim3_model.py, the sampler over a scripted RandomInt, iterate(chunk) until bNoMore.  Arguments: in.bin out.bin.
// in.bin: int32 n1, fix_scale, min_inliers, max_iterations, chunk, K; float fx, fy, cx, cy; float T1w[16], T2w[16];
// float sigma2[8]; int32 valid[n1], octave1[n1], octave2[n1]; float Xw1[n1][3], Xw2[n1][3]; int32 rand[K].
// out.bin: int32 N, max_its; int32 triples[max_its][3]; per iterate call int32 accepted (1 / 0), nInliers, bNoMore,
// iterations and, when accepted, float T12[16], R[9], t[3], s and uint8 vbInliers[n1].
#include <fstream>
#include <iostream>
#include <iterator>

#include "sim3_standin.hpp"

using namespace ORB_SLAM2;

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::cerr << "usage: sim3_shim_gpu_test in.bin out.bin\n";
        return 2;
    }
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const char *p = buf.data();
    auto take = [&p](void *dst, size_t n) { std::memcpy(dst, p, n), p += n; };
    int32_t hd[6];
    float K[4], sigma2[8];
    take(hd, sizeof(hd)), take(K, sizeof(K));
    const int n1 = hd[0], chunk = hd[4], nrand = hd[5];
    KeyFrame kf1, kf2;
    for (KeyFrame *kf : {&kf1, &kf2}) {
        kf->Tcw.create(4, 4, CV_32F);
        take(kf->Tcw.data, 64);
        kf->fx = K[0], kf->fy = K[1], kf->cx = K[2], kf->cy = K[3];
        kf->mvKeysUn.resize(n1);
    }
    take(sigma2, sizeof(sigma2));
    kf1.mvLevelSigma2.assign(sigma2, sigma2 + 8), kf2.mvLevelSigma2 = kf1.mvLevelSigma2;
    std::vector<int32_t> valid(n1), o1(n1), o2(n1), rnd(nrand);
    take(valid.data(), 4 * (size_t)n1), take(o1.data(), 4 * (size_t)n1), take(o2.data(), 4 * (size_t)n1);
    std::vector<MapPoint> m1(n1), m2(n1);
    std::vector<MapPoint *> matched(n1, nullptr);
    kf1.mvpMapPoints.assign(n1, nullptr);
    for (std::vector<MapPoint> *ms : {&m1, &m2})
        for (int i = 0; i < n1; i++) {
            MapPoint &m = (*ms)[i];
            m.mnIndex = i;
            m.mWorldPos.create(3, 1, CV_32F);
            take(m.mWorldPos.data, 12);
        }
    take(rnd.data(), 4 * (size_t)nrand);
    for (int i = 0; i < n1; i++) {
        kf1.mvKeysUn[i].octave = o1[i], kf2.mvKeysUn[i].octave = o2[i];
        kf1.mvpMapPoints[i] = &m1[i];
        if (valid[i])
            matched[i] = &m2[i];
        else if (i % 2)
            matched[i] = &m2[i], m2[i].mbBad = true;  // dropped as bad; the others have no match
    }
    int at = 0;
    try {
        Sim3Solver solver(
            &kf1, &kf2, matched, hd[1] != 0, [](KeyFrame *kf) { return kf->Tcw.ptr<float>(); },
            [](MapPoint *mp) { return mp->mWorldPos.ptr<float>(); }, [&](int, int) { return at < nrand ? rnd[at++] : 0; });
        solver.SetRansacParameters(0.99, hd[2], hd[3]);
        std::ofstream o(argv[2], std::ios::binary);
        auto put = [&o](const void *v, size_t n) { o.write(reinterpret_cast<const char *>(v), (std::streamsize)n); };
        auto put32 = [&put](int32_t v) { put(&v, 4); };
        put32(solver.NumCorrespondences()), put32(solver.MaxIterations());
        bool no_more = false, first = true;
        for (int call = 0; call < 10000 && !no_more; call++) {
            std::vector<bool> inl;
            int n_inl = 0;
            const float *T12 = solver.iterate(chunk, no_more, inl, n_inl);
            if (first) {  // the triples exist once the first iterate has asked the library
                for (int32_t v : solver.Triples())
                    put32(v);
                for (size_t k = solver.Triples().size(); k < 3 * (size_t)solver.MaxIterations(); k++)
                    put32(0);
                first = false;
            }
            put32(T12 != nullptr), put32(n_inl), put32(no_more), put32(solver.Iterations());
            if (T12) {
                const float s = solver.GetEstimatedScale();
                put(T12, 64), put(solver.GetEstimatedRotation(), 36), put(solver.GetEstimatedTranslation(), 12), put(&s, 4);
                for (bool b : inl) {
                    const char c = b ? 1 : 0;
                    put(&c, 1);
                }
            }
        }
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    std::cout << "sim3 shim ok\n";
    return 0;
}

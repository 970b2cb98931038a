// Sim3SolverT (orbgpu_shim.hpp) without a device: the sampler replay over a scripted RandomInt and the iterate state
// machine over injected counts.  Arguments: in.bin out.bin.  in.bin: int32 n1, min_inliers, max_iterations, chunk, K;
// int32 valid[n1]; int32 rand[K] (the values RandomInt returns, in call order); int32 counts[max_its].  out.bin: int32 N,
// max_its; int32 triples[max_its][3]; then per iterate(chunk) call until bNoMore: int32 accepted (1 / 0), nInliers, bNoMore,
// iterations, popcount of vbInliers, (int32) GetEstimatedScale() -- s[h] is loaded as h, so that is the best iteration.  For tests/test_sim3_shim.py to compare with tests/sim3_model.py.
#include <fstream>
#include <iostream>
#include <iterator>

#include "sim3_standin.hpp"

using namespace ORB_SLAM2;

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::cerr << "usage: sim3_shim_test in.bin out.bin\n";
        return 2;
    }
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const int32_t *p = reinterpret_cast<const int32_t *>(buf.data());
    const int n1 = p[0], min_inliers = p[1], max_iterations = p[2], chunk = p[3], K = p[4];
    const int32_t *valid = p + 5, *rnd = valid + n1, *counts = rnd + K;
    KeyFrame kf1, kf2;
    for (KeyFrame *kf : {&kf1, &kf2}) {
        kf->mvKeysUn.resize(n1);
        kf->mvLevelSigma2.assign(8, 1.f);
        kf->Tcw.create(4, 4, CV_32F);
        for (int i = 0; i < 16; i++)
            kf->Tcw.ptr<float>()[i] = i % 5 == 0 ? 1.f : 0.f;
    }
    std::vector<MapPoint> m1(n1), m2(n1);
    std::vector<MapPoint *> matched(n1, nullptr);
    kf1.mvpMapPoints.assign(n1, nullptr);
    for (int i = 0; i < n1; i++) {
        for (MapPoint *m : {&m1[i], &m2[i]}) {
            m->mnIndex = i;
            m->mWorldPos.create(3, 1, CV_32F);
            m->mWorldPos.ptr<float>()[0] = (float)i, m->mWorldPos.ptr<float>()[1] = 1.f, m->mWorldPos.ptr<float>()[2] = 5.f;
        }
        kf1.mvpMapPoints[i] = &m1[i];
        // the four ways a row is dropped, in turn
        if (valid[i])
            matched[i] = &m2[i];
        else if (i % 4 == 0)
            matched[i] = nullptr;
        else if (i % 4 == 1)
            matched[i] = &m2[i], m2[i].mbBad = true;
        else if (i % 4 == 2)
            matched[i] = &m2[i], m1[i].mnIndex = -1;
        else
            matched[i] = &m2[i], kf1.mvpMapPoints[i] = nullptr;
    }
    int at = 0;
    std::vector<float> w(3);
    try {
        Sim3Solver solver(
            &kf1, &kf2, matched, true, [](KeyFrame *kf) { return kf->Tcw.ptr<float>(); },
            [](MapPoint *mp) { return mp->mWorldPos.ptr<float>(); }, [&](int, int) { return at < K ? rnd[at++] : 0; });
        solver.SetRansacParameters(0.99, min_inliers, max_iterations);
        const int H = solver.MaxIterations(), words = (n1 + 63) / 64;
        solver.DrawTriples();
        std::ofstream o(argv[2], std::ios::binary);
        auto put = [&o](int32_t v) { o.write(reinterpret_cast<const char *>(&v), 4); };
        put(solver.NumCorrespondences()), put(H);
        for (int32_t v : solver.Triples())
            put(v);
        // masks: hypothesis h has its first counts[h] rows set
        std::vector<uint64_t> masks((size_t)H * words, 0);
        for (int h = 0; h < H; h++)
            for (int i = 0; i < counts[h] && i < n1; i++)
                masks[(size_t)h * words + i / 64] |= 1ull << (i % 64);
        std::vector<float> R(9 * (size_t)H, 0.f), t(3 * (size_t)H, 0.f), s((size_t)H, 0.f), T(16 * (size_t)H, 0.f);
        for (int h = 0; h < H; h++)
            s[h] = (float)h;
        solver.LoadResults(counts, masks.data(), R.data(), t.data(), s.data(), T.data());
        bool no_more = false;
        for (int call = 0; call < 10000 && !no_more; call++) {
            std::vector<bool> inl;
            int n_inl = 0;
            const float *T12 = solver.iterate(chunk, no_more, inl, n_inl);
            int pop = 0;
            for (bool b : inl)
                pop += b;
            put(T12 != nullptr), put(n_inl), put(no_more), put(solver.Iterations()), put(pop);
            put((int32_t)solver.GetEstimatedScale());
        }
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    std::cout << "sim3 shim ok\n";
    return 0;
}

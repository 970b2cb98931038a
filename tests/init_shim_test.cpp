// InitializerT (orbgpu_shim.hpp) without a device: the sampler replay and what Initialize hands the library and its caller,
// with the call served from a recorded result.  Arguments: in.bin out.bin.  in.bin: int32 n1, n2, iterations, K, success;
// int32 matches[n1]; int32 rand[K].  out.bin: int32 returned, N, n_hyp handed over (or -1: no call), then the sets handed
// over; a second Initialize follows (the draw goes on in the same stream): int32 returned, then its sets.
// For tests/test_init_shim.py; the MonocularInitialization wiring of INTEGRATION.md is compiled below.
#include <fstream>
#include <iostream>
#include <iterator>

#include "init_standin.hpp"

using namespace ORB_SLAM2;

// INTEGRATION.md, Tracking::MonocularInitialization (Tracking.cc:857, 891), as written there
static bool monocular_initialization(Frame &mInitialFrame, Frame &mCurrentFrame, std::vector<int> &mvIniMatches,
                                     std::vector<cv::Point3f> &mvIniP3D, Initializer *&mpInitializer)
{
    if (!mpInitializer)
        mpInitializer = new Initializer(mInitialFrame, 1.0, 200, RandomInt);
    cv::Mat Rcw, tcw;
    std::vector<bool> vbTriangulated;
    if (mpInitializer->Initialize(mCurrentFrame, mvIniMatches, Rcw, tcw, mvIniP3D, vbTriangulated)) {
        for (size_t i = 0, iend = mvIniMatches.size(); i < iend; i++)
            if (mvIniMatches[i] >= 0 && !vbTriangulated[i])
                mvIniMatches[i] = -1;
        return true;
    }
    return false;
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::cerr << "usage: init_shim_test in.bin out.bin\n";
        return 2;
    }
    (void)&monocular_initialization;
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const int32_t *p = reinterpret_cast<const int32_t *>(buf.data());
    const int n1 = p[0], n2 = p[1], iterations = p[2], K = p[3], success = p[4];
    const int32_t *matches = p + 5, *rnd = matches + n1;
    Frame F1, F2;
    F1.mvKeysUn.resize(n1), F2.mvKeysUn.resize(n2);
    for (int i = 0; i < n1; i++)
        F1.mvKeysUn[i].pt.x = (float)i, F1.mvKeysUn[i].pt.y = (float)(2 * i);
    for (int i = 0; i < n2; i++)
        F2.mvKeysUn[i].pt.x = (float)(3 * i), F2.mvKeysUn[i].pt.y = (float)(5 * i);
    F1.fx = 500, F1.fy = 501, F1.cx = 320, F1.cy = 240;
    int at = 0;
    try {
        Initializer init(F1, 1.5f, iterations, [&](int, int) { return at < K ? rnd[at++] : 0; });
        std::ofstream o(argv[2], std::ios::binary);
        auto put = [&o](int32_t v) { o.write(reinterpret_cast<const char *>(&v), 4); };
        int handed = -1;
        std::vector<int32_t> sets;
        bool ok = true;
        init.SetSolver([&](const orbgpu_init_problem *q, float *P3D, uint8_t *tri, orbgpu_init_result *r) {
            handed = q->n_hyp;
            sets.assign(q->sets, q->sets + 8 * (size_t)q->n_hyp);
            ok = ok && q->n1 == n1 && q->n2 == n2 && q->sigma == 1.5f && q->min_parallax == 1.0f && q->min_triangulated == 50;
            ok = ok && q->fx == 500 && q->fy == 501 && q->cx == 320 && q->cy == 240;
            ok = ok && q->kp1[2] == 1.f && q->kp1[3] == 2.f && (n2 < 2 || (q->kp2[2] == 3.f && q->kp2[3] == 5.f));
            for (int i = 0; i < n1; i++)
                ok = ok && q->matches12[i] == matches[i];
            std::memset(r, 0, sizeof(*r));
            r->success = success;
            for (int e = 0; e < 9; e++)
                r->R21[e] = (float)(e + 1);
            r->t21[0] = 10, r->t21[1] = 11, r->t21[2] = 12;
            for (int i = 0; i < n1; i++)
                P3D[3 * i] = (float)i, P3D[3 * i + 1] = 0.5f, P3D[3 * i + 2] = 2.f, tri[i] = (uint8_t)(i % 3 == 0);
            return (int)ORBGPU_OK;
        });
        const std::vector<int> m12(matches, matches + n1);
        for (int call = 0; call < 2; call++) {
            cv::Mat R21, t21;
            std::vector<cv::Point3f> P;
            std::vector<bool> tri;
            handed = -1, sets.clear();
            const bool got = init.Initialize(F2, m12, R21, t21, P, tri);
            put(got);
            if (call == 0)
                put(init.NumMatches()), put(handed);
            if (got) {
                ok = ok && R21.rows == 3 && R21.cols == 3 && t21.rows == 3 && t21.cols == 1 && R21.at<float>(1, 2) == 6.f;
                ok = ok && t21.at<float>(2, 0) == 12.f && (int)P.size() == n1 && (int)tri.size() == n1;
                for (int i = 0; i < n1 && ok; i++)
                    ok = P[i].x == (float)i && P[i].z == 2.f && tri[i] == (i % 3 == 0);
            } else {
                ok = ok && R21.empty() && P.empty() && tri.empty();
            }
            for (int32_t v : sets)
                put(v);
        }
        if (!ok) {
            std::cerr << "the shim handed over or returned something else\n";
            return 1;
        }
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    std::cout << "init shim ok\n";
    return 0;
}

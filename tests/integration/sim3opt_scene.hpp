// Reads the key-frame pair the two OptimizeSim3 shim test programs run on (written by tests/test_sim3opt_shim.py):
// int32 n1, n2, fix_scale; float K[4], T1w[16], T2w[16], inv_sigma2[8], R12[9], t12[3], s12, th2;
// int32 kind[n1] (0 no match, 1 a match, 2 the match is bad, 3 KF1 has no map point there, 4 KF1's map point is bad,
// 5 the match is not seen in KF2), int32 i2[n1]; KF1 keys float xy[n1][2], int32 octave[n1]; KF2 keys float xy[n2][2],
// int32 octave[n2]; float Xw1[n1][3], Xw2[n1][3].  Test scaffolding.
#pragma once
#include <fstream>
#include <iterator>

#include "sim3opt_standin.hpp"

struct Sim3OptScene {
    int n1 = 0, n2 = 0, fix_scale = 0;
    float R12[9], t12[3], s12 = 1.f, th2 = 10.f;
    ORB_SLAM2::KeyFrame kf1, kf2;
    std::vector<ORB_SLAM2::MapPoint> m1, m2;
    std::vector<ORB_SLAM2::MapPoint *> matches;

    explicit Sim3OptScene(const char *path)
    {
        using namespace ORB_SLAM2;
        std::ifstream f(path, std::ios::binary);
        const std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        const char *p = buf.data();
        auto take = [&p](void *dst, size_t n) { std::memcpy(dst, p, n), p += n; };
        int32_t hd[3];
        float K[4], sg[8];
        take(hd, sizeof(hd)), take(K, sizeof(K));
        n1 = hd[0], n2 = hd[1], fix_scale = hd[2];
        for (KeyFrame *kf : {&kf1, &kf2}) {
            kf->Tcw.create(4, 4, CV_32F);
            take(kf->Tcw.data, 64);
            kf->fx = K[0], kf->fy = K[1], kf->cx = K[2], kf->cy = K[3];
        }
        take(sg, sizeof(sg)), take(R12, sizeof(R12)), take(t12, sizeof(t12)), take(&s12, 4), take(&th2, 4);
        kf1.mvInvLevelSigma2.assign(sg, sg + 8), kf2.mvInvLevelSigma2 = kf1.mvInvLevelSigma2;
        std::vector<int32_t> kind(n1), i2(n1);
        take(kind.data(), 4 * (size_t)n1), take(i2.data(), 4 * (size_t)n1);
        kf1.mvKeysUn.resize(n1), kf2.mvKeysUn.resize(n2);
        for (KeyFrame *kf : {&kf1, &kf2}) {
            for (cv::KeyPoint &k : kf->mvKeysUn)
                take(&k.pt, 8);
            for (cv::KeyPoint &k : kf->mvKeysUn)
                take(&k.octave, 4);
        }
        m1.resize(n1), m2.resize(n1);
        for (std::vector<MapPoint> *ms : {&m1, &m2})
            for (int i = 0; i < n1; i++) {
                (*ms)[i].mWorldPos.create(3, 1, CV_32F);
                take((*ms)[i].mWorldPos.data, 12);
            }
        kf1.mvpMapPoints.assign(n1, nullptr);
        matches.assign(n1, nullptr);
        for (int i = 0; i < n1; i++) {
            m1[i].mnIndex = i, m2[i].mnIndex = kind[i] == 5 ? -1 : i2[i];
            m1[i].mbBad = kind[i] == 4, m2[i].mbBad = kind[i] == 2;
            kf1.mvpMapPoints[i] = kind[i] == 3 ? nullptr : &m1[i];
            matches[i] = kind[i] == 0 ? nullptr : &m2[i];
        }
    }
};

// An injected map for the LocalBundleAdjustment shim tests, read from the file tests/test_lba_shim.py writes.  Little-endian
// int32 / float32:  nK nP cur;  per key frame: mnId bad nkp | fx fy cx cy mbf | Tcw[16] | nlev inv_sigma2[nlev] | ncov
// cov[ncov] (key-frame indices) | per key point: x y u_right (float) octave mp (int, map-point index or -1);  per map point:
// mnId bad | pos[3] | nobs (key-frame index, key-point index)[nobs].  Key frames live in one array, so that the pointer order
// of std::map<KeyFrame *, size_t> is the index order.
#pragma once
#include <fstream>
#include <stdexcept>
#include <string>

#include "lba_standin.hpp"

namespace ORB_SLAM2 {
// the accessors of INTEGRATION.md's LocalBundleAdjustment block
struct LocalBAAccess {
    cv::Mat pose_, pos_, normal_;
    const float *pose(KeyFrame *kf) { pose_ = kf->GetPose(); return pose_.ptr<float>(); }
    const float *world_pos(MapPoint *mp) { pos_ = mp->GetWorldPos(); return pos_.ptr<float>(); }
    const float *normal(MapPoint *mp) { normal_ = mp->GetNormal(); return normal_.ptr<float>(); }
    float min_dist(MapPoint *mp) { return mp->GetMinDistanceInvariance(); }
    float max_dist(MapPoint *mp) { return mp->GetMaxDistanceInvariance(); }
    void set_pose(KeyFrame *kf, const float *T)
    {
        cv::Mat m(4, 4, CV_32F);
        std::memcpy(m.data, T, 64);
        kf->SetPose(m);
    }
    void set_world_pos(MapPoint *mp, const float *x)
    {
        cv::Mat m(3, 1, CV_32F);
        std::memcpy(m.data, x, 12);
        mp->SetWorldPos(m);
    }
};
struct LbaScene {
    std::vector<KeyFrame> kfs;
    std::vector<MapPoint> mps;
    Map map;
    int cur = 0;

    explicit LbaScene(const char *path)
    {
        std::ifstream in(path, std::ios::binary);
        if (!in)
            throw std::runtime_error(std::string("cannot read ") + path);
        const int nK = i32(in), nP = i32(in);
        cur = i32(in);
        kfs.resize((size_t)nK), mps.resize((size_t)nP);
        for (KeyFrame &k : kfs) {
            k.mnId = (long unsigned int)i32(in), k.mbBad = i32(in) != 0;
            const int nkp = i32(in);
            k.fx = f32(in), k.fy = f32(in), k.cx = f32(in), k.cy = f32(in), k.mbf = f32(in);
            k.Tcw.create(4, 4, CV_32F);
            for (int i = 0; i < 16; i++)
                k.Tcw.ptr<float>()[i] = f32(in);
            k.mvInvLevelSigma2.resize((size_t)i32(in));
            for (float &v : k.mvInvLevelSigma2)
                v = f32(in);
            const int ncov = i32(in);
            for (int i = 0; i < ncov; i++)
                k.mvpOrderedConnectedKeyFrames.push_back(&kfs[(size_t)i32(in)]);
            k.mvKeysUn.resize((size_t)nkp), k.mvuRight.resize((size_t)nkp), k.mvpMapPoints.resize((size_t)nkp);
            for (int i = 0; i < nkp; i++) {
                k.mvKeysUn[i].pt.x = f32(in), k.mvKeysUn[i].pt.y = f32(in), k.mvuRight[i] = f32(in);
                k.mvKeysUn[i].octave = i32(in);
                const int m = i32(in);
                k.mvpMapPoints[i] = m < 0 ? static_cast<MapPoint *>(NULL) : &mps[(size_t)m];
            }
        }
        for (MapPoint &m : mps) {
            m.mnId = (long unsigned int)i32(in), m.mbBad = i32(in) != 0;
            m.mWorldPos.create(3, 1, CV_32F), m.mNormalVector.create(3, 1, CV_32F);
            for (int i = 0; i < 3; i++)
                m.mWorldPos.ptr<float>()[i] = f32(in), m.mNormalVector.ptr<float>()[i] = i == 2 ? 1.f : 0.f;
            m.mfMinDistance = 1.f, m.mfMaxDistance = 10.f;
            const int nobs = i32(in);
            for (int i = 0; i < nobs; i++) {
                const int k = i32(in), kp = i32(in);
                m.mObservations[&kfs[(size_t)k]] = (size_t)kp;
            }
        }
        if (!in)
            throw std::runtime_error("short scene file");
    }
    int kf_index(const KeyFrame *k) const { return (int)(k - kfs.data()); }
    int mp_index(const MapPoint *m) const { return m ? (int)(m - mps.data()) : -1; }

  private:
    static int i32(std::ifstream &in)
    {
        int32_t v = 0;
        in.read(reinterpret_cast<char *>(&v), 4);
        return v;
    }
    static float f32(std::ifstream &in)
    {
        float v = 0;
        in.read(reinterpret_cast<char *>(&v), 4);
        return v;
    }
};
} // namespace ORB_SLAM2

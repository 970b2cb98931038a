// The declarations INTEGRATION.md's BundleAdjustment block is written against (include/KeyFrame.h, MapPoint.h, Map.h,
// Optimizer.h), reduced to the members the block and OptimizerT::BundleAdjustment / GlobalBundleAdjustemnt touch, with the
// reference's names and types; and, for the shim tests, a map injected from the file tests/test_ba_shim.py writes (the format
// of tests/integration/lba_scene.hpp) with the rows handed in read from a second file: int32 nK, key-frame indices (vpKFs),
// nP, map-point indices (vpMP).  Test scaffolding: declarations only.
#pragma once
#include <cstdlib>
#include <fstream>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "cv_standin.hpp"
#include "orbgpu_shim.hpp"

namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint {
  public:
    bool isBad() { return mbBad; }
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    int Observations() { return (int)mObservations.size(); }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat &Pos) { mWorldPos = Pos.clone(); }
    cv::Mat GetNormal() { return mNormalVector.clone(); }
    float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
    float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
    void UpdateNormalAndDepth() { nUpdates++; }
    long unsigned int mnId = 0;
    cv::Mat mPosGBA;
    long unsigned int mnBAGlobalForKF = 0;
    bool mbBad = false;
    std::map<KeyFrame *, size_t> mObservations;
    cv::Mat mWorldPos, mNormalVector;
    float mfMinDistance = 0, mfMaxDistance = 0;
    int nUpdates = 0;  // the stand-in's own: calls of UpdateNormalAndDepth
};

class KeyFrame {
  public:
    bool isBad() { return mbBad; }
    cv::Mat GetPose() { return Tcw.clone(); }
    void SetPose(const cv::Mat &Tcw_) { Tcw = Tcw_.clone(); }
    long unsigned int mnId = 0;
    cv::Mat mTcwGBA;
    long unsigned int mnBAGlobalForKF = 0;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<MapPoint *> mvpMapPoints;
    cv::Mat Tcw;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    bool mbBad = false;
};

class Map {
  public:
    std::vector<KeyFrame *> GetAllKeyFrames() { return mspKeyFrames; }
    std::vector<MapPoint *> GetAllMapPoints() { return mspMapPoints; }
    std::vector<KeyFrame *> mspKeyFrames;  // the reference keeps sets; the tests need a stated order
    std::vector<MapPoint *> mspMapPoints;
};

// a Frame type is needed only by PoseOptimization, which these tests do not instantiate
struct Frame;
typedef orbgpu_shim::OptimizerT<Frame, MapPoint> Optimizer;
typedef orbgpu_shim::MapPointTableT<MapPoint> MapPointTable;
} // namespace ORB_SLAM2

#ifdef ORBGPU_BA_SCENE
namespace ORB_SLAM2 {
// the accessors of INTEGRATION.md's BundleAdjustment block
struct FullBAAccess {
    cv::Mat pose_, pos_, normal_;
    const float *pose(KeyFrame *kf) { pose_ = kf->GetPose(); return pose_.ptr<float>(); }
    const float *world_pos(MapPoint *mp) { pos_ = mp->GetWorldPos(); return pos_.ptr<float>(); }
    const float *normal(MapPoint *mp) { normal_ = mp->GetNormal(); return normal_.ptr<float>(); }
    float min_dist(MapPoint *mp) { return mp->GetMinDistanceInvariance(); }
    float max_dist(MapPoint *mp) { return mp->GetMaxDistanceInvariance(); }
    static cv::Mat mat(int rows, int cols, const float *v)
    {
        cv::Mat m(rows, cols, CV_32F);
        std::memcpy(m.data, v, 4 * (size_t)rows * (size_t)cols);
        return m;
    }
    void set_pose(KeyFrame *kf, const float *T) { kf->SetPose(mat(4, 4, T)); }
    void set_world_pos(MapPoint *mp, const float *x) { mp->SetWorldPos(mat(3, 1, x)); }
    void set_pose_gba(KeyFrame *kf, const float *T) { kf->mTcwGBA = mat(4, 4, T); }
    void set_world_pos_gba(MapPoint *mp, const float *x) { mp->mPosGBA = mat(3, 1, x); }
};

struct BaScene {
    std::vector<KeyFrame> kfs;
    std::vector<MapPoint> mps;
    Map map;  // vpKFs / vpMP of the rows file, in its order

    BaScene(const char *path, const char *rows_path)
    {
        std::ifstream in(path, std::ios::binary);
        if (!in)
            throw std::runtime_error(std::string("cannot read ") + path);
        const int nK = i32(in), nP = i32(in);
        (void)i32(in);  // the current key frame of the local-BA tests
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
                (void)i32(in);
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
        std::ifstream rows(rows_path, std::ios::binary);
        if (!rows)
            throw std::runtime_error(std::string("cannot read ") + rows_path);
        for (int i = 0, n = i32(rows); i < n; i++)
            map.mspKeyFrames.push_back(&kfs.at((size_t)i32(rows)));
        for (int i = 0, n = i32(rows); i < n; i++)
            map.mspMapPoints.push_back(&mps.at((size_t)i32(rows)));
        if (!rows)
            throw std::runtime_error("short rows file");
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
#endif

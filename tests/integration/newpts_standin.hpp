// The declarations INTEGRATION.md's CreateNewMapPoints block is written against (include/KeyFrame.h, MapPoint.h, Map.h,
// LocalMapping.h), reduced to the members the block and orbgpu_shim::CreateNewMapPointsT touch, with the reference's names
// and types.  Test scaffolding: declarations and recording bodies only.
#pragma once
#include <cstdlib>
#include <list>
#include <map>
#include <vector>

#include "cv_standin.hpp"
#include "orbgpu_shim.hpp"

namespace ORB_SLAM2 {
class KeyFrame;
class Map;
class MapPoint {
  public:
    MapPoint(const cv::Mat &Pos, KeyFrame *pRefKF, Map *pMap) : mWorldPos(Pos.clone()), mpRefKF(pRefKF), mpMap(pMap)
    {
        mnId = nNextId++;
    }
    void AddObservation(KeyFrame *pKF, size_t idx)
    {
        if (!mObservations.count(pKF))
            mObservations[pKF] = idx;
        order.push_back(pKF);
    }
    int Observations() { return (int)mObservations.size(); }
    bool isBad() { return false; }
    void ComputeDistinctiveDescriptors();  // records what the key frames held at that moment (below)
    void UpdateNormalAndDepth()
    {
        nUpdates++;
        float *n = mNormalVector.ptr<float>();
        n[0] = 0.25f, n[1] = -0.5f, n[2] = 0.75f;  // unlike any world position of the tests
    }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    cv::Mat GetNormal() { return mNormalVector.clone(); }
    cv::Mat GetDescriptor() { return mDescriptor.clone(); }
    float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
    float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
    long unsigned int mnId;
    inline static long unsigned int nNextId = 0;
    std::map<KeyFrame *, size_t> mObservations;
    cv::Mat mWorldPos, mNormalVector = cv::Mat(3, 1, CV_32F), mDescriptor = cv::Mat(1, 32, CV_8U);
    float mfMinDistance = 1, mfMaxDistance = 2;
    KeyFrame *mpRefKF;
    Map *mpMap;
    // the stand-in's own records
    std::vector<KeyFrame *> order;  // AddObservation calls in order
    int nUpdates = 0, nDescriptors = 0;
    bool held_at_descriptor = false;  // every observing key frame held this point when ComputeDistinctiveDescriptors ran
};

class KeyFrame {
  public:
    MapPoint *GetMapPoint(const size_t &idx) { return mvpMapPoints[idx]; }
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints[idx] = pMP; }
    cv::Mat GetPose() { return Tcw.clone(); }
    cv::Mat GetPoseInverse() { return Twc.clone(); }
    float ComputeSceneMedianDepth(const int q) { return q == 2 ? median_depth : -1.f; }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N) { return std::vector<KeyFrame *>(best.begin(), best.begin() + std::min<size_t>(best.size(), (size_t)N)); }
    long unsigned int mnId = 0;
    int N = 0;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<float> mvuRight, mvDepth, mvLevelSigma2, mvScaleFactors;
    cv::Mat mDescriptors, Tcw, Twc;
    orbgpu_shim::FeatureVector mFeatVec;
    std::vector<MapPoint *> mvpMapPoints;
    float fx = 0, fy = 0, cx = 0, cy = 0, invfx = 0, invfy = 0, mbf = 0, mb = 0, mfScaleFactor = 0;
    float median_depth = 0;  // the stand-in's own
    std::vector<KeyFrame *> best;  // the stand-in's own: the covisibility order
    cv::Mat F12;             // the stand-in's own: what ComputeF12(current, this) returns
};

inline void MapPoint::ComputeDistinctiveDescriptors()
{
    nDescriptors++;
    std::memset(mDescriptor.data, (int)(mnId & 0xff), 32);
    held_at_descriptor = true;
    for (const auto &o : mObservations)
        held_at_descriptor = held_at_descriptor && o.first->GetMapPoint(o.second) == this;
}

class Map {
  public:
    void AddMapPoint(MapPoint *pMP) { added.push_back(pMP); }
    std::vector<MapPoint *> added;
};

class LocalMapping {
  public:
    void CreateNewMapPoints();
    bool CheckNewKeyFrames() { return new_keyframes; }
    cv::Mat ComputeF12(KeyFrame *&, KeyFrame *&pKF2) { return pKF2->F12.clone(); }
    bool mbMonocular = false;
    Map *mpMap = NULL;
    KeyFrame *mpCurrentKeyFrame = NULL;
    std::list<MapPoint *> mlpRecentAddedMapPoints;
    bool new_keyframes = false;          // the stand-in's own
};

typedef orbgpu_shim::MapPointTableT<MapPoint> MapPointTable;
} // namespace ORB_SLAM2

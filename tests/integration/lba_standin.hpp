// The declarations INTEGRATION.md's LocalBundleAdjustment block is written against (include/KeyFrame.h, MapPoint.h, Map.h,
// Optimizer.h), reduced to the members the block and OptimizerT::LocalBundleAdjustment touch, with the reference's names
// and types.  Test scaffolding: declarations only.
#pragma once
#include <cstdlib>
#include <map>
#include <mutex>
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
    void EraseObservation(KeyFrame *pKF) { mObservations.erase(pKF); }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat &Pos) { mWorldPos = Pos.clone(); }
    cv::Mat GetNormal() { return mNormalVector.clone(); }
    float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
    float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
    void UpdateNormalAndDepth() { nUpdates++; }
    long unsigned int mnId = 0;
    long unsigned int mnBALocalForKF = 0;
    bool mbBad = false;
    std::map<KeyFrame *, size_t> mObservations;
    cv::Mat mWorldPos, mNormalVector;
    float mfMinDistance = 0, mfMaxDistance = 0;
    int nUpdates = 0;  // the stand-in's own: calls of UpdateNormalAndDepth
};

class KeyFrame {
  public:
    std::vector<KeyFrame *> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    bool isBad() { return mbBad; }
    cv::Mat GetPose() { return Tcw.clone(); }
    void SetPose(const cv::Mat &Tcw_) { Tcw = Tcw_.clone(); }
    void EraseMapPointMatch(MapPoint *pMP)
    {
        for (MapPoint *&p : mvpMapPoints)
            if (p == pMP)
                p = static_cast<MapPoint *>(NULL);
    }
    long unsigned int mnId = 0;
    long unsigned int mnBALocalForKF = 0, mnBAFixedForKF = 0;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    cv::Mat Tcw;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    bool mbBad = false;
};

class Map {
  public:
    std::mutex mMutexMapUpdate;
};

// a Frame type is needed only by PoseOptimization, which these tests do not instantiate
struct Frame;
typedef orbgpu_shim::OptimizerT<Frame, MapPoint> Optimizer;
typedef orbgpu_shim::MapPointTableT<MapPoint> MapPointTable;
} // namespace ORB_SLAM2

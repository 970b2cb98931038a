// The declarations INTEGRATION.md's OptimizeSim3 block is written against (include/KeyFrame.h, MapPoint.h, Optimizer.h),
// reduced to the members the block and OptimizerT::OptimizeSim3 touch, with the reference's names and types.
// Test scaffolding: declarations only.
#pragma once
#include <cstdlib>
#include <vector>

#include "cv_standin.hpp"
#include "orbgpu_shim.hpp"

namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint {
  public:
    bool isBad() { return mbBad; }
    int GetIndexInKeyFrame(KeyFrame *pKF) { return pKF ? mnIndex : -1; }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    bool mbBad = false;
    int mnIndex = -1;
    cv::Mat mWorldPos;
};

class KeyFrame {
  public:
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    cv::Mat GetPose() { return Tcw.clone(); }
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvInvLevelSigma2;
    std::vector<MapPoint *> mvpMapPoints;
    cv::Mat Tcw;
    float fx = 0, fy = 0, cx = 0, cy = 0;
};

// a Frame type is needed only by PoseOptimization, which these tests do not instantiate
struct Frame;
typedef orbgpu_shim::OptimizerT<Frame, MapPoint> Optimizer;
} // namespace ORB_SLAM2

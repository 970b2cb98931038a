// The declarations INTEGRATION.md's pose-optimisation block is written against (include/Optimizer.h:52, Frame.h,
// MapPoint.h), reduced to the members the block and OptimizerT touch, with the reference's names and types.
// Test scaffolding: declarations only.  Separate from ref_standin.hpp, whose Frame has no SetPose / mvInvLevelSigma2.
#pragma once
#include <vector>

#include "cv_standin.hpp"
#include "orbgpu_shim.hpp"

namespace ORB_SLAM2 {
class MapPoint {
  public:
    long unsigned int mnId = 0;
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    cv::Mat mWorldPos;
};

class Frame {
  public:
    int N = 0;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    cv::Mat mTcw;
    void SetPose(cv::Mat Tcw) { mTcw = Tcw.clone(); }
    static float fx, fy, cx, cy;
    float mbf = 0;
    // what INTEGRATION.md section 2b adds to Frame for the device-resident path
    orbgpu_shim::DeviceFrameT<Frame> *mpDeviceFrame = nullptr;
};

class Optimizer {
  public:
    int static PoseOptimization(Frame *pFrame);
};

extern orbgpu_shim::MapPointTableT<MapPoint> *gpMapPointTable;  // the table of section 2b'
} // namespace ORB_SLAM2

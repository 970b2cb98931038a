// The declarations INTEGRATION.md's Relocalization block is written against (include/Frame.h, MapPoint.h, PnPsolver.h),
// reduced to the members the block and PnPsolverT touch, with the reference's names and types.
// Test scaffolding: declarations only.
#pragma once
#include <cstdlib>
#include <vector>

#include "cv_standin.hpp"
#include "orbgpu_shim.hpp"

namespace ORB_SLAM2 {
class MapPoint {
  public:
    bool isBad() { return mbBad; }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    bool mbBad = false;
    cv::Mat mWorldPos;
};

class Frame {
  public:
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvLevelSigma2;
    std::vector<MapPoint *> mvpMapPoints;
    float fx = 0, fy = 0, cx = 0, cy = 0;
};

typedef orbgpu_shim::PnPsolverT<Frame, MapPoint> PnPsolver;
} // namespace ORB_SLAM2

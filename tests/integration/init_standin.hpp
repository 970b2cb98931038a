// The declarations INTEGRATION.md's MonocularInitialization block is written against (include/Frame.h, Initializer.h),
// reduced to the members the block and InitializerT touch, with the reference's names and types.
// Test scaffolding: declarations only.
#pragma once
#include <cstdlib>
#include <vector>

#include "cv_standin.hpp"
#include "orbgpu_shim.hpp"

namespace cv {
struct Point3f { float x = 0, y = 0, z = 0; };
} // namespace cv

namespace ORB_SLAM2 {
class Frame {
  public:
    std::vector<cv::KeyPoint> mvKeysUn;
    float fx = 0, fy = 0, cx = 0, cy = 0;
};

typedef orbgpu_shim::InitializerT<Frame> Initializer;

// stands for DUtils::Random::RandomInt
inline int RandomInt(int min, int max) { return min + std::rand() % (max - min + 1); }
} // namespace ORB_SLAM2

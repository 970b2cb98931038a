// The declarations INTEGRATION.md's compaction block (section 2p, second block) is written against: cull_standin.hpp's, and
// the key-frame database beside the observation graph.  Test scaffolding: declarations only.
#pragma once
#include "cull_standin.hpp"

namespace ORB_SLAM2 {
typedef orbgpu_shim::KeyFrameDatabaseT<KeyFrame> KeyFrameDatabase;
} // namespace ORB_SLAM2

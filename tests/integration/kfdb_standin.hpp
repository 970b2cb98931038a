// The declarations INTEGRATION.md's KeyFrameDatabase block is written against (include/KeyFrame.h, Frame.h,
// KeyFrameDatabase.h), reduced to the members the block and KeyFrameDatabaseT touch, with the reference's names and types.
// Test scaffolding: declarations only.
#pragma once
#include <mutex>
#include <set>
#include <vector>

#include "orbgpu_shim.hpp"

namespace DBoW2 {
typedef orbgpu_shim::BowVector BowVector;  // std::map<WordId, WordValue> (BowVector.h:59)
}

namespace ORB_SLAM2 {
class KeyFrame;
typedef orbgpu_shim::KeyFrameDatabaseT<KeyFrame> KeyFrameDatabase;

class Frame {
  public:
    DBoW2::BowVector mBowVec;
};

class KeyFrame {
  public:
    // every reader of the covisibility vectors takes mMutexConnections, as in KeyFrame.cc:197-217: a hook that calls one
    // of them from inside UpdateBestCovisibles (which holds it) does not return
    std::set<KeyFrame *> GetConnectedKeyFrames()
    {
        std::unique_lock<std::mutex> lock(mMutexConnections);
        return std::set<KeyFrame *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.end());
    }
    std::vector<KeyFrame *> GetVectorCovisibleKeyFrames()
    {
        std::unique_lock<std::mutex> lock(mMutexConnections);
        return mvpOrderedConnectedKeyFrames;
    }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N)
    {
        std::unique_lock<std::mutex> lock(mMutexConnections);
        if ((int)mvpOrderedConnectedKeyFrames.size() < N)
            return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    void UpdateBestCovisibles();
    void SetBadFlag();
    bool isBad() { return mbBad; }
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    bool mbBad = false;
    std::mutex mMutexConnections;
    KeyFrameDatabase *mpKeyFrameDB = nullptr;
};
} // namespace ORB_SLAM2

// The declarations INTEGRATION.md's key-frame culling block (section 2p) is written against (include/LocalMapping.h,
// KeyFrame.h, MapPoint.h, Map.h, and cv::KeyPoint), reduced to the members the block and CovisibilityGraphT's SetKeyPoints /
// Observations / KeyFrameCulling touch, with the reference's names and types.  Test scaffolding: declarations and trivial
// accessors only; what the block does not define, the test program does.
#pragma once
#include <map>
#include <mutex>
#include <set>
#include <vector>

#include "orbgpu_shim.hpp"

namespace cv {
struct KeyPoint {
    float x = 0, y = 0, size = 0, angle = -1, response = 0;
    int octave = 0, class_id = -1;
};
} // namespace cv

namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint;
typedef orbgpu_shim::CovisibilityGraphT<KeyFrame, MapPoint> CovisibilityGraph;

class MapPoint {
  public:
    explicit MapPoint(long unsigned int id) : mnId(id) {}
    bool isBad() { return mbBad; }
    int Observations() { return nObs; }
    long unsigned int mnId;
    long unsigned int mnTrackReferenceForFrame = 0;
    int nObs = 0;
    bool mbBad = false;
};

class KeyFrame {
  public:
    KeyFrame(long unsigned int id, int n)
        : mnId(id), N(n), mvKeysUn((size_t)n), mvuRight((size_t)n, -1.f), mvDepth((size_t)n, -1.f), mThDepth(40.f),
          mvpMapPoints((size_t)n, nullptr)
    {
    }
    KeyFrame(long unsigned int id, const std::vector<cv::KeyPoint> &keys, const std::vector<float> &uRight,
             const std::vector<float> &depth, float thDepth)
        : mnId(id), N((int)keys.size()), mvKeysUn(keys), mvuRight(uRight), mvDepth(depth), mThDepth(thDepth),
          mvpMapPoints(keys.size(), nullptr)
    {
    }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    MapPoint *GetMapPoint(const size_t &idx) { return mvpMapPoints[idx]; }
    void AddConnection(KeyFrame *pKF, const int &weight) { mConnectedKeyFrameWeights[pKF] = weight; }
    std::vector<KeyFrame *> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    bool GetNotErase();  // the block adds it: mbNotErase has no reader in the reference
    void SetBadFlag();
    bool isBad() { return mbBad; }
    long unsigned int mnId;
    const int N;
    long unsigned int mnTrackReferenceForFrame = 0;
    const std::vector<cv::KeyPoint> mvKeysUn;
    const std::vector<float> mvuRight;
    const std::vector<float> mvDepth;
    const float mThDepth;
    std::vector<MapPoint *> mvpMapPoints;
    std::map<KeyFrame *, int> mConnectedKeyFrameWeights;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    bool mbNotErase = false;
    bool mbToBeErased = false;
    bool mbBad = false;
    std::mutex mMutexConnections;
    static inline CovisibilityGraph *mpCovisibilityGraph = nullptr;
};

class Map {
  public:
    void AddKeyFrame(KeyFrame *pKF);
    std::set<KeyFrame *> mspKeyFrames;
    long unsigned int mnMaxKFid = 0;
    std::mutex mMutexMap;
    CovisibilityGraph *mpCovisibilityGraph = nullptr;
    bool mbMonocular = false;  // the integration adds it beside mpCovisibilityGraph: mSensor == System::MONOCULAR
};

class LocalMapping {
  public:
    void KeyFrameCulling();
    KeyFrame *mpCurrentKeyFrame = nullptr;
    bool mbMonocular = false;
    CovisibilityGraph *mpCovisibilityGraph = nullptr;
};
} // namespace ORB_SLAM2

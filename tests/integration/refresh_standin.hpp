// The declarations INTEGRATION.md's refresh block (section 2q) is written against (include/LocalMapping.h, KeyFrame.h,
// MapPoint.h, Map.h and the cv types of cv_standin.hpp), reduced to the members the block and CovisibilityGraphT's
// SetScaleFactors / SetDescriptors / SetCentres / RefreshMapPoints touch, with the reference's names and types.  Test
// scaffolding: declarations and trivial accessors only; what the block does not define, the test program does.
#pragma once
#include <map>
#include <mutex>
#include <set>
#include <vector>

#include "cv_standin.hpp"
#include "orbgpu_shim.hpp"

namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint;
typedef orbgpu_shim::CovisibilityGraphT<KeyFrame, MapPoint> CovisibilityGraph;
typedef orbgpu_shim::MapPointTableT<MapPoint> MapPointTable;

class MapPoint {
  public:
    MapPoint(long unsigned int id, float x, float y, float z) : mnId(id), mWorldPos(3, 1, CV_32F), mNormalVector(3, 1, CV_32F), mDescriptor(1, 32, CV_8U)
    {
        mWorldPos.at<float>(0, 0) = x, mWorldPos.at<float>(1, 0) = y, mWorldPos.at<float>(2, 0) = z;
        std::memset(mNormalVector.data, 0, 12);
        std::memset(mDescriptor.data, 0, 32);
    }
    bool isBad() { return mbBad; }
    int Observations() { return nObs; }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    KeyFrame *GetReferenceKeyFrame() { return mpRefKF; }
    void SetRefreshed(const float *normal, float minDistance, float maxDistance, const unsigned char *descriptor);  // the block adds it
    long unsigned int mnId;
    long unsigned int mnTrackReferenceForFrame = 0;
    int nObs = 0;
    bool mbBad = false;
    cv::Mat mWorldPos, mNormalVector, mDescriptor;
    float mfMinDistance = 0, mfMaxDistance = 0;
    KeyFrame *mpRefKF = nullptr;
    std::mutex mMutexPos, mMutexFeatures;
    int nSetRefreshed = 0;  // (the test counts the calls)
};

class KeyFrame {
  public:
    KeyFrame(long unsigned int id, int n)
        : mnId(id), N(n), mvKeysUn((size_t)n), mvuRight((size_t)n, -1.f), mvDepth((size_t)n, -1.f), mThDepth(40.f),
          mDescriptors(n, 32, CV_8U), mvScaleFactors{1.0f, 1.2f, 1.44f}, mvpMapPoints((size_t)n, nullptr), Ow(3, 1, CV_32F)
    {
        std::memset(mDescriptors.data, 0, 32 * (size_t)n);
        std::memset(Ow.data, 0, 12);
    }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    MapPoint *GetMapPoint(const size_t &idx) { return mvpMapPoints[idx]; }
    void AddConnection(KeyFrame *pKF, const int &weight) { mConnectedKeyFrameWeights[pKF] = weight; }
    cv::Mat GetCameraCenter()
    {
        std::unique_lock<std::mutex> lock(mMutexPose);
        return Ow.clone();
    }
    void SetPose(const cv::Mat &Tcw);
    void ComputePose(const cv::Mat &Tcw);  // stands for the statements of KeyFrame.cc:61-72 (Tcw, Twc, Ow, Cw)
    bool isBad() { return mbBad; }
    long unsigned int mnId;
    const int N;
    long unsigned int mnTrackReferenceForFrame = 0;
    std::vector<cv::KeyPoint> mvKeysUn;  // (const in the reference; the test sets octaves after construction)
    const std::vector<float> mvuRight;
    const std::vector<float> mvDepth;
    const float mThDepth;
    cv::Mat mDescriptors;
    const std::vector<float> mvScaleFactors;
    std::vector<MapPoint *> mvpMapPoints;
    std::map<KeyFrame *, int> mConnectedKeyFrameWeights;
    cv::Mat Ow;
    bool mbBad = false;
    std::mutex mMutexPose;
    static inline CovisibilityGraph *mpCovisibilityGraph = nullptr;
};

class Map {
  public:
    void AddKeyFrame(KeyFrame *pKF);
    std::set<KeyFrame *> mspKeyFrames;
    long unsigned int mnMaxKFid = 0;
    std::mutex mMutexMap;
    CovisibilityGraph *mpCovisibilityGraph = nullptr;
    bool mbMonocular = false;
};

class LocalMapping {
  public:
    void RefreshFusedPoints();  // LocalMapping.cc:546-557, the end of SearchInNeighbors
    KeyFrame *mpCurrentKeyFrame = nullptr;
    CovisibilityGraph *mpCovisibilityGraph = nullptr;
    MapPointTable *mpMapPointTable = nullptr;  // may be null: the host form
};
} // namespace ORB_SLAM2

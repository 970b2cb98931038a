// The declarations INTEGRATION.md's observation-graph block (section 2o) is written against (include/Tracking.h, Frame.h,
// KeyFrame.h, MapPoint.h, Map.h), reduced to the members the block and CovisibilityGraphT touch, with the reference's
// names and types.  Test scaffolding: declarations and trivial accessors only; what the block does not define, the test
// programs do.
#pragma once
#include <map>
#include <mutex>
#include <set>
#include <vector>

#include "orbgpu_shim.hpp"

namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint;
typedef orbgpu_shim::CovisibilityGraphT<KeyFrame, MapPoint> CovisibilityGraph;

class MapPoint {
  public:
    explicit MapPoint(long unsigned int id) : mnId(id) {}
    void AddObservation(KeyFrame *pKF, size_t idx);
    void SetBadFlag();
    bool isBad() { return mbBad; }
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    long unsigned int mnId;
    long unsigned int mnTrackReferenceForFrame = 0;
    std::map<KeyFrame *, size_t> mObservations;
    int nObs = 0;
    bool mbBad = false;
    std::mutex mMutexFeatures;
    static inline CovisibilityGraph *mpCovisibilityGraph = nullptr;
};

class KeyFrame {
  public:
    KeyFrame(long unsigned int id, int n) : mnId(id), N(n), mvpMapPoints((size_t)n, nullptr) {}
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    MapPoint *GetMapPoint(const size_t &idx) { return mvpMapPoints[idx]; }
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints[idx] = pMP; }
    void EraseMapPointMatch(const size_t &idx) { mvpMapPoints[idx] = nullptr; }
    void AddConnection(KeyFrame *pKF, const int &weight);
    void UpdateBestCovisibles();
    void UpdateConnections();
    void AddChild(KeyFrame *pKF) { mspChildrens.insert(pKF); }
    void ChangeParent(KeyFrame *pKF);
    void SetBadFlag();
    bool isBad() { return mbBad; }
    long unsigned int mnId;
    const int N;
    long unsigned int mnTrackReferenceForFrame = 0;
    std::vector<MapPoint *> mvpMapPoints;
    std::map<KeyFrame *, int> mConnectedKeyFrameWeights;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    std::vector<int> mvOrderedWeights;
    bool mbFirstConnection = true;
    KeyFrame *mpParent = nullptr;
    std::set<KeyFrame *> mspChildrens;
    bool mbBad = false;
    std::mutex mMutexConnections;
    static inline CovisibilityGraph *mpCovisibilityGraph = nullptr;
};

class Frame {
  public:
    long unsigned int mnId = 0;
    int N = 0;
    std::vector<MapPoint *> mvpMapPoints;
    KeyFrame *mpReferenceKF = nullptr;
};

class Map {
  public:
    void SetReferenceMapPoints(const std::vector<MapPoint *> &vpMPs) { mvpReferenceMapPoints = vpMPs; }
    std::vector<MapPoint *> mvpReferenceMapPoints;
};

class Tracking {
  public:
    void UpdateLocalMap();
    Frame mCurrentFrame;
    KeyFrame *mpReferenceKF = nullptr;
    std::vector<KeyFrame *> mvpLocalKeyFrames;
    std::vector<MapPoint *> mvpLocalMapPoints;
    Map *mpMap = nullptr;
    CovisibilityGraph *mpCovisibilityGraph = nullptr;
};
} // namespace ORB_SLAM2

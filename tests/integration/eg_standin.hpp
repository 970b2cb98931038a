// The declarations INTEGRATION.md's OptimizeEssentialGraph block is written against (include/KeyFrame.h, MapPoint.h, Map.h,
// LoopClosing.h, Optimizer.h), reduced to the members the block and OptimizerT::OptimizeEssentialGraph touch, with the
// reference's names and types; and, for the shim tests, a map injected from the text file tests/test_eg_shim.py writes:
//     nK nP
//     per key frame: mnId bad parent(-1: none)  16 floats of Tcw  nChildren idx..  nLoopEdges idx..  nCov (idx weight)..
//                    (the covisibles in the order GetCovisiblesByWeight returns them: by weight, descending)
//     per map point: mnId bad refKF(-1: none) mnCorrectedByKF mnCorrectedReference  3 floats
//     pCurKF pLoopKF bFixScale
//     nNonCorrected (idx 8 doubles)..   nCorrected (idx 8 doubles)..   nLoopConnections (idx n idx..)..
// idx is a position in the file; floats and doubles are C99 hex literals.  Test scaffolding: declarations only.
#pragma once
#include <cstdlib>
#include <fstream>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "cv_standin.hpp"
#include "orbgpu_shim.hpp"

namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint {
  public:
    bool isBad() { return mbBad; }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat &Pos) { mWorldPos = Pos.clone(); }
    cv::Mat GetNormal() { return mNormalVector.clone(); }
    float GetMinDistanceInvariance() { return 0.8f; }
    float GetMaxDistanceInvariance() { return 12.f; }
    KeyFrame *GetReferenceKeyFrame() { return mpRefKF; }
    int Observations() { return 2; }
    void UpdateNormalAndDepth() { nUpdates++; }
    long unsigned int mnId = 0;
    long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;
    bool mbBad = false;
    KeyFrame *mpRefKF = nullptr;
    cv::Mat mWorldPos, mNormalVector;
    int nUpdates = 0;  // the stand-in's own: calls of UpdateNormalAndDepth
};

class KeyFrame {
  public:
    bool isBad() { return mbBad; }
    cv::Mat GetPose() { return Tcw.clone(); }
    void SetPose(const cv::Mat &Tcw_) { Tcw = Tcw_.clone(), nSetPose++; }
    KeyFrame *GetParent() { return mpParent; }
    bool hasChild(KeyFrame *pKF) { return mspChildrens.count(pKF) != 0; }
    std::set<KeyFrame *> GetLoopEdges() { return mspLoopEdges; }
    int GetWeight(KeyFrame *pKF) { return mConnectedKeyFrameWeights.count(pKF) ? mConnectedKeyFrameWeights[pKF] : 0; }
    std::vector<KeyFrame *> GetCovisiblesByWeight(const int &w)
    {
        std::vector<KeyFrame *> out;
        for (size_t i = 0; i < mvpOrderedConnectedKeyFrames.size(); i++)
            if (mvOrderedWeights[i] >= w)
                out.push_back(mvpOrderedConnectedKeyFrames[i]);
        return out;
    }
    long unsigned int mnId = 0;
    bool mbBad = false;
    cv::Mat Tcw;
    KeyFrame *mpParent = nullptr;
    std::set<KeyFrame *> mspChildrens, mspLoopEdges;
    std::map<KeyFrame *, int> mConnectedKeyFrameWeights;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    std::vector<int> mvOrderedWeights;
    int nSetPose = 0;  // the stand-in's own
};

class Map {
  public:
    std::vector<KeyFrame *> GetAllKeyFrames() { return mspKeyFrames; }
    std::vector<MapPoint *> GetAllMapPoints() { return mspMapPoints; }
    std::vector<KeyFrame *> mspKeyFrames;  // the reference keeps sets; the tests need a stated order
    std::vector<MapPoint *> mspMapPoints;
};

class LoopClosing {
  public:
    typedef std::map<KeyFrame *, orbgpu_shim::Sim3> KeyFrameAndPose;  // g2o::Sim3 in the reference
};

struct Frame;
typedef orbgpu_shim::OptimizerT<Frame, MapPoint> Optimizer;
typedef orbgpu_shim::MapPointTableT<MapPoint> MapPointTable;
} // namespace ORB_SLAM2

#ifdef ORBGPU_EG_SCENE
namespace ORB_SLAM2 {
// the accessors of INTEGRATION.md's OptimizeEssentialGraph block
struct EssentialGraphAccess {
    cv::Mat pose_, pos_, normal_;
    const float *pose(KeyFrame *kf) { pose_ = kf->GetPose(); return pose_.ptr<float>(); }
    const float *world_pos(MapPoint *mp) { pos_ = mp->GetWorldPos(); return pos_.ptr<float>(); }
    const float *normal(MapPoint *mp) { normal_ = mp->GetNormal(); return normal_.ptr<float>(); }
    float min_dist(MapPoint *mp) { return mp->GetMinDistanceInvariance(); }
    float max_dist(MapPoint *mp) { return mp->GetMaxDistanceInvariance(); }
    static cv::Mat mat(int rows, int cols, const float *v)
    {
        cv::Mat m(rows, cols, CV_32F);
        std::memcpy(m.data, v, 4 * (size_t)rows * (size_t)cols);
        return m;
    }
    void set_pose(KeyFrame *kf, const float *T) { kf->SetPose(mat(4, 4, T)); }
    void set_world_pos(MapPoint *mp, const float *x) { mp->SetWorldPos(mat(3, 1, x)); }
};

struct EgScene {
    std::vector<KeyFrame> kfs;
    std::vector<MapPoint> mps;
    Map map;
    KeyFrame *pCurKF = nullptr, *pLoopKF = nullptr;
    bool bFixScale = false;
    LoopClosing::KeyFrameAndPose NonCorrectedSim3, CorrectedSim3;
    std::map<KeyFrame *, std::set<KeyFrame *>> LoopConnections;

    explicit EgScene(const char *path)
    {
        std::ifstream in(path);
        if (!in)
            throw std::runtime_error(std::string("cannot read ") + path);
        const int nK = i(in), nP = i(in);
        kfs.resize((size_t)nK), mps.resize((size_t)nP);
        for (KeyFrame &k : kfs) {
            k.mnId = (long unsigned int)i(in), k.mbBad = i(in) != 0;
            const int parent = i(in);
            k.mpParent = parent < 0 ? nullptr : &kfs.at((size_t)parent);
            k.Tcw.create(4, 4, CV_32F);
            for (int a = 0; a < 16; a++)
                k.Tcw.ptr<float>()[a] = (float)d(in);
            for (int a = 0, n = i(in); a < n; a++)
                k.mspChildrens.insert(&kfs.at((size_t)i(in)));
            for (int a = 0, n = i(in); a < n; a++)
                k.mspLoopEdges.insert(&kfs.at((size_t)i(in)));
            for (int a = 0, n = i(in); a < n; a++) {
                KeyFrame *o = &kfs.at((size_t)i(in));
                const int w = i(in);
                k.mConnectedKeyFrameWeights[o] = w;
                k.mvpOrderedConnectedKeyFrames.push_back(o), k.mvOrderedWeights.push_back(w);
            }
            map.mspKeyFrames.push_back(&k);
        }
        for (MapPoint &m : mps) {
            m.mnId = (long unsigned int)i(in), m.mbBad = i(in) != 0;
            const int ref = i(in);
            m.mpRefKF = ref < 0 ? nullptr : &kfs.at((size_t)ref);
            m.mnCorrectedByKF = (long unsigned int)i(in), m.mnCorrectedReference = (long unsigned int)i(in);
            m.mWorldPos.create(3, 1, CV_32F), m.mNormalVector.create(3, 1, CV_32F);
            for (int a = 0; a < 3; a++)
                m.mWorldPos.ptr<float>()[a] = (float)d(in), m.mNormalVector.ptr<float>()[a] = a == 2 ? 1.f : 0.f;
            map.mspMapPoints.push_back(&m);
        }
        pCurKF = &kfs.at((size_t)i(in)), pLoopKF = &kfs.at((size_t)i(in)), bFixScale = i(in) != 0;
        for (LoopClosing::KeyFrameAndPose *poses : {&NonCorrectedSim3, &CorrectedSim3})
            for (int a = 0, n = i(in); a < n; a++) {
                KeyFrame *k = &kfs.at((size_t)i(in));
                orbgpu_shim::Sim3 S;
                for (double &v : S.r)
                    v = d(in);
                for (double &v : S.t)
                    v = d(in);
                S.s = d(in);
                (*poses)[k] = S;
            }
        for (int a = 0, n = i(in); a < n; a++) {
            KeyFrame *k = &kfs.at((size_t)i(in));
            for (int b = 0, nb = i(in); b < nb; b++)
                LoopConnections[k].insert(&kfs.at((size_t)i(in)));
        }
        if (!in)
            throw std::runtime_error("short scene file");
    }
    int kf_index(const KeyFrame *k) const { return (int)(k - kfs.data()); }
    int mp_index(const MapPoint *m) const { return (int)(m - mps.data()); }

  private:
    static int i(std::ifstream &in)
    {
        int v = 0;
        in >> v;
        return v;
    }
    static double d(std::ifstream &in)
    {
        std::string tok;
        in >> tok;
        return strtod(tok.c_str(), nullptr);
    }
};
} // namespace ORB_SLAM2
#endif

// INTEGRATION.md's observation-graph block (section 2o) run on the device over one small scene: tests/test_covis_shim.py
// extracts the block into covis_block.inc, starts this program as a child process and compares what it prints with
// tests/covis_model.py.  Input (text): n_kf, then `id N` per key frame; n_obs, then `kf_index idx mp_id` per observation;
// the id of a map point and the index of a key frame to set bad; two frames as `n {mp_id or -1}*n`.
#include <algorithm>
#include <cstdio>
#include <deque>
#include <memory>

#include "covis_standin.hpp"
#include "covis_block.inc"

using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;

// what the block leaves to the reference's own text
void KeyFrame::AddConnection(KeyFrame *pKF, const int &weight)  // KeyFrame.cc:161-174
{
    {
        std::unique_lock<std::mutex> lock(mMutexConnections);
        if (mConnectedKeyFrameWeights.count(pKF) && mConnectedKeyFrameWeights[pKF] == weight)
            return;
        mConnectedKeyFrameWeights[pKF] = weight;
    }
    UpdateBestCovisibles();
}
void KeyFrame::UpdateBestCovisibles()  // KeyFrame.cc:176-195, pointers ordered by mnId (V4)
{
    std::unique_lock<std::mutex> lock(mMutexConnections);
    std::vector<std::pair<int, long unsigned int>> pairs;
    std::map<long unsigned int, KeyFrame *> by_id;
    for (const auto &kw : mConnectedKeyFrameWeights) {
        pairs.emplace_back(kw.second, kw.first->mnId);
        by_id[kw.first->mnId] = kw.first;
    }
    std::sort(pairs.begin(), pairs.end());
    mvpOrderedConnectedKeyFrames.clear(), mvOrderedWeights.clear();
    for (size_t i = pairs.size(); i-- > 0;) {
        mvpOrderedConnectedKeyFrames.push_back(by_id[pairs[i].second]);
        mvOrderedWeights.push_back(pairs[i].first);
    }
    mpCovisibilityGraph->UpdateCovisibles(this, mvpOrderedConnectedKeyFrames);
}

static bool read_frame(std::FILE *f, std::map<long, std::unique_ptr<MapPoint>> &mps, ORB_SLAM2::Frame &F)
{
    int n = 0;
    if (std::fscanf(f, "%d", &n) != 1 || n < 0)
        return false;
    F.N = n;
    F.mvpMapPoints.assign((size_t)n, nullptr);
    for (int i = 0; i < n; i++) {
        long id;
        if (std::fscanf(f, "%ld", &id) != 1)
            return false;
        if (id >= 0) {
            if (!mps.count(id))
                mps[id].reset(new MapPoint((long unsigned int)id));
            F.mvpMapPoints[(size_t)i] = mps[id].get();
        }
    }
    return true;
}

static void print(const char *tag, const ORB_SLAM2::Tracking &t)
{
    std::printf("KFS%s %zu", tag, t.mvpLocalKeyFrames.size());
    for (KeyFrame *p : t.mvpLocalKeyFrames)
        std::printf(" %lu", p->mnId);
    std::printf("\nPTS%s %zu", tag, t.mvpLocalMapPoints.size());
    for (MapPoint *p : t.mvpLocalMapPoints)
        std::printf(" %lu", p->mnId);
    std::printf("\nREF%s %ld\n", tag, t.mpReferenceKF ? (long)t.mpReferenceKF->mnId : -1L);
    for (KeyFrame *p : t.mvpLocalKeyFrames)
        if (p->mnTrackReferenceForFrame != t.mCurrentFrame.mnId)
            std::printf("STAMP %lu\n", p->mnId);
    for (MapPoint *p : t.mvpLocalMapPoints)
        if (p->mnTrackReferenceForFrame != t.mCurrentFrame.mnId)
            std::printf("STAMP %lu\n", p->mnId);
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: covis_shim_gpu_test scene.txt\n");
        return 2;
    }
    std::FILE *f = std::fopen(argv[1], "r");
    int n_kf = 0, n_obs = 0, bad_kf = -1;
    long bad_mp = -1;
    if (!f || std::fscanf(f, "%d", &n_kf) != 1 || n_kf < 1)
        return 3;
    std::deque<KeyFrame> kfs;
    for (int i = 0; i < n_kf; i++) {
        unsigned long id;
        int n;
        if (std::fscanf(f, "%lu %d", &id, &n) != 2 || n < 0)
            return 3;
        kfs.emplace_back(id, n);
    }
    struct Obs {
        int kf, idx;
        long mp;
    };
    std::vector<Obs> obs;
    if (std::fscanf(f, "%d", &n_obs) != 1 || n_obs < 0)
        return 3;
    for (int i = 0; i < n_obs; i++) {
        Obs o;
        if (std::fscanf(f, "%d %d %ld", &o.kf, &o.idx, &o.mp) != 3 || o.kf < 0 || o.kf >= n_kf || o.idx < 0 ||
            o.idx >= kfs[(size_t)o.kf].N || o.mp < 0)
            return 3;
        obs.push_back(o);
    }
    std::map<long, std::unique_ptr<MapPoint>> mps;
    ORB_SLAM2::Frame F1, F2;
    if (std::fscanf(f, "%ld %d", &bad_mp, &bad_kf) != 2 || bad_kf < 0 || bad_kf >= n_kf || !read_frame(f, mps, F1) ||
        !read_frame(f, mps, F2))
        return 3;
    std::fclose(f);
    try {
        ORB_SLAM2::CovisibilityGraph graph(0, 2, 8);
        KeyFrame::mpCovisibilityGraph = MapPoint::mpCovisibilityGraph = &graph;
        ORB_SLAM2::Map map;
        ORB_SLAM2::Tracking tracking;
        tracking.mpMap = &map;
        tracking.mpCovisibilityGraph = &graph;
        for (int i = 0; i < n_kf; i++) {
            KeyFrame *pKF = &kfs[(size_t)i];
            graph.AddKeyFrame(pKF);  // Map::AddKeyFrame
            for (const Obs &o : obs)  // LocalMapping::ProcessNewKeyFrame
                if (o.kf == i) {
                    if (!mps.count(o.mp))
                        mps[o.mp].reset(new MapPoint((long unsigned int)o.mp));
                    pKF->AddMapPoint(mps[o.mp].get(), (size_t)o.idx);
                    mps[o.mp]->AddObservation(pKF, (size_t)o.idx);
                }
            pKF->UpdateConnections();
            std::printf("CONN %lu %ld %zu", pKF->mnId, pKF->mpParent ? (long)pKF->mpParent->mnId : -1L,
                        pKF->mvpOrderedConnectedKeyFrames.size());
            for (size_t k = 0; k < pKF->mvpOrderedConnectedKeyFrames.size(); k++)
                std::printf(" %lu %d", pKF->mvpOrderedConnectedKeyFrames[k]->mnId, pKF->mvOrderedWeights[k]);
            std::printf("\n");
        }
        tracking.mCurrentFrame = F1;
        tracking.mCurrentFrame.mnId = 1001;
        tracking.UpdateLocalMap();
        print("", tracking);
        if (mps.count(bad_mp))
            mps[bad_mp]->SetBadFlag();
        KeyFrame *pBad = &kfs[(size_t)bad_kf];
        for (MapPoint *p : pBad->GetMapPointMatches())  // KeyFrame.cc:507-509 (without MapPoint::EraseObservation's cascade)
            if (p)
                p->mObservations.erase(pBad);
        const std::set<KeyFrame *> children = pBad->mspChildrens;
        for (KeyFrame *c : children)  // :568-573
            if (pBad->mpParent)
                c->ChangeParent(pBad->mpParent);
        pBad->SetBadFlag();
        tracking.mCurrentFrame = F2;
        tracking.mCurrentFrame.mnId = 1002;
        tracking.UpdateLocalMap();
        print("2", tracking);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    std::printf("covis shim ok\n");
    return 0;
}

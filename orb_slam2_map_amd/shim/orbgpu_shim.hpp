// orbgpu_shim.hpp -- C++ host side above the C ABI: re-creates the reference's three hot-path
// interfaces (ORB_SLAM2::ORBextractor, ORBmatcher::SearchByProjection x2 + DescriptorDistance,
// PointCloudMapping) on top of liborbgpu.so.
//
// The reference's own classes depend on OpenCV 2.4 / PCL 1.7 (absent from the build image), so
// everything that touches Frame / MapPoint / KeyFrame / cv::Mat is a template on those types: inside
// the reference tree the templates bind to the real classes (INTEGRATION.md shows the three edits);
// in this repository tests/shim_test.cpp binds them to small stand-ins with the same member names.
// Field names, argument meaning and return values follow the reference (file:line cited per item).
#pragma once

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <map>
#include <vector>

#include "orbgpu.h"

namespace orbgpu_shim {

inline void check(int status, const char *what)
{
    if (status != ORBGPU_OK)
        throw std::runtime_error(std::string(what) + ": " + orbgpu_last_error_string());
}

// --------------------------------------------------------------------------------------------
// ORBextractor (reference include/ORBextractor.h:46-110)
// KeyPointT must be layout-compatible with cv::KeyPoint (pt.x, pt.y, size, angle, response,
// octave, class_id = 28 bytes), which orbgpu_keypoint mirrors.
// --------------------------------------------------------------------------------------------
template <typename KeyPointT> class ORBextractorT {
  public:
    enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };

    ORBextractorT(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int device_id = 0)
    {
        static_assert(sizeof(KeyPointT) == sizeof(orbgpu_keypoint), "KeyPointT must match cv::KeyPoint");
        orbgpu_extractor_params p{nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device_id, 1};
        check(orbgpu_extractor_create(&p, &h_), "ORBextractor");
        nlevels_ = nlevels;
        scaleFactor_ = scaleFactor;
        mvScaleFactor.resize(nlevels);
        mvInvScaleFactor.resize(nlevels);
        mvLevelSigma2.resize(nlevels);
        mvInvLevelSigma2.resize(nlevels);
        check(orbgpu_extractor_get_scale_factors(h_, mvScaleFactor.data()), "scale factors");
        check(orbgpu_extractor_get_inv_scale_factors(h_, mvInvScaleFactor.data()), "scale factors");
        check(orbgpu_extractor_get_sigma2(h_, mvLevelSigma2.data()), "scale factors");
        check(orbgpu_extractor_get_inv_sigma2(h_, mvInvLevelSigma2.data()), "scale factors");
    }
    ~ORBextractorT() { orbgpu_extractor_destroy(h_); }
    ORBextractorT(const ORBextractorT &) = delete;
    ORBextractorT &operator=(const ORBextractorT &) = delete;

    // operator()(InputArray image, InputArray mask, vector<KeyPoint>&, OutputArray descriptors)
    // (ORBextractor.h:59-61).  `image`: 8-bit gray rows x cols with `step` bytes per row; the mask is
    // ignored as in the reference; descriptors: N x 32 bytes, contiguous (ORBextractor.cc:1068).
    void operator()(const uint8_t *image, int rows, int cols, size_t step, std::vector<KeyPointT> &keypoints,
                    std::vector<uint8_t> &descriptors)
    {
        keypoints.clear();
        descriptors.clear();
        if (!image || rows <= 0 || cols <= 0)
            return;  // ORBextractor.cc:1046
        int32_t cap = 0;
        check(orbgpu_extractor_max_keypoints(h_, cols, rows, &cap), "ORBextractor::operator()");
        keypoints.resize(cap);
        descriptors.resize((size_t)cap * 32);
        int32_t n = 0;
        check(orbgpu_extract(h_, image, cols, rows, step, reinterpret_cast<orbgpu_keypoint *>(keypoints.data()),
                             descriptors.data(), cap, &n),
              "ORBextractor::operator()");
        keypoints.resize(n);
        descriptors.resize((size_t)n * 32);
        last_rows_ = rows;
        last_cols_ = cols;
    }

    int GetLevels() { return nlevels_; }
    float GetScaleFactor() { return scaleFactor_; }
    std::vector<float> GetScaleFactors() { return mvScaleFactor; }
    std::vector<float> GetInverseScaleFactors() { return mvInvScaleFactor; }
    std::vector<float> GetScaleSigmaSquares() { return mvLevelSigma2; }
    std::vector<float> GetInverseScaleSigmaSquares() { return mvInvLevelSigma2; }

    // mvImagePyramid[level] (ORBextractor.h:85): lazily copied from the device; only stereo
    // matching reads it (Frame.cc:471,561,578).
    void GetPyramidLevel(int level, std::vector<uint8_t> &pixels, int &width, int &height)
    {
        // level size as ComputePyramid computes it (ORBextractor.cc:1112)
        int32_t w = (int32_t)lrintf((float)last_cols_ * mvInvScaleFactor[level]);
        int32_t h = (int32_t)lrintf((float)last_rows_ * mvInvScaleFactor[level]);
        pixels.resize((size_t)w * h);
        check(orbgpu_extractor_get_pyramid_level(h_, 0, level, pixels.data(), (size_t)w, &w, &h), "pyramid");
        width = w;
        height = h;
    }

    orbgpu_extractor *handle() { return h_; }

  protected:
    orbgpu_extractor *h_ = nullptr;
    int nlevels_ = 0, last_rows_ = 0, last_cols_ = 0;
    float scaleFactor_ = 0;
    std::vector<float> mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2;
};

// --------------------------------------------------------------------------------------------
// Frame::ComputeStereoMatches (reference src/Frame.cc:466-638) for the stereo constructor (Frame.cc:59-117): fills
// F.mvuRight / F.mvDepth from F.mvKeys, F.mvKeysRight, F.mDescriptors, F.mDescriptorsRight, F.mbf and F.fx, reading
// the pyramids of the two extractors' last calls (the ones that just extracted F's images) on the device.  mb is read
// by the reference before the constructor assigns it (Frame.cc:90 against :114): minZ = mbf / fx here.
// --------------------------------------------------------------------------------------------
// descriptor rows as N x 32 contiguous bytes: a std::vector<uint8_t> or anything with a `data` pointer (cv::Mat)
inline const uint8_t *DescriptorBytes(const std::vector<uint8_t> &d) { return d.data(); }
template <typename MatT> auto DescriptorBytes(const MatT &m) -> decltype((const uint8_t *)m.data)
{
    return (const uint8_t *)m.data;
}

template <typename FrameT, typename KeyPointT>
void ComputeStereoMatchesT(FrameT &F, ORBextractorT<KeyPointT> &left, ORBextractorT<KeyPointT> &right)
{
    const int32_t n = (int32_t)F.mvKeys.size(), nr = (int32_t)F.mvKeysRight.size();
    F.mvuRight = std::vector<float>(n, -1.0f);  // Frame.cc:468-469
    F.mvDepth = std::vector<float>(n, -1.0f);
    if (n == 0)
        return;
    check(orbgpu_compute_stereo_matches(left.handle(), right.handle(), n,
                                        reinterpret_cast<const orbgpu_keypoint *>(F.mvKeys.data()),
                                        DescriptorBytes(F.mDescriptors), nr,
                                        reinterpret_cast<const orbgpu_keypoint *>(F.mvKeysRight.data()),
                                        nr ? DescriptorBytes(F.mDescriptorsRight) : nullptr, F.mbf, F.fx,
                                        F.mvuRight.data(), F.mvDepth.data()),
          "Frame::ComputeStereoMatches");
}

// --------------------------------------------------------------------------------------------
// ORBVocabulary (reference include/ORBVocabulary.h: DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>)
// The file readers (loadFromTextFile / loadFromBinaryFile) stay the reference's; after loading, hand the node arrays
// over once (node i > 0: parent, isLeaf, descriptor row, weight -- m_nodes in index order).
// --------------------------------------------------------------------------------------------
typedef std::map<unsigned int, double> BowVector;                      // DBoW2::BowVector
typedef std::map<unsigned int, std::vector<unsigned int>> FeatureVector;  // DBoW2::FeatureVector

class ORBVocabularyT {
  public:
    ORBVocabularyT(int k, int L, const std::vector<int32_t> &parent, const std::vector<uint8_t> &is_leaf,
                   const std::vector<uint8_t> &desc, const std::vector<double> &weight, int weighting = 0,
                   int scoring = 0, int device_id = 0)
    {
        check(orbgpu_vocabulary_create(k, L, (int32_t)parent.size(), parent.data(), is_leaf.data(), desc.data(),
                                       weight.data(), weighting, scoring, device_id, &h_),
              "ORBVocabulary");
    }
    ~ORBVocabularyT() { orbgpu_vocabulary_destroy(h_); }
    ORBVocabularyT(const ORBVocabularyT &) = delete;
    ORBVocabularyT &operator=(const ORBVocabularyT &) = delete;

    // void transform(const std::vector<TDescriptor>& features, BowVector &v, FeatureVector &fv, int levelsup) const
    // (TemplatedVocabulary.h:145-146; Frame::ComputeBoW, Frame.cc:395-402).  descriptors: n rows of 32 bytes.
    void transform(const uint8_t *descriptors, int n, BowVector &v, FeatureVector &fv, int levelsup) const
    {
        v.clear();
        fv.clear();
        const size_t m = (size_t)std::max(n, 1);
        std::vector<int32_t> wid(m), nid(m), bid(m), fvn(m), fvs(m + 1), fvi(m);
        std::vector<double> wgt(m), bval(m);
        int32_t nb = 0, nf = 0;
        check(orbgpu_bow_transform(h_, descriptors, n, levelsup, wid.data(), wgt.data(), nid.data(), bid.data(),
                                   bval.data(), &nb, fvn.data(), fvs.data(), fvi.data(), &nf),
              "ORBVocabulary::transform");
        for (int i = 0; i < nb; i++)
            v.emplace_hint(v.end(), (unsigned)bid[i], bval[i]);
        for (int t = 0; t < nf; t++)
            fv.emplace_hint(fv.end(), (unsigned)fvn[t],
                            std::vector<unsigned int>(fvi.begin() + fvs[t], fvi.begin() + fvs[t + 1]));
    }
    orbgpu_vocabulary *handle() const { return h_; }

  protected:
    orbgpu_vocabulary *h_ = nullptr;
};

// per-feature node ids (-1 = not in the vector) from a FeatureVector: what orbgpu_search_by_bow consumes
inline std::vector<int32_t> NodeIdsOf(const FeatureVector &fv, int n)
{
    std::vector<int32_t> node((size_t)std::max(n, 1), -1);
    for (const auto &kv : fv)
        for (unsigned int i : kv.second)
            if ((int)i < n)
                node[i] = (int32_t)kv.first;
    return node;
}

// --------------------------------------------------------------------------------------------
// ORBmatcher (reference include/ORBmatcher.h:41-106)
// --------------------------------------------------------------------------------------------
constexpr int FRAME_GRID_ROWS = ORBGPU_GRID_ROWS, FRAME_GRID_COLS = ORBGPU_GRID_COLS;

// Flattens the Frame members the matcher reads into the ABI's SoA view.  FrameT needs the
// reference's member names: N, mvKeysUn[i].pt/.octave/.angle, mvuRight, descriptor rows via
// desc_row(F,i), mGrid[COLS][ROWS], mnMinX.., mfGridElementWidthInv.., mvScaleFactors.
template <typename FrameT> struct FrameSoA {
    std::vector<float> x, y, angle, uright;
    std::vector<int32_t> octave, cell_start, cell_items;
    std::vector<uint8_t> desc;
    orbgpu_frame_view view{};
    template <typename DescRow> FrameSoA(const FrameT &F, DescRow desc_row)
    {
        const int n = F.N;
        x.resize(n), y.resize(n), angle.resize(n), uright.resize(n), octave.resize(n), desc.resize((size_t)n * 32);
        for (int i = 0; i < n; i++) {
            x[i] = F.mvKeysUn[i].pt.x;
            y[i] = F.mvKeysUn[i].pt.y;
            angle[i] = F.mvKeysUn[i].angle;
            octave[i] = F.mvKeysUn[i].octave;
            uright[i] = F.mvuRight[i];
            std::memcpy(&desc[(size_t)i * 32], desc_row(F, i), 32);
        }
        cell_start.assign(FRAME_GRID_COLS * FRAME_GRID_ROWS + 1, 0);
        for (int ix = 0; ix < FRAME_GRID_COLS; ix++)
            for (int iy = 0; iy < FRAME_GRID_ROWS; iy++) {
                const auto &cell = F.mGrid[ix][iy];
                cell_start[ix * FRAME_GRID_ROWS + iy + 1] = cell_start[ix * FRAME_GRID_ROWS + iy] + (int32_t)cell.size();
                for (size_t k = 0; k < cell.size(); k++)
                    cell_items.push_back((int32_t)cell[k]);
            }
        if (cell_items.empty())
            cell_items.push_back(0);
        view.n = n;
        view.kp_x = x.data(), view.kp_y = y.data(), view.kp_octave = octave.data(), view.kp_angle = angle.data();
        view.u_right = uright.data(), view.desc = desc.data();
        view.min_x = F.mnMinX, view.max_x = F.mnMaxX, view.min_y = F.mnMinY, view.max_y = F.mnMaxY;
        view.grid_inv_w = F.mfGridElementWidthInv, view.grid_inv_h = F.mfGridElementHeightInv;
        view.scale_factors = F.mvScaleFactors.data(), view.nlevels = (int32_t)F.mvScaleFactors.size();
        view.cell_start = cell_start.data(), view.cell_items = cell_items.data();
    }
};

// Positions of a few pointers inside a long pointer list in O(list + queries): the queries go into a small
// open-addressing set (cache resident), the list is walked once.  Replaces the per-key-point linear search over
// vpMapPoints (2 016 x 10 059 pointer compares per SearchByProjection call at C3's size).
template <typename T> class PtrIndex {
  public:
    // keys: the pointers to look for (nullptr entries are ignored)
    template <typename It> PtrIndex(It first, It last)
    {
        size_t n = 0;
        for (It it = first; it != last; ++it)
            n += *it != nullptr;
        size_t cap = 16;
        while (cap < 2 * n + 2)
            cap *= 2;
        mask_ = cap - 1;
        key_.assign(cap, nullptr);
        val_.assign(cap, -1);
        for (It it = first; it != last; ++it)
            if (*it != nullptr)
                slot(*it, true);
    }
    // first position of every key inside [list, list + m)
    void locate(T *const *list, int m)
    {
        for (int i = 0; i < m; i++) {
            const long s = slot(list[i], false);
            if (s >= 0 && val_[(size_t)s] < 0)
                val_[(size_t)s] = i;
        }
    }
    int position(T *p) const
    {
        if (!p)
            return -1;
        for (size_t s = hash(p) & mask_;; s = (s + 1) & mask_) {
            if (key_[s] == p)
                return val_[s];
            if (!key_[s])
                return -1;
        }
    }

  private:
    static size_t hash(const T *p) { return (size_t)(((uintptr_t)p >> 4) * 0x9E3779B97F4A7C15ull >> 20); }
    long slot(T *p, bool insert)
    {
        if (!p)
            return -1;
        for (size_t s = hash(p) & mask_;; s = (s + 1) & mask_) {
            if (key_[s] == p)
                return (long)s;
            if (!key_[s]) {
                if (!insert)
                    return -1;
                key_[s] = p;
                return (long)s;
            }
        }
    }
    std::vector<T *> key_;
    std::vector<int> val_;
    size_t mask_ = 0;
};

// --------------------------------------------------------------------------------------------
// Device-resident MapPoint table (orbgpu_mappoint_table_*): what the matchers read of every map point, keyed by
// MapPoint::mnId (MapPoint.h:84), so that a matcher call hands over ids instead of locking and cloning 10 k objects
// (MapPoint::GetDescriptor, MapPoint.cc:309-313).  MapPointT needs mnId; the accessors are the same callables the
// matcher overloads take.  INTEGRATION.md section 2c lists where the reference calls these.
// --------------------------------------------------------------------------------------------
template <typename MapPointT> class MapPointTableT {
  public:
    explicit MapPointTableT(int device_id = 0, int initial_rows = 0)
    {
        check(orbgpu_mappoint_table_create(device_id, initial_rows, &h_), "MapPointTable");
    }
    ~MapPointTableT() { orbgpu_mappoint_table_destroy(h_); }
    MapPointTableT(const MapPointTableT &) = delete;
    MapPointTableT &operator=(const MapPointTableT &) = delete;
    orbgpu_mappoint_table *handle() const { return h_; }
    // One caller at a time (the C ABI's rule for a table).  In the reference LocalMapping creates and culls map points
    // while Tracking searches, and only some of those edits happen under Map::mMutexMapUpdate, so the wrapper serialises
    // its own calls and the matcher overloads that search the table take the same lock.
    std::mutex &mutex() const { return mu_; }
    int rows() const
    {
        std::lock_guard<std::mutex> g(mu_);
        int32_t r = 0;
        check(orbgpu_mappoint_table_rows(h_, &r), "MapPointTable::rows");
        return r;
    }

    // every attribute of a batch of points (new key frame: MapPoint constructors, UpdateNormalAndDepth,
    // ComputeDistinctiveDescriptors of the points it created or observed)
    template <typename WorldPos, typename Normal, typename MinDist, typename MaxDist, typename MpDesc>
    void Upsert(const std::vector<MapPointT *> &pts, WorldPos world_pos, Normal normal, MinDist min_dist, MaxDist max_dist,
                MpDesc mp_desc)
    {
        std::lock_guard<std::mutex> g(mu_);
        const size_t n = pts.size();
        ids_.resize(n), wp_.resize(3 * n), nr_.resize(3 * n), mn_.resize(n), mx_.resize(n), ds_.resize(32 * n), ob_.resize(n);
        for (size_t i = 0; i < n; i++) {
            MapPointT *p = pts[i];
            ids_[i] = (int64_t)p->mnId;
            const float *w = world_pos(p), *nn = normal(p);
            for (int c = 0; c < 3; c++)
                wp_[3 * i + c] = w[c], nr_[3 * i + c] = nn[c];
            mn_[i] = min_dist(p), mx_[i] = max_dist(p);
            std::memcpy(&ds_[32 * i], mp_desc(p), 32);
            ob_[i] = p->Observations();
        }
        check(orbgpu_mappoint_table_upsert(h_, (int32_t)n, ids_.data(), wp_.data(), nr_.data(), mn_.data(), mx_.data(),
                                           ds_.data(), ob_.data()),
              "MapPointTable::Upsert");
        for (size_t i = 0; i < n; i++)
            if (pts[i]->isBad())
                bad_.push_back(ids_[i]);
        if (!bad_.empty()) {
            check(orbgpu_mappoint_table_set_bad(h_, (int32_t)bad_.size(), bad_.data(), nullptr), "MapPointTable::SetBad");
            bad_.clear();
        }
    }
    // MapPoint::SetWorldPos (MapPoint.cc:73-78)
    void SetWorldPos(MapPointT *p, const float *w)
    {
        std::lock_guard<std::mutex> g(mu_);
        const int64_t id = (int64_t)p->mnId;
        check(orbgpu_mappoint_table_upsert(h_, 1, &id, w, nullptr, nullptr, nullptr, nullptr, nullptr), "SetWorldPos");
    }
    // MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:242-307): the chosen descriptor
    void SetDescriptor(MapPointT *p, const uint8_t *d)
    {
        std::lock_guard<std::mutex> g(mu_);
        const int64_t id = (int64_t)p->mnId;
        check(orbgpu_mappoint_table_upsert(h_, 1, &id, nullptr, nullptr, nullptr, nullptr, d, nullptr), "SetDescriptor");
    }
    // MapPoint::AddObservation / EraseObservation (MapPoint.cc:98-149)
    void SetObservations(MapPointT *p)
    {
        std::lock_guard<std::mutex> g(mu_);
        const int64_t id = (int64_t)p->mnId;
        const int32_t n = p->Observations();
        check(orbgpu_mappoint_table_set_observations(h_, 1, &id, &n, nullptr), "SetObservations");
    }
    // MapPoint::SetBadFlag (MapPoint.cc:151-175), MapPoint::Replace (:177-228)
    void SetBad(MapPointT *p)
    {
        std::lock_guard<std::mutex> g(mu_);
        const int64_t id = (int64_t)p->mnId;
        check(orbgpu_mappoint_table_set_bad(h_, 1, &id, nullptr), "SetBad");
    }
    // Batch forms: ONE staged copy, launch and synchronisation for the whole set, under one hold of the mutex Tracking's
    // searches take.  These are what the bulk writers call: the write-back loops of bundle adjustment
    // (Optimizer.cc:775 / 1040: SetWorldPos + UpdateNormalAndDepth per point, thousands per local BA), loop correction
    // (LoopClosing.cc:520-560) and MapPointCulling.  The one-id forms above cost a full host <-> device round trip each.
    template <typename WorldPos, typename Normal, typename MinDist, typename MaxDist>
    void SetWorldPos(const std::vector<MapPointT *> &pts, WorldPos world_pos, Normal normal, MinDist min_dist, MaxDist max_dist)
    {
        std::lock_guard<std::mutex> g(mu_);
        const size_t n = pts.size();
        ids_.resize(n), wp_.resize(3 * n), nr_.resize(3 * n), mn_.resize(n), mx_.resize(n);
        for (size_t i = 0; i < n; i++) {
            MapPointT *p = pts[i];
            ids_[i] = (int64_t)p->mnId;
            const float *w = world_pos(p), *nn = normal(p);
            for (int c = 0; c < 3; c++)
                wp_[3 * i + c] = w[c], nr_[3 * i + c] = nn[c];
            mn_[i] = min_dist(p), mx_[i] = max_dist(p);
        }
        check(orbgpu_mappoint_table_upsert(h_, (int32_t)n, ids_.data(), wp_.data(), nr_.data(), mn_.data(), mx_.data(), nullptr,
                                           nullptr),
              "SetWorldPos (batch)");
    }
    // the same through an accessor with world_pos(p), normal(p), min_dist(p), max_dist(p): the optimisers' write-backs
    template <typename Access> void SetWorldPos(const std::vector<MapPointT *> &pts, Access &access)
    {
        SetWorldPos(pts, [&access](MapPointT *q) { return access.world_pos(q); }, [&access](MapPointT *q) { return access.normal(q); },
                    [&access](MapPointT *q) { return access.min_dist(q); }, [&access](MapPointT *q) { return access.max_dist(q); });
    }
    void SetObservations(const std::vector<MapPointT *> &pts)
    {
        std::lock_guard<std::mutex> g(mu_);
        const size_t n = pts.size();
        ids_.resize(n), ob_.resize(n);
        for (size_t i = 0; i < n; i++)
            ids_[i] = (int64_t)pts[i]->mnId, ob_[i] = pts[i]->Observations();
        check(orbgpu_mappoint_table_set_observations(h_, (int32_t)n, ids_.data(), ob_.data(), nullptr), "SetObservations (batch)");
    }
    // the count taken by the caller: for a hook that runs where MapPoint::mMutexFeatures is held (Observations() would
    // lock it again)
    void SetObservations(MapPointT *p, int nObs)
    {
        std::lock_guard<std::mutex> g(mu_);
        const int64_t id = (int64_t)p->mnId;
        const int32_t n = nObs;
        check(orbgpu_mappoint_table_set_observations(h_, 1, &id, &n, nullptr), "SetObservations");
    }
    void SetBad(const std::vector<MapPointT *> &pts)
    {
        std::lock_guard<std::mutex> g(mu_);
        ids_.resize(pts.size());
        for (size_t i = 0; i < pts.size(); i++)
            ids_[i] = (int64_t)pts[i]->mnId;
        check(orbgpu_mappoint_table_set_bad(h_, (int32_t)ids_.size(), ids_.data(), nullptr), "SetBad (batch)");
    }
    // Bounds the table: only the listed points stay (Map::GetAllMapPoints() + what the current / last Frame still hold);
    // returns the number of rows released.  The reference never frees a MapPoint; its table equivalent is this call.
    int Retain(const std::vector<MapPointT *> &pts)
    {
        std::lock_guard<std::mutex> g(mu_);
        ids_.resize(pts.size());
        for (size_t i = 0; i < pts.size(); i++)
            ids_[i] = (int64_t)pts[i]->mnId;
        int32_t dropped = 0;
        check(orbgpu_mappoint_table_retain(h_, (int32_t)ids_.size(), ids_.data(), &dropped), "Retain");
        return dropped;
    }
    // ids of the last table search that the table had not been told about yet (skipped rows, held key points)
    std::pair<int, int> LastUnknown() const
    {
        std::lock_guard<std::mutex> g(mu_);
        int32_t a = 0, b = 0;
        check(orbgpu_mappoint_table_last_unknown(h_, &a, &b), "LastUnknown");
        return {a, b};
    }

  private:
    mutable std::mutex mu_;
    orbgpu_mappoint_table *h_ = nullptr;
    std::vector<int64_t> ids_, bad_;
    std::vector<float> wp_, nr_, mn_, mx_;
    std::vector<uint8_t> ds_;
    std::vector<int32_t> ob_;
};

// A Frame's matcher-side members on the device (orbgpu_frame_*): uploaded once per frame, then current frame of
// SearchByProjection(Cur, Last) and of SearchLocalPoints, and last frame of the next call.
template <typename FrameT> class DeviceFrameT {
  public:
    explicit DeviceFrameT(int device_id = 0) { check(orbgpu_frame_create(device_id, &h_), "DeviceFrame"); }
    ~DeviceFrameT() { orbgpu_frame_destroy(h_); }
    DeviceFrameT(const DeviceFrameT &) = delete;
    DeviceFrameT &operator=(const DeviceFrameT &) = delete;
    template <typename DescRow> void Upload(const FrameT &F, DescRow desc_row)
    {
        FrameSoA<FrameT> soa(F, desc_row);
        check(orbgpu_frame_upload(h_, &soa.view), "DeviceFrame::Upload");
        n_ = F.N;
    }
    orbgpu_frame *handle() const { return h_; }
    int N() const { return n_; }

  private:
    orbgpu_frame *h_ = nullptr;
    int n_ = 0;
};

template <typename FrameT, typename MapPointT> class ORBmatcherT {
  public:
    static const int TH_LOW = ORBGPU_TH_LOW, TH_HIGH = ORBGPU_TH_HIGH, HISTO_LENGTH = ORBGPU_HISTO_LENGTH;

    ORBmatcherT(float nnratio = 0.6f, bool checkOri = true, int device_id = 0)
        : mfNNratio(nnratio), mbCheckOrientation(checkOri), device_(device_id)
    {
    }

    // static int DescriptorDistance(const cv::Mat &a, const cv::Mat &b)  (ORBmatcher.h:44)
    static int DescriptorDistance(const uint8_t *a, const uint8_t *b, int device_id = 0)
    {
        int32_t d = 0;
        check(orbgpu_hamming256(a, b, 1, &d, device_id), "DescriptorDistance");
        return d;
    }

    // int SearchByProjection(Frame &F, const std::vector<MapPoint*> &vpMapPoints, const float th=3)
    // (ORBmatcher.h:48, ORBmatcher.cc:45-129).  desc_row(F,i) / mp_desc(pMP) return 32-byte rows.
    template <typename DescRow, typename MpDesc>
    int SearchByProjection(FrameT &F, const std::vector<MapPointT *> &vpMapPoints, const float th, DescRow desc_row,
                           MpDesc mp_desc)
    {
        FrameSoA<FrameT> soa(F, desc_row);
        const int m = (int)vpMapPoints.size();
        std::vector<uint8_t> in_view(m), bad(m), obs(m), desc((size_t)std::max(m, 1) * 32);
        std::vector<int32_t> level(m);
        std::vector<float> vcos(m), px(m), py(m), pxr(m);
        for (int i = 0; i < m; i++) {
            MapPointT *p = vpMapPoints[i];
            in_view[i] = p->mbTrackInView;
            bad[i] = p->isBad();
            obs[i] = p->Observations() > 0;
            level[i] = p->mnTrackScaleLevel;
            vcos[i] = p->mTrackViewCos;
            px[i] = p->mTrackProjX, py[i] = p->mTrackProjY, pxr[i] = p->mTrackProjXR;
            std::memcpy(&desc[(size_t)i * 32], mp_desc(p), 32);
        }
        orbgpu_mappoint_view mv{m,         in_view.data(), bad.data(), obs.data(), level.data(),
                                vcos.data(), px.data(),      py.data(),  pxr.data(), desc.data()};
        // F.mvpMapPoints -> indices: points of the list by position, others by their Observations()
        std::vector<int32_t> k2m(F.N, -1);
        PtrIndex<MapPointT> held(F.mvpMapPoints.begin(), F.mvpMapPoints.end());
        held.locate(vpMapPoints.data(), m);
        for (int j = 0; j < F.N; j++) {
            MapPointT *p = F.mvpMapPoints[j];
            if (!p)
                continue;
            const int idx = held.position(p);
            k2m[j] = idx >= 0 ? idx : (p->Observations() > 0 ? -2 : -1);
        }
        std::vector<int32_t> before = k2m;
        int32_t nmatches = 0;
        check(orbgpu_search_by_projection(&soa.view, &mv, th, mfNNratio, k2m.data(), &nmatches, device_),
              "SearchByProjection");
        for (int j = 0; j < F.N; j++)
            if (k2m[j] != before[j] && k2m[j] >= 0)
                F.mvpMapPoints[j] = vpMapPoints[k2m[j]];  // ORBmatcher.cc:123
        return nmatches;
    }

    // int SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono)
    // (ORBmatcher.h:52, ORBmatcher.cc:1328-1470).  Tcw(F) returns the 16 floats of F.mTcw (row-major);
    // world_pos(pMP) the 3 floats of GetWorldPos().
    template <typename DescRow, typename MpDesc, typename TcwOf, typename WorldPos>
    int SearchByProjection(FrameT &CurrentFrame, const FrameT &LastFrame, const float th, const bool bMono,
                           DescRow desc_row, MpDesc mp_desc, TcwOf Tcw, WorldPos world_pos)
    {
        FrameSoA<FrameT> cur(CurrentFrame, desc_row);
        const int n = LastFrame.N;
        std::vector<uint8_t> has(n), outl(n), obs(n), desc((size_t)std::max(n, 1) * 32);
        std::vector<float> wp((size_t)std::max(n, 1) * 3), ang(n);
        std::vector<int32_t> oct(n);
        for (int i = 0; i < n; i++) {
            MapPointT *p = LastFrame.mvpMapPoints[i];
            has[i] = p != nullptr;
            outl[i] = LastFrame.mvbOutlier[i];
            oct[i] = LastFrame.mvKeys[i].octave;
            ang[i] = LastFrame.mvKeysUn[i].angle;
            if (p) {
                obs[i] = p->Observations() > 0;
                const float *w = world_pos(p);
                wp[3 * i] = w[0], wp[3 * i + 1] = w[1], wp[3 * i + 2] = w[2];
                std::memcpy(&desc[(size_t)i * 32], mp_desc(p), 32);
            }
        }
        orbgpu_lastframe_view lv{n, has.data(), outl.data(), obs.data(), wp.data(), desc.data(), oct.data(), ang.data(),
                                 Tcw(LastFrame)};
        std::vector<int32_t> k2m(CurrentFrame.N, -1);
        for (int j = 0; j < CurrentFrame.N; j++)
            if (MapPointT *p = CurrentFrame.mvpMapPoints[j])
                k2m[j] = p->Observations() > 0 ? -2 : -1;
        std::vector<int32_t> before = k2m;
        int32_t nmatches = 0;
        check(orbgpu_search_by_projection_last(&cur.view, Tcw(CurrentFrame), CurrentFrame.fx, CurrentFrame.fy,
                                               CurrentFrame.cx, CurrentFrame.cy, CurrentFrame.mbf, CurrentFrame.mb, &lv,
                                               th, bMono, mbCheckOrientation, k2m.data(), &nmatches, device_),
              "SearchByProjection(last)");
        for (int j = 0; j < CurrentFrame.N; j++) {
            if (k2m[j] == before[j])
                continue;
            CurrentFrame.mvpMapPoints[j] = k2m[j] >= 0 ? LastFrame.mvpMapPoints[k2m[j]] : nullptr;  // :1428, :1461
        }
        return nmatches;
    }

    // ---- the same two matchers over the device-resident MapPoint table ------------------------------------------------
    // SearchByProjection(F, vpMapPoints, th) (ORBmatcher.cc:45-129) as a drop-in at the ORBmatcher level: the mTrack*
    // members Frame::isInFrustum filled are uploaded (7 values per point); descriptors, isBad() and Observations() come
    // from the table by mnId.  dF holds F's matcher-side members on the device (DeviceFrameT::Upload, once per frame).
    int SearchByProjection(FrameT &F, const DeviceFrameT<FrameT> &dF, const std::vector<MapPointT *> &vpMapPoints,
                           const float th, MapPointTableT<MapPointT> &table)
    {
        const int m = (int)vpMapPoints.size();
        ids_.resize(m), b0_.resize(m), i0_.resize(m), f0_.resize(m), f1_.resize(m), f2_.resize(m), f3_.resize(m);
        for (int i = 0; i < m; i++) {
            const MapPointT *p = vpMapPoints[i];
            ids_[i] = (int64_t)p->mnId;
            b0_[i] = p->mbTrackInView;
            i0_[i] = p->mnTrackScaleLevel;
            f0_[i] = p->mTrackViewCos, f1_[i] = p->mTrackProjX, f2_[i] = p->mTrackProjY, f3_[i] = p->mTrackProjXR;
        }
        orbgpu_mappoint_view sc{m, b0_.data(), nullptr, nullptr, i0_.data(), f0_.data(), f1_.data(), f2_.data(), f3_.data(), nullptr};
        return run_local(F, dF, vpMapPoints, table, nullptr, &sc, nullptr, 0, 0, 0, 0, 0, 0, 0.5f, th, nullptr);
    }

    // Tracking::SearchLocalPoints (Tracking.cc:1468-1496) in one call: Frame::isInFrustum + MapPoint::PredictScale run on
    // the device over the table, then SearchByProjection(F, vpLocalMapPoints, th).  skip(pMP) is the host-only half of
    // :1474 (pMP->mnLastFrameSeen == F.mnId); isBad() comes from the table.  Returns the match count; *nToMatch
    // (optional) = points in the frustum; in_view(pMP, bool) is called for every listed point so that the caller can do
    // IncreaseVisible() and keep mbTrackInView current (:1479-1483).
    template <typename Skip, typename TcwOf, typename InView>
    int SearchLocalPoints(FrameT &F, const DeviceFrameT<FrameT> &dF, const std::vector<MapPointT *> &vpLocalMapPoints,
                          const float th, MapPointTableT<MapPointT> &table, Skip skip, TcwOf Tcw, InView in_view,
                          int *nToMatch = nullptr)
    {
        const int m = (int)vpLocalMapPoints.size();
        ids_.resize(m), b0_.resize(m), b1_.resize(m);
        for (int i = 0; i < m; i++) {
            ids_[i] = (int64_t)vpLocalMapPoints[i]->mnId;
            b0_[i] = skip(vpLocalMapPoints[i]) ? 1 : 0;
        }
        orbgpu_track_scratch trk{b1_.data(), nullptr, nullptr, nullptr, nullptr, nullptr};
        const int nm = run_local(F, dF, vpLocalMapPoints, table, b0_.data(), nullptr, Tcw(F), F.fx, F.fy, F.cx, F.cy, F.mbf,
                                 F.mfLogScaleFactor, 0.5f, th, &trk);
        int seen = 0;
        for (int i = 0; i < m; i++) {
            in_view(vpLocalMapPoints[i], b1_[i] != 0);
            seen += b1_[i] != 0;
        }
        if (nToMatch)
            *nToMatch = seen;
        return nm;
    }

    // SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1328-1470) with both frames on the device and
    // the last frame's map points (world position, descriptor, Observations()) looked up by mnId.
    template <typename TcwOf>
    int SearchByProjection(FrameT &CurrentFrame, const DeviceFrameT<FrameT> &dCur, const FrameT &LastFrame,
                           const DeviceFrameT<FrameT> &dLast, const float th, const bool bMono,
                           MapPointTableT<MapPointT> &table, TcwOf Tcw)
    {
        const int nl = LastFrame.N, n = CurrentFrame.N;
        ids_.resize(nl), b0_.resize(nl), kid_.resize(n), k2m_.resize(std::max(n, 1));
        for (int i = 0; i < nl; i++) {
            const MapPointT *p = LastFrame.mvpMapPoints[i];
            ids_[i] = p ? (int64_t)p->mnId : -1;
            b0_[i] = LastFrame.mvbOutlier[i];
        }
        for (int j = 0; j < n; j++)
            kid_[j] = CurrentFrame.mvpMapPoints[j] ? (int64_t)CurrentFrame.mvpMapPoints[j]->mnId : -1;
        int32_t nmatches = 0;
        std::lock_guard<std::mutex> table_lock(table.mutex());
        check(orbgpu_search_by_projection_last_table(dCur.handle(), Tcw(CurrentFrame), dLast.handle(), Tcw(LastFrame),
                                                     table.handle(), ids_.data(), b0_.data(), kid_.data(), CurrentFrame.fx,
                                                     CurrentFrame.fy, CurrentFrame.cx, CurrentFrame.cy, CurrentFrame.mbf,
                                                     CurrentFrame.mb, th, bMono, mbCheckOrientation, k2m_.data(), &nmatches),
              "SearchByProjection(last, table)");
        for (int j = 0; j < n; j++)
            if (k2m_[j] >= 0)
                CurrentFrame.mvpMapPoints[j] = LastFrame.mvpMapPoints[k2m_[j]];  // :1428
        return nmatches;
    }

    // int SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const std::set<MapPoint*> &sAlreadyFound,
    //                        const float th, const int ORBdist)   (ORBmatcher.h:56, ORBmatcher.cc:1472-1599)
    // KeyFrameT needs GetMapPointMatches() and mvKeysUn; found(pMP) tells whether pMP is in sAlreadyFound;
    // max_dist(pMP) returns mfMaxDistance (the numerator of MapPoint::PredictScale, a protected member:
    // add an accessor or a friend declaration to MapPoint.h).
    template <typename KeyFrameT, typename DescRow, typename MpDesc, typename TcwOf, typename WorldPos, typename Found,
              typename MaxDist>
    int SearchByProjection(FrameT &CurrentFrame, KeyFrameT *pKF, Found found, const float th, const int ORBdist,
                           DescRow desc_row, MpDesc mp_desc, TcwOf Tcw, WorldPos world_pos, MaxDist max_dist)
    {
        FrameSoA<FrameT> cur(CurrentFrame, desc_row);
        const std::vector<MapPointT *> vpMPs = pKF->GetMapPointMatches();
        const int n = (int)vpMPs.size();
        std::vector<uint8_t> has(n), bad(n), fnd(n), desc((size_t)std::max(n, 1) * 32);
        std::vector<float> wp((size_t)std::max(n, 1) * 3), mininv(n), maxinv(n), maxd(n), ang(n);
        for (int i = 0; i < n; i++) {
            MapPointT *p = vpMPs[i];
            has[i] = p != nullptr;
            ang[i] = pKF->mvKeysUn[i].angle;
            if (!p)
                continue;
            bad[i] = p->isBad();
            fnd[i] = found(p);
            mininv[i] = p->GetMinDistanceInvariance(), maxinv[i] = p->GetMaxDistanceInvariance();
            maxd[i] = max_dist(p);
            const float *w = world_pos(p);
            wp[3 * i] = w[0], wp[3 * i + 1] = w[1], wp[3 * i + 2] = w[2];
            std::memcpy(&desc[(size_t)i * 32], mp_desc(p), 32);
        }
        orbgpu_keyframe_view kv{n, has.data(), bad.data(), fnd.data(), wp.data(), mininv.data(), maxinv.data(), maxd.data(),
                                desc.data(), ang.data()};
        std::vector<int32_t> k2m(CurrentFrame.N, -1);
        for (int j = 0; j < CurrentFrame.N; j++)
            if (CurrentFrame.mvpMapPoints[j])
                k2m[j] = -2;
        int32_t nmatches = 0;
        check(orbgpu_search_by_projection_keyframe(&cur.view, Tcw(CurrentFrame), CurrentFrame.fx, CurrentFrame.fy,
                                                   CurrentFrame.cx, CurrentFrame.cy, CurrentFrame.mfLogScaleFactor, &kv,
                                                   th, ORBdist, mbCheckOrientation, k2m.data(), &nmatches, device_),
              "SearchByProjection(keyframe)");
        for (int j = 0; j < CurrentFrame.N; j++)
            if (k2m[j] >= 0)
                CurrentFrame.mvpMapPoints[j] = vpMPs[k2m[j]];  // :1556
        return nmatches;
    }

    // int SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const std::vector<MapPoint*> &vpPoints,
    //                        std::vector<MapPoint*> &vpMatched, int th)   (ORBmatcher.h:60, ORBmatcher.cc:290-403)
    // KeyFrameT needs the Frame member names FrameSoA reads (KeyFrame.h has them all) plus fx, fy, cx, cy and
    // mfLogScaleFactor; Scw is the 4x4 row-major float Sim3; normal / min_dist / max_dist return GetNormal() and the
    // protected mfMinDistance / mfMaxDistance of a map point.
    template <typename KeyFrameT, typename DescRow, typename MpDesc, typename WorldPos, typename Normal,
              typename MinDist, typename MaxDist>
    int SearchByProjection(KeyFrameT *pKF, const float *Scw, const std::vector<MapPointT *> &vpPoints,
                           std::vector<MapPointT *> &vpMatched, int th, DescRow desc_row, MpDesc mp_desc,
                           WorldPos world_pos, Normal normal, MinDist min_dist, MaxDist max_dist)
    {
        FrameSoA<KeyFrameT> kf(*pKF, desc_row);
        const int m = (int)vpPoints.size();
        std::vector<uint8_t> bad(std::max(m, 1)), desc((size_t)std::max(m, 1) * 32);
        std::vector<float> wp((size_t)std::max(m, 1) * 3), nr((size_t)std::max(m, 1) * 3), mind(std::max(m, 1)),
            maxd(std::max(m, 1));
        for (int i = 0; i < m; i++) {
            MapPointT *p = vpPoints[i];
            bad[i] = p->isBad();
            const float *w = world_pos(p), *nn = normal(p);
            wp[3 * i] = w[0], wp[3 * i + 1] = w[1], wp[3 * i + 2] = w[2];
            nr[3 * i] = nn[0], nr[3 * i + 1] = nn[1], nr[3 * i + 2] = nn[2];
            mind[i] = min_dist(p), maxd[i] = max_dist(p);
            std::memcpy(&desc[(size_t)i * 32], mp_desc(p), 32);
        }
        orbgpu_points_view pv{m, bad.data(), wp.data(), nr.data(), mind.data(), maxd.data(), desc.data()};
        std::vector<int32_t> k2m(pKF->N, -1);
        PtrIndex<MapPointT> row(vpMatched.begin(), vpMatched.end());  // first row of every matched point (vpPoints has no duplicates in the reference)
        row.locate(vpPoints.data(), m);
        for (int j = 0; j < pKF->N; j++)
            if (vpMatched[j]) {
                const int r = row.position(vpMatched[j]);
                k2m[j] = r < 0 ? -2 : r;
            }
        const std::vector<int32_t> before = k2m;
        int32_t nmatches = 0;
        check(orbgpu_search_by_projection_sim3(&kf.view, Scw, pKF->fx, pKF->fy, pKF->cx, pKF->cy, pKF->mfLogScaleFactor,
                                               &pv, th, k2m.data(), &nmatches, device_),
              "SearchByProjection(Sim3)");
        for (int j = 0; j < pKF->N; j++)
            if (k2m[j] != before[j])
                vpMatched[j] = vpPoints[k2m[j]];  // :394
        return nmatches;
    }

    // int SearchByBoW(KeyFrame *pKF, Frame &F, std::vector<MapPoint*> &vpMapPointMatches)
    // (ORBmatcher.h:64, ORBmatcher.cc:159-288; Tracking::TrackReferenceKeyFrame, Tracking.cc:1051).
    // KeyFrameT: N, mvKeysUn, mFeatVec, GetMapPointMatches(); FrameT: N, mvKeys, mFeatVec.
    template <typename KeyFrameT, typename KfDescRow, typename DescRow>
    int SearchByBoW(KeyFrameT *pKF, FrameT &F, std::vector<MapPointT *> &vpMapPointMatches, KfDescRow kf_desc_row,
                    DescRow desc_row)
    {
        const std::vector<MapPointT *> vpMapPointsKF = pKF->GetMapPointMatches();
        vpMapPointMatches.assign(F.N, nullptr);  // :163
        const int nk = (int)vpMapPointsKF.size(), nf = F.N;
        std::vector<uint8_t> dk((size_t)std::max(nk, 1) * 32), df((size_t)std::max(nf, 1) * 32), valid(std::max(nk, 1));
        std::vector<float> ak(std::max(nk, 1)), af(std::max(nf, 1));
        for (int i = 0; i < nk; i++) {
            std::memcpy(&dk[(size_t)i * 32], kf_desc_row(*pKF, i), 32);
            ak[i] = pKF->mvKeysUn[i].angle;
            valid[i] = vpMapPointsKF[i] && !vpMapPointsKF[i]->isBad();  // :195-199
        }
        for (int j = 0; j < nf; j++) {
            std::memcpy(&df[(size_t)j * 32], desc_row(F, j), 32);
            af[j] = F.mvKeys[j].angle;  // :238
        }
        const std::vector<int32_t> nodek = NodeIdsOf(pKF->mFeatVec, nk), nodef = NodeIdsOf(F.mFeatVec, nf);
        std::vector<int32_t> match(std::max(nf, 1), -1);
        int32_t nmatches = 0;
        check(orbgpu_search_by_bow(dk.data(), ak.data(), valid.data(), nodek.data(), nk, df.data(), af.data(), nodef.data(),
                                   nf, TH_LOW, mfNNratio, mbCheckOrientation, match.data(), &nmatches, device_),
              "SearchByBoW");
        for (int j = 0; j < nf; j++)
            if (match[j] >= 0)
                vpMapPointMatches[j] = vpMapPointsKF[match[j]];  // :232
        return nmatches;
    }

    // int SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12,
    //                            std::vector<pair<size_t,size_t>> &vMatchedPairs, const bool bOnlyStereo)
    // (ORBmatcher.h:79, ORBmatcher.cc:657-823; LocalMapping::CreateNewMapPoints, LocalMapping.cc:268).
    // KeyFrameT: the members FrameSoA reads (N, mvKeysUn, mvuRight, mGrid, mnMinX.., mvScaleFactors), mFeatVec,
    // GetMapPoint(idx), fx, fy, cx, cy, mvLevelSigma2.  F12: the 9 floats of the fundamental matrix, row-major;
    // camera_center(kf, float[3]) / rotation(kf, float[9]) / translation(kf, float[3]) read GetCameraCenter(),
    // GetRotation(), GetTranslation().
    template <typename KeyFrameT, typename DescRow, typename Vec3Of, typename Mat3Of, typename Vec3Of2>
    int SearchForTriangulation(KeyFrameT *pKF1, KeyFrameT *pKF2, const float *F12,
                               std::vector<std::pair<size_t, size_t>> &vMatchedPairs, const bool bOnlyStereo,
                               DescRow desc_row, Vec3Of camera_center, Mat3Of rotation, Vec3Of2 translation)
    {
        // epipole in the second image (:664-670): C2 = R2w * Cw + t2w as cv::gemm computes a 3x3 * 3x1 float product
        // (products summed left to right, then the C term)
        float Cw[3], R2w[9], t2w[3], C2[3];
        camera_center(pKF1, Cw);
        rotation(pKF2, R2w);
        translation(pKF2, t2w);
        for (int r = 0; r < 3; r++) {
            volatile float a = R2w[3 * r] * Cw[0], b = R2w[3 * r + 1] * Cw[1], c = R2w[3 * r + 2] * Cw[2];
            volatile float ab = a + b;
            volatile float abc = ab + c;
            C2[r] = abc + t2w[r];
        }
        const float invz = 1.0f / C2[2];
        const float ex = pKF2->fx * C2[0] * invz + pKF2->cx;
        const float ey = pKF2->fy * C2[1] * invz + pKF2->cy;
        FrameSoA<KeyFrameT> s1(*pKF1, desc_row), s2(*pKF2, desc_row);
        std::vector<uint8_t> has1(std::max(pKF1->N, 1)), has2(std::max(pKF2->N, 1));
        for (int i = 0; i < pKF1->N; i++)
            has1[i] = pKF1->GetMapPoint(i) != nullptr;  // :702-705
        for (int i = 0; i < pKF2->N; i++)
            has2[i] = pKF2->GetMapPoint(i) != nullptr;  // :726-729
        const std::vector<int32_t> node1 = NodeIdsOf(pKF1->mFeatVec, pKF1->N), node2 = NodeIdsOf(pKF2->mFeatVec, pKF2->N);
        std::vector<int32_t> match12(std::max(pKF1->N, 1), -1);
        int32_t nmatches = 0;
        check(orbgpu_search_for_triangulation(&s1.view, has1.data(), node1.data(), &s2.view, has2.data(), node2.data(), F12, ex,
                                              ey, pKF2->mvLevelSigma2.data(), bOnlyStereo, mbCheckOrientation, match12.data(),
                                              &nmatches, device_),
              "SearchForTriangulation");
        vMatchedPairs.clear();  // :812-820
        vMatchedPairs.reserve((size_t)nmatches);
        for (int i = 0; i < pKF1->N; i++)
            if (match12[i] >= 0)
                vMatchedPairs.push_back(std::make_pair((size_t)i, (size_t)match12[i]));
        return nmatches;
    }

    // int Fuse(KeyFrame *pKF, const vector<MapPoint *> &vpMapPoints, const float th=3.0)
    // (ORBmatcher.h:88, ORBmatcher.cc:825-975; LocalMapping::SearchInNeighbors, LocalMapping.cc:489, 514).
    // The candidate of every map point (projection, level and chi-square gates, best descriptor within TH_LOW) comes
    // from the device in one call; the edits of :946-969 -- Replace / AddObservation / AddMapPoint, which mutate the
    // pointer graph -- are applied here in index order exactly as the reference's loop does, re-checking isBad() and
    // IsInKeyFrame() since an earlier edit can change them.  pose(kf, float[16]) reads GetPose() (row-major Tcw);
    // world_pos / normal(pMP) return 3 floats, min_dist / max_dist the protected mfMinDistance / mfMaxDistance,
    // mp_desc(pMP) the 32 descriptor bytes (as for the Sim3 overload above).
    template <typename KeyFrameT, typename DescRow, typename PoseOf, typename MpDesc, typename WorldPos, typename Normal,
              typename MinDist, typename MaxDist>
    int Fuse(KeyFrameT *pKF, const std::vector<MapPointT *> &vpMapPoints, const float th, DescRow desc_row, PoseOf pose,
             MpDesc mp_desc, WorldPos world_pos, Normal normal, MinDist min_dist, MaxDist max_dist)
    {
        FrameSoA<KeyFrameT> soa(*pKF, desc_row);
        const int m = (int)vpMapPoints.size();
        std::vector<uint8_t> bad(std::max(m, 1)), desc((size_t)std::max(m, 1) * 32);
        std::vector<float> wp((size_t)std::max(m, 1) * 3), nrm((size_t)std::max(m, 1) * 3), dmin(std::max(m, 1)), dmax(std::max(m, 1));
        for (int i = 0; i < m; i++) {
            MapPointT *p = vpMapPoints[i];
            bad[i] = !p || p->isBad() || p->IsInKeyFrame(pKF);  // :843-848
            if (!p)
                continue;
            const float *w = world_pos(p), *nn = normal(p);
            wp[3 * i] = w[0], wp[3 * i + 1] = w[1], wp[3 * i + 2] = w[2];
            nrm[3 * i] = nn[0], nrm[3 * i + 1] = nn[1], nrm[3 * i + 2] = nn[2];
            dmin[i] = min_dist(p), dmax[i] = max_dist(p);
            std::memcpy(&desc[(size_t)i * 32], mp_desc(p), 32);
        }
        orbgpu_points_view pv{m, bad.data(), wp.data(), nrm.data(), dmin.data(), dmax.data(), desc.data()};
        float Tcw[16];
        pose(pKF, Tcw);
        std::vector<int32_t> best(std::max(m, 1), -1);
        int32_t ncand = 0;
        check(orbgpu_fuse(&soa.view, Tcw, pKF->fx, pKF->fy, pKF->cx, pKF->cy, pKF->mbf, pKF->mfLogScaleFactor, &pv, th,
                          pKF->mvInvLevelSigma2.data(), best.data(), &ncand, device_),
              "Fuse");
        int nFused = 0;
        for (int i = 0; i < m; i++) {
            MapPointT *pMP = vpMapPoints[i];
            if (best[i] < 0 || !pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF))
                continue;
            MapPointT *pMPinKF = pKF->GetMapPoint(best[i]);  // :948
            if (pMPinKF) {
                if (!pMPinKF->isBad()) {
                    if (pMPinKF->Observations() > pMP->Observations())
                        pMP->Replace(pMPinKF);
                    else
                        pMPinKF->Replace(pMP);
                }
            } else {
                pMP->AddObservation(pKF, best[i]);
                pKF->AddMapPoint(pMP, best[i]);
            }
            nFused++;
        }
        return nFused;
    }

    // void MapPoint::ComputeDistinctiveDescriptors()  (MapPoint.cc:242-307) for a batch of map points: groups[g] holds
    // the descriptor rows of the non-bad observing key frames of point g (in mObservations order); returns the index
    // of the chosen row per point (-1: no observation, mDescriptor stays).
    static std::vector<int32_t> ComputeDistinctiveDescriptors(const std::vector<std::vector<const uint8_t *>> &groups,
                                                              int device_id = 0)
    {
        std::vector<int32_t> off(groups.size() + 1, 0), best(std::max<size_t>(groups.size(), 1), -1);
        for (size_t g = 0; g < groups.size(); g++)
            off[g + 1] = off[g] + (int32_t)groups[g].size();
        std::vector<uint8_t> flat((size_t)std::max(off.back(), 1) * 32);
        for (size_t g = 0; g < groups.size(); g++)
            for (size_t i = 0; i < groups[g].size(); i++)
                std::memcpy(&flat[((size_t)off[g] + i) * 32], groups[g][i], 32);
        check(orbgpu_distinctive_descriptors((int32_t)groups.size(), off.data(), flat.data(), best.data(), device_id),
              "ComputeDistinctiveDescriptors");
        best.resize(groups.size());
        return best;
    }

  protected:
    // the common tail of the table flavours of SearchByProjection(F, vpMapPoints, th): ids in, list positions out
    int run_local(FrameT &F, const DeviceFrameT<FrameT> &dF, const std::vector<MapPointT *> &vp,
                  MapPointTableT<MapPointT> &table, const uint8_t *skip, const orbgpu_mappoint_view *scratch,
                  const float *Tcw, float fx, float fy, float cx, float cy, float mbf, float log_sf, float cos_limit, float th,
                  orbgpu_track_scratch *trk)
    {
        const int n = F.N, m = (int)vp.size();
        kid_.resize(n), k2m_.resize(std::max(n, 1));
        for (int j = 0; j < n; j++)
            kid_[j] = F.mvpMapPoints[j] ? (int64_t)F.mvpMapPoints[j]->mnId : -1;
        int32_t nmatches = 0;
        std::lock_guard<std::mutex> table_lock(table.mutex());
        check(orbgpu_search_local_points_table(dF.handle(), table.handle(), m, ids_.data(), skip, scratch, Tcw, fx, fy, cx, cy,
                                               mbf, log_sf, cos_limit, th, mfNNratio, kid_.data(), k2m_.data(), &nmatches, trk),
              "SearchByProjection(table)");
        for (int j = 0; j < n; j++)
            if (k2m_[j] >= 0 && F.mvpMapPoints[j] != vp[k2m_[j]])
                F.mvpMapPoints[j] = vp[k2m_[j]];  // ORBmatcher.cc:123
        return nmatches;
    }

    float mfNNratio;
    bool mbCheckOrientation;
    int device_;
    // per-call staging, kept between calls (a matcher that lives on the stack per call site, as in the reference, pays
    // these allocations every time; Tracking can keep one matcher per thread instead)
    std::vector<int64_t> ids_, kid_;
    std::vector<int32_t> k2m_, i0_;
    std::vector<uint8_t> b0_, b1_;
    std::vector<float> f0_, f1_, f2_, f3_;
};

// --------------------------------------------------------------------------------------------
// Optimizer::PoseOptimization (reference include/Optimizer.h:52, src/Optimizer.cc:239-451): motion-only bundle
// adjustment of pFrame's pose.  Side effects as in the reference: pFrame->mvbOutlier[i] for every key point with a map
// point, the optimised pose handed to set_pose (Frame::SetPose), return value = inliers.  g2o is restated, not linked
// ("g2o unpinned", include/orbgpu.h).  FrameT needs N, mvKeysUn, mvuRight, mvpMapPoints, mvbOutlier, mvInvLevelSigma2,
// fx, fy, cx, cy, mbf; Tcw(F) returns the 16 floats of mTcw, world_pos(pMP) 3 floats (both valid during the call).
// --------------------------------------------------------------------------------------------
// A plain stand-in for g2o::Sim3 at the boundary of OptimizerT::OptimizeSim3 (g2o stays outside the shim):
//     orbgpu_shim::Sim3 a;  const Eigen::Quaterniond &q = g.rotation();  a.r[0] = q.x(), a.r[1] = q.y(), a.r[2] = q.z(),
//         a.r[3] = q.w();  for (int i = 0; i < 3; i++) a.t[i] = g.translation()[i];  a.s = g.scale();
//     g2o::Sim3 g(Eigen::Quaterniond(a.r[3], a.r[0], a.r[1], a.r[2]), Eigen::Vector3d(a.t[0], a.t[1], a.t[2]), a.s);
struct Sim3 {
    double r[4] = {0.0, 0.0, 0.0, 1.0};  // quaternion x, y, z, w
    double t[3] = {0.0, 0.0, 0.0};
    double s = 1.0;

    Sim3() = default;
    // g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s) over the floats of a cv::Mat (row-major 3x3, 3)
    Sim3(const float *R, const float *t_, float s_)
    {
        double m[9];
        for (int i = 0; i < 9; i++)
            m[i] = (double)R[i];
        const double td[3] = {(double)t_[0], (double)t_[1], (double)t_[2]};
        Set(m, td, (double)s_);
    }
    // from a row-major rotation matrix (Eigen's Quaterniond(Matrix3d), then normalised with w >= 0)
    void Set(const double m[9], const double t_[3], double s_)
    {
        double tr = m[0] + m[4] + m[8];
        if (tr > 0) {
            tr = std::sqrt(tr + 1.0);
            r[3] = 0.5 * tr;
            tr = 0.5 / tr;
            r[0] = (m[7] - m[5]) * tr, r[1] = (m[2] - m[6]) * tr, r[2] = (m[3] - m[1]) * tr;
        } else {
            int i = 0;
            if (m[4] > m[0])
                i = 1;
            if (m[8] > m[4 * i])
                i = 2;
            const int j = (i + 1) % 3, k = (j + 1) % 3;
            tr = std::sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
            r[i] = 0.5 * tr;
            tr = 0.5 / tr;
            r[3] = (m[3 * k + j] - m[3 * j + k]) * tr;
            r[j] = (m[3 * j + i] + m[3 * i + j]) * tr;
            r[k] = (m[3 * k + i] + m[3 * i + k]) * tr;
        }
        const double n = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]) * (r[3] < 0 ? -1.0 : 1.0);
        for (int i = 0; i < 4; i++)
            r[i] /= n;
        for (int i = 0; i < 3; i++)
            t[i] = t_[i];
        s = s_;
    }
    void RotationMatrix(double R[9]) const
    {
        const double x = r[0], y = r[1], z = r[2], w = r[3];
        R[0] = 1.0 - 2.0 * (y * y + z * z), R[1] = 2.0 * (x * y - z * w), R[2] = 2.0 * (x * z + y * w);
        R[3] = 2.0 * (x * y + z * w), R[4] = 1.0 - 2.0 * (x * x + z * z), R[5] = 2.0 * (y * z - x * w);
        R[6] = 2.0 * (x * z - y * w), R[7] = 2.0 * (y * z + x * w), R[8] = 1.0 - 2.0 * (x * x + y * y);
    }
};

// The rows of orbgpu_sim3_opt_problem from two key frames and the matches of key frame 1, exactly as Optimizer.cc:1099-1137
// walks them (O1): valid[i] iff vpMatches1[i] and KF1's own map point i exist, neither is bad, and the match has an index
// i2 >= 0 in KF2; then obs1 = mvKeysUn1[i] (index i itself, :1142), obs2 = mvKeysUn2[i2] (:1159).  in_range[i]: both octaves
// lie inside pKF1's sigma table -- what the library requires of a correspondence on top of valid[i].
template <typename KeyFrameT, typename MapPointT> struct Sim3OptRows {
    std::vector<uint8_t> valid, in_range;
    std::vector<int32_t> o1, o2;
    std::vector<float> x1, x2, k1, k2;

    template <typename WorldPos>
    Sim3OptRows(KeyFrameT *pKF1, KeyFrameT *pKF2, const std::vector<MapPointT *> &vpMatches1, WorldPos world_pos)
    {
        const size_t N = vpMatches1.size();
        const std::vector<MapPointT *> vpMapPoints1 = pKF1->GetMapPointMatches();
        const int nlevels = (int)std::min(pKF1->mvInvLevelSigma2.size(), (size_t)ORBGPU_MAX_LEVELS);
        valid.assign(N + 1, 0), in_range.assign(N + 1, 0), o1.assign(N + 1, 0), o2.assign(N + 1, 0);
        x1.assign(3 * N + 3, 0.f), x2.assign(3 * N + 3, 0.f), k1.assign(2 * N + 2, 0.f), k2.assign(2 * N + 2, 0.f);
        for (size_t i = 0; i < N; i++) {
            MapPointT *pMP2 = vpMatches1[i];
            if (!pMP2)
                continue;
            MapPointT *pMP1 = i < vpMapPoints1.size() ? vpMapPoints1[i] : nullptr;
            const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (!pMP1 || pMP1->isBad() || pMP2->isBad() || i2 < 0)
                continue;
            valid[i] = 1;
            o1[i] = pKF1->mvKeysUn[i].octave, o2[i] = pKF2->mvKeysUn[i2].octave;
            in_range[i] = o1[i] >= 0 && o1[i] < nlevels && o2[i] >= 0 && o2[i] < nlevels;
            k1[2 * i] = pKF1->mvKeysUn[i].pt.x, k1[2 * i + 1] = pKF1->mvKeysUn[i].pt.y;
            k2[2 * i] = pKF2->mvKeysUn[i2].pt.x, k2[2 * i + 1] = pKF2->mvKeysUn[i2].pt.y;
            std::memcpy(&x1[3 * i], world_pos(pMP1), 12);
            std::memcpy(&x2[3 * i], world_pos(pMP2), 12);
        }
        valid.resize(N), in_range.resize(N);  // the arrays keep one spare row so that data() is never null
    }
};

// What the graphs of the two bundle adjustments share: the arrays of the library's problem, the pose rows, and the edges --
// per point row, its observations in the order of the map GetObservations() returns.  An observer that is in no pose row
// (the reference reads through a null vertex there), or an octave outside that key frame's sigma table, keeps its edge with
// pose / octave -1: the library skips and counts it.  Every array but fixed_flag keeps one spare row, and fixed_flag at
// least one element, so that data() is never null.
template <typename KeyFrameT, typename MapPointT> struct BAGraphBase {
    std::vector<KeyFrameT *> edge_kf;
    std::vector<MapPointT *> points, edge_mp;
    std::vector<int32_t> edge_point, edge_pose, edge_octave;
    std::vector<float> edge_xy, edge_ur, Tcw, cam, inv_sigma2, world_pos;
    std::vector<uint8_t> fixed_flag;
    int nlevels = 1;

  protected:
    std::map<KeyFrameT *, int32_t> row;
    size_t n_rows = 0;

    // pose rows row_kf(0 .. P-1): pose, camera, sigma table (as many levels as `levels_of` has, if there is one); the first
    // n_flags of them carry a fixed flag, set iff mnId == 0
    template <typename RowKF, typename Access> void fill_poses(size_t P, RowKF row_kf, size_t n_flags, KeyFrameT *levels_of, Access &access)
    {
        if (levels_of)
            nlevels = (int)std::max<size_t>(1, std::min(levels_of->mvInvLevelSigma2.size(), (size_t)ORBGPU_MAX_LEVELS));
        Tcw.assign(16 * P + 16, 0.f), cam.assign(5 * P + 5, 0.f), inv_sigma2.assign((size_t)nlevels * (P + 1), 0.f);
        fixed_flag.assign(std::max<size_t>(n_flags, 1), 0);  // one per flagged row: callers walk the vector
        n_rows = P;
        for (size_t i = 0; i < P; i++) {
            KeyFrameT *k = row_kf(i);
            row[k] = (int32_t)i;
            std::memcpy(&Tcw[16 * i], access.pose(k), 64);
            const float c[5] = {k->fx, k->fy, k->cx, k->cy, k->mbf};
            std::memcpy(&cam[5 * i], c, sizeof(c));
            for (size_t l = 0; l < std::min(k->mvInvLevelSigma2.size(), (size_t)nlevels); l++)
                inv_sigma2[(size_t)nlevels * i + l] = k->mvInvLevelSigma2[l];
            if (i < n_flags)
                fixed_flag[i] = k->mnId == 0;
        }
    }

    // the point rows' positions and their edges; skipped(pKFi): this observer is no edge
    template <typename Skipped, typename Access> void gather_edges(Skipped skipped, Access &access)
    {
        world_pos.assign(3 * points.size() + 3, 0.f);
        for (size_t j = 0; j < points.size(); j++) {
            MapPointT *pMP = points[j];
            std::memcpy(&world_pos[3 * j], access.world_pos(pMP), 12);
            const auto observations = pMP->GetObservations();
            for (const auto &ob : observations) {
                KeyFrameT *pKFi = ob.first;
                if (skipped(pKFi))
                    continue;
                const auto &kpUn = pKFi->mvKeysUn[ob.second];
                const auto it = row.find(pKFi);
                const bool has_sigma = kpUn.octave >= 0 && (size_t)kpUn.octave < pKFi->mvInvLevelSigma2.size();
                edge_kf.push_back(pKFi), edge_mp.push_back(pMP);
                edge_point.push_back((int32_t)j), edge_pose.push_back(it == row.end() ? -1 : it->second);
                edge_octave.push_back(has_sigma ? kpUn.octave : -1);
                edge_xy.push_back(kpUn.pt.x), edge_xy.push_back(kpUn.pt.y), edge_ur.push_back(pKFi->mvuRight[ob.second]);
            }
        }
    }

    // the host part both problems have; valid while the graph lives
    template <typename Problem> Problem HostPart() const
    {
        Problem p;
        std::memset(&p, 0, sizeof(p));
        p.n_poses = (int32_t)n_rows, p.n_points = (int32_t)points.size(), p.n_edges = (int32_t)edge_point.size();
        p.nlevels = nlevels;
        p.Tcw = Tcw.data(), p.fixed = fixed_flag.data(), p.cam = cam.data(), p.inv_level_sigma2 = inv_sigma2.data();
        p.world_pos = world_pos.data(), p.edge_point = edge_point.data(), p.edge_pose = edge_pose.data();
        p.edge_octave = edge_octave.data(), p.edge_xy = edge_xy.data(), p.edge_u_right = edge_ur.data();
        return p;
    }
};

// The graph of Optimizer::LocalBundleAdjustment as orbgpu_local_ba takes it: the breadth-first gathering of
// Optimizer.cc:455-504 (it walks pointers, so it stays on the host) in the reference's list order, then the vertices and
// edges of :522-652.  Pose rows: lLocalKeyFrames, then lFixedCameras; point rows: lLocalMapPoints.  Marks mnBALocalForKF /
// mnBAFixedForKF as the reference does.  An observation by a key frame that is bad is no edge (:589).
template <typename KeyFrameT, typename MapPointT> struct LocalBAGraph : BAGraphBase<KeyFrameT, MapPointT> {
    std::vector<KeyFrameT *> local, fixed;

    template <typename Access> LocalBAGraph(KeyFrameT *pKF, Access &access)
    {
        local.push_back(pKF);
        pKF->mnBALocalForKF = pKF->mnId;
        const std::vector<KeyFrameT *> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
        for (KeyFrameT *pKFi : vNeighKFs) {
            pKFi->mnBALocalForKF = pKF->mnId;
            if (!pKFi->isBad())
                local.push_back(pKFi);
        }
        for (KeyFrameT *pKFi : local) {
            const std::vector<MapPointT *> vpMPs = pKFi->GetMapPointMatches();
            for (MapPointT *pMP : vpMPs)
                if (pMP && !pMP->isBad() && pMP->mnBALocalForKF != pKF->mnId) {
                    this->points.push_back(pMP);
                    pMP->mnBALocalForKF = pKF->mnId;
                }
        }
        for (MapPointT *pMP : this->points) {
            const auto observations = pMP->GetObservations();
            for (const auto &ob : observations) {
                KeyFrameT *pKFi = ob.first;
                if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
                    pKFi->mnBAFixedForKF = pKF->mnId;
                    if (!pKFi->isBad())
                        fixed.push_back(pKFi);
                }
            }
        }
        this->fill_poses(local.size() + fixed.size(), [this](size_t i) { return i < local.size() ? local[i] : fixed[i - local.size()]; },
                         local.size(), pKF, access);
        this->gather_edges([](KeyFrameT *pKFi) { return pKFi->isBad(); }, access);
    }

    orbgpu_local_ba_problem Problem() const
    {
        orbgpu_local_ba_problem p = this->template HostPart<orbgpu_local_ba_problem>();
        p.n_local = (int32_t)local.size();
        return p;
    }
};

// The graph of Optimizer::BundleAdjustment (Optimizer.cc:68-184) as orbgpu_bundle_adjustment takes it.  Pose rows: vpKFs in
// order without the bad ones, fixed iff mnId == 0; maxKFid over those rows; point rows: vpMP in order without the bad
// ones; no edge for an observer that is bad or whose mnId > maxKFid (:109).  A point whose every observation is skipped
// comes back not included.
template <typename KeyFrameT, typename MapPointT> struct FullBAGraph : BAGraphBase<KeyFrameT, MapPointT> {
    std::vector<KeyFrameT *> rows;
    long unsigned int maxKFid = 0;

    template <typename Access>
    FullBAGraph(const std::vector<KeyFrameT *> &vpKFs, const std::vector<MapPointT *> &vpMP, Access &access)
    {
        for (KeyFrameT *pKF : vpKFs) {
            if (pKF->isBad())
                continue;
            rows.push_back(pKF);
            if (pKF->mnId > maxKFid)
                maxKFid = pKF->mnId;
        }
        this->fill_poses(rows.size(), [this](size_t i) { return rows[i]; }, rows.size(), rows.empty() ? nullptr : rows[0], access);
        for (MapPointT *pMP : vpMP)
            if (!pMP->isBad())
                this->points.push_back(pMP);
        this->gather_edges([this](KeyFrameT *pKFi) { return pKFi->isBad() || pKFi->mnId > maxKFid; }, access);
    }

    orbgpu_bundle_adjustment_problem Problem(int nIterations, bool bRobust) const
    {
        orbgpu_bundle_adjustment_problem p = this->template HostPart<orbgpu_bundle_adjustment_problem>();
        p.n_iterations = nIterations, p.robust = bRobust ? 1 : 0;
        return p;
    }
};

// The graph of Optimizer::OptimizeEssentialGraph (Optimizer.cc:796-983) as orbgpu_essential_graph takes it (G1).  Vertex
// rows: pMap->GetAllKeyFrames() in order without the bad ones; Scw[v] = CorrectedSim3[pKF] if present, else Sim3(Rcw, tcw, 1)
// of its pose (:818-832); Snc[v] = NonCorrectedSim3[pKF] if present, else Scw[v] -- which is what every "find in
// NonCorrectedSim3, else vScw" of :894-967 reads; fixed iff pKF == pLoopKF.  Edges in the reference's order: first the loop
// connections (kind 0, :852-880), then per key frame its spanning-tree edge, its older loop edges and its strong
// covisibility edges (kind 1, :883-983); i is vertex 0 (the key frame the loop is over), j vertex 1.  A key frame that is
// in no row (a bad one: the reference reads through a null vertex there) keeps its edge with row -1: the library skips
// and counts it.  Point rows: pMap->GetAllMapPoints() without the bad ones, each with the row of mnCorrectedReference if
// pCurKF corrected it, else of its reference key frame (:1023-1032); -1 when that key frame has no row.
template <typename KeyFrameT, typename MapPointT> struct EssentialGraphT {
    std::vector<KeyFrameT *> rows;
    std::vector<MapPointT *> points;
    std::vector<double> Scw, Snc;
    std::vector<uint8_t> fixed_flag;
    std::vector<int32_t> edge_i, edge_j, edge_kind, point_ref;
    std::vector<float> world_pos;
    std::map<unsigned long, int32_t> row_of_id;

    int32_t Row(unsigned long id) const
    {
        const auto it = row_of_id.find(id);
        return it == row_of_id.end() ? -1 : it->second;
    }

    template <typename MapT, typename PoseMap, typename Connections, typename Access>
    EssentialGraphT(MapT *pMap, KeyFrameT *pLoopKF, KeyFrameT *pCurKF, const PoseMap &NonCorrectedSim3,
                    const PoseMap &CorrectedSim3, const Connections &LoopConnections, Access &access)
    {
        const auto vpKFs = pMap->GetAllKeyFrames();
        const auto vpMPs = pMap->GetAllMapPoints();
        const int minFeat = 100;
        auto put = [](std::vector<double> &to, const Sim3 &S) {
            to.insert(to.end(), S.r, S.r + 4), to.insert(to.end(), S.t, S.t + 3), to.push_back(S.s);
        };
        // Set KeyFrame vertices
        for (KeyFrameT *pKF : vpKFs) {
            if (pKF->isBad())
                continue;
            row_of_id[pKF->mnId] = (int32_t)rows.size();
            rows.push_back(pKF);
            const auto it = CorrectedSim3.find(pKF);
            if (it != CorrectedSim3.end()) {
                put(Scw, it->second);
            } else {
                double S[8];
                check(orbgpu_sim3_from_pose(access.pose(pKF), S), "Optimizer::OptimizeEssentialGraph");
                Scw.insert(Scw.end(), S, S + 8);
            }
            const auto itn = NonCorrectedSim3.find(pKF);
            if (itn != NonCorrectedSim3.end())
                put(Snc, itn->second);
            else
                Snc.insert(Snc.end(), Scw.end() - 8, Scw.end());
            fixed_flag.push_back(pKF == pLoopKF);
        }
        auto edge = [this](unsigned long idi, unsigned long idj, int kind) {
            edge_i.push_back(Row(idi)), edge_j.push_back(Row(idj)), edge_kind.push_back(kind);
        };
        std::set<std::pair<unsigned long, unsigned long>> sInsertedEdges;
        // Set Loop edges
        for (const auto &mit : LoopConnections) {
            KeyFrameT *pKF = mit.first;
            const unsigned long nIDi = pKF->mnId;
            for (KeyFrameT *pKFj : mit.second) {
                const unsigned long nIDj = pKFj->mnId;
                if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(pKFj) < minFeat)
                    continue;
                edge(nIDi, nIDj, 0);
                sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
            }
        }
        // Set normal edges
        for (KeyFrameT *pKF : vpKFs) {
            const unsigned long nIDi = pKF->mnId;
            KeyFrameT *pParentKF = pKF->GetParent();
            if (pParentKF)  // Spanning tree edge
                edge(nIDi, pParentKF->mnId, 1);
            const auto sLoopEdges = pKF->GetLoopEdges();  // Loop edges
            for (KeyFrameT *pLKF : sLoopEdges)
                if (pLKF->mnId < pKF->mnId)
                    edge(nIDi, pLKF->mnId, 1);
            const auto vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);  // Covisibility graph edges
            for (KeyFrameT *pKFn : vpConnectedKFs) {
                if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                    if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                        if (sInsertedEdges.count(std::make_pair(std::min<unsigned long>(pKF->mnId, pKFn->mnId),
                                                                std::max<unsigned long>(pKF->mnId, pKFn->mnId))))
                            continue;
                        edge(nIDi, pKFn->mnId, 1);
                    }
                }
            }
        }
        // the points and the row each is corrected through
        for (MapPointT *pMP : vpMPs) {
            if (pMP->isBad())
                continue;
            points.push_back(pMP);
            const float *x = access.world_pos(pMP);
            world_pos.insert(world_pos.end(), x, x + 3);
            if (pMP->mnCorrectedByKF == pCurKF->mnId) {
                point_ref.push_back(Row(pMP->mnCorrectedReference));
            } else {
                KeyFrameT *pRefKF = pMP->GetReferenceKeyFrame();
                point_ref.push_back(pRefKF ? Row(pRefKF->mnId) : -1);
            }
        }
    }

    // the host part of the library's problem; valid while the graph lives
    orbgpu_essential_graph_problem Problem(bool bFixScale, int nIterations = 20) const
    {
        orbgpu_essential_graph_problem p;
        std::memset(&p, 0, sizeof(p));
        p.n_vertices = (int32_t)rows.size(), p.n_edges = (int32_t)edge_i.size();
        p.n_iterations = nIterations, p.fix_scale = bFixScale ? 1 : 0;
        p.Scw = Scw.data(), p.Snc = Snc.data(), p.fixed = fixed_flag.data();
        p.edge_i = edge_i.data(), p.edge_j = edge_j.data(), p.edge_kind = edge_kind.data();
        return p;
    }
};

template <typename FrameT, typename MapPointT> class OptimizerT {
  public:
    // host arrays: one upload per call
    template <typename TcwOf, typename WorldPos, typename SetPose>
    static int PoseOptimization(FrameT *pFrame, TcwOf Tcw, WorldPos world_pos, SetPose set_pose, int device_id = 0,
                                orbgpu_pose_result *result = nullptr)
    {
        FrameT &F = *pFrame;
        const int n = F.N;
        std::vector<float> x(n), y(n), ur(n), wp(3 * (size_t)n, 0.f);
        std::vector<int32_t> oct(n);
        std::vector<uint8_t> has(n), out(n);
        for (int i = 0; i < n; i++) {
            x[i] = F.mvKeysUn[i].pt.x, y[i] = F.mvKeysUn[i].pt.y, oct[i] = F.mvKeysUn[i].octave, ur[i] = F.mvuRight[i];
            MapPointT *p = F.mvpMapPoints[i];
            has[i] = p != nullptr;
            out[i] = F.mvbOutlier[i];
            if (p) {
                const float *w = world_pos(p);
                wp[3 * (size_t)i] = w[0], wp[3 * (size_t)i + 1] = w[1], wp[3 * (size_t)i + 2] = w[2];
            }
        }
        orbgpu_frame_view v{};
        v.n = n, v.kp_x = x.data(), v.kp_y = y.data(), v.kp_octave = oct.data(), v.u_right = ur.data();
        v.nlevels = (int32_t)F.mvInvLevelSigma2.size();
        float T[16];
        std::memcpy(T, Tcw(F), sizeof(T));
        int32_t inliers = 0;
        check(orbgpu_pose_optimization(&v, has.data(), wp.data(), T, F.mvInvLevelSigma2.data(), F.fx, F.fy, F.cx, F.cy, F.mbf,
                                       out.data(), &inliers, result, device_id),
              "Optimizer::PoseOptimization");
        for (int i = 0; i < n; i++)
            if (has[i])
                F.mvbOutlier[i] = out[i] != 0;
        set_pose(F, T);
        return inliers;
    }

    // device-resident frame + MapPoint table: ids and the pose go up, mvbOutlier and the pose come back
    template <typename TcwOf, typename SetPose>
    static int PoseOptimization(FrameT *pFrame, const DeviceFrameT<FrameT> &dF, MapPointTableT<MapPointT> &table, TcwOf Tcw,
                                SetPose set_pose, orbgpu_pose_result *result = nullptr)
    {
        FrameT &F = *pFrame;
        const int n = F.N;
        std::vector<int64_t> ids(n);
        std::vector<uint8_t> out(n);
        for (int i = 0; i < n; i++) {
            ids[i] = F.mvpMapPoints[i] ? (int64_t)F.mvpMapPoints[i]->mnId : -1;
            out[i] = F.mvbOutlier[i];
        }
        float T[16];
        std::memcpy(T, Tcw(F), sizeof(T));
        int32_t inliers = 0;
        {
            std::lock_guard<std::mutex> table_lock(table.mutex());
            check(orbgpu_pose_optimization_table(dF.handle(), table.handle(), ids.data(), T, F.mvInvLevelSigma2.data(), F.fx,
                                                 F.fy, F.cx, F.cy, F.mbf, out.data(), &inliers, result),
                  "Optimizer::PoseOptimization(table)");
        }
        for (int i = 0; i < n; i++)
            if (ids[i] >= 0)
                F.mvbOutlier[i] = out[i] != 0;
        set_pose(F, T);
        return inliers;
    }

    // Optimizer::OptimizeSim3 (include/Optimizer.h:58, src/Optimizer.cc:1054-1241): refines S12 over the matches of a loop
    // candidate.  Side effects as in the reference: vpMatches1[i] = NULL for every correspondence the optimisation
    // clears, S12 replaced by the refined Sim3 (left as it came when fewer than 10 correspondences survive stage 1), return
    // value = inliers.  The conventions are O1-O9 of include/orbgpu.h ("g2o unpinned").  KeyFrameT needs
    // GetMapPointMatches(), mvKeysUn, mvInvLevelSigma2 (pKF1's table serves both key frames: one extractor), fx, fy, cx,
    // cy; MapPointT isBad() and GetIndexInKeyFrame(KeyFrameT *).  pose(pKF) returns the 16 floats of Tcw, world_pos(pMP) 3
    // floats.  R12_float: the float rotation S12 was built from (ComputeSim3 holds it: the solver's R); when given it is
    // passed on as it is, so the entry state is the reference's bit for bit -- otherwise the matrix of S12.r is rounded.
    // result (optional) also carries Scw = toCvMat(S12 * Smw), what LoopClosing.cc:334-336 computes next.
    template <typename KeyFrameT, typename PoseOf, typename WorldPos>
    static int OptimizeSim3(KeyFrameT *pKF1, KeyFrameT *pKF2, std::vector<MapPointT *> &vpMatches1, Sim3 &S12, const float th2,
                            const bool bFixScale, PoseOf pose, WorldPos world_pos, int device_id = 0,
                            orbgpu_sim3_opt_result *result = nullptr, const float *R12_float = nullptr)
    {
        const Sim3OptRows<KeyFrameT, MapPointT> rows(pKF1, pKF2, vpMatches1, world_pos);
        orbgpu_sim3_opt_problem p;
        std::memset(&p, 0, sizeof(p));
        p.n1 = (int32_t)rows.valid.size();
        p.nlevels = (int32_t)std::min(pKF1->mvInvLevelSigma2.size(), (size_t)ORBGPU_MAX_LEVELS);
        p.valid = rows.valid.data(), p.Xw1 = rows.x1.data(), p.Xw2 = rows.x2.data();
        p.octave1 = rows.o1.data(), p.octave2 = rows.o2.data(), p.kp1_xy = rows.k1.data(), p.kp2_xy = rows.k2.data();
        std::memcpy(p.T1w, pose(pKF1), 64);
        std::memcpy(p.T2w, pose(pKF2), 64);
        p.fx1 = pKF1->fx, p.fy1 = pKF1->fy, p.cx1 = pKF1->cx, p.cy1 = pKF1->cy;
        p.fx2 = pKF2->fx, p.fy2 = pKF2->fy, p.cx2 = pKF2->cx, p.cy2 = pKF2->cy;
        for (int l = 0; l < p.nlevels; l++)
            p.inv_level_sigma2[l] = pKF1->mvInvLevelSigma2[l];
        if (R12_float) {
            std::memcpy(p.R12, R12_float, sizeof(p.R12));
        } else {
            double R[9];
            S12.RotationMatrix(R);
            for (int i = 0; i < 9; i++)
                p.R12[i] = (float)R[i];
        }
        for (int i = 0; i < 3; i++)
            p.t12[i] = (float)S12.t[i];
        p.s12 = (float)S12.s;
        p.th2 = th2, p.fix_scale = bFixScale ? 1 : 0;
        std::vector<uint8_t> inlier(rows.valid.size() + 1, 0);
        int32_t inliers = 0;
        orbgpu_sim3_opt_result r;
        check(orbgpu_sim3_optimize(&p, inlier.data(), &inliers, &r, device_id), "Optimizer::OptimizeSim3");
        // rows that are no correspondence keep their 0 but are not touched: only correspondences can be cleared
        for (size_t i = 0; i < rows.valid.size(); i++)
            if (rows.valid[i] && rows.in_range[i] && inlier[i] == 0)
                vpMatches1[i] = static_cast<MapPointT *>(nullptr);
        if (r.stages == 2)
            S12.Set(r.R12_d, r.t12_d, r.s12_d);
        if (result)
            *result = r;
        return inliers;
    }

    // Optimizer::LocalBundleAdjustment (include/Optimizer.h:50, src/Optimizer.cc:453-778): the local key frames and the
    // points they see.  Side effects as in the reference: under pMap->mMutexMapUpdate, EraseMapPointMatch /
    // EraseObservation for every observation the final test rejects (its map point not bad by then, :720, :735), SetPose of
    // every local key frame, SetWorldPos + UpdateNormalAndDepth of every local point; nothing at all when *pbStopFlag is
    // set at the call (:655).  The flag is sampled once, at the call: a flag raised later does not reach the device
    // through this host flavour (orbgpu_local_ba_device takes a device-readable flag).  The conventions are L1-L12 of
    // include/orbgpu.h ("g2o unpinned").  KeyFrameT needs mnId, mnBALocalForKF, mnBAFixedForKF,
    // GetVectorCovisibleKeyFrames(), GetMapPointMatches(), isBad(), mvKeysUn, mvuRight, mvInvLevelSigma2, fx, fy, cx, cy,
    // mbf, EraseMapPointMatch(MapPointT *); MapPointT mnId, mnBALocalForKF, isBad(), GetObservations(),
    // EraseObservation(KeyFrameT *), UpdateNormalAndDepth(); MapT mMutexMapUpdate.  access: pose(pKF) the 16 floats of
    // Tcw, world_pos(pMP) 3 floats (both valid until the next call of the same accessor), set_pose(pKF, T),
    // set_world_pos(pMP, x); with a table also normal(pMP), min_dist(pMP), max_dist(pMP), read after
    // UpdateNormalAndDepth for the batched MapPointTableT::SetWorldPos.  Beyond the library's capacities
    // (ORBGPU_LBA_MAX_*) the call throws: the caller keeps its g2o path for such maps.
    template <typename KeyFrameT, typename MapT, typename Access>
    static void LocalBundleAdjustment(KeyFrameT *pKF, bool *pbStopFlag, MapT *pMap, Access access,
                                      MapPointTableT<MapPointT> *table = nullptr, int device_id = 0,
                                      orbgpu_local_ba_result *result = nullptr)
    {
        const LocalBAGraph<KeyFrameT, MapPointT> g(pKF, access);
        const orbgpu_local_ba_problem p = g.Problem();
        const size_t nl = g.local.size(), M = g.points.size(), E = g.edge_point.size();
        std::vector<float> T(16 * nl), X(3 * M + 3);
        std::vector<uint8_t> erase(E + 1, 0);
        const int32_t stop = pbStopFlag && *pbStopFlag ? 1 : 0;
        orbgpu_local_ba_result r;
        check(orbgpu_local_ba(&p, pbStopFlag ? &stop : nullptr, nullptr, T.data(), nullptr, X.data(), erase.data(), &r, device_id),
              "Optimizer::LocalBundleAdjustment");
        if (result)
            *result = r;
        if (r.stopped && r.rounds == 0)
            return;
        std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
        std::vector<MapPointT *> touched;
        for (size_t e = 0; e < E; e++)
            if (erase[e] && !g.edge_mp[e]->isBad()) {
                g.edge_kf[e]->EraseMapPointMatch(g.edge_mp[e]);
                g.edge_mp[e]->EraseObservation(g.edge_kf[e]);
                touched.push_back(g.edge_mp[e]);
            }
        for (size_t i = 0; i < nl; i++)
            access.set_pose(g.local[i], &T[16 * i]);
        for (size_t j = 0; j < M; j++) {
            access.set_world_pos(g.points[j], &X[3 * j]);
            g.points[j]->UpdateNormalAndDepth();
        }
        if (table) {
            if (!touched.empty())
                table->SetObservations(touched);
            table->SetWorldPos(g.points, access);
        }
    }

    // Optimizer::BundleAdjustment (include/Optimizer.h:41, src/Optimizer.cc:49-237): every key frame of vpKFs and every
    // point of vpMP in one optimize(nIterations).  Write-back as :190-235: with nLoopKF == 0 SetPose of every key frame
    // that is not bad, SetWorldPos + UpdateNormalAndDepth of every point that is not bad and was included (and the table's
    // batched SetWorldPos); otherwise set_pose_gba / set_world_pos_gba (mTcwGBA, mPosGBA) and mnBAGlobalForKF = nLoopKF on
    // both.  Not-included and bad entries are skipped.  The flag is sampled once, at the call, as for
    // LocalBundleAdjustment; when it is set nothing is written back (the reference's optimize(0 iterations) would write
    // the quaternion round trip of every estimate).  The spanning-tree propagation of LoopClosing.cc:672-733 walks
    // pointers and stays with the caller.  The conventions are B1-B7 of include/orbgpu.h ("g2o unpinned").  KeyFrameT
    // needs mnId, mnBAGlobalForKF, isBad(), mvKeysUn, mvuRight, mvInvLevelSigma2, fx, fy, cx, cy, mbf; MapPointT
    // mnBAGlobalForKF, isBad(), GetObservations(), UpdateNormalAndDepth().  access: pose, world_pos, set_pose,
    // set_world_pos as for LocalBundleAdjustment, plus set_pose_gba(pKF, T) and set_world_pos_gba(pMP, x); with a table
    // also normal, min_dist, max_dist.  Beyond the library's capacities (ORBGPU_BA_MAX_*) the call throws: the caller
    // keeps its g2o path for such maps.
    template <typename KeyFrameT, typename Access>
    static void BundleAdjustment(const std::vector<KeyFrameT *> &vpKFs, const std::vector<MapPointT *> &vpMP, int nIterations,
                                 bool *pbStopFlag, const unsigned long nLoopKF, const bool bRobust, Access access,
                                 MapPointTableT<MapPointT> *table = nullptr, int device_id = 0,
                                 orbgpu_bundle_adjustment_result *result = nullptr)
    {
        const FullBAGraph<KeyFrameT, MapPointT> g(vpKFs, vpMP, access);
        const orbgpu_bundle_adjustment_problem p = g.Problem(nIterations, bRobust);
        const size_t P = g.rows.size(), M = g.points.size();
        std::vector<float> T(16 * P + 16), X(3 * M + 3);
        std::vector<uint8_t> not_included(M + 1, 0);
        const int32_t stop = pbStopFlag && *pbStopFlag ? 1 : 0;
        orbgpu_bundle_adjustment_result r;
        check(orbgpu_bundle_adjustment(&p, pbStopFlag ? &stop : nullptr, nullptr, T.data(), nullptr, X.data(), not_included.data(),
                                       &r, device_id),
              "Optimizer::BundleAdjustment");
        if (result)
            *result = r;
        if (r.stopped)
            return;
        for (size_t i = 0; i < P; i++) {
            if (g.rows[i]->isBad())
                continue;
            if (nLoopKF == 0) {
                access.set_pose(g.rows[i], &T[16 * i]);
            } else {
                access.set_pose_gba(g.rows[i], &T[16 * i]);
                g.rows[i]->mnBAGlobalForKF = nLoopKF;
            }
        }
        std::vector<MapPointT *> moved;
        for (size_t j = 0; j < M; j++) {
            if (not_included[j] || g.points[j]->isBad())
                continue;
            if (nLoopKF == 0) {
                access.set_world_pos(g.points[j], &X[3 * j]);
                g.points[j]->UpdateNormalAndDepth();
                moved.push_back(g.points[j]);
            } else {
                access.set_world_pos_gba(g.points[j], &X[3 * j]);
                g.points[j]->mnBAGlobalForKF = nLoopKF;
            }
        }
        if (table && !moved.empty())
            table->SetWorldPos(moved, access);
    }

    // Optimizer::GlobalBundleAdjustemnt (Optimizer.cc:41-46, spelt as there): BundleAdjustment over pMap->GetAllKeyFrames()
    // and pMap->GetAllMapPoints().  Tracking.cc:963 calls it with (mpMap, 20), LoopClosing.cc:647 with
    // (mpMap, 20, &mbStopGBA, nLoopKF, false).
    template <typename MapT, typename Access>
    static void GlobalBundleAdjustemnt(MapT *pMap, int nIterations, bool *pbStopFlag, const unsigned long nLoopKF, const bool bRobust,
                                       Access access, MapPointTableT<MapPointT> *table = nullptr, int device_id = 0,
                                       orbgpu_bundle_adjustment_result *result = nullptr)
    {
        const auto vpKFs = pMap->GetAllKeyFrames();
        const std::vector<MapPointT *> vpMP = pMap->GetAllMapPoints();
        BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust, access, table, device_id, result);
    }

    // Optimizer::OptimizeEssentialGraph (include/Optimizer.h:52, src/Optimizer.cc:781-1044): the Sim3 pose graph of
    // LoopClosing::CorrectLoop (LoopClosing.cc:565) over every key frame of the map, optimize(20), then SetPose of every key
    // frame with [R t / s; 0 1] (:992-1010) and SetWorldPos + UpdateNormalAndDepth of every point that is not bad, moved
    // through its reference row (:1013-1043).  The edge gathering of :847-983 is EssentialGraphT's, statement for
    // statement; NonCorrectedSim3 / CorrectedSim3 are LoopClosing::KeyFrameAndPose with the stand-in Sim3 above in the place
    // of g2o::Sim3 (a std::map<KeyFrameT *, Sim3> or anything with its find / end), LoopConnections the map<KeyFrame *,
    // set<KeyFrame *>> of :556.  The reference has no stop flag here (G9): none is passed.  A point whose reference key
    // frame has no row is left as it came (the reference would read vScw of a bad key frame's id).  The caller holds
    // pMap->mMutexMapUpdate for the write-back, as :990 does.  The conventions are G1-G12 of include/orbgpu.h ("g2o
    // unpinned").  KeyFrameT needs mnId, isBad(), GetParent(), GetLoopEdges(), GetCovisiblesByWeight(), hasChild(),
    // GetWeight(); MapPointT isBad(), mnCorrectedByKF, mnCorrectedReference, GetReferenceKeyFrame(), UpdateNormalAndDepth();
    // access: pose(pKF) (16 floats), world_pos(pMP) (3 floats), set_pose(pKF, T), set_world_pos(pMP, x); with a table also
    // normal, min_dist, max_dist.  Beyond the library's capacities (ORBGPU_EG_MAX_*, the envelope included) the call
    // throws: the caller keeps its g2o path for such maps.
    template <typename MapT, typename KeyFrameT, typename PoseMap, typename Connections, typename Access>
    static void OptimizeEssentialGraph(MapT *pMap, KeyFrameT *pLoopKF, KeyFrameT *pCurKF, const PoseMap &NonCorrectedSim3,
                                       const PoseMap &CorrectedSim3, const Connections &LoopConnections, const bool &bFixScale,
                                       Access access, MapPointTableT<MapPointT> *table = nullptr, int device_id = 0,
                                       orbgpu_essential_graph_result *result = nullptr)
    {
        const EssentialGraphT<KeyFrameT, MapPointT> g(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, access);
        const orbgpu_essential_graph_problem p = g.Problem(bFixScale);
        const size_t V = g.rows.size(), M = g.points.size();
        std::vector<float> T(16 * V + 16), X(g.world_pos);
        X.resize(3 * M + 3);
        orbgpu_essential_graph_result r;
        check(orbgpu_essential_graph(&p, nullptr, nullptr, T.data(), (int32_t)M, X.data(), g.point_ref.data(), X.data(), &r, device_id),
              "Optimizer::OptimizeEssentialGraph");
        if (result)
            *result = r;
        for (size_t i = 0; i < V; i++)
            access.set_pose(g.rows[i], &T[16 * i]);
        std::vector<MapPointT *> moved;
        for (size_t j = 0; j < M; j++) {
            if (g.point_ref[j] < 0)
                continue;
            access.set_world_pos(g.points[j], &X[3 * j]);
            g.points[j]->UpdateNormalAndDepth();
            moved.push_back(g.points[j]);
        }
        if (table && !moved.empty())
            table->SetWorldPos(moved, access);
    }
};

// --------------------------------------------------------------------------------------------
// Sim3Solver (reference include/Sim3Solver.h, src/Sim3Solver.cc): the Sim3 of a loop candidate.  The conventions are H1-H8
// of include/orbgpu.h.
// --------------------------------------------------------------------------------------------
// DUtils::Random::RandomInt over a caller's rand(): int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min
template <typename Rand> inline int Sim3ReferenceRandomInt(Rand rand_fn, int rand_max, int min, int max)
{
    const int d = max - min + 1;
    return int(((double)rand_fn() / ((double)rand_max + 1.0)) * d) + min;
}

// The draw of Sim3Solver::iterate (:163-177) replayed for `iterations` iterations over n correspondences: it overwrites
// vAvailableIndices[idx], not [randi], so one point can be drawn twice, and after the pop it may write at position size()
// or size() + 1 -- here into an array that keeps n entries.  random_int(min, max) is called three times per iteration.
// n < 3 (the reference would call RandomInt(0, -1) and read an empty vector) and a random_int outside [min, max] are
// refused with std::invalid_argument, as tests/sim3_model.py refuses them.
template <typename RandomInt> inline std::vector<int32_t> Sim3SampleTriples(int n, int iterations, RandomInt random_int)
{
    if (n < 3)
        throw std::invalid_argument("Sim3SampleTriples: fewer than 3 correspondences");
    std::vector<int32_t> out((size_t)std::max(iterations, 0) * 3, 0);
    std::vector<int32_t> avail((size_t)n);
    for (int it = 0; it < iterations; it++) {
        for (int i = 0; i < n; i++)
            avail[i] = i;
        int size = n;
        for (int i = 0; i < 3; i++) {
            const int randi = random_int(0, size - 1);
            if (randi < 0 || randi >= size)
                throw std::invalid_argument("Sim3SampleTriples: RandomInt outside [min, max]");
            const int idx = avail[randi];
            out[3 * (size_t)it + i] = idx;
            avail[idx] = avail[size - 1];
            size--;
        }
    }
    return out;
}

// KeyFrameT needs GetMapPointMatches(), mvKeysUn, mvLevelSigma2, fx, fy, cx, cy; MapPointT isBad() and
// GetIndexInKeyFrame(KeyFrameT *).  pose(pKF) returns the 16 floats of Tcw, world_pos(pMP) 3 floats (both valid during the
// constructor); random_int(min, max) stands for DUtils::Random::RandomInt.  The triples of all max_its iterations are
// drawn up front, the library is called once (orbgpu_sim3_solve_all), on the first iterate, and every iterate(n, ...) is
// then served from the stored counts, masks and transformations with the reference's persistent state (mnIterations,
// mnBestInliers).  With fewer than 3 kept correspondences no minimal set exists (the reference reads an empty vector
// there): iterate reports bNoMore, whatever minInliers is.
template <typename KeyFrameT, typename MapPointT> class Sim3SolverT {
  public:
    template <typename PoseOf, typename WorldPos, typename RandomInt>
    Sim3SolverT(KeyFrameT *pKF1, KeyFrameT *pKF2, const std::vector<MapPointT *> &vpMatched12, bool bFixScale, PoseOf pose,
                WorldPos world_pos, RandomInt random_int, int device_id = 0)
        : random_int_(random_int), device_id_(device_id), fix_scale_(bFixScale)
    {
        const std::vector<MapPointT *> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
        mN1 = (int)vpMatched12.size();
        valid_.assign((size_t)mN1, 0), o1_.assign((size_t)mN1, 0), o2_.assign((size_t)mN1, 0);
        x1_.assign(3 * (size_t)mN1, 0.f), x2_.assign(3 * (size_t)mN1, 0.f);
        nlevels_ = (int)std::min(pKF1->mvLevelSigma2.size(), (size_t)ORBGPU_MAX_LEVELS);
        N = 0;
        for (int i1 = 0; i1 < mN1; i1++) {
            MapPointT *pMP1 = vpKeyFrameMP1[i1], *pMP2 = vpMatched12[i1];
            if (!pMP2 || !pMP1 || pMP1->isBad() || pMP2->isBad())
                continue;
            const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1), indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (indexKF1 < 0 || indexKF2 < 0)
                continue;
            valid_[i1] = 1;
            o1_[i1] = pKF1->mvKeysUn[indexKF1].octave, o2_[i1] = pKF2->mvKeysUn[indexKF2].octave;
            std::memcpy(&x1_[3 * (size_t)i1], world_pos(pMP1), 12);
            std::memcpy(&x2_[3 * (size_t)i1], world_pos(pMP2), 12);
            if (o1_[i1] >= 0 && o1_[i1] < nlevels_ && o2_[i1] >= 0 && o2_[i1] < nlevels_)
                N++;  // H1: the rows the library keeps
        }
        std::memset(&p_, 0, sizeof(p_));
        std::memcpy(p_.T1w, pose(pKF1), 64);
        std::memcpy(p_.T2w, pose(pKF2), 64);
        p_.fx1 = pKF1->fx, p_.fy1 = pKF1->fy, p_.cx1 = pKF1->cx, p_.cy1 = pKF1->cy;
        p_.fx2 = pKF2->fx, p_.fy2 = pKF2->fy, p_.cx2 = pKF2->cx, p_.cy2 = pKF2->cy;
        for (int l = 0; l < nlevels_; l++)
            p_.level_sigma2[l] = pKF1->mvLevelSigma2[l];
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)
    {
        mRansacProb = probability, mRansacMinInliers = minInliers;
        int32_t its = 1;
        check(orbgpu_sim3_ransac_iterations(N, probability, minInliers, maxIterations, &its), "Sim3Solver::SetRansacParameters");
        mRansacMaxIts = its;
        mnIterations = 0;
        solved_ = false;  // the triples depend on max_its
    }

    // cv::Mat-free form of iterate: returns the accepted iteration's T12 (16 floats, valid until the next call) or nullptr
    const float *iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers)
    {
        bNoMore = false;
        vbInliers.assign((size_t)mN1, false);
        nInliers = 0;
        if (N < mRansacMinInliers || N < 3) {
            bNoMore = true;
            return nullptr;
        }
        if (!solved_)
            Solve();
        int nCurrentIterations = 0;
        while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
            nCurrentIterations++;
            const int it = mnIterations++;
            if (counts_[it] >= mnBestInliers) {
                mnBestInliers = counts_[it], best_ = it;
                if (counts_[it] > mRansacMinInliers) {
                    nInliers = counts_[it];
                    const size_t words = ((size_t)mN1 + 63) / 64;
                    for (int i = 0; i < mN1; i++)
                        vbInliers[i] = (masks_[(size_t)it * words + ((size_t)i >> 6)] >> (i & 63)) & 1u;
                    return &T12_[16 * (size_t)it];
                }
            }
        }
        if (mnIterations >= mRansacMaxIts)
            bNoMore = true;
        return nullptr;
    }

    const float *find(std::vector<bool> &vbInliers12, int &nInliers)
    {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
    }

    // of the best iteration so far (mBestRotation ...); nullptr / 0 before any iteration
    const float *GetEstimatedRotation() const { return best_ < 0 ? nullptr : &R_[9 * (size_t)best_]; }
    const float *GetEstimatedTranslation() const { return best_ < 0 ? nullptr : &t_[3 * (size_t)best_]; }
    float GetEstimatedScale() const { return best_ < 0 ? 0.f : s_[(size_t)best_]; }

    int NumCorrespondences() const { return N; }
    int MaxIterations() const { return mRansacMaxIts; }
    int Iterations() const { return mnIterations; }
    const std::vector<int32_t> &Triples() const { return triples_; }

    // The answer of the library for hypotheses [0, max_its): what Solve() stores.  Public so that a test can serve
    // iterate() from recorded counts without a device.
    void LoadResults(const int32_t *counts, const uint64_t *masks, const float *R, const float *t, const float *s,
                     const float *T12)
    {
        const size_t H = (size_t)mRansacMaxIts, words = ((size_t)mN1 + 63) / 64;
        counts_.assign(counts, counts + H);
        masks_.assign(masks, masks + H * words);
        R_.assign(R, R + 9 * H), t_.assign(t, t + 3 * H), s_.assign(s, s + H), T12_.assign(T12, T12 + 16 * H);
        solved_ = true;
    }

    void DrawTriples() { triples_ = Sim3SampleTriples(N, mRansacMaxIts, random_int_); }

  private:
    void Solve()
    {
        DrawTriples();
        const size_t H = (size_t)mRansacMaxIts, words = ((size_t)mN1 + 63) / 64;
        p_.n1 = mN1, p_.n_hyp = (int32_t)H;
        p_.valid = valid_.data(), p_.Xw1 = x1_.data(), p_.Xw2 = x2_.data(), p_.octave1 = o1_.data(), p_.octave2 = o2_.data();
        p_.triples = triples_.data();
        p_.nlevels = nlevels_, p_.fix_scale = fix_scale_, p_.min_inliers = mRansacMinInliers;
        p_.max_iterations = mRansacMaxIts, p_.probability = mRansacProb;
        counts_.assign(H, 0), masks_.assign(H * words, 0);
        R_.assign(9 * H, 0.f), t_.assign(3 * H, 0.f), s_.assign(H, 0.f), T12_.assign(16 * H, 0.f);
        orbgpu_sim3_result r;
        check(orbgpu_sim3_solve_all(&p_, counts_.data(), R_.data(), t_.data(), s_.data(), T12_.data(), masks_.data(), &r,
                                    device_id_),
              "Sim3Solver");
        solved_ = true;
    }

    std::function<int(int, int)> random_int_;
    int device_id_ = 0;
    bool fix_scale_ = false, solved_ = false;
    int mN1 = 0, N = 0, nlevels_ = 0;
    double mRansacProb = 0.99;
    int mRansacMinInliers = 6, mRansacMaxIts = 300, mnIterations = 0, mnBestInliers = 0, best_ = -1;
    orbgpu_sim3_problem p_;
    std::vector<uint8_t> valid_;
    std::vector<int32_t> o1_, o2_, triples_, counts_;
    std::vector<float> x1_, x2_, R_, t_, s_, T12_;
    std::vector<uint64_t> masks_;
};

// --------------------------------------------------------------------------------------------
// PnPsolver (reference include/PnPsolver.h, src/PnPsolver.cc): the pose of a relocalisation candidate.  The conventions are
// P1-P10 of include/orbgpu.h.
// --------------------------------------------------------------------------------------------
// The draw of PnPsolver::iterate (:188-201) replayed for `iterations` iterations over n correspondences, min_set indices
// each: it overwrites vAvailableIndices[idx], not [randi], so one index can be drawn twice within a set.  random_int(min,
// max) is called min_set times per iteration.  n < min_set and a random_int outside [min, max] are refused with
// std::invalid_argument, as tests/pnp_model.py refuses them.
template <typename RandomInt>
inline std::vector<int32_t> PnPSampleSets(int n, int iterations, int min_set, RandomInt random_int)
{
    if (min_set < 1 || n < min_set)
        throw std::invalid_argument("PnPSampleSets: fewer correspondences than the minimal set");
    std::vector<int32_t> out((size_t)std::max(iterations, 0) * (size_t)min_set, 0);
    std::vector<int32_t> avail((size_t)n);
    for (int it = 0; it < iterations; it++) {
        for (int i = 0; i < n; i++)
            avail[i] = i;
        int size = n;
        for (int i = 0; i < min_set; i++) {
            const int randi = random_int(0, size - 1);
            if (randi < 0 || randi >= size)
                throw std::invalid_argument("PnPSampleSets: RandomInt outside [min, max]");
            const int idx = avail[randi];
            out[(size_t)it * min_set + i] = idx;
            avail[idx] = avail[size - 1];
            size--;
        }
    }
    return out;
}

// FrameT needs mvKeysUn, mvLevelSigma2, fx, fy, cx, cy; MapPointT isBad().  world_pos(pMP) returns 3 floats (valid during
// the constructor); random_int(min, max) stands for DUtils::Random::RandomInt.  The acceptance scan (P8) runs in the
// library; this class carries its state (mnIterations, mnBestInliers, the best record's pose and inliers) between calls.
// Every iterate(n, ...) draws the sets its scan can reach and that are not drawn yet -- up to max(max_its, mnIterations + n),
// in the reference's order over the one RandomInt stream, so a scan that runs past what was drawn gets further sets --
// and asks the library once (orbgpu_pnp_solve_all, resumed at (mnIterations, mnBestInliers)).  cv::Mat stays
// outside: iterate returns the 16 floats of Tcw (valid until the next call) or nullptr.
template <typename FrameT, typename MapPointT> class PnPsolverT {
  public:
    // (problem, counts, Tcw [H][16], masks, refined_mask, result) -> status: orbgpu_pnp_solve_all on this device
    typedef std::function<int(const orbgpu_pnp_problem *, int32_t *, float *, uint64_t *, uint64_t *, orbgpu_pnp_result *)> Solver;

    template <typename WorldPos, typename RandomInt>
    PnPsolverT(const FrameT &F, const std::vector<MapPointT *> &vpMapPointMatches, WorldPos world_pos, RandomInt random_int,
               int device_id = 0)
        : random_int_(random_int)
    {
        solver_ = [device_id](const orbgpu_pnp_problem *p, int32_t *counts, float *Tcw, uint64_t *masks, uint64_t *refined,
                              orbgpu_pnp_result *r) { return orbgpu_pnp_solve_all(p, counts, Tcw, masks, refined, r, device_id); };
        n1_ = (int)vpMapPointMatches.size();
        valid_.assign((size_t)n1_, 0), octave_.assign((size_t)n1_, 0);
        xw_.assign(3 * (size_t)n1_, 0.f), kp_.assign(2 * (size_t)n1_, 0.f);
        nlevels_ = (int)std::min(F.mvLevelSigma2.size(), (size_t)ORBGPU_MAX_LEVELS);
        N = 0;
        for (int i = 0; i < n1_; i++) {
            MapPointT *pMP = vpMapPointMatches[i];
            if (!pMP || pMP->isBad())
                continue;
            valid_[i] = 1;
            octave_[i] = F.mvKeysUn[i].octave;
            kp_[2 * (size_t)i] = F.mvKeysUn[i].pt.x, kp_[2 * (size_t)i + 1] = F.mvKeysUn[i].pt.y;
            std::memcpy(&xw_[3 * (size_t)i], world_pos(pMP), 12);
            if (octave_[i] >= 0 && octave_[i] < nlevels_)
                N++;  // P1: the rows the library keeps
        }
        std::memset(&p_, 0, sizeof(p_));
        p_.fx = F.fx, p_.fy = F.fy, p_.cx = F.cx, p_.cy = F.cy;
        for (int l = 0; l < nlevels_; l++)
            p_.level_sigma2[l] = F.mvLevelSigma2[l];
        SetRansacParameters();
    }

    // A fresh search: the iteration count, the best record and the drawn sets are reset.
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4,
                             float epsilon = 0.4f, float th2 = 5.991f)
    {
        int32_t mi = 0, its = 1;
        check(orbgpu_pnp_ransac_parameters(N, probability, minInliers, maxIterations, minSet, epsilon, &mi, &its),
              "PnPsolver::SetRansacParameters");
        mRansacMinInliers = mi, mRansacMaxIts = its, mRansacMinSet = minSet;
        p_.probability = probability, p_.min_inliers = minInliers, p_.max_iterations = maxIterations, p_.min_set = minSet;
        p_.epsilon = epsilon, p_.th2 = th2;
        mnIterations = 0, mnBestInliers = 0;
        sets_.clear(), best_mask_.clear();
        have_best_ = false;
    }

    const float *iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers)
    {
        bNoMore = false;
        vbInliers.clear();
        nInliers = 0;
        if (N < mRansacMinInliers || N < mRansacMinSet) {
            bNoMore = true;
            return nullptr;
        }
        const size_t words = ((size_t)n1_ + 63) / 64;
        // every set the scan of this call can reach: the reference's loop runs while mnIterations < max_its OR fewer than
        // nIterations were done in this call
        const long long reach = std::max<long long>(mRansacMaxIts, (long long)mnIterations + std::max(nIterations, 0));
        const int H = (int)std::min<long long>(reach, 4096);  // P10; a search that long ends without bNoMore
        Draw(H);
        p_.n1 = n1_, p_.n_hyp = H;
        p_.valid = valid_.data(), p_.Xw = xw_.data(), p_.kp = kp_.data(), p_.octave = octave_.data(), p_.sets = sets_.data();
        p_.nlevels = nlevels_;
        p_.start_iteration = mnIterations, p_.best_so_far = mnBestInliers, p_.n_iterations = std::max(nIterations, 0);
        counts_.assign((size_t)H, 0), tcw_.assign(16 * (size_t)H, 0.f), masks_.assign((size_t)H * words, 0);
        refined_.assign(std::max<size_t>(words, 1), 0);
        orbgpu_pnp_result r;
        check(solver_(&p_, counts_.data(), tcw_.data(), masks_.data(), refined_.data(), &r), "PnPsolver");
        mnIterations = r.iterations, mnBestInliers = r.best_inliers;
        if (r.best_iteration >= 0) {  // mBestTcw, mvbBestInliers
            std::memcpy(best_tcw_, &tcw_[16 * (size_t)r.best_iteration], 64);
            best_mask_.assign(masks_.begin() + (ptrdiff_t)((size_t)r.best_iteration * words),
                              masks_.begin() + (ptrdiff_t)(((size_t)r.best_iteration + 1) * words));
            have_best_ = true;
        }
        if (r.accepted >= 0) {
            nInliers = r.n_inliers;
            Expand(refined_, vbInliers);
            std::memcpy(out_tcw_, r.Tcw, 64);
            return out_tcw_;
        }
        if (r.no_more) {
            bNoMore = true;
            if (have_best_ && mnBestInliers >= mRansacMinInliers) {
                nInliers = mnBestInliers;
                Expand(best_mask_, vbInliers);
                std::memcpy(out_tcw_, best_tcw_, 64);
                return out_tcw_;
            }
        }
        return nullptr;
    }

    const float *find(std::vector<bool> &vbInliers, int &nInliers)
    {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
    }

    int NumCorrespondences() const { return N; }
    int MinInliers() const { return mRansacMinInliers; }
    int MaxIterations() const { return mRansacMaxIts; }
    int Iterations() const { return mnIterations; }
    int BestInliers() const { return mnBestInliers; }
    const std::vector<int32_t> &Sets() const { return sets_; }
    // a test serves the calls from recorded counts without a device
    void SetSolver(Solver s) { solver_ = s; }

  private:
    void Draw(int H)
    {
        const int have = (int)(sets_.size() / (size_t)mRansacMinSet);
        if (H <= have)
            return;
        const std::vector<int32_t> more = PnPSampleSets(N, H - have, mRansacMinSet, random_int_);
        sets_.insert(sets_.end(), more.begin(), more.end());
    }
    void Expand(const std::vector<uint64_t> &mask, std::vector<bool> &vbInliers) const
    {
        vbInliers.assign((size_t)n1_, false);
        for (int i = 0; i < n1_; i++)
            vbInliers[i] = (mask[(size_t)i >> 6] >> (i & 63)) & 1u;
    }

    std::function<int(int, int)> random_int_;
    Solver solver_;
    int n1_ = 0, N = 0, nlevels_ = 0;
    int mRansacMinInliers = 8, mRansacMaxIts = 300, mRansacMinSet = 4, mnIterations = 0, mnBestInliers = 0;
    bool have_best_ = false;
    float best_tcw_[16] = {0}, out_tcw_[16] = {0};
    orbgpu_pnp_problem p_;
    std::vector<uint8_t> valid_;
    std::vector<int32_t> octave_, sets_, counts_;
    std::vector<float> xw_, kp_, tcw_;
    std::vector<uint64_t> masks_, refined_, best_mask_;
};

// --------------------------------------------------------------------------------------------
// Initializer (reference include/Initializer.h, src/Initializer.cc): the monocular bootstrap.  The conventions are I1-I10
// of include/orbgpu.h.
// --------------------------------------------------------------------------------------------
// The draw of Initializer::Initialize (:82-97) replayed for `iterations` sets of 8 over n matches: WITHOUT replacement -- the
// back element moves into position randi (not PnPsolver's quirk).  random_int(min, max) is called 8 times per iteration.
// n < 8 and a random_int outside [min, max] are refused with std::invalid_argument, as tests/init_model.py refuses them.
template <typename RandomInt> inline std::vector<int32_t> InitializerSampleSets(int n, int iterations, RandomInt random_int)
{
    if (n < 8)
        throw std::invalid_argument("InitializerSampleSets: fewer matches than the minimal set");
    std::vector<int32_t> out((size_t)std::max(iterations, 0) * 8, 0);
    std::vector<int32_t> avail;
    for (int it = 0; it < iterations; it++) {
        avail.resize((size_t)n);
        for (int i = 0; i < n; i++)
            avail[i] = i;
        for (int j = 0; j < 8; j++) {
            const int randi = random_int(0, (int)avail.size() - 1);
            if (randi < 0 || randi >= (int)avail.size())
                throw std::invalid_argument("InitializerSampleSets: RandomInt outside [min, max]");
            out[(size_t)it * 8 + j] = avail[randi];
            avail[randi] = avail.back();
            avail.pop_back();
        }
    }
    return out;
}

// FrameT needs mvKeysUn, fx, fy, cx, cy.  The reference's constructor (ReferenceFrame, sigma, iterations) with the
// generator behind it: random_int(min, max) stands for DUtils::Random::RandomInt (the reference seeds it with
// SeedRandOnce(0)).  Initialize has the reference's arguments and return value; MatT is cv::Mat (create(rows, cols, type)
// and ptr<float>(row) are used), Point3T cv::Point3f.  Fewer than 8 matches return false without a draw (the reference
// would call RandomInt(0, -1); Tracking.cc asks for 100 matches).  At most 4096 iterations (the library's limit).
template <typename FrameT> class InitializerT {
  public:
    // (problem, P3D [n1][3], triangulated [n1], result) -> status: orbgpu_initializer on this device
    typedef std::function<int(const orbgpu_init_problem *, float *, uint8_t *, orbgpu_init_result *)> Solver;

    template <typename RandomInt>
    InitializerT(const FrameT &ReferenceFrame, float sigma, int iterations, RandomInt random_int, int device_id = 0)
        : random_int_(random_int), mSigma(sigma), mMaxIterations(std::min(std::max(iterations, 0), 4096))
    {
        solver_ = [device_id](const orbgpu_init_problem *p, float *P3D, uint8_t *tri, orbgpu_init_result *r) {
            return orbgpu_initializer(p, P3D, tri, r, device_id);
        };
        std::memset(&p_, 0, sizeof(p_));
        p_.fx = ReferenceFrame.fx, p_.fy = ReferenceFrame.fy, p_.cx = ReferenceFrame.cx, p_.cy = ReferenceFrame.cy;
        Keys(ReferenceFrame, kp1_);
        std::memset(&result_, 0, sizeof(result_));
    }

    template <typename MatT, typename Point3T>
    bool Initialize(const FrameT &CurrentFrame, const std::vector<int> &vMatches12, MatT &R21, MatT &t21,
                    std::vector<Point3T> &vP3D, std::vector<bool> &vbTriangulated, float minParallax = 1.0f,
                    int minTriangulated = 50)
    {
        const size_t n1 = kp1_.size() / 2;
        if (vMatches12.size() != n1)
            throw std::invalid_argument("Initializer::Initialize: one match entry per key point of the reference frame");
        Keys(CurrentFrame, kp2_);
        const int n2 = (int)(kp2_.size() / 2);
        matches_.assign(vMatches12.begin(), vMatches12.end());
        int N = 0;  // I1
        for (size_t i = 0; i < n1; i++)
            N += matches_[i] >= 0 && matches_[i] < n2;
        std::memset(&result_, 0, sizeof(result_));
        result_.n = N, result_.best_h = result_.best_f = result_.best_motion = -1;
        N_ = N;
        if (N < 8)
            return false;
        sets_ = InitializerSampleSets(N, mMaxIterations, random_int_);
        p_.n1 = (int32_t)n1, p_.n2 = n2, p_.kp1 = kp1_.data(), p_.kp2 = kp2_.data(), p_.matches12 = matches_.data();
        p_.sets = sets_.data(), p_.n_hyp = mMaxIterations;
        p_.sigma = mSigma, p_.min_parallax = minParallax, p_.min_triangulated = minTriangulated;
        p3d_.assign(3 * std::max<size_t>(n1, 1), 0.f), tri_.assign(std::max<size_t>(n1, 1), 0);
        check(solver_(&p_, p3d_.data(), tri_.data(), &result_), "Initializer");
        if (!result_.success)
            return false;
        R21.create(3, 3, 5), t21.create(3, 1, 5);  // CV_32F
        for (int i = 0; i < 3; i++) {
            std::memcpy(R21.template ptr<float>(i), result_.R21 + 3 * i, 12);
            *t21.template ptr<float>(i) = result_.t21[i];
        }
        vP3D.resize(n1), vbTriangulated.assign(n1, false);
        for (size_t i = 0; i < n1; i++) {
            vP3D[i].x = p3d_[3 * i], vP3D[i].y = p3d_[3 * i + 1], vP3D[i].z = p3d_[3 * i + 2];
            vbTriangulated[i] = tri_[i] != 0;
        }
        return true;
    }

    const orbgpu_init_result &Result() const { return result_; }  // of the last Initialize
    int NumMatches() const { return N_; }                         // I1's N of the last Initialize
    const std::vector<int32_t> &Sets() const { return sets_; }
    int MaxIterations() const { return mMaxIterations; }
    // a test serves the call from a recorded result without a device
    void SetSolver(Solver s) { solver_ = s; }

  private:
    static void Keys(const FrameT &F, std::vector<float> &kp)
    {
        kp.resize(2 * F.mvKeysUn.size());
        for (size_t i = 0; i < F.mvKeysUn.size(); i++)
            kp[2 * i] = F.mvKeysUn[i].pt.x, kp[2 * i + 1] = F.mvKeysUn[i].pt.y;
    }

    std::function<int(int, int)> random_int_;
    Solver solver_;
    float mSigma;
    int mMaxIterations, N_ = 0;
    orbgpu_init_problem p_;
    orbgpu_init_result result_;
    std::vector<float> kp1_, kp2_, p3d_;
    std::vector<int32_t> matches_, sets_;
    std::vector<uint8_t> tri_;
};

// --------------------------------------------------------------------------------------------
// LocalMapping::CreateNewMapPoints (LocalMapping.cc:207-452) on the device (orbgpu_create_new_map_points): the baseline
// test, ComputeF12 and the epipole per neighbour on the host, ONE library call for the whole neighbour loop, then the map
// edits of :434-449 in the reference's order.  KeyFrameT needs N, mvKeys, mvKeysUn, mvuRight, mvDepth, mFeatVec,
// GetMapPoint(i), AddMapPoint(pMP, i), fx, fy, cx, cy, invfx, invfy, mbf, mb, mvLevelSigma2, mvScaleFactors, mfScaleFactor;
// MapPointT needs mnId, AddObservation(pKF, i), ComputeDistinctiveDescriptors(), UpdateNormalAndDepth().  access:
//   desc_row(kf, i) -> 32 bytes;  pose(kf, float[16]) / pose_inverse(kf, float[16]) = GetPose() / GetPoseInverse();
//   median_depth(kf) = ComputeSceneMedianDepth(2);  F12(kf1, kf2, float[9]) = LocalMapping::ComputeF12, row-major;
//   new_map_point(const float x[3], kf1) = new MapPoint(x3D, mpCurrentKeyFrame, mpMap);
//   add_to_map(pMP) = mpMap->AddMapPoint(pMP) and mlpRecentAddedMapPoints.push_back(pMP);
//   with a table: world_pos / normal (3 floats), min_dist / max_dist, mp_desc (32 bytes) of a map point.
// --------------------------------------------------------------------------------------------
template <typename KeyFrameT> struct NewPointsFrameSoA {
    std::vector<float> x, y, angle, uright, depth, raw, cs;
    std::vector<int32_t> octave, node;
    std::vector<uint8_t> desc, has;
    orbgpu_new_points_frame f{};
    template <typename Access> NewPointsFrameSoA(KeyFrameT *kf, Access &access)
    {
        const int n = kf->N;
        x.resize(n), y.resize(n), angle.resize(n), uright.resize(n), depth.resize(n), raw.resize(2 * (size_t)n), cs.resize(n);
        octave.resize(n), desc.resize(32 * (size_t)n), has.resize(n);
        for (int i = 0; i < n; i++) {
            x[i] = kf->mvKeysUn[i].pt.x, y[i] = kf->mvKeysUn[i].pt.y;
            angle[i] = kf->mvKeysUn[i].angle, octave[i] = kf->mvKeysUn[i].octave;
            raw[2 * i] = kf->mvKeys[i].pt.x, raw[2 * i + 1] = kf->mvKeys[i].pt.y;  // KeyFrame::UnprojectStereo reads mvKeys
            uright[i] = kf->mvuRight[i], depth[i] = kf->mvDepth[i];
            // :312 / :314 as written: LocalMapping.cc sees <cmath> and a using-directive for std through its headers, so
            // cos and atan2 of float arguments are the float overloads and 2 * and / 2 stay in float
            cs[i] = std::cos(2 * std::atan2(kf->mb / 2, kf->mvDepth[i]));
            has[i] = kf->GetMapPoint(i) != nullptr;
            std::memcpy(&desc[32 * (size_t)i], access.desc_row(kf, i), 32);
        }
        node = NodeIdsOf(kf->mFeatVec, n);
        f.n = n, f.nlevels = (int32_t)kf->mvScaleFactors.size();
        f.kp_x = x.data(), f.kp_y = y.data(), f.kp_octave = octave.data(), f.kp_angle = angle.data(), f.u_right = uright.data();
        f.desc = desc.data(), f.has_mp = has.data(), f.node = node.data(), f.depth = depth.data(), f.kp_raw = raw.data();
        f.cos_stereo = cs.data();
        access.pose(kf, f.Tcw), access.pose_inverse(kf, f.Twc);
        f.fx = kf->fx, f.fy = kf->fy, f.cx = kf->cx, f.cy = kf->cy, f.invfx = kf->invfx, f.invfy = kf->invfy, f.mbf = kf->mbf;
        for (int l = 0; l < f.nlevels && l < ORBGPU_MAX_LEVELS; l++)
            f.level_sigma2[l] = kf->mvLevelSigma2[l], f.scale_factors[l] = kf->mvScaleFactors[l];
    }
};

template <typename KeyFrameT> struct NewPointsCall {
    KeyFrameT *cur;
    std::vector<KeyFrameT *> kept;  // the neighbours that pass :239 and :244-261, in the reference's order
    std::vector<std::unique_ptr<NewPointsFrameSoA<KeyFrameT>>> frames;  // [0] the current key frame, then kept
    std::vector<orbgpu_new_points_frame> nb;
    std::vector<int32_t> match12, status, n_matches, n_created;
    std::vector<float> x3d;
    int32_t n_done = 0;
    orbgpu_new_points_problem p{};

    // stop = CheckNewKeyFrames() sampled at the call: the reference returns before neighbour i > 0 then (:239)
    template <typename Access>
    NewPointsCall(KeyFrameT *pCurrentKF, const std::vector<KeyFrameT *> &vpNeighKFs, bool bMonocular, bool stop, Access &access)
        : cur(pCurrentKF)
    {
        frames.emplace_back(new NewPointsFrameSoA<KeyFrameT>(cur, access));
        const orbgpu_new_points_frame &f1 = frames[0]->f;
        const float Ow1[3] = {f1.Twc[3], f1.Twc[7], f1.Twc[11]};
        for (size_t i = 0; i < vpNeighKFs.size(); i++) {
            if (i > 0 && stop)
                break;
            KeyFrameT *pKF2 = vpNeighKFs[i];
            // :245-261 first, from the pose alone (a neighbour that fails is not flattened); cv::norm of the float difference
            // as an FP64 sum
            float Twc2[16];
            access.pose_inverse(pKF2, Twc2);
            const float b[3] = {Twc2[3] - Ow1[0], Twc2[7] - Ow1[1], Twc2[11] - Ow1[2]};
            const float baseline = (float)std::sqrt(((double)b[0] * b[0] + (double)b[1] * b[1]) + (double)b[2] * b[2]);
            if (!bMonocular) {
                if (baseline < pKF2->mb)
                    continue;
            } else {
                const float medianDepthKF2 = access.median_depth(pKF2);
                const float ratioBaselineDepth = baseline / medianDepthKF2;
                if (ratioBaselineDepth < 0.01)
                    continue;
            }
            std::unique_ptr<NewPointsFrameSoA<KeyFrameT>> s(new NewPointsFrameSoA<KeyFrameT>(pKF2, access));
            orbgpu_new_points_frame &f2 = s->f;
            access.F12(cur, pKF2, f2.F12);
            // the epipole (ORBmatcher.cc:664-670): C2 = R2w * Cw + t2w as a float 3x3 * 3x1 product, summed left to right
            float C2[3];
            for (int r = 0; r < 3; r++) {
                volatile float a = f2.Tcw[4 * r] * Ow1[0], bb = f2.Tcw[4 * r + 1] * Ow1[1], c = f2.Tcw[4 * r + 2] * Ow1[2];
                volatile float ab = a + bb;
                volatile float abc = ab + c;
                C2[r] = abc + f2.Tcw[4 * r + 3];
            }
            const float invz = 1.0f / C2[2];
            f2.ex = pKF2->fx * C2[0] * invz + pKF2->cx;
            f2.ey = pKF2->fy * C2[1] * invz + pKF2->cy;
            kept.push_back(pKF2);
            frames.push_back(std::move(s));
        }
        const size_t nn = kept.size(), n1 = (size_t)cur->N;
        if (nn > (size_t)ORBGPU_NEW_POINTS_MAX_NEIGHBOURS)
            throw std::runtime_error("CreateNewMapPoints: more neighbours than ORBGPU_NEW_POINTS_MAX_NEIGHBOURS");
        for (size_t k = 0; k < nn; k++)
            nb.push_back(frames[k + 1]->f);
        match12.assign(std::max<size_t>(nn * n1, 1), -1), status.assign(std::max<size_t>(nn * n1, 1), 0);
        x3d.assign(std::max<size_t>(3 * nn * n1, 1), 0.f), n_matches.assign(std::max<size_t>(nn, 1), 0);
        n_created.assign(std::max<size_t>(nn, 1), 0);
        p.kf1 = f1, p.neighbours = nb.data(), p.nn = (int32_t)nn;
        p.only_stereo = 0, p.check_orientation = 0;  // ORBmatcher matcher(0.6, false), bOnlyStereo = false (:215, :268)
        p.ratio_factor = 1.5f * cur->mfScaleFactor;
        p.stop = nullptr;
        p.match12 = match12.data(), p.status = status.data(), p.x3d = x3d.data();
        p.n_matches = n_matches.data(), p.n_created = n_created.data(), p.n_done = &n_done;
    }

    void Run(int device_id) { check(orbgpu_create_new_map_points(&p, device_id), "CreateNewMapPoints"); }

    // :434-449 per created point, neighbour ascending, key point ascending; returns nnew
    template <typename MapPointT, typename Access>
    int WriteBack(Access &access, MapPointTableT<MapPointT> *table, std::vector<MapPointT *> *created_out = nullptr)
    {
        std::vector<MapPointT *> created;
        const size_t n1 = (size_t)cur->N;
        for (size_t k = 0; k < kept.size(); k++)
            for (size_t i = 0; i < n1; i++) {
                if (status[k * n1 + i] <= 0)
                    continue;
                const int idx1 = (int)i, idx2 = match12[k * n1 + i];
                MapPointT *pMP = access.new_map_point(&x3d[3 * (k * n1 + i)], cur);
                pMP->AddObservation(cur, idx1);
                pMP->AddObservation(kept[k], idx2);
                cur->AddMapPoint(pMP, idx1);
                kept[k]->AddMapPoint(pMP, idx2);
                pMP->ComputeDistinctiveDescriptors();
                pMP->UpdateNormalAndDepth();
                access.add_to_map(pMP);
                created.push_back(pMP);
            }
        if (table && !created.empty())
            table->Upsert(
                created, [&access](MapPointT *m) { return access.world_pos(m); }, [&access](MapPointT *m) { return access.normal(m); },
                [&access](MapPointT *m) { return access.min_dist(m); }, [&access](MapPointT *m) { return access.max_dist(m); },
                [&access](MapPointT *m) { return access.mp_desc(m); });
        if (created_out)
            *created_out = created;
        return (int)created.size();
    }
};

// void LocalMapping::CreateNewMapPoints() with its state as arguments: the neighbours are
// mpCurrentKeyFrame->GetBestCovisibilityKeyFrames(mbMonocular ? 20 : 10), stop is CheckNewKeyFrames().  Returns nnew.
template <typename MapPointT, typename KeyFrameT, typename Access>
int CreateNewMapPointsT(KeyFrameT *pCurrentKF, const std::vector<KeyFrameT *> &vpNeighKFs, bool bMonocular, bool stop,
                        Access access, MapPointTableT<MapPointT> *table = nullptr, int device_id = 0)
{
    NewPointsCall<KeyFrameT> call(pCurrentKF, vpNeighKFs, bMonocular, stop, access);
    if (call.kept.empty())
        return 0;
    call.Run(device_id);
    return call.template WriteBack<MapPointT>(access, table);
}

// --------------------------------------------------------------------------------------------
// KeyFrameDatabase (reference include/KeyFrameDatabase.h:45-75, src/KeyFrameDatabase.cc) on the device
// (orbgpu_keyframe_db_*): add / erase / clear / DetectLoopCandidates / DetectRelocalizationCandidates with the
// reference's signatures, candidates in the reference's order.  KeyFrameT needs mnId, mBowVec (DBoW2::BowVector: an
// ordered map word id -> value), GetConnectedKeyFrames() (std::set<KeyFrameT *>) and GetBestCovisibilityKeyFrames(int);
// the frame passed to DetectRelocalizationCandidates needs mBowVec.  Neighbours are stored as ids: call
// UpdateCovisibles(pKF, ordered) where KeyFrame::UpdateBestCovisibles ends (INTEGRATION.md lists the hook sites).
// Lock order: a key frame's mMutexConnections may be held when this class's mutex is taken, never the other way round --
// no member calls into a key frame while it holds the class's mutex.  The class has its own mutex, like
// KeyFrameDatabase::mMutex, and keeps id -> KeyFrameT * so that the returned vectors hold the caller's pointers.
// --------------------------------------------------------------------------------------------
// id -> the caller's object (host only): what turns the ids a query returns back into KeyFrame pointers
template <typename T> class IdPtrMap {
  public:
    void put(int64_t id, T *p) { m_[id] = p; }
    void erase(int64_t id) { m_.erase(id); }
    void clear() { m_.clear(); }
    size_t size() const { return m_.size(); }
    // the pointers of ids[0..n) in order; an id the map does not hold is skipped
    std::vector<T *> Resolve(const int64_t *ids, size_t n) const
    {
        std::vector<T *> out;
        out.reserve(n);
        for (size_t i = 0; i < n; i++) {
            const auto it = m_.find(ids[i]);
            if (it != m_.end())
                out.push_back(it->second);
        }
        return out;
    }

  private:
    std::map<int64_t, T *> m_;
};

template <typename KeyFrameT> class KeyFrameDatabaseT {
  public:
    // n_words = voc.size() (KeyFrameDatabase.cc:36); the ORB vocabulary scores with L1_NORM (0), others are refused
    explicit KeyFrameDatabaseT(int n_words, int scoring = 0, int device_id = 0, int initial_rows = 0)
    {
        check(orbgpu_keyframe_db_create(n_words, scoring, device_id, initial_rows, &h_), "KeyFrameDatabase");
    }
    ~KeyFrameDatabaseT() { orbgpu_keyframe_db_destroy(h_); }
    KeyFrameDatabaseT(const KeyFrameDatabaseT &) = delete;
    KeyFrameDatabaseT &operator=(const KeyFrameDatabaseT &) = delete;
    orbgpu_keyframe_db *handle() const { return h_; }

    // DBoW2::BowVector -> the ABI's arrays (ascending word ids by the map's order)
    template <typename BowVectorT> static void Flatten(const BowVectorT &v, std::vector<int32_t> &ids, std::vector<double> &vals)
    {
        ids.clear(), vals.clear();
        ids.reserve(v.size()), vals.reserve(v.size());
        for (const auto &kv : v) {
            ids.push_back((int32_t)kv.first);
            vals.push_back((double)kv.second);
        }
    }

    void add(KeyFrameT *pKF)  // KeyFrameDatabase.cc:40-46
    {
        std::lock_guard<std::mutex> g(mu_);
        Flatten(pKF->mBowVec, ids_, vals_);
        check(orbgpu_keyframe_db_add(h_, (int64_t)pKF->mnId, (int32_t)ids_.size(), ids_.data(), vals_.data()),
              "KeyFrameDatabase::add");
        kfs_.put((int64_t)pKF->mnId, pKF);
    }
    void erase(KeyFrameT *pKF)  // :48-67
    {
        std::lock_guard<std::mutex> g(mu_);
        const int64_t id = (int64_t)pKF->mnId;
        check(orbgpu_keyframe_db_erase(h_, 1, &id, nullptr), "KeyFrameDatabase::erase");
        kfs_.erase(id);
    }
    void clear()  // :69-73
    {
        std::lock_guard<std::mutex> g(mu_);
        check(orbgpu_keyframe_db_clear(h_), "KeyFrameDatabase::clear");
        kfs_.clear();
    }
    // Drops the rows of erased key frames and gives their rows and pool space back (D1-D4 of orbgpu.h); invisible to every
    // other function of this class.  No function of this class calls it: INTEGRATION.md 2h says where a caller puts it.
    orbgpu_compact_result Compact()
    {
        std::lock_guard<std::mutex> g(mu_);
        orbgpu_compact_result res;
        check(orbgpu_keyframe_db_compact(h_, &res), "KeyFrameDatabase::Compact");
        return res;
    }
    int size() const
    {
        std::lock_guard<std::mutex> g(mu_);
        int32_t n = 0;
        check(orbgpu_keyframe_db_size(h_, &n), "KeyFrameDatabase::size");
        return n;
    }
    // hook: the end of KeyFrame::UpdateBestCovisibles (and of UpdateConnections, which fills the same vectors), INSIDE the
    // function, where mMutexConnections is held: it takes the list just built (mvpOrderedConnectedKeyFrames, of which the
    // first ten are GetBestCovisibilityKeyFrames(10)) and does not call back into the key frame.
    void UpdateCovisibles(KeyFrameT *pKF, const std::vector<KeyFrameT *> &ordered)
    {
        std::lock_guard<std::mutex> g(mu_);
        nb_.clear();
        for (size_t i = 0; i < ordered.size() && i < 10; i++)
            nb_.push_back((int64_t)ordered[i]->mnId);
        check(orbgpu_keyframe_db_set_covisibles(h_, (int64_t)pKF->mnId, (int32_t)nb_.size(), nb_.data()),
              "KeyFrameDatabase::UpdateCovisibles");
    }
    // the same from a place where mMutexConnections is NOT held (GetBestCovisibilityKeyFrames takes it, and it is not
    // recursive): after UpdateBestCovisibles / UpdateConnections has returned
    void UpdateCovisibles(KeyFrameT *pKF) { UpdateCovisibles(pKF, pKF->GetBestCovisibilityKeyFrames(10)); }
    // LoopClosing.cc:128-139: mpORBVocabulary->score(CurrentBowVec, pKF->mBowVec) of every key frame in one call (NaN for
    // one that is not in the database); minScore is the smallest of the non-bad ones
    std::vector<float> Score(KeyFrameT *pKF, const std::vector<KeyFrameT *> &others)
    {
        std::lock_guard<std::mutex> g(mu_);
        Flatten(pKF->mBowVec, ids_, vals_);
        nb_.clear();
        for (KeyFrameT *p : others)
            nb_.push_back((int64_t)p->mnId);
        std::vector<float> out(others.size());
        check(orbgpu_keyframe_db_score(h_, (int32_t)ids_.size(), ids_.data(), vals_.data(), (int32_t)nb_.size(), nb_.data(),
                                       out.data()),
              "KeyFrameDatabase::Score");
        return out;
    }
    std::vector<KeyFrameT *> DetectLoopCandidates(KeyFrameT *pKF, float minScore)  // :76-197
    {
        const std::set<KeyFrameT *> connected = pKF->GetConnectedKeyFrames();
        std::lock_guard<std::mutex> g(mu_);
        Flatten(pKF->mBowVec, ids_, vals_);
        nb_.clear();
        for (KeyFrameT *p : connected)
            nb_.push_back((int64_t)p->mnId);
        const std::vector<int64_t> conn = nb_;
        return Candidates([&](int32_t cap, int64_t *out, int32_t *n) {
            return orbgpu_keyframe_db_detect_loop(h_, (int32_t)ids_.size(), ids_.data(), vals_.data(), (int32_t)conn.size(),
                                                  conn.data(), minScore, cap, out, n);
        }, "KeyFrameDatabase::DetectLoopCandidates");
    }
    template <typename FrameT> std::vector<KeyFrameT *> DetectRelocalizationCandidates(FrameT *F)  // :199-309
    {
        std::lock_guard<std::mutex> g(mu_);
        Flatten(F->mBowVec, ids_, vals_);
        return Candidates([&](int32_t cap, int64_t *out, int32_t *n) {
            return orbgpu_keyframe_db_detect_reloc(h_, (int32_t)ids_.size(), ids_.data(), vals_.data(), cap, out, n);
        }, "KeyFrameDatabase::DetectRelocalizationCandidates");
    }

  private:
    // Candidates never outnumber the key frames of the database, so one call with that capacity returns all of them
    // (a query changes the reloc score register, so it is not run twice).
    template <typename Call> std::vector<KeyFrameT *> Candidates(Call call, const char *what)
    {
        nb_.assign(std::max<size_t>(kfs_.size(), 1), -1);
        int32_t n = 0;
        check(call((int32_t)nb_.size(), nb_.data(), &n), what);
        return kfs_.Resolve(nb_.data(), (size_t)std::min<int64_t>(n, (int64_t)nb_.size()));
    }

    orbgpu_keyframe_db *h_ = nullptr;
    mutable std::mutex mu_;
    IdPtrMap<KeyFrameT> kfs_;
    std::vector<int32_t> ids_;
    std::vector<double> vals_;
    std::vector<int64_t> nb_;
};

// --------------------------------------------------------------------------------------------
// Observation graph (orbgpu_covis_*): Tracking::UpdateLocalMap and the counting half of KeyFrame::UpdateConnections over
// the device-resident relation between key frames and map points (include/orbgpu.h, conventions V1-V8), and
// LocalMapping::KeyFrameCulling over it.
// KeyFrameT needs mnId, N, GetMapPointMatches(), GetMapPoint(idx), AddConnection(KeyFrameT *, int), isBad() and
// mnTrackReferenceForFrame -- and, for SetKeyPoints and KeyFrameCulling only, mvKeysUn, mvuRight, mvDepth, mThDepth,
// GetVectorCovisibleKeyFrames() and SetBadFlag(); MapPointT needs mnId, isBad() and mnTrackReferenceForFrame; the frame passed to UpdateLocalMap
// needs N, mnId, mvpMapPoints and mpReferenceKF.  The class keeps id -> pointer maps of the key frames it was given and of
// the map points its hooks have seen (ORB-SLAM2 never deletes either), so that the lists hold the caller's pointers.
// It serialises its calls with a mutex of its own, as MapPointTableT does, and never calls into a key frame or a map
// point while it holds it -- except the lock-free reads named at each hook.  INTEGRATION.md 2o lists the hook sites.
// --------------------------------------------------------------------------------------------
template <typename KeyFrameT, typename MapPointT> class CovisibilityGraphT {
  public:
    struct SlotEdit {
        KeyFrameT *kf;
        size_t idx;
        MapPointT *mp;  // nullptr clears the slot
    };
    struct Connections {
        std::vector<std::pair<KeyFrameT *, int>> counter;  // ascending mnId: mConnectedKeyFrameWeights
        std::vector<KeyFrameT *> ordered;                  // mvpOrderedConnectedKeyFrames
        std::vector<int> weights;                          // mvOrderedWeights
    };

    explicit CovisibilityGraphT(int device_id = 0, int initial_rows = 0, int64_t initial_slots = 0)
    {
        check(orbgpu_covis_graph_create(device_id, initial_rows, initial_slots, &h_), "CovisibilityGraph");
    }
    ~CovisibilityGraphT() { orbgpu_covis_graph_destroy(h_); }
    CovisibilityGraphT(const CovisibilityGraphT &) = delete;
    CovisibilityGraphT &operator=(const CovisibilityGraphT &) = delete;
    orbgpu_covis_graph *handle() const { return h_; }

    // the ids of a key frame's mvpMapPoints: -1 for an empty slot and for a bad point (V2: a bad point holds no slot)
    static std::vector<int64_t> SlotIds(const std::vector<MapPointT *> &mps)
    {
        std::vector<int64_t> ids(mps.size(), -1);
        for (size_t i = 0; i < mps.size(); i++)
            if (mps[i] && !mps[i]->isBad())
                ids[i] = (int64_t)mps[i]->mnId;
        return ids;
    }

    // hook: where a key frame enters the map (Map::AddKeyFrame), with the matches it holds at that moment
    void AddKeyFrame(KeyFrameT *pKF)
    {
        const std::vector<MapPointT *> mps = pKF->GetMapPointMatches();
        const std::vector<int64_t> ids = SlotIds(mps);
        std::lock_guard<std::mutex> g(mu_);
        check(orbgpu_covis_graph_add_keyframe(h_, (int64_t)pKF->mnId, (int32_t)ids.size(), ids.data()), "CovisibilityGraph::AddKeyFrame");
        kfs_.put((int64_t)pKF->mnId, pKF);
        for (MapPointT *p : mps)
            if (p)
                mps_.put((int64_t)p->mnId, p);
    }
    // hook: AddObservation / EraseObservation / EraseMapPointMatch / ReplaceMapPointMatch, batched: one call per key frame
    // from ProcessNewKeyFrame, from NewPointsCall::WriteBack and from the Fuse edit loop.  Applied in order.
    void SetSlots(const std::vector<SlotEdit> &edits)
    {
        if (edits.empty())
            return;
        std::lock_guard<std::mutex> g(mu_);
        Marshal(edits);
        check(orbgpu_covis_graph_set_slots(h_, (int32_t)ids_.size(), ids_.data(), idx_.data(), vals_.data(), nullptr),
              "CovisibilityGraph::SetSlots");
        for (const SlotEdit &e : edits)
            if (e.mp)
                mps_.put((int64_t)e.mp->mnId, e.mp);
    }
    void SetSlot(KeyFrameT *pKF, size_t idx, MapPointT *pMP) { SetSlots({SlotEdit{pKF, idx, pMP}}); }
    // hook: the end of MapPoint::SetBadFlag and of MapPoint::Replace, with the observation list those functions copied
    // (`obs`): every slot it names takes what the reference's loop left there -- nothing, or the replacing point.
    template <typename ObservationsT> void SyncObservations(const ObservationsT &obs)
    {
        std::vector<SlotEdit> edits;
        for (const auto &kv : obs) {
            MapPointT *now = kv.first->GetMapPoint(kv.second);
            edits.push_back(SlotEdit{kv.first, (size_t)kv.second, now && !now->isBad() ? now : nullptr});
        }
        SetSlots(edits);
    }
    // hook: the end of KeyFrame::SetBadFlag (after mbBad = true); the children's ChangeParent calls reach SetParent
    void SetKeyFrameBad(KeyFrameT *pKF)
    {
        std::lock_guard<std::mutex> g(mu_);
        const int64_t id = (int64_t)pKF->mnId;
        check(orbgpu_covis_graph_set_bad(h_, 1, &id, nullptr), "CovisibilityGraph::SetKeyFrameBad");
    }
    // hook: KeyFrame::ChangeParent and the first connection of UpdateConnections
    void SetParent(KeyFrameT *pKF, KeyFrameT *pParent)
    {
        std::lock_guard<std::mutex> g(mu_);
        check(orbgpu_covis_graph_set_parent(h_, (int64_t)pKF->mnId, pParent ? (int64_t)pParent->mnId : -1), "CovisibilityGraph::SetParent");
    }
    // hook: the end of KeyFrame::UpdateBestCovisibles, inside the function (KeyFrameDatabaseT::UpdateCovisibles's place)
    void UpdateCovisibles(KeyFrameT *pKF, const std::vector<KeyFrameT *> &ordered)
    {
        std::lock_guard<std::mutex> g(mu_);
        ids_.clear();
        for (size_t i = 0; i < ordered.size() && i < ORBGPU_COVIS_MAX_COVISIBLES; i++)
            ids_.push_back((int64_t)ordered[i]->mnId);
        check(orbgpu_covis_graph_set_covisibles(h_, (int64_t)pKF->mnId, (int32_t)ids_.size(), ids_.data()),
              "CovisibilityGraph::UpdateCovisibles");
    }
    void clear()  // Map::clear
    {
        std::lock_guard<std::mutex> g(mu_);
        check(orbgpu_covis_graph_clear(h_), "CovisibilityGraph::clear");
        kfs_.clear();
        mps_.clear();
    }
    // Drops the bad rows that no live row names as its parent and gives their rows and pool space back (C1-C7 of
    // orbgpu.h).  No function of this class calls it: KeyFrameCulling and the hooks behave as they did.  The caller decides
    // when -- INTEGRATION.md 2o: after the SetBadFlag loop that follows KeyFrameCulling.  A dropped key frame stays in this
    // class's id map (the reference never deletes a KeyFrame), where no answer of the graph names it any more.
    orbgpu_compact_result Compact()
    {
        std::lock_guard<std::mutex> g(mu_);
        orbgpu_compact_result res;
        check(orbgpu_covis_graph_compact(h_, &res), "CovisibilityGraph::Compact");
        return res;
    }
    size_t KeyFrames() const
    {
        std::lock_guard<std::mutex> g(mu_);
        return kfs_.size();
    }

    // Tracking::UpdateLocalMap (Tracking.cc:1499-1643) with the reference's side effects: bad points leave the frame
    // (:1552), the listed key frames and points are stamped with the frame's id, the reference key frame is set on the
    // tracker and on the frame if a key frame was voted for; without a vote mvpLocalKeyFrames stays as it is (:1557-1558).
    template <typename FrameT>
    void UpdateLocalMap(FrameT &F, std::vector<KeyFrameT *> &mvpLocalKeyFrames, std::vector<MapPointT *> &mvpLocalMapPoints,
                        KeyFrameT *&mpReferenceKF)
    {
        std::vector<int64_t> kp((size_t)F.N, -1), prev;
        for (int i = 0; i < F.N; i++)
            if (F.mvpMapPoints[(size_t)i]) {
                if (!F.mvpMapPoints[(size_t)i]->isBad())
                    kp[(size_t)i] = (int64_t)F.mvpMapPoints[(size_t)i]->mnId;
                else
                    F.mvpMapPoints[(size_t)i] = nullptr;
            }
        for (KeyFrameT *p : mvpLocalKeyFrames)
            prev.push_back((int64_t)p->mnId);
        std::vector<KeyFrameT *> kfs;
        std::vector<MapPointT *> mps;
        orbgpu_covis_local_map_result res;
        {
            std::lock_guard<std::mutex> g(mu_);
            // the lists never outnumber the key frames (plus the previous list) and the slots: one call returns them all
            ids_.assign(kfs_.size() + prev.size() + 1, -1);
            vals_.assign(std::max<size_t>(last_points_ * 2, 4096), -1);
            for (int attempt = 0; attempt < 2; attempt++) {
                check(orbgpu_covis_local_map(h_, (int32_t)kp.size(), kp.data(), (int32_t)prev.size(), prev.data(), (int32_t)ids_.size(),
                                             ids_.data(), (int32_t)vals_.size(), vals_.data(), &res),
                      "CovisibilityGraph::UpdateLocalMap");
                if ((size_t)res.n_points <= vals_.size())
                    break;
                vals_.assign((size_t)res.n_points, -1);  // (a local map that more than doubled: once more, with room)
            }
            last_points_ = (size_t)res.n_points;
            kfs = kfs_.Resolve(ids_.data(), std::min((size_t)res.n_kfs, ids_.size()));
            mps = mps_.Resolve(vals_.data(), std::min((size_t)res.n_points, vals_.size()));
        }
        if (!res.kept_previous)
            mvpLocalKeyFrames.swap(kfs);
        for (KeyFrameT *p : mvpLocalKeyFrames)
            p->mnTrackReferenceForFrame = F.mnId;
        mvpLocalMapPoints.swap(mps);
        for (MapPointT *p : mvpLocalMapPoints)
            p->mnTrackReferenceForFrame = F.mnId;
        if (res.ref_kf >= 0) {
            const std::vector<KeyFrameT *> ref = [&] {
                std::lock_guard<std::mutex> g(mu_);
                return kfs_.Resolve(&res.ref_kf, 1);
            }();
            if (!ref.empty()) {
                mpReferenceKF = ref[0];
                F.mpReferenceKF = ref[0];
            }
        }
    }

    // The counting half of KeyFrame::UpdateConnections (KeyFrame.cc:327-399) and its host half: the counter, AddConnection
    // on the key frames at the threshold (or on the single best one), the ordered vectors.  `apply(connections)` runs where
    // the reference takes mMutexConnections (:401-416): it stores the three containers and returns the new parent if this
    // was the first connection (nullptr otherwise).  The two hooks follow.  Returns false if no key frame was counted
    // (:361-362: nothing changes).
    template <typename Apply> bool UpdateConnections(KeyFrameT *pKF, Apply apply, int th = 15)
    {
        Connections c;
        {
            std::lock_guard<std::mutex> g(mu_);
            const int32_t cap = (int32_t)std::max<size_t>(kfs_.size(), 1);
            ids_.assign((size_t)cap, -1);
            vals_.assign((size_t)cap, -1);
            std::vector<int32_t> counts((size_t)cap), weights((size_t)cap);
            int32_t n = 0, n_ordered = 0;
            check(orbgpu_covis_connections(h_, (int64_t)pKF->mnId, th, cap, ids_.data(), counts.data(), &n, cap, vals_.data(),
                                           weights.data(), &n_ordered),
                  "CovisibilityGraph::UpdateConnections");
            c = MakeConnections(kfs_, ids_.data(), counts.data(), (size_t)std::min(n, cap), vals_.data(), weights.data(),
                                (size_t)std::min(n_ordered, cap));
        }
        if (c.counter.empty() || c.ordered.empty())
            return false;
        KeyFrameT *parent = HostHalf(pKF, c, apply);
        UpdateCovisibles(pKF, c.ordered);
        if (parent)
            SetParent(pKF, parent);
        return true;
    }

    // host only: V1's attribute byte of every key point.  KeyFrameT needs mvKeysUn (elements with .octave), mvuRight,
    // mvDepth and mThDepth; bMonocular is LocalMapping's mbMonocular (LocalMapping.cc:660-664).
    static std::vector<uint8_t> KeyPointBytes(const KeyFrameT &kf, bool bMonocular)
    {
        std::vector<uint8_t> kp(kf.mvKeysUn.size());
        for (size_t i = 0; i < kp.size(); i++) {
            const int octave = std::min(std::max((int)kf.mvKeysUn[i].octave, 0), ORBGPU_COVIS_MAX_LEVELS - 1);
            const bool stereo = kf.mvuRight[i] >= 0;
            const bool far_point = !bMonocular && (kf.mvDepth[i] > kf.mThDepth || kf.mvDepth[i] < 0);
            kp[i] = (uint8_t)(octave | (stereo ? ORBGPU_COVIS_KP_STEREO : 0) | (far_point ? ORBGPU_COVIS_KP_FAR : 0));
        }
        return kp;
    }
    // hook: after AddKeyFrame(pKF), once -- key points do not change (reads const members only: no lock of the key frame)
    void SetKeyPoints(KeyFrameT *pKF, bool bMonocular)
    {
        const std::vector<uint8_t> kp = KeyPointBytes(*pKF, bMonocular);
        std::lock_guard<std::mutex> g(mu_);
        check(orbgpu_covis_graph_set_keypoints(h_, (int64_t)pKF->mnId, (int32_t)kp.size(), kp.data()), "CovisibilityGraph::SetKeyPoints");
    }
    // MapPoint::Observations() of every point of pts (0 for a null or bad one), read from the graph: what
    // LocalMapping::MapPointCulling (LocalMapping.cc:195) and KeyFrame::TrackedMapPoints compare with their thresholds
    std::vector<int> Observations(const std::vector<MapPointT *> &pts)
    {
        std::vector<int64_t> ids(pts.size(), -1);
        for (size_t i = 0; i < pts.size(); i++)
            if (pts[i] && !pts[i]->isBad())
                ids[i] = (int64_t)pts[i]->mnId;
        std::vector<int32_t> n_obs(pts.size()), n_slots(pts.size());
        std::lock_guard<std::mutex> g(mu_);
        check(orbgpu_covis_observations(h_, (int32_t)ids.size(), ids.data(), n_obs.data(), n_slots.data()), "CovisibilityGraph::Observations");
        return std::vector<int>(n_obs.begin(), n_obs.end());
    }
    // LocalMapping::KeyFrameCulling (LocalMapping.cc:632-698, V8) over pCurrentKF->GetVectorCovisibleKeyFrames();
    // not_erase(pKF) reads the key frame's mbNotErase (under its
    // mMutexConnections, outside this class's mutex).  The library decides; SetBadFlag() then runs on every key frame with
    // verdict 1, in order, outside the mutex -- its hooks (SetKeyFrameBad, SyncObservations, SetParent) bring the graph to
    // the state the call predicted; a key frame with verdict 2 gets SetBadFlag() too, which only sets mbToBeErased
    // (KeyFrame.cc:497-501).  Returns the culled key frames.
    template <typename NotErase> std::vector<KeyFrameT *> KeyFrameCulling(KeyFrameT *pCurrentKF, NotErase not_erase, int thObs = 3)
    {
        const std::vector<KeyFrameT *> vpLocalKeyFrames = pCurrentKF->GetVectorCovisibleKeyFrames();
        const size_t n = vpLocalKeyFrames.size();
        std::vector<int64_t> ids(n);
        std::vector<uint8_t> keep(n);
        for (size_t i = 0; i < n; i++) {
            ids[i] = (int64_t)vpLocalKeyFrames[i]->mnId;
            keep[i] = not_erase(vpLocalKeyFrames[i]) ? 1 : 0;
        }
        std::vector<int8_t> verdict(n);
        std::vector<int32_t> n_mps(n), n_red(n);
        orbgpu_covis_culling_result res;
        {
            std::lock_guard<std::mutex> g(mu_);
            check(orbgpu_covis_keyframe_culling(h_, (int32_t)n, ids.data(), keep.data(), thObs, verdict.data(), n_mps.data(), n_red.data(), 0,
                                                nullptr, &res),
                  "CovisibilityGraph::KeyFrameCulling");
        }
        std::vector<KeyFrameT *> culled;
        for (size_t i = 0; i < n; i++)
            if (verdict[i] == 1 || verdict[i] == 2) {
                vpLocalKeyFrames[i]->SetBadFlag();
                if (verdict[i] == 1)
                    culled.push_back(vpLocalKeyFrames[i]);
            }
        return culled;
    }

    // ---- MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth over the graph (R1-R8) ----
    // hook: once per map, KeyFrame::mvScaleFactors (the same for every key frame)
    void SetScaleFactors(const std::vector<float> &v)
    {
        std::lock_guard<std::mutex> g(mu_);
        check(orbgpu_covis_graph_set_scale_factors(h_, (int32_t)v.size(), v.data()), "CovisibilityGraph::SetScaleFactors");
    }
    // hook: behind SetKeyPoints(pKF), once -- descriptors do not change.  desc_row(pKF, i) -> the 32 bytes of
    // mDescriptors.row(i) (a const member: no lock of the key frame)
    template <typename DescRow> void SetDescriptors(KeyFrameT *pKF, DescRow desc_row)
    {
        const size_t n = (size_t)pKF->N;
        std::vector<uint8_t> d(32 * n);
        for (size_t i = 0; i < n; i++)
            std::memcpy(&d[32 * i], desc_row(pKF, i), 32);
        std::lock_guard<std::mutex> g(mu_);
        check(orbgpu_covis_graph_set_descriptors(h_, (int64_t)pKF->mnId, (int32_t)n, d.data()), "CovisibilityGraph::SetDescriptors");
    }
    // hook: KeyFrame::SetPose (one key frame), and after the write-back of a bundle adjustment or of the essential graph
    // (every key frame it moved, one call).  centre(pKF, out[3]) writes GetCameraCenter(); it runs outside the mutex.
    template <typename Centre> void SetCentres(const std::vector<KeyFrameT *> &keyframes, Centre centre)
    {
        std::vector<int64_t> ids(keyframes.size());
        std::vector<float> ow(3 * keyframes.size());
        for (size_t i = 0; i < keyframes.size(); i++) {
            ids[i] = (int64_t)keyframes[i]->mnId;
            centre(keyframes[i], &ow[3 * i]);
        }
        std::lock_guard<std::mutex> g(mu_);
        check(orbgpu_covis_graph_set_centres(h_, (int32_t)ids.size(), ids.data(), ow.data(), nullptr), "CovisibilityGraph::SetCentres");
    }
    // The two calls that end every chain that edits the map, for a batch of points.  `what`: ORBGPU_REFRESH_DESCRIPTOR |
    // ORBGPU_REFRESH_NORMAL_DEPTH.  access supplies ref_kf(pMP) -> KeyFrameT * (mpRefKF), world_pos(pMP) -> const float *
    // (read before the call; unused with a table) and set_refreshed(pMP, normal, minDist, maxDist, desc): normal is null
    // where the status left normal and depth untouched, desc is null where it left the descriptor untouched; a point with
    // neither is not called.  Null, bad and repeated points are passed over (mbBad returns at MapPoint.cc:251 / :338).
    // With a table the positions come from its rows and the results go into its rows on the device -- no Upsert afterwards;
    // its mutex is taken first, then this class's, and both are released before set_refreshed runs.
    template <typename Access>
    orbgpu_covis_refresh_result RefreshMapPoints(const std::vector<MapPointT *> &points, unsigned what, Access &access,
                                                 MapPointTableT<MapPointT> *table = nullptr)
    {
        std::vector<MapPointT *> pts;
        std::vector<int64_t> ids, refs;
        std::vector<float> pos;
        {
            std::vector<int64_t> seen;
            for (MapPointT *p : points)
                if (p && !p->isBad())
                    seen.push_back((int64_t)p->mnId);
            std::sort(seen.begin(), seen.end());
            std::vector<char> taken(seen.size(), 0);
            for (MapPointT *p : points) {
                if (!p || p->isBad())
                    continue;
                const size_t at = (size_t)(std::lower_bound(seen.begin(), seen.end(), (int64_t)p->mnId) - seen.begin());
                if (taken[at])
                    continue;
                taken[at] = 1;
                KeyFrameT *ref = access.ref_kf(p);
                pts.push_back(p);
                ids.push_back((int64_t)p->mnId);
                refs.push_back(ref ? (int64_t)ref->mnId : -1);
                if (!table) {
                    const float *w = access.world_pos(p);
                    pos.insert(pos.end(), w, w + 3);
                }
            }
        }
        const size_t n = pts.size();
        std::vector<float> normal(3 * n), mn(n), mx(n);
        std::vector<uint8_t> desc(32 * n), status(n);
        std::vector<int32_t> n_slots(n);
        orbgpu_covis_refresh_result res;
        if (table) {
            std::lock_guard<std::mutex> table_lock(table->mutex());
            std::lock_guard<std::mutex> g(mu_);
            check(orbgpu_mappoint_table_refresh(table->handle(), h_, (int32_t)n, ids.data(), refs.data(), what, normal.data(), mn.data(),
                                                mx.data(), desc.data(), nullptr, nullptr, n_slots.data(), status.data(), &res),
                  "CovisibilityGraph::RefreshMapPoints (table)");
        } else {
            std::lock_guard<std::mutex> g(mu_);
            check(orbgpu_covis_refresh_points(h_, (int32_t)n, ids.data(), refs.data(), pos.data(), what, normal.data(), mn.data(), mx.data(),
                                              desc.data(), nullptr, nullptr, n_slots.data(), status.data(), &res),
                  "CovisibilityGraph::RefreshMapPoints");
        }
        const unsigned no_point = ORBGPU_REFRESH_NO_OBS | ORBGPU_REFRESH_OVERFLOW | ORBGPU_REFRESH_UNKNOWN | ORBGPU_REFRESH_BAD;
        for (size_t i = 0; i < n; i++) {
            const unsigned s = status[i];
            const bool has_desc = (what & ORBGPU_REFRESH_DESCRIPTOR) && !(s & (no_point | ORBGPU_REFRESH_NO_DESC));
            const bool has_normal = (what & ORBGPU_REFRESH_NORMAL_DEPTH) && !(s & (no_point | ORBGPU_REFRESH_NO_CENTRE | ORBGPU_REFRESH_NO_REF));
            if (has_desc || has_normal)
                access.set_refreshed(pts[i], has_normal ? &normal[3 * i] : nullptr, mn[i], mx[i], has_desc ? &desc[32 * i] : nullptr);
        }
        return res;
    }

    // host only: a batch of slot edits as the ABI's three arrays
    static void MarshalSlots(const std::vector<SlotEdit> &edits, std::vector<int64_t> &kf_ids, std::vector<int32_t> &idx,
                             std::vector<int64_t> &mp_ids)
    {
        kf_ids.clear(), idx.clear(), mp_ids.clear();
        for (const SlotEdit &e : edits) {
            kf_ids.push_back((int64_t)e.kf->mnId);
            idx.push_back((int32_t)e.idx);
            mp_ids.push_back(e.mp ? (int64_t)e.mp->mnId : -1);
        }
    }
    // host only: the lists of orbgpu_covis_connections as the reference's containers (an id the map does not hold is skipped)
    static Connections MakeConnections(const IdPtrMap<KeyFrameT> &kfs, const int64_t *ids, const int32_t *counts, size_t n,
                                       const int64_t *ordered_ids, const int32_t *weights, size_t n_ordered)
    {
        Connections c;
        for (size_t i = 0; i < n; i++)
            for (KeyFrameT *p : kfs.Resolve(ids + i, 1))
                c.counter.emplace_back(p, (int)counts[i]);
        for (size_t i = 0; i < n_ordered; i++)
            for (KeyFrameT *p : kfs.Resolve(ordered_ids + i, 1)) {
                c.ordered.push_back(p);
                c.weights.push_back((int)weights[i]);
            }
        return c;
    }
    // host only: KeyFrame.cc:382 / :389 (AddConnection on every listed key frame; the order among them does not matter)
    // and :401-416 through `apply`
    template <typename Apply> static KeyFrameT *HostHalf(KeyFrameT *pKF, const Connections &c, Apply apply)
    {
        for (size_t i = 0; i < c.ordered.size(); i++)
            c.ordered[i]->AddConnection(pKF, c.weights[i]);
        return apply(c);
    }

  private:
    void Marshal(const std::vector<SlotEdit> &edits) { MarshalSlots(edits, ids_, idx_, vals_); }
    orbgpu_covis_graph *h_ = nullptr;
    mutable std::mutex mu_;
    IdPtrMap<KeyFrameT> kfs_;
    IdPtrMap<MapPointT> mps_;
    std::vector<int64_t> ids_, vals_;
    std::vector<int32_t> idx_;
    size_t last_points_ = 0;
};

// --------------------------------------------------------------------------------------------
// PointCloudMapping (reference include/PointCloudMap.h:41-88, src/PointCloudMap.cc)
// Keeps the reference's thread / condition-variable protocol; the per-key-frame arithmetic runs on
// the GPU.  KeyFrameT needs mImDep (float depth), mImRGB (8UC3), fx, fy, cx, cy and GetPose();
// the Adapter adapts cv::Mat (or a stand-in): depth(kf), rgb(kf) -> ImageView, pose(kf, float[16]),
// fx/fy/cx/cy(kf), and -- only for the loop-closure branch -- id(kf) (mnId) and isBad(kf).
// Visualisation stays out; the outlier filter of the shutdown pass is orbgpu_cloud_remove_outliers, the PCD writer
// orbgpu_cloud_save_pcd.
//
// viewer() follows PointCloudMap.cc:182-289 branch by branch:
//   * wait for key frames (:195-198) -- with a predicate: the reference's bare wait() can lose a wake-up and, woken
//     by shutdown() with no new key frame, indexes keyframes[N] (:246);
//   * loop closure (:217-243): when the hook reports LoopClosing::loop_detected (and clears it, :219), the map is
//     rebuilt from all non-bad key frames of the Map sorted by id;
//   * otherwise (:244-267) the new key frames are inserted.  The reference transforms only the LAST new cloud
//     (keyFrameCloud.back(), :247) with the pose of the FIRST new key frame (keyframes[lastKeyframeSize], :246) and,
//     in the loop branch, does not advance lastKeyframeSize (so the next insert takes the pose of the first key frame
//     that arrived with the loop closure).  That IS the default here -- the drop-in's map equals the reference's for the
//     same grouping of key frames into wake-ups.  setReferenceQuirks(false) is the corrected opt-in: every new key
//     frame is inserted with its own pose and the loop branch consumes its key frames.  After a loop branch the
//     reference only runs again on the next notify, i.e. the next insertKeyFrame: the wait predicate therefore
//     compares against the number of key frames SEEN (seenSize), not against the stale lastKeyframeSize;
//   * after the loop (:270-288): clear, per key frame generatePointCloud + voxel.filter + `+=`, then sor.filter
//     (meanK 50, stddev factor 1.0: the constructor's settings, :46-47) and, if an output path is set,
//     savePCDFileBinary.  A map of meanK points or fewer is left unfiltered (PCL reads past its neighbour list there).
// --------------------------------------------------------------------------------------------
struct ImageView {
    const void *data;
    int rows, cols;
    size_t step;  // bytes
};

template <typename KeyFrameT, typename Adapter> class PointCloudMappingT {
  public:
    struct LoopHooks {
        // returns true once per detected loop: `if (loopCloser->loop_detected) { loopCloser->loop_detected = false; ...`
        std::function<bool()> take_loop_detected;
        // loopCloser->getMap()->GetAllKeyFrames()
        std::function<std::vector<KeyFrameT *>()> all_keyframes;
    };

    PointCloudMappingT(double resolution_, Adapter adapter = Adapter(), int device_id = 0, LoopHooks hooks_ = LoopHooks())
        : resolution(resolution_), adapt(adapter), hooks(hooks_)
    {
        check(orbgpu_cloud_create(resolution, device_id, &cloud_), "PointCloudMapping");
        viewerThread = std::make_shared<std::thread>(&PointCloudMappingT::viewer, this);  // PointCloudMap.cc:53
    }
    ~PointCloudMappingT()
    {
        if (viewerThread && viewerThread->joinable())
            shutdown();
        orbgpu_cloud_destroy(cloud_);
    }

    // true (default): PointCloudMap.cc:217-262 statement by statement; false: the corrected insert (own pose per key
    // frame, loop branch advances lastKeyframeSize).  Set before the first insertKeyFrame.
    void setReferenceQuirks(bool on)
    {
        std::unique_lock<std::mutex> lck(keyframeMutex);
        quirks = on;
    }
    // "optimized_pointcloud.pcd" in the reference (:287); empty (default) = do not write a file
    void setOutputPath(const std::string &path) { outputPath = path; }
    // the reference fixes these in its constructor (:46-47); meanK <= 0 skips the filter
    void setOutlierFilter(int meanK, double stddevMul) { sorMeanK = meanK, sorStddevMul = stddevMul; }

    void insertKeyFrame(KeyFrameT *kf)  // PointCloudMap.cc:69-76
    {
        std::unique_lock<std::mutex> lck(keyframeMutex);
        keyframes.push_back(kf);
        keyFrameUpdated.notify_one();
    }

    // blocks until the viewer has consumed every key frame / loop notification handed over so far (not in the
    // reference: there the only way to know is the console output)
    void waitProcessed()
    {
        std::unique_lock<std::mutex> lck(keyframeMutex);
        processed.wait(lck, [&] { return finished || (!busy && !loopPending && keyframes.size() <= seenSize); });
    }

    // a detected loop must wake the viewer too (the reference relies on the next key frame's notify)
    void notifyLoop()
    {
        std::unique_lock<std::mutex> lck(keyframeMutex);
        loopPending = true;
        keyFrameUpdated.notify_one();
    }

    void shutdown()  // PointCloudMap.cc:59-67
    {
        {
            // The flag is published under keyframeMutex, the mutex the condition variable waits on: a notify
            // between the viewer's predicate evaluation and its block cannot be lost (the reference sets it under
            // shutDownMutex only and can hang in join()).
            std::unique_lock<std::mutex> lck(keyframeMutex);
            {
                std::unique_lock<std::mutex> lck2(shutDownMutex);
                shutDownFlag = true;
            }
            keyFrameUpdated.notify_one();
        }
        if (viewerThread->joinable())
            viewerThread->join();
    }

    void viewer()  // PointCloudMap.cc:182-289
    {
        while (true) {
            if (shutDownFlagLocked())  // :186-192
                break;
            size_t N, first;
            bool ref;
            {
                std::unique_lock<std::mutex> lck(keyframeMutex);  // :195-198
                keyFrameUpdated.wait(lck, [&] { return shutDownFlagLocked() || loopPending || keyframes.size() > seenSize; });
                loopPending = false;
                busy = true;
                N = keyframes.size();  // :202-205
                first = lastKeyframeSize;
                seenSize = N;
                ref = quirks;
            }
            size_t done = first;
            if (hooks.take_loop_detected && hooks.all_keyframes && hooks.take_loop_detected()) {  // :217-243
                std::vector<KeyFrameT *> all = hooks.all_keyframes();
                std::sort(all.begin(), all.end(), [&](KeyFrameT *a, KeyFrameT *b) { return adapt.id(a) < adapt.id(b); });
                std::vector<KeyFrameT *> good;
                for (KeyFrameT *kf : all)
                    if (!adapt.isBad(kf))
                        good.push_back(kf);
                rebuild(good);
                if (!ref)
                    done = N;  // the reference leaves it (:243 falls out of the branch without `lastKeyframeSize = N`)
            } else if (N > first) {  // :244-267
                if (ref)
                    insertOne(keyframeAt(N - 1), keyframeAt(first));  // keyFrameCloud.back() with keyframes[lastKeyframeSize]'s pose (:246-247)
                else
                    for (size_t i = first; i < N; i++)
                        insertOne(keyframeAt(i), keyframeAt(i));
                done = N;
            }
            {
                std::unique_lock<std::mutex> lck(keyframeMutex);
                lastKeyframeSize = done;
                busy = false;
                processed.notify_all();
            }
        }
        {
            std::unique_lock<std::mutex> lck(keyframeMutex);
            busy = false;
            finished = true;
            processed.notify_all();
        }
        // :270-288: the down-sampled clouds of all key frames, one by one
        std::vector<KeyFrameT *> kfs;
        {
            std::unique_lock<std::mutex> lck(keyframeMutex);
            kfs = keyframes;
        }
        {
            std::unique_lock<std::mutex> lck(cloudMutex);
            check(orbgpu_cloud_clear(cloud_), "PointCloudMapping::shutdown");
            for (KeyFrameT *kf : kfs) {
                ImageView d = adapt.depth(kf), c = adapt.rgb(kf);
                float Tcw[16];
                adapt.pose(kf, Tcw);
                check(orbgpu_cloud_append_filtered(cloud_, (const float *)d.data, d.step / sizeof(float),
                                                   (const uint8_t *)c.data, c.step, d.cols, d.rows, adapt.fx(kf),
                                                   adapt.fy(kf), adapt.cx(kf), adapt.cy(kf), Tcw),
                      "PointCloudMapping::shutdown");
            }
            int64_t npts = 0;
            check(orbgpu_cloud_size(cloud_, &npts), "PointCloudMapping::shutdown");
            if (sorMeanK > 0 && npts > sorMeanK)  // :283-285
                check(orbgpu_cloud_remove_outliers(cloud_, sorMeanK, sorStddevMul, nullptr), "PointCloudMapping::shutdown");
            if (!outputPath.empty())
                check(orbgpu_cloud_save_pcd(cloud_, outputPath.c_str()), "PointCloudMapping::save");
        }
    }

    // loop-closure branch (PointCloudMap.cc:217-243): regenerate every key frame with its new pose
    void rebuild(const std::vector<KeyFrameT *> &kfs)
    {
        std::vector<const float *> depth, Tcw;
        std::vector<const uint8_t *> rgb;
        std::vector<std::vector<float>> poses;
        if (kfs.empty())
            return;
        ImageView d0 = adapt.depth(kfs[0]), c0 = adapt.rgb(kfs[0]);
        for (KeyFrameT *kf : kfs) {
            depth.push_back((const float *)adapt.depth(kf).data);
            rgb.push_back((const uint8_t *)adapt.rgb(kf).data);
            poses.emplace_back(16);
            adapt.pose(kf, poses.back().data());
        }
        for (auto &p : poses)
            Tcw.push_back(p.data());
        std::unique_lock<std::mutex> lck(cloudMutex);
        check(orbgpu_cloud_rebuild(cloud_, (int)kfs.size(), depth.data(), d0.step / sizeof(float), rgb.data(), c0.step,
                                   d0.cols, d0.rows, adapt.fx(kfs[0]), adapt.fy(kfs[0]), adapt.cx(kfs[0]),
                                   adapt.cy(kfs[0]), Tcw.data()),
              "PointCloudMapping::rebuild");
    }

    // globalMapRGBD (PointCloudMap.h:55)
    std::vector<orbgpu_point_xyzrgba> globalMap()
    {
        std::unique_lock<std::mutex> lck(cloudMutex);
        int64_t n = 0;
        check(orbgpu_cloud_size(cloud_, &n), "size");
        std::vector<orbgpu_point_xyzrgba> out((size_t)std::max<int64_t>(n, 1));
        check(orbgpu_cloud_download(cloud_, out.data(), (int64_t)out.size(), &n), "download");
        out.resize((size_t)n);
        return out;
    }

  protected:
    bool shutDownFlagLocked()
    {
        std::unique_lock<std::mutex> lck(shutDownMutex);
        return shutDownFlag;
    }
    KeyFrameT *keyframeAt(size_t i)
    {
        std::unique_lock<std::mutex> lck(keyframeMutex);
        return keyframes[i];
    }
    void insertOne(KeyFrameT *image_kf, KeyFrameT *pose_kf)
    {
        ImageView d = adapt.depth(image_kf), c = adapt.rgb(image_kf);
        float Tcw[16];
        adapt.pose(pose_kf, Tcw);
        std::unique_lock<std::mutex> lck(cloudMutex);
        check(orbgpu_cloud_insert(cloud_, (const float *)d.data, d.step / sizeof(float), (const uint8_t *)c.data, c.step,
                                  d.cols, d.rows, adapt.fx(image_kf), adapt.fy(image_kf), adapt.cx(image_kf),
                                  adapt.cy(image_kf), Tcw),
              "PointCloudMapping::insertKeyFrame");
    }

    orbgpu_cloud *cloud_ = nullptr;
    std::shared_ptr<std::thread> viewerThread;
    bool shutDownFlag = false, loopPending = false, quirks = true, busy = false, finished = false;
    std::mutex shutDownMutex, keyframeMutex, cloudMutex;
    std::condition_variable keyFrameUpdated, processed;
    std::vector<KeyFrameT *> keyframes;
    size_t lastKeyframeSize = 0;  // the reference's member (:207, :265)
    size_t seenSize = 0;          // keyframes.size() at the last wake-up (what a bare wait() + notify per insert amounts to)
    double resolution = 0.01;
    int sorMeanK = 50;          // sor.setMeanK(50), PointCloudMap.cc:46
    double sorStddevMul = 1.0;  // sor.setStddevMulThresh(1.0), :47
    Adapter adapt;
    LoopHooks hooks;
    std::string outputPath;
};

} // namespace orbgpu_shim

// KeyFrameDatabaseT's host-only parts -- the id -> pointer map and the marshalling of DBoW2::BowVector and of the neighbour
// lists -- as a stand-alone program (tests/test_kfdb_shim.py builds it with and without -fsanitize=address,undefined).
// It makes no call that binds the device: everything here is refused, or answered, on the host.
#include <cstdio>
#include <cstring>
#include <limits>

#include "kfdb_standin.hpp"

using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::KeyFrameDatabase;

#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);       \
            return 1;                                                     \
        }                                                                 \
    } while (0)

template <typename F> static bool throws(F f)
{
    try {
        f();
    } catch (const std::exception &) {
        return true;
    }
    return false;
}

int main(int argc, char **argv)
{
    if (argc != 2 || std::strcmp(argv[1], "run") != 0) {
        std::fprintf(stderr, "usage: kfdb_shim_test run\n");
        return 2;
    }
    // marshalling: the map's order is the ABI's order
    DBoW2::BowVector v;
    v[900] = 0.25, v[3] = 0.5, v[41] = 0.125, v[40] = 0.125;
    std::vector<int32_t> ids(7, -1);
    std::vector<double> vals(2, -1.0);
    KeyFrameDatabase::Flatten(v, ids, vals);
    EXPECT((ids == std::vector<int32_t>{3, 40, 41, 900}) && (vals == std::vector<double>{0.5, 0.125, 0.125, 0.25}));
    KeyFrameDatabase::Flatten(DBoW2::BowVector(), ids, vals);
    EXPECT(ids.empty() && vals.empty());

    // the pointer map: put / overwrite / erase / resolve in the order asked for, unknown ids skipped
    std::vector<KeyFrame> kfs(16);
    for (size_t i = 0; i < kfs.size(); i++)
        kfs[i].mnId = 100 + 3 * i;
    orbgpu_shim::IdPtrMap<KeyFrame> map;
    for (KeyFrame &k : kfs)
        map.put((int64_t)k.mnId, &k);
    map.put(103, &kfs[1]);
    EXPECT(map.size() == 16);
    const int64_t ask[] = {145, 100, 7, 103, 145};
    std::vector<KeyFrame *> got = map.Resolve(ask, 5);
    EXPECT(got.size() == 4 && got[0] == &kfs[15] && got[1] == &kfs[0] && got[2] == &kfs[1] && got[3] == &kfs[15]);
    map.erase(100), map.erase(5);
    got = map.Resolve(ask, 5);
    EXPECT(got.size() == 3 && got[0] == &kfs[15] && got[1] == &kfs[1]);
    EXPECT(map.Resolve(ask, 0).empty() && map.Resolve(nullptr, 0).empty());
    map.clear();
    EXPECT(map.size() == 0 && map.Resolve(ask, 5).empty());

    // the class over the C ABI, host-side answers only
    EXPECT(throws([] { KeyFrameDatabase bad(1000, 1); }));  // L2_NORM: refused
    EXPECT(throws([] { KeyFrameDatabase bad(0); }));
    KeyFrameDatabase db(1000, 0, 0, 2);
    EXPECT(db.size() == 0);
    for (size_t i = 1; i < kfs.size(); i++)
        kfs[0].mvpOrderedConnectedKeyFrames.push_back(&kfs[i]);  // 15 connected: the ten best are handed over
    db.UpdateCovisibles(&kfs[0]);  // outside the key frame's mutex: reads the list through GetBestCovisibilityKeyFrames
    {
        std::unique_lock<std::mutex> lock(kfs[1].mMutexConnections);  // inside it: the list is handed over
        db.UpdateCovisibles(&kfs[1], kfs[1].mvpOrderedConnectedKeyFrames);  // none
        db.UpdateCovisibles(&kfs[1], kfs[0].mvpOrderedConnectedKeyFrames);  // 15: ten are taken
    }
    kfs[2].mBowVec[1000] = 0.5;    // outside the vocabulary
    EXPECT(throws([&] { db.add(&kfs[2]); }));
    EXPECT(std::strstr(orbgpu_last_error_string(), "word id 1000") != nullptr);
    ORB_SLAM2::Frame f;
    f.mBowVec[5] = 1.0, f.mBowVec[2000] = 1.0;
    EXPECT(throws([&] { db.DetectRelocalizationCandidates(&f); }));
    kfs[3].mBowVec[4] = std::numeric_limits<double>::infinity();
    EXPECT(throws([&] { db.DetectLoopCandidates(&kfs[3], 0.1f); }));
    EXPECT(throws([&] { db.Score(&kfs[3], kfs[0].mvpOrderedConnectedKeyFrames); }));
    db.erase(&kfs[4]);  // not in the database: ignored
    db.clear();
    EXPECT(db.size() == 0);
    std::printf("kfdb shim ok\n");
    return 0;
}

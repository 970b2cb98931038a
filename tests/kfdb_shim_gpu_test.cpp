// INTEGRATION.md's KeyFrameDatabase block (section 2h) run on the device over one small scene: tests/test_kfdb_shim.py
// extracts the block into kfdb_block.inc, starts this program as a child process and compares what it prints with
// tests/kfdb_model.py.  Input (text): n_words n_kf, then per key frame `id n {word value}*n m {index}*m` (m ordered
// connected key frames as indices), the current key frame in the same form, the frame's vector `n {word value}*n`, and
// the index of a key frame to set bad before the last query.
#include <cstdio>
#include <cstring>
#include <deque>

#include "kfdb_standin.hpp"
#include "kfdb_block.inc"

using ORB_SLAM2::KeyFrame;

static bool read_vector(std::FILE *f, DBoW2::BowVector &v)
{
    int n = 0;
    if (std::fscanf(f, "%d", &n) != 1 || n < 0)
        return false;
    for (int i = 0; i < n; i++) {
        unsigned w;
        double x;
        if (std::fscanf(f, "%u %lf", &w, &x) != 2)
            return false;
        v[w] = x;
    }
    return true;
}

static bool read_keyframe(std::FILE *f, KeyFrame &kf, std::vector<int> &conn)
{
    unsigned long id;
    int m = 0;
    if (std::fscanf(f, "%lu", &id) != 1 || !read_vector(f, kf.mBowVec) || std::fscanf(f, "%d", &m) != 1 || m < 0)
        return false;
    kf.mnId = id;
    conn.resize((size_t)m);
    for (int &c : conn)
        if (std::fscanf(f, "%d", &c) != 1)
            return false;
    return true;
}

static void print(const char *tag, const std::vector<KeyFrame *> &v)
{
    std::printf("%s %zu", tag, v.size());
    for (KeyFrame *p : v)
        std::printf(" %lu", p->mnId);
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: kfdb_shim_gpu_test scene.txt\n");
        return 2;
    }
    std::FILE *f = std::fopen(argv[1], "r");
    int n_words = 0, n_kf = 0, bad = -1;
    if (!f || std::fscanf(f, "%d %d", &n_words, &n_kf) != 2 || n_kf < 0)
        return 3;
    std::deque<KeyFrame> kfs((size_t)n_kf + 1);  // the last one is the current key frame
    std::vector<std::vector<int>> conn((size_t)n_kf + 1);
    for (int i = 0; i <= n_kf; i++)
        if (!read_keyframe(f, kfs[(size_t)i], conn[(size_t)i]))
            return 3;
    ORB_SLAM2::Frame frame;
    if (!read_vector(f, frame.mBowVec) || std::fscanf(f, "%d", &bad) != 1 || bad < 0 || bad >= n_kf)
        return 3;
    std::fclose(f);
    for (int i = 0; i <= n_kf; i++)
        for (int c : conn[(size_t)i]) {
            if (c < 0 || c >= n_kf)
                return 3;
            kfs[(size_t)i].mvpOrderedConnectedKeyFrames.push_back(&kfs[(size_t)c]);
        }
    try {
        ORB_SLAM2::KeyFrameDatabase db(n_words, 0, 0, 2);
        for (int i = 0; i <= n_kf; i++)
            kfs[(size_t)i].mpKeyFrameDB = &db;
        for (int i = 0; i < n_kf; i++) {
            kfs[(size_t)i].UpdateBestCovisibles();  // names key frames that are added later
            db.add(&kfs[(size_t)i]);                 // LoopClosing.cc:117
        }
        KeyFrame *cur = &kfs[(size_t)n_kf];
        print("LOOP", ORB_SLAM2::LoopCandidates(&db, cur));
        print("RELOC", ORB_SLAM2::RelocalizationCandidates(&db, &frame));
        kfs[(size_t)bad].SetBadFlag();  // KeyFrame.cc:582
        print("RELOC2", ORB_SLAM2::RelocalizationCandidates(&db, &frame));
        db.add(cur);  // LoopClosing.cc:147
        std::printf("SIZE %d\n", db.size());
        db.clear();  // Tracking.cc:1828
        print("RELOC3", ORB_SLAM2::RelocalizationCandidates(&db, &frame));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    std::printf("kfdb shim ok\n");
    return 0;
}

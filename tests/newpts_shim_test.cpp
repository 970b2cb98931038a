// orbgpu_shim::NewPointsCall / CreateNewMapPointsT over stand-in key frames from a file of tests/test_newpts_shim.py.
// Arguments: in.bin out.txt.  Without NEWPTS_RUN_ON_DEVICE the library is not called: the outputs in in.bin (the model's)
// are injected before the write-back, so the program needs no device.  With it (newpts_shim_gpu_test.cpp) the whole
// LocalMapping::CreateNewMapPoints of INTEGRATION.md runs once.  out.txt: one record per line, see the puts below.
#include <fstream>
#include <iostream>

#include "newpts_standin.hpp"
#include "newpts_block.inc"  // INTEGRATION.md's newpts-snippet, written out by the test

using namespace ORB_SLAM2;

namespace ORB_SLAM2 {
MapPointTable *gpMapPointTable = NULL;
}

struct Reader {
    std::ifstream f;
    explicit Reader(const char *path) : f(path, std::ios::binary)
    {
        if (!f)
            throw std::runtime_error("cannot open input");
    }
    template <typename T> T one()
    {
        T v;
        f.read(reinterpret_cast<char *>(&v), sizeof(T));
        return v;
    }
    template <typename T> std::vector<T> many(size_t n)
    {
        std::vector<T> v(n);
        f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(n * sizeof(T)));
        if (!f)
            throw std::runtime_error("short input");
        return v;
    }
};

static cv::Mat mat_of(const std::vector<float> &v, int r, int c)
{
    cv::Mat m(r, c, CV_32F);
    std::memcpy(m.data, v.data(), 4 * (size_t)r * c);
    return m;
}

static void read_frame(Reader &in, KeyFrame &kf, int id)
{
    kf.mnId = (long unsigned int)id;
    const int n = kf.N = in.one<int32_t>(), nl = in.one<int32_t>();
    kf.mb = in.one<float>(), kf.mfScaleFactor = in.one<float>();
    const std::vector<float> K = in.many<float>(7);
    kf.fx = K[0], kf.fy = K[1], kf.cx = K[2], kf.cy = K[3], kf.invfx = K[4], kf.invfy = K[5], kf.mbf = K[6];
    kf.Tcw = mat_of(in.many<float>(16), 4, 4), kf.Twc = mat_of(in.many<float>(16), 4, 4);
    kf.median_depth = in.one<float>();
    kf.F12 = mat_of(in.many<float>(9), 3, 3);
    kf.mvLevelSigma2 = in.many<float>((size_t)nl), kf.mvScaleFactors = in.many<float>((size_t)nl);
    const std::vector<float> x = in.many<float>(n), y = in.many<float>(n);
    const std::vector<int32_t> oct = in.many<int32_t>(n);
    const std::vector<float> ang = in.many<float>(n);
    kf.mvuRight = in.many<float>(n), kf.mvDepth = in.many<float>(n);
    const std::vector<float> raw = in.many<float>(2 * (size_t)n);
    const std::vector<int32_t> node = in.many<int32_t>(n), has = in.many<int32_t>(n);
    const std::vector<uint8_t> desc = in.many<uint8_t>(32 * (size_t)n);
    kf.mvKeys.resize(n), kf.mvKeysUn.resize(n), kf.mvpMapPoints.assign(n, static_cast<MapPoint *>(NULL));
    kf.mDescriptors.create(std::max(n, 1), 32, CV_8U);
    static cv::Mat nowhere(3, 1, CV_32F);
    for (int i = 0; i < n; i++) {
        kf.mvKeysUn[i].pt.x = x[i], kf.mvKeysUn[i].pt.y = y[i], kf.mvKeysUn[i].octave = oct[i], kf.mvKeysUn[i].angle = ang[i];
        kf.mvKeys[i] = kf.mvKeysUn[i];
        kf.mvKeys[i].pt.x = raw[2 * i], kf.mvKeys[i].pt.y = raw[2 * i + 1];
        if (node[i] >= 0)
            kf.mFeatVec[(unsigned)node[i]].push_back((unsigned)i);
        if (has[i])
            kf.mvpMapPoints[i] = new MapPoint(nowhere, &kf, static_cast<Map *>(NULL));  // an older point
        std::memcpy(kf.mDescriptors.ptr<uint8_t>(i), &desc[32 * (size_t)i], 32);
    }
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::cerr << "usage: newpts_shim_test in.bin out.txt\n";
        return 2;
    }
    try {
        Reader in(argv[1]);
        const int nframes = in.one<int32_t>(), mono = in.one<int32_t>(), stop = in.one<int32_t>();
        std::vector<KeyFrame> kfs((size_t)nframes);
        for (int k = 0; k < nframes; k++)
            read_frame(in, kfs[(size_t)k], k);
        const long unsigned int first_new = MapPoint::nNextId;
        Map map;
        LocalMapping lm;
        lm.mbMonocular = mono != 0, lm.mpMap = &map, lm.mpCurrentKeyFrame = &kfs[0], lm.new_keyframes = stop != 0;
        for (int k = 1; k < nframes; k++)
            kfs[0].best.push_back(&kfs[(size_t)k]);
        std::ofstream out(argv[2]);
        out.precision(9);
#ifdef NEWPTS_RUN_ON_DEVICE
        MapPointTable table(0, 0);
        gpMapPointTable = &table;
        lm.CreateNewMapPoints();
        // what the batched Upsert left in the table, per created point
        for (MapPoint *p : map.added) {
            float w[3], nrm[3], mn = 0, mx = 0;
            uint8_t d[32];
            int32_t obs = 0, bad = 0;
            orbgpu_shim::check(orbgpu_mappoint_table_read(table.handle(), (int64_t)p->mnId, w, nrm, &mn, &mx, d, &obs, &bad), "read");
            out << "row " << (p->mnId - first_new) << " " << w[0] << " " << w[1] << " " << w[2] << " " << nrm[0] << " " << nrm[1] << " "
                << nrm[2] << " " << mn << " " << mx << " " << (int)d[0] << " " << (int)d[31] << " " << obs << " " << bad << "\n";
        }
        out << "rows " << table.rows() << "\n";
        gpMapPointTable = NULL;
#else
        const int n1 = kfs[0].N;
        NewPointsAccess access{&lm, cv::Mat(), cv::Mat(), cv::Mat(), cv::Mat()};
        orbgpu_shim::NewPointsCall<KeyFrame> call(&kfs[0], kfs[0].GetBestCovisibilityKeyFrames(mono ? 20 : 10), mono != 0,
                                                  lm.CheckNewKeyFrames(), access);
        out << "kept";
        for (KeyFrame *k : call.kept)
            out << " " << k->mnId;
        out << "\n";
        for (size_t k = 0; k < call.kept.size(); k++) {
            const orbgpu_new_points_frame &f = call.nb[k];
            out << "neighbour " << call.kept[k]->mnId << " " << f.ex << " " << f.ey << " " << f.n << " " << f.nlevels;
            for (int i = 0; i < f.n; i++)
                out << " " << f.cos_stereo[i] << " " << (int)f.has_mp[i] << " " << f.node[i] << " " << f.kp_raw[2 * i];
            out << "\n";
        }
        out << "problem " << call.p.nn << " " << call.p.only_stereo << " " << call.p.check_orientation << " " << call.p.ratio_factor
            << " " << call.p.kf1.n << "\n";
        const int nk = in.one<int32_t>();
        if (nk != (int)call.kept.size())
            throw std::runtime_error("the model kept another number of neighbours");
        const size_t cells = (size_t)nk * (size_t)n1;
        const std::vector<int32_t> m = in.many<int32_t>(cells), s = in.many<int32_t>(cells);
        const std::vector<float> x = in.many<float>(3 * cells);
        std::copy(m.begin(), m.end(), call.match12.begin()), std::copy(s.begin(), s.end(), call.status.begin());
        std::copy(x.begin(), x.end(), call.x3d.begin());
        out << "nnew " << call.WriteBack<MapPoint>(access, static_cast<MapPointTable *>(NULL)) << "\n";
#endif
        // the object graph the reference's loop leaves behind
        for (MapPoint *p : map.added) {
            out << "point " << (p->mnId - first_new) << " " << p->mWorldPos.ptr<float>()[0] << " " << p->mWorldPos.ptr<float>()[1] << " "
                << p->mWorldPos.ptr<float>()[2] << " ref " << p->mpRefKF->mnId << " obs";
            for (KeyFrame *k : p->order)
                out << " " << k->mnId << ":" << p->mObservations[k];
            out << " calls " << p->nDescriptors << " " << p->nUpdates << " " << (int)p->held_at_descriptor << "\n";
        }
        out << "recent";
        for (MapPoint *p : lm.mlpRecentAddedMapPoints)
            out << " " << (p->mnId - first_new);
        out << "\n";
        for (int k = 0; k < nframes; k++) {
            out << "holds " << k;
            for (MapPoint *p : kfs[(size_t)k].mvpMapPoints)
                out << " " << (p == NULL ? -1 : p->mnId < first_new ? -2 : (long)(p->mnId - first_new));
            out << "\n";
        }
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    std::cout << "newpts shim ok\n";
    return 0;
}

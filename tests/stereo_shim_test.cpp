// Frame::ComputeStereoMatches through the C++ shim (ComputeStereoMatchesT) on a stand-in Frame that carries the
// reference's stereo members (Frame.h:100-190).  Arguments: left.raw right.raw width height nfeatures mbf fx out.bin;
// writes N, mvuRight[N], mvDepth[N] for tests/test_stereo_shim.py to compare with the host entry point.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>

#include "orbgpu_shim.hpp"

struct Point2f { float x, y; };
struct KeyPoint { Point2f pt; float size, angle, response; int octave, class_id; };  // cv::KeyPoint layout

struct StereoFrame {  // the members ComputeStereoMatches reads and writes
    int N = 0;
    std::vector<KeyPoint> mvKeys, mvKeysRight;
    std::vector<uint8_t> mDescriptors, mDescriptorsRight;
    std::vector<float> mvuRight, mvDepth;
    float mbf = 0, mb = 0;
    static float fx;
};
float StereoFrame::fx = 0;

static std::vector<uint8_t> read_file(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv)
{
    if (argc != 9) {
        std::cerr << "usage: stereo_shim_test left.raw right.raw width height nfeatures mbf fx out.bin\n";
        return 2;
    }
    const int w = atoi(argv[3]), h = atoi(argv[4]), nf = atoi(argv[5]);
    const std::vector<uint8_t> left = read_file(argv[1]), right = read_file(argv[2]);
    if ((int)left.size() != w * h || (int)right.size() != w * h) {
        std::cerr << "bad image size\n";
        return 1;
    }
    try {
        orbgpu_shim::ORBextractorT<KeyPoint> el(nf, 1.2f, 8, 20, 7), er(nf, 1.2f, 8, 20, 7);
        StereoFrame F;
        el(left.data(), h, w, (size_t)w, F.mvKeys, F.mDescriptors);  // Frame.cc:73-75 (two threads there)
        er(right.data(), h, w, (size_t)w, F.mvKeysRight, F.mDescriptorsRight);
        F.N = (int)F.mvKeys.size();
        F.mbf = (float)atof(argv[6]);
        StereoFrame::fx = (float)atof(argv[7]);
        orbgpu_shim::ComputeStereoMatchesT(F, el, er);  // Frame.cc:90
        F.mb = F.mbf / StereoFrame::fx;                 // Frame.cc:114
        std::ofstream o(argv[8], std::ios::binary);
        const int32_t n = F.N;
        o.write(reinterpret_cast<const char *>(&n), 4);
        o.write(reinterpret_cast<const char *>(F.mvuRight.data()), 4 * (std::streamsize)n);
        o.write(reinterpret_cast<const char *>(F.mvDepth.data()), 4 * (std::streamsize)n);
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    std::cout << "stereo shim ok\n";
    return 0;
}

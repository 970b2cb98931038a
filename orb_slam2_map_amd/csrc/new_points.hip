// LocalMapping::CreateNewMapPoints (LocalMapping.cc:207-452): the neighbour loop as one chain of launches on one stream.
// Per neighbour: k_np_latch (the stop decision, N12), k_np_match + k_np_finish (SearchForTriangulation through the bodies
// of tri_match.h, N1), k_np_triangulate (one lane per key point of key frame 1, N2-N11), which also sets the working
// has_mp bit the next neighbour's matcher reads.  Conventions N1-N13: include/orbgpu.h; restatement: tests/newpts_model.py.
#include <algorithm>
#include <cstring>
#include <vector>

#include "carve.h"
#include "common.h"
#include "jacobi.h"
#include "staging.h"
#include "tri_match.h"

namespace orbgpu {
namespace {

using Frame = orbgpu_new_points_frame;

enum { NP_WORK, NP_IN, NP_OUT, NP_N_BUF };
struct NpWs : Staging<NP_N_BUF> {
    std::vector<uint8_t> h_in, h_out;  // the host flavour's two blocks
};

__device__ inline float np_fdiv(float a, float b) { return (float)((double)a / (double)b); }
__device__ inline float np_finv(float x) { return (float)(1.0 / (double)x); }
// Mat::dot of a float row of T (3 entries from T[o]) with (x, y, z), plus the float t: an FP64 sum rounded once (N8)
__device__ inline float np_row(const float *T, int o, float x, float y, float z)
{
    return (float)((((double)T[o] * (double)x + (double)T[o + 1] * (double)y) + (double)T[o + 2] * (double)z) + (double)T[o + 3]);
}
__device__ inline float np_norm3(float x, float y, float z)
{
    return (float)sqrt(((double)x * (double)x + (double)y * (double)y) + (double)z * (double)z);
}

// N12: go[k] = neighbour k is processed.  One workgroup, one lane reads the flag.
__global__ __launch_bounds__(64) void k_np_latch(int k, const int *__restrict__ stop, int *__restrict__ go, int *__restrict__ n_done)
{
    if (threadIdx.x != 0)
        return;
    int g = 1;
    if (k > 0)
        g = go[k - 1] && !(stop && *reinterpret_cast<const volatile int *>(stop) != 0);
    go[k] = g;
    if (g)
        *n_done = k + 1;
}

__global__ __launch_bounds__(256) void k_np_match(const int *__restrict__ go, Frame K1, const uint8_t *__restrict__ work_has,
                                                  Frame K2, TriParams P, int *__restrict__ match12)
{
    if (!*go)
        return;
    tri_match_wave<true>(K1.n, K1.kp_x, K1.kp_y, K1.u_right, work_has, K1.node, K1.desc, K2.n, K2.kp_x, K2.kp_y, K2.kp_octave,
                         K2.u_right, K2.has_mp, K2.node, K2.desc, P, match12);
}

__global__ __launch_bounds__(1024) void k_np_finish(const int *__restrict__ go, int n1, const float *__restrict__ angle1,
                                                    const float *__restrict__ angle2, int check_orientation,
                                                    int *__restrict__ match12, int *__restrict__ nmatches)
{
    if (!*go)
        return;
    tri_finish_block(n1, angle1, angle2, check_orientation, match12, nmatches);
}

// KeyFrame::UnprojectStereo (N6); false: depth <= 0 (D2)
__device__ inline bool np_unproject(const Frame &K, int i, float &X, float &Y, float &Z)
{
    const float z = K.depth[i];
    if (!(z > 0.f))
        return false;
    const float u = K.kp_raw ? K.kp_raw[2 * i] : K.kp_x[i], v = K.kp_raw ? K.kp_raw[2 * i + 1] : K.kp_y[i];
    const float x = ((u - K.cx) * z) * K.invfx, y = ((v - K.cy) * z) * K.invfy;
    const float *T = K.Twc;
    X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    Y = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    Z = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
    return true;
}

// one matched pair (i of key frame 1, j of key frame 2): :286-431
__device__ inline int np_pair(const Frame &K1, const Frame &K2, float ratio_factor, int i, int j, float &X, float &Y, float &Z)
{
    const int o1 = K1.kp_octave[i], o2 = K2.kp_octave[j];
    if ((unsigned)o1 >= (unsigned)K1.nlevels || (unsigned)o2 >= (unsigned)K2.nlevels)
        return ORBGPU_NP_BAD_OCTAVE;
    const float px1 = K1.kp_x[i], py1 = K1.kp_y[i], ur1 = K1.u_right[i];
    const float px2 = K2.kp_x[j], py2 = K2.kp_y[j], ur2 = K2.u_right[j];
    const bool s1 = ur1 >= 0, s2 = ur2 >= 0;
    const float *T1 = K1.Tcw, *T2 = K2.Tcw;
    // N2
    const float xn1[3] = {(px1 - K1.cx) * K1.invfx, (py1 - K1.cy) * K1.invfy, 1.0f};
    const float xn2[3] = {(px2 - K2.cx) * K2.invfx, (py2 - K2.cy) * K2.invfy, 1.0f};
    float r1[3], r2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        r1[r] = (T1[r] * xn1[0] + T1[4 + r] * xn1[1]) + T1[8 + r] * xn1[2];
        r2[r] = (T2[r] * xn2[0] + T2[4 + r] * xn2[1]) + T2[8 + r] * xn2[2];
    }
    // N3
    const double dot = ((double)r1[0] * (double)r2[0] + (double)r1[1] * (double)r2[1]) + (double)r1[2] * (double)r2[2];
    const double nr1 = sqrt(((double)r1[0] * (double)r1[0] + (double)r1[1] * (double)r1[1]) + (double)r1[2] * (double)r1[2]);
    const double nr2 = sqrt(((double)r2[0] * (double)r2[0] + (double)r2[1] * (double)r2[1]) + (double)r2[2] * (double)r2[2]);
    const float cos_rays = (float)(dot / (nr1 * nr2));
    const float cs = cos_rays + 1.0f;
    float cs1 = cs, cs2 = cs;
    if (s1)
        cs1 = K1.cos_stereo[i];
    else if (s2)
        cs2 = K2.cos_stereo[j];
    const float cs_min = cs2 < cs1 ? cs2 : cs1;  // std::min(cs1, cs2)
    int made;
    if (cos_rays < cs_min && cos_rays > 0 && (s1 || s2 || (double)cos_rays < 0.9998)) {
        float Af[4][4];  // N4
#pragma unroll
        for (int c = 0; c < 4; c++) {
            Af[0][c] = xn1[0] * T1[8 + c] - T1[c];
            Af[1][c] = xn1[1] * T1[8 + c] - T1[4 + c];
            Af[2][c] = xn2[0] * T2[8 + c] - T2[c];
            Af[3][c] = xn2[1] * T2[8 + c] - T2[4 + c];
        }
        float x4[4];
        null_vector4(Af, x4);  // N5
        if (x4[3] == 0.f)
            return ORBGPU_NP_W_ZERO;
        X = np_fdiv(x4[0], x4[3]), Y = np_fdiv(x4[1], x4[3]), Z = np_fdiv(x4[2], x4[3]);
        made = ORBGPU_NP_TRIANGULATED;
    } else if (s1 && cs1 < cs2) {
        if (!np_unproject(K1, i, X, Y, Z))
            return ORBGPU_NP_STEREO_DEPTH;
        made = ORBGPU_NP_UNPROJECT1;
    } else if (s2 && cs2 < cs1) {
        if (!np_unproject(K2, j, X, Y, Z))
            return ORBGPU_NP_STEREO_DEPTH;
        made = ORBGPU_NP_UNPROJECT2;
    } else {
        return ORBGPU_NP_LOW_PARALLAX;
    }
    if (!((X - X == 0.f) && (Y - Y == 0.f) && (Z - Z == 0.f)))  // N7
        return ORBGPU_NP_NON_FINITE;
    const float z1 = np_row(T1, 8, X, Y, Z);  // N8
    if (z1 <= 0)
        return ORBGPU_NP_Z1;
    const float z2 = np_row(T2, 8, X, Y, Z);
    if (z2 <= 0)
        return ORBGPU_NP_Z2;
    {  // N9, key frame 1
        const float sg = K1.level_sigma2[o1];
        const float xc = np_row(T1, 0, X, Y, Z), yc = np_row(T1, 4, X, Y, Z), invz = np_finv(z1);
        const float u = (K1.fx * xc) * invz + K1.cx, v = (K1.fy * yc) * invz + K1.cy;
        const float ex = u - px1, ey = v - py1;
        if (!s1) {
            if ((double)(ex * ex + ey * ey) > 5.991 * (double)sg)
                return ORBGPU_NP_REPROJ1;
        } else {
            const float er = (u - K1.mbf * invz) - ur1;
            if ((double)((ex * ex + ey * ey) + er * er) > 7.8 * (double)sg)
                return ORBGPU_NP_REPROJ1;
        }
    }
    {  // key frame 2, with key frame 1's mbf (:406)
        const float sg = K2.level_sigma2[o2];
        const float xc = np_row(T2, 0, X, Y, Z), yc = np_row(T2, 4, X, Y, Z), invz = np_finv(z2);
        const float u = (K2.fx * xc) * invz + K2.cx, v = (K2.fy * yc) * invz + K2.cy;
        const float ex = u - px2, ey = v - py2;
        if (!s2) {
            if ((double)(ex * ex + ey * ey) > 5.991 * (double)sg)
                return ORBGPU_NP_REPROJ2;
        } else {
            const float er = (u - K1.mbf * invz) - ur2;
            if ((double)((ex * ex + ey * ey) + er * er) > 7.8 * (double)sg)
                return ORBGPU_NP_REPROJ2;
        }
    }
    // N10
    const float d1 = np_norm3(X - K1.Twc[3], Y - K1.Twc[7], Z - K1.Twc[11]);
    const float d2 = np_norm3(X - K2.Twc[3], Y - K2.Twc[7], Z - K2.Twc[11]);
    if (d1 == 0 || d2 == 0)
        return ORBGPU_NP_ZERO_DIST;
    const float ratio_dist = np_fdiv(d2, d1);
    const float ratio_octave = np_fdiv(K1.scale_factors[o1], K2.scale_factors[o2]);
    if (ratio_dist * ratio_factor < ratio_octave || ratio_dist > ratio_octave * ratio_factor)
        return ORBGPU_NP_SCALE;
    return made;
}

// one lane per key point of key frame 1
__global__ __launch_bounds__(64) void k_np_triangulate(const int *__restrict__ go, Frame K1, Frame K2, float ratio_factor,
                                                       const int *__restrict__ match12, int *__restrict__ status,
                                                       float *__restrict__ x3d, uint8_t *__restrict__ work_has,
                                                       int *__restrict__ n_created)
{
    if (!*go)
        return;
    const int i = blockIdx.x * 64 + threadIdx.x;
    int st = ORBGPU_NP_NONE;
    float X = 0.f, Y = 0.f, Z = 0.f;
    if (i < K1.n) {
        const int j = match12[i];
        if (j >= 0 && j < K2.n)
            st = np_pair(K1, K2, ratio_factor, i, j, X, Y, Z);
        status[i] = st;
        if (st > 0) {
            x3d[3 * (size_t)i] = X, x3d[3 * (size_t)i + 1] = Y, x3d[3 * (size_t)i + 2] = Z;
            work_has[i] = 1;
        }
    }
    const int c = __popcll(__ballot(st > 0));
    if (threadIdx.x == 0 && c > 0)
        atomicAdd(n_created, c);
}

int check_frame(const Frame &f, const char *what, int k, bool orientation)
{
    ORBGPU_REQUIRE(f.n >= 0 && f.n <= 65535, "%s %d: key point count outside [0, 65535]", what, k);
    ORBGPU_REQUIRE(f.nlevels >= 1 && f.nlevels <= ORBGPU_MAX_LEVELS, "%s %d: nlevels outside [1, %d]", what, k, ORBGPU_MAX_LEVELS);
    if (f.n > 0) {
        ORBGPU_REQUIRE(f.kp_x && f.kp_y && f.kp_octave && f.u_right && f.desc && f.has_mp && f.node && f.depth && f.cos_stereo,
                       "%s %d: null key-frame arrays", what, k);
        ORBGPU_REQUIRE(!orientation || f.kp_angle, "%s %d: orientation check needs angles", what, k);
    }
    return ORBGPU_OK;
}

int check_problem(const orbgpu_new_points_problem *p)
{
    ORBGPU_REQUIRE(p, "null argument");
    ORBGPU_REQUIRE(p->nn >= 0 && p->nn <= ORBGPU_NEW_POINTS_MAX_NEIGHBOURS, "neighbour count outside [0, %d]",
                   ORBGPU_NEW_POINTS_MAX_NEIGHBOURS);
    ORBGPU_REQUIRE(p->nn == 0 || p->neighbours, "null neighbours");
    int rc = check_frame(p->kf1, "key frame", 1, p->check_orientation != 0);
    for (int k = 0; k < p->nn && rc == ORBGPU_OK; k++)
        rc = check_frame(p->neighbours[k], "neighbour", k, p->check_orientation != 0);
    if (rc != ORBGPU_OK)
        return rc;
    ORBGPU_REQUIRE(p->n_done, "null n_done");
    ORBGPU_REQUIRE(p->nn == 0 || (p->n_matches && p->n_created), "null count arrays");
    ORBGPU_REQUIRE(p->nn == 0 || p->kf1.n == 0 || (p->match12 && p->status && p->x3d), "null output arrays");
    return ORBGPU_OK;
}

// the frame with every level beyond nlevels zeroed, as the kernels expect (sigma2 = 0 fails the epipolar test)
Frame device_frame(const Frame &f)
{
    Frame d = f;
    for (int l = f.nlevels; l < ORBGPU_MAX_LEVELS; l++)
        d.level_sigma2[l] = d.scale_factors[l] = 0.f;
    return d;
}

} // namespace
} // namespace orbgpu

using namespace orbgpu;

extern "C" int orbgpu_create_new_map_points_device(const orbgpu_new_points_problem *p, int32_t device_id, void *hip_stream)
{
    int rc = check_problem(p);
    if (rc != ORBGPU_OK || (rc = select_device(device_id)) != ORBGPU_OK)
        return rc;
    NpWs &ws = per_device_workspace<NpWs>(device_id);
    if ((rc = ws.bind(device_id, false)) != ORBGPU_OK)
        return rc;
    const int nn = p->nn, n1 = p->kf1.n;
    const size_t w1 = (size_t)n1, cells = (size_t)nn * w1;
    // the working copy of has_mp1, then go[nn]
    const size_t off_go = (w1 + 15) & ~(size_t)15;
    ws.reserve(NP_WORK, off_go + 4 * (size_t)std::max(nn, 1));
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    const hipStream_t st = (hipStream_t)hip_stream;
    uint8_t *work_has = ws.as<uint8_t>(NP_WORK);
    int *go = ws.at<int>(NP_WORK, off_go);
    ORBGPU_HIP_TRY(hipMemsetAsync(p->n_done, 0, sizeof(int32_t), st));
    if (nn > 0) {
        ORBGPU_HIP_TRY(hipMemsetAsync(p->n_matches, 0, 4 * (size_t)nn, st));
        ORBGPU_HIP_TRY(hipMemsetAsync(p->n_created, 0, 4 * (size_t)nn, st));
    }
    if (cells > 0) {
        ORBGPU_HIP_TRY(hipMemsetAsync(p->match12, 0xFF, 4 * cells, st));  // -1
        ORBGPU_HIP_TRY(hipMemsetAsync(p->status, 0, 4 * cells, st));
        ORBGPU_HIP_TRY(hipMemsetAsync(p->x3d, 0, 12 * cells, st));
        ORBGPU_HIP_TRY(hipMemcpyAsync(work_has, p->kf1.has_mp, w1, hipMemcpyDeviceToDevice, st));
    }
    const Frame K1 = device_frame(p->kf1);
    for (int k = 0; k < nn; k++) {
        hipLaunchKernelGGL(k_np_latch, dim3(1), dim3(64), 0, st, k, p->stop, go, p->n_done);
        const Frame K2 = device_frame(p->neighbours[k]);
        if (n1 == 0 || K2.n == 0)
            continue;  // nothing can match: the outputs keep their initial values
        TriParams P;
        for (int e = 0; e < 9; e++)
            P.F12[e] = K2.F12[e];
        P.ex = K2.ex, P.ey = K2.ey, P.only_stereo = p->only_stereo ? 1 : 0;
        for (int l = 0; l < ORBGPU_MAX_LEVELS; l++)
            P.sigma2[l] = K2.level_sigma2[l], P.scale[l] = K2.scale_factors[l];
        int *match = p->match12 + (size_t)k * w1;
        hipLaunchKernelGGL(k_np_match, dim3((n1 + 3) / 4), dim3(256), 0, st, go + k, K1, work_has, K2, P, match);
        hipLaunchKernelGGL(k_np_finish, dim3(1), dim3(1024), 0, st, go + k, n1, K1.kp_angle, K2.kp_angle,
                           p->check_orientation ? 1 : 0, match, p->n_matches + k);
        hipLaunchKernelGGL(k_np_triangulate, dim3((n1 + 63) / 64), dim3(64), 0, st, go + k, K1, K2, p->ratio_factor, match,
                           p->status + (size_t)k * w1, p->x3d + 3 * (size_t)k * w1, work_has, p->n_created + k);
    }
    ORBGPU_HIP_TRY(hipGetLastError());
    return ORBGPU_OK;
}

namespace {

// the segments of one frame inside the host flavour's input block
struct FrameSeg {
    size_t x, y, oct, ang, ur, desc, has, node, depth, raw, cs;
};

FrameSeg carve_frame(Carver &c, const Frame &f)
{
    const size_t n = (size_t)f.n;
    FrameSeg s;
    s.desc = c.take(32 * n), s.x = c.take(4 * n), s.y = c.take(4 * n), s.oct = c.take(4 * n), s.ang = c.take(4 * n);
    s.ur = c.take(4 * n), s.node = c.take(4 * n), s.depth = c.take(4 * n), s.raw = c.take(8 * n), s.cs = c.take(4 * n);
    s.has = c.take(n);
    return s;
}

void pack_frame(uint8_t *base, const FrameSeg &s, const Frame &f)
{
    const size_t n = (size_t)f.n;
    if (n == 0)
        return;
    auto put = [&](size_t off, const void *src, size_t bytes) {
        if (src)
            memcpy(base + off, src, bytes);
    };
    put(s.desc, f.desc, 32 * n), put(s.x, f.kp_x, 4 * n), put(s.y, f.kp_y, 4 * n), put(s.oct, f.kp_octave, 4 * n);
    put(s.ang, f.kp_angle, 4 * n), put(s.ur, f.u_right, 4 * n), put(s.node, f.node, 4 * n), put(s.depth, f.depth, 4 * n);
    put(s.raw, f.kp_raw, 8 * n), put(s.cs, f.cos_stereo, 4 * n), put(s.has, f.has_mp, n);
}

Frame point_frame(uint8_t *dev, const FrameSeg &s, const Frame &f)
{
    Frame d = f;
    d.desc = dev + s.desc, d.has_mp = dev + s.has;
    d.kp_x = reinterpret_cast<const float *>(dev + s.x), d.kp_y = reinterpret_cast<const float *>(dev + s.y);
    d.kp_octave = reinterpret_cast<const int32_t *>(dev + s.oct);
    d.kp_angle = f.kp_angle ? reinterpret_cast<const float *>(dev + s.ang) : nullptr;
    d.u_right = reinterpret_cast<const float *>(dev + s.ur), d.node = reinterpret_cast<const int32_t *>(dev + s.node);
    d.depth = reinterpret_cast<const float *>(dev + s.depth);
    d.kp_raw = f.kp_raw ? reinterpret_cast<const float *>(dev + s.raw) : nullptr;
    d.cos_stereo = reinterpret_cast<const float *>(dev + s.cs);
    return d;
}

int check_octaves(const Frame &f, const char *what, int k)
{
    for (int i = 0; i < f.n; i++)
        ORBGPU_REQUIRE(f.kp_octave[i] >= 0 && f.kp_octave[i] < f.nlevels, "%s %d: key point %d: octave out of range", what, k, i);
    return ORBGPU_OK;
}

} // namespace

extern "C" int orbgpu_create_new_map_points(const orbgpu_new_points_problem *p, int32_t device_id)
{
    int rc = check_problem(p);
    if (rc != ORBGPU_OK)
        return rc;
    const int nn = p->nn, n1 = p->kf1.n;
    rc = check_octaves(p->kf1, "key frame", 1);
    for (int k = 0; k < nn && rc == ORBGPU_OK; k++)
        rc = check_octaves(p->neighbours[k], "neighbour", k);
    if (rc != ORBGPU_OK)
        return rc;
    const size_t cells = (size_t)nn * (size_t)n1, cn = (size_t)std::max(nn, 1);
    Carver in(16), out(16);
    const size_t i_stop = in.take(4);
    const FrameSeg s1 = carve_frame(in, p->kf1);
    std::vector<FrameSeg> s2((size_t)nn);
    for (int k = 0; k < nn; k++)
        s2[k] = carve_frame(in, p->neighbours[k]);
    const size_t o_done = out.take(4), o_nm = out.take(4 * cn), o_nc = out.take(4 * cn), o_match = out.take(4 * cells),
                 o_status = out.take(4 * cells), o_x = out.take(12 * cells);
    NpWs *wsp;
    if ((rc = host_begin(device_id, NP_IN, in.off, NP_OUT, out.off, wsp)) != ORBGPU_OK)
        return rc;
    NpWs &ws = *wsp;
    NpWs::FinishOnError on_error{ws};
    ws.h_in.assign(in.off, 0), ws.h_out.assign(out.off, 0);
    uint8_t *hb = ws.h_in.data(), *dev = ws.as<uint8_t>(NP_IN), *dout = ws.as<uint8_t>(NP_OUT);
    const int32_t stop_now = p->stop ? *p->stop : 0;
    memcpy(hb + i_stop, &stop_now, 4);
    pack_frame(hb, s1, p->kf1);
    for (int k = 0; k < nn; k++)
        pack_frame(hb, s2[k], p->neighbours[k]);
    ws.upload(NP_IN, hb, in.off);  // the one upload
    if ((rc = ws.status()) != ORBGPU_OK)
        return rc;
    orbgpu_new_points_problem d = *p;
    std::vector<Frame> nb((size_t)nn);
    d.kf1 = point_frame(dev, s1, p->kf1);
    for (int k = 0; k < nn; k++)
        nb[k] = point_frame(dev, s2[k], p->neighbours[k]);
    d.neighbours = nb.data();
    d.stop = p->stop ? reinterpret_cast<const int32_t *>(dev + i_stop) : nullptr;
    d.n_done = reinterpret_cast<int32_t *>(dout + o_done), d.n_matches = reinterpret_cast<int32_t *>(dout + o_nm);
    d.n_created = reinterpret_cast<int32_t *>(dout + o_nc), d.match12 = reinterpret_cast<int32_t *>(dout + o_match);
    d.status = reinterpret_cast<int32_t *>(dout + o_status), d.x3d = reinterpret_cast<float *>(dout + o_x);
    if ((rc = orbgpu_create_new_map_points_device(&d, device_id, ws.stream)) != ORBGPU_OK)
        return rc;
    ws.download(ws.h_out.data(), NP_OUT, out.off);  // the one download
    if ((rc = ws.finish()) != ORBGPU_OK)
        return rc;
    const uint8_t *ho = ws.h_out.data();
    memcpy(p->n_done, ho + o_done, 4);
    if (nn > 0)
        memcpy(p->n_matches, ho + o_nm, 4 * (size_t)nn), memcpy(p->n_created, ho + o_nc, 4 * (size_t)nn);
    if (cells > 0)
        memcpy(p->match12, ho + o_match, 4 * cells), memcpy(p->status, ho + o_status, 4 * cells), memcpy(p->x3d, ho + o_x, 12 * cells);
    return ORBGPU_OK;
}

// Host boundary of the projection matchers: host views -> std::vector<Query> in the reference's float conventions
// (DESIGN.md "float conventions": `volatile` float products, double reciprocals, cv::norm in double).  Host-only, no HIP:
// compiles with plain g++ -std=c++17 -ffp-contract=off (tests/proj_boundary_test.cpp).  No error state either: a
// builder returns a status plus the offending row and level (Built), and the entry point words the message.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "orbgpu.h"

namespace orbgpu {

struct Query {  // one row of the matcher: a projected map point
    float x, y, r;      // window centre and half-size (r already multiplied by the level scale)
    float ur;           // predicted right coordinate (mTrackProjXR / u - mbf*invz)
    int min_level, max_level;
    int active;         // 0: the reference `continue`s before the candidate loop
    int blocking;       // a claim by this row hides the key point from later rows
    int check_ur;       // apply the mvuRight gate (ORBmatcher.cc:91-96 / 1407-1413); off for :1472-1599
    int gate;           // 1: Fuse's reprojection-error gates (ORBmatcher.cc:908-933) against F.inv_sigma2
};

struct Pinhole {  // bf: mbf, 0 where the flavour predicts no right coordinate
    float fx, fy, cx, cy, bf;
};
struct Built {  // what a builder returns: ORBGPU_OK, or ORBGPU_ELEVEL (H5) with the row whose level is outside [0, nlevels)
    int status = ORBGPU_OK, row = -1, level = 0;
};

// ---- cv::Mat algebra ---------------------------------------------------------------------------------------
// One row of cv::gemm's small-matrix path (CV_32F): float products summed left to right.
inline float row_dot(const float *row, const float *p)
{
    volatile float a = row[0] * p[0];
    volatile float b = row[1] * p[1];
    volatile float c = row[2] * p[2];
    volatile float t0 = a + b;
    volatile float t1 = t0 + c;
    return t1;
}
// cv::Mat 3x3 * 3x1 + 3x1: the products as above, then one add of the C term.  T: rows of [R | t], 4 floats apart.
inline void rt_apply(const float *T, const float *p, float *out)
{
    for (int i = 0; i < 3; i++)
        out[i] = row_dot(T + 4 * i, p) + T[4 * i + 3];
}
// -R^T t (Frame.cc:266): the general gemm path, double accumulators
inline void minus_rt_t(const float *T, float *out)
{
    for (int i = 0; i < 3; i++) {
        double s = 0;
        for (int k = 0; k < 3; k++)
            s += (double)T[4 * k + i] * (double)T[4 * k + 3];
        out[i] = (float)(s * -1.0);
    }
}
// Scw = [s R | s t] decomposed as ORBmatcher.cc:299-303 / :985-989 do: scw from the first row (Mat::dot: double), then
// cv::Mat / scalar (float multiply by (float)(1/scw)), Ow = -Rcw^T tcw.  T: 16 floats, rows of [Rcw | tcw], last row 0.
// False for a degenerate Scw (scw == 0).
inline bool sim3_to_rt(const float *Scw, float *T, float *Ow)
{
    const double d = (double)Scw[0] * Scw[0] + (double)Scw[1] * Scw[1] + (double)Scw[2] * Scw[2];
    const float scw = (float)sqrt(d);
    if (!(scw > 0.f))
        return false;
    const float alpha = (float)(1.0 / (double)scw);
    std::fill(T, T + 16, 0.f);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) {
            volatile float v = Scw[4 * r + c] * alpha;
            T[4 * r + c] = v;
        }
    minus_rt_t(T, Ow);
    return true;
}
// SearchBySim3's pair of transforms (ORBmatcher.cc:1121-1123): sR12 = s12*R12, sR21 = (1.0/s12)*R12.t() (double
// scalar), t21 = -sR21*t12.  3x3 row-major.
inline void sim3_pair(float s12, const float *R12, const float *t12, float *sR12, float *sR21, float *t21)
{
    const double inv_s = 1.0 / (double)s12;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            volatile float a = s12 * R12[3 * r + c];
            sR12[3 * r + c] = a;
            sR21[3 * r + c] = (float)((double)R12[3 * c + r] * inv_s);
        }
    for (int r = 0; r < 3; r++)
        t21[r] = -row_dot(sR21 + 3 * r, t12);
}
// :1339-1349 forward / backward motion of SearchByProjection(CurrentFrame, LastFrame): tlc = Rlw*twc + tlw against the
// baseline, never for a monocular frame
inline void last_motion(const float *cur_Tcw, const float *last_Tcw, float mb, int mono, bool &forward, bool &backward)
{
    float twc[3], tlc[3];
    minus_rt_t(cur_Tcw, twc);
    rt_apply(last_Tcw, twc, tlc);
    forward = tlc[2] > mb && !mono;
    backward = -tlc[2] > mb && !mono;
}

// ---- the two pin-hole conventions ----------------------------------------------------------------------------
enum class Recip {
    Float,      // 1/z in float (:331 sim3 projection, :859 Fuse)
    ViaDouble,  // 1.0/z: double division rounded to float (:1019, :1166, :1246, :1365, :1502)
};
inline float reciprocal(float z, Recip how) { return how == Recip::Float ? 1 / z : (float)(1.0 / (double)z); }

// `fx*xc*invzc + cx` (ORBmatcher.cc:1370-1371 last frame, :1504-1505 key frame): scaled by the focal length first, then
// by the reciprocal.
inline void project_focal_first(const Pinhole &K, const float pc[3], float invz, float &u, float &v)
{
    volatile float ux = K.fx * pc[0];
    volatile float ux2 = ux * invz;
    u = ux2 + K.cx;
    volatile float vy = K.fy * pc[1];
    volatile float vy2 = vy * invz;
    v = vy2 + K.cy;
}
// `x = p(0)*invz; u = fx*x + cx` (ORBmatcher.cc:332-336 sim3 projection, :860-864 Fuse, :1020-1024 Fuse-Sim3,
// :1167-1171 / :1247-1251 SearchBySim3): normalised by the reciprocal first, then scaled.
inline void project_normalised_first(const Pinhole &K, const float pc[3], float invz, float &u, float &v)
{
    volatile float x = pc[0] * invz, y = pc[1] * invz;
    volatile float ux = K.fx * x, vy = K.fy * y;
    u = ux + K.cx, v = vy + K.cy;
}
// Frame-side bounds of :1373-1376 / :1507-1510: both ends inclusive (and a NaN passes, as there)
inline bool in_frame_bounds(const orbgpu_frame_view *f, float u, float v)
{
    return !(u < f->min_x || u > f->max_x) && !(v < f->min_y || v > f->max_y);
}
// KeyFrame::IsInImage (KeyFrame.cc:648-651): the upper end is exclusive
inline bool is_in_image(const orbgpu_frame_view *kf, float u, float v)
{
    return u >= kf->min_x && u < kf->max_x && v >= kf->min_y && v < kf->max_y;
}

// cv::norm(v): accumulates in double
inline float norm3(const float *v) { return (float)sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]); }
// PO = Pw - Ow and its norm, the distance of a point from the camera centre
inline float cam_distance(const float *Pw, const float *Ow, float *PO)
{
    PO[0] = Pw[0] - Ow[0], PO[1] = Pw[1] - Ow[1], PO[2] = Pw[2] - Ow[2];
    return norm3(PO);
}
// MapPoint::PredictScale (MapPoint.cc:385-394); the caller checks the range.  The float is tested before it is converted:
// a level that no int holds (NaN or infinite, from a non-finite position or max_dist, or dist == 0) comes back as INT_MIN
// or INT_MAX, out of every range, and not as whatever the conversion happens to give.
inline int predict_level(float max_dist, float dist, float log_sf)
{
    const float level = ceilf(logf(max_dist / dist) / log_sf);
    if (!(level > -2147483648.f))
        return INT_MIN;
    return level < 2147483648.f ? (int)level : INT_MAX;
}

// ---- claim tables --------------------------------------------------------------------------------------------
// kp_to_mp -> claim_init where only rows with Observations()>0 hold their key point (:87-89, :1403-1405): -2 and a held
// row give -1, anything else INT_MAX.  Returns the index of the first entry outside [-2, m), -1 if there is none.
inline int claim_init_observed(const int32_t *kp_to_mp, int n, int m, const uint8_t *obs_pos, std::vector<int> &init)
{
    init.assign((size_t)std::max(n, 1), 0);
    for (int j = 0; j < n; j++) {
        const int v = kp_to_mp[j];
        if (!(v >= -2 && v < m))
            return j;
        const bool held = v == -2 || (v >= 0 && (obs_pos ? obs_pos[v] != 0 : true));
        init[j] = held ? -1 : INT_MAX;
    }
    return -1;
}
// ... where any association hides the key point (:373, :1540-1541): -1 gives INT_MAX, anything else -1.  With `found`
// (spAlreadyFound, :306-307: the rows of [0, m) some key point holds) the entries are checked and reported as above.
inline int claim_init_free(const int32_t *kp_to_mp, int n, std::vector<int> &init, int m = 0,
                           std::vector<uint8_t> *found = nullptr)
{
    init.assign((size_t)std::max(n, 1), 0);
    if (found)
        found->assign((size_t)std::max(m, 1), 0);
    for (int j = 0; j < n; j++) {
        const int v = kp_to_mp[j];
        if (found && !(v >= -2 && v < m))
            return j;
        if (found && v >= 0)
            (*found)[v] = 1;
        init[j] = v == -1 ? INT_MAX : -1;
    }
    return -1;
}

// ---- query builders, one per flavour -------------------------------------------------------------------------
inline void accept(Query &Q, float u, float v, float r, int min_level, int max_level)
{
    Q.x = u, Q.y = v, Q.r = r;
    Q.min_level = min_level, Q.max_level = max_level;
    Q.active = 1;
}

// ORBmatcher::SearchByProjection(Frame&, vpMapPoints, th), :45-129: rows the caller's Frame::isInFrustum left in view.
// Levels [lvl-1, lvl], mvuRight gate on, blocking from Observations()>0.
inline Built queries_local(const orbgpu_frame_view *f, const orbgpu_mappoint_view *mp, float th, std::vector<Query> &q)
{
    const bool bFactor = th != 1.0;
    q.assign((size_t)mp->m, Query{});
    for (int i = 0; i < mp->m; i++) {
        Query &Q = q[i];
        Q.blocking = mp->obs_pos ? (mp->obs_pos[i] != 0) : 1;
        if (!mp->in_view[i] || (mp->bad && mp->bad[i]))
            continue;
        const int lvl = mp->level[i];
        if (lvl < 0 || lvl >= f->nlevels)
            return {ORBGPU_ELEVEL, i, lvl};
        float r = (double)mp->view_cos[i] > 0.998 ? 2.5f : 4.0f;  // RadiusByViewingCos, :131-137
        if (bFactor)
            r *= th;
        accept(Q, mp->proj_x[i], mp->proj_y[i], r * f->scale_factors[lvl], lvl - 1, lvl);
        Q.ur = mp->proj_xr[i], Q.check_ur = 1;
    }
    return {};
}

// SearchByProjection(CurrentFrame, LastFrame, th, bMono), :1328-1470.  Focal-first projection with the double
// reciprocal, `invzc < 0` behind the camera (:1367), inclusive bounds; levels [oct-1, oct+1], [oct, -1] (= no upper end)
// moving forward or [0, oct] moving backward; mvuRight gate on, blocking from Observations()>0.
inline Built queries_last(const orbgpu_frame_view *cur, const float *cur_Tcw, const Pinhole &K, float mb,
                          const orbgpu_lastframe_view *last, float th, int mono, std::vector<Query> &q)
{
    bool bForward, bBackward;
    last_motion(cur_Tcw, last->Tcw, mb, mono, bForward, bBackward);
    q.assign((size_t)last->n, Query{});
    for (int i = 0; i < last->n; i++) {
        Query &Q = q[i];
        Q.blocking = last->obs_pos ? (last->obs_pos[i] != 0) : 1;
        if (!last->has_mp[i] || (last->outlier && last->outlier[i]))
            continue;
        float xc3[3], u, v;  // :1360-1376 projection (per-point float arithmetic of the boundary, O(n))
        rt_apply(cur_Tcw, last->world_pos + 3 * (size_t)i, xc3);
        const float invzc = reciprocal(xc3[2], Recip::ViaDouble);
        if (invzc < 0)
            continue;
        project_focal_first(K, xc3, invzc, u, v);
        if (!in_frame_bounds(cur, u, v))
            continue;
        const int oct = last->kp_octave[i];
        if (oct < 0 || oct >= cur->nlevels)
            return {ORBGPU_ELEVEL, i, oct};
        const int lo = bForward ? oct : bBackward ? 0 : oct - 1, hi = bForward ? -1 : bBackward ? oct : oct + 1;  // :1385-1390
        accept(Q, u, v, th * cur->scale_factors[oct], lo, hi);
        volatile float bz = K.bf * invzc;
        Q.ur = u - bz, Q.check_ur = 1;
    }
    return {};
}

// SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist), :1472-1599 (relocalisation).  Focal-first
// projection with the double reciprocal and NO behind-camera test (the reference has none, :1502-1510), inclusive
// bounds, the caller's pre-scaled Get{Min,Max}DistanceInvariance; levels [lvl-1, lvl+1], no mvuRight gate, every row
// blocks (:1540-1541: any association hides the key point).
inline Built queries_keyframe(const orbgpu_frame_view *cur, const float *cur_Tcw, const Pinhole &K, float log_sf,
                              const orbgpu_keyframe_view *kf, float th, std::vector<Query> &q)
{
    float Ow[3];
    minus_rt_t(cur_Tcw, Ow);  // :1478
    q.assign((size_t)kf->n, Query{});
    for (int i = 0; i < kf->n; i++) {
        Query &Q = q[i];
        Q.blocking = 1;
        if (!kf->has_mp[i] || (kf->bad && kf->bad[i]) || (kf->already_found && kf->already_found[i]))
            continue;
        const float *Pw = kf->world_pos + 3 * (size_t)i;
        float xc3[3], u, v, PO[3];
        rt_apply(cur_Tcw, Pw, xc3);
        project_focal_first(K, xc3, reciprocal(xc3[2], Recip::ViaDouble), u, v);
        if (!in_frame_bounds(cur, u, v))
            continue;
        const float dist3D = cam_distance(Pw, Ow, PO);
        if (dist3D < kf->min_dist_inv[i] || dist3D > kf->max_dist_inv[i])
            continue;
        const int lvl = predict_level(kf->max_dist[i], dist3D, log_sf);
        if (lvl < 0 || lvl >= cur->nlevels)
            return {ORBGPU_ELEVEL, i, lvl};
        accept(Q, u, v, th * cur->scale_factors[lvl], lvl - 1, lvl + 1);
    }
    return {};
}

// Common tail of the per-point tests of the loop-closing / fusing matchers, up to the row itself: normalised-first
// projection, image bounds (KeyFrame::IsInImage), scale-invariance range, viewing angle below 60 degrees (:354; Pn ==
// nullptr: not tested), PredictScale, then levels [lvl-1, lvl] and, with `gate`, Fuse's ur = u - bf*invz (:870).
// Forced into its two callers: left to itself clang calls it, at 3 ns a row (3000 rows of Fuse: 74 instead of 67 us).
__attribute__((always_inline)) inline Built point_gate(Query &Q, int i, const float pc[3], float invz, const Pinhole &K, const orbgpu_frame_view *kf,
                        float dist3D, const float *PO, const float *Pn, float min_dist, float max_dist, float log_sf, float th,
                        int gate)
{
    float u, v;
    project_normalised_first(K, pc, invz, u, v);
    if (!is_in_image(kf, u, v))
        return {};
    const float maxDistance = 1.2f * max_dist, minDistance = 0.8f * min_dist;
    if (dist3D < minDistance || dist3D > maxDistance)
        return {};
    if (Pn) {
        const double dot = (double)PO[0] * Pn[0] + (double)PO[1] * Pn[1] + (double)PO[2] * Pn[2];
        if (dot < 0.5 * dist3D)
            return {};
    }
    const int lvl = predict_level(max_dist, dist3D, log_sf);
    if (lvl < 0 || lvl >= kf->nlevels)
        return {ORBGPU_ELEVEL, i, lvl};
    accept(Q, u, v, th * kf->scale_factors[lvl], lvl - 1, lvl);
    if (gate) {
        volatile float bz = K.bf * invz;
        Q.ur = u - bz, Q.gate = 1;
    }
    return {};
}

// World points against a key frame under Tcw = [R | t] with centre Ow: SearchByProjection(pKF, Scw, vpPoints, vpMatched,
// th) (:290-403: Recip::Float, blocking 1, gate 0, skip = spAlreadyFound), Fuse(pKF, vpMapPoints, th) (:825-975:
// Recip::Float, blocking 0, gate 1) and Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:977-1100: Recip::ViaDouble,
// blocking 0, gate 0).  `pc[2] < 0.0f` behind the camera, the normal is tested.
inline Built queries_points(const orbgpu_frame_view *kf, const float *T, const float *Ow, const Pinhole &K, float log_sf,
                            const orbgpu_points_view *pts, const uint8_t *skip, float th, Recip recip, int blocking, int gate,
                            std::vector<Query> &q)
{
    q.assign((size_t)pts->m, Query{});
    for (int i = 0; i < pts->m; i++) {
        q[i].blocking = blocking;
        if ((pts->bad && pts->bad[i]) || (skip && skip[i]))
            continue;
        const float *Pw = pts->world_pos + 3 * (size_t)i;
        float pc[3], PO[3];
        rt_apply(T, Pw, pc);
        if (pc[2] < 0.0f)
            continue;
        const float dist3D = cam_distance(Pw, Ow, PO);
        const Built b = point_gate(q[i], i, pc, reciprocal(pc[2], recip), K, kf, dist3D, PO, pts->normal + 3 * (size_t)i,
                                   pts->min_dist[i], pts->max_dist[i], log_sf, th, gate);
        if (b.status != ORBGPU_OK)
            return b;
    }
    return {};
}

// One direction of SearchBySim3 (:1143-1227 / :1229-1307): the points of key frame A into key frame B through
// sR*(Taw*p) + t.  `(double)z < 0.0` behind the camera, double reciprocal, the distance is the norm of the camera-B
// point itself, no normal, blocking 0, gate 0.
inline Built queries_sim3_direction(const orbgpu_frame_view *kfB, const float *Taw, const float sR[9], const float t[3],
                                    const Pinhole &K, float log_sfB, const orbgpu_points_view *ptsA, const uint8_t *skipA,
                                    float th, std::vector<Query> &q)
{
    q.assign((size_t)ptsA->m, Query{});
    for (int i = 0; i < ptsA->m; i++) {
        if ((ptsA->bad && ptsA->bad[i]) || (skipA && skipA[i]))
            continue;
        float pa[3], pb[3];
        rt_apply(Taw, ptsA->world_pos + 3 * (size_t)i, pa);
        for (int r = 0; r < 3; r++)
            pb[r] = row_dot(sR + 3 * r, pa) + t[r];
        if ((double)pb[2] < 0.0)
            continue;
        const Built b = point_gate(q[i], i, pb, reciprocal(pb[2], Recip::ViaDouble), K, kfB, norm3(pb), nullptr, nullptr,
                                   ptsA->min_dist[i], ptsA->max_dist[i], log_sfB, th, 0);
        if (b.status != ORBGPU_OK)
            return b;
    }
    return {};
}

// SearchForInitialization (:405-518): rows = the level-0 key points of F1 (:419-422), each a window of `window_size`
// around its previous match on its own level (GetFeaturesInArea(.., level1, level1)).  row_of: the F1 index of a row.
inline void queries_initialization(const orbgpu_frame_view *f1, const float *prev_matched, int window_size,
                                   std::vector<int> &row_of, std::vector<Query> &q, std::vector<uint8_t> &rdesc)
{
    for (int i1 = 0; i1 < f1->n; i1++) {
        const int level1 = f1->kp_octave[i1];
        if (level1 > 0)
            continue;
        row_of.push_back(i1);
        q.push_back(Query{});
        accept(q.back(), prev_matched[2 * i1], prev_matched[2 * i1 + 1], (float)window_size, level1, level1);
        rdesc.insert(rdesc.end(), f1->desc + (size_t)i1 * 32, f1->desc + (size_t)i1 * 32 + 32);
    }
}

} // namespace orbgpu

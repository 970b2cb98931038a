/*
 * orbgpu.h -- C ABI of liborbgpu.so: MI355X (gfx950) implementation of the per-frame hot path
 * of carry4985/ORB_SLAM2_MAP (ORBextractor + ORBmatcher + PointCloudMapping arithmetic).
 *
 * The reference has no FFI/plugin layer: its boundary is three C++ classes compiled into
 * libORB_SLAM2.so (reference CMakeLists.txt:63-84).  Every entry point below names the
 * reference interface (file:line, relative to the reference tree) it replaces; the C++ shims
 * that re-create those classes on top of this ABI are in orb_slam2_map_amd/shim/ and the binding a
 * maintainer adds is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++/torch types; never throws across the ABI;
 *  - every function returns an orbgpu_status (0 = OK, <0 = error); orbgpu_last_error_string()
 *    gives a thread-local message;
 *  - "host" entry points take host pointers and synchronise before returning;
 *    "*_device" entry points take device pointers plus a hipStream_t (passed as void*), enqueue
 *    work on that stream and return without synchronising;
 *  - a handle must not be used from two threads at once; distinct handles are independent.
 *  - there is NO CPU fallback: without a HIP device every compute entry point fails with
 *    ORBGPU_EHIP.
 */
#ifndef ORBGPU_H
#define ORBGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBGPU_ABI_VERSION 1
#define ORBGPU_MAX_LEVELS 16

typedef enum {
    ORBGPU_OK = 0,
    ORBGPU_EINVAL = -1,    /* bad argument */
    ORBGPU_ENOMEM = -2,    /* host or device allocation failed */
    ORBGPU_EHIP = -3,      /* HIP runtime error / no device */
    ORBGPU_ECAPACITY = -4, /* caller-provided output capacity too small */
    ORBGPU_ELEVEL = -5     /* predicted pyramid level outside [0,nlevels) (UB in the reference:
                              ORBmatcher.cc:69 indexes mvScaleFactors with an unclamped
                              MapPoint::PredictScale, MapPoint.cc:385-394) */
} orbgpu_status;

const char *orbgpu_last_error_string(void);
int orbgpu_abi_version(void);
/* Number of visible HIP devices (0 if none); never fails. */
int orbgpu_device_count(void);
/* Measurement aid: achieved HBM GB/s (bytes read + bytes written per second) of a plain 16-byte-per-lane
 * device-to-device copy kernel over `bytes` (>= 1 MiB; use a size well past the 256 MB Infinity Cache) --
 * the practical roofline bench.py reports next to the nominal 8 TB/s. */
int orbgpu_measure_copy_bandwidth(size_t bytes, int32_t reps, int32_t device_id, float *gbs);

/* ======================================================================================
 * ORBextractor  (reference include/ORBextractor.h:46-110, src/ORBextractor.cc)
 * ====================================================================================== */

/* cv::KeyPoint layout (28 B): pt.x, pt.y, size, angle, response, octave, class_id. */
typedef struct {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} orbgpu_keypoint;

/* ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
 * (ORBextractor.h:51-52; values come from the YAML keys read at Tracking.cc:193-197). */
typedef struct {
    int32_t nfeatures;
    float scale_factor;
    int32_t nlevels;
    int32_t ini_th_fast;
    int32_t min_th_fast;
    int32_t device_id; /* HIP device ordinal */
    int32_t max_batch; /* frames per batched launch the handle pre-sizes for (>=1) */
} orbgpu_extractor_params;

typedef struct orbgpu_extractor orbgpu_extractor;

/* replaces `new ORBextractor(...)` (Tracking.cc:201-213) */
int orbgpu_extractor_create(const orbgpu_extractor_params *params, orbgpu_extractor **out);
int orbgpu_extractor_destroy(orbgpu_extractor *h);

/* computeOrbDescriptor's  a = (float)cos(angle), b = (float)sin(angle)  (ORBextractor.cc:112-113).  With
 * `using namespace std;` in force (:66-67) the calls resolve to std::cos(float) / std::sin(float) = libm's cosf / sinf,
 * which are not correctly rounded: their last bit is a property of the host's libm.  Process-wide, read by
 * orbgpu_extractor_create:
 *   ORBGPU_TRIG_HOST_LIBM (default)  the values THIS host's cosf / sinf return, bit for bit: the device evaluates a fixed
 *       IEEE-double sequence and corrects it from a table of the arguments where the host differs, built by scanning
 *       every float of [0, 2 pi] once per process at the first extractor creation (about 15 core-seconds, spread over
 *       the CPUs the process may use; 18 MB on the device);
 *   ORBGPU_TRIG_ROUNDED_DOUBLE       (float)cos((double)angle): the correctly rounded value, no table, no start-up scan
 *       (differs from glibc 2.35's cosf / sinf in 1.3e-3 of the arguments, from a descriptor bit far more rarely:
 *       DESIGN.md section 2). */
enum { ORBGPU_TRIG_HOST_LIBM = 0, ORBGPU_TRIG_ROUNDED_DOUBLE = 1 };
int orbgpu_set_trig_mode(int32_t mode);
int orbgpu_get_trig_mode(void);
/* entries of the exception table (-1: not built yet) and the time its scan took */
int orbgpu_trig_table_info(int64_t *entries, double *build_ms);
/* Test aid, needs no device: cos / sin of x as ORBGPU_TRIG_HOST_LIBM delivers them (builds the table if necessary);
 * *from_table = 1 if the table corrected the base value. */
int orbgpu_trig_host_eval(float x, float *c, float *s, int32_t *from_table);
/* Test aid: the DEVICE's values (the function the descriptor stage calls) for n host floats, current mode. */
int orbgpu_trig_eval(const float *x, int32_t n, float *c, float *s, int32_t device_id);

/* GetLevels / GetScaleFactor / GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares /
 * GetInverseScaleSigmaSquares (ORBextractor.h:63-83). Arrays receive nlevels floats. */
int orbgpu_extractor_get_levels(const orbgpu_extractor *h, int32_t *nlevels);
int orbgpu_extractor_get_scale_factor(const orbgpu_extractor *h, float *scale_factor);
int orbgpu_extractor_get_scale_factors(const orbgpu_extractor *h, float *out);
int orbgpu_extractor_get_inv_scale_factors(const orbgpu_extractor *h, float *out);
int orbgpu_extractor_get_sigma2(const orbgpu_extractor *h, float *out);
int orbgpu_extractor_get_inv_sigma2(const orbgpu_extractor *h, float *out);
/* mnFeaturesPerLevel (ORBextractor.h:102) */
int orbgpu_extractor_get_quotas(const orbgpu_extractor *h, int32_t *out);
/* Upper bound of keypoints one frame can produce (SURVEY.md E3': a level may return up to
 * max(4*nIni, quota+2) keypoints) -- the `cap` every extract call needs. */
int orbgpu_extractor_max_keypoints(const orbgpu_extractor *h, int32_t width, int32_t height, int32_t *cap);

/* ORBextractor::operator()(image, mask, keypoints, descriptors) (ORBextractor.h:59-61,
 * ORBextractor.cc:1043-1105; called from Frame::ExtractORB, Frame.cc:247-253).  The mask is
 * ignored by the reference (ORBextractor.h:58) and has no parameter here.
 * gray: 8-bit single channel, `stride` bytes per row.  kps[cap], desc[cap*32].  An empty image
 * (width or height 0) returns OK with *n_out = 0 (ORBextractor.cc:1046). */
int orbgpu_extract(orbgpu_extractor *h, const uint8_t *gray, int32_t width, int32_t height, size_t stride,
                   orbgpu_keypoint *kps, uint8_t *desc, int32_t cap, int32_t *n_out);

/* `batch` independent frames of one size in one launch sequence (frames x levels as grid
 * dimensions).  gray: batch images, `frame_stride` bytes apart.  Outputs are [batch][cap]. */
int orbgpu_extract_batch(orbgpu_extractor *h, const uint8_t *gray, int32_t batch, int32_t width, int32_t height,
                         size_t stride, size_t frame_stride, orbgpu_keypoint *kps, uint8_t *desc, int32_t cap,
                         int32_t *n_out);

/* Device-resident variant: all pointers are device pointers, nothing is copied or synchronised;
 * d_n_out[batch] receives the per-frame keypoint counts.  If a frame would exceed `cap` its
 * count is reported as -1 - (required count) and its outputs are unspecified. */
int orbgpu_extract_batch_device(orbgpu_extractor *h, const uint8_t *d_gray, int32_t batch, int32_t width,
                                int32_t height, size_t stride, size_t frame_stride, orbgpu_keypoint *d_kps,
                                uint8_t *d_desc, int32_t cap, int32_t *d_n_out, void *hip_stream);

/* mvImagePyramid[level] (public member, ORBextractor.h:85; read by Frame::ComputeStereoMatches,
 * Frame.cc:471,561,578).  Copies level `level` of frame `frame` of the LAST call (without the
 * 19 px border) to host memory, dst_stride bytes per row.
 * Level 0: when the input rows of the last call were 4-byte aligned (base pointer, stride, frame stride) and the width a
 * multiple of 8, no stage needs ComputePyramid's padded copy of the image (ORBextractor.cc:1125-1129: FAST, the
 * orientation disc and the resize only read the image interior, the blur reflects its own rim) and the library does not
 * make one ("direct mode"); this getter then makes it on demand from the image of the last call.  For the host entry
 * points that is the handle's own staging copy; after orbgpu_extract_batch_device it is the CALLER's device buffer, which
 * must still hold the images when level 0 is asked for (the RGB-D path never asks: only stereo matching reads it).
 * A call that fails before it launches (ENOMEM, an unsupported size) may leave no last call to read: EINVAL. */
int orbgpu_extractor_get_pyramid_level(orbgpu_extractor *h, int32_t frame, int32_t level, uint8_t *dst,
                                       size_t dst_stride, int32_t *width, int32_t *height);

/* Stage introspection of the last call, for stage-by-stage parity tests (not part of the
 * drop-in surface).  what: */
enum {
    ORBGPU_DBG_PYRAMID_PADDED = 0, /* u8, (h+38) rows of `pitch` bytes; *n = bytes, aux = pitch   */
    ORBGPU_DBG_BLURRED_PADDED = 1, /* same geometry, only the w x h interior is defined           */
    ORBGPU_DBG_CANDIDATES = 2,     /* int32 triples (x,y,response), vToDistributeKeys order       */
    ORBGPU_DBG_SELECTED = 3,       /* int32 triples (x,y,response), DistributeOctTree list order  */
    ORBGPU_DBG_GRAPH_COUNTS = 4    /* int32 pair: graphs recorded, graph replays of the host entry
                                      points since creation; *n = 2 (frame / level ignored)        */
};
int orbgpu_extractor_debug_read(orbgpu_extractor *h, int32_t what, int32_t frame, int32_t level, void *dst,
                                size_t dst_bytes, size_t *n, int32_t *aux);

/* Per-stage device time (ms), measured with HIP events recorded on the call's own stream at the stage
 * boundaries of every call made while profiling is enabled (up to 256 calls per window; enabling and
 * disabling keeps the window, so a caller may profile a sample of its calls).
 * Names are returned by orbgpu_extractor_stage_name(i); count by orbgpu_extractor_stage_count(). */
/* The host entry points (orbgpu_extract, orbgpu_extract_batch) replay their launch sequence as a hipGraph from the
 * third call of a configuration on: *state = 1 graph in use, 0 not recorded yet, -1 recording failed (plain launches).
 * The graph is built node by node (hipGraphAddKernelNode), never by stream capture: nothing process-wide is touched. */
int orbgpu_extractor_graph_state(const orbgpu_extractor *h, int32_t *state);
/* How DistributeOctTree (ORBextractor.cc:539-763) is launched for a call of `batch` frames at the configured image size:
 * keys of a level the workgroup keeps in LDS (0 = the batch variant, all keys in memory), threads per workgroup and the
 * dynamic LDS bytes.  Test aid: the environment hook ORBGPU_DEBUG_QT_KEYS (read by orbgpu_extractor_create) shrinks
 * the LDS share so that the mixed LDS / memory path runs; this getter tells a test that it really did. */
int orbgpu_extractor_debug_quadtree_config(const orbgpu_extractor *h, int32_t batch, int32_t *lds_keys, int32_t *threads,
                                           int32_t *lds_bytes);
int orbgpu_extractor_set_profiling(orbgpu_extractor *h, int32_t enable);
/* Throughput option for resident batches (no counterpart in the reference): the 7x7 blur (ORBextractor.cc:1085-1086;
 * HBM-bound) runs on a stream owned by the handle next to the FAST pass (VALU-bound) and the quadtree, forked after the
 * pyramid and joined in front of the descriptor stage.  Results are unchanged; with profiling on, the blur's stage time
 * is the one measured on its own stream (it overlaps the "fast" / "quadtree" stage times). */
int orbgpu_extractor_set_concurrent_blur(orbgpu_extractor *h, int32_t enable);
/* Option of the FAST stage (no counterpart in the reference, results unchanged): before the corner-score network of a
 * pixel pair runs, an exact bound from the four compass pixels of the ring (cv::FAST's own high-speed test, A4: an arc of
 * 9 contains two adjacent compass pixels) is evaluated; where it clears every pixel pair of a wavefront's row segment, the
 * network is skipped.  Pays on images with flat regions (walls, table tops); costs ~20 % of the FAST stage on images that
 * are textured everywhere, like the synthetic benchmark stream -- hence off by default.  Environment variable
 * ORBGPU_FAST_EARLY_OUT=1 turns it on for handles created afterwards. */
int orbgpu_extractor_set_fast_early_out(orbgpu_extractor *h, int32_t enable);

/* Pipelining aid for callers that run other work next to an extraction (bench.py starts the matcher of the previous
 * batch there): `hip_event` (a hipEvent_t, or NULL to clear) is recorded on the launch stream of every later
 * orbgpu_extract_batch_device call right after stage `stage` (index as in orbgpu_extractor_stage_name). */
int orbgpu_extractor_set_stage_signal(orbgpu_extractor *h, int32_t stage, void *hip_event);
int orbgpu_extractor_stage_count(void);
const char *orbgpu_extractor_stage_name(int32_t i);
/* Synchronises the recorded events, returns the AVERAGE ms per stage over the calls profiled since
 * the last stage_times, and starts a new window. */
int orbgpu_extractor_stage_times(orbgpu_extractor *h, float *ms_out);

/* Throughput mode of ORBextractor::operator() over a resident batch (no counterpart in the reference, which extracts one
 * frame per call, Frame.cc:247-253): the batch is cut into `parts` sub-batches, each with an extractor handle and a HIP
 * stream of its own; part k starts when part k-1 (part 0: the last part of the previous call) has passed its pyramid
 * stage, so the HBM-bound, VALU-bound and latency-bound stages of neighbouring parts overlap -- across calls too, because
 * a call only ENQUEUES.  params->max_batch = frames per call.  Results are bit-identical to orbgpu_extract_batch_device.
 *   wait_event (hipEvent_t or NULL): every part waits for it first (inputs uploaded, output buffers free);
 *   done_event (hipEvent_t or NULL): recorded when every part of THIS call has finished;
 *   orbgpu_pipeline_wait: makes `hip_stream` wait for everything enqueued so far (plain stream-ordered use);
 *   orbgpu_pipeline_part: the handle of part k, for set_profiling / stage_times / set_stage_signal. */
typedef struct orbgpu_pipeline orbgpu_pipeline;
int orbgpu_pipeline_create(const orbgpu_extractor_params *params, int32_t parts, orbgpu_pipeline **out);
int orbgpu_pipeline_destroy(orbgpu_pipeline *pl);
int orbgpu_pipeline_parts(const orbgpu_pipeline *pl, int32_t *parts);
int orbgpu_pipeline_part(orbgpu_pipeline *pl, int32_t k, orbgpu_extractor **part);
int orbgpu_pipeline_extract_device(orbgpu_pipeline *pl, const uint8_t *d_gray, int32_t batch, int32_t width,
                                   int32_t height, size_t stride, size_t frame_stride, orbgpu_keypoint *d_kps,
                                   uint8_t *d_desc, int32_t cap, int32_t *d_n_out, void *wait_event, void *done_event);
int orbgpu_pipeline_wait(orbgpu_pipeline *pl, void *hip_stream);

/* ======================================================================================
 * ORBmatcher  (reference include/ORBmatcher.h:41-106, src/ORBmatcher.cc)
 * ====================================================================================== */

#define ORBGPU_TH_HIGH 100     /* ORBmatcher::TH_HIGH  ORBmatcher.cc:37 */
#define ORBGPU_TH_LOW 50       /* ORBmatcher::TH_LOW   ORBmatcher.cc:38 */
#define ORBGPU_HISTO_LENGTH 30 /* ORBmatcher::HISTO_LENGTH ORBmatcher.cc:39 */
#define ORBGPU_GRID_COLS 64    /* FRAME_GRID_COLS Frame.h:38 */
#define ORBGPU_GRID_ROWS 48    /* FRAME_GRID_ROWS Frame.h:37 */

/* ORBmatcher::DescriptorDistance (ORBmatcher.h:44, ORBmatcher.cc:1647-1663) for n pairs:
 * out[i] = Hamming(a[i], b[i]) over 256 bits. Host pointers. */
int orbgpu_hamming256(const uint8_t *a, const uint8_t *b, int32_t n, int32_t *out, int32_t device_id);

/* MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:242-307), batched over `groups` map points: group g owns the
 * descriptors [offsets[g], offsets[g+1]) of desc (the rows of its non-bad observing key frames, in the iteration
 * order of mObservations).  best_idx[g] = index INSIDE the group of the descriptor with the least median Hamming
 * distance to the group (median = sorted row [(size_t)(0.5*(N-1))], first minimum), -1 for an empty group (the
 * reference leaves mDescriptor untouched).  Host pointers; at most 2048 descriptors per group. */
int orbgpu_distinctive_descriptors(int32_t groups, const int32_t *offsets, const uint8_t *desc, int32_t *best_idx,
                                   int32_t device_id);

/* Brute-force 256-bit Hamming matcher with the acceptance rule, greedy claim order and rotation
 * consistency of ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) (ORBmatcher.cc:159-288) when all
 * features share one vocabulary node (the reference has no other brute-force matcher).
 * For each valid A row in index order: best/second-best over B rows not yet claimed; accept iff
 * best <= th_low and (float)best < nnratio*(float)second; claim.  match_b[j] = A index or -1.
 * valid_a may be NULL.  angle_* are cv::KeyPoint::angle (degrees), used iff check_orientation.
 * Angles are not validated, here or in any other matcher of this header.  The rotation bin of a pair is
 * roundf(rot / 30) with rot = angle_a - angle_b, plus 360 when negative (ORBmatcher.cc:238-243; 30 folds onto 0).  A
 * pair whose rounded quotient is not in [0, 30] -- a difference of 915 degrees or more or of -375 or less, a NaN or an
 * infinite angle -- has no bin (the reference asserts there): it casts no vote in the histogram and, with
 * check_orientation, is removed like a pair outside the three maxima.  The status stays ORBGPU_OK. */
int orbgpu_match_bf(const uint8_t *desc_a, const float *angle_a, const uint8_t *valid_a, int32_t na,
                    const uint8_t *desc_b, const float *angle_b, int32_t nb, int32_t th_low, float nnratio,
                    int32_t check_orientation, int32_t *match_b, int32_t *nmatches, int32_t device_id);

/* Batched device-resident variant: `pairs` independent (A,B) problems.  Row p of every array is
 * `cap` elements apart; na[p]/nb[p] are device int32 counts (e.g. d_n_out of the extractor).
 * d_desc: [pairs][cap][32]; d_angle_stride_bytes lets the angle be read in place from an
 * orbgpu_keypoint array (stride 28) or from a packed float array (stride 4).
 * d_match_b: [pairs][cap]; d_nmatches: [pairs].  d_valid_a may be NULL. */
typedef struct orbgpu_matcher orbgpu_matcher;
int orbgpu_matcher_create(int32_t device_id, int32_t max_pairs, int32_t cap, orbgpu_matcher **out);
int orbgpu_matcher_destroy(orbgpu_matcher *m);
int orbgpu_match_bf_batch_device(orbgpu_matcher *m, int32_t pairs, int32_t cap, const uint8_t *d_desc_a,
                                 const void *d_angle_a, const uint8_t *d_valid_a, const int32_t *d_na,
                                 const uint8_t *d_desc_b, const void *d_angle_b, const int32_t *d_nb,
                                 size_t angle_stride_bytes, int32_t th_low, float nnratio,
                                 int32_t check_orientation, int32_t *d_match_b, int32_t *d_nmatches,
                                 void *hip_stream);
/* Fixpoint sweeps the last batched call needed (diagnostic). */
int orbgpu_matcher_last_sweeps(orbgpu_matcher *m, int32_t *sweeps);
/* Launch shape of the last batched call (diagnostic; host values, no device access): the number of B row ranges
 * with a candidate list of their own (1, 2, 4, 8 or 16), whether the exact full scan read the B descriptors from
 * LDS (1) or from global memory (0), and the workgroup size of the resolve kernel.  ORBGPU_EINVAL before the
 * first call. */
int orbgpu_matcher_last_launch(orbgpu_matcher *m, int32_t *nsplit, int32_t *stage_b, int32_t *resolve_threads);

/* SoA view of the Frame members the projection matchers read (Frame.h:100-190):
 * mvKeysUn (pt, octave, angle), mvuRight, mDescriptors, image bounds, grid metrics, the
 * extractor's scale factors, and mGrid flattened to CSR in (ix*ROWS+iy) order with items in
 * insertion order (Frame::AssignFeaturesToGrid, Frame.cc:230-245). Host pointers. */
typedef struct {
    int32_t n;
    const float *kp_x, *kp_y;
    const int32_t *kp_octave;
    const float *kp_angle;
    const float *u_right;
    const uint8_t *desc;
    float min_x, max_x, min_y, max_y;
    float grid_inv_w, grid_inv_h;
    const float *scale_factors;
    int32_t nlevels;
    const int32_t *cell_start; /* COLS*ROWS+1 */
    const int32_t *cell_items; /* cell_start[COLS*ROWS] entries */
} orbgpu_frame_view;

/* Frame::AssignFeaturesToGrid + PosInGrid (Frame.cc:230-245, 382-392): fills the CSR arrays. */
int orbgpu_assign_features_to_grid(int32_t n, const float *kp_x, const float *kp_y, float min_x, float min_y,
                                   float grid_inv_w, float grid_inv_h, int32_t *cell_start, int32_t *cell_items);

/* Camera of a Frame: mK (Frame.h:107-111), mDistCoef (k1 k2 p1 p2 k3; k3 = 0 for the 4-entry form, Tracking.cc:96-106),
 * mbf, and the undistorted image bounds mnMinX..mnMaxY (Frame::ComputeImageBounds, Frame.cc:436-468). */
typedef struct orbgpu_camera {
    float fx, fy, cx, cy;
    float dist[5];
    float mbf;
    float min_x, max_x, min_y, max_y;
} orbgpu_camera;

/* cv::undistortPoints(src, dst, mK, mDistCoef, Mat(), mK) as Frame::UndistortKeyPoints (Frame.cc:404-434) and
 * Frame::ComputeImageBounds (:436-468) call it: n interleaved (x, y) pairs, host pointers, evaluated on the device
 * in double exactly as OpenCV 2.4 cvUndistortPoints does (5 iterations).  For the four image corners this gives
 * the bounds to put into orbgpu_camera. */
int orbgpu_undistort_points(int32_t n, const float *xy_in, const orbgpu_camera *cam, float *xy_out, int32_t device_id);

/* Device-resident Frame glue for a batch of frames straight out of orbgpu_extract_batch_device:
 * Frame::UndistortKeyPoints (Frame.cc:404-434; d_kps_un [batch][cap] receives mvKeysUn, required when
 * cam->dist[0] != 0, optional otherwise), Frame::ComputeStereoFromRGBD (Frame.cc:641-662: depth looked up at the
 * distorted key point, mvuRight = kpUn.x - mbf/d, mvDepth = d where d > 0, else -1) and
 * Frame::AssignFeaturesToGrid (Frame.cc:230-245, on mvKeysUn) as CSR per frame (cell_start[batch][COLS*ROWS+1],
 * cell_items[batch][cap], items in insertion order).  d_depth may be NULL (no stereo outputs); depth strides are
 * in floats.  All pointers except cam are device pointers; nothing is synchronised.
 * Preconditions and conventions, the first one shared with the reference:
 *  - with d_depth, the distorted position (x, y) of every counted key point must be finite and inside the depth image,
 *    0 <= (int)x < width and 0 <= (int)y < height: the lookup depth[(int)y][(int)x] is not checked, as imDepth.at is not;
 *  - d_n[f] is clamped to [0, cap]; only the first n rows of frame f are read;
 *  - rows at and beyond n of d_kps_un, d_u_right and d_kp_depth are not written, nor is d_cell_items beyond
 *    cell_start[f][COLS*ROWS]; d_cell_start is written whole (all zero for n = 0);
 *  - the mvKeysUn copy and the grid follow the reference's gate: only dist[0] != 0 undistorts, whatever dist[1..4] hold
 *    (Frame.cc:406), while orbgpu_undistort_points applies all five coefficients;
 *  - a key point whose rounded grid coordinate is NaN, +-inf or beyond the grid has no cell (the reference converts to
 *    int first, which C leaves undefined for these); orbgpu_assign_features_to_grid does the same. */
int orbgpu_frame_glue_batch_device(int32_t device_id, int32_t batch, int32_t cap, const orbgpu_keypoint *d_kps,
                                   const int32_t *d_n, const float *d_depth, size_t depth_stride,
                                   size_t depth_frame_stride, const orbgpu_camera *cam, orbgpu_keypoint *d_kps_un,
                                   float *d_u_right, float *d_kp_depth, int32_t *d_cell_start,
                                   int32_t *d_cell_items, void *hip_stream);

/* ---- Stereo frames: Frame::ComputeStereoMatches (Frame.cc:466-638) -------------------------------------------------
 * The stereo Frame constructor (Frame.cc:59-117) extracts both rectified images and matches every left key point along
 * its row: descriptor search over the right key points listed in the row (octave within +-1, uR in
 * [uL - maxD, uL + 3]: minD = -3 in this tree, Frame.cc:494), then eleven 11x11 SAD windows on the UNBLURRED pyramid
 * level of the left key point, a parabola fit, and a cut of the matches whose SAD is >= 2.1 x the median.  Outputs are
 * mvuRight / mvDepth (-1 where there is no match), bit-exact to the reference's float arithmetic.
 * Conventions where the reference is undefined:
 *  - mb is read before the constructor assigns it (Frame.cc:90 against :114): minZ = mb = mbf / fx, maxD = mbf / minZ;
 *  - no match at all: nothing is cut (the reference reads element 0 of an empty vector);
 *  - a key point whose row, octave or SAD windows leave the image / level plane gets no match (never a read outside it);
 *    a right key point with an octave outside [0, nlevels) is never a candidate.  Key points the extractor made always
 *    lie inside.
 * The pyramids are those of the handles' LAST extraction call (orbgpu_extractor_get_pyramid_level): `left` and `right`
 * must have the same levels, scale factor and image size, and may be the same handle.  Level 0 of a call that ran in
 * direct mode is read from that call's own images -- after orbgpu_extract_batch_device the CALLER's device buffer, which
 * must still hold them when the stereo kernels run; nothing is materialised and nothing runs on the handles' streams.
 * The next extraction call on either handle replaces what this reads: order it after the stereo call. */

/* Pair p matches frame left_frame0 + p of the left handle's last call with frame right_frame0 + p of the right handle's
 * (one orbgpu_extract_batch_device of 2B frames, B left images then B right images, on one handle is the cheapest way to
 * get B pairs).  Key points / descriptors / counts are device arrays [batch][cap] as orbgpu_extract_batch_device writes
 * them (a negative count reads as 0); d_u_right / d_depth [batch][cap] receive mvuRight / mvDepth (-1 where no match,
 * entries past the count included); d_n_stereo [batch] (optional) the matches kept.  Scratch lives on the left handle,
 * so two calls with the same left handle must be ordered.  EINVAL: null handles or arrays, batch or cap < 0, handles
 * that differ in levels, scale factor or image size, a handle without a last call, a frame range outside it.  Enqueued
 * on hip_stream, not synchronised. */
int orbgpu_stereo_matches_batch_device(const orbgpu_extractor *left, int32_t left_frame0, const orbgpu_extractor *right,
                                       int32_t right_frame0, int32_t batch, int32_t cap, const orbgpu_keypoint *d_kps_l,
                                       const int32_t *d_n_l, const uint8_t *d_desc_l, const orbgpu_keypoint *d_kps_r,
                                       const int32_t *d_n_r, const uint8_t *d_desc_r, float mbf, float fx,
                                       float *d_u_right, float *d_depth, int32_t *d_n_stereo, void *hip_stream);
/* Frame::ComputeStereoMatches for one pair, host arrays: frame 0 of each handle's last call (orbgpu_extract), mvKeys /
 * mDescriptors (n_l), mvKeysRight / mDescriptorsRight (n_r); u_right / depth receive n_l floats.  Synchronises. */
int orbgpu_compute_stereo_matches(const orbgpu_extractor *left, const orbgpu_extractor *right, int32_t n_l,
                                  const orbgpu_keypoint *kps_l, const uint8_t *desc_l, int32_t n_r,
                                  const orbgpu_keypoint *kps_r, const uint8_t *desc_r, float mbf, float fx,
                                  float *u_right, float *depth);

/* ---- Device-resident Tracking::SearchLocalPoints (Tracking.cc:1447-1497) ----------------------------------
 * = Frame::isInFrustum (Frame.cc:269-325) + MapPoint::PredictScale (MapPoint.cc:385-394) over a MapPoint table
 * kept in HBM, followed by ORBmatcher::SearchByProjection(F, vpMapPoints, th) (ORBmatcher.cc:45-137), for a
 * frame that never left the device (orbgpu_extract_batch_device -> orbgpu_frame_glue_batch_device).  Only the
 * pose crosses PCIe. */
typedef struct orbgpu_device_frame_view {
    int32_t cap;                  /* capacity of the per-frame arrays (upper bound of *n) */
    const int32_t *n;             /* device: N */
    const orbgpu_keypoint *kps;   /* device [cap]: mvKeysUn */
    const uint8_t *desc;          /* device [cap][32]: mDescriptors */
    const float *u_right;         /* device [cap]: mvuRight */
    const int32_t *cell_start;    /* device [COLS*ROWS+1]: mGrid as CSR */
    const int32_t *cell_items;    /* device [cap] */
    int32_t nlevels;
    const float *scale_factors;   /* HOST [nlevels]: mvScaleFactors */
    float min_x, max_x, min_y, max_y; /* mnMinX .. mnMaxY */
} orbgpu_device_frame_view;

typedef struct orbgpu_device_mappoint_table { /* all device pointers, row i = mvpLocalMapPoints[i] */
    int32_t m;
    const float *world_pos;   /* [m][3] GetWorldPos() */
    const float *normal;      /* [m][3] GetNormal() */
    const float *min_dist;    /* [m] mfMinDistance (the 0.8 / 1.2 invariance factors are applied inside) */
    const float *max_dist;    /* [m] mfMaxDistance */
    const uint8_t *desc;      /* [m][32] GetDescriptor() */
    const uint8_t *skip;      /* [m] or NULL: isBad() || mnLastFrameSeen == F.mnId (Tracking.cc:1474-1477) */
    const uint8_t *obs_pos;   /* [m] or NULL (= all 1): Observations() > 0 (ORBmatcher.cc:87-89) */
} orbgpu_device_mappoint_table;

typedef struct orbgpu_track_scratch { /* optional device outputs: the MapPoint::mTrack* members isInFrustum fills */
    uint8_t *in_view;  /* [m] mbTrackInView (written for every row; drives IncreaseVisible, Tracking.cc:1481) */
    float *proj_x, *proj_y, *proj_xr, *view_cos; /* [m] written where in_view */
    int32_t *level;    /* [m] mnTrackScaleLevel */
} orbgpu_track_scratch;

/* d_kp_to_mp [cap] in/out (device): -1 free, -2 held by a point outside the table, >= 0 row of the table.
 * d_counts [2] (device): [0] = return value of SearchByProjection, [1] = map points whose predicted level fell
 * outside [0, nlevels) (the reference reads mvScaleFactors out of range there; they are left unmatched).
 * Tcw: HOST, 4x4 row-major float (mTcw).  Asynchronous on hip_stream; calls issued by one host thread share a
 * workspace and must be ordered on one stream. */
int orbgpu_search_local_points_device(const orbgpu_device_frame_view *f, const orbgpu_device_mappoint_table *mp,
                                      const float *Tcw, float fx, float fy, float cx, float cy, float mbf,
                                      float log_scale_factor, float cos_limit, float th, float nnratio,
                                      int32_t *d_kp_to_mp, int32_t *d_counts, const orbgpu_track_scratch *d_track,
                                      int32_t device_id, void *hip_stream);

/* The same for n independent problems (one per sequence: frames shard by sequence) in four launches:
 * the claim fixpoint of one frame is one workgroup by construction, so many sequences are what fills the device.
 * Every problem has its own frame, map-point table, pose and outputs; cos_limit / th / nnratio are shared. */
typedef struct orbgpu_local_points_problem {
    const orbgpu_device_frame_view *frame;
    const orbgpu_device_mappoint_table *table;
    const float *Tcw;                     /* HOST 4x4 row-major float */
    float fx, fy, cx, cy, mbf, log_scale_factor;
    int32_t *d_kp_to_mp;                  /* device [frame->cap] in/out */
    int32_t *d_counts;                    /* device [2] */
    const orbgpu_track_scratch *d_track;  /* optional */
} orbgpu_local_points_problem;
int orbgpu_search_local_points_batch_device(int32_t n, const orbgpu_local_points_problem *problems, float cos_limit,
                                            float th, float nnratio, int32_t device_id, void *hip_stream);

/* Device-resident ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono)
 * (ORBmatcher.cc:1328-1470; Tracking::TrackWithMotionModel, Tracking.cc:1169/1175): the per-frame matcher of
 * RGB-D tracking.  cur = the frame that never left the device; last = the previous frame's key points (octave and
 * angle are read from the records) plus, per key point, what Tracking keeps of its map point.  Both poses are HOST
 * 4x4 row-major floats; nothing else crosses PCIe.  The projection (:1360-1376), the level window by direction of
 * motion (:1339-1349, :1385-1390), the greedy claims, TH_HIGH and the rotation histogram are the reference's.
 * d_kp_to_mp [cur->cap] in/out: -1 free, -2 held by a map point outside `last`, >= 0 row of `last`.
 * d_counts [2]: [0] = nmatches, [1] = rows whose octave fell outside [0, nlevels) (left unmatched). */
typedef struct orbgpu_device_lastframe_view { /* device pointers unless noted */
    int32_t cap;                 /* rows (upper bound of *n) */
    const int32_t *n;            /* LastFrame.N */
    const orbgpu_keypoint *kps;  /* [cap] LastFrame.mvKeys (octave, angle) */
    const uint8_t *has_mp;       /* [cap] LastFrame.mvpMapPoints[i] != NULL */
    const uint8_t *outlier;      /* [cap] or NULL: LastFrame.mvbOutlier[i] */
    const uint8_t *obs_pos;      /* [cap] or NULL (= all 1): Observations() > 0 */
    const float *world_pos;      /* [cap][3] GetWorldPos() */
    const uint8_t *desc;         /* [cap][32] GetDescriptor() of the map point */
} orbgpu_device_lastframe_view;
int orbgpu_search_by_projection_last_device(const orbgpu_device_frame_view *cur, const float *cur_Tcw,
                                            const orbgpu_device_lastframe_view *last, const float *last_Tcw, float fx,
                                            float fy, float cx, float cy, float mbf, float mb, float th, int32_t mono,
                                            int32_t check_orientation, int32_t *d_kp_to_mp, int32_t *d_counts,
                                            int32_t device_id, void *hip_stream);

/* ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints,
 * vector<MapPoint*>& vpMatched, int th) (ORBmatcher.cc:290-403; loop closing, LoopClosing.cc:397).
 * kf: the key frame as a frame view (mvKeysUn, mDescriptors, mGrid; u_right is not read).  Scw: HOST 4x4 row-major
 * float Sim3 [sR | st].  pts: the candidate points.  kp_to_mp [kf->n] in/out = vpMatched: -1 NULL, -2 a map point
 * outside pts, >= 0 row of pts (those rows form spAlreadyFound and are skipped); every accepted point (best
 * distance <= TH_LOW among the free key points of levels [l-1, l] in the window) is written there.
 * ORBGPU_ELEVEL if a predicted level falls outside [0, nlevels). */
typedef struct orbgpu_points_view {
    int32_t m;
    const uint8_t *bad;      /* [m] isBad(), may be NULL */
    const float *world_pos;  /* [m][3] GetWorldPos() */
    const float *normal;     /* [m][3] GetNormal() */
    const float *min_dist;   /* [m] mfMinDistance */
    const float *max_dist;   /* [m] mfMaxDistance */
    const uint8_t *desc;     /* [m][32] GetDescriptor() */
} orbgpu_points_view;
int orbgpu_search_by_projection_sim3(const orbgpu_frame_view *kf, const float *Scw, float fx, float fy, float cx,
                                     float cy, float log_scale_factor, const orbgpu_points_view *pts, int32_t th,
                                     int32_t *kp_to_mp, int32_t *nmatches, int32_t device_id);

/* Convergence diagnostics of the calling thread's most recent projection match (orbgpu_search_by_projection*,
 * orbgpu_search_local_points_device): claim sweeps run and rows that had to be re-walked with the claim filter.
 * Synchronises the device. */
int orbgpu_projection_last_sweeps(int32_t *sweeps, int32_t *rewalked_rows);

/* MapPoint tracking scratch filled by Frame::isInFrustum (MapPoint.h:91-96, Frame.cc:317-322)
 * plus the flags and descriptor the matcher reads per point (ORBmatcher.cc:53-63, 77, 88). */
typedef struct {
    int32_t m;
    const uint8_t *in_view;  /* mbTrackInView */
    const uint8_t *bad;      /* isBad(); may be NULL */
    const uint8_t *obs_pos;  /* Observations()>0; may be NULL (= all true) */
    const int32_t *level;    /* mnTrackScaleLevel */
    const float *view_cos;   /* mTrackViewCos */
    const float *proj_x, *proj_y, *proj_xr;
    const uint8_t *desc;     /* GetDescriptor(), m x 32 */
} orbgpu_mappoint_view;

/* ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (ORBmatcher.h:48,
 * ORBmatcher.cc:45-129; called from Tracking::SearchLocalPoints, Tracking.cc:1495).
 * kp_to_mp[f->n] in/out: in  >=0 existing association (index into mp), -1 free, -2 held by a map
 * point outside `mp` with Observations()>0; out: as F.mvpMapPoints after the call. */
int orbgpu_search_by_projection(const orbgpu_frame_view *f, const orbgpu_mappoint_view *mp, float th,
                                float nnratio, int32_t *kp_to_mp, int32_t *nmatches, int32_t device_id);

/* ---- Device-resident MapPoint table ("Host-side gather cost") -------------------------------------
 * What the projection matchers read of a map point -- GetWorldPos(), GetNormal(), mfMinDistance / mfMaxDistance,
 * GetDescriptor() (a per-point mutex + 32-byte clone in the reference, MapPoint.cc:309-313), isBad(), Observations() > 0
 * (ORBmatcher.cc:53-63, 88) -- kept in HBM, keyed by MapPoint::mnId (MapPoint.h:84).  The table is edited where the
 * reference edits the object (INTEGRATION.md section 2c lists the one-line hooks):
 *   upsert            MapPoint::MapPoint (MapPoint.cc:32-71), SetWorldPos (:73-78), UpdateNormalAndDepth (:330-371),
 *                     ComputeDistinctiveDescriptors (:242-307); RGB-D temporal points (Tracking::UpdateLastFrame) with
 *                     n_obs = 0
 *   set_observations  AddObservation / EraseObservation (:98-149)
 *   set_bad           SetBadFlag (:151-175), Replace (:177-228)
 * Per frame the caller passes ids; id -> row lookup, the gather of the call's local map and the translation of the
 * frame's existing associations run on the device.  A table is used by ONE host thread at a time and the CALLER must
 * serialise: most of the reference's edit sites run WITHOUT Map::mMutexMapUpdate (`new MapPoint` at LocalMapping.cc:434,
 * SetBadFlag in MapPointCulling and at Tracking.cc:806 / 937 / 1416; only Tracking.cc:463, Optimizer.cc:746 / 989 and
 * the LoopClosing sites hold it), while Tracking searches the table concurrently -- an unserialised edit mutates the
 * host-side id hash under a running lookup.  The C++ wrapper MapPointTableT serialises its own calls and the matcher
 * overloads that search it through MapPointTableT::mutex().  Every call returns synchronised.
 * Limits: at most 2^26 ids per call, 2^27 rows per table. */
typedef struct orbgpu_mappoint_table orbgpu_mappoint_table;
int orbgpu_mappoint_table_create(int32_t device_id, int32_t initial_rows, orbgpu_mappoint_table **out);
int orbgpu_mappoint_table_destroy(orbgpu_mappoint_table *t);
/* Rows in use: distinct ids inserted since creation or since the last orbgpu_mappoint_table_retain. */
int orbgpu_mappoint_table_rows(const orbgpu_mappoint_table *t, int32_t *rows);
/* Inserts or updates n points (ids distinct within a call, >= 0; host arrays).  An attribute array may be NULL: known
 * ids keep that attribute, new ids get zeros (n_obs NULL: a new point counts as observed).  world_pos / normal
 * [n][3], desc [n][32], n_obs = Observations(). */
int orbgpu_mappoint_table_upsert(orbgpu_mappoint_table *t, int32_t n, const int64_t *ids, const float *world_pos,
                                 const float *normal, const float *min_dist, const float *max_dist, const uint8_t *desc,
                                 const int32_t *n_obs);
/* Ids the table does not know are ignored; *known (optional) = how many it knew. */
int orbgpu_mappoint_table_set_bad(orbgpu_mappoint_table *t, int32_t n, const int64_t *ids, int32_t *known);
int orbgpu_mappoint_table_set_observations(orbgpu_mappoint_table *t, int32_t n, const int64_t *ids, const int32_t *n_obs,
                                           int32_t *known);
/* Ids of the most recent orbgpu_search_local_points_table / orbgpu_search_by_projection_last_table call that the table
 * had never been told about: list rows (skipped) and key-point associations (treated as held).  Either may be NULL. */
int orbgpu_mappoint_table_last_unknown(const orbgpu_mappoint_table *t, int32_t *list_ids, int32_t *kp_ids);
/* Rows are not recycled by the edits above (a bad point keeps its row, flagged), like the reference, which never frees a
 * MapPoint (Map.cc:76-83, "This only erase the pointer").  This call bounds the table: only the listed ids stay -- typically
 * Map::GetAllMapPoints() plus whatever the current and the last Frame still reference --, rows are renumbered densely in the
 * order given, capacity shrinks to fit; *dropped (optional) = rows released.  Ids dropped here are "unknown" afterwards
 * (skipped as list entries, held as key-point associations: orbgpu_search_local_points_table). */
int orbgpu_mappoint_table_retain(orbgpu_mappoint_table *t, int32_t n, const int64_t *ids, int32_t *dropped);
/* One row back to the host (tests, debugging); any output may be NULL. */
int orbgpu_mappoint_table_read(orbgpu_mappoint_table *t, int64_t id, float *world_pos, float *normal, float *min_dist,
                               float *max_dist, uint8_t *desc, int32_t *has_observations, int32_t *bad);

/* A Frame's matcher-side members (orbgpu_frame_view: mvKeysUn, mvuRight, mDescriptors, mGrid, bounds, scale factors)
 * uploaded ONCE and kept on the device: the same frame is the current frame of SearchByProjection(Cur, Last) and of
 * SearchLocalPoints, and the last frame of the next call.  Uploads return synchronised. */
typedef struct orbgpu_frame orbgpu_frame;
int orbgpu_frame_create(int32_t device_id, orbgpu_frame **out);
int orbgpu_frame_destroy(orbgpu_frame *fr);
int orbgpu_frame_upload(orbgpu_frame *fr, const orbgpu_frame_view *host_view);
/* The device pointers of the uploaded frame (valid until the next upload / destroy), for the *_device entry points. */
int orbgpu_frame_device_view(const orbgpu_frame *fr, orbgpu_device_frame_view *view, int32_t *n);

/* Tracking::SearchLocalPoints (Tracking.cc:1447-1497) / ORBmatcher::SearchByProjection(F, vpMapPoints, th)
 * (ORBmatcher.cc:45-129) over the table.  ids [m] (host) = mvpLocalMapPoints[i]->mnId; skip [m] or NULL = the host-only
 * part of Tracking.cc:1474 (mnLastFrameSeen == F.mnId); isBad() comes from the table.
 *   scratch != NULL: drop-in at the ORBmatcher level -- the caller's Frame::isInFrustum has filled the mTrack* members;
 *                    in_view, level, view_cos, proj_x, proj_y, proj_xr [m] are uploaded (the struct's bad / obs_pos /
 *                    desc fields are ignored: they come from the table).  ORBGPU_ELEVEL as orbgpu_search_by_projection.
 *   scratch == NULL: isInFrustum + PredictScale run on the device from Tcw and the camera (as
 *                    orbgpu_search_local_points_device); track_out (optional, HOST arrays [m], any may be NULL) receives
 *                    mbTrackInView etc. so that the caller can IncreaseVisible() (Tracking.cc:1479-1483).
 * kp_ids [n] or NULL (host): mnId of F.mvpMapPoints[j], -1 = none.  kp_to_mp [n] (host, out): position in ids[] of the
 * point key point j holds after the call, -1 none, -2 a point outside the list that has observations (untouched).
 * An id the table does not know yet is NOT an error: LocalMapping publishes a new point to the key frames
 * (LocalMapping.cc:434-440, AddMapPoint) before ComputeDistinctiveDescriptors / UpdateNormalAndDepth have run, and
 * Tracking::UpdateLocalPoints may list it in that window; the reference tolerates the window, so does this call: an
 * unknown list id is a skipped row, an unknown key-point id counts as "held" (-2).  orbgpu_mappoint_table_last_unknown
 * reports how many of each the most recent search call over the table met.
 * With m == 0 (or an empty frame) nothing is searched; kp_to_mp is still translated through the table. */
int orbgpu_search_local_points_table(const orbgpu_frame *fr, orbgpu_mappoint_table *t, int32_t m, const int64_t *ids,
                                     const uint8_t *skip, const orbgpu_mappoint_view *scratch, const float *Tcw, float fx,
                                     float fy, float cx, float cy, float mbf, float log_scale_factor, float cos_limit,
                                     float th, float nnratio, const int64_t *kp_ids, int32_t *kp_to_mp, int32_t *nmatches,
                                     orbgpu_track_scratch *track_out);

/* ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1328-1470) over the table: both
 * frames are device-resident; last_ids [last n] (host) = mnId of LastFrame.mvpMapPoints[i] or -1, last_outlier [last n]
 * or NULL = LastFrame.mvbOutlier, cur_kp_ids [cur n] or NULL = mnId of CurrentFrame.mvpMapPoints[j] or -1.
 * kp_to_mp [cur n] (host, out): index i of the last-frame key point whose map point key point j now holds, -1, -2.
 * ORBGPU_ELEVEL, with nothing written, if a last-frame key point whose map point projects into the image has an octave
 * outside [0, nlevels), as orbgpu_search_by_projection_last. */
int orbgpu_search_by_projection_last_table(const orbgpu_frame *cur, const float *cur_Tcw, const orbgpu_frame *last,
                                           const float *last_Tcw, orbgpu_mappoint_table *t, const int64_t *last_ids,
                                           const uint8_t *last_outlier, const int64_t *cur_kp_ids, float fx, float fy,
                                           float cx, float cy, float mbf, float mb, float th, int32_t mono,
                                           int32_t check_orientation, int32_t *kp_to_mp, int32_t *nmatches);

/* ---- Optimizer::PoseOptimization (Optimizer.cc:239-451): motion-only bundle adjustment on the device --------------------
 * The step Tracking runs between SearchByProjection(Cur, Last) and SearchLocalPoints and again after it (Tracking.cc:1182,
 * :1059, :1224, :1744-1775): one 6-DoF pose, one unary reprojection edge per key point that holds a map point.  g2o is not
 * part of the reference tree: its behaviour is restated, NOT read ("g2o unpinned"); tests/pose_model.py is the float64
 * restatement every result is compared with.  The definition, all in IEEE double unless a float is named:
 *   set-up (:253-365)   edge iff kp_to_mp[i] >= 0; mono iff mvuRight[i] < 0 (2 residuals, Huber delta (float)sqrt(5.991)),
 *                       else stereo (3 residuals, delta (float)sqrt(7.815)); information = (double)mvInvLevelSigma2[octave];
 *                       pose in as Converter::toSE3Quat (Converter.cc:37-47), out as Converter::toCvMat (:49-71); every
 *                       edge gets mvbOutlier = false; fewer than 3 edges: returns 0, pose untouched
 *   error               (x, y, z) = R Xw + t;  e = obs - (fx x/z + cx, fy y/z + cy[, fx x/z + cx - bf/z]);
 *                       chi2 = invSigma2 e'e; no depth-sign test; non-finite values follow IEEE through the steps below
 *   Jacobian            d e / d (omega, upsilon) of the left update T <- exp(omega, upsilon) T at zero
 *   optimize(10)        Levenberg-Marquardt on the level-0 edges: H = sum J'(rho1 W)J, b = -sum J'(rho1 W)e with Huber rho
 *                       (no second-order term); lambda0 = 1e-5 max diag H, nu = 2; per iteration at most 10 trials of
 *                       (H + lambda I) x = b by Cholesky (not positive definite: the trial fails), T' = exp(x) T,
 *                       rho = (chi - chi') / (x'(lambda x + b) + 1e-3); accepted iff rho > 0 and chi' finite
 *                       (lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3)), nu = 2), else lambda *= nu, nu *= 2; the
 *                       iteration's trials end when rho >= 0; optimize ends after 10 iterations, 10 failed trials in a
 *                       row, rho == 0 or a non-finite lambda
 *   four rounds (:369-442)  each restarts from the input pose, optimises, then classifies EVERY edge: (float)chi2 >
 *                       5.991f (mono) / 7.815f (stereo) -> outlier, left out of the next round; after the third round
 *                       the Huber kernel is dropped; fewer than 10 edges in total: one round only
 * Two conventions where g2o is loose: (1) an edge is classified at the round's final, KEPT pose (g2o uses the error it
 * computed last, which after a rejected final trial belongs to the discarded pose); (2) rho at convergence is rounding
 * noise, so the sums' order can decide a trial: sums over edges run in a fixed order (per-lane partial sums, then a fixed
 * tree; no floating-point atomics) -- the same problem gives the same bits on every run, alone or anywhere in a batch,
 * and agrees with the model to a tolerance, not bit for bit. */
typedef struct orbgpu_pose_result { /* device or host, 8-byte aligned */
    double Tcw_d[16];    /* the optimised pose before Converter::toCvMat, row-major homogeneous */
    float Tcw[16];       /* = (float) of Tcw_d entry by entry: what Frame::SetPose receives */
    int32_t n_initial;   /* nInitialCorrespondences */
    int32_t n_inliers;   /* the return value (0 and pose = input when n_initial < 3) */
    int32_t rounds, iterations, trials; /* diagnostics: rounds run, LM iterations, LM trials over all rounds */
    int32_t n_bad_index; /* edges whose kp_to_mp row or octave was out of range: skipped, reported */
} orbgpu_pose_result;

typedef struct orbgpu_pose_problem {
    const orbgpu_device_frame_view *frame; /* cap, n, kps = mvKeysUn (pt, octave), u_right = mvuRight, nlevels; the
                                              grid, descriptors, scale factors and bounds are not read */
    const int32_t *d_kp_to_mp;             /* device [cap]: >= 0 row of d_world_pos, < 0 no edge */
    const float *d_world_pos;              /* device [rows][3]: table / last-frame world_pos as the matchers take them */
    int32_t rows;
    const float *Tcw;                      /* HOST 4x4 row-major float: mTcw on entry */
    const float *inv_level_sigma2;         /* HOST [frame->nlevels]: mvInvLevelSigma2 */
    float fx, fy, cx, cy, mbf;
    uint8_t *d_outlier;                    /* device [cap]: mvbOutlier, written for edges only */
    orbgpu_pose_result *d_result;          /* device */
} orbgpu_pose_problem;

/* Enqueued on hip_stream, not synchronised; the host arrays (pose, sigma table) are read before the call returns.  Calls
 * of one host thread share a workspace and must be ordered on one stream.  EINVAL: null pointers, n < 0, cap outside
 * [0, 16384], nlevels outside [1, ORBGPU_MAX_LEVELS]; EHIP without a device.  A kp_to_mp row >= rows or an octave outside
 * [0, nlevels) (both undefined reads in the reference) is never read through: the edge is skipped and counted in
 * n_bad_index.  The batch form is ONE launch, one workgroup per problem. */
int orbgpu_pose_optimization_device(const orbgpu_pose_problem *p, int32_t device_id, void *hip_stream);
int orbgpu_pose_optimization_batch_device(int32_t n, const orbgpu_pose_problem *problems, int32_t device_id,
                                          void *hip_stream);
/* Host arrays, synchronises: has_mp [n], world_pos [n][3] per key point; Tcw in/out; outlier [n] in/out (written for
 * edges only); result may be NULL. */
int orbgpu_pose_optimization(const orbgpu_frame_view *f, const uint8_t *has_mp, const float *world_pos, float *Tcw,
                             const float *inv_level_sigma2, float fx, float fy, float cx, float cy, float mbf,
                             uint8_t *outlier, int32_t *n_inliers, orbgpu_pose_result *result, int32_t device_id);
/* Over the MapPoint table and an uploaded frame: kp_ids [n] = mnId of F.mvpMapPoints[j] or -1; ids the table does not
 * know are not edges and are counted through orbgpu_mappoint_table_last_unknown, like the search calls.  Synchronises. */
int orbgpu_pose_optimization_table(const orbgpu_frame *fr, orbgpu_mappoint_table *t, const int64_t *kp_ids, float *Tcw,
                                   const float *inv_level_sigma2, float fx, float fy, float cx, float cy, float mbf,
                                   uint8_t *outlier, int32_t *n_inliers, orbgpu_pose_result *result);
/* Diagnostic: problems of the calling thread's most recent pose optimisation on device_id whose edges did not fit the
 * workgroup's LDS and went through the global-memory spill (ORBGPU_DEBUG_POSE_LDS_EDGES=<k> lowers the limit for tests).
 * Synchronises the device. */
int orbgpu_pose_last_spills(int32_t device_id, int32_t *problems_spilled);

/* ---- Optimizer::LocalBundleAdjustment (Optimizer.cc:453-778): local bundle adjustment on the device -----------------------
 * The most expensive call of LocalMapping (LocalMapping.cc:85): the poses of the local key frames and the positions of the
 * points they see, over every observation of those points; the other key frames that see them are fixed cameras.  g2o is
 * not part of the reference tree: its behaviour (OptimizationAlgorithmLevenberg over BlockSolver_6_3, points marginalised)
 * is restated, NOT read ("g2o unpinned"); tests/lba_model.py is the float64 restatement every result is compared with.
 * The definition, all in IEEE double unless a float is named:
 *   L1 problem             P pose rows: the first n_local are lLocalKeyFrames, free unless fixed[i] (mnId == 0), the rest are
 *                          lFixedCameras; M point rows; E edges (point row, pose row, key point x, y, u_right, octave); an
 *                          edge is mono iff u_right < 0.  Every pose row has its own fx, fy, cx, cy, mbf and its own
 *                          mvInvLevelSigma2 table.  The graph gathering of :455-504 walks pointers and stays with the caller.
 *   L2 set-up (:522-653)   poses in as Converter::toSE3Quat of the float Tcw, points as (double) of the float position;
 *                          information = (double)invSigma2[pose][octave]; Huber delta (float)sqrt(5.991) for mono edges,
 *                          (float)sqrt(7.815) for stereo edges
 *   L3 error, Jacobians    the edge error of orbgpu_pose_optimization (e = obs - projection of R Xw + t);
 *                          J_pose = d e / d (omega, upsilon) of T <- exp(omega, upsilon) T, as there;
 *                          J_point = -(d proj / d Pc) R
 *   L4 system              with s = rho1 invSigma2 (Huber, no second-order term): Hpp[f] += J_pose' s J_pose and
 *                          bp[f] -= J_pose' s e per free pose f (6x6, 6); Hll[p] += J_point' s J_point and
 *                          bl[p] -= J_point' s e per point (3x3, 3); Hpl[e] = J_pose' s J_point per edge to a free pose (6x3);
 *                          an edge to a fixed pose feeds Hll and bl only.  A vertex takes part (is ACTIVE) iff it has a
 *                          level-0 edge; an inactive vertex keeps its estimate.
 *   L5 solve               per active point inv[p] = (Hll[p] + lambda I)^-1 by the 3x3 cofactor inverse (Eigen's; no test of
 *                          the determinant, non-finite values follow IEEE); S = Hpp + lambda I - sum Hpl inv Hpl' over the
 *                          pairs of edges that share a point, g = bp - sum Hpl inv bl, both over 6 slots per free pose (an
 *                          inactive free pose keeps its slot as an identity block with g = 0: x = 0, coupled to nothing);
 *                          S xp = g by dense LL' (a pivot that is not > 0 fails the trial, x = 0);
 *                          xl[p] = inv[p] (bl[p] - sum Hpl' xp); pose <- exp(xp) pose, point <- point + xl.  No free pose:
 *                          xl = inv bl.
 *   L6 optimize(k)         the Levenberg-Marquardt loop of orbgpu_pose_optimization (lambda0, nu, at most 10 trials, the rho
 *                          rule, the termination rules) with: max diag over the diagonals of Hpp and Hll of active
 *                          vertices, lambda added to both, scale = sum x (lambda x + b) + 1e-3 over pose and point increments
 *   L7 two rounds (:659-707)  optimize(5) on all edges with Huber; then every edge is classified at the round's final KEPT
 *                          state (convention (1) of the pose section): chi2 > 5.991 (mono) / 7.815 (stereo), compared in
 *                          double, or depth not > 0 -> level 1; the kernel is dropped on every edge; optimize(10) on the
 *                          level-0 edges CONTINUES from round 1's state with lambda re-initialised (g2o recomputes it at
 *                          iteration 0 of each optimize)
 *   L8 result (:714-743)   the same test on every edge at the final state: erase[e] = 1 is vToErase.  The pMP->isBad()
 *                          skips are the caller's.
 *   L9 stop flag           optional device-readable int32, read by one lane and broadcast: before anything (:655), at the
 *                          start of each iteration and each trial (g2o's forceStopFlag), and between the rounds (:664).
 *                          Non-zero at the first read: nothing is written but the result, stopped = 1.  Later: the running
 *                          optimize ends with the state it has kept, round 2 is skipped (bDoMore), L8 still runs,
 *                          stopped = 1.  A flag raised while the kernel runs ends it at a time that is NOT reproducible; L10
 *                          covers runs whose flag does not change.
 *   L10 determinism        convention (2) of the pose section: every sum over edges, edge pairs or vertices runs in a
 *                          fixed order (per point: its edges one by one in edge order; per pose, per block of S and over
 *                          the workgroup: per-lane partial sums, then a fixed tree; no floating-point atomics) -- the same
 *                          problem gives the same bytes on every run, alone or anywhere in a batch, with S in LDS or in
 *                          global memory, and agrees with the model to a tolerance, not bit for bit.
 *   L11 out of range       an edge whose point row, pose row or octave is out of range is skipped, counted in n_bad_index
 *                          and never read through; its erase byte is not written.
 *   L12 out                per local pose Tcw_d and (float)Tcw_d (Converter::toCvMat), fixed ones included (the quaternion
 *                          round trip of their input); per point the double and the float position; erase; the result. */
#define ORBGPU_LBA_MAX_POSES 1024     /* pose rows (local + fixed cameras) */
#define ORBGPU_LBA_MAX_FREE 96        /* free poses: the reduced system has 6 * 96 rows */
#define ORBGPU_LBA_MAX_POINTS 16384
#define ORBGPU_LBA_MAX_EDGES 262144
#define ORBGPU_LBA_MAX_PAIRS (1 << 24) /* edge pairs that share a point between free poses (terms of S) */

typedef struct orbgpu_local_ba_result { /* device or host, 8-byte aligned */
    double chi2_start[2], chi2_end[2]; /* robust chi2 of the active edges per round: at its start, at its kept end */
    int32_t n_edges;       /* edges taken (E less the out-of-range ones) */
    int32_t n_erased;      /* erase bytes set */
    int32_t iterations[2], trials[2]; /* LM iterations and trials per round */
    int32_t rounds;        /* optimize calls that ran: 0, 1 or 2 */
    int32_t stopped;       /* the stop flag was seen non-zero */
    int32_t n_bad_index;   /* edges skipped for an out-of-range row or octave */
    int32_t reduced_in_lds; /* 1: S lived in LDS, 0: in the global workspace */
} orbgpu_local_ba_result;

typedef struct orbgpu_local_ba_problem {
    int32_t n_poses, n_local, n_points, n_edges, nlevels;
    const float *Tcw;              /* HOST [n_poses][16]: GetPose(), local key frames first */
    const uint8_t *fixed;          /* HOST [n_local]: non-zero = mnId == 0 */
    const float *cam;              /* HOST [n_poses][5]: fx, fy, cx, cy, mbf */
    const float *inv_level_sigma2; /* HOST [n_poses][nlevels] */
    const float *world_pos;        /* HOST [n_points][3] */
    const int32_t *edge_point, *edge_pose, *edge_octave; /* HOST [n_edges] */
    const float *edge_xy;          /* HOST [n_edges][2]: mvKeysUn[...].pt */
    const float *edge_u_right;     /* HOST [n_edges]: mvuRight[...] */
    const int32_t *d_stop;         /* device or NULL */
    double *d_Tcw_d;               /* device [n_local][16] */
    float *d_Tcw;                  /* device [n_local][16] */
    double *d_pos_d;               /* device [n_points][3] */
    float *d_pos;                  /* device [n_points][3] */
    uint8_t *d_erase;              /* device [n_edges]: written for taken edges only */
    orbgpu_local_ba_result *d_result; /* device */
} orbgpu_local_ba_problem;

/* Enqueued on hip_stream, not synchronised; every HOST array is read, and the index structure the fixed summation order
 * needs (edges sorted by point, per-pose edge lists, per-block pair lists of S) is built and uploaded, before the call
 * returns.  Calls of one host thread share a workspace and must be ordered on one stream.  EINVAL: null pointers, negative
 * counts, n_local > n_poses, nlevels outside [1, ORBGPU_MAX_LEVELS], more than ORBGPU_LBA_MAX_* of anything (there is no CPU
 * fallback: the caller keeps its g2o path); EHIP without a device.  The batch form is ONE launch, one workgroup per problem,
 * which runs both rounds and every trial without returning to the host. */
int orbgpu_local_ba_device(const orbgpu_local_ba_problem *p, int32_t device_id, void *hip_stream);
int orbgpu_local_ba_batch_device(int32_t n, const orbgpu_local_ba_problem *problems, int32_t device_id, void *hip_stream);
/* Host arrays, synchronises: the d_* members of p are not read; Tcw_d / Tcw [n_local][16], pos_d / pos [n_points][3] and
 * erase [n_edges] are in/out (a stopped call leaves them alone), any of Tcw_d, pos_d and result may be NULL.  stop: HOST
 * int32 sampled at the call, or NULL. */
int orbgpu_local_ba(const orbgpu_local_ba_problem *p, const int32_t *stop, double *Tcw_d, float *Tcw, double *pos_d,
                    float *pos, uint8_t *erase, orbgpu_local_ba_result *result, int32_t device_id);
/* Diagnostic: problems of the calling thread's most recent local bundle adjustment on device_id whose reduced system did
 * not fit the workgroup's LDS (more than 28 free poses; ORBGPU_DEBUG_LBA_LDS_POSES=<k> lowers the limit for tests) and
 * lived in the global workspace.  Synchronises the device. */
int orbgpu_local_ba_last_spills(int32_t device_id, int32_t *problems_spilled);

/* ---- Optimizer::BundleAdjustment / GlobalBundleAdjustemnt (Optimizer.cc:41-237): full bundle adjustment on the device -------
 * The call of Tracking::CreateInitialMapMonocular (Tracking.cc:963: two key frames, 20 iterations, robust) and of
 * LoopClosing::RunGlobalBundleAdjustment (LoopClosing.cc:647: the whole map, 20 iterations, bRobust = false): every key
 * frame and every point of a map in ONE optimize().  The kernel is orbgpu_local_ba's Levenberg-Marquardt loop with another
 * round structure; tests/ba_model.py is the float64 restatement (g2o unpinned, as above).  Where a rule says no more than
 * "as Lk", nothing differs from orbgpu_local_ba:
 *   B1 problem             P pose rows: vpKFs without the bad ones, free unless fixed[i] (the reference fixes mnId == 0 only;
 *                          any mask is taken, none fixed included: the gauge is then left to lambda); M point rows: vpMP
 *                          without the bad ones; edges as L1.  Skipping the observations of key frames that are bad or whose
 *                          mnId > maxKFid (:109) is the caller's.  Set-up as L2 but for the Huber deltas (B2).
 *   B2 kernel (:85, :131)  robust != 0: Huber delta (float)sqrt(5.99) for mono edges -- 5.99, not L2's 5.991 -- and
 *                          (float)sqrt(7.815) for stereo edges; robust == 0: no kernel on any edge (rho0 = chi2, rho1 = 1),
 *                          the state L7's second round runs in.
 *   B3 optimize            ONE optimize(n_iterations) by L3-L6 over all edges, 0 <= n_iterations <=
 *                          ORBGPU_BA_MAX_ITERATIONS.  No classification, no level-1 edge, no second round, no erase.
 *   B4 activity (:175-179) a point without a taken edge is vbNotIncludedMP: not_included = 1, its outputs are the round trip
 *                          of its input, and it never reaches the inverse; every other point's byte is 0.  A pose row without
 *                          a taken edge keeps its estimate (L4).  n_iterations == 0 writes the round trip of every input with
 *                          iterations = trials = 0 and chi2_start = chi2_end = the robust chi2 of the input.
 *   B5 stop flag           L9 without the read between rounds: before anything, then at each iteration and each trial.
 *                          Non-zero at the first read: nothing is written but the result, stopped = 1.  Later: the outputs
 *                          are the kept state, stopped = 1.
 *   B6 determinism, range  as L10 and L11; an out-of-range edge makes no point included.
 *   B7 out                 as L12 with not_included [M] in place of erase: Tcw_d and (float)Tcw_d for EVERY pose row (fixed
 *                          rows: the quaternion round trip of their input), both positions per point, the result.
 * A whole map is larger than a local one, so the capacities are the call's own (a first choice, like LBA's);
 * the cap on edge pairs is ORBGPU_LBA_MAX_PAIRS. */
#define ORBGPU_BA_MAX_POSES 1024
#define ORBGPU_BA_MAX_FREE 256        /* free poses: the reduced system has 6 * 256 rows */
#define ORBGPU_BA_MAX_POINTS 65536
#define ORBGPU_BA_MAX_EDGES (1 << 20)
#define ORBGPU_BA_MAX_ITERATIONS 100

typedef struct orbgpu_bundle_adjustment_result { /* device or host, 8-byte aligned */
    double chi2_start, chi2_end; /* robust chi2 of the edges at the input and at the kept end */
    int32_t n_edges;        /* edges taken (E less the out-of-range ones) */
    int32_t iterations, trials; /* LM iterations and trials */
    int32_t stopped;        /* the stop flag was seen non-zero */
    int32_t n_bad_index;    /* edges skipped for an out-of-range row or octave */
    int32_t n_not_included; /* points without a taken edge */
    int32_t reduced_in_lds; /* 1: S lived in LDS, 0: in the global workspace */
    int32_t pad_;
} orbgpu_bundle_adjustment_result;

typedef struct orbgpu_bundle_adjustment_problem {
    int32_t n_poses, n_points, n_edges, nlevels;
    int32_t n_iterations;          /* 0 .. ORBGPU_BA_MAX_ITERATIONS */
    int32_t robust;                /* non-zero: Huber kernel on every edge (B2) */
    const float *Tcw;              /* HOST [n_poses][16]: GetPose() */
    const uint8_t *fixed;          /* HOST [n_poses]: non-zero = the row is not optimised (mnId == 0) */
    const float *cam;              /* HOST [n_poses][5]: fx, fy, cx, cy, mbf */
    const float *inv_level_sigma2; /* HOST [n_poses][nlevels] */
    const float *world_pos;        /* HOST [n_points][3] */
    const int32_t *edge_point, *edge_pose, *edge_octave; /* HOST [n_edges] */
    const float *edge_xy;          /* HOST [n_edges][2]: mvKeysUn[...].pt */
    const float *edge_u_right;     /* HOST [n_edges]: mvuRight[...] */
    const int32_t *d_stop;         /* device or NULL */
    double *d_Tcw_d;               /* device [n_poses][16] */
    float *d_Tcw;                  /* device [n_poses][16] */
    double *d_pos_d;               /* device [n_points][3] */
    float *d_pos;                  /* device [n_points][3] */
    uint8_t *d_not_included;       /* device [n_points] */
    orbgpu_bundle_adjustment_result *d_result; /* device */
} orbgpu_bundle_adjustment_problem;

/* Enqueued on hip_stream, not synchronised, under orbgpu_local_ba_device's rules (the index structure is built and uploaded
 * before the call returns; calls of one host thread share a workspace -- not orbgpu_local_ba's -- and must be ordered on one
 * stream).  EINVAL: null pointers, negative counts, n_iterations outside [0, ORBGPU_BA_MAX_ITERATIONS], nlevels outside
 * [1, ORBGPU_MAX_LEVELS], more than ORBGPU_BA_MAX_* of anything or than ORBGPU_LBA_MAX_PAIRS edge pairs (no CPU fallback: the
 * caller keeps its g2o path); EHIP without a device.  The batch form is ONE launch, one workgroup per problem. */
int orbgpu_bundle_adjustment_device(const orbgpu_bundle_adjustment_problem *p, int32_t device_id, void *hip_stream);
int orbgpu_bundle_adjustment_batch_device(int32_t n, const orbgpu_bundle_adjustment_problem *problems, int32_t device_id,
                                          void *hip_stream);
/* Host arrays, synchronises: the d_* members of p are not read; Tcw_d / Tcw [n_poses][16], pos_d / pos [n_points][3] and
 * not_included [n_points] are in/out (a call stopped at once leaves them alone), any of Tcw_d, pos_d and result may be NULL.
 * stop: HOST int32 sampled at the call, or NULL. */
int orbgpu_bundle_adjustment(const orbgpu_bundle_adjustment_problem *p, const int32_t *stop, double *Tcw_d, float *Tcw,
                             double *pos_d, float *pos, uint8_t *not_included, orbgpu_bundle_adjustment_result *result,
                             int32_t device_id);
/* Diagnostic, as orbgpu_local_ba_last_spills, for the calling thread's most recent bundle adjustment on device_id (the same
 * limit of 28 free poses and the same ORBGPU_DEBUG_LBA_LDS_POSES). */
int orbgpu_bundle_adjustment_last_spills(int32_t device_id, int32_t *problems_spilled);

/* ---- Optimizer::OptimizeEssentialGraph (Optimizer.cc:780-1045): the Sim3 pose graph of a loop closure on the device --------
 * The step of LoopClosing::CorrectLoop (LoopClosing.cc:565) that spreads a detected loop's correction over every key frame
 * and every map point: one 7-DoF vertex per key frame, one EdgeSim3 per loop connection, spanning-tree edge, old loop edge
 * and strong covisibility edge, Levenberg-Marquardt over a sparse system of 7 rows per key frame.  g2o is not part of the
 * reference tree: its behaviour (OptimizationAlgorithmLevenberg with setUserLambdaInit(1e-16) over BlockSolver_7_3,
 * VertexSim3Expmap, EdgeSim3, Sim3::log) is restated, NOT read ("g2o unpinned"); tests/eg_model.py is the float64
 * restatement every result is compared with.  All arithmetic is IEEE double, unfused, three-term sums left to right.  Where
 * a rule says "as Ok", "as Lk" or "as Bk", nothing differs from that section:
 *   G1 problem             V vertex rows, each with two Sim3 states of 8 doubles (qx, qy, qz, qw, tx, ty, tz, s): Scw[v] is the
 *                          entry estimate -- CorrectedSim3[pKF] if present, else Sim3(Rcw, tcw, 1) (:818-832) -- and Snc[v] is
 *                          NonCorrectedSim3[pKF] if present, else Scw[v].  States are used as given: nothing is normalised
 *                          on entry or after an update (O4).  fixed[v] is a mask (the reference fixes pLoopKF only; any mask
 *                          is taken).  E edges (i, j, kind): the measurement is Scw[j] * Scw[i]^-1 for kind 0 (the loop
 *                          connections of :852-880) and Snc[j] * Snc[i]^-1 for any other kind (spanning tree, old loop
 *                          edges and covisibility, :883-983).  WHICH edges exist (minFeat, sInsertedEdges, the parent /
 *                          child / loop-edge exclusions, the mnId order) is pointer walking and stays with the caller.
 *                          orbgpu_sim3_from_pose gives Sim3(Rcw, tcw, 1) of a float pose: O9's Smw.
 *   G2 Sim3 algebra        S X = s (R X) + t with R the matrix of the quaternion as it is (O3);
 *                          A * B = (qa qb, sa (Ra tb) + ta, sa sb); S^-1 = (q conjugate, R'((-1 / s) t), 1 / s).
 *   G3 log(S)              g2o's published branches, recalled, not read, in the style of O5: sigma = log(s),
 *                          d = 0.5 (R00 + R11 + R22 - 1), dR = (R21 - R12, R02 - R20, R10 - R01), eps = 1e-5;
 *                          d > 1 - eps: omega = 0.5 dR; otherwise theta = acos(d), omega = (theta / (2 sqrt(1 - d d))) dR.
 *                          C, A and B are O5's four cases with the test theta < eps replaced by d > 1 - eps and s_x by s;
 *                          W = (A Om + B Om Om) + C I; upsilon = W^-1 t by 3x3 LU with partial pivoting (column by column a
 *                          later row is swapped in when its entry is strictly larger in magnitude: row 1 against 0, 2
 *                          against 0, then 2 against 1); the result is (omega, upsilon, sigma).  B of the small-angle,
 *                          |sigma| >= eps case is kept as published, ((sigma^2 / 2 - sigma + 1) s) / sigma^3, although it is
 *                          not the limit of the general case; with fix_scale the scale stays exactly 1,
 *                          sigma is exactly 0 and that case is never entered.
 *   G4 edge (EdgeSim3)     e = log((M * S_i) * S_j^-1), a 7-vector; i is vertex 0, j is vertex 1.  Information is the
 *                          identity, chi2 = e'e summed left to right, no robust kernel.
 *   G5 Jacobians           numeric, as O6: per non-fixed end vertex, per k = 0..6,
 *                          (e(exp(+d 1_k) S) - e(exp(-d 1_k) S)) (1 / (2 d)) with d = 1e-9, through O4 / O5's update; with
 *                          fix_scale x[6] is set to 0 before exp, so column 6 is exactly 0.  A fixed vertex has no Jacobian.
 *   G6 system              H is block-symmetric with 7x7 blocks over the free ACTIVE vertices; a vertex is active when it has
 *                          at least one taken edge.  H_ii += Ji'Ji, H_jj += Jj'Jj, H_ij += Ji'Jj, b_i -= Ji'e, b_j -= Jj'e,
 *                          each product summed over the 7 error rows in turn.  An edge with one fixed end feeds the other
 *                          end's diagonal block and b only; an edge between two fixed vertices feeds chi2 only; parallel
 *                          edges accumulate; an inactive vertex keeps its estimate and has no rows.
 *   G7 solve               (H + lambda I) x = b by LL' over the envelope of H in a reverse Cuthill-McKee order chosen on the
 *                          host (csrc/skyline.h).  A pivot that is not > 0 fails the trial and x = 0.
 *                          Vertex <- exp(x_v) vertex by O4.
 *   G8 optimize            ONE optimize(n_iterations), 0 <= n_iterations <= ORBGPU_EG_MAX_ITERATIONS (the reference passes
 *                          20): the Levenberg-Marquardt loop of orbgpu_pose_optimization (nu, at most 10 trials, the rho rule
 *                          with scale x'(lambda x + b) + 1e-3, the same termination rules) with lambda0 = 1e-16, a constant
 *                          (:794), and no kernel.  n_iterations == 0 writes the inputs through G10 with
 *                          iterations = trials = 0 and chi2_start = chi2_end = the chi2 of the input.
 *   G9 stop flag           as B5.  The reference has none here; the member exists so that a caller can abandon a long solve.
 *   G10 poses out (:992-1010)  per vertex the optimised state Siw_d[8] and Tiw[16]: (float) of R and of t * (1 / s), last
 *                          row 0 0 0 1 (Converter::toCvSE3 of eigR, eigt / s).  Fixed and inactive rows get their input
 *                          state through the same formula.
 *   G11 points out (:1013-1043)  M points with a float world position and a vertex row r[m] (the caller resolves
 *                          mnCorrectedByKF / mnCorrectedReference / GetReferenceKeyFrame):
 *                          out = (float)(Siw_opt[r]^-1 map (Scw[r] map (double)P)) by G2.  A row outside [0, V) leaves the
 *                          point as it came and is counted in n_bad_ref.
 *   G12 determinism, range as L10: every sum over edges is a per-vertex or per-block list in edge order, or per-lane
 *                          partials plus a fixed tree; no floating-point atomics; the same problem gives the same bytes on
 *                          every run, alone or anywhere in a batch.  An edge with i == j or with an end outside [0, V) is
 *                          skipped, counted in n_bad_index and never read through.
 * Capacities: a first choice, like LBA's.  Anything larger is EINVAL; there is no CPU fallback: the caller
 * keeps its g2o path. */
#define ORBGPU_EG_MAX_VERTICES 8192
#define ORBGPU_EG_MAX_EDGES (1 << 18)
#define ORBGPU_EG_MAX_POINTS (1 << 22)
#define ORBGPU_EG_MAX_ENVELOPE (1 << 26) /* doubles of factor storage */
#define ORBGPU_EG_MAX_ITERATIONS 100

typedef struct orbgpu_essential_graph_result { /* device or host, 8-byte aligned */
    double chi2_start, chi2_end; /* chi2 of the taken edges at the input and at the kept end */
    int32_t iterations, trials;  /* LM iterations and trials */
    int32_t stopped;             /* the stop flag was seen non-zero */
    int32_t n_edges;             /* edges taken (E less the skipped ones) */
    int32_t n_bad_index;         /* edges skipped: i == j or an end outside [0, V) */
    int32_t n_free_active;       /* vertices with rows in H */
    int32_t envelope;            /* doubles of the factor's envelope */
    int32_t bandwidth;           /* the longest row of the envelope, diagonal included, in scalars */
    int32_t n_bad_ref;           /* points left alone for a row outside [0, V) (host flavour; G11) */
    int32_t pad_;
} orbgpu_essential_graph_result;

typedef struct orbgpu_essential_graph_problem {
    int32_t n_vertices, n_edges;
    int32_t n_iterations;        /* 0 .. ORBGPU_EG_MAX_ITERATIONS */
    int32_t fix_scale;           /* non-zero: bFixScale (stereo / RGB-D) */
    const double *Scw;           /* HOST [n_vertices][8] */
    const double *Snc;           /* HOST [n_vertices][8] */
    const uint8_t *fixed;        /* HOST [n_vertices] */
    const int32_t *edge_i, *edge_j, *edge_kind; /* HOST [n_edges] */
    const int32_t *d_stop;       /* device or NULL */
    double *d_Siw_d;             /* device [n_vertices][8] */
    float *d_Tiw;                /* device [n_vertices][16] */
    orbgpu_essential_graph_result *d_result; /* device */
} orbgpu_essential_graph_problem;

/* Sim3(Rcw, tcw, 1) of a float pose as 8 doubles: quat_normalize(quat_from_matrix((double)R)), (double)t, 1.  Host only. */
int orbgpu_sim3_from_pose(const float *Tcw, double *out);
/* Enqueued on hip_stream, not synchronised, under orbgpu_bundle_adjustment_device's rules: every HOST array is read, and the
 * index structure (the taken edges, the reverse Cuthill-McKee order, the envelope layout, the per-block edge lists) is built
 * and uploaded, before the call returns; calls of one host thread share a workspace of their own and must be ordered on one
 * stream.  EINVAL: null pointers, negative counts, n_iterations outside [0, ORBGPU_EG_MAX_ITERATIONS], more than
 * ORBGPU_EG_MAX_* of anything, an envelope above ORBGPU_EG_MAX_ENVELOPE (all found before a device is touched); EHIP without
 * a device.  The batch form is ONE launch, one workgroup per problem, which runs every iteration and trial without returning
 * to the host. */
int orbgpu_essential_graph_device(const orbgpu_essential_graph_problem *p, int32_t device_id, void *hip_stream);
int orbgpu_essential_graph_batch_device(int32_t n, const orbgpu_essential_graph_problem *problems, int32_t device_id,
                                        void *hip_stream);
/* G11 alone, over device arrays, enqueued on hip_stream: d_Scw / d_Siw [n_vertices][8] (the entry states and
 * orbgpu_essential_graph_device's d_Siw_d), d_pos_in / d_pos_out [n_points][3] (they may be the same array), d_ref
 * [n_points].  d_n_bad_ref: device int32 the call ADDS its count to, or NULL.  EINVAL: null pointers, negative counts, more
 * than ORBGPU_EG_MAX_VERTICES / ORBGPU_EG_MAX_POINTS. */
int orbgpu_essential_graph_correct_points_device(int32_t n_vertices, const double *d_Scw, const double *d_Siw, int32_t n_points,
                                                 const float *d_pos_in, const int32_t *d_ref, float *d_pos_out,
                                                 int32_t *d_n_bad_ref, int32_t device_id, void *hip_stream);
/* Host arrays, synchronises: the d_* members of p are not read.  Siw_d [n_vertices][8] (may be NULL) and Tiw
 * [n_vertices][16] are in/out (a call stopped at once leaves them alone).  n_points points (world_pos [n_points][3],
 * point_ref [n_points], HOST) are corrected on the same stream after the optimiser into pos_out [n_points][3], which may be
 * world_pos; a call stopped at once corrects nothing.  stop: HOST int32 sampled at the call, or NULL; result may be NULL. */
int orbgpu_essential_graph(const orbgpu_essential_graph_problem *p, const int32_t *stop, double *Siw_d, float *Tiw,
                           int32_t n_points, const float *world_pos, const int32_t *point_ref, float *pos_out,
                           orbgpu_essential_graph_result *result, int32_t device_id);

/* ---- Sim3Solver (Sim3Solver.cc, Horn 1987 + RANSAC): the Sim3 of a loop candidate on the device --------------------------
 * The second of the five steps of LoopClosing::ComputeSim3 (LoopClosing.cc:236-343); its result is the R12 / t12 / s12 that
 * orbgpu_search_by_sim3 takes.  All hypotheses of a candidate are evaluated at once, one wave each; the reference's
 * sequential acceptance rule is replayed over the per-hypothesis counts.  OpenCV is not part of the reference tree: every
 * result is "vs CPU restatement; OpenCV boundary unpinned"; tests/sim3_model.py is the restatement.  Conventions H1-H8
 * (DESIGN.md section 2), float32 with one rounding per operation unless a double is named:
 *   H1 rows (:62-103)     row i1 is kept iff valid[i1] != 0 (the caller's verdict on: has a match, both map points exist
 *                         and are not bad, both indices in their key frame >= 0) and both octaves lie in [0, nlevels); a
 *                         valid row with an octave outside is not kept and counted in n_bad_index (the reference reads
 *                         out of range).  Kept rows are compacted in index order (mvnIndices1): N of them.
 *   H2 points             Xc = Rcw Xw + tcw: products summed left to right, then one add (cv::gemm's small-matrix path);
 *                         own-image projection invz = 1/z, u = fx*(x*invz) + cx, v = fy*(y*invz) + cy
 *   H3 thresholds         mvnMaxError is a vector<size_t>: maxError = (float)trunc(9.210 * (double)sigma2[octave]) -- 9,
 *                         13, 19, ...; a product that is not >= 0 gives 0
 *   H4 iterations (:114-138)  epsilon = (float)minInliers / N; nIterations = 1 if minInliers == N, else
 *                         ceil(log(1 - p) / log(1 - pow((double)epsilon, 3))) in double; NaN or outside int counts as larger
 *                         than maxIterations; max_its = max(1, min(nIterations, maxIterations)); N = 0 gives 1.  Computed
 *                         on the host (orbgpu_sim3_ransac_iterations).
 *   H5 minimal sets       the library draws nothing: triples[h][3] index the compacted list, only the first
 *                         n_use = min(n_hyp, max_its) are used (none if N < minInliers).  orbgpu_shim::Sim3SampleTriples
 *                         replays the reference's draw (:163-177), its quirk included.
 *   H6 Horn (:226-337)    centroid = ((a + b) + c) / 3; M = Pr2 Pr1' and N11..N44 with double sums rounded once to float;
 *                         from here FP64 on the float N: cyclic Jacobi (pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); stop when
 *                         the off-diagonal square sum is <= 1e-32 x the square sum of all entries, at most 16 sweeps;
 *                         theta = (aqq - app) / (2 apq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1),
 *                         s = t c), eigenvector q of the largest eigenvalue (first on ties), ang = atan2(|v|, q0),
 *                         vec = 2 ang v / |v|, Rodrigues; R rounded once to float.  P3 = R Pr2 (small-matrix);
 *                         s = (float)(nom / den) with double sums in row-major order, or 1.0f with fix_scale;
 *                         t = O1 - s (R O2); T12 = [sR t]; sRinv = (1.0f / s) R'; T21 = [sRinv, -(sRinv t)].
 *                         No special cases: a degenerate triple gives NaN and, NaN < x being false, 0 inliers.
 *   H7 inliers (:340-364) X2 through T12 into image 1, X1 through T21 into image 2 (H2); err = (float)((double)dx*dx +
 *                         (double)dy*dy); inlier iff err1 < maxError1 && err2 < maxError2
 *   H8 acceptance (:140-207)  N < minInliers: no_more at once.  Iteration h becomes the best iff count >= best so far, and
 *                         is accepted iff it then has count > minInliers; the scan starts at (start_iteration, best_so_far)
 *                         and ends at the first acceptance or at n_use; no_more iff it ended at max_its unaccepted. */
typedef struct orbgpu_sim3_result { /* device or host */
    int32_t n;              /* N: kept rows */
    int32_t max_its;        /* mRansacMaxIts (H4) */
    int32_t n_bad_index;    /* valid rows with an octave outside [0, nlevels): not kept */
    int32_t n_bad_triple;   /* used hypotheses with an index outside [0, N): never read through, count 0, NaN outputs */
    int32_t accepted;       /* first accepted iteration (0-based index into triples) or -1 */
    int32_t n_inliers;      /* its count, 0 if none */
    int32_t best_inliers;   /* mnBestInliers after the scan */
    int32_t best_iteration; /* the iteration that holds it (GetEstimated*), -1 if none was scanned and none passed in */
    int32_t iterations;     /* mnIterations after the scan */
    int32_t no_more;        /* bNoMore */
} orbgpu_sim3_result;

/* The array pointers are DEVICE pointers for the *_device entry points and HOST pointers for orbgpu_sim3_solve. */
typedef struct orbgpu_sim3_problem {
    int32_t n1;             /* mN1 = vpMatched12.size() */
    int32_t n_hyp;          /* H: rows of triples */
    const uint8_t *valid;   /* [n1] (H1) */
    const float *Xw1;       /* [n1][3] world position of KF1's map point i1 (read for valid rows only) */
    const float *Xw2;       /* [n1][3] world position of vpMatched12[i1] */
    const int32_t *octave1; /* [n1] mvKeysUn[indexKF1].octave */
    const int32_t *octave2; /* [n1] */
    const int32_t *triples; /* [n_hyp][3] (H5) */
    float T1w[16], T2w[16]; /* key-frame poses, 4x4 row-major */
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
    float level_sigma2[ORBGPU_MAX_LEVELS]; /* mvLevelSigma2 */
    int32_t nlevels;
    int32_t fix_scale;
    int32_t min_inliers, max_iterations;
    double probability;
    int32_t start_iteration, best_so_far; /* H8: 0, 0 for a fresh solver */
    /* outputs (orbgpu_sim3_solve ignores them) */
    int32_t *counts;        /* [n_hyp]: inliers of hypothesis h; 0 for h >= n_use */
    float *R;               /* [n_hyp][9]  R12, written for h < n_use */
    float *t;               /* [n_hyp][3] */
    float *s;               /* [n_hyp] */
    float *T12;             /* [n_hyp][16] */
    uint64_t *masks;        /* [n_hyp][(n1 + 63) / 64]: bit i1 % 64 of word i1 / 64 = vbInliers[i1]; written for h < n_use */
    int32_t *indices1;      /* [n1] mvnIndices1 (compacted -> i1), first N written; may be NULL */
    orbgpu_sim3_result *result;
} orbgpu_sim3_problem;

/* H4 on the host; EINVAL for a null pointer or negative n / min_inliers / max_iterations. */
int orbgpu_sim3_ransac_iterations(int32_t n, double probability, int32_t min_inliers, int32_t max_iterations,
                                  int32_t *max_its);
/* Enqueued on hip_stream.  The call waits for the stream TWICE: on entry (the host staging of the thread's previous call
 * must have left for the device; in effect that call's kernels are waited for too) and between the preparation and the
 * hypotheses, to read every N and compute max_its on the host (H4).  The hypotheses and the scan of THIS call are
 * enqueued and not waited for.  Calls of one host thread share a workspace and must be ordered on one stream.  EINVAL: null pointers, n1 outside [0, 65536], n_hyp outside
 * [0, 4096], nlevels outside [1, ORBGPU_MAX_LEVELS], negative min_inliers / max_iterations / start_iteration /
 * best_so_far; nothing is launched then.  EHIP without a device.  The batch form is one launch sequence (three kernels) for
 * all candidates of a ComputeSim3 call. */
int orbgpu_sim3_solve_device(const orbgpu_sim3_problem *p, int32_t device_id, void *hip_stream);
int orbgpu_sim3_solve_batch_device(int32_t n, const orbgpu_sim3_problem *problems, int32_t device_id, void *hip_stream);
/* Host arrays, synchronises.  counts [n_hyp]; R [9], t [3], s [1], T12 [16] of the best iteration (= the accepted one when
 * one is accepted; untouched if best_iteration is -1 or names an iteration of an earlier call); inliers [n1] bytes of the
 * accepted iteration (all 0 if none).  counts, R, t, s, T12 and inliers may be NULL.  A triple index outside [0, N) among
 * the used hypotheses is EINVAL here, before anything is launched.
 * The host flavours run on a stream of the workspace's own and wait for the whole device on entry, so they may follow a
 * device-flavour call of the same thread on any stream. */
int orbgpu_sim3_solve(const orbgpu_sim3_problem *p, int32_t *counts, float *R, float *t, float *s, float *T12,
                      uint8_t *inliers, orbgpu_sim3_result *result, int32_t device_id);
/* As orbgpu_sim3_solve, but every hypothesis comes back: counts [n_hyp], R [n_hyp][9], t [n_hyp][3], s [n_hyp], T12
 * [n_hyp][16], masks [n_hyp][(n1 + 63) / 64] (any may be NULL); hypotheses h >= n_use are zeros.  One upload, one launch
 * sequence: what a caller needs that serves iterate(n, ...) itself (orbgpu_shim::Sim3SolverT). */
int orbgpu_sim3_solve_all(const orbgpu_sim3_problem *p, int32_t *counts, float *R, float *t, float *s, float *T12,
                          uint64_t *masks, orbgpu_sim3_result *result, int32_t device_id);

/* ---- Optimizer::OptimizeSim3 (Optimizer.cc:1079-1236): 7-DoF refinement of a loop candidate's Sim3 on the device -----------
 * The fourth of the five steps of LoopClosing::ComputeSim3 (LoopClosing.cc:326-336), between orbgpu_search_by_sim3 and
 * orbgpu_search_by_projection_sim3: ONE Sim3 vertex, two reprojection edges per correspondence (map point of key frame 2
 * into image 1, map point of key frame 1 into image 2), the map points fixed.  g2o is not part of the reference tree: its
 * behaviour is restated, NOT read ("vs CPU restatement; g2o boundary unpinned"); tests/sim3opt_model.py is the float64
 * restatement every result is compared with.  Conventions O1-O9, all arithmetic IEEE double and
 * unfused unless a float is named; three-term sums run left to right:
 *   O1 rows (:1099-1137)  row i in [0, n1) is a correspondence iff valid[i] != 0 (the caller's verdict on: vpMatches1[i]
 *                         exists, both map points exist and are not bad, i2 >= 0) and both octaves lie in [0, nlevels); a
 *                         valid row with an octave outside is not a correspondence and is counted in n_bad_index (the
 *                         reference reads out of range).  Correspondences keep index order: N = nCorrespondences.
 *   O2 points             X1c = R1w Xw1 + t1w, X2c = R2w Xw2 + t2w in FLOAT exactly as H2 of the Sim3Solver (products summed
 *                         left to right, then one add), then widened to double (Converter::toVector3d)
 *   O3 edges              S X = s (R X) + t with R = the matrix of the state's quaternion; S^-1 = (r', R'((-1/s) t), 1/s);
 *                         cam(X) = ((x / z) fx + cx, (y / z) fy + cy);  e12 = obs1 - cam1(S12 X2c),
 *                         e21 = obs2 - cam2(S12^-1 X1c); obs1 = mvKeysUn1[i].pt, obs2 = mvKeysUn2[i2].pt as floats widened;
 *                         information w = (double)inv_level_sigma2[octave], chi2 = w (e0 e0 + e1 e1); both edges carry a
 *                         Huber kernel with delta = (double)(float)sqrt(th2) (sqrt of the float, :1095) in BOTH stages;
 *                         no depth-sign test; non-finite values follow IEEE through the steps below
 *   O4 state, update      state (q, t, s): q = quat_from_matrix((double)R12) normalised once on entry (w >= 0, unit norm),
 *                         t and s the float inputs widened.  S <- exp(x) S: q = q_x q, t = s_x (R_x t) + t_x, s = s_x s with
 *                         R_x the matrix of q_x; NO renormalisation afterwards (g2o's Sim3 does none).  With fix_scale
 *                         x[6] is set to 0 before exp.
 *   O5 exp(x)             x = (omega, upsilon, sigma), theta = |omega|, Om = [omega]x, s_x = exp(sigma), eps = 1e-5:
 *                           |sigma| <  eps, theta <  eps: C = 1, A = 1/2, B = 1/6, R = (I + Om) + Om Om
 *                           |sigma| <  eps, theta >= eps: C = 1, A = (1 - cos theta) / theta^2, B = (theta - sin theta) / theta^3,
 *                                                         R = (I + (sin theta / theta) Om) + ((1 - cos theta) / theta^2) Om Om
 *                           |sigma| >= eps, theta <  eps: C = (s_x - 1) / sigma, A = ((sigma - 1) s_x + 1) / sigma^2,
 *                                                         B = ((sigma^2 / 2 - sigma + 1) s_x) / sigma^3, R as in the first
 *                           |sigma| >= eps, theta >= eps: C as in the third, R as in the second; a = s_x sin theta,
 *                                                         b = s_x cos theta, c = theta^2 + sigma^2,
 *                                                         A = (a sigma + (1 - b) theta) / (theta c),
 *                                                         B = (C - ((b - 1) sigma + a theta) / c) / theta^2
 *                         t_x = ((A Om + B Om Om) + C I) upsilon, q_x = quat_from_matrix(R) (not normalised).  These are the
 *                         branches as g2o publishes them, recalled, not read.
 *   O6 Jacobian           NUMERIC, as g2o differentiates these two edge types (BaseBinaryEdge::linearizeOplus):
 *                         d e / d x_k = (e(exp(+d 1_k) S) - e(exp(-d 1_k) S)) (1 / (2 d)), d = 1e-9, k = 0..6, through O4's
 *                         update -- with fix_scale column 6 is exactly 0.  The point vertices are fixed.
 *   O7 optimize(k)        the Levenberg-Marquardt loop of orbgpu_pose_optimization with 7 unknowns: H = sum J'(rho1 w)J,
 *                         b = -sum J'(rho1 w)e over the active edges; lambda0 = 1e-5 max diag H, nu = 2 at the first
 *                         iteration of EACH optimize call; per iteration at most 10 trials of (H + lambda I) x = b by LL'
 *                         (a pivot that is not > 0 fails the trial); rho = (chi - chi') / (x'(lambda x + b) + 1e-3);
 *                         acceptance, lambda / nu rule and stop conditions as there; at most k iterations
 *   O8 stages (:1181-1234)  stage 1: optimize(5) over all 2N edges, then every correspondence is classified at the stage's
 *                         final KEPT state: bad iff chi2_12 > (double)th2 || chi2_21 > (double)th2 (compared in double);
 *                         bad correspondences are cleared in inlier[], their edges leave, nBad counts them.
 *                         N - nBad < 10: returns 0, S12 out = the entry state, inlier[] keeps the clearing, stages = 1.
 *                         Stage 2: optimize(nBad > 0 ? 10 : 5) over the remaining edges from the stage-1 state, then the
 *                         remaining correspondences are classified again; n_inliers = those that pass, S12 out = the final
 *                         state.  N = 0: returns 0, nothing is written to inlier[], stages = 0.
 *   O9 outputs            R12_d = the matrix of q, t12_d, s12_d; R12 / t12 / s12 their entry-wise float casts;
 *                         T12 = Converter::toCvMat(Sim3): (float)(s R), (float)t, last row 0 0 0 1;
 *                         Scw (LoopClosing.cc:334-336) = toCvMat(S12 Smw) with Smw = (quat_normalize(quat_from_matrix(
 *                         (double)R2w)), (double)t2w, 1): the Scw argument of orbgpu_search_by_projection_sim3.
 * Sums over edges run in a fixed order (lane l takes correspondences l, l + 256, ..., e12 before e21, then a fixed tree; no
 * floating-point atomics): the same problem gives the same bytes on every run, alone or anywhere in a batch, and agrees
 * with the model to a tolerance, not bit for bit. */
typedef struct orbgpu_sim3_opt_result { /* device or host, 8-byte aligned */
    double R12_d[9], t12_d[3], s12_d; /* the refined Sim3 (O9) */
    float R12[9], t12[3], s12;        /* = (float) of the doubles entry by entry: what orbgpu_search_by_sim3 takes */
    float T12[16];                    /* Converter::toCvMat(g2oS12) */
    float Scw[16];                    /* toCvMat(S12 Smw) */
    int32_t n_correspondences;        /* N (O1) */
    int32_t n_bad;                    /* nBad of stage 1 */
    int32_t n_inliers;                /* the return value */
    int32_t stages;                   /* 0 (N = 0), 1 (fewer than 10 left after stage 1) or 2 */
    int32_t iterations, trials;       /* diagnostics: LM iterations and trials over both stages */
    int32_t n_bad_index;              /* valid rows with an octave outside [0, nlevels): not correspondences */
} orbgpu_sim3_opt_result;

/* The array pointers are DEVICE pointers for the *_device entry points and HOST pointers for orbgpu_sim3_optimize; the
 * row arrays are those of orbgpu_sim3_problem, so a ComputeSim3 caller passes the same buffers on. */
typedef struct orbgpu_sim3_opt_problem {
    int32_t n1;             /* vpMatches1.size() */
    int32_t nlevels;
    const uint8_t *valid;   /* [n1] (O1) */
    const float *Xw1;       /* [n1][3] world position of KF1's map point i (read for valid rows only) */
    const float *Xw2;       /* [n1][3] world position of vpMatches1[i] */
    const int32_t *octave1; /* [n1] mvKeysUn1[i].octave */
    const int32_t *octave2; /* [n1] mvKeysUn2[i2].octave */
    const float *kp1_xy;    /* [n1][2] mvKeysUn1[i].pt */
    const float *kp2_xy;    /* [n1][2] mvKeysUn2[i2].pt, gathered by the caller */
    float T1w[16], T2w[16]; /* key-frame poses, 4x4 row-major */
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
    float inv_level_sigma2[ORBGPU_MAX_LEVELS]; /* mvInvLevelSigma2 */
    float R12[9], t12[3], s12; /* the Sim3 on entry (x1 = s12 R12 x2 + t12) */
    float th2;
    int32_t fix_scale;
    int32_t pad_;
    /* outputs (orbgpu_sim3_optimize ignores them) */
    uint8_t *inlier;        /* [n1]: 1 for a correspondence that stays, 0 for a cleared one; other rows are not written */
    orbgpu_sim3_opt_result *result;
} orbgpu_sim3_opt_problem;

/* Enqueued on hip_stream, not synchronised, no host round trip; the problem structs are read before the call returns.
 * Calls of one host thread share a workspace and must be ordered on one stream.  EINVAL without touching the device: null
 * pointers, n < 0, n1 outside [0, 65536], nlevels outside [1, ORBGPU_MAX_LEVELS]; EHIP without a device.  An octave
 * outside [0, nlevels) is never read through (O1).  The batch form is ONE launch, one workgroup per candidate. */
int orbgpu_sim3_optimize_device(const orbgpu_sim3_opt_problem *p, int32_t device_id, void *hip_stream);
int orbgpu_sim3_optimize_batch_device(int32_t n, const orbgpu_sim3_opt_problem *problems, int32_t device_id,
                                      void *hip_stream);
/* Host arrays, synchronises: inlier [n1] in/out (written for correspondences only; may be NULL when n1 == 0), n_inliers
 * the return value of OptimizeSim3, result may be NULL.  Runs on a stream of the workspace's own and waits for the whole
 * device on entry, like the other host flavours. */
int orbgpu_sim3_optimize(const orbgpu_sim3_opt_problem *p, uint8_t *inlier, int32_t *n_inliers,
                         orbgpu_sim3_opt_result *result, int32_t device_id);
/* Diagnostic: problems of the calling thread's most recent Sim3 optimisation on device_id whose correspondences did not
 * fit the workgroup's LDS and went through the global-memory spill (ORBGPU_DEBUG_SIM3OPT_LDS_PAIRS=<k> lowers the limit
 * for tests).  Synchronises the device. */
int orbgpu_sim3_opt_last_spills(int32_t device_id, int32_t *problems_spilled);

/* ---- PnPsolver (PnPsolver.cc, EPnP + RANSAC): the pose of a relocalisation candidate on the device ----------------------
 * The third of the six steps Tracking::Relocalization runs per candidate key frame (Tracking.cc:1645-1810), between
 * orbgpu_search_by_bow and orbgpu_pose_optimization.  All hypotheses of a candidate are evaluated at once, one wave each;
 * the reference's sequential acceptance rule, its Refine included, is replayed over the per-hypothesis counts.  Every
 * result is "vs CPU restatement; OpenCV boundary unpinned"; tests/pnp_model.py is the restatement.  Conventions P1-P10
 * (DESIGN.md section 2):
 *   P1 rows (:67-101)     row i is kept iff valid[i] != 0 (the caller's verdict on: has a map point that is not bad) and
 *                         octave[i] lies in [0, nlevels); a valid row with an octave outside is not kept and counted in
 *                         n_bad_index.  Kept rows are compacted in index order: N of them.  kp[i] = mvKeysUn[i].pt,
 *                         Xw[i] the float world position.
 *   P2 thresholds (:154-156)  maxError = level_sigma2[octave] * th2, one float product
 *   P3 parameters (:121-152)  on the host (orbgpu_pnp_ransac_parameters): nMinInliers = (int)((float)N * epsilon), raised
 *                         to min_inliers, then to min_set; epsilon raised to (float)nMinInliers / N; nIterations = 1 if
 *                         nMinInliers == N, else ceil(log(1 - p) / log(1 - pow((double)epsilon, 3))) in double -- the
 *                         exponent is 3 whatever min_set is; NaN or outside int counts as larger than max_iterations (H4);
 *                         max_its = max(1, min(nIterations, max_iterations)); N = 0 gives 1.
 *   P4 minimal sets       the library draws nothing: sets[h][min_set] index the compacted list.  The first
 *                         n_use = min(n_hyp, max(max_its, start_iteration + n_iterations)) are used (none if N <
 *                         nMinInliers).  orbgpu_shim::PnPSampleSets replays the reference's draw (:188-201), its quirk
 *                         included (position idx, not randi, is overwritten: an index may repeat within a set).  A used set
 *                         with an index outside [0, N) is never read through: count 0, NaN Tcw, counted in n_bad_set.  A
 *                         set with a repeated index is computed like any other.
 *   P5 EPnP (:375-525, :651-858)  FP64, one rounding per operation, only + - * / sqrt.  A sum over the points of a set is
 *                         a wave sum: lane l of 64 adds the terms l, l + 64, ... from +0.0, then the partial sums are folded
 *                         by halves (l += l + 32, 16, ... 1).  Symmetric eigenproblems (3x3 PCA, 12x12 M'M, the normal
 *                         matrices below, abt'abt) use cyclic Jacobi: pairs row by row, at most 30 sweeps, H6's stopping
 *                         rule and rotation formulas; where an order matters eigenvalues are sorted descending with a
 *                         stable sort and every eigenvector is flipped so that its component of largest magnitude (lowest
 *                         index on ties) is positive.  Control points: centroid + sqrt(max(lambda_i, 0) / n) u_i.  The
 *                         inverse of CC = U diag(k_i) is diag(1 / k_i) U' with 1 / k_i = 0 when k_i <= 1e-6 k_0 (coplanar
 *                         sets).  Null-space basis: for k = max(0, 12 - 2n) > 0 the k smallest eigenvectors are replaced by
 *                         the canonical basis of their span -- the projector's columns orthonormalised by pivoted
 *                         Gram-Schmidt (largest remaining column, lowest index on ties), sign rule as above; the others
 *                         are the plain eigenvectors.  L, rho and the three beta approximations as the reference; their
 *                         least-squares solves go through the Jacobi of L'L, eigenvalues <= 1e-12 x the largest dropped
 *                         (minimum-norm solution).  Gauss-Newton: 5 iterations, Householder QR, the column scale taken
 *                         over all remaining rows; a zero pivot column gives x = 0.  R = U V' of abt = U S V' with V from
 *                         the Jacobi of abt'abt and u_k = abt v_k / |abt v_k|; the third ROW is flipped when det < 0
 *                         (:618-622).  Among the three solutions the mean reprojection error decides by strict <.  No
 *                         special cases beyond these: NaN follows IEEE and ends in count 0.
 *   P6 inliers (:308-339) Xc, Yc: double expressions rounded to float; invZc = (float)(1.0 / double expression); ue, ve
 *                         double; distX, distY, error2 float; inlier iff error2 < maxError
 *   P7 refine (:260-305)  EPnP over the best inlier set in index order, then P6; successful iff the refined count >
 *                         nMinInliers (strict; the gate before it is >=)
 *   P8 acceptance (:165-258)  N < nMinInliers: no_more at once.  Scanning from (start_iteration, best_so_far), hypothesis h
 *                         sets a record iff count >= nMinInliers && count > best; only records are refined (only a record
 *                         changes what Refine reads).  The scan ends at the first successful refine, or when
 *                         iterations >= max_its AND this call has scanned at least n_iterations hypotheses (the
 *                         reference's || in :182: the first iterate(5, ...) runs to max_its); no_more iff it ended that
 *                         way, and then the result is the best record's own pose and mask if this call set one.  A scan
 *                         that reaches n_use first ends with no_more = 0: draw further sets and call again.
 *   P9 outputs            Tcw = the float of R, t entry by entry in a 4x4 identity; masks one bit per original row i
 *   P10 limits            n1 in [0, 16384], n_hyp in [0, 4096], min_set in [4, 64], nlevels in [1, ORBGPU_MAX_LEVELS];
 *                         every device loop has a fixed bound */
typedef struct orbgpu_pnp_result { /* device or host */
    int32_t n;              /* N: kept rows */
    int32_t min_inliers;    /* mRansacMinInliers after P3 */
    int32_t max_its;        /* mRansacMaxIts (P3) */
    int32_t n_bad_index;    /* valid rows with an octave outside [0, nlevels): not kept */
    int32_t n_bad_set;      /* used sets with an index outside [0, N) */
    int32_t accepted;       /* the iteration whose Refine succeeded (0-based index into sets) or -1 */
    int32_t n_inliers;      /* nInliers: the refined count, or the best record's with the fallback of no_more, else 0 */
    int32_t best_inliers;   /* mnBestInliers after the scan */
    int32_t best_iteration; /* the record that holds it, -1 if this call set none */
    int32_t iterations;     /* mnIterations after the scan */
    int32_t no_more;        /* bNoMore */
    int32_t pad_;
    float Tcw[16];          /* the returned pose (refined, or the fallback's); zeros if none */
} orbgpu_pnp_result;

/* The array pointers are DEVICE pointers for the *_device entry points and HOST pointers for the host flavours. */
typedef struct orbgpu_pnp_problem {
    int32_t n1;             /* vpMapPointMatches.size() */
    int32_t n_hyp;          /* H: rows of sets */
    const uint8_t *valid;   /* [n1] (P1) */
    const float *Xw;        /* [n1][3] world position of the map point of key point i (read for valid rows only) */
    const float *kp;        /* [n1][2] mvKeysUn[i].pt */
    const int32_t *octave;  /* [n1] mvKeysUn[i].octave */
    const int32_t *sets;    /* [n_hyp][min_set] (P4) */
    float fx, fy, cx, cy;
    float level_sigma2[ORBGPU_MAX_LEVELS]; /* mvLevelSigma2 */
    int32_t nlevels;
    int32_t min_set, min_inliers, max_iterations; /* SetRansacParameters' arguments */
    float epsilon, th2;
    double probability;
    int32_t start_iteration, best_so_far; /* P8: 0, 0 for a fresh solver */
    int32_t n_iterations;   /* iterate's argument; 0: scan to max_its */
    int32_t pad_;
    /* outputs (the host flavours ignore them) */
    int32_t *counts;        /* [n_hyp]: inliers of hypothesis h; 0 for h >= n_use */
    float *Tcw;             /* [n_hyp][16], written for h < n_use */
    uint64_t *masks;        /* [n_hyp][(n1 + 63) / 64]: bit i % 64 of word i / 64; written for h < n_use */
    uint64_t *refined_mask; /* [(n1 + 63) / 64]: vbInliers of the returned pose; zeros if none */
    int32_t *indices;       /* [n1] mvKeyPointIndices (compacted -> i), first N written; may be NULL */
    orbgpu_pnp_result *result;
} orbgpu_pnp_problem;

/* P3 on the host; EINVAL for a null pointer or a negative n / min_inliers / max_iterations / min_set. */
int orbgpu_pnp_ransac_parameters(int32_t n, double probability, int32_t min_inliers, int32_t max_iterations, int32_t min_set,
                                 float epsilon, int32_t *adjusted_min_inliers, int32_t *max_its);
/* Enqueued on hip_stream; synchronisation, workspace and error rules as orbgpu_sim3_solve_device: the call waits for the
 * stream on entry and between the preparation and the hypotheses (N is read back for P3); the hypotheses and the scan are
 * enqueued and not waited for.  EINVAL: null pointers, a P10 violation, negative min_inliers / max_iterations /
 * start_iteration / best_so_far / n_iterations; nothing is launched then.  EHIP without a device.  The batch form is one
 * launch sequence (three kernels) for all candidates of a Relocalization call. */
int orbgpu_pnp_solve_device(const orbgpu_pnp_problem *p, int32_t device_id, void *hip_stream);
int orbgpu_pnp_solve_batch_device(int32_t n, const orbgpu_pnp_problem *problems, int32_t device_id, void *hip_stream);
/* Host arrays, synchronises.  counts [n_hyp]; Tcw [16] the returned pose (= result->Tcw); inliers [n1] bytes of the
 * returned pose (all 0 if none).  counts, Tcw and inliers may be NULL.  A set index outside [0, N) among the used
 * hypotheses is EINVAL here, before anything is launched. */
int orbgpu_pnp_solve(const orbgpu_pnp_problem *p, int32_t *counts, float *Tcw, uint8_t *inliers, orbgpu_pnp_result *result,
                     int32_t device_id);
/* As orbgpu_pnp_solve, but every hypothesis comes back: counts [n_hyp], Tcw [n_hyp][16], masks [n_hyp][(n1 + 63) / 64],
 * refined_mask [(n1 + 63) / 64] (any may be NULL); hypotheses h >= n_use are zeros (orbgpu_shim::PnPsolverT). */
int orbgpu_pnp_solve_all(const orbgpu_pnp_problem *p, int32_t *counts, float *Tcw, uint64_t *masks, uint64_t *refined_mask,
                         orbgpu_pnp_result *result, int32_t device_id);
/* Over the MapPoint table and an uploaded frame: kp_ids [n] = mnId of vpMapPointMatches[i] or -1.  The rows of P1 are built
 * on the device: row i is valid iff its id is known and the point is not bad, Xw is the table's world position, kp and
 * octave the frame's key point.  Ids the table does not know are not rows and are counted through
 * orbgpu_mappoint_table_last_unknown, as orbgpu_pose_optimization_table does.  params: the scalar members of the problem
 * and n_hyp / sets (a HOST array); n1 and the other array pointers are ignored (n1 = the frame's key points).  counts
 * [n_hyp], Tcw [16] and inliers [n] as orbgpu_pnp_solve (any may be NULL).  A set index outside [0, N) is counted in
 * n_bad_set, as in the device flavours (N depends on the table's bad flags).  Synchronises. */
int orbgpu_pnp_solve_table(const orbgpu_frame *fr, orbgpu_mappoint_table *t, const int64_t *kp_ids,
                           const orbgpu_pnp_problem *params, int32_t *counts, float *Tcw, uint8_t *inliers,
                           orbgpu_pnp_result *result);

/* ---- Initializer (Initializer.cc, H / F RANSAC and two-view reconstruction): the monocular bootstrap on the device ------
 * The consumer of orbgpu_search_for_initialization (Tracking.cc:891): all homography and fundamental-matrix hypotheses at
 * once, one wave each; the reference's scans, its branch, the 8 (Faugeras) or 4 (DecomposeE) motions, CheckRT with a
 * per-lane triangulation, and its accept rule.  Every result is "vs CPU restatement; OpenCV boundary unpinned";
 * tests/init_model.py is the restatement.  Conventions I1-I10:
 *   I1 rows (:54-63)      pair i is kept iff 0 <= matches12[i] < n2; a value >= n2 is not kept and counted in n_bad_index.
 *                         N kept pairs, compacted in index order.
 *   I2 sets (:78-97)      the library draws nothing: sets[h][8] index the compacted list (orbgpu_shim replays the draw).  A
 *                         set with an index outside [0, N) is never read through: score 0, empty mask, cannot be selected,
 *                         counted (once) in n_bad_set; EINVAL in the host flavours before anything is launched.  N < 8:
 *                         nothing is computed, success = 0, every output zero.  A repeated index is computed like any other.
 *   I3 Normalize (:749-795)  over ALL key points of a frame: the reference's running float sums in index order (mean, then
 *                         mean absolute deviation), mean = sum / (float)n, sX = (float)(1.0 / (double)meanDevX), the
 *                         normalised point (x - meanX) * sX, T = [sX 0 -meanX*sX; 0 sY -meanY*sY; 0 0 1] in float.
 *   I4 DLT, 3x3 products  A's entries are the reference's float products (:239-257, :281-289); A'A accumulated in FP64 in
 *                         row order; cyclic Jacobi, stopping rule, stable descending sort and sign rule as P5 / H6; the null
 *                         vector (smallest eigenvalue) is rounded to float.  3x3 products are FP64 over the float entries,
 *                         (a b + c d) + e f per entry, left product first, each entry rounded to float once: inv(T2) Hn T1
 *                         (inv(T2) written out: 1 / sX, -t / sX), H12 = adj(H21) / det(H21), T2' Fn T1, K' F K and
 *                         inv(K) H K (inv(K) written out).  A 3x3 SVD A = U diag(d) V': V from the Jacobi of A'A (sorted,
 *                         sign rule), u_k = A v_k / |A v_k| and d_k = |A v_k| for k = 0, 1; u_2 = u_0 x u_1 normalised,
 *                         d_2 = |A v_2|; for ReconstructH u_2 is flipped when u_2 . (A v_2) < 0 (a proper SVD, s depends on
 *                         it), for DecomposeE by the sign rule (A v_2 is rounding noise there).  F's rank-2 projection is
 *                         (d_0 u_0) v_0' + (d_1 u_1) v_1' in FP64, rounded to float.
 *   I5 checks (:305-468)  float, one rounding per operation, the reference's expression order; 1.0 / x is a double division
 *                         of the float expression rounded to float, invSigmaSquare likewise; thresholds 5.991f, 3.841f.
 *                         A term is an inlier's iff chiSquare <= th (a NaN chiSquare is an outlier's and adds nothing: it
 *                         would poison every score in the reference).  The score is the running float sum in index order,
 *                         term 1 before term 2.  Mask bit e = compacted pair e.
 *   I6 selection          h ascending, strict > from 0.0f; a NaN score never wins; no winner: best = -1, empty mask, zero
 *                         matrix (the F branch then has N = 0 inliers and fails, the quirk of :178 restated).
 *   I7 branch (:112-118)  RH = SH / (SH + SF) in float, H iff (double)RH > 0.40; NaN takes the F branch.
 *   I8 motions (:470-732, :909-929)  SVDs as I4, rounded to float; everything after in float in the reference's order, 3x3
 *                         float products (a b + c d) + e f, left product first; determinants cv::determinant's double
 *                         expression over the float entries; s = (float)(det(U) det(Vt)); ratio tests
 *                         (double)(d1 / d2) < 1.00001; cv::norm an FP64 sum and sqrt rounded to float; the eight motions in
 *                         the reference's order, F's as (R1,t) (R2,t) (R1,-t) (R2,-t) with DecomposeE's determinant flips;
 *                         nMinGood = max((int)(0.9 * N), min_triangulated) and the 0.7 / 0.75 / 0.9 products in double;
 *                         first wins on ties exactly as the two if chains are written (H: > scan with a second best; F: the
 *                         == chain, which stops at the first motion that has maxGood whether its parallax passes or not).
 *   I9 CheckRT, Triangulate (:734-747, :798-907)  A's rows the reference's float expressions, P2 = K [R|t] a float product;
 *                         the eigenvector of the smallest eigenvalue of the 4x4 A'A (FP64, Jacobi as I4) rounded to float
 *                         and divided by its fourth component in float; isfinite checked; normal . normal an FP64 sum,
 *                         cosParallax = (float)(dot / (double)(dist1 * dist2)); both depth tests use
 *                         (double)cosParallax < 0.99998; reprojection tests in float, th2 = (float)(4.0 * sigma * sigma);
 *                         P3D and triangulated have n1 entries indexed by pair.first.  A pair that passes every test with
 *                         cosParallax >= 0.99998 writes its point and counts in nGood but is not triangulated.  The parallax
 *                         cosine of a motion is the element of rank min(50, nGood - 1) in ascending order (order of the
 *                         sign-magnitude float keys); 1.0f for nGood = 0 (the reference's parallax = 0).
 *   I10 parallax          no acosf on the device: the entry point computes, with the host's acosf and a bisection over the
 *                         float's bits, the largest cosines for which (float)(acosf(c) * 180 / CV_PI) > min_parallax (F)
 *                         and >= min_parallax (H) hold (NaN if none does); the kernel compares cosines.  cos_parallax[] is
 *                         carried in the result; the host flavours fill parallax_deg with the reference's expression.
 *   Limits                n1, n2 in [0, 16384], n_hyp in [0, 4096], sigma > 0, min_triangulated >= 0; every device loop has
 *                         a fixed bound. */
typedef struct orbgpu_init_result { /* device or host */
    int32_t n;                  /* N: kept pairs */
    int32_t n_bad_index;        /* matches12[i] >= n2 */
    int32_t n_bad_set;          /* sets with an index outside [0, N) */
    int32_t best_h, best_f;     /* the winning hypotheses or -1 */
    float SH, SF, RH;
    int32_t used_homography;    /* the branch of I7 */
    int32_t n_inliers;          /* the N of Reconstruct*: inliers of the selected model */
    int32_t n_good[8];          /* nGood per motion (F: four, the rest 0) */
    float cos_parallax[8];      /* I9's cosine per motion; 0 for a motion that was not checked */
    int32_t best_motion;        /* H: bestSolutionIdx; F: the first motion with maxGood; -1 if none */
    int32_t second_best_good;   /* H: secondBestGood; F: nsimilar */
    int32_t success;            /* Initialize's return value */
    float parallax_deg;         /* host flavours only: the reference's parallax of best_motion; 0 otherwise */
    float H21[9], F21[9];       /* the selected matrices (zeros if none won) */
    float R21[9], t21[3];       /* the motion on success, zeros otherwise */
} orbgpu_init_result;

/* The array pointers are DEVICE pointers for the *_device entry points and HOST pointers for the host flavours. */
typedef struct orbgpu_init_problem {
    int32_t n1, n2;             /* key points of the reference (1) and the current (2) frame */
    const float *kp1, *kp2;     /* [n1][2], [n2][2] mvKeysUn[i].pt */
    const int32_t *matches12;   /* [n1] (I1) */
    const int32_t *sets;        /* [n_hyp][8] (I2) */
    int32_t n_hyp;
    float fx, fy, cx, cy;
    float sigma, min_parallax;  /* 1.0, 1.0 in Tracking.cc */
    int32_t min_triangulated;   /* 50 */
    /* outputs (the host flavours ignore them) */
    float *scores_h, *scores_f; /* [n_hyp] */
    uint64_t *masks_h, *masks_f; /* [n_hyp][(n1 + 63) / 64], bit e of a row = compacted pair e */
    float *R21, *t21;           /* [9], [3]; may be NULL (the result holds them too) */
    float *P3D;                 /* [n1][3] vIniP3D, zeros unless success */
    uint8_t *triangulated;      /* [n1] vbTriangulated, zeros unless success */
    orbgpu_init_result *result;
} orbgpu_init_problem;

/* I10 on the host: the two cosine limits of min_parallax (F's strict one, H's); EINVAL for a null pointer. */
int orbgpu_initializer_cos_limits(float min_parallax, float *limit_f, float *limit_h);
/* Enqueued on hip_stream; workspace and error rules as orbgpu_pnp_solve_device.  The call waits for the stream on entry
 * only (N stays on the device).  EINVAL: null pointers, a limit violated, sigma <= 0 or NaN, min_triangulated < 0; nothing
 * is launched then.  EHIP without a device.  The batch form is one launch sequence (five kernels) for all problems. */
int orbgpu_initializer_device(const orbgpu_init_problem *p, int32_t device_id, void *hip_stream);
int orbgpu_initializer_batch_device(int32_t n, const orbgpu_init_problem *problems, int32_t device_id, void *hip_stream);
/* Host arrays, synchronises.  P3D [n1][3] and triangulated [n1] may be NULL.  A set index outside [0, N) is EINVAL here
 * (when N >= 8), before anything is launched. */
int orbgpu_initializer(const orbgpu_init_problem *p, float *P3D, uint8_t *triangulated, orbgpu_init_result *result,
                       int32_t device_id);
/* As orbgpu_initializer, but every hypothesis comes back: scores_h, scores_f [n_hyp], masks_h, masks_f
 * [n_hyp][(n1 + 63) / 64] (any may be NULL). */
int orbgpu_initializer_all(const orbgpu_init_problem *p, float *scores_h, float *scores_f, uint64_t *masks_h,
                           uint64_t *masks_f, float *P3D, uint8_t *triangulated, orbgpu_init_result *result,
                           int32_t device_id);

/* ---- LocalMapping::CreateNewMapPoints (LocalMapping.cc:207-452): the neighbour loop on the device ------------------------
 * One call runs the loop for one current key frame (kf1) and nn neighbours: per neighbour SearchForTriangulation, then per
 * match the parallax branch, the 4x4 triangulation or the stereo back-projection, and the depth, reprojection and scale
 * gates.  Neighbour k's matcher skips the key points of kf1 that got a point from neighbours < k (ORBmatcher.cc:702-705
 * reads GetMapPoint): a working copy of kf1's has_mp carries that on the device, all launches go onto one stream and the
 * host is not consulted in between.  The caller chooses the neighbours, applies the baseline / median-depth test
 * (:244-261), computes F12 and the epipole, and does the map edits (:434-449) from the outputs in (neighbour, key point)
 * order.  vs CPU restatement; OpenCV boundary unpinned -- tests/newpts_model.py is the restatement.  Conventions:
 *   N1 match (:268)        per neighbour exactly orbgpu_search_for_triangulation (same device code) over has_mp1 OR every
 *                          status > 0 of earlier neighbours; the caller's has_mp array is not written.
 *   N2 rays (:300-304)     xn = ((x - cx) * invfx, (y - cy) * invfy, 1) in float; Rwc = the transpose of Tcw's rotation (the
 *                          reference's Rcw.t()); 3x3 . 3x1 products in float, (a b + c d) + e f, then the added term if any.
 *   N3 parallax (:305-319) Mat::dot and cv::norm are FP64 sums over the float entries (norm: sqrt of the sum, kept in
 *                          double); cosParallaxRays = (float)(dot / (norm1 * norm2)); cosParallaxStereo = cosRays + 1 in
 *                          float; cos_stereo[i] = cos(2*atan2(mb/2, mvDepth[i])) comes from the caller (no libm on the
 *                          device); kf2's is only looked at when kf1's key point is not stereo (the else-if of :313);
 *                          `cosRays < 0.9998` compares in double.
 *   N4 A (:322-326)        rows x * Tcw.row(2) - Tcw.row(0) etc., float, one rounding per operation.
 *   N5 null vector (:329-337)  A'A in FP64 in row order, cyclic Jacobi in one lane (I9's jacobi4_lane), the eigenvector of
 *                          the least eigenvalue (last of the stable descending order, sign rule), rounded to float; fourth
 *                          component == 0 rejects; the point is the float quotient by it.
 *   N6 UnprojectStereo (KeyFrame.cc:653-669)  z = depth[i]; x = (u - cx) * z * invfx, y likewise, float, left to right, with
 *                          (u, v) = kp_raw[i] (mvKeys, not mvKeysUn; NULL: kp_x / kp_y); Twc's rotation times (x, y, z) plus
 *                          its translation as N2.  Deviation D2: depth <= 0 rejects (the reference dereferences an empty Mat).
 *   N7 finite              deviation D1: a point with a non-finite coordinate rejects (the reference keeps it: NaN fails
 *                          every > test).
 *   N8 depths (:354-360)   z = (float)(dot + (double)t) with dot the FP64 sum over float entries; x, y likewise.
 *   N9 reprojection (:363-413)  invz = (float)(1.0 / (double)z); u = fx * x * invz + cx in float left to right; u_r = u -
 *                          mbf * invz with kf1's mbf for BOTH key frames (:406 restated); the error sums in float left to
 *                          right, compared as (double)err2 > 5.991 * (double)sigma2 (mono) or 7.8 (stereo); sigma2 =
 *                          level_sigma2[octave] of the frame.
 *   N10 scale (:416-431)   normal = x3D - Ow in float with Ow = Twc's translation; dist = (float)sqrt(FP64 sum); either == 0
 *                          rejects; ratioDist = dist2 / dist1, ratioOctave = scale1[o1] / scale2[o2] in float;
 *                          ratioDist * ratio_factor < ratioOctave || ratioDist > ratioOctave * ratio_factor rejects.
 *   N11 outputs            [nn][n1] indexed by kf1's key point: match12 (after the rotation check), status, x3d (zeros unless
 *                          status > 0); n_matches[nn], n_created[nn], n_done.  Two key points of kf1 may create a point on
 *                          the same key point of kf2 (the reference's later AddMapPoint overwrites the earlier).
 *   N12 stop flag (:239)   optional device-readable int32; a single-workgroup kernel latches go/stop once per neighbour
 *                          before that neighbour's matcher, so a neighbour is processed completely or not at all; neighbour 0
 *                          always is; once one is skipped all later ones are (match12 -1, status 0, x3d 0, counts 0).  The
 *                          result is reproducible only for a flag that does not change during the call.
 *   N13 determinism        no floating-point atomics; every device loop has a fixed bound; the same problem gives the same
 *                          bytes.
 *   Limits                 nn in [0, ORBGPU_NEW_POINTS_MAX_NEIGHBOURS]; key points per frame in [0, 65535]; nlevels in
 *                          [1, ORBGPU_MAX_LEVELS].  An octave outside [0, nlevels) is EINVAL in the host flavour; the device
 *                          flavour cannot see the arrays: such a candidate never matches and such a key point of kf1
 *                          rejects with ORBGPU_NP_BAD_OCTAVE, nothing is read out of range. */
#define ORBGPU_NEW_POINTS_MAX_NEIGHBOURS 32
enum {
    ORBGPU_NP_NONE = 0,            /* no match */
    ORBGPU_NP_TRIANGULATED = 1,    /* :320-339 */
    ORBGPU_NP_UNPROJECT1 = 2,      /* :342 */
    ORBGPU_NP_UNPROJECT2 = 3,      /* :346 */
    ORBGPU_NP_LOW_PARALLAX = -1,   /* :349 */
    ORBGPU_NP_W_ZERO = -2,         /* :333 */
    ORBGPU_NP_Z1 = -3,             /* :355 */
    ORBGPU_NP_Z2 = -4,             /* :359 */
    ORBGPU_NP_REPROJ1 = -5,        /* :374 / :385 */
    ORBGPU_NP_REPROJ2 = -6,        /* :400 / :411 */
    ORBGPU_NP_ZERO_DIST = -7,      /* :422 */
    ORBGPU_NP_SCALE = -8,          /* :430 */
    ORBGPU_NP_NON_FINITE = -9,     /* D1 */
    ORBGPU_NP_STEREO_DEPTH = -10,  /* D2 */
    ORBGPU_NP_BAD_OCTAVE = -11     /* device flavour only, see Limits */
};
/* A key frame as CreateNewMapPoints reads it; arrays [n], device pointers in the device flavour and host pointers in the
 * host flavour.  kp_angle may be NULL without check_orientation, kp_raw may be NULL (N6).  F12 (row-major, as
 * orbgpu_search_for_triangulation takes it) and the epipole are read for neighbours only; a neighbour's mbf is not read. */
typedef struct orbgpu_new_points_frame {
    int32_t n, nlevels;
    const float *kp_x, *kp_y;   /* mvKeysUn */
    const int32_t *kp_octave;
    const float *kp_angle;
    const float *u_right;       /* mvuRight */
    const uint8_t *desc;        /* [n][32] */
    const uint8_t *has_mp;      /* the key point has a map point */
    const int32_t *node;        /* orbgpu_bow_transform's node_id */
    const float *depth;         /* mvDepth */
    const float *kp_raw;        /* [n][2] mvKeys[i].pt or NULL */
    const float *cos_stereo;    /* N3 */
    float Tcw[16], Twc[16];     /* both as the key frame stores them */
    float fx, fy, cx, cy, invfx, invfy, mbf;
    float level_sigma2[ORBGPU_MAX_LEVELS], scale_factors[ORBGPU_MAX_LEVELS];
    float F12[9], ex, ey;
} orbgpu_new_points_frame;

typedef struct orbgpu_new_points_problem {
    orbgpu_new_points_frame kf1;
    const orbgpu_new_points_frame *neighbours; /* HOST array [nn] in both flavours */
    int32_t nn;
    int32_t only_stereo, check_orientation;
    float ratio_factor;      /* 1.5f * mfScaleFactor */
    const int32_t *stop;     /* N12 or NULL; the host flavour samples *stop at the call */
    int32_t *match12;        /* [nn][n1] */
    int32_t *status;         /* [nn][n1] */
    float *x3d;              /* [nn][n1][3] */
    int32_t *n_matches;      /* [nn] */
    int32_t *n_created;      /* [nn] */
    int32_t *n_done;         /* [1] neighbours processed */
} orbgpu_new_points_problem;

/* Device arrays, enqueued on hip_stream; workspace rules as orbgpu_pnp_solve_device (one call at a time per thread and
 * device), but nothing is waited for: the call returns once the launches are queued.  EINVAL (nothing launched): null
 * pointers, a limit violated.  EHIP without a device. */
int orbgpu_create_new_map_points_device(const orbgpu_new_points_problem *p, int32_t device_id, void *hip_stream);
/* Host arrays: one staged upload of everything, the chain, one download; synchronises. */
int orbgpu_create_new_map_points(const orbgpu_new_points_problem *p, int32_t device_id);


/* LastFrame members read by SearchByProjection(CurrentFrame, LastFrame, th, bMono). */
typedef struct {
    int32_t n;
    const uint8_t *has_mp;    /* mvpMapPoints[i] != NULL */
    const uint8_t *outlier;   /* mvbOutlier[i]; may be NULL */
    const uint8_t *obs_pos;   /* pMP->Observations()>0; may be NULL (= all true) */
    const float *world_pos;   /* n x 3 */
    const uint8_t *desc;      /* pMP->GetDescriptor(), n x 32 */
    const int32_t *kp_octave; /* LastFrame.mvKeys[i].octave */
    const float *kp_angle;    /* LastFrame.mvKeysUn[i].angle */
    const float *Tcw;         /* LastFrame.mTcw, 4x4 row-major */
} orbgpu_lastframe_view;

/* ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono)
 * (ORBmatcher.h:52, ORBmatcher.cc:1328-1470; Tracking::TrackWithMotionModel, Tracking.cc:1169). */
int orbgpu_search_by_projection_last(const orbgpu_frame_view *cur, const float *cur_Tcw, float fx, float fy,
                                     float cx, float cy, float mbf, float mb, const orbgpu_lastframe_view *last,
                                     float th, int32_t mono, int32_t check_orientation, int32_t *kp_to_mp,
                                     int32_t *nmatches, int32_t device_id);

/* pKF->GetMapPointMatches() members read by the relocalisation matcher. */
typedef struct {
    int32_t n;
    const uint8_t *has_mp;        /* vpMPs[i] != NULL */
    const uint8_t *bad;           /* isBad(); may be NULL */
    const uint8_t *already_found; /* sAlreadyFound.count(pMP); may be NULL */
    const float *world_pos;       /* n x 3 */
    const float *min_dist_inv;    /* GetMinDistanceInvariance() (MapPoint.cc:373-377) */
    const float *max_dist_inv;    /* GetMaxDistanceInvariance() (MapPoint.cc:379-383) */
    const float *max_dist;        /* mfMaxDistance, the numerator of MapPoint::PredictScale (MapPoint.cc:385-394) */
    const uint8_t *desc;          /* GetDescriptor(), n x 32 */
    const float *kp_angle;        /* pKF->mvKeysUn[i].angle */
} orbgpu_keyframe_view;

/* ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound,
 * th, ORBdist) (ORBmatcher.h:56, ORBmatcher.cc:1472-1599; Tracking::Relocalization, Tracking.cc:1756,1770).
 * log_scale_factor = CurrentFrame.mfLogScaleFactor.  kp_to_mp in: -1 = free, anything else = occupied
 * (any association hides the key point, :1540-1541); out: index of the key-frame map point. */
int orbgpu_search_by_projection_keyframe(const orbgpu_frame_view *cur, const float *cur_Tcw, float fx, float fy,
                                         float cx, float cy, float log_scale_factor,
                                         const orbgpu_keyframe_view *kf, float th, int32_t orb_dist,
                                         int32_t check_orientation, int32_t *kp_to_mp, int32_t *nmatches,
                                         int32_t device_id);

/* ======================================================================================
 * Vocabulary tree (DBoW2, vendored in the reference): Frame::ComputeBoW (src/Frame.cc:395-402) and the node-wise
 * ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) (src/ORBmatcher.cc:159-288).
 * ====================================================================================== */
typedef struct orbgpu_vocabulary orbgpu_vocabulary;

/* The tree as TemplatedVocabulary::loadFromTextFile builds it (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1348-1437):
 * node 0 is the root, node i > 0 has parent[i] < i (file order), children of a node are visited in ascending id,
 * leaves are numbered in node order (= word ids).  desc [n_nodes][32], weight [n_nodes] (Node::weight, doubles);
 * weighting 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY; scoring 0 L1_NORM .. 5 DOT_PRODUCT (BowVector.h:30-54).
 * The binary / text vocabulary FILE readers stay host code of the caller (the reference's own loader can fill
 * these arrays from m_nodes). */
int orbgpu_vocabulary_create(int32_t k, int32_t L, int32_t n_nodes, const int32_t *parent, const uint8_t *is_leaf,
                             const uint8_t *desc, const double *weight, int32_t weighting, int32_t scoring,
                             int32_t device_id, orbgpu_vocabulary **out);
int orbgpu_vocabulary_destroy(orbgpu_vocabulary *v);
int orbgpu_vocabulary_size(const orbgpu_vocabulary *v, int32_t *n_words);

/* TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup) (:1140-1207): per feature the
 * word id, the word's weight and the id of the node `levelsup` levels above the word (:1231-1274; -1 if the word
 * is stopped, i.e. weight <= 0: such a feature enters neither vector); the BowVector as n_bow ascending
 * (bow_ids, bow_vals) pairs, weighted / normalised as the vocabulary's weighting and scoring types prescribe; the
 * FeatureVector as CSR: node fv_nodes[t] (ascending) holds features fv_items[fv_start[t] .. fv_start[t+1]) in
 * ascending feature index.  Capacities: n for every array, n + 1 for fv_start.  bow_* / fv_* may be NULL. */
int orbgpu_bow_transform(orbgpu_vocabulary *v, const uint8_t *desc, int32_t n, int32_t levelsup, int32_t *word_id,
                         double *word_weight, int32_t *node_id, int32_t *bow_ids, double *bow_vals, int32_t *n_bow,
                         int32_t *fv_nodes, int32_t *fv_start, int32_t *fv_items, int32_t *n_fv);
/* Device-resident: descriptors [batch][cap][32] straight out of the extractor, counts d_n [batch]; outputs
 * [batch][cap].  Asynchronous on hip_stream. */
int orbgpu_bow_transform_batch_device(orbgpu_vocabulary *v, const uint8_t *d_desc, int32_t batch, int32_t cap,
                                      const int32_t *d_n, int32_t levelsup, int32_t *d_word_id, double *d_word_weight,
                                      int32_t *d_node_id, void *hip_stream);

/* ORBmatcher::SearchByBoW(KeyFrame *pKF, Frame &F, vector<MapPoint*> &vpMapPointMatches) (ORBmatcher.cc:159-288):
 * key-frame feature i (valid_kf[i]: has a map point that is not bad) is compared with the frame features under the
 * same vocabulary node (node_kf / node_f: orbgpu_bow_transform's node_id, -1 = not in the feature vector), greedy
 * claims in the reference's visiting order, TH_LOW / ratio test, rotation histogram.  match_f[j] = key-frame
 * feature whose map point frame feature j received, or -1; *nmatches = the return value. */
int orbgpu_search_by_bow(const uint8_t *desc_kf, const float *angle_kf, const uint8_t *valid_kf,
                         const int32_t *node_kf, int32_t n_kf, const uint8_t *desc_f, const float *angle_f,
                         const int32_t *node_f, int32_t n_f, int32_t th_low, float nnratio, int32_t check_orientation,
                         int32_t *match_f, int32_t *nmatches, int32_t device_id);
/* The same for `pairs` independent (key frame, frame) pairs resident on the device; arguments as
 * orbgpu_match_bf_batch_device plus the node arrays [pairs][cap]. */
int orbgpu_search_by_bow_batch_device(orbgpu_matcher *m, int32_t pairs, int32_t cap, const uint8_t *d_desc_a,
                                      const void *d_angle_a, const uint8_t *d_valid_a, const int32_t *d_node_a,
                                      const int32_t *d_na, const uint8_t *d_desc_b, const void *d_angle_b,
                                      const int32_t *d_node_b, const int32_t *d_nb, size_t angle_stride, int32_t th_low,
                                      float nnratio, int32_t check_orientation, int32_t *d_match_b,
                                      int32_t *d_nmatches, void *hip_stream);

/* ---- the background-thread matchers (LocalMapping / LoopClosing), SURVEY.md M6 ----------------------------- */

/* ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12) (ORBmatcher.cc:522-655;
 * LoopClosing::ComputeSim3, LoopClosing.cc:266).  valid1 / valid2: the key point has a map point that is not bad.
 * match12[i1] = key point of key frame 2 whose map point vpMatches12[i1] receives, or -1. */
int orbgpu_search_by_bow_keyframes(const uint8_t *desc1, const float *angle1, const uint8_t *valid1,
                                   const int32_t *node1, int32_t n1, const uint8_t *desc2, const float *angle2,
                                   const uint8_t *valid2, const int32_t *node2, int32_t n2, float nnratio,
                                   int32_t check_orientation, int32_t *match12, int32_t *nmatches, int32_t device_id);

/* ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (ORBmatcher.cc:405-520;
 * Tracking::MonocularInitialization, Tracking.cc:877 -- monocular bootstrap only).  f1: kp_octave, kp_angle, desc of
 * the initial frame (its grid is not read); f2: the current frame; prev_matched [f1->n][2] in/out.  The Hamming
 * distances of every window candidate are computed on the device; the steal-if-strictly-closer bookkeeping between
 * rows (:441-470) is sequential and runs on the host over those lists, statement by statement. */
int orbgpu_search_for_initialization(const orbgpu_frame_view *f1, const orbgpu_frame_view *f2, float *prev_matched,
                                     int32_t window_size, float nnratio, int32_t check_orientation,
                                     int32_t *matches12, int32_t *nmatches, int32_t device_id);

/* ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) (ORBmatcher.cc:657-823, epipolar
 * test :140-157; LocalMapping::CreateNewMapPoints, LocalMapping.cc:268).  kf1 / kf2: the key frames as frame views
 * (kp_x / kp_y = mvKeysUn, u_right = mvuRight, kp_octave, kp_angle, desc; grids are not read); has_mp*: the key
 * point already has a map point; node*: orbgpu_bow_transform's node_id; F12 row-major 3x3; (ex, ey) the epipole
 * in image 2 (:664-670, from the poses); level_sigma2_2 = pKF2->mvLevelSigma2.  match12[i1] = i2 or -1; the pairs
 * vector of the reference is its non-negative entries in order. */
int orbgpu_search_for_triangulation(const orbgpu_frame_view *kf1, const uint8_t *has_mp1, const int32_t *node1,
                                    const orbgpu_frame_view *kf2, const uint8_t *has_mp2, const int32_t *node2,
                                    const float *F12, float ex, float ey, const float *level_sigma2_2,
                                    int32_t only_stereo, int32_t check_orientation, int32_t *match12,
                                    int32_t *nmatches, int32_t device_id);

/* ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, th) (ORBmatcher.cc:825-975;
 * LocalMapping::SearchInNeighbors, LocalMapping.cc:489, 514): the candidate phase.  pts->bad[i] = !pMP ||
 * pMP->isBad() || pMP->IsInKeyFrame(pKF).  best_idx[i] = the key point map point i fuses with (least distance in its
 * window after the level and reprojection-error gates, <= TH_LOW) or -1.  The map edits of :948-968 (Replace /
 * AddObservation / AddMapPoint) mutate the pointer graph and stay with the caller, applied in index order.
 * ORBGPU_ELEVEL if a predicted level falls outside [0, nlevels). */
int orbgpu_fuse(const orbgpu_frame_view *kf, const float *Tcw, float fx, float fy, float cx, float cy, float bf,
                float log_scale_factor, const orbgpu_points_view *pts, float th, const float *inv_level_sigma2,
                int32_t *best_idx, int32_t *n_candidates, int32_t device_id);
/* ORBmatcher::Fuse(KeyFrame *pKF, cv::Mat Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.cc:977-1100;
 * LoopClosing::SearchAndFuse, LoopClosing.cc:597): candidate phase.  pts->bad[i] = isBad() || already in pKF. */
int orbgpu_fuse_sim3(const orbgpu_frame_view *kf, const float *Scw, float fx, float fy, float cx, float cy,
                     float log_scale_factor, const orbgpu_points_view *pts, float th, int32_t *best_idx,
                     int32_t *n_candidates, int32_t device_id);
/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (ORBmatcher.cc:1102-1326;
 * LoopClosing::ComputeSim3, LoopClosing.cc:324).  pts1 / pts2: one row per key point of the key frame (bad[i] = no
 * map point or isBad(); normal is not read); already1 / already2 = vbAlreadyMatched1 / 2 (:1133-1144) or NULL;
 * T1w / T2w: the key-frame poses, R12 row-major 3x3.  match12[i1] = i2 where both directions agree, else -1. */
int orbgpu_search_by_sim3(const orbgpu_frame_view *kf1, const orbgpu_frame_view *kf2, const float *T1w, const float *T2w,
                          float s12, const float *R12, const float *t12, float fx, float fy, float cx, float cy,
                          float log_sf1, float log_sf2, const orbgpu_points_view *pts1, const uint8_t *already1,
                          const orbgpu_points_view *pts2, const uint8_t *already2, float th, int32_t *match12,
                          int32_t *nfound, int32_t device_id);

/* ======================================================================================
 * PointCloudMapping  (reference include/PointCloudMap.h:41-88, src/PointCloudMap.cc)
 * ====================================================================================== */

/* pcl::PointXYZRGBA payload: xyz + packed colour (b | g<<8 | r<<16 | a<<24). 16 B. */
typedef struct {
    float x, y, z;
    uint32_t rgba;
} orbgpu_point_xyzrgba;

typedef struct orbgpu_cloud orbgpu_cloud;

/* PointCloudMapping::PointCloudMapping(resolution, loopCloser) (PointCloudMap.h:46,
 * PointCloudMap.cc:36-57): voxel leaf = (float)resolution on all axes. */
int orbgpu_cloud_create(double resolution, int32_t device_id, orbgpu_cloud **out);
int orbgpu_cloud_destroy(orbgpu_cloud *h);

/* One key-frame step of PointCloudMapping::viewer (PointCloudMap.cc:204-262, no-loop branch):
 * convertToPointCloud(kf) -> transformPointCloud(Twc) -> globalMap += -> voxel.filter(globalMap).
 * depth: float32 metres (after DepthMapFactor), rgb: 8UC3 in the byte order of KeyFrame::mImRGB,
 * Tcw: kf->GetPose() 4x4 row-major float.  depth_stride in floats, rgb_stride in bytes. */
int orbgpu_cloud_insert(orbgpu_cloud *h, const float *depth, size_t depth_stride, const uint8_t *rgb,
                        size_t rgb_stride, int32_t width, int32_t height, float fx, float fy, float cx, float cy,
                        const float *Tcw);
/* Same step with the key frame's images already resident in device memory (e.g. the frame the extractor just
 * processed): nothing but the pose crosses PCIe.  Runs on the handle's stream and returns when the map is
 * updated. */
int orbgpu_cloud_insert_device(orbgpu_cloud *h, const float *d_depth, size_t depth_stride, const uint8_t *d_rgb,
                               size_t rgb_stride, int32_t width, int32_t height, float fx, float fy, float cx,
                               float cy, const float *Tcw);
/* Loop-closure branch (PointCloudMap.cc:217-243): drop the map, re-generate every key-frame cloud
 * with its (new) pose, filter once. Arrays of n key-frames of one size. */
int orbgpu_cloud_rebuild(orbgpu_cloud *h, int32_t n, const float *const *depth, size_t depth_stride,
                         const uint8_t *const *rgb, size_t rgb_stride, int32_t width, int32_t height, float fx,
                         float fy, float cx, float cy, const float *const *Tcw);
/* The shutdown pass of PointCloudMapping::viewer (PointCloudMap.cc:270-282): clear the map, then for every key
 * frame generatePointCloud + voxel.filter of THAT cloud alone + `globalMap += `.  After it the map is a
 * concatenation of per-key-frame filtered clouds (what optimized_pointcloud.pcd holds before the outlier filter). */
int orbgpu_cloud_clear(orbgpu_cloud *h);
int orbgpu_cloud_append_filtered(orbgpu_cloud *h, const float *depth, size_t depth_stride, const uint8_t *rgb,
                                 size_t rgb_stride, int32_t width, int32_t height, float fx, float fy, float cx,
                                 float cy, const float *Tcw);
/* The outlier filter of the shutdown pass (PointCloudMap.cc:46-47: sor.setMeanK(50), sor.setStddevMulThresh(1.0);
 * :283-285: sor.setInputCloud(globalMap); sor.filter(*tmp); globalMap->swap(*tmp)), applied to the handle's map in
 * place; the points that stay keep their order.  pcl::StatisticalOutlierRemoval is restated from PCL 1.7
 * (filters/impl/statistical_outlier_removal.hpp -- PCL is not vendored by the reference: unpinned): mean distance of
 * every point to its mean_k nearest neighbours (exact search, float squared distances as FLANN's L2_Simple, summed
 * in double), a point goes when that exceeds mean + stddev_mul * stddev of all of them.  mean_k <= 63; needs more
 * than mean_k points (PCL reads past the neighbour list otherwise).  removed may be NULL. */
int orbgpu_cloud_remove_outliers(orbgpu_cloud *h, int32_t mean_k, double stddev_mul, int64_t *removed);
int orbgpu_cloud_size(orbgpu_cloud *h, int64_t *n);
/* Global map in ascending voxel-index order (pcl::VoxelGrid output order). */
int orbgpu_cloud_download(orbgpu_cloud *h, orbgpu_point_xyzrgba *out, int64_t cap, int64_t *n);
/* 1 if the last filter hit PCL's int32 voxel-index overflow and returned its input unfiltered. */
int orbgpu_cloud_last_overflow(orbgpu_cloud *h, int32_t *overflow);
/* Which implementation served the last insert / rebuild: 1 = merge of the new points into the sorted resident
 * map, 2 = general path (sort of everything), 3 = merge attempted, its precondition check failed, redone by the
 * general path.  Results are identical; this is for tests and measurements. */
int orbgpu_cloud_last_path(orbgpu_cloud *h, int32_t *path);
/* Measurement aid: HIP events on the handle's stream around the kernels of an insert (first launch to last,
 * uploads and the final state read-back excluded); last_insert_ms fails if no profiled insert happened. */
int orbgpu_cloud_set_profiling(orbgpu_cloud *h, int32_t enable);
int orbgpu_cloud_last_insert_ms(orbgpu_cloud *h, float *ms);

/* Stateless stages (host pointers), for parity tests and other callers:
 * convertToPointCloud (PointCloudMap.cc:112-138) with optional pose transform (Tcw != NULL:
 * generatePointCloud, :78-110).  out cap >= ceil(h/3)*ceil(w/3). */
int orbgpu_backproject(const float *depth, size_t depth_stride, const uint8_t *rgb, size_t rgb_stride,
                       int32_t width, int32_t height, float fx, float fy, float cx, float cy, const float *Tcw,
                       orbgpu_point_xyzrgba *out, int64_t cap, int64_t *n, int32_t device_id);
/* pcl::VoxelGrid<PointXYZRGBA>::filter with leaf = (float)resolution (PointCloudMap.cc:41, 240-243). */
int orbgpu_voxel_filter(const orbgpu_point_xyzrgba *in, int64_t n, double resolution, orbgpu_point_xyzrgba *out,
                        int64_t cap, int64_t *n_out, int32_t *overflow, int32_t device_id);

/* pcl::StatisticalOutlierRemoval<PointXYZRGBA>::filter on host points (see orbgpu_cloud_remove_outliers).  cap >= n;
 * mean_dist ([n], may be NULL) receives every point's mean neighbour distance (0 for non-finite points, which stay). */
int orbgpu_statistical_outlier_removal(const orbgpu_point_xyzrgba *in, int64_t n, int32_t mean_k, double stddev_mul,
                                       orbgpu_point_xyzrgba *out, int64_t cap, int64_t *n_out, float *mean_dist,
                                       int32_t device_id);

/* ======================================================================================
 * KeyFrameDatabase  (reference include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc:33-309)
 * ======================================================================================
 * The BoW candidate search that starts relocalisation (Tracking::Relocalization, Tracking.cc:1652) and loop detection
 * (LoopClosing::DetectLoop, LoopClosing.cc:125-142), device-resident and keyed by KeyFrame::mnId.  A key frame is a row
 * with its BoW vector (ascending word ids, double values) and up to 10 neighbour ids (GetBestCovisibilityKeyFrames(10),
 * stored as ids and resolved when a query runs); a query streams all vectors once instead of walking the reference's
 * per-word lists.  Conventions K1-K9: candidates come back in the reference's order, scores are
 * L1Scoring::score's bits.  "vs CPU restatement; DBoW2 boundary unpinned": tests/kfdb_model.py is the restatement.
 *   add             KeyFrameDatabase::add (:40-46; LoopClosing.cc:117 / 147 / 216)
 *   erase           KeyFrameDatabase::erase (:48-67; KeyFrame.cc:582); forgets the key frame's neighbour list
 *   clear           KeyFrameDatabase::clear (:69-73; Tracking.cc:1828); forgets the neighbour lists as well
 *   set_covisibles  hook at the end of KeyFrame::UpdateBestCovisibles; accepts an id that is not in the database (yet):
 *                   the list is kept for when it is added
 *   score           mpORBVocabulary->score(CurrentBowVec, pKF->mBowVec) of LoopClosing.cc:128-139 (NaN for unknown ids)
 *   detect_loop     DetectLoopCandidates (:76-197); connected_ids = pKF->GetConnectedKeyFrames()
 *   detect_reloc    DetectRelocalizationCandidates (:199-309).  The only state a query leaves behind: the score of every
 *                   row it scored (KeyFrame::mRelocScore), which a later reloc query adds for a neighbour it does not
 *                   score itself (:273-276); 0.0f before the first write (uninitialised in the reference).
 * All arrays are HOST arrays.  Refused with ORBGPU_EINVAL, nothing changed and no device needed: an id that is present,
 * word ids not strictly ascending or outside [0, n_words), values that are not finite, more than 10 neighbours or a
 * negative neighbour id, a min_score that is not finite, a scoring type other than 0 (L1_NORM, the ORB vocabulary's).  Erasing an unknown id is ignored and not counted in *known.
 * *n_candidates is always the full count: if `capacity` is smaller the call writes `capacity` ids and still returns
 * ORBGPU_OK.  The device is bound by the first call that computes or stores; without one those calls return ORBGPU_EHIP
 * (no CPU fallback).  A database is used by ONE host thread at a time (KeyFrameDatabaseT serialises); every call returns
 * synchronised.  Limits: 2^24 rows between two clears or compactions (an erased row is dead; rows and pool space come
 * back on clear and on orbgpu_keyframe_db_compact), 2^24 entries per vector, 2^30 entries in all.
 * Compaction (orbgpu_keyframe_db_compact; an edit: host call, one host thread at a time, returns synchronised; it takes the
 * lifecycle lock because it always allocates when it does anything), D1-D4:
 *   D1  rows that were erased are dropped; the live rows stay in add order, each with its BoW vector, its neighbour list,
 *       its add sequence number (K1 orders by it) and its relocalisation score register (K5).
 *   D2  invisible to add, erase, score, detect_loop, detect_reloc, set_covisibles and size: tests/kfdb_model.py has no dead
 *       rows.  The one exception: last_query reports n = 0 after a compact call until the next detect call, as after clear
 *       (its per-row columns describe rows that may be gone; the same after a call that found nothing to drop, so that
 *       the model needs no dead rows to say when).
 *   D3  afterwards row and pool capacity are what the doubling rules give a fresh database with the same creation
 *       arguments once it holds rows_after rows and slots_after entries: the memory comes back.
 *   D4  nothing erased since the last clear or compaction: compacted = 0, no allocation, no device call, also on a handle
 *       that was never bound.  A failure (ORBGPU_ENOMEM, ORBGPU_EHIP) leaves the database bit for bit as it was. */
typedef struct orbgpu_compact_result {
    int32_t compacted;               /* 0: nothing to drop, the handle was not touched */
    int32_t rows_before, rows_after; /* rows of the handle, dead / bad ones included */
    int32_t rows_bad_kept;           /* graph: bad rows kept by C1; database: 0 */
    int32_t row_capacity;
    int64_t slots_before, slots_after, slot_capacity; /* pool entries in use / allocated */
} orbgpu_compact_result;
typedef struct orbgpu_keyframe_db orbgpu_keyframe_db;
int orbgpu_keyframe_db_create(int32_t n_words, int32_t scoring, int32_t device_id, int32_t initial_rows,
                              orbgpu_keyframe_db **out);
int orbgpu_keyframe_db_destroy(orbgpu_keyframe_db *db);
int orbgpu_keyframe_db_clear(orbgpu_keyframe_db *db);
/* Key frames in the database (added and not erased). */
int orbgpu_keyframe_db_size(const orbgpu_keyframe_db *db, int32_t *alive);
int orbgpu_keyframe_db_add(orbgpu_keyframe_db *db, int64_t id, int32_t n_bow, const int32_t *bow_ids, const double *bow_vals);
int orbgpu_keyframe_db_erase(orbgpu_keyframe_db *db, int32_t n, const int64_t *ids, int32_t *known);
int orbgpu_keyframe_db_set_covisibles(orbgpu_keyframe_db *db, int64_t id, int32_t n, const int64_t *neighbour_ids);
int orbgpu_keyframe_db_score(orbgpu_keyframe_db *db, int32_t n_bow, const int32_t *bow_ids, const double *bow_vals, int32_t n,
                             const int64_t *ids, float *scores);
int orbgpu_keyframe_db_detect_loop(orbgpu_keyframe_db *db, int32_t n_bow, const int32_t *bow_ids, const double *bow_vals,
                                   int32_t n_connected, const int64_t *connected_ids, float min_score, int32_t capacity,
                                   int64_t *candidate_ids, int32_t *n_candidates);
int orbgpu_keyframe_db_detect_reloc(orbgpu_keyframe_db *db, int32_t n_bow, const int32_t *bow_ids, const double *bow_vals,
                                    int32_t capacity, int64_t *candidate_ids, int32_t *n_candidates);
/* Tests, debugging: lKFsSharingWords of the most recent detect call, in the reference's order (K1), until the next clear.
 * words = mnLoopWords / mnRelocWords, first_word = the query word at which the row was met, score = NaN for a row that was
 * not scored, acc = NaN and best_id = -1 for a row that did not enter the accumulation.  Any output may be NULL; *n is the
 * full count, at most `capacity` records are written. */
int orbgpu_keyframe_db_last_query(orbgpu_keyframe_db *db, int32_t capacity, int64_t *ids, int32_t *words, int32_t *first_word,
                                  float *score, float *acc, int64_t *best_id, int32_t *n);
/* Tests: how many score launches of this handle read the query from global memory (a query longer than the LDS staging, or
 * ORBGPU_DEBUG_KFDB_LDS_WORDS=<k> in the environment: a query of more than k words takes that path). */
int orbgpu_keyframe_db_debug_global_queries(const orbgpu_keyframe_db *db, int64_t *n);
/* D1-D4 above.  res may be NULL. */
int orbgpu_keyframe_db_compact(orbgpu_keyframe_db *db, orbgpu_compact_result *res);

/* ======================================================================================
 * Observation graph  (Tracking::UpdateLocalMap, Tracking.cc:1499-1643; KeyFrame::UpdateConnections, KeyFrame.cc:327-417;
 *                     LocalMapping::KeyFrameCulling, LocalMapping.cc:632-698)
 * ======================================================================================
 * The relation between key frames and map points, device-resident and keyed by KeyFrame::mnId, and the two votes over
 * it: the frame's map points vote for the key frames that observe them (the local map of Tracking::TrackLocalMap), and a
 * key frame's own points vote for the other key frames (its covisibility weights); and the redundancy test of
 * KeyFrameCulling over the same relation.  Conventions V1-V8; all of it is integer work and the
 * results are equal to tests/covis_model.py's and tests/cull_model.py's, entry for entry.
 *   V1 rows    one row per key frame, n_slots (the frame's N, 0 allowed) fixed at add; the slots lie in one pool,
 *              key-frame-major, one int64 each: the id of the map point at that key-point index, -1 for none.  A row has
 *              a bad flag, a parent id (-1: none), up to 10 best-covisible ids in the caller's order (stored as ids and
 *              resolved when a query runs) and a per-query stamp (mnTrackReferenceForFrame).  Rows are in add order.
 *              A second pool column holds one attribute byte per slot, set once per key frame (set_keypoints): bits 0-3 the
 *              key point's octave (mvKeysUn[idx].octave, below ORBGPU_COVIS_MAX_LEVELS), ORBGPU_COVIS_KP_STEREO if
 *              mvuRight[idx] >= 0 (the observation weighs 2 in MapPoint::nObs, MapPoint.cc:105-108), ORBGPU_COVIS_KP_FAR if
 *              !mbMonocular && (mvDepth[idx] > mThDepth || mvDepth[idx] < 0) (LocalMapping.cc:660-664); bits 4-5 are
 *              reserved and refused.  Every slot of a new row holds 0: octave 0, monocular, close.  Only V8 and
 *              orbgpu_covis_observations read the column; the votes of V5-V7 do not.
 *   V2 one relation   slot (kf, idx) = p stands for both "kf holds p at idx" (KeyFrame::mvpMapPoints) and "p is observed
 *              by kf at idx" (MapPoint::mObservations).  The hooks keep it so: a bad point holds no slot, a bad key frame
 *              holds no slot.  Deviations: the window between AddMapPoint and AddObservation is not represented; a bad key
 *              frame's slots are cleared, where KeyFrame::SetBadFlag leaves mvpMapPoints alone -- the reference would list
 *              the stale points of a bad parent (Tracking.cc:1625-1634 has no isBad test), the library lists none of them
 *              but still appends the bad parent itself; a point that sits in two slots of one row counts twice
 *              (MapPoint::AddObservation's guard excludes that, and the hook goes behind the guard).
 *   V3 children are derived   the children of k are the rows whose parent is k, in ascending id (AddChild / ChangeParent
 *              keep mspChildrens equal to that set).
 *   V4 pointer order unpinned   wherever the reference iterates a std::map<KeyFrame*, ..> or std::set<KeyFrame*> by address,
 *              the library iterates by ascending id.
 *   V5 vote    for a query list q (ids; -1 skipped, duplicates kept), count(row) = sum over the row's slots of the
 *              multiplicity of the slot's id in q: keyframeCounter[it->first]++ per key point.  (Saturates at 2^31 - 1.)
 *   V6 local_map     UpdateLocalKeyFrames + UpdateLocalPoints.  kp_ids: the frame's map point ids per key point, bad ones
 *              already -1 (Tracking.cc:1552).  K1 = the not-bad rows with count > 0 in ascending id, each stamped; ref_kf
 *              = the first of K1 with the strictly greatest count, max_votes that count.  If no row has a vote the
 *              previous list is kept (:1557-1558), its unknown ids skipped and counted, and kept_previous = 1.  Otherwise
 *              the extension runs over the positions of K1 only, in order (:1586-1636); at the top of a step it stops if
 *              the list holds more than 80 entries; then (a) the first stored covisible that is known, not bad and not
 *              stamped is appended and stamped, (b) the first child (V3) that is not bad and not stamped likewise, (c) the
 *              parent, if known and not stamped, is appended and stamped with no bad test, and THE WHOLE EXTENSION ENDS
 *              THERE (the break at :1632 belongs to the outer loop).  Points: over the final list in order, slots in
 *              ascending index, ids >= 0, first occurrence kept.  point_ids is what orbgpu_search_local_points_table takes.
 *   V7 connections   the counting half of UpdateConnections: q = the row's own slots, every other row is counted.  ids /
 *              counts: the full counter in ascending id (mConnectedKeyFrameWeights).  ordered_*: the entries with count >=
 *              th, or -- if there are none but a row was counted -- the single first-strictly-greatest entry, in descending
 *              (weight, id): sort(vPairs) reversed, id standing for the pointer.  An unknown or bad kf gives empty outputs;
 *              the graph is not modified.  AddConnection, mpParent and the set_covisibles / set_parent hooks stay with the
 *              caller (CovisibilityGraphT::UpdateConnections does them).
 *   V8 keyframe_culling   LocalMapping::KeyFrameCulling (LocalMapping.cc:632-698).  kf_ids: GetVectorCovisibleKeyFrames()
 *              of the current key frame, in that order; th_obs: thObs (3 for every sensor in this reference, :647-650).
 *              S is the relation at the start of the call, the weight of a slot is 2 if it is STEREO and 1 otherwise,
 *              Obs_S(p) is the weight sum of p's slots in S (MapPoint::Observations() under V2).  For k = 0 .. n-1 in order:
 *              kf_ids[k] is SKIPPED (verdict -1, n_mps = n_redundant = 0) if it is 0 (:643), no row, a bad row, or got
 *              verdict 1 earlier in this call; an id that was not culled and occurs again is evaluated again.  Otherwise,
 *              over the row's slots that hold a point p still in S: a FAR slot is passed over; else n_mps++, and if
 *              Obs_S(p) > th_obs and at least th_obs slots of S on OTHER rows hold p with octave <= own octave + 1, then
 *              n_redundant++ (every slot counts as an observation -- V2's deviation for a point in two slots of one row --
 *              and all slots of the candidate's own row are excluded).  The candidate is culled iff
 *              (double)n_redundant > 0.9 * (double)n_mps (:695; never with n_mps == 0).  Not culled: verdict 0.  Culled with
 *              not_erase[k] != 0: verdict 2 (mbToBeErased, KeyFrame.cc:497-501), S unchanged.  Otherwise verdict 1: every
 *              slot of the row leaves S and Obs_S(p) drops by the slot's weight; every point that thereby reaches
 *              Obs_S(p) <= 2 is bad (MapPoint.cc:130) and all its slots on every row leave S.  bad_point_ids: those points
 *              in ascending id.  n_query_points: the distinct points in the slots of the candidates that are rows, not bad
 *              and not id 0.  THE GRAPH IS NOT MODIFIED: S lives in per-call scratch; the caller runs
 *              KeyFrame::SetBadFlag on every key frame with verdict 1, whose hooks (set_bad, set_slots, set_parent) bring
 *              the graph to the state the call predicted (CovisibilityGraphT::KeyFrameCulling does).  Deviations: the
 *              reference's early `break` at nObs >= thObs changes no count; a covisible list never holds a bad key frame,
 *              the library skips one; mbNotErase is sampled by the caller before the call, not at each SetBadFlag.
 *   observations   n_obs[i] = Obs(mp_ids[i]) over the rows that are not bad, n_slots[i] = the unweighted number of those
 *              slots; an id of -1 or one held nowhere gives 0, duplicates are allowed.  What MapPointCulling
 *              (LocalMapping.cc:195) and KeyFrame::TrackedMapPoints read.  The graph is not modified.
 * Edits (HOST arrays; every call returns synchronised; ONE host thread at a time -- CovisibilityGraphT serialises):
 *   add_keyframe    mp_ids NULL: every slot empty
 *   set_slots       batched and applied in order (later entries win); mp_id -1 clears a slot; an unknown kf id is ignored,
 *                   *known counts the entries whose key frame is a row; an entry on a bad row is known and changes nothing.
 *                   The hook of AddObservation / EraseObservation / EraseMapPointMatch / ReplaceMapPointMatch; for
 *                   MapPoint::SetBadFlag and Replace pass the observation list those functions hold.
 *   set_bad         sets the flag, clears the row's slots, forgets its covisibles; the row and its parent value stay.
 *                   *known counts the entries whose key frame is a row.
 *   set_parent      the parent may be unknown or -1; for a kf that is no row yet the value is kept until it is added
 *   set_covisibles  orbgpu_keyframe_db_set_covisibles's rule: a list for an id that is no row yet is kept until it is
 *                   added; a bad row ignores the call
 *   set_keypoints   the whole attribute row (V1), once after add_keyframe: key points do not change.  Refused: an unknown
 *                   id, n_slots different from the row's, a byte with bit 4 or 5 set, a null array with n_slots > 0.  A bad
 *                   row ignores the call.
 * keyframe_culling refuses null required outputs, n < 0 or above 2^16, th_obs outside [1, 255] and a negative id;
 * observations refuses ids below -1 and more than 2^20 of them.  Candidates that hold more than 2^20 distinct points
 * return ORBGPU_ECAPACITY (64 bytes of counters per point; a first choice, not a measured limit).
 * Refused with ORBGPU_EINVAL before any device is touched, nothing changed: an id that is present (bad rows included), a
 * negative id, idx outside the row, a map point id below -1, n_slots (or a query) above ORBGPU_COVIS_MAX_SLOTS, more than
 * 10 covisibles, more than 2^20 rows or 2^30 pool slots (first choices, not measured limits).  A local map of more than
 * 2^22 points returns ORBGPU_ECAPACITY.  The rows and the pool space of bad rows come back on clear and on
 * orbgpu_covis_graph_compact (41 bytes per slot once descriptors are set).
 * Compaction (orbgpu_covis_graph_compact; an edit in the sense above; it takes the lifecycle lock because it always
 * allocates when it does anything), C1-C7:
 *   C1 kept rows   every row that is not bad; a bad row if and only if at least one not-bad row's parent value equals its
 *              id (V6(c) appends a known parent with no bad test, so such a row must stay a row).  Kept rows keep their
 *              relative add order; all other bad rows are dropped.
 *   C2 a dropped id is an unknown id from then on, for every call: add_keyframe accepts it again, as a new empty row at the
 *              end; set_bad and set_slots no longer count it in *known; local_map counts it in n_unknown_previous if the
 *              previous list holds it; set_parent and set_covisibles for it go to the pending maps as for any id that is
 *              no row; set_keypoints, set_descriptors refuse it.  Deviation: a later set_parent(live, dropped_id) stores
 *              an unknown parent, which V6(c) does not append -- without compaction the bad row would be appended (the
 *              reference's ChangeParent never hands out a bad parent).  Stored covisible lists and parent values of kept
 *              rows are not rewritten: they are ids, resolved when a query runs.
 *   C3 a kept row is what it was: id, parent, bad, covisibles, descriptor flag, n_slots, centre, stamp and count.  The
 *              slots, attribute bytes and descriptors of a not-bad row are the same bytes at a new offset, the exclusive
 *              prefix sum of n_slots over the kept not-bad rows in order.  A kept bad row owns no pool space afterwards;
 *              its n_slots stays (the refusals of set_slots, set_keypoints and set_descriptors read it), and its pool
 *              offset is a negative value that every reader takes for "no slot": the point gather of V6 does read the
 *              offset of a bad parent it appended and finds all its slots outside the pool, as it found them empty before.
 *   C4 untouched: the pending covisible / parent values of ids that are no rows, the scale factors, the query stamp, the
 *              descriptor column's existence, per-call scratch.
 *   C5 capacities  afterwards row and pool capacity are what the doubling rules give a fresh graph with the same creation
 *              arguments once it holds rows_after rows and slots_after slots: the memory comes back.
 *   C6 nothing to do   no row would be dropped and no kept bad row owns pool space: compacted = 0, no allocation, no
 *              device call, also on a handle that was never bound (all zeros on an empty one).
 *   C7 all or nothing   a failure (ORBGPU_ENOMEM, ORBGPU_EHIP) leaves the graph bit for bit as it was.
 * Counts are always the full ones; at most `capacity` entries of a list are written.  prev_kf_ids and kf_ids may be one
 * array.  Without a device the calls that compute or store return ORBGPU_EHIP (no CPU fallback). */
#define ORBGPU_COVIS_MAX_SLOTS 65536
#define ORBGPU_COVIS_MAX_COVISIBLES 10
typedef struct orbgpu_covis_graph orbgpu_covis_graph;
typedef struct orbgpu_covis_local_map_result {
    int64_t ref_kf;             /* -1: no row has a vote (mpReferenceKF stays) */
    int32_t n_kfs, n_points;    /* full lengths of the two lists */
    int32_t max_votes, n_voted; /* n_voted = |K1| */
    int32_t kept_previous, n_unknown_previous;
} orbgpu_covis_local_map_result;
int orbgpu_covis_graph_create(int32_t device_id, int32_t initial_rows, int64_t initial_slots, orbgpu_covis_graph **out);
int orbgpu_covis_graph_destroy(orbgpu_covis_graph *g);
int orbgpu_covis_graph_clear(orbgpu_covis_graph *g);
/* Rows that are not bad, rows that are. */
int orbgpu_covis_graph_size(const orbgpu_covis_graph *g, int32_t *alive, int32_t *bad);
int orbgpu_covis_graph_add_keyframe(orbgpu_covis_graph *g, int64_t id, int32_t n_slots, const int64_t *mp_ids);
int orbgpu_covis_graph_set_slots(orbgpu_covis_graph *g, int32_t n, const int64_t *kf_ids, const int32_t *idx, const int64_t *mp_ids,
                                 int32_t *known);
int orbgpu_covis_graph_set_bad(orbgpu_covis_graph *g, int32_t n, const int64_t *kf_ids, int32_t *known);
int orbgpu_covis_graph_set_parent(orbgpu_covis_graph *g, int64_t kf_id, int64_t parent_id);
int orbgpu_covis_graph_set_covisibles(orbgpu_covis_graph *g, int64_t kf_id, int32_t n, const int64_t *ids);
int orbgpu_covis_local_map(orbgpu_covis_graph *g, int32_t n_kp, const int64_t *kp_ids, int32_t n_prev, const int64_t *prev_kf_ids,
                           int32_t kf_capacity, int64_t *kf_ids, int32_t point_capacity, int64_t *point_ids,
                           orbgpu_covis_local_map_result *res);
int orbgpu_covis_connections(orbgpu_covis_graph *g, int64_t kf_id, int32_t th, int32_t capacity, int64_t *ids, int32_t *counts,
                             int32_t *n, int32_t ordered_capacity, int64_t *ordered_ids, int32_t *ordered_weights, int32_t *n_ordered);
/* Tests: how many vote launches of this handle read the query from global memory (more distinct ids than the LDS staging
 * holds, or than ORBGPU_DEBUG_COVIS_LDS_IDS=<k>, read when the handle is created). */
int orbgpu_covis_graph_debug_global_queries(const orbgpu_covis_graph *g, int64_t *n);
/* C1-C7 above.  res may be NULL. */
int orbgpu_covis_graph_compact(orbgpu_covis_graph *g, orbgpu_compact_result *res);
#define ORBGPU_COVIS_MAX_LEVELS 16
#define ORBGPU_COVIS_KP_STEREO 0x40
#define ORBGPU_COVIS_KP_FAR 0x80
typedef struct orbgpu_covis_culling_result {
    int32_t n_culled, n_to_be_erased, n_skipped; /* verdicts 1, 2, -1 */
    int32_t n_points_bad;                        /* full length of bad_point_ids */
    int32_t n_query_points;                      /* distinct map points in the candidates' slots */
} orbgpu_covis_culling_result;
int orbgpu_covis_graph_set_keypoints(orbgpu_covis_graph *g, int64_t kf_id, int32_t n_slots, const uint8_t *kp);
int orbgpu_covis_observations(orbgpu_covis_graph *g, int32_t n, const int64_t *mp_ids, int32_t *n_obs, int32_t *n_slots);
/* not_erase NULL: none.  verdict, n_mps, n_redundant: n entries each.  The query of its counting launch goes through LDS or
 * global memory as the vote's does (orbgpu_covis_graph_debug_global_queries counts both). */
int orbgpu_covis_keyframe_culling(orbgpu_covis_graph *g, int32_t n, const int64_t *kf_ids, const uint8_t *not_erase, int32_t th_obs,
                                  int8_t *verdict, int32_t *n_mps, int32_t *n_redundant, int32_t point_capacity,
                                  int64_t *bad_point_ids, orbgpu_covis_culling_result *res);

/* MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:242-307) and MapPoint::UpdateNormalAndDepth (:330-371) for a batch of
 * map points, over the observation graph: the step that ends every chain that edits the map.  Three more columns carry what
 * the two functions read besides the relation itself (edited from HOST arrays, returning synchronised, refusals answered
 * with ORBGPU_EINVAL before any device is touched and with nothing changed):
 *   set_scale_factors   KeyFrame::mvScaleFactors, one table per graph (it is the same for every key frame of a map);
 *                       n_levels in [1, ORBGPU_COVIS_MAX_LEVELS]; may be called again; a value that is not finite or not
 *                       positive is refused.  Held on the host and handed to the kernels by value.
 *   set_descriptors     mDescriptors of one key frame, 32 bytes per slot, once behind add_keyframe.  Refused: an unknown id,
 *                       n_slots different from the row's, a null array with n_slots > 0; a bad row ignores the call.  A third
 *                       pool column beside the slots and the attribute bytes, allocated by the first call of this function
 *                       and not before; from then on the pool grows three columns or none.  The row records that it has
 *                       descriptors.
 *   set_centres         KeyFrame::GetCameraCenter() of n key frames, centres [n][3], applied in order (later entries win);
 *                       the hook of KeyFrame::SetPose and of the bundle adjustments' write-backs.  An unknown id is ignored
 *                       (*known, optional, counts the entries whose key frame is a row), a bad row changes nothing.
 *                       A row column of its own: the centre and a "has centre"
 *                       flag.  set_bad leaves the centre alone.
 *   clear               forgets the contents of all three.
 * Conventions R1-R8; tests/refresh_model.py restates them and is compared bit for bit, floats as
 * their 32-bit patterns.
 *   R1 observations   the observations of p are the slots of rows that are not bad and that hold p (V2), ordered by
 *              ascending key-frame id, then ascending slot index (V4: the reference iterates std::map<KeyFrame*, size_t> by
 *              address).  A point in two slots of one row counts twice (V2's deviation); a bad key frame holds no slot,
 *              which is also what the isBad() test at :265 leaves.
 *   R2 none    no observation: status NO_OBS, everything untouched (:256, :345).
 *   R3 capacity   more than ORBGPU_COVIS_REFRESH_MAX_OBS observations: status OVERFLOW, everything untouched, n_slots still
 *              exact (a first choice, not a measured limit; the reference's float Distances[N][N] on the stack fails long
 *              before).
 *   R4 descriptor   if any observing row has no descriptors: status NO_DESC, descriptor untouched.  Otherwise desc is the
 *              observation's row with the least median Hamming distance to all of them, itself included; the median is the
 *              sorted distance row at index (N - 1) >> 1; the first minimum in R1's order wins
 *              (orbgpu_distinctive_descriptors' rule).  desc_kf / desc_idx name the key frame and key-point index chosen.
 *   R5 normal  if any observing row has no centre: status NO_CENTRE, normal and depth untouched.  Otherwise, per
 *              observation in R1's order and per component: d = P - Ow in float; nrm = sqrt((double)dx * dx + (double)dy *
 *              dy + (double)dz * dz), summed left to right in FP64; inv = (float)(1.0 / nrm); acc = acc + d * inv (two
 *              float roundings, acc starting at 0); finally normal = acc * (float)(1.0 / (double)N).  This restates how
 *              cv::norm and the Mat / double, Mat + Mat * s expressions evaluate for CV_32F; OpenCV is not part of the
 *              reference tree, so the boundary is unpinned and tests/refresh_model.py is the definition.  A zero norm
 *              follows IEEE arithmetic (a NaN normal); it is not a refusal.
 *   R6 depth   ref_kf_ids[i] = mpRefKF->mnId must be a row that is not bad and holds p (the lowest slot index counts if it
 *              holds p twice), level = the octave bits of that slot's attribute byte (V1) must be below n_levels, and a
 *              scale table must be set; otherwise status NO_REF, normal AND depth untouched.  dist = (float)nrm of P -
 *              Ow_ref as in R5; max_dist = dist * sf[level]; min_dist = max_dist / sf[n_levels - 1]: the raw mfMaxDistance /
 *              mfMinDistance, not the 0.8 / 1.2 forms.  Deviation: the reference's observations[pRefKF] default-inserts 0
 *              for a reference key frame that does not observe the point and reads key point 0's octave;
 *              MapPoint::EraseObservation (:111-149) keeps mpRefKF an observer, so the flow never gets there.
 *   R7 independence   the descriptor half (ORBGPU_REFRESH_DESCRIPTOR) and the normal / depth half
 *              (ORBGPU_REFRESH_NORMAL_DEPTH) are independent: a status bit of one leaves the other to run; a half that
 *              `what` leaves out sets no bit and writes nothing.  NO_CENTRE and NO_REF are tested separately (both may be
 *              set).
 *   R8 the graph is not modified, and the result does not depend on scheduling: atomics decide where an entry of an
 *              observation list lands, never the order of its use.
 * refresh_points: mp_ids >= 0 and distinct within a call, at most 2^20 of them; world_pos [n][3].  normal [n][3], min_dist,
 * max_dist, desc [n][32] are in/out (an entry the rules leave untouched keeps the caller's bytes) and may be NULL, as may
 * desc_kf / desc_idx (-1 where the descriptor was left untouched); n_slots (the number of observations) and status are
 * required.  Refused: a null required argument, n < 0 or above 2^20, `what` zero or with other bits, a negative or repeated
 * id.  One wait per call: the observation lists are bounded by the pool slots in use, so their buffer is sized without
 * asking the device (scratch as large as the slot column).
 * orbgpu_mappoint_table_refresh: the same query with the positions gathered from the table's rows on the device and the
 * results written into the table's rows on the device (no orbgpu_mappoint_table_upsert afterwards).  An id the table does
 * not know gives status UNKNOWN, a row flagged bad gives BAD (mbBad returns at :251 / :338); both leave the point untouched
 * (n_slots is still exact).  The host outputs are optional copies of what was written (in/out as above); with all of them
 * NULL only the status bytes, n_slots and the result record come back.  Table and graph must live on one device; each has
 * its own stream, the call synchronises between the gather and the graph's kernels and returns synchronised; THE CALLER
 * SERIALISES BOTH HANDLES for the duration of the call. */
#define ORBGPU_COVIS_REFRESH_MAX_OBS 1024
#define ORBGPU_REFRESH_DESCRIPTOR 1
#define ORBGPU_REFRESH_NORMAL_DEPTH 2
#define ORBGPU_REFRESH_NO_OBS 0x01
#define ORBGPU_REFRESH_OVERFLOW 0x02
#define ORBGPU_REFRESH_NO_DESC 0x04
#define ORBGPU_REFRESH_NO_CENTRE 0x08
#define ORBGPU_REFRESH_NO_REF 0x10
#define ORBGPU_REFRESH_UNKNOWN 0x20
#define ORBGPU_REFRESH_BAD 0x40
typedef struct orbgpu_covis_refresh_result {
    int32_t n_descriptors, n_normals; /* points whose descriptor / whose normal and depth were written */
    int32_t n_no_obs, n_overflow, n_no_desc, n_no_centre, n_no_ref, n_unknown, n_bad; /* points per status bit */
    int32_t max_obs;                  /* the longest observation list (overflowing ones included) */
    int64_t n_entries;                /* entries of all lists that were built */
} orbgpu_covis_refresh_result;
int orbgpu_covis_graph_set_scale_factors(orbgpu_covis_graph *g, int32_t n_levels, const float *scale_factors);
int orbgpu_covis_graph_set_descriptors(orbgpu_covis_graph *g, int64_t kf_id, int32_t n_slots, const uint8_t *desc);
int orbgpu_covis_graph_set_centres(orbgpu_covis_graph *g, int32_t n, const int64_t *kf_ids, const float *centres, int32_t *known);
int orbgpu_covis_refresh_points(orbgpu_covis_graph *g, int32_t n, const int64_t *mp_ids, const int64_t *ref_kf_ids,
                                const float *world_pos, uint32_t what, float *normal, float *min_dist, float *max_dist,
                                uint8_t *desc, int64_t *desc_kf, int32_t *desc_idx, int32_t *n_slots, uint8_t *status,
                                orbgpu_covis_refresh_result *res);
int orbgpu_mappoint_table_refresh(orbgpu_mappoint_table *t, orbgpu_covis_graph *g, int32_t n, const int64_t *mp_ids,
                                  const int64_t *ref_kf_ids, uint32_t what, float *normal, float *min_dist, float *max_dist,
                                  uint8_t *desc, int64_t *desc_kf, int32_t *desc_idx, int32_t *n_slots, uint8_t *status,
                                  orbgpu_covis_refresh_result *res);

/* ======================================================================================
 * On-disk formats of the end-of-run artefacts: host serialisers, byte for byte.
 * ====================================================================================== */
/* Map::_WriteMapPoint (Map.cc:123-130): id (u64) + world position (3 x f32) = 20 bytes. */
size_t orbgpu_mappoint_record_bytes(void);
int orbgpu_write_mappoint_record(uint64_t id, const float *world_pos, uint8_t *out, size_t cap, size_t *written);
/* Map::_WriteKeyFrame (Map.cc:133-183): id (u64), time stamp (f64), translation (3 x f32), rotation as the Eigen
 * quaternion x y z w of Converter::toQuaternion (Converter.cc:137-149, 4 x f32), N (i32), then per key point
 * x, y, size, angle, response (f32), octave (i32), the 32 descriptor bytes and the index of its map point in the
 * file's map-point list (u64, ULONG_MAX = none): 64 bytes per key point.  keys = mvKeys (orbgpu_keypoint records
 * as the extractor writes them). */
size_t orbgpu_keyframe_record_bytes(int32_t n_features);
int orbgpu_write_keyframe_record(uint64_t id, double timestamp, const float *Tcw, int32_t n,
                                 const orbgpu_keypoint *keys, const uint8_t *desc, const uint64_t *mappoint_index,
                                 uint8_t *out, size_t cap, size_t *written);
/* pcl::io::savePCDFileBinary of a PointCloud<PointXYZRGBA> (PointCloudMap.cc:287; PCL 1.7 PCDWriter, header text
 * as recalled -- unpinned): header, then n packed (x, y, z, rgba) records of 16 bytes. */
int orbgpu_pcd_binary_header(int64_t n_points, char *buf, size_t cap, size_t *len);
int orbgpu_write_pcd_binary(const char *path, const orbgpu_point_xyzrgba *points, int64_t n);
/* pcl::io::savePCDFileBinary("optimized_pointcloud.pcd", *globalMap) (PointCloudMap.cc:287): the handle's map as it
 * is (call orbgpu_cloud_remove_outliers first for the reference's shutdown sequence). */
int orbgpu_cloud_save_pcd(orbgpu_cloud *h, const char *path);

#ifdef __cplusplus
}
#endif
#endif /* ORBGPU_H */

"""Crafted key points, depth images and cameras for the device frame glue (k_frame_glue: Frame::UndistortKeyPoints,
Frame::ComputeStereoFromRGBD, Frame::AssignFeaturesToGrid), with a reference in plain numpy that calls neither the
oracle nor the library (test-side helper, shared by test_glue_cases.py on the host and test_gpu_frame_glue.py on the
device).  test_glue_cases.py holds the oracle to this reference and this reference to the hand-worked literals below.

Three geometries:
  A  512 x 384, no distortion, bounds = image: cells of 8 x 8 pixels, inv_w = inv_h = 0.125 exactly;
  B  640 x 480, the TUM1 camera, bounds from the undistorted corners;
  C  512 x 384, no distortion, bounds set by hand to x in [128, 384], y in [96, 288]: inv_w = inv_h = 0.25 exactly,
     and points inside the image fall outside the grid.

A key point is seven floats (x, y, size, angle, response, octave, class_id; the last two are int32)."""
import numpy as np

F32 = np.float32
COLS, ROWS = 64, 48
CELLS = COLS * ROWS
NAN, INF = F32(np.nan), F32(np.inf)
TUM1_K = (517.306408, 516.469215, 318.643040, 255.313989)
TUM1_DIST = (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)


def toward0(x):
    """The next float from x towards zero."""
    return np.nextafter(F32(x), F32(0))


class Cam:
    """A camera as the caller states it; every number is rounded to float once, as orbgpu_camera holds it."""

    def __init__(self, name, w, h, fx, fy, cx, cy, mbf=40.0, dist=(), bounds=None):
        self.name, self.w, self.h = name, w, h
        self.fx, self.fy, self.cx, self.cy, self.mbf = (F32(v) for v in (fx, fy, cx, cy, mbf))
        self.dist = np.zeros(5, F32)
        self.dist[:len(dist)] = dist
        self.hand_bounds = None if bounds is None else tuple(F32(b) for b in bounds)

    def __repr__(self):
        return self.name

    def undistorts(self):
        return self.dist[0] != 0  # the reference's gate, Frame.cc:406: only k1 is looked at

    def bounds(self):
        """(min_x, max_x, min_y, max_y) of Frame::ComputeImageBounds (Frame.cc:436-468), or the hand-set ones."""
        if self.hand_bounds is not None:
            return self.hand_bounds
        if not self.undistorts():
            return F32(0), F32(self.w), F32(0), F32(self.h)
        c = ref_undistort(np.array([[0, 0], [self.w, 0], [0, self.h], [self.w, self.h]], F32), self)
        return min(c[0, 0], c[2, 0]), max(c[1, 0], c[3, 0]), min(c[0, 1], c[1, 1]), max(c[2, 1], c[3, 1])

    def grid_inv(self):
        """mfGridElementWidthInv / HeightInv (Frame.cc:155-156) in float."""
        b = self.bounds()
        return F32(COLS) / (b[1] - b[0]), F32(ROWS) / (b[3] - b[2])

    def on_device(self, gpu):
        """The library's Camera (make_camera computes the bounds itself; hand-set bounds replace them)."""
        cam = gpu.make_camera(float(self.fx), float(self.fy), float(self.cx), float(self.cy), float(self.mbf), self.w,
                              self.h, tuple(float(d) for d in self.dist))
        if self.hand_bounds is not None:
            cam.min_x, cam.max_x, cam.min_y, cam.max_y = (float(b) for b in self.hand_bounds)
        return cam


GEOM_A = Cam("A", 512, 384, 400.0, 400.0, 256.0, 192.0)
GEOM_B = Cam("B_tum1", 640, 480, *TUM1_K, dist=TUM1_DIST)
GEOM_C = Cam("C", 512, 384, 400.0, 400.0, 256.0, 192.0, bounds=(128, 384, 96, 288))


# ---- the reference ----------------------------------------------------------------------------------------------------
def ref_undistort(xy, cam):
    """cv::undistortPoints(xy, xy, K, dist, Mat(), K) of OpenCV 2.4 (cvUndistortPoints): double arithmetic in the order
    of the C source, five fixed-point iterations of the Brown model, reprojection with P = K, one rounding to float."""
    xy = np.asarray(xy, F32).reshape(-1, 2)
    fx, fy, cx, cy = (float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy))
    ifx, ify = 1. / fx, 1. / fy
    k0, k1, k2, k3, k4 = (float(d) for d in cam.dist)
    x = xy[:, 0].astype(np.float64)
    y = xy[:, 1].astype(np.float64)
    x0 = x = (x - cx) * ifx
    y0 = y = (y - cy) * ify
    with np.errstate(all="ignore"):
        for _ in range(5):
            r2 = x * x + y * y
            icdist = (1 + ((0. * r2 + 0.) * r2 + 0.) * r2) / (1 + ((k4 * r2 + k1) * r2 + k0) * r2)
            delta_x = 2 * k2 * x * y + k3 * (r2 + 2 * x * x)
            delta_y = k2 * (r2 + 2 * y * y) + 2 * k3 * x * y
            x = (x0 - delta_x) * icdist
            y = (y0 - delta_y) * icdist
        xx = fx * x + 0. * y + cx
        yy = 0. * x + fy * y + cy
        ww = 1. / (0. * x + 0. * y + 1.)
        return np.stack([xx * ww, yy * ww], 1).astype(F32)


def ref_pos_in_grid(v, min_v, inv):
    """round((v - min) * inv) of Frame::PosInGrid (Frame.cc:382-392) as a float64 array: the product in float, one
    rounding per operation, then roundf -- half away from zero -- done exactly in double."""
    with np.errstate(all="ignore"):
        t = ((np.asarray(v, F32) - F32(min_v)) * F32(inv)).astype(np.float64)
        return np.trunc(t + np.copysign(0.5, t))


def ref_cells(xu, yu, cam):
    """The cell px*ROWS + py of every point, -1 where PosInGrid refuses it."""
    (min_x, _, min_y, _), (inv_w, inv_h) = cam.bounds(), cam.grid_inv()
    px, py = ref_pos_in_grid(xu, min_x, inv_w), ref_pos_in_grid(yu, min_y, inv_h)
    ok = (px >= 0) & (px < COLS) & (py >= 0) & (py < ROWS)  # false for NaN
    return np.where(ok, np.where(ok, px, 0) * ROWS + np.where(ok, py, 0), -1).astype(np.int64)


def ref_grid(xu, yu, cam):
    """Frame::AssignFeaturesToGrid (Frame.cc:230-245) as CSR: (cell_start[CELLS + 1], cell_items[total]), the items of
    a cell in ascending key-point index, which is push_back's order."""
    cell = ref_cells(xu, yu, cam)
    kept = np.nonzero(cell >= 0)[0]
    cell_start = np.zeros(CELLS + 1, np.int32)
    cell_start[1:] = np.cumsum(np.bincount(cell[kept], minlength=CELLS))
    return cell_start, kept[np.argsort(cell[kept], kind="stable")].astype(np.int32)


def ref_stereo(x, y, xu, depth, mbf):
    """Frame::ComputeStereoFromRGBD (Frame.cc:641-662): d = imDepth.at<float>(int(y), int(x)) at the distorted position
    (truncation); where d > 0, mvDepth = d and mvuRight = xu - mbf/d in float, otherwise both are -1."""
    x, y, xu = (np.asarray(a, F32) for a in (x, y, xu))
    d = np.asarray(depth, F32)[np.trunc(y).astype(np.int64), np.trunc(x).astype(np.int64)]
    with np.errstate(all="ignore"):
        hit = d > 0  # false for -0, NaN and negatives; true for denormals and +inf
        ur = np.where(hit, xu - F32(mbf) / d, F32(-1)).astype(F32)
    return ur, np.where(hit, d, F32(-1)).astype(F32)


class Depth:
    """A batch of depth images inside one flat buffer, strides in floats as the entry point takes them."""

    def __init__(self, buf, w, h, stride, frame_stride):
        self.buf, self.w, self.h, self.stride, self.frame_stride = np.ascontiguousarray(buf, F32), w, h, stride, frame_stride

    @classmethod
    def contiguous(cls, planes):
        planes = np.ascontiguousarray(planes, F32)
        b, h, w = planes.shape
        return cls(planes.reshape(-1), w, h, w, w * h)

    def offset(self, f, row, col):
        return f * self.frame_stride + row * self.stride + col

    def plane(self, f):
        """Image f as a contiguous [h][w] copy."""
        o = f * self.frame_stride
        return self.buf[o:o + self.h * self.stride].reshape(self.h, self.stride)[:, :self.w].copy()


class Case:
    def __init__(self, name, cam, kps, n_kp, depth=None):
        self.name, self.cam, self.depth = name, cam, depth
        self.kps = np.ascontiguousarray(kps, F32)
        self.batch, self.cap = self.kps.shape[:2]
        self.n_kp = np.asarray(n_kp, np.int32).reshape(self.batch)

    def __repr__(self):
        return self.name

    def n(self, f):
        """Key points of frame f that count: n_kp clamped to [0, cap]."""
        return int(min(max(int(self.n_kp[f]), 0), self.cap))

    def frames(self, sel):
        """The same case with the frames of `sel` only (depth-free cases)."""
        assert self.depth is None
        return Case("%s[%s]" % (self.name, sel), self.cam, self.kps[sel], self.n_kp[sel])


def ref_frame(case, f):
    """What the glue owes for frame f: mvKeysUn[:n] as raw words, mvuRight[:n], mvDepth[:n] (None without a depth
    image), cell_start and cell_items[:total]."""
    n, cam = case.n(f), case.cam
    k = case.kps[f, :n]
    kun = k.copy()
    if cam.undistorts():
        kun[:, :2] = ref_undistort(k[:, :2], cam)
    ur = dz = None
    if case.depth is not None:
        ur, dz = ref_stereo(k[:, 0], k[:, 1], kun[:, 0], case.depth.plane(f), cam.mbf)
    cell_start, cell_items = ref_grid(kun[:, 0], kun[:, 1], cam)
    return {"n": n, "kps_un": kun, "u_right": ur, "kp_depth": dz, "cell_start": cell_start, "cell_items": cell_items}


def make_kps(xy):
    """[B][cap][7] key points at xy [B][cap][2]; the other five fields differ from row to row, so that a copy from the
    wrong row or a field left out shows."""
    xy = np.asarray(xy, F32)
    b, cap = xy.shape[:2]
    kps = np.zeros((b, cap, 7), F32)
    kps[:, :, :2] = xy
    i = np.arange(b * cap, dtype=np.int64).reshape(b, cap)
    kps[:, :, 2] = 31 + (i % 5)
    kps[:, :, 3] = (i % 1440) * F32(0.25)
    kps[:, :, 4] = i + F32(0.5)
    kps[:, :, 5] = (i % 8).astype(np.int32).view(F32)
    kps[:, :, 6] = (-1 - i).astype(np.int32).view(F32)
    return kps


# ---- hand-worked literals on geometry A -------------------------------------------------------------------------------
# (x, y, column, row), or None for column and row where PosInGrid refuses the point.  v = x * 0.125 is exact, roundf
# rounds half away from zero, and a point is kept iff 0 <= column < 64 and 0 <= row < 48.  100 * 0.125 = 12.5 -> 13.
LITERALS_X = [
    (F32(4), F32(100), 1, 13),             # 0.5 -> 1: away from zero (rintf and np.round say 0)
    (toward0(4), F32(100), 0, 13),         # 0.49999997 -> 0 (adding 0.5 in float would give 1)
    (F32(12), F32(100), 2, 13),            # 1.5 -> 2 under either rule
    (toward0(508), F32(100), 63, 13),      # 63.499996 -> 63
    (F32(508), F32(100), None, None),      # 63.5 -> 64: refused
    (F32(-4), F32(100), None, None),       # -0.5 -> -1: refused
    (toward0(-4), F32(100), 0, 13),        # -0.49999997 -> -0: a negative coordinate that is kept
    (F32(-0.0), F32(100), 0, 13),
    (F32(0), F32(100), 0, 13),
]
LITERALS_Y = [
    (F32(100), F32(4), 13, 1),
    (F32(100), toward0(4), 13, 0),
    (F32(100), F32(12), 13, 2),
    (F32(100), toward0(380), 13, 47),      # 47.499996 -> 47
    (F32(100), F32(380), None, None),      # 47.5 -> 48: refused
    (F32(100), F32(-4), None, None),
    (F32(100), toward0(-4), 13, 0),
    (F32(100), F32(-0.0), 13, 0),
    (F32(100), F32(0), 13, 0),
]
LITERALS_BOTH = [
    (F32(600), F32(500), None, None),      # outside in both axes
    (F32(-10), F32(-10), None, None),
    (toward0(508), toward0(380), 63, 47),  # the last cell
]
LITERALS = LITERALS_X + LITERALS_Y + LITERALS_BOTH

# depth at the looked-up pixel -> (mvuRight - xu, mvDepth) with mbf = 40; None stands for "both are -1"
DEPTH_SPECIALS = [
    (F32(0), None),
    (F32(-0.0), None),
    (F32(-1), None),
    (NAN, None),
    (INF, (F32(0), INF)),                  # 40/inf = 0
    (F32(1e-40), (-INF, F32(1e-40))),      # a denormal is > 0; 40/1e-40 overflows
    (F32(0.5), (F32(-80), F32(0.5))),
    (F32(5), (F32(-8), F32(5))),
]


# ---- case groups ------------------------------------------------------------------------------------------------------
def boundary_case():
    """Group 1: the literals and a seeded sweep that crosses every edge of the grid; no depth image (positions lie
    outside the image, where a depth lookup would be out of bounds)."""
    rng = np.random.default_rng(101)
    sweep = np.stack([rng.uniform(-40, 552, 2000), rng.uniform(-40, 424, 2000)], 1).astype(F32)
    xy = np.concatenate([np.array([(x, y) for x, y, _, _ in LITERALS], F32), sweep])
    return Case("boundaries", GEOM_A, make_kps(xy[None]), [len(xy)])


def out_of_grid_case():
    """Group 2: geometry C with a depth image: every position is inside the image and about half are outside the
    hand-set bounds; the stereo outputs are owed for those as well."""
    rng = np.random.default_rng(102)
    n = 600
    xy = np.stack([rng.uniform(64, 448, n), rng.uniform(48, 336, n)], 1).astype(F32)
    depth = rng.uniform(0.3, 8, (1, GEOM_C.h, GEOM_C.w)).astype(F32)
    depth[rng.random(depth.shape) < 0.2] = 0
    return Case("out_of_grid", GEOM_C, make_kps(xy[None]), [n], Depth.contiguous(depth))


CROWD_CELL, CROWD_N, NEIGHBOUR_N = (20, 10), 512, 100


def crowding_case():
    """Group 3: 512 key points in cell (20, 10), 100 each in (21, 10) and (20, 11), 388 spread over columns >= 25, in a
    seeded random order of indices, so that the order the scatter leaves behind is not the order owed."""
    rng = np.random.default_rng(103)
    n = 1100

    def inside(col, row, m):  # cell (col, row) is x in [8 col - 4, 8 col + 4), y likewise; stay half a pixel inside
        return np.stack([8 * col - 3.5 + rng.random(m) * 7, 8 * row - 3.5 + rng.random(m) * 7], 1)

    rest = n - CROWD_N - 2 * NEIGHBOUR_N
    xy = np.concatenate([inside(*CROWD_CELL, CROWD_N), inside(CROWD_CELL[0] + 1, CROWD_CELL[1], NEIGHBOUR_N),
                         inside(CROWD_CELL[0], CROWD_CELL[1] + 1, NEIGHBOUR_N),
                         np.stack([rng.uniform(200, 500, rest), rng.uniform(10, 370, rest)], 1)])
    xy = xy[rng.permutation(n)].astype(F32)
    return Case("crowding", GEOM_A, make_kps(xy[None]), [n])


COUNTS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 1100, -5, 1300]


def counts_case():
    """Group 4: one launch of eleven frames with cap = 1100 and n_kp on both sides of the wave, of the 1024-thread
    stride and of cap, and outside [0, cap].  Every row holds a valid in-image key point."""
    rng = np.random.default_rng(104)
    b, cap = len(COUNTS), 1100
    xy = np.stack([rng.uniform(0, 511.9, (b, cap)), rng.uniform(0, 383.9, (b, cap))], 2).astype(F32)
    depth = rng.uniform(0.3, 8, (b, GEOM_A.h, GEOM_A.w)).astype(F32)
    depth[rng.random(depth.shape) < 0.2] = 0
    return Case("counts", GEOM_A, make_kps(xy), COUNTS, Depth.contiguous(depth))


def depth_values_case():
    """Group 5: three depth images of 512 x 384 inside a buffer with a row stride of W + 5 and a frame stride of
    (H + 3)(W + 5) + 7.  Every float of the buffer, padding included, is a distinct positive number, so a lookup at any
    other offset changes an output; the special values then go under the first 24 key points of every frame."""
    rng = np.random.default_rng(105)
    cam = GEOM_A
    w, h, b, n = cam.w, cam.h, 3, 64
    stride, frame_stride = w + 5, (h + 3) * (w + 5) + 7
    depth = Depth(1000 + np.arange(b * frame_stride), w, h, stride, frame_stride)  # < 2^24: exact and distinct
    fixed = [(10.99, 20.999998), (w - 0.5, h - 0.5), (0, 0), (w - 0.01, 0.5), (0.25, h - 0.25)]
    taken = {int(y) * w + int(x) for x, y in fixed}
    free = np.array([p for p in rng.permutation(w * h)[:4 * n] if p not in taken])
    xy = np.zeros((b, n, 2), F32)
    for f in range(b):
        pix = free[f * (n - len(fixed)):(f + 1) * (n - len(fixed))]  # distinct pixels: one key point each
        frac = rng.uniform(0, 0.99, (len(pix), 2))
        xy[f] = np.concatenate([np.array(fixed), np.stack([pix % w + frac[:, 0], pix // w + frac[:, 1]], 1)])
        for j in range(24):
            x, y = xy[f, j]
            depth.buf[depth.offset(f, int(y), int(x))] = DEPTH_SPECIALS[(j + f) % len(DEPTH_SPECIALS)][0]
    return Case("depth_values", cam, make_kps(xy), [n] * b, depth)


CAMERAS = [
    GEOM_B,
    Cam("k1_only", 640, 480, 520.0, 520.0, 320.0, 240.0, dist=(0.1,)),
    Cam("strong_barrel", 640, 480, 520.0, 520.0, 320.0, 240.0, dist=(-0.4, 0.2)),
    Cam("fx_ne_fy", 640, 480, 500.0, 380.0, 300.0, 250.0, dist=(0.05, -0.02, 0.001, -0.002, 0.0)),
    # the reference's gate looks at k1 alone (Frame.cc:406): mvKeysUn is a copy although k2 p1 p2 k3 are set
    Cam("gate_quirk", 640, 480, 520.0, 520.0, 320.0, 240.0, dist=(0.0, -0.9, 0.01, 0.01, 1.1)),
]


def camera_case(cam):
    """Group 6: 400 in-image key points and a depth image under one camera."""
    rng = np.random.default_rng(106)
    n = 400
    xy = np.stack([rng.uniform(0, cam.w - 0.1, n), rng.uniform(0, cam.h - 0.1, n)], 1).astype(F32)
    depth = rng.uniform(0.3, 8, (1, cam.h, cam.w)).astype(F32)
    depth[rng.random(depth.shape) < 0.2] = 0
    return Case("camera_" + cam.name, cam, make_kps(xy[None]), [n], Depth.contiguous(depth))


def camera_cases():
    return [camera_case(cam) for cam in CAMERAS]


def batch_case():
    """Group 8: 70 frames of seeded random length in [0, cap] on geometry A, positions across every edge of the grid."""
    rng = np.random.default_rng(108)
    b, cap = 70, 300
    xy = np.stack([rng.uniform(-40, 552, (b, cap)), rng.uniform(-40, 424, (b, cap))], 2).astype(F32)
    return Case("batch", GEOM_A, make_kps(xy), rng.integers(0, cap + 1, b))


# positions whose rounded grid coordinate has no int (NaN, +-inf, beyond 2^31): the reference converts before it tests
# the range, which C leaves undefined and x86 answers with INT_MIN, a refusal.  The library's rule: they have no cell.
NONFINITE = [(NAN, 100), (100, NAN), (NAN, NAN), (INF, 100), (100, -INF), (-INF, INF), (1e30, 100), (100, -1e30),
             (3.5e10, 100)]


def nonfinite_case():
    """Positions that have no cell, every third key point, between ordinary ones; no depth image.  Not part of
    all_cases(): the oracle, like the reference, converts before it tests and leaves these undefined."""
    rng = np.random.default_rng(109)
    n = 3 * len(NONFINITE)
    xy = np.stack([rng.uniform(0, 500, n), rng.uniform(0, 370, n)], 1).astype(F32)
    xy[1::3] = np.array(NONFINITE, F32)
    return Case("nonfinite", GEOM_A, make_kps(xy[None]), [n])


def all_cases():
    return [boundary_case(), out_of_grid_case(), crowding_case(), counts_case(), depth_values_case()] + camera_cases() + [
        batch_case()]

"""The frame-glue cases of glue_cases.py on the host: the numpy reference gives every hand-worked literal, the oracle
gives what the numpy reference gives for every case, and every case's premise holds.  This keeps the expectations that
test_gpu_frame_glue.py holds the device to independent of the device code."""
import numpy as np
import pytest

import glue_cases as G

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in G.all_cases()}


def test_grid_literals():
    """Every literal of geometry A, one point at a time and all at once (the CSR lists each kept point under its
    cell, in index order)."""
    assert G.GEOM_A.bounds() == (0, 512, 0, 384) and G.GEOM_A.grid_inv() == (0.125, 0.125)
    want = np.array([-1 if col is None else col * G.ROWS + row for _, _, col, row in G.LITERALS])
    for (x, y, _, _), cell in zip(G.LITERALS, want):
        assert G.ref_cells([x], [y], G.GEOM_A)[0] == cell, (x, y, cell)
    x, y = (np.array([l[i] for l in G.LITERALS], F32) for i in (0, 1))
    cell_start, cell_items = G.ref_grid(x, y, G.GEOM_A)
    assert cell_start[-1] == (want >= 0).sum() == len(cell_items)
    for c in np.unique(want[want >= 0]):
        assert list(cell_items[cell_start[c]:cell_start[c + 1]]) == list(np.nonzero(want == c)[0])
    # the rule that separates roundf from rint and from a float addition of one half
    assert np.rint(F32(4) * F32(0.125)) == 0 and np.floor(G.toward0(4) * F32(0.125) + F32(0.5)) == 1


def test_hand_set_bounds_reject_in_image_points():
    """Geometry C: inv = 0.25 exactly; x = 126 is column round(-0.5) = -1, x = 127 is column round(-0.25) = 0,
    x = 382 is round(63.5) = 64; the same along y against 48 rows."""
    assert G.GEOM_C.grid_inv() == (0.25, 0.25)
    pts = [(126, 100, -1), (127, 100, 0 * G.ROWS + 1), (382, 100, -1), (381, 100, 63 * G.ROWS + 1), (200, 94, -1),
           (200, 95, 18 * G.ROWS + 0), (200, 286, -1), (200, 285, 18 * G.ROWS + 47)]
    for x, y, cell in pts:
        assert G.ref_cells([x], [y], G.GEOM_C)[0] == cell, (x, y)


def test_depth_literals():
    """The d > 0 rule at every special depth value, with xu = 100.25 and mbf = 40."""
    for d, want in G.DEPTH_SPECIALS:
        ur, dz = G.ref_stereo([3.9], [2.9], [100.25], np.full((3, 4), d, F32), 40.0)
        if want is None:
            assert (ur[0], dz[0]) == (-1, -1), d
        else:
            assert bits(ur)[0] == bits(F32(100.25) + want[0])[0] and bits(dz)[0] == bits(want[1])[0], d
    # truncation, not rounding: (3.9, 2.9) reads pixel [2][3]
    img = np.arange(12, dtype=F32).reshape(3, 4) + 1
    assert G.ref_stereo([3.9], [2.9], [0.0], img, 40.0)[1][0] == img[2, 3]


@pytest.mark.parametrize("case", G.all_cases(), ids=repr)
def test_reference_is_the_oracles_answer(oracle, case):
    cam = case.cam
    (min_x, _, min_y, _), (inv_w, inv_h) = cam.bounds(), cam.grid_inv()
    for f in range(case.batch):
        want = G.ref_frame(case, f)
        n = want["n"]
        k, kun = case.kps[f, :n], want["kps_un"]
        assert np.array_equal(bits(kun[:, 2:]), bits(k[:, 2:]))
        if cam.undistorts():
            oun = oracle.undistort_points(k[:, :2], cam.fx, cam.fy, cam.cx, cam.cy, cam.dist)
            assert np.array_equal(bits(kun[:, :2]), bits(oun))
        else:
            assert np.array_equal(bits(kun), bits(k))
        ocs, oit = oracle.assign_grid(kun[:, 0], kun[:, 1], min_x, min_y, inv_w, inv_h)
        assert np.array_equal(want["cell_start"], ocs) and np.array_equal(want["cell_items"], oit)
        if case.depth is not None:
            our, od = oracle.compute_stereo_from_rgbd(k[:, 0], k[:, 1], kun[:, 0], case.depth.plane(f), float(cam.mbf))
            assert np.array_equal(bits(want["u_right"]), bits(our)) and np.array_equal(bits(want["kp_depth"]), bits(od))


def test_undistortion_is_the_oracles_bit_for_bit(oracle):
    """Far outside the image as well, for every camera (finite results only: no NaN payloads are compared)."""
    pts = np.random.default_rng(0).uniform(-200, 900, (20000, 2)).astype(F32)
    for cam in G.CAMERAS:
        ours = G.ref_undistort(pts, cam)
        theirs = oracle.undistort_points(pts, cam.fx, cam.fy, cam.cx, cam.cy, cam.dist)
        ok = np.isfinite(ours).all(1)
        assert np.array_equal(ok, np.isfinite(theirs).all(1)) and ok.mean() > 0.5, cam
        assert np.array_equal(bits(ours[ok]), bits(theirs[ok])), cam


@pytest.mark.parametrize("cam", G.CAMERAS, ids=repr)
def test_camera_premises(oracle, cam):
    """Bounds as Frame::ComputeImageBounds has them, through the oracle; the undistorted key points are finite and
    have moved; the gate-quirk camera has non-zero coefficients behind a zero k1."""
    case = G.camera_case(cam)
    b = cam.bounds()
    if cam.undistorts():
        c = oracle.undistort_points(np.array([[0, 0], [cam.w, 0], [0, cam.h], [cam.w, cam.h]], F32), cam.fx, cam.fy,
                                    cam.cx, cam.cy, cam.dist)
        assert b == (min(c[0, 0], c[2, 0]), max(c[1, 0], c[3, 0]), min(c[0, 1], c[1, 1]), max(c[2, 1], c[3, 1]))
        assert abs(b[0]) > 1 and abs(b[1] - cam.w) > 1  # the bounds really moved
    else:
        assert b == (0, cam.w, 0, cam.h) and np.any(cam.dist[1:] != 0)
    assert all(np.isfinite(b)) and b[1] > b[0] and b[3] > b[2]
    moved = G.ref_undistort(case.kps[0, :, :2], cam)  # what undistort_points owes, gate or no gate
    assert np.isfinite(moved).all() and np.abs(moved - case.kps[0, :, :2]).max() > 1.0
    kun = G.ref_frame(case, 0)["kps_un"]
    assert np.isfinite(kun[:, :2]).all() and np.array_equal(bits(kun[:, :2]), bits(moved)) == bool(cam.undistorts())


def test_depth_lookups_stay_inside_the_image(cases):
    for case in cases.values():
        if case.depth is None:
            continue
        d = case.depth
        assert d.stride >= d.w and d.frame_stride >= d.h * d.stride or case.batch == 1
        assert len(d.buf) >= (case.batch - 1) * d.frame_stride + (d.h - 1) * d.stride + d.w
        x, y = case.kps[:, :, 0], case.kps[:, :, 1]  # every row, counted or not
        assert np.isfinite(x).all() and np.isfinite(y).all()
        xi, yi = np.trunc(x).astype(np.int64), np.trunc(y).astype(np.int64)
        assert xi.min() >= 0 and xi.max() < d.w and yi.min() >= 0 and yi.max() < d.h, case


def test_crowded_cell_holds_512(cases):
    case = cases["crowding"]
    want = G.ref_frame(case, 0)
    sizes = np.diff(want["cell_start"])
    col, row = G.CROWD_CELL
    assert case.n(0) == 1100 and want["cell_start"][-1] == 1100
    assert sizes[col * G.ROWS + row] == G.CROWD_N == sizes.max() == 512
    assert sizes[(col + 1) * G.ROWS + row] == G.NEIGHBOUR_N and sizes[col * G.ROWS + row + 1] == G.NEIGHBOUR_N
    items = want["cell_items"][want["cell_start"][col * G.ROWS + row]:][:G.CROWD_N]
    assert np.all(np.diff(items) > 0) and np.diff(items).max() > 1  # interleaved with the other cells' indices


def test_out_of_grid_share(cases):
    case = cases["out_of_grid"]
    want = G.ref_frame(case, 0)
    share = 1 - want["cell_start"][-1] / want["n"]
    assert 0.3 <= share <= 0.7, share
    # rejected points still owe their stereo outputs, and some of them have a depth
    rejected = G.ref_cells(want["kps_un"][:, 0], want["kps_un"][:, 1], case.cam) < 0
    assert (want["kp_depth"][rejected] > 0).sum() > 50 and (want["kp_depth"][rejected] == -1).sum() > 10


def test_boundary_sweep_crosses_every_edge(cases):
    case = cases["boundaries"]
    x, y = case.kps[0, :, 0], case.kps[0, :, 1]
    assert case.depth is None and case.n(0) == len(G.LITERALS) + 2000
    assert (x < -4).any() and (x >= 508).any() and (y < -4).any() and (y >= 380).any()
    assert ((x < 0) & (x > -4) & (y > 0) & (y < 380)).any()  # negative and kept


def test_counts_and_batch_premises(cases):
    case = cases["counts"]
    assert list(case.n_kp) == [0, 1, 63, 64, 65, 1023, 1024, 1025, 1100, -5, 1300] and case.cap == 1100
    assert [case.n(f) for f in range(case.batch)] == [0, 1, 63, 64, 65, 1023, 1024, 1025, 1100, 0, 1100]
    assert not G.ref_frame(case, 0)["cell_start"].any() and not G.ref_frame(case, 9)["cell_start"].any()
    case = cases["batch"]
    assert case.batch == 70 and case.n_kp.min() >= 0 and case.n_kp.max() <= case.cap
    assert all(case.n(f) > 0 for f in (0, 37, 69)) and len(set(case.n_kp)) > 40


def test_nonfinite_positions_have_no_cell():
    case = G.nonfinite_case()
    want = G.ref_frame(case, 0)
    cell = G.ref_cells(case.kps[0, :, 0], case.kps[0, :, 1], case.cam)
    assert case.depth is None and np.all(cell[1::3] == -1) and np.all(cell[0::3] >= 0) and np.all(cell[2::3] >= 0)
    assert want["cell_start"][-1] == 2 * len(G.NONFINITE)
    assert not set(want["cell_items"]) & set(range(1, case.cap, 3))


def test_depth_values_premises(cases):
    """Distinct positive padding, strides that differ from the packed ones, every special value under a key point of
    every frame, and the fractional positions of the issue truncating as stated."""
    case = cases["depth_values"]
    d = case.depth
    assert (d.stride, d.frame_stride) == (d.w + 5, (d.h + 3) * (d.w + 5) + 7) and case.batch == 3
    x, y = case.kps[:, :, 0], case.kps[:, :, 1]
    assert (x[0, 0], y[0, 0]) == (F32(10.99), F32(20.999998)) and (int(x[0, 0]), int(y[0, 0])) == (10, 20)
    assert (x[0, 1], y[0, 1]) == (d.w - 0.5, d.h - 0.5)
    off = (np.arange(3)[:, None] * d.frame_stride + np.trunc(y).astype(np.int64) * d.stride + np.trunc(x).astype(np.int64))
    assert len(np.unique(off)) == off.size  # one pixel per key point
    plain = np.ones(len(d.buf), bool)
    plain[off[:, :24].reshape(-1)] = False
    assert len(np.unique(d.buf[plain])) == plain.sum() and d.buf[plain].min() > 0
    for f in range(3):
        seen = d.buf[off[f, :24]]
        for v, _ in G.DEPTH_SPECIALS:
            assert (bits(seen) == bits(v)).sum() == 3, (f, v)
        assert not np.array_equal(d.plane(f), d.plane((f + 1) % 3))

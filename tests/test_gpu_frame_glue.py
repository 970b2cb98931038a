"""The device frame glue (k_frame_glue behind frame_glue_batch_device, k_undistort_points behind undistort_points) on the
crafted cases of glue_cases.py: every output has to equal the numpy reference bit for bit, sentinels have to survive
wherever nothing is owed, and the CSR has to be the one the host entry assign_features_to_grid builds from the same
undistorted points (test_glue_cases.py holds the reference to the oracle and to the hand-worked literals).  No
extractor and no image stream: key points are a [B][cap][7] tensor, the camera is a plain struct."""
import time

import numpy as np
import pytest

import glue_cases as G

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL_F, SENTINEL_I = F32(-12345.5), -77


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def ptr(t):
    return None if t is None else t.data_ptr()


def sentinel_outputs(torch, batch, cap):
    f = dict(dtype=torch.float32, device="cuda")
    i = dict(dtype=torch.int32, device="cuda")
    return {"kps_un": torch.full((batch, cap, 7), float(SENTINEL_F), **f),
            "u_right": torch.full((batch, cap), float(SENTINEL_F), **f),
            "kp_depth": torch.full((batch, cap), float(SENTINEL_F), **f),
            "cell_start": torch.full((batch, G.CELLS + 1), SENTINEL_I, **i),
            "cell_items": torch.full((batch, cap), SENTINEL_I, **i)}


def glue(gpu, torch, case, cam=None, un=True, use_depth=True, stereo=True, batch=None, cap=None, timing=None, out=None):
    """One launch over sentinel-filled outputs (`out`, or fresh ones); returns them as numpy arrays."""
    kps, n_kp = torch.from_numpy(case.kps).cuda(), torch.from_numpy(case.n_kp).cuda()
    d = case.depth if use_depth else None
    depth = None if d is None else torch.from_numpy(d.buf).cuda()
    out = sentinel_outputs(torch, case.batch, case.cap) if out is None else out
    cam = case.cam.on_device(gpu) if cam is None else cam
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gpu.frame_glue_batch_device(case.batch if batch is None else batch, case.cap if cap is None else cap, kps.data_ptr(),
                                n_kp.data_ptr(), ptr(depth), 0 if d is None else d.stride, 0 if d is None else d.frame_stride,
                                cam, ptr(out["kps_un"]) if un else None,
                                ptr(out["u_right"]) if stereo else None, ptr(out["kp_depth"]) if stereo else None,
                                ptr(out["cell_start"]), ptr(out["cell_items"]), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if timing is not None:
        timing.append(time.perf_counter() - t0)
    return {k: v.cpu().numpy() for k, v in out.items()}


def untouched(a):
    return bool(np.all(bits(a) == bits(SENTINEL_F)[0])) if a.dtype == F32 else bool(np.all(a == SENTINEL_I))


def check(gpu, out, case, un=True, stereo=None):
    """Every frame of `out` against the reference, the sentinels, and the host entry's CSR."""
    stereo = case.depth is not None if stereo is None else stereo
    cam = case.cam
    (min_x, _, min_y, _), (inv_w, inv_h) = cam.bounds(), cam.grid_inv()
    for f in range(case.batch):
        want = G.ref_frame(case, f)
        n, total = want["n"], int(want["cell_start"][-1])
        cs, items = out["cell_start"][f], out["cell_items"][f]
        bad = np.nonzero(cs != want["cell_start"])[0]
        print(case, "frame", f, "n", n, "total", total, "device total", cs[-1], "cell_start differs at", bad[:8])
        assert np.array_equal(cs, want["cell_start"]), (case, f)
        assert np.array_equal(items[:total], want["cell_items"]), (case, f, np.nonzero(items[:total] != want["cell_items"])[0][:8])
        if un:
            assert np.array_equal(bits(out["kps_un"][f, :n, :2]), bits(want["kps_un"][:, :2])), (case, f)
            assert np.array_equal(bits(out["kps_un"][f, :n, 2:]), bits(case.kps[f, :n, 2:])), (case, f)  # the input's bytes
            assert untouched(out["kps_un"][f, n:]), (case, f)
        else:
            assert untouched(out["kps_un"][f]), (case, f)
        if stereo:
            assert np.array_equal(bits(out["u_right"][f, :n]), bits(want["u_right"])), (case, f)
            assert np.array_equal(bits(out["kp_depth"][f, :n]), bits(want["kp_depth"])), (case, f)
            assert untouched(out["u_right"][f, n:]) and untouched(out["kp_depth"][f, n:]), (case, f)
        else:
            assert untouched(out["u_right"][f]) and untouched(out["kp_depth"][f]), (case, f)
        # consumers fed by the host entry see the same frame
        src = out["kps_un"][f, :n] if un else case.kps[f, :n]
        hs, hi = gpu.assign_features_to_grid(src[:, 0], src[:, 1], min_x, min_y, inv_w, inv_h)
        assert np.array_equal(cs, hs) and np.array_equal(items[:total], hi), (case, f)


def same_bounds(gpu, cam):
    d = cam.on_device(gpu)
    got = tuple(F32(v) for v in (d.min_x, d.max_x, d.min_y, d.max_y))
    assert bits(got).tolist() == bits(cam.bounds()).tolist(), (cam, got, cam.bounds())


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in G.all_cases()}


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def test_boundaries(gpu, torch, cases):
    """Group 1: the hand-worked literals and the sweep across every edge of the grid, no depth image."""
    case = cases["boundaries"]
    out = glue(gpu, torch, case)
    cs, items = out["cell_start"][0], out["cell_items"][0]
    for i, (x, y, col, row) in enumerate(G.LITERALS):  # the literals themselves, before the reference
        where = np.nonzero(items[:cs[-1]] == i)[0]
        if col is None:
            assert len(where) == 0, (i, x, y)
        else:
            c = col * G.ROWS + row
            assert len(where) == 1 and cs[c] <= where[0] < cs[c + 1], (i, x, y, col, row)
    check(gpu, out, case)


def test_nonfinite_positions_have_no_cell(gpu, torch):
    """NaN, +-inf and positions beyond int's range are refused by the grid (a float-to-int conversion on the device gives
    0 for NaN, which would be column or row 0), by the glue and by the host entry alike; mvKeysUn still copies them."""
    case = G.nonfinite_case()
    out = glue(gpu, torch, case)
    listed = set(out["cell_items"][0, :out["cell_start"][0, -1]].tolist())
    assert not listed & set(range(1, case.cap, 3)), sorted(listed & set(range(1, case.cap, 3)))
    check(gpu, out, case)


def test_out_of_grid_with_depth(gpu, torch, cases):
    """Group 2: hand-set bounds inside the image; the key points the grid refuses still get mvuRight and mvDepth."""
    check(gpu, glue(gpu, torch, cases["out_of_grid"]), cases["out_of_grid"])


def test_crowding(gpu, torch, cases):
    """Group 3: a cell of 512 and two of 100 with interleaved indices: the in-cell order restore at its stated ceiling."""
    case, timing = cases["crowding"], []
    out = glue(gpu, torch, case, timing=timing)
    out2 = glue(gpu, torch, case, timing=timing)
    print("crowding: launch + synchronise %.3f ms first, %.3f ms second" % (timing[0] * 1e3, timing[1] * 1e3))
    check(gpu, out, case)
    assert all(out[k].tobytes() == out2[k].tobytes() for k in ("cell_start", "kps_un"))
    assert out["cell_items"][0, :1100].tobytes() == out2["cell_items"][0, :1100].tobytes()


def test_counts(gpu, torch, cases):
    """Group 4: n_kp of 0, 1, 63..65, 1023..1025, cap, -5 and cap + 200 in one launch; rows at and beyond the clamped
    n keep their sentinels and an empty frame has an all-zero cell_start."""
    case = cases["counts"]
    out = glue(gpu, torch, case)
    for f in (0, 9):
        assert not out["cell_start"][f].any() and untouched(out["u_right"][f]) and untouched(out["kps_un"][f])
    assert out["cell_start"][10, -1] > 1000 and not untouched(out["u_right"][10, -1:])
    check(gpu, out, case)


def test_depth_values_and_strides(gpu, torch, cases):
    """Group 5: 0, -0, -1, NaN, +inf, a denormal, 0.5 and 5 under truncated fractional positions, in a padded buffer
    whose every float is distinct."""
    check(gpu, glue(gpu, torch, cases["depth_values"]), cases["depth_values"])


@pytest.mark.parametrize("cam", G.CAMERAS, ids=repr)
def test_cameras(gpu, torch, cases, cam):
    """Group 6: TUM1, k1 alone, a strong barrel, fx != fy, and k1 == 0 in front of non-zero coefficients (mvKeysUn is
    then a copy and the grid uses the distorted positions, while undistort_points still moves the points)."""
    case = cases["camera_" + cam.name]
    same_bounds(gpu, cam)
    out = glue(gpu, torch, case)
    check(gpu, out, case)
    if not cam.undistorts():
        assert np.array_equal(bits(out["kps_un"][0]), bits(case.kps[0]))
    xy = case.kps[0, :, :2]
    moved = gpu.undistort_points(xy, cam.on_device(gpu))
    assert np.array_equal(bits(moved), bits(G.ref_undistort(xy, cam))) and np.abs(moved - xy).max() > 1.0
    wide = np.random.default_rng(0).uniform(-200, 900, (5000, 2)).astype(F32)
    got, want = gpu.undistort_points(wide, cam.on_device(gpu)), G.ref_undistort(wide, cam)
    ok = np.isfinite(want).all(1)
    assert np.array_equal(ok, np.isfinite(got).all(1)) and np.array_equal(bits(got[ok]), bits(want[ok]))


def test_bounds_of_the_plain_geometries(gpu):
    for cam in (G.GEOM_A, G.GEOM_C):
        same_bounds(gpu, cam)


def test_optional_outputs(gpu, torch, cases):
    """Group 7: without a depth image the stereo outputs are left alone; without mvKeysUn (no distortion) the grid
    is the same one."""
    case = cases["out_of_grid"]
    full = glue(gpu, torch, case)
    no_depth = glue(gpu, torch, case, use_depth=False)
    check(gpu, no_depth, case, stereo=False)
    no_un = glue(gpu, torch, case, un=False)
    check(gpu, no_un, case, un=False)
    neither = glue(gpu, torch, case, un=False, use_depth=False, stereo=False)
    check(gpu, neither, case, un=False, stereo=False)
    total = full["cell_start"][0, -1]
    for other in (no_depth, no_un, neither):
        assert np.array_equal(other["cell_start"], full["cell_start"])
        assert np.array_equal(other["cell_items"][0, :total], full["cell_items"][0, :total])
    assert np.array_equal(bits(no_un["u_right"]), bits(full["u_right"]))


def test_refused_arguments_launch_nothing(gpu, torch, cases):
    """Group 7: distortion without mvKeysUn, depth without stereo outputs, empty bounds, batch or cap < 1: EINVAL, and
    every output keeps its sentinels."""
    tum = cases["camera_B_tum1"]
    plain = cases["out_of_grid"]
    empty_x, empty_y = plain.cam.on_device(gpu), plain.cam.on_device(gpu)
    empty_x.max_x = empty_x.min_x
    empty_y.min_y = empty_y.max_y + 1
    refused = [(tum, dict(un=False)), (plain, dict(stereo=False)), (plain, dict(cam=empty_x)), (plain, dict(cam=empty_y)),
               (plain, dict(batch=0)), (plain, dict(cap=0)), (plain, dict(batch=-1))]
    for case, how in refused:
        out = sentinel_outputs(torch, case.batch, case.cap)
        with pytest.raises(gpu.OrbGpuError) as ei:
            glue(gpu, torch, case, out=out, **how)
        assert ei.value.status == gpu.EINVAL, how
        torch.cuda.synchronize()
        assert all(untouched(v.cpu().numpy()) for v in out.values()), how


def test_batch_independence_and_determinism(gpu, torch, cases):
    """Group 8: 70 frames of random length; frames 0, 37 and 69 give the same bytes alone as inside the batch, and two
    runs of the batch give identical bytes up to cell_start's total (the order the atomics ran in must not show)."""
    case = cases["batch"]
    first, second = glue(gpu, torch, case), glue(gpu, torch, case)
    check(gpu, first, case)

    def owed(out, f, n):  # everything that is owed, sentinels included; cell_items only up to the total
        total = out["cell_start"][f, -1]
        return (out["cell_start"][f].tobytes(), out["cell_items"][f, :total].tobytes(), out["kps_un"][f].tobytes(),
                out["u_right"][f].tobytes(), out["kp_depth"][f].tobytes())

    for f in range(case.batch):
        assert owed(first, f, case.n(f)) == owed(second, f, case.n(f)), f
    for f in (0, 37, 69):
        alone = glue(gpu, torch, case.frames([f]))
        assert owed(alone, 0, case.n(f)) == owed(first, f, case.n(f)), f

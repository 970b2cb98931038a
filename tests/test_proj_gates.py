"""The hand-worked gate cases of the projection matchers (proj_gate_cases.py) against the oracle, on the host: the
oracle has to give the literal expectation of every case, which keeps the expectations independent of the device code
that test_gpu_proj_gates.py holds to them."""
import numpy as np
import pytest

import proj_gate_cases as G


@pytest.mark.parametrize("case", G.local_cases(), ids=repr)
def test_local_case_literal_is_the_oracles_answer(oracle, case):
    frame = G.make_frame(oracle, case.kps)
    n, k2m = oracle.search_by_projection(frame, G.make_mp(case.rows), case.th, case.nnratio, case.k0)
    assert n >= 0
    assert np.array_equal(k2m, case.expect), (np.nonzero(k2m != case.expect)[0][:8], k2m[k2m != case.expect][:8])


def test_key_width_case_crowds_an_even_cell():
    """The premise of the key-width case: the crowded cell is an even number of the window and holds position 4096,
    whose bit 12 would fall on the lowest bit of the cell number; the lone key point's cell is the next one."""
    for swapped in (False, True):
        c = G.key_width_case(swapped)
        x, y, level = c.rows[0][:3]
        r = float(np.float32(4.0) * G.SF[level])
        crowd = G.window_cell_number(x, y, r, *c.kps[1][:2])
        lone = G.window_cell_number(x, y, r, *c.kps[0][:2])
        assert len(c.kps) == 4098 and (crowd, lone) == ((5, 4) if swapped else (4, 5))
        assert sum(1 for k in c.kps if k[:2] == c.kps[1][:2]) == 4097


def test_frustum_rows_literal_is_the_oracles_answer(oracle):
    rows = G.frustum_rows()
    in_view, nbad, trk = G.frustum_expected()
    for i, (name, pos, normal, mn, mx, skip, _obs, _e) in enumerate(rows):
        if skip:
            continue
        ok, px, py, pxr, lvl, vc = oracle.is_in_frustum(G.TCW, G.FX, G.FY, G.CX, G.CY, G.MBF, G.W, G.H, pos, normal,
                                                        float(mn), float(mx), G.LOG_SF)
        level_ok = 0 <= lvl < G.NLEVELS
        assert (ok and level_ok) == bool(in_view[i]), (name, ok, lvl)
        if in_view[i]:
            got = np.array([px, py, pxr, vc], np.float32)
            want = np.array([trk[k][i] for k in ("proj_x", "proj_y", "proj_xr", "view_cos")], np.float32)
            assert got.tobytes() == want.tobytes() and lvl == trk["level"][i], (name, got, want, lvl)
        elif _e == G.BAD:
            assert ok and not level_ok, (name, ok, lvl)  # reached PredictScale: a counted row
        else:
            assert not ok, name
    frame = G.make_frame(oracle, G.FRUSTUM_KPS)
    n, k2m, iv, nlo = oracle.search_local_points(frame, G.TCW, G.FX, G.FY, G.CX, G.CY, G.MBF, G.frustum_table(), G.LOG_SF,
                                                 th=G.FRUSTUM_TH, nnratio=G.FRUSTUM_NNRATIO)
    assert np.array_equal(iv, in_view) and nlo == nbad
    assert n == G.FRUSTUM_NMATCHES and np.array_equal(k2m, G.FRUSTUM_KP_TO_MP)


def test_non_finite_level_is_out_of_range_not_a_conversion(oracle):
    """A NaN or infinite predicted level is reported as INT_MIN / INT_MAX by an explicit test of the float."""
    lo, hi = -2 ** 31, 2 ** 31 - 1
    for pos, mn, mx, want in (((G.NAN, 0, 2), 0.5, 3.0, lo), (G.A, 0.5, float("nan"), lo), ((0, 0, 0), 0.0, 3.0, hi)):
        ok, *_rest, lvl, _vc = oracle.is_in_frustum(G.TCW, G.FX, G.FY, G.CX, G.CY, G.MBF, G.W, G.H, pos, G.TOWARDS, mn, mx,
                                                    G.LOG_SF)
        assert ok and lvl == want, (pos, mx, lvl)


def test_frustum_batch_slices_literal_is_the_oracles_answer(oracle):
    t = G.frustum_table()
    frame = G.make_frame(oracle, G.FRUSTUM_KPS)
    assert sum(len(t["skip"][sl]) for sl, *_ in G.FRUSTUM_BATCH) == len(t["skip"])
    for sl, k2m_want, n_want, bad_want in G.FRUSTUM_BATCH:
        n, k2m, _iv, nlo = oracle.search_local_points(frame, G.TCW, G.FX, G.FY, G.CX, G.CY, G.MBF,
                                                      {k: v[sl] for k, v in t.items()}, G.LOG_SF, th=G.FRUSTUM_TH,
                                                      nnratio=G.FRUSTUM_NNRATIO)
        assert (n, nlo) == (n_want, bad_want) and np.array_equal(k2m, k2m_want), sl


@pytest.mark.parametrize("factor", [1.2, 2.0])
def test_sweep_straddles_every_level(oracle, factor):
    """The PredictScale sweep does what it is for: on the axis rows, both sides of every threshold factor^k occur."""
    t = G.sweep_table(factor, n_axis=17 * 8 * 40, n_random=0)
    log_sf = float(np.log(np.float32(factor)))
    lv = np.array([oracle.is_in_frustum(G.TCW, G.FX, G.FY, G.CX, G.CY, G.MBF, G.W, G.H, t["world_pos"][i], t["normal"][i],
                                        0.0, float(t["max_dist"][i]), log_sf)[4] for i in range(len(t["max_dist"]))])
    lv = lv.reshape(40, 8, 17)
    for k in range(8):
        assert np.all(lv[:, k, 0] == k) and np.all(lv[:, k, 16] == k + 1), k  # 8 floats below / above the threshold
        assert np.all(np.diff(lv[:, k, :], axis=1) >= 0)


def test_key_width_point_projects_onto_the_cases_row(oracle):
    t = G.KEY_WIDTH_POINT
    ok, px, py, _pxr, lvl, vc = oracle.is_in_frustum(G.TCW, G.FX, G.FY, G.CX, G.CY, G.MBF, G.W, G.H, t["world_pos"][0],
                                                     t["normal"][0], 0.5, 2.5, G.LOG_SF)
    x, y, level = G.key_width_case(False).rows[0][:3]
    assert ok and (px, py, lvl) == (x, y, level) and vc < 0.998
    for swapped in (False, True):
        c = G.key_width_case(swapped)
        n, k2m, iv, nlo = oracle.search_local_points(G.make_frame(oracle, c.kps), G.TCW, G.FX, G.FY, G.CX, G.CY, G.MBF, t,
                                                     G.LOG_SF, th=1.0, nnratio=0.8)
        assert n == 1 and nlo == 0 and np.array_equal(k2m, c.expect)


@pytest.mark.parametrize("motion", list(G.LAST_MOTIONS))
def test_last_frame_case_literal_is_the_oracles_answer(oracle, motion):
    kps, last, expect = G.last_case(motion)
    n, k2m = oracle.search_by_projection_last(G.make_frame(oracle, kps), G.TCW, G.FX, G.FY, G.CX, G.CY, G.MBF, G.MB, last,
                                              G.LAST_TH, False, True, np.full(len(kps), -1, np.int32))
    assert np.array_equal(k2m, expect) and n == int((expect >= 0).sum())


def test_fuse_case_literal_is_the_oracles_answer(oracle):
    kps, pts, gated, ungated = G.fuse_case()
    frame = G.make_frame(oracle, kps)
    S = np.eye(4, dtype=np.float32)
    n, best = oracle.fuse(frame, G.TCW, G.FX, G.FY, G.CX, G.CY, G.MBF, G.LOG_SF, pts, G.FUSE_TH, G.INV_SIGMA2)
    assert np.array_equal(best, gated) and n == 3
    n, best = oracle.fuse_sim3(frame, S, G.FX, G.FY, G.CX, G.CY, G.LOG_SF, pts, G.FUSE_TH)
    assert np.array_equal(best, ungated) and n == 5
    n, k2m = oracle.search_by_projection_sim3(frame, S, G.FX, G.FY, G.CX, G.CY, G.LOG_SF, pts, int(G.FUSE_TH),
                                              np.full(len(kps), -1, np.int32))
    assert np.array_equal(k2m, ungated) and n == 5  # point i takes key point i here, so both read the same


def test_keyframe_and_initialization_literals_are_the_oracles_answer(oracle):
    kps, kf, expect = G.keyframe_case()
    n, k2m = oracle.search_by_projection_keyframe(G.make_frame(oracle, kps), G.TCW, G.FX, G.FY, G.CX, G.CY, G.LOG_SF, kf,
                                                  3.0, G.ORB_DIST, True, np.full(len(kps), -1, np.int32))
    assert np.array_equal(k2m, expect) and n == 1
    f1, f2, prev, m12 = G.init_case()
    n, out, pm = oracle.search_for_initialization(G.make_frame(oracle, f1), G.make_frame(oracle, f2), prev, G.INIT_WINDOW,
                                                  G.INIT_NNRATIO, False)
    assert np.array_equal(out, m12) and n == int((m12 >= 0).sum())


@pytest.mark.parametrize("swapped", [False, True])
def test_key_width_through_initialization_literal_is_the_oracles_answer(oracle, swapped):
    f1, f2, prev, m12 = G.init_key_width_case(swapped)
    n, out, _pm = oracle.search_for_initialization(G.make_frame(oracle, f1), G.make_frame(oracle, f2), prev, 5,
                                                   G.INIT_NNRATIO, False)
    assert n == 1 and np.array_equal(out, m12)


def test_sim3_pair_literal_is_the_oracles_answer(oracle):
    kps, pts, already1, plain, skipped = G.sim3_pair_case()
    f, eye4, eye3, zero3 = G.make_frame(oracle, kps), np.eye(4, dtype=np.float32), np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    for already, want in ((None, plain), (already1, skipped)):
        n, m12 = oracle.search_by_sim3(f, f, eye4, eye4, 1.0, eye3, zero3, G.FX, G.FY, G.CX, G.CY, G.LOG_SF, G.LOG_SF, pts,
                                       already, pts, None, G.FUSE_TH)
        assert np.array_equal(m12, want) and n == int((want >= 0).sum())

"""The projection matchers' device gates on the hand-worked cases of proj_gate_cases.py: every flavour that can express
a case has to give the case's literal expectation exactly (test_proj_gates.py holds the oracle to the same literals)."""
import numpy as np
import pytest

import proj_gate_cases as G

pytestmark = pytest.mark.gpu

SENTINEL_F, SENTINEL_I, SENTINEL_B = np.float32(-12345.5), -77, 9


def table_for(gpu, case):
    """The rows of a local-map case in a MapPoint table (ids 1000 + row; 999 is an observed point outside the list, what
    a key point's -2 stands for) and the frame's associations as ids."""
    mp = G.make_mp(case.rows)
    m = len(case.rows)
    ids = np.arange(1000, 1000 + m, dtype=np.int64)
    tbl = gpu.MapPointTable(initial_rows=16)
    z3 = np.zeros((m, 3), np.float32)
    tbl.upsert(ids, z3, z3, np.zeros(m, np.float32), np.zeros(m, np.float32), mp["desc"], mp["obs_pos"].astype(np.int32))
    tbl.upsert(np.array([999], np.int64), n_obs=np.array([1], np.int32))
    if mp["bad"].any():
        assert tbl.set_bad(ids[mp["bad"] != 0]) == int(mp["bad"].sum())
    kp_ids = np.where(case.k0 == -2, 999, np.where(case.k0 >= 0, ids[np.maximum(case.k0, 0)], -1)).astype(np.int64)
    return tbl, ids, mp, kp_ids


@pytest.mark.parametrize("case", G.local_cases(), ids=repr)
def test_local_case_on_the_device(gpu, case):
    """Host-built queries (SearchByProjection: k_proj_lists, k_proj_resolve) and the table's scratch flavour
    (k_scratch_queries in front of the same two) give the literal expectation; the host flavour also reports whether
    pass 2 had to walk a row again, which the decision-depth and key-width cases pin."""
    frame = G.make_frame(gpu, case.kps)
    mp = G.make_mp(case.rows)
    n, k2m = gpu.ORBmatcher(case.nnratio).SearchByProjection(frame, mp, case.th, case.k0)
    sweeps, rewalked = gpu.projection_last_sweeps()
    print(case, "host flavour:", n, "matches, differing key points", np.nonzero(k2m != case.expect)[0][:8],
          k2m[k2m != case.expect][:8], "sweeps", sweeps, "rewalked", rewalked)
    assert np.array_equal(k2m, case.expect)
    if case.rewalk is not None:
        assert (rewalked > 0) == case.rewalk, (sweeps, rewalked)
    tbl, ids, mp, kp_ids = table_for(gpu, case)
    dfr = gpu.DeviceFrame().upload(frame)
    n2, k2 = gpu.search_local_points_table(dfr, tbl, ids, None, G.FX, G.FY, G.CX, G.CY, G.MBF, G.LOG_SF, case.th,
                                           case.nnratio, scratch=mp, kp_ids=kp_ids)
    print(case, "scratch flavour:", n2, "matches, differing key points", np.nonzero(k2 != case.expect)[0][:8])
    assert np.array_equal(k2, case.expect) and n2 == n


def test_caller_filled_level_out_of_range_is_refused(gpu):
    """A caller-filled level of -1 or nlevels: the host flavour names the row with ELEVEL, and the table's scratch flavour
    (k_scratch_queries counts the row and leaves it inactive) reports the count with ELEVEL as well."""
    case = G.LocalCase("bad_levels", [G.kp(100, 100), G.kp(200, 100, 7), G.kp(300, 100)],
                       [G.row(100, 100, -1), G.row(200, 100, G.NLEVELS), G.row(300, 100, 0)], [-1, -1, 2])
    frame = G.make_frame(gpu, case.kps)
    dfr = gpu.DeviceFrame().upload(frame)
    for bad_row in (0, 1):
        sub = G.LocalCase("bad_level_row", case.kps, [case.rows[2], case.rows[bad_row]], [-1, -1, 0])
        with pytest.raises(gpu.OrbGpuError) as ei:
            gpu.ORBmatcher(0.8).SearchByProjection(frame, G.make_mp(sub.rows), 1.0, sub.k0)
        assert ei.value.status == gpu.ELEVEL and "map point 1:" in str(ei.value)
        tbl, ids, mp, kp_ids = table_for(gpu, sub)
        with pytest.raises(gpu.OrbGpuError) as ei:
            gpu.search_local_points_table(dfr, tbl, ids, None, G.FX, G.FY, G.CX, G.CY, G.MBF, G.LOG_SF, 1.0, 0.8, scratch=mp,
                                          kp_ids=kp_ids)
        assert ei.value.status == gpu.ELEVEL and "1 map point(s)" in str(ei.value)


# ---- device query builders -----------------------------------------------------------------------------------------
def sentinel_track(gpu, torch, m):
    """A track scratch of m rows on the device, every entry a sentinel.  Returns (tensors, TrackScratch)."""
    trk = {"in_view": torch.full((m,), SENTINEL_B, dtype=torch.uint8, device="cuda"),
           "level": torch.full((m,), SENTINEL_I, dtype=torch.int32, device="cuda")}
    for k in ("proj_x", "proj_y", "proj_xr", "view_cos"):
        trk[k] = torch.full((m,), float(SENTINEL_F), dtype=torch.float32, device="cuda")
    ts = gpu.TrackScratch()
    for k in trk:
        setattr(ts, k, trk[k].data_ptr())
    return trk, ts


def device_frustum(gpu, frame, table, log_sf, th, nnratio):
    """search_local_points_device (k_frustum_queries) over device arrays with the track scratch pre-filled with
    sentinels.  Returns (kp_to_mp, counts, track)."""
    torch = pytest.importorskip("torch")
    m = len(table["min_dist"])
    dfr = gpu.DeviceFrame().upload(frame)
    fv, n = dfr.device_view()
    dev = {k: torch.from_numpy(np.ascontiguousarray(table[k])).cuda() for k in
           ("world_pos", "normal", "min_dist", "max_dist", "desc", "skip", "obs_pos")}
    tb = gpu.DeviceMapPointTable()
    tb.m = m
    for k in dev:
        setattr(tb, k, dev[k].data_ptr())
    trk, ts = sentinel_track(gpu, torch, m)
    k2m = torch.full((max(fv.cap, 1),), -1, dtype=torch.int32, device="cuda")
    counts = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    gpu.search_local_points_device(fv, tb, G.TCW, G.FX, G.FY, G.CX, G.CY, G.MBF, log_sf, th, nnratio, k2m.data_ptr(),
                                   counts.data_ptr(), ts, stream=s)
    torch.cuda.synchronize()
    del dfr
    return k2m.cpu().numpy()[:n], counts.cpu().numpy(), {k: v.cpu().numpy() for k, v in trk.items()}


def check_track(trk, in_view, want):
    """in_view everywhere; the scratch bit for bit on the in-view rows, and as it was on the others."""
    print("in_view", trk["in_view"], "\nlevel", trk["level"], "\nproj_x", trk["proj_x"])
    assert np.array_equal(trk["in_view"], in_view)
    on = in_view != 0
    for k in ("proj_x", "proj_y", "proj_xr", "view_cos", "level"):
        assert trk[k][on].tobytes() == want[k][on].tobytes(), (k, trk[k][on], want[k][on])
        left = SENTINEL_I if k == "level" else SENTINEL_F
        assert np.all(trk[k][~on] == left), (k, trk[k][~on])


def test_frustum_builder_on_hand_worked_rows(gpu):
    """k_frustum_queries row by row: image bounds, distance range and viewing cosine on their thresholds, levels out of
    range, and positions and distances that are not numbers, which are levels out of range: counted, not in view."""
    in_view, nbad, want = G.frustum_expected()
    frame = G.make_frame(gpu, G.FRUSTUM_KPS)
    k2m, counts, trk = device_frustum(gpu, frame, G.frustum_table(), G.LOG_SF, G.FRUSTUM_TH, G.FRUSTUM_NNRATIO)
    print("counts", counts, "kp_to_mp", k2m)
    check_track(trk, in_view, want)
    assert counts[1] == nbad
    assert counts[0] == G.FRUSTUM_NMATCHES and np.array_equal(k2m, G.FRUSTUM_KP_TO_MP)


@pytest.mark.parametrize("swapped", [False, True])
def test_key_width_through_the_device_builder(gpu, swapped):
    """The key-width case with its row built on the device (k_frustum_queries) from a map point that projects onto it."""
    case = G.key_width_case(swapped)
    k2m, counts, trk = device_frustum(gpu, G.make_frame(gpu, case.kps), G.KEY_WIDTH_POINT, G.LOG_SF, 1.0, 0.8)
    print(case, "counts", counts, "held key points", np.nonzero(k2m >= 0)[0], "track", {k: v[0] for k, v in trk.items()})
    assert trk["in_view"][0] == 1 and (trk["proj_x"][0], trk["proj_y"][0], trk["level"][0]) == (103.0, 103.0, 1)
    assert counts[0] == 1 and counts[1] == 0 and np.array_equal(k2m, case.expect)


def test_frustum_builder_over_the_table_and_batched(gpu):
    """The same rows through search_local_points_table (isInFrustum on the device) and spread over three problems of
    different m in one search_local_points_batch_device call (k_frustum_queries_batch), each with a track scratch of its
    own that is held to the same bits and sentinels."""
    torch = pytest.importorskip("torch")
    in_view, nbad, want = G.frustum_expected()
    t = G.frustum_table()
    m = len(in_view)
    frame = G.make_frame(gpu, G.FRUSTUM_KPS)
    dfr = gpu.DeviceFrame().upload(frame)
    ids = np.arange(5000, 5000 + m, dtype=np.int64)
    tbl = gpu.MapPointTable(initial_rows=16)
    tbl.upsert(ids, t["world_pos"], t["normal"], t["min_dist"], t["max_dist"], t["desc"], t["obs_pos"].astype(np.int32))
    n, k2m, trk = gpu.search_local_points_table(dfr, tbl, ids, G.TCW, G.FX, G.FY, G.CX, G.CY, G.MBF, G.LOG_SF, G.FRUSTUM_TH,
                                                G.FRUSTUM_NNRATIO, skip=t["skip"], want_track=True)
    assert np.array_equal(trk["in_view"], in_view)
    on = in_view != 0
    for k in ("proj_x", "proj_y", "proj_xr", "view_cos", "level"):
        assert trk[k][on].tobytes() == want[k][on].tobytes(), k
    assert n == G.FRUSTUM_NMATCHES and np.array_equal(k2m, G.FRUSTUM_KP_TO_MP)
    # batched: one frame, three slices of the rows
    fv, nkp = dfr.device_view()
    keep, problems = [], []
    for sl, _k2m, _n, _bad in G.FRUSTUM_BATCH:
        dev = {k: torch.from_numpy(np.ascontiguousarray(t[k][sl])).cuda() for k in
               ("world_pos", "normal", "min_dist", "max_dist", "desc", "skip", "obs_pos")}
        tb = gpu.DeviceMapPointTable()
        tb.m = len(dev["min_dist"])
        for k in dev:
            setattr(tb, k, dev[k].data_ptr())
        out = torch.full((max(fv.cap, 1),), -1, dtype=torch.int32, device="cuda")
        cnt = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        trk_d, ts = sentinel_track(gpu, torch, tb.m)
        keep.append((dev, tb, out, cnt, trk_d, ts))
        problems.append({"frame": fv, "table": tb, "Tcw": G.TCW, "fx": G.FX, "fy": G.FY, "cx": G.CX, "cy": G.CY,
                         "mbf": G.MBF, "log_sf": G.LOG_SF, "d_kp_to_mp": out.data_ptr(), "d_counts": cnt.data_ptr(),
                         "track": ts})
    gpu.search_local_points_batch_device(problems, 0.5, G.FRUSTUM_TH, G.FRUSTUM_NNRATIO,
                                         stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for (sl, want_k2m, want_n, want_bad), (_dev, _tb, out, cnt, trk_d, _ts) in zip(G.FRUSTUM_BATCH, keep):
        c = cnt.cpu().numpy()
        print(sl, c, out.cpu().numpy()[:nkp])
        assert c[0] == want_n and c[1] == want_bad, (sl, c)
        assert np.array_equal(out.cpu().numpy()[:nkp], want_k2m), sl
        check_track({k: v.cpu().numpy() for k, v in trk_d.items()}, in_view[sl], {k: v[sl] for k, v in want.items()})


@pytest.mark.parametrize("factor", [1.2, 2.0])
def test_predict_scale_sweep_matches_the_oracle_bit_for_bit(gpu, oracle, factor):
    """2^17 points on the optical axis whose max_dist / dist straddles factor^k by -8..+8 floats for k = 0..7, and 2^16
    random exact positions: the device's (float)log((double)ratio) against the host's logf, and its 1.0f / z against the
    host's division, through level, proj_x, proj_y and proj_xr of every in-view row, the in-view flags and the count of
    levels out of range."""
    t = G.sweep_table(factor)
    m = len(t["min_dist"])
    sf = G.scale_factors(factor)
    log_sf = float(np.log(np.float32(factor)))
    oframe = G.make_frame(oracle, G.SWEEP_KPS, sf)
    _n, k2m_o, iv, nlo, want = oracle.search_local_points(oframe, G.TCW, G.FX, G.FY, G.CX, G.CY, G.MBF, t, log_sf, th=1.0,
                                                          nnratio=0.8, want_track=True)
    # the sweep does straddle: every level occurs, and so does level 8 = nlevels (the rows above factor^7's threshold,
    # 8 of 17 of an eighth of the axis rows); level -1 cannot: a ratio just below 1 gives -0, a lower one fails the range
    assert set(np.unique(want["level"][iv != 0])) == set(range(G.NLEVELS)) and nlo > 1000
    k2m, counts, trk = device_frustum(gpu, G.make_frame(gpu, G.SWEEP_KPS, sf), t, log_sf, 1.0, 0.8)
    diff = np.nonzero(trk["in_view"] != iv)[0]
    print("factor", factor, "rows", m, "in view", int(iv.sum()), "out of range", nlo, "device", counts,
          "in_view differs at", diff[:8])
    assert len(diff) == 0 and counts[1] == nlo and np.array_equal(k2m, k2m_o)
    on = iv != 0
    for k in ("level", "proj_x", "proj_y", "proj_xr", "view_cos"):
        bad = np.nonzero(trk[k][on].view(np.int32) != want[k][on].view(np.int32))[0]
        assert len(bad) == 0, (k, len(bad), trk[k][on][bad[:4]], want[k][on][bad[:4]])


@pytest.mark.parametrize("motion", list(G.LAST_MOTIONS))
def test_last_frame_builder_on_hand_worked_rows(gpu, motion):
    """SearchByProjection(CurrentFrame, LastFrame): the host builder and k_project_last_queries (through the table
    flavour) on depth 0 and below, both image bounds, the three level windows and a NaN position."""
    kps, last, expect = G.last_case(motion)
    cur = G.make_frame(gpu, kps)
    k0 = np.full(len(kps), -1, np.int32)
    n, k2m = gpu.ORBmatcher(0.9, True).SearchByProjectionLast(cur, G.TCW, G.FX, G.FY, G.CX, G.CY, G.MBF, G.MB, last,
                                                              G.LAST_TH, False, k0)
    print(motion, "host flavour", n, k2m)
    assert np.array_equal(k2m, expect) and n == int((expect >= 0).sum())
    m = len(last["kp_octave"])
    ids = np.arange(7000, 7000 + m, dtype=np.int64)
    tbl = gpu.MapPointTable(initial_rows=16)
    tbl.upsert(ids, world_pos=last["world_pos"], desc=last["desc"], n_obs=last["obs_pos"].astype(np.int32))
    lastf = G.make_frame(gpu, [G.kp(10 + 20 * i, 20, int(o)) for i, o in enumerate(last["kp_octave"])])
    dl, dc = gpu.DeviceFrame().upload(lastf), gpu.DeviceFrame().upload(cur)
    n2, k2 = gpu.search_by_projection_last_table(dc, G.TCW, dl, last["Tcw"], tbl, ids, G.FX, G.FY, G.CX, G.CY, G.MBF, G.MB,
                                                 G.LAST_TH, False, True)
    print(motion, "table flavour", n2, k2)
    assert np.array_equal(k2, expect) and n2 == n


def last_table_call(gpu, kps, last):
    m = len(last["kp_octave"])
    ids = np.arange(7000, 7000 + m, dtype=np.int64)
    tbl = gpu.MapPointTable(initial_rows=16)
    tbl.upsert(ids, world_pos=last["world_pos"], desc=last["desc"], n_obs=last["obs_pos"].astype(np.int32))
    lastf = G.make_frame(gpu, [G.kp(10 + 20 * i, 20, int(o)) for i, o in enumerate(last["kp_octave"])])
    dl, dc = gpu.DeviceFrame().upload(lastf), gpu.DeviceFrame().upload(G.make_frame(gpu, kps))
    return gpu.search_by_projection_last_table(dc, G.TCW, dl, last["Tcw"], tbl, ids, G.FX, G.FY, G.CX, G.CY, G.MBF, G.MB,
                                               G.LAST_TH, False, True)


@pytest.mark.parametrize("octave", [-1, G.NLEVELS])
def test_last_frame_octave_out_of_range(gpu, octave):
    """An octave of -1 or nlevels on a row that projects into the image: the host flavour names the row with ELEVEL, the
    table flavour (k_project_last_queries counts the row) reports the count with ELEVEL."""
    kps, last, expect = G.last_case("neither")
    last["kp_octave"][10] = octave
    with pytest.raises(gpu.OrbGpuError) as ei:
        gpu.ORBmatcher(0.9, True).SearchByProjectionLast(G.make_frame(gpu, kps), G.TCW, G.FX, G.FY, G.CX, G.CY, G.MBF, G.MB,
                                                         last, G.LAST_TH, False, np.full(len(kps), -1, np.int32))
    assert ei.value.status == gpu.ELEVEL and "key point 10:" in str(ei.value)
    with pytest.raises(gpu.OrbGpuError) as ei:
        last_table_call(gpu, kps, last)
    assert ei.value.status == gpu.ELEVEL and "1 last-frame key point(s)" in str(ei.value)
    last["kp_octave"][10], last["kp_octave"][7] = 0, octave  # behind the camera: the octave is never read (:1367)
    n, k2m = gpu.ORBmatcher(0.9, True).SearchByProjectionLast(G.make_frame(gpu, kps), G.TCW, G.FX, G.FY, G.CX, G.CY, G.MBF,
                                                              G.MB, last, G.LAST_TH, False, np.full(len(kps), -1, np.int32))
    assert np.array_equal(k2m, expect)
    n2, k2 = last_table_call(gpu, kps, last)
    assert np.array_equal(k2, expect) and n2 == n


def test_fuse_gates_and_the_flavours_without_them(gpu):
    """Fuse's chi-square gates (mono 5.99, stereo 7.8 with u_right >= 0) and TH_LOW at equality in proj_walk_each;
    fuse_sim3 and search_by_projection_sim3 walk the same windows without the gates."""
    kps, pts, gated, ungated = G.fuse_case()
    frame = G.make_frame(gpu, kps)
    S = np.eye(4, dtype=np.float32)
    n, best = gpu.fuse(frame, G.TCW, G.FX, G.FY, G.CX, G.CY, G.MBF, G.LOG_SF, pts, G.FUSE_TH, G.INV_SIGMA2)
    print("fuse", n, best)
    assert np.array_equal(best, gated) and n == 3
    n, best = gpu.fuse_sim3(frame, S, G.FX, G.FY, G.CX, G.CY, G.LOG_SF, pts, G.FUSE_TH)
    print("fuse_sim3", n, best)
    assert np.array_equal(best, ungated) and n == 5
    n, k2m = gpu.search_by_projection_sim3(frame, S, G.FX, G.FY, G.CX, G.CY, G.LOG_SF, pts, int(G.FUSE_TH),
                                           np.full(len(kps), -1, np.int32))
    print("search_by_projection_sim3", n, k2m)
    assert np.array_equal(k2m, ungated) and n == 5


def test_keyframe_flavour_accepts_orb_dist_itself(gpu):
    kps, kf, expect = G.keyframe_case()
    n, k2m = gpu.ORBmatcher(0.9, True).SearchByProjectionKeyFrame(G.make_frame(gpu, kps), G.TCW, G.FX, G.FY, G.CX, G.CY,
                                                                  G.LOG_SF, kf, 3.0, G.ORB_DIST,
                                                                  np.full(len(kps), -1, np.int32))
    assert np.array_equal(k2m, expect) and n == 1


def test_initialization_windows_and_tie_order(gpu):
    """k_window_candidates: strict window, level 0 alone, level-1 key points of F1 are no rows, and the visiting order
    that decides between equal distances."""
    f1, f2, prev, m12 = G.init_case()
    n, out, pm = gpu.search_for_initialization(G.make_frame(gpu, f1), G.make_frame(gpu, f2), prev, G.INIT_WINDOW,
                                               G.INIT_NNRATIO, False)
    print("matches12", out)
    assert np.array_equal(out, m12) and n == int((m12 >= 0).sum())
    f2x = np.array([k[0] for k in f2], np.float32)
    assert np.array_equal(pm[m12 >= 0, 0], f2x[m12[m12 >= 0]]) and np.array_equal(pm[m12 < 0], prev[m12 < 0])


@pytest.mark.parametrize("swapped", [False, True])
def test_key_width_through_initialization(gpu, swapped):
    """Position 4096 of a cell in the keys that k_window_candidates hands to the host's sequential part."""
    f1, f2, prev, m12 = G.init_key_width_case(swapped)
    n, out, _pm = gpu.search_for_initialization(G.make_frame(gpu, f1), G.make_frame(gpu, f2), prev, 5, G.INIT_NNRATIO, False)
    print("matches12", out)
    assert n == 1 and np.array_equal(out, m12)


@pytest.mark.parametrize("motion", list(G.LAST_MOTIONS))
def test_last_frame_device_view_and_n_last(gpu, motion):
    """k_project_last_queries over a device view: all rows; an octave of -1 or nlevels is counted and its row left out, on
    the depth +0 row, whose NaN projection passes the bounds and which matches nothing anyway, and on row 10, which
    otherwise takes key point 7; with n_last = 10 the rows from 10 on are no rows."""
    torch = pytest.importorskip("torch")
    kps, last, expect = G.last_case(motion)
    m = len(last["kp_octave"])
    dc = gpu.DeviceFrame().upload(G.make_frame(gpu, kps))
    fv, ncur = dc.device_view()
    s = torch.cuda.current_stream().cuda_stream

    def run(octave, n_last):
        rec = np.zeros((m, 7), np.float32)
        rec.view(np.int32)[:, 5] = octave
        d = {"n": torch.tensor([n_last], dtype=torch.int32).cuda(), "kps": torch.from_numpy(rec).cuda(),
             "has_mp": torch.from_numpy(last["has_mp"]).cuda(), "obs_pos": torch.from_numpy(last["obs_pos"]).cuda(),
             "world_pos": torch.from_numpy(last["world_pos"]).cuda(), "desc": torch.from_numpy(last["desc"]).cuda()}
        lv = gpu.DeviceLastFrameView()
        lv.cap, lv.outlier = m, None
        for k in d:
            setattr(lv, k, d[k].data_ptr())
        k2m = torch.full((max(fv.cap, 1),), -1, dtype=torch.int32, device="cuda")
        counts = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        gpu.search_by_projection_last_device(fv, G.TCW, lv, last["Tcw"], G.FX, G.FY, G.CX, G.CY, G.MBF, G.MB, G.LAST_TH, False,
                                             False, k2m.data_ptr(), counts.data_ptr(), stream=s)
        torch.cuda.synchronize()
        print(motion, n_last, counts.cpu().numpy(), k2m.cpu().numpy()[:ncur])
        return k2m.cpu().numpy()[:ncur], counts.cpu().numpy()

    k2m, counts = run(last["kp_octave"], m)
    assert np.array_equal(k2m, expect) and tuple(counts) == (int((expect >= 0).sum()), 0)
    without7 = expect.copy()
    without7[7] = -1  # row 10 is the one that takes key point 7
    for bad in (-1, G.NLEVELS):
        octave = last["kp_octave"].copy()
        octave[9] = bad
        k2m, counts = run(octave, m)
        assert np.array_equal(k2m, expect) and tuple(counts) == (int((expect >= 0).sum()), 1), bad
        octave = last["kp_octave"].copy()
        octave[10] = bad  # a row that projects inside the image: counted, left out, everything else as it was
        k2m, counts = run(octave, m)
        assert np.array_equal(k2m, without7) and tuple(counts) == (int((without7 >= 0).sum()), 1), bad
    cut = expect.copy()
    cut[7:] = -1  # key points 7, 8, 9 were taken by rows 10, 11, 12
    k2m, counts = run(last["kp_octave"], 10)
    assert np.array_equal(k2m, cut) and tuple(counts) == (int((cut >= 0).sum()), 0)


def test_search_by_sim3_has_no_gates_and_takes_th_high(gpu):
    kps, pts, already1, plain, skipped = G.sim3_pair_case()
    f, eye4, eye3, zero3 = G.make_frame(gpu, kps), np.eye(4, dtype=np.float32), np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    for already, want in ((None, plain), (already1, skipped)):
        n, m12 = gpu.search_by_sim3(f, f, eye4, eye4, 1.0, eye3, zero3, G.FX, G.FY, G.CX, G.CY, G.LOG_SF, G.LOG_SF, pts,
                                    already, pts, None, G.FUSE_TH)
        print("match12", m12)
        assert np.array_equal(m12, want) and n == int((want >= 0).sum())

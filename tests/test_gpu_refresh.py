"""orbgpu_covis_refresh_points, orbgpu_mappoint_table_refresh and the three columns behind them on the device against
tests/refresh_model.py: every output bit for bit, floats as their 32-bit patterns.  Every graph starts with
initial_rows = 2 and a pool of 8 slots, so rows, the pool columns -- the descriptor column among them -- and the hash grow in
every test.  In/out arrays start from random bytes: what the rules leave untouched must come back as it went in."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import refresh_model as RM  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F(gpu):
    import fuzz_refresh
    return fuzz_refresh


def base(F, seed=1, **kw):
    pair = F.RefreshPair(initial_rows=2, initial_slots=8)
    rng = np.random.default_rng(seed)
    return (pair, rng) + RM.base_scene(rng, pair, **kw)


def snapshot(pair, pts):
    flat = lambda d: {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in d.items()}  # noqa: E731
    return pair.dev.size(), flat(pair.dev.local_map(pts[:40], []))


@pytest.mark.parametrize("what", [RM.DESCRIPTOR, RM.NORMAL_DEPTH, RM.DESCRIPTOR | RM.NORMAL_DEPTH])
def test_base_graph_in_shuffled_order(F, what):
    pair, rng, kf_ids, pts, pos, ref = base(F)
    try:
        order = [int(i) for i in rng.permutation(len(pts))]
        want = pair.model.refresh(order, [ref[p] for p in order], pos[order], what)
        assert want["status"].tolist() == [0] * len(pts) and want["max_obs"] == 12 and want["n_slots"].min() == 1
        if what & RM.DESCRIPTOR:
            assert len(set(zip(want["desc_kf"].tolist(), want["desc_idx"].tolist()))) > 100
        before = snapshot(pair, pts)
        assert pair.refresh(order, [ref[p] for p in order], pos[order], what, RM.junk(rng, len(pts))) == ""
        assert pair.refresh(order[:1], [ref[order[0]]], pos[order[:1]], what, RM.junk(rng, 1)) == ""
        assert snapshot(pair, pts) == before and pair.size() == "" and pair.dev.debug_global_queries() == 0
    finally:
        pair.close()


def test_status_cases(F):
    pair, rng, kf_ids, pts, pos, ref = base(F, 2)
    try:
        p0 = pts[0]
        holder = pair.model.observations_of(p0)[0][0]
        other = next(k for k in kf_ids if all(k != o for o, _ in pair.model.observations_of(p0)))
        # a point held nowhere; references that are unknown and not an observer
        ids, refs = [10 ** 12, p0, pts[1], pts[2]], [kf_ids[0], 10 ** 13, ref[1], ref[2]]
        want = pair.model.refresh(ids, refs, pos[[0, 0, 1, 2]])
        assert want["status"].tolist() == [RM.NO_OBS, RM.NO_REF, 0, 0] and want["n_descriptors"] == 3 and want["n_normals"] == 2
        assert pair.refresh(ids, refs, pos[[0, 0, 1, 2]], 3, RM.junk(rng, 4)) == ""
        assert pair.refresh([p0], [other], pos[[0]], 3, RM.junk(rng, 1)) == "" and pair.model.refresh([p0], [other], pos[[0]])["status"][0] == RM.NO_REF
        # a row without descriptors and one without a centre: the other half still runs
        pair.add_keyframe(5, 3, [p0, pts[1], -1])
        pair.set_centres([5], [[0.5, 0.25, 0.125]])
        pair.add_keyframe(6, 2, [pts[2], -1])
        pair.set_descriptors(6, RM.PATTERNS[:2])
        ids, refs = [pts[2], p0, pts[1], pts[3]], [ref[2], holder, ref[1], ref[3]]
        want = pair.model.refresh(ids, refs, pos[[2, 0, 1, 3]])
        assert want["status"].tolist() == [RM.NO_CENTRE, RM.NO_DESC, RM.NO_DESC, 0]
        for what in (1, 2, 3):
            assert pair.refresh(ids, refs, pos[[2, 0, 1, 3]], what, RM.junk(rng, 4)) == ""
        # a reference that is bad: its slots are gone, the others still observe the point
        many = next(p for p in pts if len(pair.model.observations_of(p)) >= 3 and p not in (p0, pts[1], pts[2]))
        gone = pair.model.observations_of(many)[1][0]
        before = len(pair.model.observations_of(many))
        pair.set_bad([gone])
        assert len(pair.model.observations_of(many)) == before - 1
        assert pair.model.refresh([many], [gone], pos[[many]])["status"].tolist() == [RM.NO_REF]
        assert pair.refresh([many], [gone], pos[[many]], 3, RM.junk(rng, 1)) == ""
        snap = snapshot(pair, pts)
        assert pair.refresh(pts, [ref[p] for p in pts], pos, 3, RM.junk(rng, len(pts))) == ""
        assert snapshot(pair, pts) == snap and pair.size() == ""
        # a reference octave at and above n_levels: two levels instead of three
        pair.set_scale_factors([1.0, 1.2])
        want = pair.model.refresh(pts, [ref[p] for p in pts], pos, 2)
        assert 10 < want["n_no_ref"] < len(pts) - 10
        assert pair.refresh(pts, [ref[p] for p in pts], pos, 2, RM.junk(rng, len(pts))) == ""
    finally:
        pair.close()


def test_no_scale_table_and_no_centres_and_no_descriptors(F):
    for kw, status in ((dict(scale=False), RM.NO_REF), (dict(centres=False), RM.NO_CENTRE), (dict(descriptors=False), RM.NO_DESC)):
        pair, rng, kf_ids, pts, pos, ref = base(F, 3, n_pts=40, **kw)
        try:
            want = pair.model.refresh(pts, [ref[p] for p in pts], pos)
            assert want["status"].tolist() == [status] * len(pts)
            assert pair.refresh(pts, [ref[p] for p in pts], pos, 3, RM.junk(rng, len(pts))) == ""
        finally:
            pair.close()


def test_two_slots_of_one_row_and_clear(F):
    pair, rng, kf_ids, pts, pos, ref = base(F, 4)
    try:
        p = pts[5]
        k, j = pair.model.observations_of(p)[0]
        free = [i for i, q in enumerate(pair.model.row_of[k].slots) if q < 0][:2]
        pair.set_slots([k, k], free, [p, p])  # V2's deviation: the row now holds p three times
        n = len(pair.model.observations_of(p))
        assert [o for o in pair.model.observations_of(p) if o[0] == k] == sorted([(k, j)] + [(k, i) for i in free])
        want = pair.model.refresh([p], [k], pos[[p]])
        assert want["n_slots"].tolist() == [n] and want["status"].tolist() == [0]
        assert pair.refresh([p], [k], pos[[p]], 3, RM.junk(rng, 1)) == ""
        assert pair.clear() == ""
        assert pair.model.scale is None and pair.refresh(pts[:4], [ref[q] for q in pts[:4]], pos[:4], 3, RM.junk(rng, 4)) == ""
        kf2, pts2, pos2, ref2 = RM.base_scene(rng, pair, n_kf=5, n_slots=33, n_pts=30, max_obs=5, descriptors=False, scale=False)
        assert pair.refresh(pts2, ref2, pos2, 3, RM.junk(rng, 30)) == ""  # what the cleared rows held does not come back
        assert pair.model.refresh(pts2, ref2, pos2)["status"].tolist() == [RM.NO_DESC | RM.NO_REF] * 30
        for k2 in kf2:
            pair.set_descriptors(k2, RM.PATTERNS[rng.integers(0, 8, 33)])
        pair.set_scale_factors([1.0, 1.25, 1.5625])
        assert pair.refresh(pts2, ref2, pos2, 3, RM.junk(rng, 30)) == "" and pair.model.refresh(pts2, ref2, pos2)["n_normals"] == 30
    finally:
        pair.close()


def test_query_from_global_memory(F, monkeypatch):
    monkeypatch.setenv("ORBGPU_DEBUG_COVIS_LDS_IDS", "4")
    pair, rng, kf_ids, pts, pos, ref = base(F, 5)
    monkeypatch.delenv("ORBGPU_DEBUG_COVIS_LDS_IDS")
    try:
        assert pair.refresh(pts, [ref[p] for p in pts], pos, 3, RM.junk(rng, len(pts))) == ""
        assert pair.dev.debug_global_queries() == 2  # the count and the fill
        assert pair.refresh(pts[:4], [ref[p] for p in pts[:4]], pos[:4], 3, RM.junk(rng, 4)) == ""
        assert pair.dev.debug_global_queries() == 2  # four ids fit
    finally:
        pair.close()


def test_wave_and_workgroup_boundary(F):
    """130 rows of 8 slots; points 0-3 are observed 63, 64, 65 and 130 times: the last two take the workgroup path"""
    pair = F.RefreshPair(initial_rows=2, initial_slots=8)
    rng = np.random.default_rng(6)
    try:
        counts = (63, 64, 65, 130)
        kf_ids = [int(k) for k in rng.permutation(130) * 3 + 2 ** 33]
        for r, k in enumerate(kf_ids):
            slots = [-1] * 8
            for p, c in enumerate(counts):
                if r < c:
                    slots[2 * p + (r & 1)] = p
            slots[7 - (r & 1)] = 4 + r % 7
            pair.add_keyframe(k, 8, slots)
            pair.set_keypoints(k, rng.integers(0, 3, 8).astype(np.uint8))
            pair.set_descriptors(k, RM.PATTERNS[rng.integers(0, 8, 8)] ^ rng.integers(0, 2, (8, 32)).astype(np.uint8))
        pair.set_centres(kf_ids, rng.random((130, 3)).astype(np.float32))
        pair.set_scale_factors([1.0, 1.2, 1.44])
        ids = list(range(11))
        pos = (rng.random((11, 3)) * 2 + 3).astype(np.float32)
        refs = [kf_ids[0]] * 4 + [kf_ids[p - 4] for p in range(4, 11)]
        want = pair.model.refresh(ids, refs, pos)
        assert want["n_slots"][:4].tolist() == list(counts) and want["status"].tolist() == [0] * 11 and want["n_entries"] == 322 + 130
        for what in (1, 2, 3):
            assert pair.refresh(ids, refs, pos, what, RM.junk(rng, 11)) == ""
        assert pair.refresh([3, 1], [kf_ids[129], kf_ids[63]], pos[[3, 1]], 3, RM.junk(rng, 2)) == ""
    finally:
        pair.close()


def test_capacity(F):
    """R3: 1024 observations are refreshed, 1025 overflow with the count still exact"""
    pair = F.RefreshPair(initial_rows=2, initial_slots=8)
    rng = np.random.default_rng(7)
    try:
        for k in range(17):
            pair.add_keyframe(100 - k, 64, [7] * 64 if k < 16 else [8] * 64)
            pair.set_keypoints(100 - k, np.full(64, k % 3, np.uint8))
            pair.set_descriptors(100 - k, rng.integers(0, 256, (64, 32)).astype(np.uint8) & RM.PATTERNS[k % 8])
        pair.set_centres([100 - k for k in range(17)], rng.random((17, 3)).astype(np.float32))
        pair.set_scale_factors([1.0, 1.2, 1.44])
        pos = np.array([[3, 4, 5], [4, 3, 2]], np.float32)
        want = pair.model.refresh([7, 8], [90, 84], pos)
        assert want["n_slots"].tolist() == [1024, 64] and want["status"].tolist() == [0, 0]
        assert pair.refresh([7, 8], [90, 84], pos, 3, RM.junk(rng, 2)) == ""
        pair.add_keyframe(200, 2, [-1, 7])
        pair.set_descriptors(200, RM.PATTERNS[:2])
        pair.set_centres([200], [[0, 0, 0]])
        want = pair.model.refresh([8, 7], [84, 90], pos[::-1])
        assert want["n_slots"].tolist() == [64, 1025] and want["status"].tolist() == [0, RM.OVERFLOW] and want["max_obs"] == 1025
        assert pair.refresh([8, 7], [84, 90], pos[::-1], 3, RM.junk(rng, 2)) == ""
    finally:
        pair.close()


def test_pool_growth_keeps_descriptors_and_a_graph_without_them_is_what_it_was(F):
    pair, rng, kf_ids, pts, pos, ref = base(F, 8, n_kf=4, n_pts=40, max_obs=4)
    plain = F.RefreshPair(initial_rows=2, initial_slots=8)  # the same rows, never given descriptors, centres or a table
    try:
        for k in kf_ids:
            plain.add_keyframe(k, 64, pair.model.row_of[k].slots)
            plain.set_keypoints(k, pair.model.kp[k])
        assert pair.refresh(pts, [ref[p] for p in pts], pos, 3, RM.junk(rng, 40)) == ""
        for i in range(8):  # 4 rows of 64 slots filled a pool of 256: every further row doubles it sooner or later
            pair.add_keyframe(5000 + i, 100, [int(rng.choice(pts)) for _ in range(100)])
            pair.set_descriptors(5000 + i, RM.PATTERNS[rng.integers(0, 8, 100)])
            pair.set_centres([5000 + i], rng.random((1, 3)).astype(np.float32))
            assert pair.refresh(pts, [ref[p] for p in pts], pos, 3, RM.junk(rng, 40)) == ""
        for g in (plain, pair):
            assert g.local_map(pts[:30], []) == "" and g.connections(kf_ids[0], 1) == "" and g.keyframe_culling(kf_ids, None, 1) == ""
            assert g.observations(pts) == "" and g.size() == ""
    finally:
        pair.close()
        plain.close()


def test_table_form(F, gpu):
    pair, rng, kf_ids, pts, pos, ref = base(F, 9)
    table = gpu.MapPointTable(initial_rows=8)
    twin = gpu.MapPointTable(initial_rows=8)
    try:
        known = pts[:140]
        mirror = F.fill_table(rng, table, known, pos[known], n_bad=5)
        start = {p: {k: np.array(v) for k, v in row.items()} for p, row in mirror.items()}
        ids = [int(i) for i in rng.permutation(150)] + [10 ** 12]
        refs = [ref[p] for p in ids[:-1]] + [kf_ids[0]]
        pre = [RM.UNKNOWN if p not in mirror else RM.BAD if mirror[p]["bad"] else 0 for p in ids]
        assert (pre.count(RM.UNKNOWN), pre.count(RM.BAD)) == (11, 5)
        # only status bytes and the record come back; the rows are read one by one and compared
        assert pair.refresh_table(table, mirror, ids, refs, RM.DESCRIPTOR, None, ()) == ""
        for p in known:  # the normal half was not asked for: bit-identical to the upserted values
            assert all(np.array_equal(mirror[p][k], start[p][k]) for k in ("normal", "min_dist", "max_dist", "world_pos"))
        assert sum(not np.array_equal(mirror[p]["desc"], start[p]["desc"]) for p in known) == 135
        assert pair.refresh_table(table, mirror, ids, refs, 3, RM.junk(rng, len(ids))) == ""
        for p in known:
            if mirror[p]["bad"]:
                assert all(np.array_equal(mirror[p][k], start[p][k]) for k in start[p])
        # the matcher over the refreshed table and over a table upserted with the model's values
        live = [p for p in known if not mirror[p]["bad"]]
        twin.upsert(live, *[np.stack([mirror[p][k] for p in live]) for k in ("world_pos", "normal", "min_dist", "max_dist", "desc")],
                    np.ones(len(live), np.int32))
        fx = fy = 500.0
        cx, cy = 320.0, 240.0
        P = np.stack([mirror[p]["world_pos"] for p in live])
        u, v = fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy
        seen = [i for i in range(len(live)) if P[i, 2] > 0.5 and 20 < u[i] < 620 and 20 < v[i] < 460][:21]
        assert len(seen) >= 5
        kp = [(u[i], v[i], o, mirror[live[i]]["desc"]) for i in seen for o in range(3)]
        sf = np.float32(1.2) ** np.arange(3, dtype=np.float32)
        frame = gpu.Frame([k[0] for k in kp], [k[1] for k in kp], [k[2] for k in kp], np.zeros(len(kp)), -np.ones(len(kp)),
                          np.stack([k[3] for k in kp]), 640, 480, sf)
        assert frame.n <= 64
        dfr = gpu.DeviceFrame().upload(frame)
        Tcw = np.eye(4, dtype=np.float32)
        args = (Tcw, fx, fy, cx, cy, 40.0, float(np.log(np.float32(1.2))), 5.0, 0.9)
        n1, k1 = gpu.search_local_points_table(dfr, table, live, *args)
        n2, k2 = gpu.search_local_points_table(dfr, twin, live, *args)
        print("matches over the refreshed table: %d of %d key points" % (n1, frame.n))
        assert n1 == n2 and np.array_equal(k1, k2) and n1 > 0
        dfr.close()
    finally:
        table.close()
        twin.close()
        pair.close()

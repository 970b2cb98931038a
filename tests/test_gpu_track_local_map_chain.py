"""Tracking::TrackLocalMap's first two steps chained on the device: orbgpu_covis_local_map's point list goes, as it is,
into orbgpu_search_local_points_table and gives the kp_to_mp and the count of the same search handed the list of
tests/covis_model.py.  A small scene: 8 key frames over a few hundred points of the suite's local-map scenario."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import covis_model as M  # noqa: E402
from test_gpu_map_table import local_map_scenario, make_gframe  # noqa: E402  (scene helpers)

pytestmark = pytest.mark.gpu


def test_local_map_feeds_search_local_points(gpu, oracle):
    st, sf, Tcw, wp, mp, of, rng = local_map_scenario(gpu, oracle, 640, 480, 500, 2, 0.0, 91)
    m = len(wp)
    ids = (rng.permutation(10 * m)[:m].astype(np.int64) * 7919 + 2 ** 33)
    tbl = gpu.MapPointTable(initial_rows=64)
    tbl.upsert(ids, wp, mp["normal"], mp["min_dist"], mp["max_dist"], mp["desc"], mp["obs_pos"].astype(np.int32) * 3)
    # the map: a few hundred of the points, each observed by two or three of 8 key frames
    used = rng.permutation(m)[:min(m, 400)]
    dev, model = gpu.CovisibilityGraph(initial_rows=2, initial_slots=8), M.CovisGraph()
    slots = {k: [] for k in range(8)}
    for p in used:
        for k in rng.choice(8, size=int(rng.integers(2, 4)), replace=False):
            slots[int(k)].append(int(ids[p]))
    try:
        for k in range(8):
            row = slots[k] + [-1] * 7
            order = rng.permutation(len(row))
            for g in (dev, model):
                g.add_keyframe(10 + k, len(row), [row[i] for i in order])
                g.set_parent(10 + k, 10 + k - 1 if k else -1)
                g.set_covisibles(10 + k, [10 + (k + 3) % 8, 10 + (k + 5) % 8])
        # the frame tracks 40 points that key frames 10 .. 12 hold: they vote, with whoever else observes them
        seen = [p for k in range(3) for p in slots[k]]
        kp_ids = np.full(of.n, -1, np.int64)
        kp_ids[rng.choice(of.n, 40, replace=False)] = rng.choice(seen, 40)
        got, want = dev.local_map(kp_ids, []), model.local_map(kp_ids, [])
        assert got["kf_ids"].tolist() == want["kf_ids"].tolist() and len(want["kf_ids"]) >= got["n_voted"] >= 3
        assert 100 < len(want["point_ids"]) <= len(used)
        fx, fy, cx, cy, bf = (float(v) for v in (st.fx, st.fy, st.cx, st.cy, st.bf))
        log_sf = float(np.log(np.float32(sf[1])))
        dfr = gpu.DeviceFrame().upload(make_gframe(gpu, of))
        n1, k1 = gpu.search_local_points_table(dfr, tbl, got["point_ids"], Tcw, fx, fy, cx, cy, bf, log_sf, 3.0, 0.8, kp_ids=kp_ids)
        n2, k2 = gpu.search_local_points_table(dfr, tbl, want["point_ids"], Tcw, fx, fy, cx, cy, bf, log_sf, 3.0, 0.8, kp_ids=kp_ids)
        assert n1 == n2 and np.array_equal(k1, k2) and n1 > 0
        assert got["point_ids"].dtype == np.int64 and np.array_equal(got["point_ids"], want["point_ids"])
    finally:
        dev.close()

"""The refusals of the refresh that need a row or a table to exist, on the device: orbgpu_covis_graph_set_descriptors with a
wrong n_slots or a null array, the call on a bad row (ignored), and every refusal of orbgpu_mappoint_table_refresh behind a
real table.  Each returns ORBGPU_EINVAL with its message, graph and table are what they were, and a following refresh
still equals tests/refresh_model.py bit for bit.  (The refusals that need neither are in tests/test_refresh_abi.py.)  The
last test runs the base graph and the 63 / 64 / 65 / 130-observation cases once more with the one-wave kernel's stored
distance row (ORBGPU_DEBUG_REFRESH_SELECT=rows), the variant the default leaves out."""
import ctypes as C
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
import test_gpu_refresh as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F(gpu):
    import fuzz_refresh
    return fuzz_refresh


def refused(G, call, text):
    with pytest.raises(G.OrbGpuError) as ei:
        call()
    assert ei.value.status == G.EINVAL and text in str(ei.value), str(ei.value)


def test_set_descriptors_refusals_that_need_a_row(F, gpu):
    pair, rng, kf_ids, pts, pos, ref = T.base(F, 21)
    G, L, dev = gpu, gpu.lib(), pair.dev
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        pair.add_keyframe(5, 3, [pts[0], pts[1], -1])  # a row without descriptors: its points answer NO_DESC
        pair.set_centres([5], [[0.5, 0.25, 0.125]])
        with_desc, without = kf_ids[3], 5
        everything = lambda: pair.refresh(pts, [ref[q] for q in pts], pos, 3, RM.junk(rng, len(pts)))  # noqa: E731
        assert all(s & RM.NO_DESC for s in pair.model.refresh(pts[:2], [ref[q] for q in pts[:2]], pos[:2])["status"])
        assert everything() == ""
        before = T.snapshot(pair, pts)
        other = rng.integers(0, 256, (70, 32)).astype(np.uint8)  # bytes that would change every choice if they arrived
        for k, n in ((with_desc, 64), (without, 3)):
            refused(G, lambda: dev.set_descriptors(k, other[:n + 1]), "n_slots = %d, key frame %d has %d" % (n + 1, k, n))
            refused(G, lambda: dev.set_descriptors(k, other[:n - 1]), "n_slots = %d, key frame %d has %d" % (n - 1, k, n))
            refused(G, lambda: dev.set_descriptors(k, None), "n_slots = 0, key frame %d has %d" % (k, n))
            assert L.orbgpu_covis_graph_set_descriptors(dev.h, k, n, None) == G.EINVAL  # a null array with n_slots > 0
            assert b"null argument" in L.orbgpu_last_error_string()
            assert L.orbgpu_covis_graph_set_descriptors(None, k, n, p(other)) == G.EINVAL
        refused(G, lambda: dev.set_descriptors(10 ** 12, other[:64]), "key frame 1000000000000 is not in the graph")
        # the model refuses the same calls, and nothing arrived: the row with descriptors chooses as before, the row without
        # still has none (its flag did not go up), the graph is what it was
        for k, n in ((with_desc, 65), (without, 2)):
            with pytest.raises(RM.Refused):
                pair.model.set_descriptors(k, other[:n])
        assert everything() == "" and T.snapshot(pair, pts) == before and pair.size() == ""
        assert pair.refresh(pts[:2], [ref[q] for q in pts[:2]], pos[:2], 1, RM.junk(rng, 2)) == ""
        # a bad row ignores the call (V2: it holds no slot), whatever it held: OK is returned and nothing changes
        pair.set_bad([with_desc, without])
        assert everything() == ""
        before = T.snapshot(pair, pts)
        pair.set_descriptors(with_desc, other[:64])
        pair.set_descriptors(without, other[:3])
        refused(G, lambda: dev.set_descriptors(without, other[:4]), "n_slots = 4, key frame 5 has 3")  # still refused first
        assert everything() == "" and T.snapshot(pair, pts) == before and pair.size() == ""
        assert not any(s & RM.NO_DESC for s in pair.model.refresh(pts[:2], [ref[q] for q in pts[:2]], pos[:2])["status"])  # the row is gone
    finally:
        pair.close()


def test_table_form_refusals_behind_a_real_table(F, gpu):
    pair, rng, kf_ids, pts, pos, ref = T.base(F, 22)
    G, L = gpu, gpu.lib()
    table = G.MapPointTable(initial_rows=8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        known = pts[:120]
        mirror = F.fill_table(rng, table, known, pos[known], n_bad=4)
        assert pair.refresh_table(table, mirror, pts, [ref[q] for q in pts], 3, RM.junk(rng, len(pts))) == ""
        before = T.snapshot(pair, pts)
        rows = {q: table.read(q) for q in known}
        ids, refs = pts[:6], [ref[q] for q in pts[:6]]
        refused(G, lambda: table.refresh(pair.dev, ids, refs, 0), "what = 0x0")
        refused(G, lambda: table.refresh(pair.dev, ids, refs, 4), "what = 0x4")
        refused(G, lambda: table.refresh(pair.dev, ids, refs, 7), "what = 0x7")
        refused(G, lambda: table.refresh(pair.dev, ids + [ids[2]], refs + [refs[2]], 3), "map point id %d appears twice in one refresh call" % ids[2])
        refused(G, lambda: table.refresh(pair.dev, ids + [-1], refs + [refs[0]], 3), "map point id -1 (entry 6)")
        refused(G, lambda: table.refresh(pair.dev, [-5] + ids, [refs[0]] + refs, 3, G.REFRESH_OUTPUTS), "map point id -5 (entry 0)")
        a_ids, a_refs = np.array(ids, np.int64), np.array(refs, np.int64)
        ns, st, res = np.zeros(6, np.int32), np.zeros(6, np.uint8), G.CovisRefreshResult()
        args = lambda **kw: [kw.get("t", table.h), kw.get("g", pair.dev.h), kw.get("n", 6), kw.get("ids", p(a_ids)), kw.get("ref", p(a_refs)),  # noqa: E731
                             3, None, None, None, None, None, None, kw.get("ns", p(ns)), kw.get("st", p(st)), kw.get("res", C.byref(res))]
        for bad_args in (dict(t=None), dict(g=None), dict(n=-1), dict(n=(1 << 20) + 1), dict(ids=None), dict(ref=None), dict(ns=None),
                         dict(st=None), dict(res=None)):
            assert L.orbgpu_mappoint_table_refresh(*args(**bad_args)) == G.EINVAL, bad_args
        assert L.orbgpu_mappoint_table_refresh(*args()) == 0 and st.tolist() == pair.model.refresh(
            ids, refs, pos[ids], 3, None, [RM.BAD if mirror[q]["bad"] else 0 for q in ids])["status"].tolist()
        # table and graph are what they were: every row bit for bit, and the next refresh in both forms equals the model
        for q in known:
            r = table.read(q)
            assert all(np.array_equal(np.asarray(r[k]), np.asarray(rows[q][k])) for k in r), q
        assert T.snapshot(pair, pts) == before and pair.size() == "" and table.rows() == len(known)
        order = [int(i) for i in rng.permutation(len(pts))]
        assert pair.refresh_table(table, mirror, order, [ref[q] for q in order], 3, RM.junk(rng, len(pts))) == ""
        assert pair.refresh(order, [ref[q] for q in order], pos[order], 3, RM.junk(rng, len(pts))) == ""
    finally:
        table.close()
        pair.close()


def test_stored_distance_row_variant_of_the_one_wave_kernel(F, monkeypatch):
    monkeypatch.setenv("ORBGPU_DEBUG_REFRESH_SELECT", "rows")  # read when a graph is created
    for what in (RM.DESCRIPTOR, RM.DESCRIPTOR | RM.NORMAL_DEPTH):
        T.test_base_graph_in_shuffled_order(F, what)
    T.test_wave_and_workgroup_boundary(F)
    T.test_two_slots_of_one_row_and_clear(F)

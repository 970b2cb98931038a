"""The PnP solver on the device (orbgpu_pnp_*) against the restatement in pnp_model.py -- vs CPU restatement; OpenCV
boundary unpinned.  Discrete outputs are compared exactly, except hypotheses the model alone calls not well-conditioned
(a repeated index, an eigenvalue gap below pnp_model.GAP, a choice among the three solutions within the bound) or that
hold a near-threshold pair (pnp_model.MARGIN_FACTOR x the bound); continuous outputs within 16 x the model's own spread
between its Jacobi and numpy.linalg.eigh / the same steps.  The reasoning for the constants is next to them in
tests/pnp_model.py; the figures of a run go to profiles/pnp_parity.json."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pnp_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

FIGURES = {}


@pytest.fixture(scope="module")
def G():
    from orb_slam2_map_amd import lib
    if lib.device_count() < 1:
        pytest.skip("no HIP device")
    return lib


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def F(G):
    import fuzz_pnp
    return fuzz_pnp


@pytest.fixture(scope="module")
def base(G, torch, F):
    """one scene and its device result, shared by the tests that vary it"""
    sc = M.make_scene(120, 31, n_hyp=60, min_inliers=10)
    return sc, F.run_batch(torch, [sc])[0]


def record():
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pnp_parity.json"), "w") as f:
        json.dump({"note": "vs CPU restatement; OpenCV boundary unpinned", "gap": M.GAP, "bound_factor": M.BOUND_FACTOR,
                   "margin_factor": M.MARGIN_FACTOR, "model_spread_jacobi_vs_eigh": max(v["spread"] for v in FIGURES.values()),
                   "device_max_deviation": max(v["device_dev"] for v in FIGURES.values()),
                   "largest_left_out_share": max(v["left_out"] for v in FIGURES.values()),
                   "by_size": {k: FIGURES[k] for k in FIGURES}}, f, indent=1)


@pytest.mark.parametrize("key", list(M.PARITY_SCENES))
def test_parity_with_the_model(G, torch, F, key):
    n, _, min_set = M.PARITY_SCENES[key]
    # one batched call: the scene as it is, and the same scene asked for 40 iterations (the scan runs past max_its = 35)
    scenes = [M.parity_scene(key), M.parity_scene(key)]
    passes = [M.model_pass(scenes[0]), None]
    m2, e2 = M.solve(scenes[1], n_iterations=40), M.solve(scenes[1], eig="eigh", n_iterations=40)
    m2["well"] = M.well_conditioned(m2)
    ok = m2["well"] & M.well_conditioned(e2)
    passes[1] = (m2, M.dev(m2["Tcw"][:m2["n_use"]][ok], e2["Tcw"][:m2["n_use"]][ok]))
    ups = [F.upload(torch, scenes[0]), F.upload(torch, scenes[1], n_iterations=40)]
    G.pnp_solve_batch_device([u[0] for u in ups], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = [F.download(u[1], sc) for u, sc in zip(ups, scenes)]
    rep = F.compare(scenes, got, passes)
    print("pnp parity %s: spread %.3e, bound %.3e, margin %.3e, device deviation %.3e, left out %d of %d" % (
        key, rep["spread"], rep["bound"], rep["margin"], rep["device_dev"], rep["hypotheses_left_out"], rep["hypotheses"]))
    FIGURES[key] = {k: rep[k] for k in ("spread", "bound", "margin", "device_dev", "left_out", "hypotheses", "hypotheses_left_out")}
    FIGURES[key]["mismatches"] = rep["mismatches"][:5]
    record()
    for sc, (m, _), r in zip(scenes, passes, got):
        assert m["N"] == n and r["n"] == n and len(sc["valid"]) > n and sc["min_set"] == min_set
        if n < 10:
            assert r["no_more"] == 1 and r["iterations"] == 0 and not r["counts"].any() and not r["Tcw"].any()
        if n >= 300:
            assert r["accepted"] >= 0 and r["n_inliers"] > r["min_inliers"] >= n // 2
    if n >= 10:
        assert passes[1][0]["n_use"] == 40 and got[1]["iterations"] == (40 if got[1]["accepted"] < 0 else got[1]["accepted"] + 1)
    assert rep["left_out"] <= M.LEFT_OUT_CAP
    assert not rep["mismatches"], rep["mismatches"][:10]


def test_degenerate_and_hostile_input(G, torch, F, base):
    sc, ref = base
    idx = np.flatnonzero(sc["valid"])
    u = ref["max_its"]
    assert ref["n"] == 120 and u == 35 and ref["n_bad_set"] == 0
    # a set naming one row four times, and a coplanar set: computed like any other, nothing else moves
    sc2 = dict(sc, sets=sc["sets"].copy())
    sc2["sets"][2] = (8, 8, 8, 8)
    got = F.run_batch(torch, [sc2])[0]
    m2 = M.solve(sc2)
    assert m2["repeated"][2] and got["counts"][2] == m2["counts"][2] == 0 and got["n_bad_set"] == 0
    keep = np.arange(u) != 2
    assert np.array_equal(got["counts"][:u][keep], ref["counts"][:u][keep]) and np.array_equal(got["masks"][:u][keep], ref["masks"][:u][keep])
    assert got["Tcw_all"][:u][keep].tobytes() == ref["Tcw_all"][:u][keep].tobytes()
    scp = dict(sc, Xw=sc["Xw"].copy(), sets=sc["sets"].copy())
    plane = scp["Xw"][idx[[3, 4, 5]]].astype(np.float64)
    scp["Xw"][idx[6]] = (0.2 * plane[0] + 0.3 * plane[1] + 0.5 * plane[2]).astype(np.float32)
    scp["sets"][1] = (3, 4, 5, 6)
    gp, mp = F.run_batch(torch, [scp])[0], M.solve(scp)
    assert gp["counts"][1] == mp["counts"][1] and M.dev(mp["Tcw"][1], gp["Tcw_all"][1]) <= 1e-6
    # a NaN world point in a compacted row that is drawn: every hypothesis that draws it has count 0, nowhere is it an inlier
    k5 = int(sc["sets"][0, 0])
    sc3 = dict(sc, Xw=sc["Xw"].copy())
    sc3["Xw"][idx[k5]] = np.nan
    got3, m3 = F.run_batch(torch, [sc3])[0], M.solve(sc3)
    uses = (sc["sets"][:u] == k5).any(1)
    assert uses.any() and not got3["counts"][:u][uses].any() and got3["n"] == m3["N"] == 120
    assert np.isnan(got3["Tcw_all"][:u][uses][:, :3]).all()
    w, bit = idx[k5] // 64, np.uint64(1) << np.uint64(idx[k5] % 64)
    assert not (got3["masks"][:, w] & bit).any() and not (got3["refined_mask"][w] & bit)
    want = ref["masks"].copy()
    want[:, w] &= ~bit
    had = ((ref["masks"][:, w] & bit) != 0).astype(np.int32)
    assert np.array_equal(got3["masks"][:u][~uses], want[:u][~uses])
    assert np.array_equal(got3["counts"][:u][~uses], (ref["counts"] - had)[:u][~uses])
    assert got3["Tcw_all"][:u][~uses].tobytes() == ref["Tcw_all"][:u][~uses].tobytes()
    assert np.array_equal(got3["counts"], m3["counts"])
    # an octave of -1 and of nlevels: not kept, and counted
    sc4 = dict(sc, octave=sc["octave"].copy())
    sc4["octave"][idx[-1]], sc4["octave"][idx[-2]] = M.NLEVELS, -1
    got4, m4 = F.run_batch(torch, [sc4])[0], M.solve(sc4)
    assert got4["n_bad_index"] == 2 == m4["n_bad_index"] and got4["n"] == 118 == m4["N"]
    assert np.array_equal(got4["indices"][:118], idx[:-2])
    rep = F.compare([sc4], [got4])
    assert rep["left_out"] <= M.LEFT_OUT_CAP and not rep["mismatches"], rep["mismatches"]
    # a set index of N (and a negative one): counted, never read through; EINVAL in the host flavour
    bad = dict(sc, sets=sc["sets"].copy())
    bad["sets"][3, 1] = 120
    with pytest.raises(G.OrbGpuError) as ei:
        G.pnp_solve(bad)
    assert ei.value.status == G.EINVAL
    bad["sets"][5, 0] = -1
    r = F.run_batch(torch, [bad])[0]
    assert r["n_bad_set"] == 2 and not r["counts"][[3, 5]].any() and np.isnan(r["Tcw_all"][[3, 5]]).all() and not r["masks"][[3, 5]].any()
    keep = ~np.isin(np.arange(u), (3, 5))
    assert np.array_equal(r["counts"][:u][keep], ref["counts"][:u][keep])
    assert r["n_bad_set"] == M.solve(bad)["n_bad_set"]


def test_empty_problem_and_empty_batch(G, torch, F):
    sc = M.make_scene(3, 1, n1=5, n_hyp=4)
    sc0 = dict(sc, valid=np.zeros(0, np.uint8), Xw=np.zeros((0, 3), np.float32), kp=np.zeros((0, 2), np.float32),
               octave=np.zeros(0, np.int32))
    r = F.run_batch(torch, [sc0])[0]
    assert (r["n"], r["min_inliers"], r["max_its"], r["no_more"], r["accepted"], r["iterations"]) == (0, 10, 1, 1, -1, 0)
    assert not r["counts"].any()
    h = G.pnp_solve(sc0)
    assert (h["n"], h["max_its"], h["no_more"], h["accepted"]) == (0, 1, 1, -1) and len(h["inliers"]) == 0
    r = F.run_batch(torch, [dict(sc, sets=np.zeros((0, 4), np.int32))])[0]
    assert (r["n"], r["no_more"], r["accepted"]) == (3, 1, -1)
    G.pnp_solve_batch_device([])


def test_same_bytes_twice_in_a_batch_and_through_every_flavour(G, torch, F):
    sc = M.make_scene(300, 4242)
    rng = np.random.default_rng(1)
    others = [M.make_scene(int(n), 5000 + i, n_hyp=int(rng.choice([1, 5, 40])), min_set=int(rng.choice([4, 5, 6])))
              for i, n in enumerate(rng.integers(3, 200, 31))]
    alone, again = (F.result_bytes(F.run_batch(torch, [sc])[0]) for _ in range(2))
    assert alone == again
    for pos in (0, 15, 31):
        batch = others[:pos] + [sc] + others[pos:]
        got = F.run_batch(torch, batch + [sc])
        assert F.result_bytes(got[pos]) == alone and F.result_bytes(got[-1]) == alone, pos
    p, d = F.upload(torch, sc)
    G.pnp_solve_device(p, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    one = F.download(d, sc)
    assert F.result_bytes(one) == alone and one["accepted"] >= 0
    a = G.pnp_solve_all(sc)
    assert all(a[k] == one[k] for k in F.RESULT_KEYS) and a["Tcw"].tobytes() == one["Tcw"].tobytes()
    for k in ("counts", "Tcw_all", "masks", "refined_mask"):
        assert a[k].tobytes() == one[k].tobytes(), k
    h = G.pnp_solve(sc)
    assert all(h[k] == one[k] for k in F.RESULT_KEYS) and np.array_equal(h["counts"], one["counts"])
    assert h["Tcw"].tobytes() == one["Tcw"].tobytes() == h["Tcw_out"].tobytes()
    i = np.arange(len(sc["valid"]))
    bits = (one["refined_mask"][i // 64] >> (i % 64).astype(np.uint64)) & np.uint64(1)
    assert np.array_equal(h["inliers"], bits.astype(np.uint8)) and h["inliers"].sum() == one["n_inliers"]
    # table flavour: ids instead of arrays; the invalid rows hold no id, a bad point or an id the table never heard of
    n1 = len(sc["valid"])
    tb = G.MapPointTable()
    ids = 1000 + 3 * i.astype(np.int64)
    tb.upsert(ids, world_pos=sc["Xw"], normal=np.zeros((n1, 3), np.float32), min_dist=np.ones(n1, np.float32),
              max_dist=np.ones(n1, np.float32), desc=np.zeros((n1, 32), np.uint8))
    off = np.flatnonzero(sc["valid"] == 0)
    kp_ids = ids.copy()
    kp_ids[off[0::3]] = -1
    kp_ids[off[1::3]] = 5 + 3 * np.arange(len(off[1::3]))       # unknown ids
    tb.set_bad(ids[off[2::3]])
    fr = G.Frame(sc["kp"][:, 0], sc["kp"][:, 1], sc["octave"], np.zeros(n1, np.float32), np.full(n1, -1, np.float32),
                 np.zeros((n1, 32), np.uint8), 640, 480, np.ones(M.NLEVELS, np.float32))
    df = G.DeviceFrame().upload(fr)
    tr = G.pnp_solve_table(df, tb, kp_ids, sc)
    assert all(tr[k] == one[k] for k in F.RESULT_KEYS) and np.array_equal(tr["counts"], one["counts"])
    assert tr["Tcw"].tobytes() == one["Tcw"].tobytes() and np.array_equal(tr["inliers"], h["inliers"])
    assert tb.last_unknown() == (0, len(off[1::3]))
    L = G.lib()
    L.orbgpu_pnp_solve_table.argtypes = [C.c_void_p] * 8
    res = G.PnpResult()
    assert L.orbgpu_pnp_solve_table(df.h, tb.h, None, None, None, None, None, C.byref(res)) == G.EINVAL
    assert L.orbgpu_pnp_solve_table(None, tb.h, kp_ids.ctypes.data, None, None, None, None, C.byref(res)) == G.EINVAL
    q = G.pnp_problem(dict({k: sc[k] for k in ("K", "level_sigma2", "min_inliers", "max_iterations", "epsilon", "th2", "probability")},
                           n1=0, n_hyp=4, min_set=3, sets=sc["sets"].ctypes.data))
    assert L.orbgpu_pnp_solve_table(df.h, tb.h, kp_ids.ctypes.data, C.byref(q), None, None, None, C.byref(res)) == G.EINVAL
    df.close()
    tb.close()


def test_the_scan_resumes_from_a_given_state(G, torch, F):
    sc = M.make_scene(300, 4242, min_inliers=10)
    whole = F.run_batch(torch, [sc])[0]
    a = whole["accepted"]
    assert a >= 1
    # the records before the accepted one were refined without success; stop before it, then resume
    first = F.run_batch(torch, [dict(sc, sets=sc["sets"][:a])])[0]
    assert first["accepted"] == -1 and first["no_more"] == 0 and first["iterations"] == a
    nxt = F.run_batch(torch, [sc], start_iteration=a, best_so_far=first["best_inliers"])[0]
    for k in ("accepted", "n_inliers", "no_more", "best_inliers", "iterations"):
        assert nxt[k] == whole[k], k
    assert nxt["Tcw"].tobytes() == whole["Tcw"].tobytes() and np.array_equal(nxt["refined_mask"], whole["refined_mask"])
    assert np.array_equal(nxt["counts"], whole["counts"])
    # past the acceptance: the scan goes on from (a + 1, best) as the model's does
    m = M.solve(sc, start_iteration=a + 1, best_so_far=whole["best_inliers"])
    r = F.run_batch(torch, [sc], start_iteration=a + 1, best_so_far=whole["best_inliers"])[0]
    for k in ("accepted", "n_inliers", "best_inliers", "best_iteration", "iterations"):
        assert r[k] == int(m[k]), k
    assert r["no_more"] == int(m["no_more"])


def test_argument_errors_launch_nothing(G, torch, F):
    sc = M.make_scene(40, 5, n_hyp=8)
    L = G.lib()
    L.orbgpu_pnp_solve_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.orbgpu_pnp_solve_batch_device.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    assert L.orbgpu_pnp_solve_device(None, 0, None) == G.EINVAL
    p, d = F.upload(torch, sc)
    assert L.orbgpu_pnp_solve_batch_device(-1, C.byref(G.pnp_problem(p)), 0, None) == G.EINVAL
    assert L.orbgpu_pnp_solve_batch_device(1, None, 0, None) == G.EINVAL
    for over in ({"valid": 0}, {"Xw": 0}, {"kp": 0}, {"octave": 0}, {"sets": 0}, {"counts": 0}, {"Tcw": 0}, {"masks": 0},
                 {"refined_mask": 0}, {"result": 0}, {"n1": -1}, {"n_hyp": -1}, {"n1": 16385}, {"n_hyp": 4097}, {"min_set": 3},
                 {"min_set": 65}, {"nlevels": 0}, {"nlevels": 17}, {"min_inliers": -1}, {"max_iterations": -1},
                 {"start_iteration": -1}, {"best_so_far": -1}, {"n_iterations": -1}):
        q = G.pnp_problem(dict(p, **over))
        assert L.orbgpu_pnp_solve_device(C.byref(q), 0, None) == G.EINVAL, over
    torch.cuda.synchronize()
    assert (d["counts"].cpu().numpy() == -7).all()  # nothing ran


def test_fuzz_slice(G):
    import fuzz_pnp
    tot = fuzz_pnp.run(5.0, 20261019)
    print("fuzz: %d scenes, %d hypotheses, %d left out, spread %.3e, device deviation %.3e" % (
        tot["scenes"], tot["hypotheses"], tot["hypotheses_left_out"], tot["spread"], tot["device_dev"]))
    assert tot["scenes"] >= 4 and not tot["mismatches"], tot["mismatches"][:10]

"""The Sim3 solver on the device (orbgpu_sim3_*) against the restatement in sim3_model.py -- vs CPU restatement; OpenCV
boundary unpinned.  Discrete outputs are compared exactly, except hypotheses that are ill-conditioned (eigenvalue gap
below fuzz_sim3.GAP) or hold a near-threshold pair (fuzz_sim3.MARGIN_FACTOR x the bound); continuous outputs within
16 x the model's own spread between its Jacobi and numpy.linalg.eigh.  The reasoning for both is next to the constants in
tools/fuzz_sim3.py; the figures of a run go to profiles/sim3_parity.json."""
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

import sim3_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = M.PARITY_SIZES
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
    import fuzz_sim3
    return fuzz_sim3


def record(F):
    """what the parity cases run so far have measured, for profiles/sim3_parity.json"""
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sim3_parity.json"), "w") as f:
        json.dump({"note": "vs CPU restatement; OpenCV boundary unpinned", "gap": F.GAP, "bound_factor": F.BOUND_FACTOR,
                   "margin_factor": F.MARGIN_FACTOR, "model_spread_jacobi_vs_eigh": max(v["spread"] for v in FIGURES.values()),
                   "device_max_deviation": max(v["device_dev"] for v in FIGURES.values()),
                   "largest_left_out_share": max(v["left_out"] for v in FIGURES.values()),
                   "by_size": {str(k): FIGURES[k] for k in sorted(FIGURES)}}, f, indent=1)


@pytest.mark.parametrize("n", SIZES)
def test_parity_with_the_model(G, torch, F, n):
    scenes = M.parity_scenes(n)
    models, spread = F.model_pass(scenes)
    got = F.run_batch(torch, scenes)
    rep = F.compare(scenes, got, models, spread)
    print("sim3 parity N %d: spread %.3e, bound %.3e, margin %.3e, device deviation %.3e, left out %d of %d" % (
        n, rep["spread"], rep["bound"], rep["margin"], rep["device_dev"], rep["hypotheses_left_out"], rep["hypotheses"]))
    FIGURES[n] = {k: rep[k] for k in ("spread", "bound", "margin", "device_dev", "left_out", "hypotheses", "hypotheses_left_out")}
    FIGURES[n]["mismatches"] = rep["mismatches"][:5]
    record(F)
    for sc, m, r in zip(scenes, models, got):
        assert m["N"] == n and r["n"] == n and len(sc["valid"]) > n
        if n < 20:
            assert r["no_more"] == 1 and r["iterations"] == 0 and not r["counts"].any()
        if n >= 63 and len(sc["triples"]) == 300:
            assert r["accepted"] >= 0 and r["n_inliers"] > 20
    assert rep["left_out"] <= F.LEFT_OUT_CAP
    assert not rep["mismatches"], rep["mismatches"][:10]


def _host(G, sc, **kw):
    return G.sim3_solve(sc["valid"], sc["Xw1"], sc["Xw2"], sc["octave1"], sc["octave2"], sc["T1w"], sc["T2w"], sc["K1"], sc["K2"],
                        sc["level_sigma2"], sc["triples"], sc["fix_scale"], sc["probability"], sc["min_inliers"],
                        sc["max_iterations"], **kw)


def test_degenerate_triple_nan_point_and_bad_octave(G, torch, F):
    sc = M.make_scene(120, 31)
    base = F.run_batch(torch, [sc])[0]
    idx = np.flatnonzero(sc["valid"])
    # one point three times.  Row 8: (p + p + p) / 3 == p in every coordinate, so M = 0, N = 0, q = (1, 0, 0, 0), |v| = 0:
    # NaN, count 0.  Row 7: the centroid rounds off p, the hypothesis is a rotation fitted to rounding residue -- whatever
    # the definition makes of it (its eigenvalue gap is 0, so only the model's count is asked for when the model has NaN)
    prep = M.prepare(sc)
    assert np.isnan(M.horn(prep["X1"][[8, 8, 8]], prep["X2"][[8, 8, 8]], False)["R"]).all()
    assert not np.isnan(M.horn(prep["X1"][[7, 7, 7]], prep["X2"][[7, 7, 7]], False)["R"]).any()
    sc2 = dict(sc, triples=sc["triples"].copy())
    sc2["triples"][2], sc2["triples"][4] = (8, 8, 8), (7, 7, 7)
    got = F.run_batch(torch, [sc2])[0]
    assert got["counts"][2] == 0 and np.isnan(got["R"][2]).all() and np.isnan(got["T12"][2][:3]).all() and not got["masks"][2].any()
    assert not np.isnan(got["R"][4]).any()
    keep = ~np.isin(np.arange(300), (2, 4))
    assert np.array_equal(got["counts"][keep], base["counts"][keep]) and np.array_equal(got["masks"][keep], base["masks"][keep])
    assert got["R"][keep].tobytes() == base["R"][keep].tobytes() and got["n_bad_triple"] == 0
    # a NaN world point in compacted row 5: every hypothesis that draws it has count 0, nowhere is it an inlier
    sc3 = dict(sc, Xw1=sc["Xw1"].copy())
    sc3["Xw1"][idx[5]] = np.nan
    got3, m3 = F.run_batch(torch, [sc3])[0], M.solve(sc3)
    uses = (sc["triples"] == 5).any(1)
    assert uses.any() and not got3["counts"][uses].any() and got3["n"] == m3["N"] == 120
    assert not ((got3["masks"][:, idx[5] // 64] >> np.uint64(idx[5] % 64)) & np.uint64(1)).any()
    # the other hypotheses lose that row, if they had it, and nothing else
    w, bit = idx[5] // 64, np.uint64(1) << np.uint64(idx[5] % 64)
    want = base["masks"].copy()
    want[:, w] &= ~bit
    had = ((base["masks"][:, w] & bit) != 0).astype(np.int32)
    assert np.array_equal(got3["masks"][~uses], want[~uses]) and np.array_equal(got3["counts"][~uses], (base["counts"] - had)[~uses])
    assert got3["R"][~uses].tobytes() == base["R"][~uses].tobytes()
    assert np.array_equal(got3["counts"], m3["counts"]) and np.isnan(got3["R"][uses]).all()
    # an octave out of range: the row is not kept and is counted
    sc4 = dict(sc, octave1=sc["octave1"].copy())
    sc4["octave1"][idx[-1]], sc4["octave1"][idx[-2]] = M.NLEVELS, -1
    got4, m4 = F.run_batch(torch, [sc4])[0], M.solve(sc4)
    assert got4["n_bad_index"] == 2 == m4["n_bad_index"] and got4["n"] == 118 == m4["N"]
    assert np.array_equal(got4["indices1"][:118], idx[:-2])
    rep = F.compare([sc4], [got4])
    assert not rep["mismatches"], rep["mismatches"]


def test_empty_problem_and_empty_batch(G, torch, F):
    sc = M.make_scene(3, 1, n1=5, n_hyp=4)
    sc0 = dict(sc, valid=np.zeros(0, np.uint8), Xw1=np.zeros((0, 3), np.float32), Xw2=np.zeros((0, 3), np.float32),
               octave1=np.zeros(0, np.int32), octave2=np.zeros(0, np.int32))
    r = F.run_batch(torch, [sc0])[0]
    assert (r["n"], r["max_its"], r["no_more"], r["accepted"], r["iterations"]) == (0, 1, 1, -1, 0) and not r["counts"].any()
    h = _host(G, sc0)
    assert (h["n"], h["max_its"], h["no_more"], h["accepted"]) == (0, 1, 1, -1) and len(h["inliers"]) == 0
    # min_inliers = 0 with no rows: one iteration is due, its triple cannot be valid
    r = F.run_batch(torch, [dict(sc0, min_inliers=0)])[0]
    assert r["n_bad_triple"] == 1 and r["accepted"] == -1 and r["no_more"] == 1 and r["iterations"] == 1
    G.sim3_solve_batch_device([])


def test_same_bytes_twice_in_a_batch_and_through_every_flavour(G, torch, F):
    sc = M.make_scene(300, 4242)
    rng = np.random.default_rng(1)
    others = [M.make_scene(int(n), 5000 + i, n_hyp=int(rng.choice([1, 5, 40]))) for i, n in enumerate(rng.integers(3, 200, 127))]
    alone, again = (F.result_bytes(F.run_batch(torch, [sc])[0]) for _ in range(2))
    assert alone == again
    for pos in (0, 63, 127):
        batch = others[:pos] + [sc] + others[pos:]
        assert F.result_bytes(F.run_batch(torch, batch)[pos]) == alone, pos
    p, d = F.upload(torch, sc)
    G.sim3_solve_device(p, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    one = F.download(d, sc)
    assert F.result_bytes(one) == alone
    h = _host(G, sc)
    b = one["best_iteration"]
    assert all(h[k] == one[k] for k, _ in G.Sim3Result._fields_) and np.array_equal(h["counts"], one["counts"])
    assert one["accepted"] >= 0 and b == one["accepted"]
    assert h["R"].tobytes() == one["R"][b].tobytes() and h["t"].tobytes() == one["t"][b].tobytes()
    assert np.float32(h["s"]).tobytes() == one["s"][b].tobytes() and h["T12"].tobytes() == one["T12"][b].tobytes()
    bits = (one["masks"][b][np.arange(len(sc["valid"])) // 64] >> (np.arange(len(sc["valid"])) % 64).astype(np.uint64)) & np.uint64(1)
    assert np.array_equal(h["inliers"], bits.astype(np.uint8)) and h["inliers"].sum() == one["n_inliers"]


def test_the_scan_resumes_from_a_given_state(G, torch, F):
    sc = M.make_scene(300, 99)
    first = F.run_batch(torch, [sc])[0]
    a = first["accepted"]
    assert 0 <= a < 299
    nxt = F.run_batch(torch, [sc], start_iteration=a + 1, best_so_far=first["best_inliers"])[0]
    st = M.RansacState(300, 20, 300)
    st.iterate(300, first["counts"])
    want = st.iterate(300, first["counts"])
    assert (nxt["accepted"], nxt["n_inliers"], bool(nxt["no_more"])) == want and nxt["best_inliers"] == st.best
    assert np.array_equal(nxt["counts"], first["counts"])


def test_argument_errors_launch_nothing(G, torch, F):
    import ctypes as C
    sc = M.make_scene(40, 5, n_hyp=8)
    L = G.lib()
    L.orbgpu_sim3_solve_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.orbgpu_sim3_solve_batch_device.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    assert L.orbgpu_sim3_solve_device(None, 0, None) == G.EINVAL
    p, d = F.upload(torch, sc)
    assert L.orbgpu_sim3_solve_batch_device(-1, C.byref(G.sim3_problem(p)), 0, None) == G.EINVAL
    assert L.orbgpu_sim3_solve_batch_device(1, None, 0, None) == G.EINVAL
    for over in ({"valid": 0}, {"Xw1": 0}, {"Xw2": 0}, {"octave1": 0}, {"octave2": 0}, {"triples": 0}, {"counts": 0}, {"R": 0},
                 {"t": 0}, {"s": 0}, {"T12": 0}, {"masks": 0}, {"result": 0}, {"n1": -1}, {"n_hyp": -1}, {"n1": 1 << 20},
                 {"nlevels": 0}, {"nlevels": 17}, {"min_inliers": -1}, {"max_iterations": -1}, {"start_iteration": -1},
                 {"best_so_far": -1}):
        q = G.sim3_problem(dict(p, **over))
        assert L.orbgpu_sim3_solve_device(C.byref(q), 0, None) == G.EINVAL, over
    torch.cuda.synchronize()
    assert (d["counts"].cpu().numpy() == -7).all()  # nothing ran
    # a triple index >= N: refused by the host flavour before any launch, clamped and flagged on the device
    bad = dict(sc, triples=sc["triples"].copy())
    bad["triples"][3, 1] = 40
    with pytest.raises(G.OrbGpuError) as ei:
        _host(G, bad)
    assert ei.value.status == G.EINVAL
    bad["triples"][5, 0] = -1
    r, ok = F.run_batch(torch, [bad])[0], F.run_batch(torch, [sc])[0]
    assert r["n_bad_triple"] == 2 and not r["counts"][[3, 5]].any() and np.isnan(r["R"][[3, 5]]).all()  # all 8 are used: max_its 35
    keep = ~np.isin(np.arange(8), (3, 5))
    assert np.array_equal(r["counts"][keep], ok["counts"][keep])


def test_fuzz_slice(G):
    import fuzz_sim3
    tot = fuzz_sim3.run(5.0, 20261018)
    print("fuzz: %d scenes, %d hypotheses, %d left out, device deviation %.3e" % (
        tot["scenes"], tot["hypotheses"], tot["hypotheses_left_out"], tot["device_dev"]))
    assert tot["scenes"] >= 8 and not tot["mismatches"], tot["mismatches"][:10]

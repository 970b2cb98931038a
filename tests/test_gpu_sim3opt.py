"""Optimizer::OptimizeSim3 on the device (orbgpu_sim3_optimize*) against the float64 restatement in sim3opt_model.py --
vs CPU restatement; g2o boundary unpinned.  Over the committed PARITY_SCENES (none left out: test_sim3opt_model.py
asserts their margins) the discrete outputs are compared exactly, the refined Sim3 within 16 x the model's own spread
(8 permutations of the summation order plus libm_nudge = +-1, largest over the set), the float outputs as the exact
casts of the device's doubles, T12 / Scw as the model's formula on the device's doubles; determinism and the three
flavours as bytes; the limits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import sim3opt_model as M  # noqa: E402

pytestmark = pytest.mark.gpu


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
    import fuzz_sim3opt
    return fuzz_sim3opt


@pytest.fixture(scope="module")
def parity(G, torch, F):
    """The whole committed set in one batched call, the model on every scene and the set's spread: computed once."""
    names = [n for n, _ in M.PARITY_SCENES]
    scenes = [s for _, s in M.PARITY_SCENES]
    models = [M.optimize_sim3(s) for s in scenes]
    got = F.run_batch(torch, scenes)
    spills = G.sim3_opt_last_spills()
    rep = F.compare(scenes, got, models=models)
    per_scene = {n: {"N": m["n_correspondences"], "n_bad": m["n_bad"], "n_inliers": m["n_inliers"], "stages": m["stages"],
                     "margin": m["margin"], "device_deviation": M.state_deviation(g[1], m),
                     "device_iterations": g[1]["iterations"], "model_iterations": m["iterations"],
                     "device_trials": g[1]["trials"], "model_trials": m["trials"]}
                 for n, m, g in zip(names, models, got)}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sim3opt_parity.json"), "w") as f:
        json.dump({"note": "vs CPU restatement; g2o boundary unpinned", "scenes": len(scenes), "compared": rep["compared"],
                   "left_out": rep["left_out"], "model_spread": rep["spread"], "model_runs_with_a_discrete_flip": rep["flips"],
                   "device_max_deviation": rep["device_dev"], "allowed": 16 * rep["spread"], "scw_max_deviation": rep["scw_dev"],
                   "mismatches": rep["mismatches"], "per_scene": per_scene}, f, indent=1)
    print("sim3opt parity: compared %d, left out %d, model spread %.3e, device deviation %.3e" % (
        rep["compared"], rep["left_out"], rep["spread"], rep["device_dev"]))
    return {"names": names, "scenes": scenes, "models": models, "got": got, "rep": rep, "spills": spills}


def test_parity_with_the_model_over_the_committed_scenes(parity):
    rep = parity["rep"]
    assert rep["left_out"] == 0 and rep["compared"] == len(M.PARITY_SCENES)
    assert not rep["mismatches"], rep["mismatches"][:10]
    # only the two scenes with more correspondences than the LDS holds took the spill path
    assert parity["spills"] == sum(m["n_correspondences"] > M.LDS_PAIRS for m in parity["models"]) == 2


def test_parity_set_covers_every_branch(parity):
    by = dict(zip(parity["names"], parity["got"]))
    assert {by["n%d_fix0" % n][1]["n_correspondences"] for n in M.PARITY_SIZES} == set(M.PARITY_SIZES)
    for n in ("clean_40", "clean_130_fix"):  # nBad == 0: five further iterations at the most
        r, m = by[n][1], parity["models"][parity["names"].index(n)]
        assert r["n_bad"] == 0 and r["stages"] == 2 and m["iterations"] <= 10 and r["iterations"] <= 10
    r = by["few_left"][1]
    sc = dict(M.PARITY_SCENES)["few_left"]
    assert r["stages"] == 1 and r["n_inliers"] == 0 and r["n_correspondences"] - r["n_bad"] < 10
    q0, t0, s0 = M.state_from_floats(sc["R12"], sc["t12"], sc["s12"])
    assert np.array_equal(r["R12_d"], M.quat_to_matrix(q0)) and np.array_equal(r["t12_d"], t0) and r["s12_d"] == s0
    assert by["bad_octaves"][1]["n_bad_index"] == 3
    for n in M.PARITY_SIZES:  # fixed scale: the scale leaves as it came, bit for bit
        assert by["n%d_fix1" % n][1]["s12_d"] == 1.0


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[2], b[2])


def test_same_bytes_alone_in_a_batch_and_through_every_flavour(G, torch, F):
    sc = M.make_scene(200, 4242)
    rng = np.random.default_rng(1)
    others = [M.make_scene(int(n), 5000 + i, fix_scale=bool(i & 1)) for i, n in enumerate(rng.integers(1, 400, 31))]
    alone = F.run_batch(torch, [sc])[0]
    again = F.run_batch(torch, [sc])[0]
    assert alone[1]["stages"] == 2 and alone[1]["n_inliers"] > 100
    assert _same(alone, again)
    for pos in (0, 15, 31):
        got = F.run_batch(torch, others[:pos] + [sc] + others[pos:])[pos]
        assert _same(got, alone), pos
    # single-problem device entry
    p, d = F.upload(torch, sc)
    G.sim3_optimize_device(p, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _same(F.download(d, len(sc["valid"])), alone)
    # host flavour
    ni, inl, res = G.sim3_optimize(sc["valid"], sc["Xw1"], sc["Xw2"], sc["octave1"], sc["octave2"], sc["kp1_xy"], sc["kp2_xy"],
                                   sc["T1w"], sc["T2w"], sc["K1"], sc["K2"], sc["inv_level_sigma2"], sc["R12"], sc["t12"],
                                   sc["s12"], th2=sc["th2"], fix_scale=sc["fix_scale"],
                                   inlier=np.full(len(sc["valid"]), F.SENTINEL, np.uint8))
    ref = alone[1]
    assert ni == ref["n_inliers"] and np.array_equal(inl, alone[2])
    assert all(np.array_equal(res[k], ref[k]) for k in ref)


def test_spill_path_gives_the_same_bytes():
    """ORBGPU_DEBUG_SIM3OPT_LDS_PAIRS=0 sends every problem through the global-memory spill; a fresh process each, so
    that the hook is read at its first call."""
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import torch, fuzz_sim3opt as F, sim3opt_model as M\nfrom orb_slam2_map_amd import lib as G\n"
            "sc = [M.make_scene(n, 900 + n, fix_scale=bool(n & 1)) for n in (1, 40, 257, 300)]\n"
            "got = F.run_batch(torch, sc)\n"
            "print('SPILLS', G.sim3_opt_last_spills())\n"
            "print('BYTES', ''.join(g[0].hex() + g[2].tobytes().hex() for g in got))\n") % (
                ROOT, HERE, os.path.join(ROOT, "tools"))
    outs = []
    for lim in (None, "0"):
        env = dict(os.environ)
        env.pop("ORBGPU_DEBUG_SIM3OPT_LDS_PAIRS", None)
        if lim is not None:
            env["ORBGPU_DEBUG_SIM3OPT_LDS_PAIRS"] = lim
        r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        outs.append({l.split()[0]: l.split()[1] for l in r.stdout.splitlines() if l.startswith(("SPILLS", "BYTES"))})
    assert outs[0]["SPILLS"] == "0" and outs[1]["SPILLS"] == "4"
    assert outs[0]["BYTES"] == outs[1]["BYTES"]


def test_limits_empty_invalid_and_non_finite_rows(G, torch, F):
    empty = M.make_scene(5, 61)
    for k in F.ROWS:
        empty[k] = empty[k][:0]
    none_valid = M.make_scene(40, 62)
    none_valid["valid"] = np.zeros_like(none_valid["valid"])
    nan_row = M.make_scene(120, 63)
    v = np.flatnonzero(nan_row["valid"])
    for k in ("Xw1", "Xw2"):  # both world positions: both of the row's chi2 are NaN
        nan_row[k] = nan_row[k].copy()
        nan_row[k][v[4]] = np.nan
    plain = [M.make_scene(70, 64), M.make_scene(150, 65, fix_scale=True)]
    scenes = [plain[0], empty, none_valid, nan_row, plain[1]]
    got = F.run_batch(torch, scenes)
    for i in (1, 2):
        r = got[i][1]
        assert r["n_correspondences"] == r["n_inliers"] == r["stages"] == r["iterations"] == 0
        assert np.all(got[i][2] == F.SENTINEL)
        q0, t0, s0 = M.state_from_floats(scenes[i]["R12"], scenes[i]["t12"], scenes[i]["s12"])
        assert np.array_equal(r["R12_d"], M.quat_to_matrix(q0)) and np.array_equal(r["t12_d"], t0) and r["s12_d"] == s0
    # the NaN row: the call returned; the counts follow IEEE through the model (a NaN chi2 is not > th2: never cleared)
    m = M.optimize_sim3(nan_row)
    r = got[3][1]
    assert all(r[k] == m[k] for k in M.DISCRETE), (r, m)
    want = np.where(m["inlier"] == 255, F.SENTINEL, m["inlier"]).astype(np.uint8)
    assert np.array_equal(got[3][2], want) and got[3][2][v[4]] == 1
    # nothing else in the batch changed, and rows that are no correspondence keep the sentinel
    alone = F.run_batch(torch, plain)
    assert _same(got[0], alone[0]) and _same(got[4], alone[1])
    for sc, g in zip(scenes, got):
        assert np.all(g[2][np.asarray(sc["valid"]) == 0] == F.SENTINEL)
    rep = F.compare(plain, [got[0], got[4]])
    assert rep["left_out"] == 0 and not rep["mismatches"], rep["mismatches"]

"""Optimizer::OptimizeEssentialGraph on the device (orbgpu_essential_graph*) against the float64 restatement in eg_model.py
-- vs CPU restatement; g2o boundary unpinned.  Over the committed PARITY_SCENES (none left out: test_eg_model.py asserts
that none of them flips a discrete output) in ONE batched call the discrete outputs are compared exactly, every state
within 16 x the model's own spread (8 permutations of the summation order plus libm_nudge = +-1, largest over the set:
measured, never fixed in advance), Tiw and the corrected points as the exact G10 / G11 formulas on the device's own
doubles; then determinism and the three flavours as bytes, permuted rows, graphs without a fixed vertex, the stop flag and
the point kernel's sizes."""
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

import eg_model as M  # noqa: E402

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
    import fuzz_eg
    return fuzz_eg


@pytest.fixture(scope="module")
def parity(G, torch, F):
    """The whole committed set in one batched call, the model on every scene and the set's spread: computed once."""
    names = [n for n, _ in M.PARITY_SCENES]
    scenes = [s for _, s in M.PARITY_SCENES]
    got = F.run_batch(torch, scenes)
    rep = F.compare_parity(names, scenes, got)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "eg_parity.json"), "w") as f:
        json.dump({"note": "vs CPU restatement; g2o boundary unpinned", "scenes": len(scenes), "left_out": 0,
                   "model_spread": rep["spread"], "model_runs_with_a_discrete_flip": rep["flips"],
                   "device_max_deviation": rep["device_dev"], "allowed": 16 * rep["spread"], "mismatches": rep["mismatches"],
                   "per_scene": rep["per_scene"]}, f, indent=1)
    print("eg parity: %d scenes, model spread %.3e, device deviation %.3e, %d mismatches" % (
        len(scenes), rep["spread"], rep["device_dev"], len(rep["mismatches"])))
    for n in names:
        print("  %-32s spread %.3e device %.3e" % (n, rep["per_scene"][n]["model_spread"], rep["per_scene"][n]["device_deviation"]))
    return {"names": names, "scenes": scenes, "got": got, "rep": rep, "by": dict(zip(names, got)),
            "model": {n: F.reference(s, 8, "parity-" + n)[0] for n, s in zip(names, scenes)}}


def test_parity_with_the_model_over_the_committed_scenes(parity):
    rep = parity["rep"]
    assert rep["flips"] == 0  # nothing may be left out
    assert not rep["mismatches"], rep["mismatches"][:10]


def test_parity_set_covers_every_shape_and_branch(parity):
    by, model = parity["by"], parity["model"]
    W = M.THREADS
    assert {model[n]["n_edges"] for n in model} >= {1, 63, 64, 65, W - 1, W, W + 1}
    nf = {model[n]["n_free_active"] for n in model}
    assert {9, 10, 73, 74} <= nf and 7 * 9 < 64 < 7 * 10 and 7 * 73 < W < 7 * 74
    # counters from the model: all four cases of G3, all four of O5, a rejected trial, a failed pivot
    logs = sum(np.asarray(model[n]["log_cases"]) for n in model)
    exps = sum(np.asarray(model[n]["exp_cases"]) for n in model)
    assert (logs > 0).all() and (exps > 0).all(), (logs, exps)
    assert any("r" in model[n]["trace"] for n in model) and "p" in model["failed_pivot"]["trace"]
    r = by["failed_pivot"][1]
    assert r["iterations"] == r["trials"] == 3 and np.isnan(r["chi2_end"])
    # the shapes
    assert by["v2_one_edge"][1]["n_edges"] == 1 and by["v2_one_edge"][1]["n_free_active"] == 1
    r = by["parallel_fixed_pair_bad_edges"][1]
    assert r["n_bad_index"] == 3 and r["n_edges"] == len(dict(M.PARITY_SCENES)["parallel_fixed_pair_bad_edges"]["edge_i"]) - 3
    assert r["n_bad_ref"] == 2
    r = by["two_components_isolated"][1]
    assert r["n_free_active"] == 12 - 2 - 1  # two fixed rows, one isolated
    for n in ("iterations0", "iterations1"):
        assert by[n][1]["iterations"] == by[n][1]["trials"] == int(n[-1])
    r, a = by["iterations0"][1], by["iterations0"][2]
    sc = dict(M.PARITY_SCENES)["iterations0"]
    assert r["chi2_start"] == r["chi2_end"] > 0 and a["Siw_d"].tobytes() == np.asarray(sc["Scw"], np.float64).tobytes()
    assert np.array_equal(a["Tiw"], M.tiw_of(sc["Scw"]))
    for n, sc in M.PARITY_SCENES:
        a = by[n][2]
        fixed = np.asarray(sc["fixed"]) != 0
        assert a["Siw_d"][fixed].tobytes() == np.asarray(sc["Scw"], np.float64)[fixed].tobytes(), n  # a fixed row leaves bit-equal
        if sc["fix_scale"]:  # every scale exactly as it came
            assert a["Siw_d"][:, 7].tobytes() == np.asarray(sc["Scw"], np.float64)[:, 7].tobytes(), n
        assert by[n][1]["envelope"] >= 28 * by[n][1]["n_free_active"] and by[n][1]["bandwidth"] % 7 == 0
    assert by["ring40_fix0"][1]["bandwidth"] <= 7 * (2 * 2 + 2)  # reach 2: at most 2 x 2 + 1 blocks off the diagonal (test_skyline.py)


def _same(a, b):
    return a[0] == b[0] and a[1] == b[1]


def test_same_bytes_alone_in_a_batch_and_through_every_flavour(G, torch, F):
    sc = M.make_scene(16, 4242, reach=2, fix_scale=True, n_iterations=3, n_points=50)
    rng = np.random.default_rng(1)
    others = [M.make_scene(int(n), 5000 + i, fix_scale=bool(i & 1), n_iterations=2) for i, n in enumerate(rng.integers(2, 30, 12))]
    alone = F.run_batch(torch, [sc])[0]
    again = F.run_batch(torch, [sc])[0]
    assert alone[1]["iterations"] == M.essential_graph(sc)["iterations"] == 3 and alone[1]["chi2_end"] < alone[1]["chi2_start"]
    assert _same(alone, again)
    for pos in (0, 5, 12):
        got = F.run_batch(torch, others[:pos] + [sc] + others[pos:])[pos]
        assert _same(got, alone), pos
    # single-problem device entry
    p, d = F.upload(torch, sc)
    G.essential_graph_device(p, stream=torch.cuda.current_stream().cuda_stream)
    F.correct_points(torch, sc, d)
    torch.cuda.synchronize()
    assert _same(F.download(d, sc), alone)
    # host flavour
    Sd, T, pos, res = G.essential_graph(F.to_problem(sc), world_pos=sc["world_pos"], point_ref=sc["point_ref"])
    assert res == alone[1]
    assert Sd.tobytes() == alone[2]["Siw_d"].tobytes() and T.tobytes() == alone[2]["Tiw"].tobytes()
    assert pos.tobytes() == alone[2]["pos"].tobytes()


def test_permuted_rows_agree_within_the_parity_tolerance(parity, torch, F):
    sc = dict(M.PARITY_SCENES)["ring8_fix0"]
    V = len(sc["Scw"])
    perm = np.random.default_rng(5).permutation(V)  # old row v becomes row perm[v]
    inv = np.argsort(perm)
    ps = dict(sc)
    ps["Scw"], ps["Snc"], ps["fixed"] = sc["Scw"][inv], sc["Snc"][inv], sc["fixed"][inv]
    ps["edge_i"], ps["edge_j"] = perm[sc["edge_i"]].astype(np.int32), perm[sc["edge_j"]].astype(np.int32)
    ps["point_ref"] = perm[sc["point_ref"]].astype(np.int32)
    got = F.run_batch(torch, [ps])[0]
    base = parity["by"]["ring8_fix0"]
    assert all(got[1][k] == base[1][k] for k in F.EG_COUNTERS)
    dev = F._dev(got[2]["Siw_d"][perm], base[2]["Siw_d"])
    assert dev <= 16 * parity["rep"]["spread"], dev
    assert np.abs(got[2]["pos"].astype(np.float64) - base[2]["pos"]).max() <= 16 * parity["rep"]["spread"] + 2.0 ** -19  # one float rounding on each side, |x| < 32


def test_graphs_without_a_fixed_vertex_return_and_repeat(torch, F):
    """No parity is claimed: the gauge is held by lambda = 1e-16 alone."""
    scenes = []
    for V, seed in ((2, 70), (6, 71), (20, 72)):
        sc = M.make_scene(V, seed, n_iterations=4, n_points=7)
        sc["fixed"] = np.zeros(V, np.uint8)
        scenes.append(sc)
    a, b = F.run_batch(torch, scenes), F.run_batch(torch, scenes)
    for sc, x, y in zip(scenes, a, b):
        r = x[1]
        assert _same(x, y)
        assert r["n_free_active"] == len(sc["Scw"]) and r["n_edges"] == len(sc["edge_i"]) and r["n_bad_index"] == 0
        assert 1 <= r["iterations"] <= 4 and r["iterations"] <= r["trials"] <= 10 * r["iterations"] and r["stopped"] == 0
        assert r["envelope"] >= 28 * r["n_free_active"] and 7 <= r["bandwidth"] <= 7 * r["n_free_active"]


def test_stop_flag_set_at_the_call_writes_nothing_but_the_result(G, torch, F):
    sc = M.make_scene(9, 81, n_iterations=5, n_points=12)
    plain = M.make_scene(7, 82, n_iterations=2)
    got = F.run_batch(torch, [plain, sc, plain], stops=[0, 1, None])
    r, a = got[1][1], got[1][2]
    assert r["stopped"] == 1 and r["iterations"] == r["trials"] == 0 and r["n_edges"] == len(sc["edge_i"])
    assert np.all(a["Siw_d"] == F.SENTINEL) and np.all(a["Tiw"] == F.SENTINEL)
    assert _same(got[0], got[2]) and got[0][1]["stopped"] == 0 and got[0][1]["iterations"] == 2
    # host flavour: the arrays come back as they went in
    Sd0, T0 = np.full((9, 8), 3.0), np.full((9, 4, 4), 5.0, np.float32)
    P0 = np.full((12, 3), 9.0, np.float32)
    Sd, T, pos, res = G.essential_graph(F.to_problem(sc), stop=1, Siw_d=Sd0, Tiw=T0, world_pos=sc["world_pos"],
                                        point_ref=sc["point_ref"], pos_out=P0)
    assert res["stopped"] == 1 and res["iterations"] == 0 and res["n_bad_ref"] == 0
    assert np.array_equal(Sd, Sd0) and np.array_equal(T, T0) and np.array_equal(pos, P0)
    Sd, T, pos, res = G.essential_graph(F.to_problem(sc), stop=0, Siw_d=Sd0, Tiw=T0, world_pos=sc["world_pos"],
                                        point_ref=sc["point_ref"], pos_out=P0)
    assert res["stopped"] == 0 and res["iterations"] >= 1 and not np.any(Sd == 3.0) and not np.any(pos == 9.0)


@pytest.mark.parametrize("n_points", [1, 255, 256, 257, 70000])
def test_point_correction_sizes(G, torch, F, n_points):
    """One point per lane over more than one workgroup; refs to a fixed row among them and two out of range."""
    sc = M.make_scene(8, 90, n_iterations=2)
    M.add_points(sc, n_points, 91)
    ref = sc["point_ref"]
    ref[:: max(n_points // 11, 1)] = 0  # the fixed row
    bad = [] if n_points == 1 else [n_points // 3, n_points - 1]
    for k, b in enumerate(bad):
        ref[b] = (-1, 8)[k]
    got = F.run_batch(torch, [sc])[0]
    m = M.essential_graph(sc)
    assert got[1]["n_bad_ref"] == len(bad) == m["n_bad_ref"]
    v = F.as_rule_arrays(got[2]["Siw_d"], got[2]["Tiw"], got[2]["pos"], sc)
    assert F._ulp(v["pos"], v["pos_d"].astype(np.float32)) == 0  # the exact G11 formula on the device's own doubles
    for b in bad:
        assert got[2]["pos"][b].tobytes() == sc["world_pos"][b].tobytes()
    fixed_row = ref == 0  # its state never moves, so G11 is Scw^-1 map (Scw map P): the model's bits
    assert np.array_equal(got[2]["pos"][fixed_row], m["pos"][fixed_row])
    # in place: pos_out may be the input array
    d = F.upload(torch, sc)[1]
    Siw = torch.from_numpy(got[2]["Siw_d"]).cuda()
    G.essential_graph_correct_points_device(8, d["Scw"].data_ptr(), Siw.data_ptr(), n_points, d["pos_in"].data_ptr(),
                                            d["ref"].data_ptr(), d["pos_in"].data_ptr(), None,
                                            stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert d["pos_in"].cpu().numpy().tobytes() == got[2]["pos"].tobytes()

"""The float64 ladder of tests/init_fp64.py without a device: the restatement (init_model.initialize) stands where the device
will stand.  Every scene is inside the caps and the margins, every committed tolerance is 16 x the largest figure measured
here (one digit, rounded up), and the ladder bites: each mutation of a correct result is reported by the rung that is
meant to see it and by no earlier one.  The figures go to profiles/init_fp64.json (column "restatement")."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import init_fp64 as L  # noqa: E402
import init_model as M  # noqa: E402

f32 = np.float32
PROFILE = os.path.join(ROOT, "profiles", "init_fp64.json")
RESULT = ("best_h", "best_f", "SH", "SF", "RH", "used_homography", "n_inliers", "n_good", "cos_parallax", "best_motion",
          "second_best_good", "success", "H21", "F21", "R21", "t21", "scores_h", "scores_f", "masks_h", "masks_f", "P3D", "triangulated")


def as_result(m):
    """the restatement's output under the keys of tools/fuzz_init.download"""
    r = {k: copy.deepcopy(m[k]) for k in RESULT}
    r.update(n=m["N"], n_bad_index=m["n_bad_index"], n_bad_set=m["n_bad_set"], R21_out=m["R21"].copy(), t21_out=m["t21"].copy())
    return r


def model_copies(m):
    """what the single-hypothesis copies of a scene give: hypothesis h alone wins both scans iff its scores are > 0.  The
    restatement computes a hypothesis from its own set only, so its rows are taken instead of 24 further passes."""
    out = []
    for h in range(len(m["scores_h"])):
        wh, wf = bool(m["scores_h"][h] > 0), bool(m["scores_f"][h] > 0)
        out.append({"scores_h": m["scores_h"][h:h + 1].copy(), "scores_f": m["scores_f"][h:h + 1].copy(),
                    "masks_h": m["masks_h"][h:h + 1].copy(), "masks_f": m["masks_f"][h:h + 1].copy(),
                    "best_h": 0 if wh else -1, "best_f": 0 if wf else -1,
                    "H21": m["mats_h"][h].copy() if wh else np.zeros((3, 3), f32),
                    "F21": m["mats_f"][h].copy() if wf else np.zeros((3, 3), f32)})
    return out


def model_wide_copies(m):
    """the copies with WIDE_SIGMA: every finite matrix wins alone.  The restatement's matrices do not know sigma."""
    out = []
    for h in range(len(m["scores_h"])):
        ok = [bool(np.isfinite(m[k][h]).all() and m[k][h].any()) for k in ("mats_h", "mats_f")]
        out.append({"scores_h": np.array([1.0 if ok[0] else 0.0], f32), "scores_f": np.array([1.0 if ok[1] else 0.0], f32),
                    "H21": m["mats_h"][h].copy() if ok[0] else np.zeros((3, 3), f32),
                    "F21": m["mats_f"][h].copy() if ok[1] else np.zeros((3, 3), f32)})
    return out


@pytest.fixture(scope="module")
def limits():
    """I10's cosine limits from the library's host-only entry point (no device is needed)"""
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "orb_slam2_map_amd", "liborbgpu.so")):
        ge.build()
    from orb_slam2_map_amd import lib
    cache = {}
    return lambda mp: cache.setdefault(float(mp), lib.initializer_cos_limits(float(mp)))


@pytest.fixture(scope="module")
def runs(limits):
    """name -> (scene, result, copies, ladder), computed once and never changed"""
    out = {}
    for name, sc in L.scenes().items():
        m = M.initialize(sc)
        r, copies, wide = as_result(m), model_copies(m), model_wide_copies(m)
        out[name] = (sc, r, (copies, wide), L.ladder(sc, r, copies, limits(sc.get("min_parallax", 1.0)), name, wide=wide))
    L.record(PROFILE, "restatement", {k: L.figures(v[3]) for k, v in out.items()})
    return out


SCENES = list(L.scenes())


@pytest.mark.parametrize("name", SCENES)
def test_restatement_passes_every_rung_inside_the_caps(runs, name):
    sc, r, (copies, wide), rungs = runs[name]
    fig = L.figures(rungs)
    print(name, {k: ("%.2e" % v if isinstance(v, float) else v) for k, v in fig.items()}, "branch", "H" if r["used_homography"] else "F",
          "success", r["success"])
    assert L.violations(rungs) == []
    H = len(sc["sets"])
    assert fig["skipped"] <= L.CAP_SKIPPED * 2 * H * r["n"] and fig["matrixless"] <= L.CAP_MATRIXLESS * 2 * H
    # in full: every hypothesis with a matrix went through rungs 1-3
    assert 2 * H - len(L.hypotheses(r, copies, wide)) <= fig["matrixless"] + (2 if name == L.DEGENERATE else 0)


def test_the_scene_list_reaches_both_branches_and_the_edges(runs):
    got = {k: (v[1]["used_homography"], v[1]["success"]) for k, v in runs.items()}
    assert got["general-300-101"] == (0, 1) and got["general-300-104"] == (0, 1)
    assert got["planar-300-103"] == (1, 1) and got["planar-300-107"] == (1, 1) and got["parity-planar"] == (1, 1)
    assert got["ngood-51"][1] == 1 and runs["ngood-51"][1]["n_good"].max() == 51
    assert sorted(v[1]["n"] for k, v in runs.items() if k.startswith("edge-")) == [8, 9, 63, 64, 65, 129]
    assert sum(1 for v in got.values() if not v[1]) >= 4              # failures are checked too (everything zero, the rule)
    rep = runs[L.DEGENERATE]
    assert len(set(rep[0]["sets"][2].tolist())) == 1


def test_the_copies_as_the_device_test_runs_them(runs, limits):
    """planar/65/107 (16 of its 24 homographies score 0) through with_copies / split_copies with a pass of the restatement
    per copy, as the device test's batched call does it: the same ladder, the same figures, and every hypothesis that
    scores 0 shows its matrix at the wide sigma"""
    name = "planar-65-107"
    sc, r0, (copies0, _), rungs0 = runs[name]
    r, copies, wide = L.split_copies([as_result(M.initialize(c)) for c in L.with_copies(sc)])
    assert sum(1 for c in copies if not c["scores_h"][0] > 0) == 16 and all(w["scores_h"][0] > 0 and w["scores_f"][0] > 0 for w in wide)
    rungs = L.ladder(sc, r, copies, limits(1.0), name, wide=wide)
    assert L.violations(rungs) == [] and L.figures(rungs) == L.figures(rungs0)
    assert all(c["H21"].tobytes() == c0["H21"].tobytes() and c["F21"].tobytes() == c0["F21"].tobytes() for c, c0 in zip(copies, copies0))


def test_tolerances_are_16_times_the_restatement(runs):
    largest = {k: max(L.figures(v[3])[k] for v in runs.values()) for k in L.TOLERANCES}
    print({k: "%.3e" % v for k, v in largest.items()})
    for k, const in L.TOLERANCES.items():
        assert largest[k] > 0.0, k
        assert getattr(L, const) == L.round_up_one_digit(L.BOUND_FACTOR * largest[k]), (const, largest[k])
    assert L.BOUND_FACTOR == M.BOUND_FACTOR
    assert [L.round_up_one_digit(x) for x in (1.28e-5, 2e-5, 9.01e-7, 9.6e-3, 0.0)] == [2e-5, 2e-5, 1e-6, 1e-2, 0.0]


# ---- the ladder must bite ------------------------------------------------------------------------------------------------
F_SCENE, H_SCENE = "general-300-101", "planar-300-103"


def _first_rung(rungs):
    for k in L.RUNGS:
        if k in rungs and rungs[k][0]:
            return k
    return None


def _mutated(runs, limits, name, mutate):
    sc, r, (copies, wide), _ = runs[name]
    r, copies, wide = copy.deepcopy(r), copy.deepcopy(copies), copy.deepcopy(wide)
    prep = M.prepare(sc)
    mutate(sc, prep, r, copies, wide)
    rungs = L.ladder(sc, r, copies, limits(sc.get("min_parallax", 1.0)), name, wide=wide)
    return rungs, L.violations(rungs)


def _other(r, key):
    """the best hypothesis that did not win"""
    return max((h for h in range(len(r[key])) if h not in (r["best_h"], r["best_f"])), key=lambda h: r[key][h])


def _rt(sc, prep, r):
    c = L.check_rt64(sc, prep, r["R21"].astype(float), r["t21"].astype(float), L.unpack(L.selected_row(r), prep["N"])[0])
    return c, prep["first"][c["e"]]


@pytest.mark.parametrize("name", [F_SCENE, H_SCENE])
@pytest.mark.parametrize("model", ["h", "f"])
def test_mutation_matrix_entry(runs, limits, name, model):
    def mutate(sc, prep, r, copies, wide):
        h, mk = _other(r, "scores_" + model), "H21" if model == "h" else "F21"
        at = (0, 0) if model == "h" else (1, 2)     # an entry that a pixel coordinate of some hundreds multiplies
        for c in (copies[h], wide[h]):          # wherever the hypothesis shows its matrix
            c[mk][at] *= f32(1.0 + 1e-4)
    rungs, bad = _mutated(runs, limits, name, mutate)
    assert _first_rung(rungs) == ("rung1" if model == "h" else "rung2") and rungs["rung3"][0], bad


@pytest.mark.parametrize("name", [F_SCENE, H_SCENE])
@pytest.mark.parametrize("model", ["h", "f"])
def test_mutation_mask_bit(runs, limits, name, model):
    def mutate(sc, prep, r, copies, wide):
        h = _other(r, "scores_" + model)
        chi1, chi2 = L.chi_squares(prep, model, copies[h]["H21" if model == "h" else "F21"].astype(float), 1.0)
        e = int(np.flatnonzero((chi1 < 1.0) & (chi2 < 1.0))[0])          # a clear inlier
        for row in (r["masks_" + model][h], copies[h]["masks_" + model][0]):
            row[e // 64] ^= np.uint64(1) << np.uint64(e % 64)
    rungs, bad = _mutated(runs, limits, name, mutate)
    assert _first_rung(rungs) == "rung3" and "mask bits wrong" in bad[0], bad


@pytest.mark.parametrize("name", [F_SCENE, H_SCENE])
@pytest.mark.parametrize("model", ["h", "f"])
def test_mutation_score_term(runs, limits, name, model):
    def mutate(sc, prep, r, copies, wide):
        # one term of at most 5.991 has to show beside the score's own rounding (TOL_SCORE x the score, or TOL_SCORE_PX
        # over a lever that grows with the inliers): the hypothesis where it shows best, one with few inliers
        k, mk = "scores_" + model, "H21" if model == "h" else "F21"
        chi = {h: L.chi_squares(prep, model, copies[h][mk].astype(float), 1.0)[0].min() for h in range(len(r[k])) if r[k][h] > 0}
        h = max(chi, key=lambda h: (L.TH_SCORE - chi[h]) - L.TOL_SCORE * max(1.0, r[k][h]))
        term = f32(L.TH_SCORE - chi[h])
        assert term > 3.0
        r[k][h] -= term
        copies[h][k][0] -= term
        for key, b in (("SH", "best_h"), ("SF", "best_f")):          # keep the scans consistent where it had won
            if key[1].lower() == model and r[b] == h:
                r[key] = r[k][h]
    rungs, bad = _mutated(runs, limits, name, mutate)
    assert _first_rung(rungs) == "rung3" and "score" in bad[0], bad


@pytest.mark.parametrize("name", [F_SCENE, H_SCENE])
def test_mutation_best_f(runs, limits, name):
    def mutate(sc, prep, r, copies, wide):
        s = r["scores_f"].copy()
        s[r["best_f"]] = -1
        r["best_f"] = int(np.argmax(s))
    rungs, bad = _mutated(runs, limits, name, mutate)
    assert _first_rung(rungs) == "rung4", bad


def test_mutation_twin_rotation(runs, limits):
    def mutate(sc, prep, r, copies, wide):
        mot, _ = L.motions_f64(sc, r["F21"].astype(float))
        twin = max((mot[0][0], mot[1][0]), key=lambda R: np.abs(R - r["R21"]).max())
        r["R21"] = twin.astype(f32)
        r["R21_out"] = r["R21"].copy()
    rungs, bad = _mutated(runs, limits, F_SCENE, mutate)
    assert _first_rung(rungs) == "rung6", bad


@pytest.mark.parametrize("name", [F_SCENE, H_SCENE])
def test_mutation_t_negated(runs, limits, name):
    def mutate(sc, prep, r, copies, wide):
        r["t21"] = -r["t21"]
        r["t21_out"] = r["t21"].copy()
    rungs, bad = _mutated(runs, limits, name, mutate)
    assert _first_rung(rungs) == "rung6", bad


@pytest.mark.parametrize("name", [F_SCENE, H_SCENE])
def test_mutation_point_moved(runs, limits, name):
    def mutate(sc, prep, r, copies, wide):
        c, rows = _rt(sc, prep, r)
        i = int(np.argmax(np.where(c["ok"], c["gap"], 0.0)))            # the best-conditioned point
        r["P3D"][rows[i]] *= f32(1.0 + 1e-3)
    rungs, bad = _mutated(runs, limits, name, mutate)
    assert _first_rung(rungs) == "rung6" and "a point is" in bad[0], bad


@pytest.mark.parametrize("name", [F_SCENE, H_SCENE])
def test_mutation_cosine_rank(runs, limits, name):
    def mutate(sc, prep, r, copies, wide):
        c, _ = _rt(sc, prep, r)
        cs = np.sort(c["cos"][c["ok"]])
        assert len(cs) > 51
        r["cos_parallax"][r["best_motion"]] = f32(cs[49])
    rungs, bad = _mutated(runs, limits, name, mutate)
    assert _first_rung(rungs) == "rung6" and "cos_parallax" in bad[0], bad


def _far_scene(base):
    """general/300/101 with three pairs, none of them in a set, moved to where the motion found in the scene (base: its
    result) sees points 300 baselines away: they pass CheckRT with cosParallax >= 0.99998, so they are written and counted
    and not triangulated (neither listed scene holds such a pair)"""
    sc = M.make_scene(300, 101, "general", n_hyp=24)
    K = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]])
    rows = np.flatnonzero(sc["matches12"] >= 0)
    keep = [e for e in np.flatnonzero(~sc["outlier"]) if e not in sc["sets"]][:3]
    for e in keep:
        x1 = np.linalg.inv(K) @ np.append(sc["kp1"][rows[e]].astype(float), 1.0) * 300.0
        x2 = K @ (base["R21"].astype(float) @ x1 + base["t21"].astype(float))
        sc["kp2"][sc["matches12"][rows[e]]] = (x2[:2] / x2[2]).astype(f32)
    return sc, keep


def test_mutation_triangulated_without_parallax(runs, limits):
    sc, keep = _far_scene(runs[F_SCENE][1])
    m = M.initialize(sc)
    r, copies, wide = as_result(m), model_copies(m), model_wide_copies(m)
    lim = limits(1.0)
    rungs = L.ladder(sc, r, copies, lim, wide=wide)
    assert L.violations(rungs) == [] and r["success"] == 1
    prep = M.prepare(sc)
    c, rows = _rt(sc, prep, r)
    flat = np.flatnonzero(c["ok"] & ~c["low"] & ~c["near"])
    assert len(flat) >= 1 and not r["triangulated"][rows[flat]].any() and r["P3D"][rows[flat]].any(1).all()
    r["triangulated"][rows[flat[0]]] = 1
    rungs = L.ladder(sc, r, copies, lim, wide=wide)
    assert _first_rung(rungs) == "rung6" and "triangulated flags wrong" in L.violations(rungs)[0]


@pytest.mark.parametrize("name,rung", [(H_SCENE, "rung6"), (F_SCENE, "rung5")])
def test_mutation_n_good(runs, limits, name, rung):
    """In the F branch rung 5 already holds all four counts to float64's CheckRT and speaks first; the H branch's counts
    are rung 6's alone."""
    def mutate(sc, prep, r, copies, wide):
        r["n_good"][r["best_motion"]] += 1
    rungs, bad = _mutated(runs, limits, name, mutate)
    assert _first_rung(rungs) == rung and (rung == "rung5" or "P3D holds" in bad[0]), bad
    if rung == "rung5":
        assert any("P3D holds" in b for b in bad)


@pytest.mark.parametrize("name", [F_SCENE, H_SCENE])
def test_mutation_success(runs, limits, name):
    """a refusal that is consistent in itself (everything zeroed, as after a failure): only the rule can tell"""
    def mutate(sc, prep, r, copies, wide):
        r["success"] = 0
        for k in ("P3D", "triangulated", "R21", "t21", "R21_out", "t21_out"):
            r[k] = np.zeros_like(r[k])
    rungs, bad = _mutated(runs, limits, name, mutate)
    assert _first_rung(rungs) == "rung7", bad

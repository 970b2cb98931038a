"""The Initializer on the device against float64, one stage at a time (tests/init_fp64.py): every
rung checks one stage on the device's own output of the stage before, so nothing is left out but single pairs within
float rounding of a threshold -- on scenes with the seeds as written, where the comparison with the restatement
(test_gpu_init.py) leaves out most hypotheses.  One batched call per scene holds the scene, one copy per hypothesis with
that hypothesis alone (its result carries the hypothesis's matrices) and the same copies with a wide sigma (a hypothesis
that scores 0 shows its matrix there).  The tolerances are the committed constants of init_fp64.py, 16 x what the
restatement costs against float64 (test_init_fp64.py); none is derived from the device's output.  The device's figures go
to profiles/init_fp64.json beside the restatement's."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import init_fp64 as L  # noqa: E402

pytestmark = pytest.mark.gpu

PROFILE = os.path.join(ROOT, "profiles", "init_fp64.json")
SCENES = L.scenes()
RUNS = {}


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
    import fuzz_init
    return fuzz_init


@pytest.fixture
def run(G, torch, F):
    """name -> (scene, result, copies, wide copies, ladder): one batched call and one ladder per scene, shared by the tests"""
    def get(name):
        if name not in RUNS:
            sc = SCENES[name]
            r, copies, wide = L.split_copies(F.run_batch(torch, L.with_copies(sc)))
            rungs = L.ladder(sc, r, copies, G.initializer_cos_limits(sc.get("min_parallax", 1.0)), name, wide=wide)
            fig = L.figures(rungs)
            fig.update(used_homography=int(r["used_homography"]), success=int(r["success"]), violations=len(L.violations(rungs)))
            L.record(PROFILE, "device", {name: fig})
            print(name, {k: ("%.2e" % v if isinstance(v, float) else v) for k, v in fig.items()})
            RUNS[name] = (sc, r, copies, wide, rungs)
        return RUNS[name]
    return get


def _clean(run, name, *rungs):
    got = run(name)[4]
    bad = [v for k in rungs for v in got[k][0]]
    assert not bad, bad[:10]
    return got


@pytest.mark.parametrize("name", list(SCENES))
def test_a_hypothesis_does_not_depend_on_its_neighbours(run, name):
    """rung 0: copy h's scores and mask rows have the bytes of row h; a matrix does not depend on sigma; at most 10 % of
    the hypotheses show no matrix at all; and every other one goes through rungs 1-3"""
    sc, r, copies, wide, rungs = run(name)
    assert r["n"] == L.prepare(sc)["N"] and len(copies) == len(wide) == len(sc["sets"]) == 24
    _clean(run, name, "copies")
    shown = len(L.hypotheses(r, copies, wide))
    assert 2 * 24 - shown <= rungs["copies"][1]["matrixless"] + (2 if name == L.DEGENERATE else 0)
    assert rungs["copies"][1]["matrixless"] <= L.CAP_MATRIXLESS * 48


@pytest.mark.parametrize("name", list(SCENES))
def test_dlt_is_optimal(run, name):
    """rungs 1, 2: every hypothesis's matrix minimises its set's DLT matrix; F has rank 2"""
    _clean(run, name, "rung1", "rung2")


@pytest.mark.parametrize("name", list(SCENES))
def test_checks(run, name):
    """rung 3: every mask bit and score from the hypothesis's own matrix"""
    got = _clean(run, name, "rung3")
    assert got["rung3"][1]["skipped"] <= L.CAP_SKIPPED * got["rung3"][1]["cells"]


@pytest.mark.parametrize("name", list(SCENES))
def test_selection_branch_and_inlier_count(run, name):
    """rung 4, exact"""
    _clean(run, name, "rung4")


@pytest.mark.parametrize("name", list(SCENES))
def test_motion(run, name):
    """rung 5"""
    _clean(run, name, "rung5")


@pytest.mark.parametrize("name", list(SCENES))
def test_check_rt_and_triangulation(run, name):
    """rung 6"""
    _clean(run, name, "rung6")


@pytest.mark.parametrize("name", list(SCENES))
def test_accept_rule(run, name):
    """rung 7, exact"""
    _clean(run, name, "rung7")


def test_both_branches_succeed_somewhere(run):
    """rungs 5 and 6 have something to check on either branch: these verdicts are far from every threshold"""
    for name, want in (("general-300-101", (0, 1)), ("general-300-104", (0, 1)), ("planar-300-103", (1, 1)), ("parity-planar", (1, 1)),
                       ("rotation-300-105", (None, 0))):
        r = run(name)[1]
        assert r["success"] == want[1] and want[0] in (None, r["used_homography"]), name
    r = run("ngood-51")[1]
    assert r["success"] == 1 and r["n_good"][r["best_motion"]] == 51        # the rank clamp: min(50, nGood - 1) = 50

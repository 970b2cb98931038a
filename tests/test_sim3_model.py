"""tests/sim3_model.py, the restatement of Sim3Solver.cc that the device entry points are compared with: it recovers a
planted similarity, and its conventions (include/orbgpu.h H1-H8) hold: truncated thresholds, the iteration formula, the
sampler's quirk, the acceptance rule across calls.  Also the CPU half of the device parity test: its committed scenes
stay inside the cap on left-out hypotheses."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import sim3_model as M  # noqa: E402


@pytest.mark.parametrize("fix_scale", [False, True])
def test_recovers_a_planted_similarity_from_noise_free_points(fix_scale):
    sc = M.make_scene(40, 3, fix_scale=fix_scale, outlier_frac=0.0, noise_px=0.0, n_hyp=6)
    m = M.solve(sc)
    tr = sc["true"]
    assert m["N"] == 40 and m["accepted"] == 0 and m["n_inliers"] == 40 and m["counts"][0] == 40
    assert np.abs(m["R"][0] - tr["R"]).max() < 2e-5 and np.abs(m["t"][0] - tr["t"]).max() < 2e-4
    assert abs(m["s"][0] - tr["s"]) < 2e-5 and (not fix_scale or m["s"][0] == np.float32(1.0))
    assert np.array_equal(m["T12"][0][:3, :3], m["s"][0] * m["R"][0]) and np.array_equal(m["T12"][0][:3, 3], m["t"][0])
    # the mask is indexed by i1
    bits = np.unpackbits(m["masks"][0].view(np.uint8), bitorder="little")[:len(sc["valid"])]
    assert np.array_equal(bits, sc["valid"])


def test_the_sign_of_the_quaternion_does_not_matter():
    sc = M.make_scene(30, 11)
    p = M.prepare(sc)
    for h in range(20):
        a = M.horn(p["X1"][sc["triples"][h]], p["X2"][sc["triples"][h]], False)
        b = M.horn(p["X1"][sc["triples"][h]], p["X2"][sc["triples"][h]], False, flip=True)
        assert np.abs(a["R_d"] - b["R_d"]).max() < 1e-12
        assert np.array_equal(b["q"], -a["q"])


def test_jacobi_agrees_with_eigh_and_is_orthogonal():
    rng = np.random.default_rng(0)
    for _ in range(20):
        A = rng.normal(size=(4, 4))
        A = A + A.T
        w, V = M.jacobi4(A)
        assert np.abs(V.T @ V - np.eye(4)).max() < 1e-14 and np.abs(V @ np.diag(w) @ V.T - A).max() < 1e-13
        assert np.abs(np.sort(w) - np.linalg.eigvalsh(A)).max() < 1e-13
    w, V = M.jacobi4(np.zeros((4, 4)))
    assert not w.any() and np.array_equal(V, np.eye(4))  # a repeated point three times: q = (1, 0, 0, 0), then NaN
    assert np.isnan(M.rotation_from_quaternion(V[:, 0])).all()


def test_thresholds_are_truncated():
    e = M.max_errors(M.SIGMA2)
    assert e.dtype == np.float32 and list(e[:4]) == [9.0, 13.0, 19.0, 27.0]  # 9.21, 13.26, 19.10, 27.50
    assert list(M.max_errors(np.array([-1.0, np.nan, 0.0], np.float32))) == [0.0, 0.0, 0.0]


def test_an_octave_out_of_range_is_not_kept():
    sc = M.make_scene(10, 2)
    i = np.flatnonzero(sc["valid"])[4]
    sc["octave2"][i] = M.NLEVELS
    p = M.prepare(sc)
    assert p["N"] == 9 and p["n_bad_index"] == 1 and i not in p["indices1"] and np.all(np.diff(p["indices1"]) > 0)


def test_ransac_iterations():
    assert M.ransac_iterations(100, 0.99, 20, 300) == 300
    assert M.ransac_iterations(25, 0.99, 20, 300) == 7
    assert M.ransac_iterations(20, 0.99, 20, 300) == 1
    assert M.ransac_iterations(0, 0.99, 20, 300) == 1
    assert M.ransac_iterations(50, 1.0, 6, 300) == 300   # log(0) / x = +inf: larger than max_iterations
    assert M.ransac_iterations(7, 1.5, 3, 10) == 10      # log of a negative: NaN
    assert M.ransac_iterations(10 ** 6, 0.99, 1, 300) == 300  # log(1 - 0) = 0: x / 0 = -inf
    assert M.ransac_iterations(30, 0.5, 29, 0) == 1
    sc = M.make_scene(19, 5)
    m = M.solve(sc)
    assert m["N"] == 19 and m["no_more"] and m["n_use"] == 0 and m["iterations"] == 0 and not m["counts"].any()


def test_the_sampler_replays_the_reference_quirk():
    # N = 5, RandomInt returns 1 three times: [0 1 2 3 4] -> pick 1, position 1 <- 4 -> [0 4 2 3] -> pick 4, position FOUR
    # <- 3 (not position 1) -> [0 4 2] -> pick 4 again
    seq = iter([1, 1, 1])
    assert M.sample_triples(5, 1, lambda lo, hi: next(seq)).tolist() == [[1, 4, 4]]
    # N = 4: pick 0 -> [3 1 2]; pick position 0 = 3, write at position 3 = size() after the pop; pick position 1 = 1
    seq = iter([0, 0, 1])
    assert M.sample_triples(4, 1, lambda lo, hi: next(seq)).tolist() == [[0, 3, 1]]
    # through the reference's RandomInt: rand() = 0.4 * 2^31 gives 1 for d = 5, 4 and 3
    r = M.reference_random_int(lambda: 858993459)
    assert [r(0, 4), r(0, 3), r(0, 2), r(2, 2)] == [1, 1, 1, 2]
    assert M.sample_triples(5, 2, r).tolist() == [[1, 4, 4], [1, 4, 4]]
    lim = []
    M.sample_triples(9, 1, lambda lo, hi: lim.append((lo, hi)) or 0)
    assert lim == [(0, 8), (0, 7), (0, 6)]


def test_the_acceptance_scan_resumes_across_calls():
    counts = np.array([5, 3, 21, 4, 4, 20, 21, 30, 2, 22, 1, 1], np.int32)
    st = M.RansacState(100, 20, 12)
    assert st.iterate(5, counts) == (2, 21, False) and st.iterations == 3 and st.best == 21
    # after a success that OptimizeSim3 rejected: 20 is not >= best, the second 21 is (>=, not >) and is > min_inliers
    assert st.iterate(5, counts) == (6, 21, False) and st.iterations == 7
    assert st.iterate(1, counts) == (7, 30, False)
    assert st.iterate(5, counts) == (-1, 0, True) and st.iterations == 12 and st.best == 30 and st.best_iteration == 7
    # exactly min_inliers is not enough; five iterations at a time
    st = M.RansacState(100, 20, 12)
    c2 = np.array([20] * 12, np.int32)
    assert st.iterate(5, c2) == (-1, 0, False) and st.iterate(5, c2) == (-1, 0, False) and st.iterate(5, c2) == (-1, 0, True)
    assert st.best == 20 and st.best_iteration == 11
    assert M.RansacState(19, 20, 300).iterate(5, counts) == (-1, 0, True)


@pytest.mark.parametrize("n", M.PARITY_SIZES)
def test_the_committed_parity_scenes_stay_inside_the_left_out_cap(n):
    """before any device run: with the spread the model measures on these scenes, no scene of tests/test_gpu_sim3.py
    leaves out more than 10 % of its hypotheses, and none is left out whole"""
    tools = os.path.join(os.path.dirname(HERE), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import fuzz_sim3 as F
    scenes = M.parity_scenes(n)
    models, spread = F.model_pass(scenes)
    margin = F.MARGIN_FACTOR * F.BOUND_FACTOR * spread
    for sc, m in zip(scenes, models):
        out = F.left_out(m, margin)
        assert m["n_use"] == 0 or out.mean() <= F.LEFT_OUT_CAP, (n, int(out.sum()), m["n_use"])
        assert m["N"] == n and len(sc["valid"]) > n

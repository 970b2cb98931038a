"""The PnP solver's definition (tests/pnp_model.py, P1-P10 of include/orbgpu.h) on its own: it recovers planted poses,
its pieces are what they claim to be, and the null-space convention of P5 does what it exists for."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import pnp_model as M  # noqa: E402


@pytest.mark.parametrize("n", [6, 8, 30])
@pytest.mark.parametrize("eig", ["jacobi", "eigh"])
def test_recovers_a_planted_pose_from_noise_free_points(n, eig):
    rng = np.random.default_rng(100 + n)
    sets = [M.planted(rng, n) for _ in range(8)]
    r = M.epnp(np.stack([s[2] for s in sets]), np.stack([s[3] for s in sets]), M.K_DEFAULT, eig)
    for b, (R, t, _, _) in enumerate(sets):
        assert np.abs(r["R"][b] - R).max() < 1e-8 and np.abs(r["t"][b] - t).max() < 1e-7, (b, r["err"][b])
        assert abs(np.linalg.det(r["R"][b]) - 1.0) < 1e-9
    assert (r["err"] < 1e-8).all()


@pytest.mark.parametrize("m", [3, 4, 5, 12])
def test_jacobi_agrees_with_eigh_and_is_orthogonal(m):
    rng = np.random.default_rng(m)
    X = rng.normal(size=(16, m, m))
    A = X @ np.swapaxes(X, 1, 2)
    A[8:, :, 0] = A[8:, 0, :] = 0.0            # a zero row and column: a null direction
    w, V = M.jacobi(A)
    assert np.abs(np.swapaxes(V, 1, 2) @ V - np.eye(m)).max() < 1e-13
    assert np.abs(V @ (w[:, :, None] * np.swapaxes(V, 1, 2)) - A).max() < 1e-12 * np.abs(A).max()
    assert np.abs(np.sort(w, 1) - np.linalg.eigvalsh(A)).max() < 1e-12 * np.abs(A).max()
    ws, Vt = M.sorted_eig(A, "jacobi")
    assert (np.diff(ws, axis=1) <= 0).all()
    lead = np.take_along_axis(Vt, np.argmax(np.abs(Vt), axis=2)[:, :, None], 2)
    assert (lead > 0).all()
    we, Ve = M.sorted_eig(A[:8], "eigh")
    assert np.abs(we - ws[:8]).max() < 1e-12 * np.abs(A).max() and np.abs(Ve - Vt[:8]).max() < 1e-9


def test_wave_sum_is_the_stated_order():
    rng = np.random.default_rng(3)
    x = rng.normal(size=(1, 150)) * 10.0 ** rng.integers(-8, 8, (1, 150))
    lanes = [0.0] * 64
    for k in range(150):
        lanes[k % 64] = lanes[k % 64] + float(x[0, k])
    s = 32
    while s:
        for l in range(s):
            lanes[l] = lanes[l] + lanes[l + s]
        s //= 2
    assert M.wave_sum(x)[0] == lanes[0]


def test_ransac_parameters_by_hand():
    P = lambda n, mi=10, mx=300, ms=4, eps=0.5, p=0.99: M.ransac_parameters(n, p, mi, mx, ms, eps)  # noqa: E731
    # N 300: nMinInliers = 150 = N epsilon; log(0.01) / log(1 - 0.125) = 34.49
    assert P(300) == (150, 35)
    # N = minInliers: one iteration
    assert P(10) == (10, 1) and P(20, mi=3) == (10, 35)
    # N < minInliers: the caller's iterate says no_more; epsilon = 10 / 9 > 1, the log of a negative number is NaN
    assert P(9) == (10, 300) and P(3) == (10, 300)
    # the epsilon raise: N 11, nMinInliers max(5, 10) = 10, epsilon 10 / 11: log(0.01) / log(1 - 0.7513) = 3.31
    assert P(11) == (10, 4)
    # min_set above both
    assert P(8, mi=2, ms=6, eps=0.1)[0] == 6
    # the truncated float product
    assert P(25, mi=1, eps=0.3)[0] == 7 and P(0) == (10, 1)
    assert P(100, p=1.0) == (50, 300) and P(100, p=0.0) == (50, 1) and P(100, mx=0) == (50, 1)
    assert P(100, eps=float("nan"))[0] == M.INT_MAX


def test_the_sampler_replays_the_quirk():
    seq = iter([0, 1, 1, 1])
    got = M.sample_sets(5, 1, 4, lambda lo, hi: next(seq))
    # [0 1 2 3 4] -> take 0, position 0 <- 4: [4 1 2 3]; take position 1 = 1, position 1 <- 3: [4 3 2]; take position 1
    # = 3, position THREE <- 2 (outside the live part): [4 3]; take position 1 = 3 again
    assert got.tolist() == [[0, 1, 3, 3]]
    # a swap-with-last sampler would have given 0 1 3 2
    calls = []

    def ri(lo, hi):
        calls.append((lo, hi))
        return hi
    got = M.sample_sets(7, 2, 4, ri)
    assert calls == [(0, 6), (0, 5), (0, 4), (0, 3)] * 2 and got[0].tolist() == got[1].tolist()
    with pytest.raises(ValueError):
        M.sample_sets(3, 1, 4, ri)
    with pytest.raises(ValueError):
        M.sample_sets(5, 1, 4, lambda lo, hi: hi + 1)
    rnd = iter([0, 2 ** 30, 2 ** 31 - 1])
    f = M.reference_random_int(lambda: next(rnd))
    assert [f(0, 9), f(0, 9), f(2, 5)] == [0, 5, 5]


def test_the_scan_resumes_and_the_first_iterate_runs_to_max_its():
    counts = np.array([3, 12, 11, 15, 12, 30, 9, 31, 40, 2, 2, 50, 60], np.int32)
    refined = {1: 9, 3: 10, 5: 10, 7: 10, 8: 10, 11: 40, 12: 70}
    seen = []

    def refine(h):
        seen.append(h)
        return refined[h]
    st = M.RansacState(100, 10, 8)
    # iterate(5) on a fresh solver: mnIterations < max_its keeps the loop going past five iterations, to max_its = 8
    assert st.iterate(5, counts, refine) == (-1, 0, True, False)
    assert st.iterations == 8 and st.best == 31 and st.best_iteration == 7 and seen == [1, 3, 5, 7]   # records only; 10 is not > 10
    # the next iterate(5) runs five more, though max_its is behind it, and accepts at 11
    assert st.iterate(5, counts, refine) == (11, 40, False, False) and st.iterations == 12 and seen[-2:] == [8, 11]
    # the same in one scan from a carried state, and a scan that runs out of hypotheses
    st2 = M.RansacState(100, 10, 8)
    st2.iterations, st2.best = 8, 31
    assert st2.iterate(5, counts, refine) == (11, 40, False, False)
    st3 = M.RansacState(100, 10, 20)
    assert st3.iterate(5, counts[:6], refine) == (-1, 0, False, True) and st3.iterations == 6
    assert st3.iterate(5, counts, refine)[0] == 11
    assert M.RansacState(9, 10, 300).iterate(5, counts, refine) == (-1, 0, True, False)


def _noisy_sets(n, count, seed):
    rng = np.random.default_rng(seed)
    sets = [M.planted(rng, n, noise_px=0.7) for _ in range(count)]
    E = rng.normal(size=(count, 12, 12))
    return np.stack([s[2] for s in sets]), np.stack([s[3] for s in sets]), 1e-14 * (E + np.swapaxes(E, 1, 2)) / 2.0


def _moved(pw, uv, perturb, eig, canonical):
    a = M.epnp(pw, uv, M.K_DEFAULT, eig, canonical)
    b = M.epnp(pw, uv, M.K_DEFAULT, eig, canonical, perturb=perturb)
    with np.errstate(all="ignore"):
        d = np.maximum(np.abs(a["R"] - b["R"]).max((1, 2)), np.abs(a["t"] - b["t"]).max(1))
    return np.where(np.isnan(d), np.inf, d)


@pytest.mark.parametrize("eig", ["eigh", "jacobi"])
@pytest.mark.parametrize("n", [4, 5])
def test_the_canonical_null_space_basis_pins_the_minimal_sets(n, eig):
    """P5's reason: with 4 (5) points M'M has an exact 4 (2)-dimensional null space whose raw eigenvector basis is
    decided by rounding noise.  300 seeded sets at 0.7 px noise, M'M perturbed by a relative 1e-14."""
    pw, uv, perturb = _noisy_sets(n, 300, 4000 + n)
    d = _moved(pw, uv, perturb, eig, canonical=True)
    print("n %d %s canonical: max %.3e median %.3e" % (n, eig, d.max(), np.median(d)))
    assert (d <= 1e-9).all(), (int((d > 1e-9).sum()), float(d.max()))
    if n == 4:
        raw = _moved(pw, uv, perturb, eig, canonical=False)
        print("n 4 %s raw: %.3f moved by more than 1e-6" % (eig, (raw > 1e-6).mean()))
        assert (raw > 1e-6).mean() > 0.5


@pytest.mark.parametrize("key", list(M.PARITY_SCENES))
def test_the_parity_scenes_stay_inside_the_left_out_cap(key):
    """The device parity test leaves a hypothesis out iff the model alone says so; here the model alone shows that the
    committed scenes leave out at most LEFT_OUT_CAP of their used hypotheses."""
    sc = M.parity_scene(key)
    m, spread = M.model_pass(sc)
    u = m["n_use"]
    out = M.left_out(m, M.BOUND_FACTOR * spread)
    print("scene %s: N %d, used %d, spread %.3e, left out %d" % (key, m["N"], u, spread, int(out.sum())))
    assert m["N"] == M.PARITY_SCENES[key][0] and len(sc["valid"]) > m["N"] and len(sc["sets"]) == 300
    assert u == 0 or out.mean() <= M.LEFT_OUT_CAP
    if m["N"] < 10:
        assert m["no_more"] and m["iterations"] == 0 and u == 0

"""What csrc/opt_math.h holds for the local bundle adjustment -- the 3x3 cofactor inverse, the runtime-size LL^T solve and
the point update -- against their definition in tests/lba_model.py: the header is compiled for the host with g++ (no
contraction, AddressSanitizer + UBSan), run once over the cases below, and every result has to be the model's, byte for
byte.  The pattern is tests/test_opt_math.py's."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import lba_model as L  # noqa: E402


def _hex(values):
    return " ".join(float(v).hex() for v in np.asarray(values, np.float64).ravel())


def _lower(A):
    return [A[i, j] for i in range(len(A)) for j in range(i + 1)]


def _solve_expected(A, b):
    ok, x = L.llt_solve(A, b)
    return np.r_[1.0 if ok else 0.0, x]


def _cases():
    rng = np.random.default_rng(21)
    cases = []

    def add(name, op, args, expected, check=None):
        expected = np.asarray(expected, np.float64).ravel()
        assert check is None or check(expected), name
        cases.append((name, op + " " + _hex(args), expected))

    # the point block of a handful of observations, undamped and damped; then rank-deficient and non-finite ones, which
    # follow IEEE (g2o does not test the determinant)
    for k in range(4):
        J = rng.normal(0, 1, (5, 3)) * rng.uniform(1.0, 300.0, 3)
        H = J.T @ J
        h = [H[0, 0], H[0, 1], H[0, 2], H[1, 1], H[1, 2], H[2, 2]]
        for tag, lam in (("lam0", 0.0), ("lam", 1e-5 * max(H[0, 0], H[1, 1], H[2, 2]))):
            inv = L.inv3_sym(h, lam)
            Hd = np.array([[h[0], h[1], h[2]], [h[1], h[3], h[4]], [h[2], h[4], h[5]]]) + lam * np.eye(3)
            assert np.abs(inv @ Hd - np.eye(3)).max() < 1e-6, (k, tag)
            add("inv3_%d_%s" % (k, tag), "inv3_sym", np.r_[h, lam], inv)
    add("inv3_rank_one", "inv3_sym", [4.0, 4.0, 4.0, 4.0, 4.0, 4.0, 0.0], L.inv3_sym([4.0] * 6, 0.0), lambda e: not np.isfinite(e).any())
    add("inv3_zero_damped", "inv3_sym", [0.0] * 6 + [0.5], L.inv3_sym([0.0] * 6, 0.5), lambda e: e[0] == 2.0 and e[1] == 0.0)
    add("inv3_nan", "inv3_sym", [1.0, np.nan, 0.0, 1.0, 0.0, 1.0, 0.0], L.inv3_sym([1.0, np.nan, 0.0, 1.0, 0.0, 1.0], 0.0),
        lambda e: np.isnan(e).all())
    for k in range(3):
        X, x = rng.normal(0, 3, 3), rng.normal(0, 0.01, 3)
        add("point_update_%d" % k, "point_update", np.r_[X, x], L.point_update(X, x))
    # the reduced camera system at the sizes the kernel meets: none, one pose, a few, more rows than a wave has lanes
    refused = lambda e: e.tobytes() == np.zeros(len(e)).tobytes()  # noqa: E731  false, and every x[i] is +0.0
    add("llt_0", "llt_solve", [0.0], _solve_expected(np.zeros((0, 0)), np.zeros(0)), lambda e: e[0] == 1.0)
    for n in (1, 6, 12, 18, 102):
        J = rng.normal(0, 1, (3 * n + 5, n)) * rng.uniform(0.1, 30.0, n)
        A, b = J.T @ J, rng.normal(0, 1, n)
        A = np.tril(A) + np.tril(A, -1).T
        e = _solve_expected(A, b)
        assert e[0] == 1.0 and np.abs(A @ e[1:] - b).max() < 1e-6 * np.abs(b).max() * np.linalg.cond(A), n
        assert e.tobytes() == np.r_[1.0, L._llt_solve_fast(A, b)[1]].tobytes(), n  # the model's own fast form
        add("llt_%d" % n, "llt_solve", np.r_[float(n), _lower(A), b], e)
        if n in (6, 18):
            Aneg = A.copy()
            Aneg[n // 2, n // 2] = -Aneg[n // 2, n // 2]
            add("llt_%d_negated_diagonal" % n, "llt_solve", np.r_[float(n), _lower(Aneg), b], _solve_expected(Aneg, b), refused)
            Anan = A.copy()
            Anan[n - 1, 1] = Anan[1, n - 1] = np.nan
            add("llt_%d_nan" % n, "llt_solve", np.r_[float(n), _lower(Anan), b], _solve_expected(Anan, b), refused)
            Asing = np.full((n, n), 4.0)  # rank one: the second pivot is 4 - 2 * 2, exactly 0
            add("llt_%d_singular" % n, "llt_solve", np.r_[float(n), _lower(Asing), b], _solve_expected(Asing, b), refused)
    # an identity block among the poses (a free pose without an active edge) leaves the other unknowns' bits alone
    n = 12
    J = rng.normal(0, 1, (40, n))
    A, b = J.T @ J, rng.normal(0, 1, n)
    A = np.tril(A) + np.tril(A, -1).T
    B, c = np.eye(18), np.zeros(18)
    keep = np.r_[0:6, 12:18]
    B[np.ix_(keep, keep)] = A
    c[keep] = b
    e = _solve_expected(B, c)
    assert e[1:][keep].tobytes() == _solve_expected(A, b)[1:].tobytes() and not e[7:13].any()
    add("llt_identity_block", "llt_solve", np.r_[18.0, _lower(B), c], e)
    return cases


CASES = _cases()


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("opt_math_lba")
    exe, inp = str(d / "opt_math_lba_test"), str(d / "cases.txt")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "orb_slam2_map_amd", "csrc"), os.path.join(ROOT, "tests", "opt_math_lba_test.cpp"),
                    "-o", exe], check=True)
    with open(inp, "w") as f:
        f.write("".join(line + "\n" for _, line, _ in CASES))
    r = subprocess.run([exe, inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr  # no sanitizer report either
    lines = r.stdout.splitlines()
    assert len(lines) == len(CASES)
    return {name: np.array([float.fromhex(t) for t in out.split()], np.float64) for (name, _, _), out in zip(CASES, lines)}


def test_case_names_are_unique():
    names = [name for name, _, _ in CASES]
    assert len(names) == len(set(names)) and len(names) >= 25


@pytest.mark.parametrize("name", [name for name, _, _ in CASES])
def test_header_equals_model_bit_for_bit(results, name):
    expected = next(e for n, _, e in CASES if n == name)
    got = results[name]
    assert got.shape == expected.shape and got.tobytes() == expected.tobytes(), (name, got, expected)

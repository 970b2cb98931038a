"""csrc/opt_math.h, the FP64 helpers pose_opt.hip, sim3_opt.hip, local_ba.hip and essential_graph.hip share, against their
definition in tests/pose_model.py: the header is compiled for the host with g++ (no contraction, AddressSanitizer + UBSan),
run once over the cases below, and every result has to be the model's, byte for byte.  The optimisers themselves are only
compared with the model through whole optimisations, within a multiple of its spread; this is the check of the arithmetic
on its own.  What the bundle adjustment adds to the header is in test_opt_math_lba.py, the Sim3 algebra of sim3_math.h in
test_sim3_math.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import pose_model as M  # noqa: E402


def _hex(values):
    return " ".join(float(v).hex() for v in np.asarray(values, np.float64).ravel())


def _pack(H):
    return [H[a, c] for a in range(len(H)) for c in range(a, len(H))]


def _rotation(axis, angle):
    return M.se3_exp(np.r_[np.asarray(axis, np.float64) * angle, 0.0, 0.0, 0.0])[0]


def _unit_quats(rng, n):
    return [M.quat_normalize(rng.normal(0, 1, 4)) for _ in range(n)]


def _cholesky_expected(H, lam, b):
    ok, x = M.cholesky_solve(H, lam, b)
    return np.r_[1.0 if ok else 0.0, x]


def _cases():
    """(name, line for the program, expected float64 array, what must hold for the model's own result)."""
    rng = np.random.default_rng(20)
    cases = []

    def add(name, op, args, expected, check=None):
        expected = np.asarray(expected, np.float64).ravel()
        assert check is None or check(expected), name
        cases.append((name, op + " " + _hex(args), expected))

    # quat_from_matrix: positive trace, and the three branches of a rotation near 180 degrees
    for k in range(4):
        m = _rotation(rng.normal(0, 1, 3) / 2.0, 1.0)
        assert np.trace(m) > 0
        add("from_matrix_trace_%d" % k, "quat_from_matrix", m, M.quat_from_matrix(m))
    for i, axis in enumerate(np.eye(3)):
        m = _rotation(axis, np.pi - 0.01 * (i + 1))
        j, k = (i + 1) % 3, (i + 2) % 3
        q = M.quat_from_matrix(m)
        # the model takes branch i: the trace is not positive, m[i, i] is the largest diagonal entry, and q[i] is that
        # branch's expression
        assert m[0, 0] + m[1, 1] + m[2, 2] <= 0 and int(np.argmax(np.diag(m))) == i
        assert q[i] == 0.5 * np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        add("from_matrix_branch_%d" % i, "quat_from_matrix", m, q)
    # quat_normalize on both sides of w = 0
    for k, w in enumerate((-0.7, 0.4, -1e-3, 2.5)):
        q = np.r_[rng.normal(0, 1, 3), w]
        add("normalize_%d" % k, "quat_normalize", q, M.quat_normalize(q), lambda e: e[3] > 0)
    for k, (a, b) in enumerate(zip(_unit_quats(rng, 4), _unit_quats(rng, 4))):
        add("to_matrix_%d" % k, "quat_to_matrix", a, M.quat_to_matrix(a))
        add("mul_%d" % k, "quat_mul", np.r_[a, b], M.quat_mul(a, b))
    # the entry state of the optimisers: float rows of stride 3 (R12) and 4 (Tcw, T2w)
    for k, stride in enumerate((3, 4, 4)):
        m = np.zeros((3, stride), np.float32)
        m[:, :3] = _rotation(rng.normal(0, 1, 3), 1.0 + k).astype(np.float32)
        m[:, 3:] = 7.0  # the translation column is not read
        add("unit_quat_stride%d_%d" % (stride, k), "unit_quat_from_floats", m,
            M.quat_normalize(M.quat_from_matrix(m[:, :3].astype(np.float64))))
    # huber below, at and above delta^2, and above it without the kernel
    delta = M.DELTA_STEREO
    d2 = delta * delta
    for name, chi2, use in (("below", 0.5 * d2, True), ("at", d2, True), ("above", 3.7 * d2, True), ("no_kernel", 3.7 * d2, False)):
        r0, r1 = M.huber(np.array([chi2]), delta, np.array([use]))
        inner = chi2 <= d2 or not use
        assert (r0[0] == chi2 and r1[0] == 1.0) if inner else (r0[0] < chi2 and r1[0] < 1.0), name
        add("huber_" + name, "huber", [chi2, delta, d2, float(use)], [r0[0], r1[0]])
    r0, r1 = M.huber(np.array([3.7 * d2]), delta, np.array([True]))
    add("huber_default_kernel", "huber", [3.7 * d2, delta, d2], [r0[0], r1[0]])
    # the damped normal equation, 6 x 6 and 7 x 7
    for n in (6, 7):
        op = "cholesky_solve%d" % n
        for k in range(3):
            J = rng.normal(0, 1, (40, n)) * rng.uniform(0.1, 30.0, n)
            H, b = J.T @ J, rng.normal(0, 1, n)
            H = np.triu(H) + np.triu(H, 1).T
            lam = 1e-5 * max(abs(H[a, a]) for a in range(n))
            add("lambda%d_%d" % (n, k), "lm_initial_lambda%d" % n, _pack(H), [lam])
            for tag, l in (("lam0", 0.0), ("lam", lam)):
                add("%s_%d_%s" % (op, k, tag), op, np.r_[l, _pack(H), b], _cholesky_expected(H, l, b), lambda e: e[0] == 1.0)
        refused = lambda e: e.tobytes() == np.zeros(len(e)).tobytes()  # noqa: E731  false, and every x[i] is +0.0
        Hneg = H.copy()
        Hneg[2, 2] = -Hneg[2, 2]
        add(op + "_negated_diagonal", op, np.r_[0.0, _pack(Hneg), b], _cholesky_expected(Hneg, 0.0, b), refused)
        Hnan = H.copy()
        Hnan[1, 3] = Hnan[3, 1] = np.nan
        add(op + "_nan", op, np.r_[lam, _pack(Hnan), b], _cholesky_expected(Hnan, lam, b), refused)
        Hsing = np.full((n, n), 4.0)  # rank one: the second pivot is 4 - 2 * 2, exactly 0
        add(op + "_singular", op, np.r_[0.0, _pack(Hsing), b], _cholesky_expected(Hsing, 0.0, b), refused)
    return cases


CASES = _cases()


def _lm_trial(cur, tmp, scale, lam, nu):
    """The decision on a trial as run_model writes it (pose_model.py, the trial loop): accepted, lam, nu, rho, stop."""
    with np.errstate(all="ignore"):
        cur, tmp, scale, lam, nu = (np.float64(v) for v in (cur, tmp, scale, lam, nu))
        rho = (cur - tmp) / scale
        if rho > 0 and np.isfinite(tmp):
            c3 = 2.0 * rho - 1.0
            alpha = min(1.0 - (c3 * c3) * c3, 2.0 / 3.0)
            return [1.0, lam * max(1.0 / 3.0, alpha), 2.0, rho, 0.0]
        lam, nu = lam * nu, nu * 2.0
        return [0.0, lam, nu, rho, 0.0 if np.isfinite(lam) else 1.0]


def _lm_cases():
    """(name, line, expected): both sides of every decision of lm_trial."""
    rows = (("accept_floor", (10.0, 1.0, 9.0, 1e-3, 8.0), 1.0, False),        # rho = 1: 1 - 1 = 0, held at 1 / 3
            ("accept_cap", (10.0, 9.0, 2.0, 1e-3, 8.0), 1.0, False),          # rho = 1 / 2: 1 - 0 = 1, held at 2 / 3
            ("accept_between", (10.0, 2.5, 8.5, 1e-3, 2.0), 1.0, False),      # rho = 0.88...: the cube itself
            ("accept_tiny_rho", (10.0, 10.0 - 1e-9, 5.0, 1e-3, 4.0), 1.0, False),
            ("reject_worse", (10.0, 12.0, 3.0, 1e-3, 2.0), 0.0, False),
            ("reject_equal", (10.0, 10.0, 3.0, 1e-3, 4.0), 0.0, False),       # rho = 0 is not > 0
            ("reject_failed_solve", (10.0, M.DBL_MAX, 3.0, 1e-3, 2.0), 0.0, False),
            ("reject_inf", (10.0, -np.inf, 3.0, 1e-3, 2.0), 0.0, False),      # rho > 0, but the trial's chi2 is not finite
            ("reject_nan", (10.0, np.nan, 3.0, 1e-3, 2.0), 0.0, False),
            ("reject_lambda_overflows", (10.0, 12.0, 3.0, 1e300, 1e10), 0.0, True))
    cases = []
    for name, args, accepted, stop in rows:
        want = _lm_trial(*args)
        assert want[0] == accepted and want[4] == float(stop), name
        cases.append((name, "lm_trial " + " ".join(float(v).hex() if np.isfinite(v) else repr(float(v)) for v in args),
                      np.asarray(want, np.float64)))
    return cases


LM_CASES = _lm_cases()


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("opt_math")
    exe, inp = str(d / "opt_math_test"), str(d / "cases.txt")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "orb_slam2_map_amd", "csrc"), os.path.join(ROOT, "tests", "opt_math_test.cpp"),
                    "-o", exe], check=True)
    every = CASES + LM_CASES
    with open(inp, "w") as f:
        f.write("".join(line + "\n" for _, line, _ in every))
    r = subprocess.run([exe, inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr  # no sanitizer report either
    lines = r.stdout.splitlines()
    assert len(lines) == len(every)
    return {name: np.array([float.fromhex(t) for t in out.split()], np.float64) for (name, _, _), out in zip(every, lines)}


@pytest.mark.parametrize("name", [name for name, _, _ in LM_CASES])
def test_lm_trial_equals_the_models_decision(results, name):
    expected = next(e for n, _, e in LM_CASES if n == name)
    got = results[name]
    nan = np.isnan(expected)
    assert np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == expected[~nan].tobytes(), (name, got, expected)


def test_case_list_covers_the_issue():
    names = [name for name, _, _ in CASES]
    assert len(names) == len(set(names)) and 36 <= len(names) <= 80
    for n in (6, 7):
        for tail in ("0_lam0", "0_lam", "negated_diagonal", "nan", "singular"):
            assert "cholesky_solve%d_%s" % (n, tail) in names


@pytest.mark.parametrize("name", [name for name, _, _ in CASES])
def test_header_equals_model_bit_for_bit(results, name):
    expected = next(e for n, _, e in CASES if n == name)
    got = results[name]
    assert got.shape == expected.shape and got.tobytes() == expected.tobytes(), (name, got, expected)

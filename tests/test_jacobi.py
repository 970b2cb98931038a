"""csrc/jacobi.h, the cyclic Jacobi every solver's parity rests on, against its definition in tests/jacobi_model.py: the
per-lane half of the header is compiled for the host with g++ (no contraction, AddressSanitizer + UBSan), run once over the
matrices below, and every value has to be the model's, bit for bit (NaN patterns included).  The models of the four
families must all use that one definition, and its scalar and batched forms must agree bit for bit at the sizes the
kernels use.

A 4 x 4 on which 16 and 30 sweeps differ is not among the cases: a search over 32 million finite symmetric matrices (unit
scale, row scales over 16 to 300 decades, entries whose squares are subnormal, nearly equal diagonals) found none -- off
shrinks quadratically and the rule stops every one of them within a few sweeps -- so <16> and <30> are each held to their
own model on the cases below, where they agree."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import init_model  # noqa: E402
import jacobi_model as J  # noqa: E402
import newpts_model  # noqa: E402
import pnp_model  # noqa: E402
import sim3_model  # noqa: E402

CSRC = os.path.join(ROOT, "orb_slam2_map_amd", "csrc")
f32, f64 = np.float32, np.float64


def _sym(rng, m, scale=1.0):
    a = rng.normal(0, 1, (m, m)) * scale
    return np.triu(a) + np.triu(a, 1).T


def _gram(Af):
    """A'A as null_vector4 forms it: FP64 sums in row order"""
    m = len(Af)
    return np.array([[sum((float(Af[r][a]) * float(Af[r][b]) for r in range(m)), 0.0) for b in range(m)] for a in range(m)], f64)


def _rotated(rng, w):
    q, _ = np.linalg.qr(rng.normal(0, 1, (len(w), len(w))))
    a = (q * np.asarray(w, f64)) @ q.T
    return np.triu(a) + np.triu(a, 1).T


def matrices(m, seed=26):
    """(name, symmetric m x m float64) of every kind the issue lists"""
    rng = np.random.default_rng(seed + m)
    out = [("random_%d" % k, _sym(rng, m, 10.0 ** (2 * k - 2))) for k in range(3)]
    out += [("gram_%d" % k, _gram(rng.normal(0, 1 + 20 * k, (m, m)).astype(f32))) for k in range(3)]
    out.append(("diagonal", np.diag(rng.normal(0, 3, m))))
    z = _sym(rng, m)
    z[0, 2] = z[2, 0] = 0.0
    out.append(("zero_entry", z))
    v = rng.normal(0, 1, m)
    out.append(("rank_one", np.outer(v, v)))
    out.append(("zero", np.zeros((m, m))))
    out.append(("equal_pair", _rotated(rng, [5.0, 2.0, 2.0] + [1.0] * (m - 3))))
    tie = np.eye(m)  # least eigenvalue 0 with the eigenvector (c, -c, 0, ...): two entries of equal magnitude lead it
    tie[0, 1] = tie[1, 0] = 1.0
    out.append(("equal_least_and_tied_lead", tie))
    out.append(("equal_least_diagonal", np.diag([9.0, 4.0] + [1.0] * (m - 2))))
    n = _sym(rng, m)
    n[1, 2] = n[2, 1] = np.nan
    out.append(("nan", n))
    i = _sym(rng, m)
    i[0, m - 1] = i[m - 1, 0] = np.inf
    out.append(("inf", i))
    return out


def _scalar(A, sweeps):
    """jacobi_sym's (diagonal, V) as arrays"""
    a = [[float(x) for x in row] for row in A]
    V = J.jacobi_sym(a, sweeps)
    return np.array([a[k][k] for k in range(len(a))], f64), np.array(V, f64)


# ---- the header on the host ----------------------------------------------------------------------------------------------
CASES = matrices(4)


def _expected(A):
    parts = []
    for sweeps in (16, 30):
        w, V = _scalar(A, sweeps)
        parts += [w, V.ravel()]
    with np.errstate(all="ignore"):
        parts.append(np.array(newpts_model.null_vector4(A.astype(f32)), f32).astype(f64))
    return np.concatenate(parts)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("jacobi")
    exe, inp = str(d / "jacobi_test"), str(d / "matrices.txt")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-I" + CSRC, os.path.join(ROOT, "tests", "jacobi_test.cpp"), "-o", exe], check=True)
    with open(inp, "w") as f:
        for _, A in CASES:
            f.write(" ".join(float(v).hex() for v in A.ravel()) + "\n")
    r = subprocess.run([exe, inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr  # no sanitizer report either
    lines = r.stdout.splitlines()
    assert len(lines) == len(CASES)
    return {name: np.array([int(t, 16) for t in line.split()], np.uint64).view(f64) for (name, _), line in zip(CASES, lines)}


def test_case_list_covers_the_issue():
    names = [n for n, _ in CASES]
    assert len(names) == len(set(names))
    by = dict(CASES)
    for name, A in CASES:
        assert A.shape == (4, 4) and A.tobytes() == A.T.copy().tobytes(), name
    # what each kind is there for holds for the model's own result
    a = [[float(x) for x in row] for row in by["diagonal"]]
    assert np.array(J.jacobi_sym(a, 30)).tobytes() == np.eye(4).tobytes() and np.array(a).tobytes() == by["diagonal"].tobytes()
    assert by["zero_entry"][0, 2] == 0.0 and np.count_nonzero(by["zero_entry"]) == 14
    assert np.linalg.matrix_rank(by["rank_one"]) == 1 and not by["zero"].any()
    w = np.sort(_scalar(by["equal_pair"], 30)[0])
    assert abs(w[2] - w[1]) < 1e-14 and w[3] - w[2] > 1 and w[1] - w[0] > 0.5
    x = np.array(newpts_model.null_vector4(by["equal_least_and_tied_lead"].astype(f32)))
    assert x[0] > 0 and x[1] == -x[0] and not x[2:].any()  # the first among equals is the positive one
    x = np.array(newpts_model.null_vector4(by["equal_least_diagonal"].astype(f32)))
    assert x.tolist() == [0.0, 0.0, 0.0, 1.0]  # of the two equal least eigenvalues the later one is last in the stable order
    assert np.isnan(by["nan"]).sum() == 2 and np.isinf(by["inf"]).sum() == 2
    assert np.isnan(_expected(by["nan"])).any() and np.isnan(_expected(by["inf"])).any()


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_header_equals_model_bit_for_bit(results, name):
    expected = _expected(dict(CASES)[name])
    got = results[name]
    assert got.shape == expected.shape == (44,) and got.tobytes() == expected.tobytes(), (name, got, expected)


# ---- one Jacobi in the models ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [3, 4, 9, 12])
@pytest.mark.parametrize("sweeps", [16, 30])
def test_scalar_and_batched_forms_agree_bit_for_bit(m, sweeps):
    mats = matrices(m)
    wb, Vb = J.jacobi_sym_batch(np.stack([A for _, A in mats]), sweeps)
    for k, (name, A) in enumerate(mats):
        w, V = _scalar(A, sweeps)
        assert w.tobytes() == wb[k].tobytes() and V.tobytes() == Vb[k].tobytes(), name
    # a batch of one is the same problem: no bit depends on the batch's other members
    w1, V1 = J.jacobi_sym_batch(mats[0][1][None], sweeps)
    assert w1[0].tobytes() == wb[0].tobytes() and V1[0].tobytes() == Vb[0].tobytes()


def test_the_family_models_take_their_jacobi_from_the_shared_one(monkeypatch):
    assert (sim3_model.JACOBI_SWEEPS, pnp_model.JACOBI_SWEEPS, init_model.JACOBI_SWEEPS, newpts_model.JACOBI_SWEEPS) == (16, 30, 30, 30)
    calls = []
    for mod in (sim3_model, newpts_model, pnp_model):
        for name in ("jacobi_sym", "jacobi_sym_batch"):
            if hasattr(mod, name):
                def spy(A, sweeps, _f=getattr(J, name), _tag=(mod.__name__, name)):
                    calls.append(_tag + (sweeps,))
                    return _f(A, sweeps)
                monkeypatch.setattr(mod, name, spy)
    A = matrices(4)[0][1]
    sim3_model.jacobi4(A)
    newpts_model.jacobi4([[float(x) for x in row] for row in A])
    pnp_model.jacobi(A[None])
    init_model.sorted_eig(A[None], "jacobi", init_model.JACOBI_SWEEPS)
    assert calls == [("sim3_model", "jacobi_sym", 16), ("newpts_model", "jacobi_sym", 30), ("pnp_model", "jacobi_sym_batch", 30),
                     ("pnp_model", "jacobi_sym_batch", 30)]
    # and none of them keeps a rotation of its own
    for mod in (sim3_model, newpts_model, pnp_model, init_model):
        src = open(mod.__file__).read()
        assert "theta * theta + 1.0" not in src and "JACOBI_STOP =" not in src, mod.__name__


# ---- one Jacobi on the device ----------------------------------------------------------------------------------------------
def test_the_device_units_share_one_jacobi():
    """The rotation is written once, in jacobi.h; the copies and their notes are gone; and the header's per-lane half stays
    compilable without HIP."""
    names = sorted(n for n in os.listdir(CSRC) if n.endswith((".hip", ".h")))
    src = {n: open(os.path.join(CSRC, n)).read() for n in names}
    assert "jacobi4.h" not in names
    assert [n for n in names if "theta >= 0.0 ? 1.0 / den" in src[n]] == ["jacobi.h"]
    assert src["jacobi.h"].count("theta >= 0.0 ? 1.0 / den") == 2  # the per-lane form and the wave-wide one
    for word in ("jacobi_rotate", "PNP_JACOBI_STOP", "INIT_JACOBI_STOP", "an edit here is an edit there", "jacobi4.h"):
        assert [n for n in names if word in src[n]] == [], word
    assert "jacobi4.h" not in open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    for name, call in (("sim3.hip", "jacobi4_lane<S3_JACOBI_SWEEPS>(A, V)"), ("initializer.hip", "null_vector4(Af, x4)"),
                       ("new_points.hip", "null_vector4("), ("matcher_proj.hip", "tri_finish_block(n1, angle1"),
                       ("pnp.hip", "sorted_eig_wave<LD, PNP_JACOBI_SWEEPS>(S,"),
                       ("initializer.hip", "sorted_eig_wave<ILD, INIT_JACOBI_SWEEPS>(S,")):
        assert call in src[name], (name, call)
    assert "S3_JACOBI_SWEEPS = 16" in src["sim3.hip"] and "PNP_JACOBI_SWEEPS = 30" in src["pnp.hip"]
    assert "INIT_JACOBI_SWEEPS = 30" in src["initializer.hip"] and "JACOBI_STOP = 1e-32" in src["jacobi.h"]
    assert "__shared__" not in src["matcher_proj.hip"].split("void k_tri_finish(")[1].split("\n}\n")[0]
    # outside its __HIPCC__ block the header needs neither HIP nor common.h
    host = re.sub(r"#if defined\(__HIPCC__\)\n// The wave-wide form.*?#endif  // __HIPCC__\n", "", src["jacobi.h"], flags=re.S)
    assert host != src["jacobi.h"] and "void jacobi_wave(" not in host and "void jacobi4_lane(" in host
    assert "#include <hip" not in src["jacobi.h"] and '#include "common.h"' not in src["jacobi.h"]
    assert "__syncthreads" not in host and "__device__" not in host.replace("__host__ __device__", "")

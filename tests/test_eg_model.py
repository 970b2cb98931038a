"""tests/eg_model.py, the float64 restatement of Optimizer::OptimizeEssentialGraph, pinned without itself: its logarithm
against sim3opt_model's exponential, its solve against numpy's, its optimum against a ground truth it was not given, and
the margins of the committed parity scenes (no GPU)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import eg_model as M  # noqa: E402
import sim3opt_model as S3  # noqa: E402


def _miss(theta, sigma, rng):
    """|log(exp(x)) - x| relative to max(1, |x|) for an x of that angle and scale, exp being sim3opt_model's."""
    x = np.concatenate([M._rand_rot(rng, theta), rng.normal(0, 1, 3), [sigma]])
    q, t, s = S3.sim3_exp(x)
    y = M.s_log(np.concatenate([q, t, [s]]))
    return float(np.abs(y - x).max() / max(1.0, np.abs(x).max()))


def test_log_inverts_exp_where_the_issue_says_it_does():
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(300):  # |sigma| < 1e-5 with theta <= 1e-3 or 0.01 <= theta < 3
        theta = float(rng.choice([rng.uniform(0, 1e-3), 10 ** rng.uniform(-9, -3), rng.uniform(0.01, 3)]))
        worst = max(worst, _miss(theta, float(rng.uniform(-1e-5, 1e-5) * 0.999), rng))
    assert worst <= 1e-9, worst
    worst = 0.0
    for _ in range(300):  # |sigma| >= 1e-5 with theta < 1e-5 or theta >= 0.01
        theta = float(rng.choice([rng.uniform(0, 1e-5) * 0.999, rng.uniform(0.01, 3)]))
        sigma = float(rng.choice([-1, 1]) * rng.choice([10 ** rng.uniform(-5, -1) * 1.001, rng.uniform(0.01, 0.3)]))
        worst = max(worst, _miss(theta, sigma, rng))
    assert worst <= 1e-9, worst


def test_the_published_small_angle_b_is_kept():
    """G3 keeps B of the small-angle, |sigma| >= eps case as published: ((sigma^2 / 2 - sigma + 1) s) / sigma^3.  It is not
    the limit of the general case (about 1 / 6 near the identity), and log takes it up to theta = sqrt(2e-5) where exp has
    long left its own small-angle case -- so between them log(exp(x)) misses x."""
    sigma, s = 0.01, np.exp(0.01)
    published = ((0.5 * sigma * sigma - sigma) + 1.0) * s / sigma ** 3
    th = 0.01  # the general case next to it
    a, b, c = s * np.sin(th), s * np.cos(th), th * th + sigma * sigma
    general = ((s - 1.0) / sigma - ((b - 1.0) * sigma + a * th) / c) / (th * th)
    assert published > 1e5 and abs(general - 1.0 / 6.0) < 0.01
    rng = np.random.default_rng(1)
    assert max(_miss(1e-3, 0.01, rng) for _ in range(20)) > 0.1       # inside the gap: off by the size of x
    assert max(_miss(0.02, 0.01, rng) for _ in range(20)) <= 1e-9     # outside it
    # the model's log does use the published value: upsilon = W^-1 t with W = (A Om + B Om Om) + C I
    x = np.concatenate([M._rand_rot(rng, 1e-3), [0.3, -0.2, 0.5], [sigma]])
    q, t, sx = S3.sim3_exp(x)
    y = M.s_log(np.concatenate([q, t, [sx]]))
    O = S3.skew(y[:3])
    A = ((sigma - 1.0) * sx + 1.0) / (sigma * sigma)
    Bp = ((0.5 * sigma * sigma - sigma) + 1.0) * sx / sigma ** 3
    W = A * O + Bp * (O @ O) + ((sx - 1.0) / sigma) * np.eye(3)
    # sigma comes back from log(exp(sigma)) with a rounding of 1e-16, which 1 / sigma^3 = 1e6 carries into B: 1e-10 of |W| |y|
    assert np.abs(W @ y[3:6] - t).max() <= 1e-10 * np.abs(W).max() * np.abs(y[3:6]).max()


def test_lu_solve3_pivots_and_solves():
    rng = np.random.default_rng(2)
    W = rng.normal(0, 1, (50, 3, 3))
    W[:10, 0, 0] = 0.0  # a zero where an unpivoted elimination would divide
    t = rng.normal(0, 1, (50, 3))
    x = M.lu_solve3(W, t)
    assert np.allclose(np.einsum("nij,nj->ni", W, x), t, atol=1e-10)


def _consistent(V, seed, fix_scale, reach=2, perturb=0.03):
    """Measurements from ground-truth states (every edge of kind 1 on the true map), perturbed entry estimates, row 0 fixed."""
    sc = M.make_scene(V, seed, reach=reach, fix_scale=fix_scale, rot_drift=0.0, trans_drift=0.0, scale_drift=0.0, n_corrected=0,
                      perturb=perturb, perturb_scale=False, n_iterations=8)
    sc["edge_kind"] = np.ones_like(sc["edge_kind"])
    return sc


def test_solve_equals_numpy_on_the_dense_system():
    sc = _consistent(9, 11, False)
    taken, _, _, free = M.index_of(sc)
    i, j = sc["edge_i"][taken], sc["edge_j"][taken]
    Mm = M.measurements(sc, taken)
    St = np.asarray(sc["Scw"], np.float64)
    e = M.edge_errors(Mm, St[i], St[j])
    Ji, Jj = M.jacobians(Mm, St, i, j, False)
    slot = np.full(len(St), -1)
    slot[free] = np.arange(len(free))
    H, b = M.assemble(e, Ji, Jj, i, j, slot, len(free), np.arange(len(taken)))
    assert H.shape == (56, 56) and np.array_equal(H, H.T)
    for lam in (1e-16, 1e-3, 10.0):
        ok, x = M.solve(H, lam, b)
        want = np.linalg.solve(H + lam * np.eye(len(b)), b)
        assert ok and np.allclose(x, want, rtol=1e-8, atol=1e-12 * np.abs(want).max())
    # the dense sums are the ones G6 writes down
    Jfull = np.zeros((len(taken), 7, 56))
    for k in range(len(taken)):
        for v, J in ((i[k], Ji[k]), (j[k], Jj[k])):
            if slot[v] >= 0:
                Jfull[k][:, 7 * slot[v]:7 * slot[v] + 7] = J
    assert np.allclose(H, np.einsum("kra,krb->ab", Jfull, Jfull), rtol=1e-12, atol=1e-9)
    assert np.allclose(b, -np.einsum("kra,kr->a", Jfull, e), rtol=1e-12, atol=1e-9)
    bad = H.copy()
    bad[5, 5] = -1.0
    ok, x = M.solve(bad, 0.0, b)
    assert not ok and not x.any()


@pytest.mark.parametrize("fix_scale", [False, True])
def test_a_consistent_graph_converges_to_the_ground_truth(fix_scale):
    sc = _consistent(10, 21 + fix_scale, fix_scale)
    r = M.essential_graph(sc)
    assert r["chi2_start"] > 1e-3 and r["chi2_end"] <= 1e-12 * r["chi2_start"], (r["chi2_start"], r["chi2_end"])
    S, G = r["Siw_d"], sc["Snc"]
    for a, b in zip(sc["edge_i"], sc["edge_j"]):  # every relative state S_j S_i^-1 is the true one
        rel = M.s_log(M.s_mul(M.s_mul(G[b], M.s_inv(G[a])), M.s_inv(M.s_mul(S[b], M.s_inv(S[a])))))
        assert np.abs(rel).max() < 1e-7, (a, b, rel)
    # and with row 0 fixed on the map, every state is
    assert np.abs(M.s_log(M.s_mul(S, M.s_inv(G)))).max() < 1e-7
    assert S[0].tobytes() == sc["Scw"][0].tobytes()  # the fixed vertex comes out bit-equal
    assert np.array_equal(r["Tiw"], M.tiw_of(S))
    if fix_scale:
        assert S[:, 7].tobytes() == np.asarray(sc["Scw"])[:, 7].tobytes()  # every scale exactly as it came
    else:
        assert not np.array_equal(S[1:, 7], sc["Scw"][1:, 7])


def test_fix_scale_leaves_every_scale_on_an_inconsistent_loop_too():
    sc = M.make_scene(8, 31, fix_scale=True, n_iterations=4)
    sc["Scw"][3, 7] = 1.25  # whatever it is, it stays
    r = M.essential_graph(sc)
    assert r["Siw_d"][:, 7].tobytes() == sc["Scw"][:, 7].tobytes() and r["chi2_end"] < r["chi2_start"]


def test_points_follow_their_reference_row():
    sc = M.make_scene(6, 41, n_iterations=3, n_points=20)
    sc["point_ref"][[2, 9]] = (-1, 6)
    r = M.essential_graph(sc)
    assert r["n_bad_ref"] == 2 and r["pos"][[2, 9]].tobytes() == sc["world_pos"][[2, 9]].tobytes()
    ok = np.ones(20, bool)
    ok[[2, 9]] = False
    # a point keeps its place in its reference key frame's camera: Siw_opt P' = Scw P
    ref = sc["point_ref"][ok]
    cam_before = M.s_map(sc["Scw"][ref], sc["world_pos"][ok].astype(np.float64))
    cam_after = M.s_map(r["Siw_d"][ref], r["pos"][ok].astype(np.float64))
    assert np.abs(cam_after - cam_before).max() < 1e-5  # the float rounding of P'


def test_bad_edges_are_skipped_and_counted():
    sc = dict(M.PARITY_SCENES)["parallel_fixed_pair_bad_edges"]
    taken, n_bad, active, free = M.index_of(sc)
    assert n_bad == 3 and len(taken) == len(sc["edge_i"]) - 3 and active.all() and list(free) == [1, 2, 4, 5, 6]


NAMES = [n for n, _ in M.PARITY_SCENES]


def test_parity_set_has_the_shapes_the_device_test_needs():
    assert len(set(NAMES)) == len(NAMES)
    by = dict(M.PARITY_SCENES)
    W = M.THREADS
    counts = {len(M.index_of(sc)[0]) for sc in by.values()}
    assert {1, 63, 64, 65, W - 1, W, W + 1} <= counts
    assert {9, 10, 73, 74} <= {len(M.index_of(sc)[3]) for sc in by.values()}
    assert by["iterations0"]["n_iterations"] == 0 and by["iterations1"]["n_iterations"] == 1
    for n in ("ring8_fix0", "ring40_fix0", "ring8_fix1", "ring40_fix1"):
        sc = by[n]
        assert not np.array_equal(sc["Scw"], sc["Snc"]) and set(sc["edge_kind"]) == {0, 1}
        # the drift at the seam is past the acos case: a rotation error above 0.01 rad (and a scale drift of 0.1)
        taken = M.index_of(sc)[0]
        e = M.edge_errors(M.measurements(sc, taken), sc["Scw"][sc["edge_i"]], sc["Scw"][sc["edge_j"]])
        assert np.linalg.norm(e[:, :3], axis=1).max() > 0.01
        assert sc["fix_scale"] or np.abs(e[:, 6]).max() > 0.05


@pytest.mark.parametrize("name", NAMES)
def test_parity_scene_keeps_its_discrete_outputs(name):
    """Under 8 permutations of the summation order and libm_nudge = +-1 no discrete output flips (iterations, trials, the
    accept / reject trace), so the device parity test may leave nothing out."""
    sc = dict(M.PARITY_SCENES)[name]
    base = M.essential_graph(sc)
    spread, flips = M.model_spread(sc, base)
    assert flips == 0, (name, base["trace"])
    assert spread < 1e-5 or name == "failed_pivot"


def test_parity_set_reaches_every_branch():
    res = {n: M.essential_graph(sc) for n, sc in M.PARITY_SCENES if n not in ("free73", "free74", "edges511", "edges512", "edges513")}
    logs = sum(r["log_cases"] for r in res.values())
    exps = sum(r["exp_cases"] for r in res.values())
    assert (logs > 0).all() and (exps > 0).all(), (logs, exps)
    assert any("r" in r["trace"] for r in res.values())
    assert res["failed_pivot"]["trace"] == "ppp" and np.isnan(res["failed_pivot"]["chi2_end"])
    assert res["iterations0"]["trace"] == "" and res["iterations0"]["chi2_start"] == res["iterations0"]["chi2_end"]

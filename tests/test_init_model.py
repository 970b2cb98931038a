"""tests/init_model.py on its own (no device): the cosine limits of I10 against libm's acosf, the sampler replay, and the
committed parity scenes -- each inside the left-out cap, on the branch and with the verdict its kind names."""
import numpy as np
import pytest

import init_model as M

f32 = np.float32


def _neighbours(c, count):
    """count floats below c and count above it, ascending, c included"""
    k = M.cos_key(c)
    return [M.key_cos(j) for j in range(k - count, k + count + 1)]


@pytest.mark.parametrize("strict", [True, False])
def test_cos_limit_is_where_the_reference_comparison_flips(strict):
    """I10 for minParallax = 1.0: over the 2^16 floats on either side of the limit the reference's comparison on
    (float)(acosf(c) * 180 / CV_PI) holds up to the limit and never after it."""
    mp = f32(1.0)
    lim = M.cos_limit(mp, strict)
    assert 0.9998 < lim < 0.99986
    cs = _neighbours(lim, 1 << 16)
    holds = np.array([(M.parallax_of(c) > mp) if strict else (M.parallax_of(c) >= mp) for c in cs])
    at = cs.index(lim)
    assert holds[:at + 1].all() and not holds[at + 1:].any()
    assert (np.diff(holds.astype(int)) != 0).sum() == 1


def test_cos_limit_edges():
    assert np.isnan(M.cos_limit(181.0, True)) and np.isnan(M.cos_limit(float("nan"), False))
    assert M.cos_limit(180.0, False) == f32(-1.0) and np.isnan(M.cos_limit(180.0, True))
    assert M.cos_limit(0.0, False) == f32(1.0) and M.cos_limit(-1.0, True) == f32(1.0)
    lim0 = M.cos_limit(0.0, True)          # parallax > 0: every cosine below 1
    assert lim0 < 1.0 and M.key_cos(M.cos_key(lim0) + 1) == f32(1.0)
    for c in (-1.0, -0.0, 0.0, 0.5, 1.0):
        assert M.key_cos(M.cos_key(f32(c))).tobytes() == f32(c).tobytes()
    ks = [M.cos_key(f32(c)) for c in (-1.0, -0.5, -0.0, 0.0, 0.25, 1.0)]
    assert ks == sorted(ks) and len(set(ks)) == len(ks)


def test_sampler_replays_a_scripted_random_int():
    """:82-97: without replacement, the back element moves into position randi"""
    script = iter([0, 0, 9, 3, 3, 3, 0, 4] + [7] * 8)
    calls = []

    def random_int(lo, hi):
        calls.append((lo, hi))
        return min(next(script), hi)
    sets = M.sample_sets(12, 2, random_int)
    # it 0: avail 0..11; 0 -> [11,1..10]; 0 -> 11, [10,1..9]; 9 -> 9, [10,1..8]; 3 -> 3, [10,1,2,8,4..7]; 3 -> 8,
    # [10,1,2,7,4,5,6]; 3 -> 7, [10,1,2,6,4,5]; 0 -> 10, [5,1,2,6,4]; 4 -> 4
    assert sets[0].tolist() == [0, 11, 9, 3, 8, 7, 10, 4]
    assert calls[:8] == [(0, 11 - j) for j in range(8)] and calls[8] == (0, 11)
    assert len(set(sets[1].tolist())) == 8 and sets[1, 0] == 7
    with pytest.raises(ValueError):
        M.sample_sets(7, 1, random_int)
    with pytest.raises(ValueError):
        M.sample_sets(12, 1, lambda lo, hi: hi + 1)
    # the reference's generator gives sets without a repeated index
    rng = np.random.default_rng(0)
    s = M.sample_sets(20, 50, M.reference_random_int(lambda: int(rng.integers(0, 2 ** 31 - 1))))
    assert all(len(set(r.tolist())) == 8 for r in s) and s.min() >= 0 and s.max() < 20


@pytest.fixture(scope="module")
def passes():
    return {k: M.model_pass(M.parity_scene(k)) for k in M.PARITY_SCENES}


@pytest.mark.parametrize("key", list(M.PARITY_SCENES))
def test_committed_scene_is_inside_the_cap_and_gives_its_verdict(passes, key):
    n, _, kind, n_hyp = M.PARITY_SCENES[key]
    m, spread = passes[key]
    oh, of = M.left_out(m, M.BOUND_FACTOR * spread)
    share = (oh.sum() + of.sum()) / (2.0 * n_hyp)
    print("%s: spread %.3e, left out %d + %d of %d, branch %s, success %d, n_good %s" % (
        key, spread, oh.sum(), of.sum(), 2 * n_hyp, "H" if m["used_homography"] else "F", m["success"], m["n_good"].tolist()))
    assert m["N"] == n and share <= M.LEFT_OUT_CAP
    assert spread == 0.0           # the seeds are chosen for it: the device is compared bit for bit
    use_h, success = M.VERDICTS[kind]
    if n >= 300:
        assert m["success"] == success and (use_h is None or m["used_homography"] == use_h)
    if m["success"]:
        tr = M.parity_scene(key)["true"]
        ang = np.degrees(np.arccos(np.clip((np.trace(m["R21"].astype(float) @ tr["R"].T) - 1) / 2, -1, 1)))
        cos_t = float(m["t21"].astype(float) @ tr["t"] / np.linalg.norm(tr["t"]))
        assert ang < 2.0 and cos_t > 0.98, (ang, cos_t)
        tri = m["triangulated"] != 0
        assert tri.sum() >= 50 and (m["P3D"][tri][:, 2] > 0).all() and not m["P3D"][~tri & (m["P3D"] == 0).all(1)].any()


def test_kinds_take_their_branches(passes):
    assert passes["general"][0]["used_homography"] == 0 and passes["general"][0]["success"] == 1
    assert passes["planar"][0]["used_homography"] == 1 and passes["planar"][0]["success"] == 1
    rot = passes["rotation"][0]
    assert rot["success"] == 0 and rot["n_motions"] > 0 and rot["second_best_good"] >= 0.75 * rot["n_good"].max()
    few = passes["few"][0]
    assert few["success"] == 0 and few["n_good"].max() < 50


@pytest.mark.parametrize("n_good", [50, 51, 52])
def test_parallax_rank_around_the_clamp(n_good):
    sc = M.ngood_scene(n_good)
    m, spread = M.model_pass(sc)
    b = m["best_motion"]
    assert spread == 0.0 and m["success"] == 1 and m["n_good"][b] == n_good == m["N"] == m["n_inliers"]
    r = M.check_rt(m["prep"], m["motions"][0][b], m["motions"][1][b], np.ones(n_good, bool), sc["K"], sc["sigma"], "jacobi")
    cs = np.sort(r["cosines"])
    rank = min(50, n_good - 1)
    assert len(cs) == n_good and m["cos_parallax"][b] == cs[rank]
    assert (rank == n_good - 1) == (n_good <= 51) and (n_good < 52 or cs[rank] <= cs[-1])


def test_branch_rule_and_never_won_f():
    """I6 / I7: no hypothesis at all -> RH is NaN, the F branch, N = 0, failure; N < 8 computes nothing"""
    sc = dict(M.make_scene(40, 3), sets=np.zeros((0, 8), np.int32))
    m = M.initialize(sc)
    assert np.isnan(m["RH"]) and m["used_homography"] == 0 and m["best_f"] == -1 and m["n_inliers"] == 0 and m["success"] == 0
    m = M.initialize(M.make_scene(7, 1, n_hyp=4))
    assert m["N"] == 7 and m["success"] == 0 and not m["scores_f"].any() and m["n_bad_set"] == 0
    sc = M.make_scene(30, 2, n_hyp=6)
    sc["sets"][1, 3], sc["sets"][4, 0] = 30, -1
    m = M.initialize(sc)
    assert m["n_bad_set"] == 2 and not m["scores_h"][[1, 4]].any() and not m["masks_f"][[1, 4]].any()
    sc = M.make_scene(30, 2, n_hyp=6)
    sc["matches12"][np.flatnonzero(sc["matches12"] >= 0)[:2]] = len(sc["kp2"])
    m = M.initialize(sc)
    assert m["n_bad_index"] == 2 and m["N"] == 28

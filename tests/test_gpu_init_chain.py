"""The monocular bootstrap chain on the device: orbgpu_search_for_initialization -> orbgpu_initializer on a synthetic
two-view scene with a planted motion.  The figures are printed; the only thresholds are the model's (tests/init_model.py)
verdicts on the same input."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import init_model as M  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    from orb_slam2_map_amd import lib
    if lib.device_count() < 1:
        pytest.skip("no HIP device")
    return lib


def _frames(G, sc, seed):
    """level-0 key points with random descriptors; a matched pair shares its descriptor up to 6 flipped bits"""
    rng = np.random.default_rng(seed)
    n1, n2 = len(sc["kp1"]), len(sc["kp2"])
    d1, d2 = rng.integers(0, 256, (n1, 32), dtype=np.uint8), rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    rows = np.flatnonzero(sc["matches12"] >= 0)
    d2[sc["matches12"][rows]] = d1[rows]
    for i in rows:
        for b in rng.integers(0, 256, 6):
            d2[sc["matches12"][i], b // 8] ^= np.uint8(1 << (b % 8))
    out = []
    for kp, d in ((sc["kp1"], d1), (sc["kp2"], d2)):
        n = len(kp)
        out.append(G.Frame(kp[:, 0].copy(), kp[:, 1].copy(), np.zeros(n, np.int32), np.zeros(n, np.float32), np.full(n, -1, np.float32),
                           d, 640, 480, np.ones(8, np.float32)))
    return out


def _figures(r, true):
    R = np.asarray(r["R21"], float)
    ang = float(np.degrees(np.arccos(np.clip((np.trace(R @ true["R"].T) - 1) / 2, -1, 1))))
    cos_t = float(np.asarray(r["t21"], float) @ true["t"] / np.linalg.norm(true["t"]))
    return ang, cos_t


def test_search_for_initialization_feeds_the_initializer(G):
    truth = M.make_scene(300, 424242, "general", n_hyp=1, n1=400, n2=400, noise_px=0.3, outlier_frac=0.0)
    f1, f2 = _frames(G, truth, 7)
    nm, matches12, _ = G.search_for_initialization(f1, f2, truth["kp1"], 100, 0.9, True)
    agree = int((matches12[truth["matches12"] >= 0] == truth["matches12"][truth["matches12"] >= 0]).sum())
    n = int((matches12 >= 0).sum())
    print("matcher: %d matches (%d returned), %d of the 300 planted pairs" % (n, nm, agree))
    assert n == nm >= 100           # Tracking.cc:880 asks for 100 before it calls Initialize
    rng = np.random.default_rng(5)
    sets = M.sample_sets(n, 200, M.reference_random_int(lambda: int(rng.integers(0, 2 ** 31 - 1))))
    sc = dict(truth, matches12=matches12.astype(np.int32), sets=sets)
    m, spread = M.model_pass(sc)
    r = G.initializer(sc)
    ang, cos_t = _figures(r, truth["true"])
    ang_m, cos_m = _figures(m, truth["true"])
    print("initializer: success %d (model %d), branch %s, n_good %s, parallax %.3f deg, rotation off by %.4f deg (model %.4f), "
          "cos(t21, planted) %.6f (model %.6f), %d points triangulated, model spread %.3e" % (
              r["success"], m["success"], "H" if r["used_homography"] else "F", r["n_good"].tolist(), r["parallax_deg"], ang, ang_m,
              cos_t, cos_m, int(r["triangulated"].sum()), spread))
    bound = M.BOUND_FACTOR * spread
    assert m["success"] == 1 and r["success"] == 1 and r["used_homography"] == m["used_homography"]
    assert M.dev(m["R21"], r["R21"]) <= bound and M.dev(m["t21"], r["t21"]) <= bound
    assert abs(ang - ang_m) <= np.degrees(4 * bound) and abs(cos_t - cos_m) <= 4 * bound
    assert ang_m < 1.0 and cos_m > 0.99           # the model's own verdict: near the planted motion
    # the two frames swapped in one argument only (the key points, not the matches): the pairs no longer follow one motion
    swapped = dict(sc, kp1=sc["kp2"], kp2=sc["kp1"])
    ms, rs = M.initialize(swapped), G.initializer(swapped)
    print("swapped key points: success %d (model %d), n_good %s" % (rs["success"], ms["success"], rs["n_good"].tolist()))
    assert ms["success"] == 0 and rs["success"] == 0 and not rs["triangulated"].any() and not rs["R21"].any()

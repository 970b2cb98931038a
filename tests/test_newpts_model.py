"""The numpy restatement of LocalMapping::CreateNewMapPoints (newpts_model.py) on its own, without a device: the parity
scenes stay under the left-out cap, created points are the true points on noise-free scenes, crafted pairs reach every status
code, the reference's quirks are restated and not repaired, and a handful of mutations of the model are each caught.

Two codes are argued from the code instead of constructed: W_ZERO needs the float null vector's fourth component to be
exactly 0, and ZERO_DIST a created point that coincides with a camera centre in float although its depth passed `> 0` --
both are single float values no geometry reaches on purpose; the branches are the literal `== 0` tests of :333 and :422."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import newpts_model as M  # noqa: E402

f32 = np.float32
# Largest |created - true| / max(1, |true|) over the three noise-free scenes below, measured from the model: 1.47e-6 in each
# (float pixels and a float A over parallaxes of a few degrees; the back-projected points are closer).  The assertion is
# 16 x the largest figure, as test_init_fp64.py's.
NOISE_FREE_MEASURED = 1.47e-6
NOISE_FREE_BOUND = 16 * NOISE_FREE_MEASURED


@pytest.mark.parametrize("name", list(M.SCENES))
def test_the_model_alone_stays_under_the_cap(name):
    m, spread, near, matched = M.model_pass(M.scene(name))
    print("%s: spread %.3g, %d of %d near a threshold" % (name, spread, int(near.sum()), matched))
    assert near.sum() <= M.LEFT_OUT_CAP * max(matched, 1)
    assert (m["n_created"] == (m["status"] > 0).sum(1)).all() and (m["n_matches"] == (m["match12"] >= 0).sum(1)).all()
    assert not m["x3d"][m["status"] <= 0].any()


@pytest.mark.parametrize("mix", ["mono", "stereo", "mixed"])
def test_noise_free_points_are_the_true_points(mix):
    sc = M.make_scene(31, mix=mix, noise=0.0, spoil_ur=0.0, wrong_octave=0.0)
    m = M.run(sc)
    worst = 0.0
    for k in range(len(sc["neighbours"])):
        for i in np.nonzero(m["status"][k] > 0)[0]:
            worst = max(worst, M.dev(sc["points"][sc["kf1"]["point"][i]], m["x3d"][k, i]))
    print("%s: %d created, largest deviation from the true point %.3g" % (mix, int(m["n_created"].sum()), worst))
    assert m["n_created"].sum() > 80
    assert worst <= NOISE_FREE_BOUND
    # nothing but parallax rejects without noise
    assert set(np.unique(m["status"])) <= {M.NONE, M.TRIANGULATED, M.UNPROJECT1, M.UNPROJECT2, M.LOW_PARALLAX}


# ---- crafted pairs ---------------------------------------------------------------------------------------------------------------
def one(X, C=(0, 0, 0), stereo=False, octave=0, mbf=40.0, depth=None, dv=0.0, dur=0.0, cos_stereo=None, pixel=None):
    """a frame with one key point: the projection of X from a camera at C looking down +z"""
    R, C = np.eye(3), np.array(C, float)
    T, Twc = M._pose(R, C)
    Xc = np.array(X, float) - C
    u, v = (M.FX * Xc[0] / Xc[2] + M.CX, M.FY * Xc[1] / Xc[2] + M.CY) if pixel is None else pixel
    z = Xc[2] if depth is None else depth
    sf, sg = M.levels()
    with np.errstate(all="ignore"):
        cs = f32(math.cos(2 * math.atan2(M.MB / 2, z))) if cos_stereo is None else f32(cos_stereo)
    return {"kp_x": np.array([u], f32), "kp_y": np.array([v + dv], f32), "kp_octave": np.array([octave], np.int32),
            "kp_angle": np.zeros(1, f32), "u_right": np.array([u - M.FX * M.MB / Xc[2] + dur if stereo else -1], f32),
            "desc": np.zeros((1, 32), np.uint8), "has_mp": np.zeros(1, np.uint8), "node": np.zeros(1, np.int32),
            "depth": np.array([z if stereo else -1], f32), "kp_raw": None, "cos_stereo": np.array([cs], f32),
            "Tcw": T.reshape(16), "Twc": Twc.reshape(16), "K": (M.FX, M.FY, M.CX, M.CY), "mbf": mbf, "level_sigma2": sg,
            "scale_factors": sf}


RF = f32(1.5) * f32(1.2)
X0 = (0.3, -0.2, 5.0)


def status(k1, k2, **kw):
    return M.pair(k1, k2, RF, 0, 0, **kw)[0]


def crafted_pairs():
    """(name, key frame 1, key frame 2, status): one key point each, every status code that can be constructed.  Shared with
    tests/test_gpu_newpts.py, which runs the same pairs on the device."""
    wide, tiny = (0.5, 0, 0), (0.01, 0, 0)
    # the disparity has the wrong sign: the rays meet behind both cameras
    behind = one(X0, wide, pixel=(M.CX + 80.0, M.CY - 20.0))
    return [
        ("triangulated", one(X0), one(X0, wide), M.TRIANGULATED),
        ("unproject 1", one(X0, stereo=True), one(X0, tiny), M.UNPROJECT1),
        ("unproject 2", one(X0), one(X0, tiny, stereo=True), M.UNPROJECT2),
        ("low parallax", one(X0), one(X0, tiny), M.LOW_PARALLAX),
        ("z1", one(X0), behind, M.Z1),
        # key frame 2 stands beyond the point key frame 1's depth gives
        ("z2", one(X0, stereo=True), one((0.005 + 0.06 * 4, -0.04 * 4, 12.0), (0.005, 0, 8.0)), M.Z2),
        ("reprojection 1, stereo", one(X0, stereo=True, dur=10.0), one(X0, wide), M.REPROJ1),
        ("reprojection 2, stereo", one(X0), one(X0, wide, stereo=True, dur=10.0), M.REPROJ2),
        ("reprojection 1, mono", one(X0, dv=9.0), one(X0, wide), M.REPROJ1),
        # the triangulation splits the error evenly: it passes key frame 1 at octave 2 (5.991 x 2.07) and fails key frame 2
        ("reprojection 2, mono", one(X0, octave=2), one(X0, wide, dv=6.0), M.REPROJ2),
        ("scale, low side", one(X0, octave=5), one(X0, wide, octave=0), M.SCALE),   # ratioDist * ratioFactor < ratioOctave
        ("scale, high side", one(X0, octave=0), one(X0, wide, octave=5), M.SCALE),  # ratioDist > ratioOctave * ratioFactor
        ("non-finite", one(X0, stereo=True, depth=np.inf, cos_stereo=0.5), one(X0, tiny), M.NON_FINITE),
        ("stereo depth", one(X0, stereo=True, depth=-1.0, cos_stereo=0.5), one(X0, tiny), M.STEREO_DEPTH),
        ("bad octave", one(X0, octave=9), one(X0, wide), M.BAD_OCTAVE),
    ]


def test_crafted_pairs_reach_every_status_code():
    pairs = crafted_pairs()
    for name, k1, k2, want in pairs:
        assert status(k1, k2) == want, name
    # every code but the two argued from the code (module docstring)
    assert {p[3] for p in pairs} == {M.TRIANGULATED, M.UNPROJECT1, M.UNPROJECT2, M.LOW_PARALLAX, M.Z1, M.Z2, M.REPROJ1, M.REPROJ2,
                                     M.SCALE, M.NON_FINITE, M.STEREO_DEPTH, M.BAD_OCTAVE}
    st, X, _ = M.pair(one(X0), one(X0, (0.5, 0, 0)), RF, 0, 0)
    assert M.dev(X0, X) < NOISE_FREE_BOUND
    st, X, _ = M.pair(pairs[4][1], pairs[4][2], RF, 0, 0)
    assert st == M.Z1 and not X.any()  # zeros unless status > 0


def cos2_pair():
    """stereo-stereo, cos_stereo2 < cosParallaxRays < cos_stereo1: triangulated as the reference has it (cosParallaxStereo2 is
    never computed, :311-314); key frame 2's back-projection if it were"""
    return one(X0, stereo=True, cos_stereo=0.99999), one(X0, (0.15, 0, 0), stereo=True, cos_stereo=0.9990)


def mbf_pair():
    """key frame 2 is stereo with a baseline of its own; its u_right is consistent with key frame 1's mbf only (:406)"""
    k2 = one(X0, (0.5, 0, 0), stereo=True, mbf=80.0)
    return one(X0, stereo=True), k2


def swapped_pair():
    """mono-mono with a reprojection error between 5.991 and 7.8 sigma2"""
    return one(X0), one(X0, (0.5, 0, 0), dv=5.2)


def test_quirks_are_restated_not_repaired():
    k1, k2 = cos2_pair()
    assert status(k1, k2) == M.TRIANGULATED and status(k1, k2, mut="cos2_always") == M.UNPROJECT2
    k1, k2 = mbf_pair()
    assert status(k1, k2) == M.TRIANGULATED and status(k1, k2, mut="own_mbf") == M.REPROJ2
    # two key points of key frame 1 create a point each on one key point of key frame 2
    sc = M.scene("mono")
    m = M.run(sc)
    i = int(np.nonzero(m["status"][0] > 0)[0][0])
    spare = int(np.nonzero((m["match12"] < 0).all(0) & (np.arange(len(m["match12"][0])) != i))[0][0])
    for k in ("kp_x", "kp_y", "kp_octave", "kp_angle", "u_right", "desc", "has_mp", "node", "depth", "cos_stereo"):
        sc["kf1"][k][spare] = sc["kf1"][k][i]
    m2 = M.run(sc)
    j = m2["match12"][0][i]
    assert j >= 0 and m2["match12"][0][spare] == j
    assert m2["status"][0][i] > 0 and m2["status"][0][spare] > 0
    assert m2["x3d"][0][i].tobytes() == m2["x3d"][0][spare].tobytes()


def test_mutations_of_the_model_are_caught():
    sc = M.scene("mixed")
    base, mut = M.run(sc), M.run(sc, mut="no_has_mp_update")
    assert np.array_equal(base["match12"][0], mut["match12"][0]) and not np.array_equal(base["match12"][1], mut["match12"][1])
    k1, k2 = mbf_pair()
    assert status(k1, k2) != status(k1, k2, mut="own_mbf")
    k1, k2 = cos2_pair()
    assert status(k1, k2) != status(k1, k2, mut="cos2_always")
    k1, k2 = swapped_pair()
    _, _, g = M.pair(k1, k2, RF, 0, 0)
    worst = max(g["e1"][0], g.get("e2", (-1,))[0])
    assert 0 < worst < 7.8 / 5.991 - 1  # between the two thresholds
    assert status(k1, k2) in (M.REPROJ1, M.REPROJ2) and status(k1, k2, mut="thresholds_swapped") == M.TRIANGULATED
    k1, k2 = one(X0, octave=5), one(X0, (0.5, 0, 0), octave=0)
    assert status(k1, k2) == M.SCALE and status(k1, k2, mut="ratio_one_sided") == M.TRIANGULATED


def test_stop_and_chain_in_the_model():
    sc = M.scene("mixed")
    full, stopped = M.run(sc), M.run(sc, stop=1)
    assert stopped["n_done"] == 1 and np.array_equal(full["match12"][0], stopped["match12"][0])
    assert (stopped["match12"][1:] == -1).all() and not stopped["status"][1:].any()
    created0 = full["status"][0] > 0
    assert created0.sum() > 20 and (full["match12"][1:, created0] == -1).all()

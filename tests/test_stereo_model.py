"""The stereo model (stereo_model.py) against a literal transcription of Frame::ComputeStereoMatches
(Frame.cc:466-638: row table of lists, candidate loop in list order, windows taken as slices), and the reach of its
branches over seeded synthetic stereo pairs.  CPU only: key points and pyramids come from the oracle."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import stereo_model as M  # noqa: E402

F = np.float32


def literal(kps_l, desc_l, kps_r, desc_r, planes_l, planes_r, scale, inv_scale, mbf, fx):
    n = len(kps_l)
    mvuRight = [F(-1.0)] * n
    mvDepth = [F(-1.0)] * n
    nRows = planes_l[0].shape[0]
    nl = len(scale)
    vRowIndices = [[] for _ in range(nRows)]
    for iR in range(len(kps_r)):
        kp = kps_r[iR]
        oc = int(kp["octave"])
        kpY = F(kp["y"])
        if not (0 <= oc < nl) or not (kpY > F(-1e6) and kpY < F(1e6)):  # S4
            continue
        r = F(2.0) * F(scale[oc])
        maxr = int(np.ceil(kpY + r))
        minr = int(np.floor(kpY - r))
        for yi in range(minr, maxr + 1):
            if 0 <= yi < nRows:
                vRowIndices[yi].append(iR)
    mb = F(mbf) / F(fx)
    minZ = mb
    minD = F(-3)
    maxD = F(mbf) / minZ
    vDistIdx = []
    for iL in range(n):
        kpL = kps_l[iL]
        levelL = int(kpL["octave"])
        vL, uL = F(kpL["y"]), F(kpL["x"])
        if not (0 <= levelL < nl and vL > -1 and vL < nRows):  # S3
            continue
        vCandidates = vRowIndices[int(vL)]
        if not vCandidates:
            continue
        minU = uL - maxD
        maxU = uL - minD
        if maxU < 0:
            continue
        bestDist, bestIdxR = 100, 0
        dL = desc_l[iL]
        for iR in vCandidates:
            kpR = kps_r[iR]
            if int(kpR["octave"]) < levelL - 1 or int(kpR["octave"]) > levelL + 1:
                continue
            uR = F(kpR["x"])
            if uR >= minU and uR <= maxU:
                dist = int(np.unpackbits(np.bitwise_xor(dL, desc_r[iR])).sum())
                if dist < bestDist:
                    bestDist, bestIdxR = dist, iR
        if bestDist < 100:
            uR0 = F(kps_r[bestIdxR]["x"])
            scaleFactor = F(inv_scale[levelL])
            scaleduL = M.round_half_away(uL * scaleFactor)
            scaledvL = M.round_half_away(vL * scaleFactor)
            scaleduR0 = M.round_half_away(uR0 * scaleFactor)
            w = 5
            Lw = 5
            iniu = scaleduR0 + F(Lw) - F(w)
            endu = scaleduR0 + F(Lw) + F(w) + F(1)
            cols, rows = planes_r[levelL].shape[1], planes_r[levelL].shape[0]
            if iniu < 0 or endu >= cols:
                continue
            if not (scaleduL - w >= 0 and scaleduL + w < cols and scaledvL - w >= 0 and scaledvL + w < rows and
                    scaleduR0 - Lw - w >= 0):  # S3
                continue
            yl, xl, xr = int(scaledvL), int(scaleduL), int(scaleduR0)
            IL = planes_l[levelL][yl - w:yl + w + 1, xl - w:xl + w + 1].astype(np.float32)
            IL = IL - IL[w, w]
            bestDist2, bestincR = 2147483647, 0
            vDists = [F(0)] * (2 * Lw + 1)
            for incR in range(-Lw, Lw + 1):
                IR = planes_r[levelL][yl - w:yl + w + 1, xr + incR - w:xr + incR + w + 1].astype(np.float32)
                IR = IR - IR[w, w]
                dist = F(np.abs(IL - IR).astype(np.float64).sum())
                if dist < bestDist2:
                    bestDist2, bestincR = int(dist), incR
                vDists[Lw + incR] = dist
            if bestincR == -Lw or bestincR == Lw:
                continue
            dist1, dist2, dist3 = vDists[Lw + bestincR - 1], vDists[Lw + bestincR], vDists[Lw + bestincR + 1]
            deltaR = (dist1 - dist3) / (F(2.0) * (dist1 + dist3 - F(2.0) * dist2))
            if deltaR < -1 or deltaR > 1:
                continue
            bestuR = F(scale[levelL]) * (F(scaleduR0) + F(bestincR) + deltaR)
            disparity = uL - bestuR
            if disparity >= 0 and disparity < maxD:
                if disparity <= 0:
                    disparity = F(0.01)
                    bestuR = F(float(uL) - 0.01)
                mvDepth[iL] = F(mbf) / disparity
                mvuRight[iL] = bestuR
                vDistIdx.append((bestDist2, iL))
    vDistIdx.sort()
    if vDistIdx:  # S2
        median = F(vDistIdx[len(vDistIdx) // 2][0])
        thDist = F(1.5) * F(1.4) * median
        for i in range(len(vDistIdx) - 1, -1, -1):
            if vDistIdx[i][0] < thDist:
                break
            mvuRight[vDistIdx[i][1]] = F(-1)
            mvDepth[vDistIdx[i][1]] = F(-1)
    return np.array(mvuRight, F), np.array(mvDepth, F)


@pytest.fixture(scope="module")
def O():
    import __graft_entry__  # noqa: F401  (puts the repository on sys.path)
    from oracle import oracle_py
    oracle_py.build()
    return oracle_py


def _pair(O, w, h, seed, t, nf):
    from orb_slam2_map_amd.synth import StereoStream
    st = StereoStream(w, h, seed)
    left, right, _ = st.frame(t)
    el, er = O.Extractor(nf), O.Extractor(nf)
    kl, dl = el.extract(left)
    kr, dr = er.extract(right)
    return st, (kl, dl, kr, dr), M.oracle_planes(el), M.oracle_planes(er), el.scale_factors(), el.inv_scale_factors()


@pytest.mark.parametrize("w,h,seed,nf", [(320, 240, 1, 300), (400, 200, 2, 400)])
def test_model_equals_literal_transcription(O, w, h, seed, nf):
    st, lists, pl, pr, sc, isc = _pair(O, w, h, seed, 0, nf)
    rng = np.random.default_rng(seed)
    for kl, dl, kr, dr in (lists, M.craft_lists(*lists, rng, w, h, 8)):
        for mbf in (st.bf, F(st.bf / 20)):
            u, d, _ = M.stereo_matches(kl, dl, kr, dr, pl, pr, sc, isc, mbf, st.fx)
            lu, ld = literal(kl, dl, kr, dr, pl, pr, sc, isc, mbf, st.fx)
            assert np.array_equal(u.view(np.int32), lu.view(np.int32))
            assert np.array_equal(d.view(np.int32), ld.view(np.int32))


def test_model_reaches_every_branch(O):
    seen = np.zeros(len(M.REASONS), np.int64)
    for w, h, seed in ((1241, 376, 3), (640, 480, 4)):
        st, lists, pl, pr, sc, isc = _pair(O, w, h, seed, 1, 1000)
        rng = np.random.default_rng(seed)
        for kl, dl, kr, dr in (lists, M.craft_lists(*lists, rng, w, h, 8)):
            for mbf in (st.bf, F(st.bf / 20)):
                _, _, reason = M.stereo_matches(kl, dl, kr, dr, pl, pr, sc, isc, mbf, st.fx)
                seen += np.bincount(reason, minlength=len(M.REASONS))
    # the zero-disparity clamp needs a symmetric scene (stereo_model.mirrored_pair)
    left, right = M.mirrored_pair(640, 480, 320, 21)
    el, er = O.Extractor(1000), O.Extractor(1000)
    lists = el.extract(left) + er.extract(right)
    kl, dl, kr, dr = M.clamp_keys(lists[0], lists[1], lists[2], lists[3], 320, 480)
    _, _, reason = M.stereo_matches(kl, dl, kr, dr, M.oracle_planes(el), M.oracle_planes(er), el.scale_factors(),
                                    el.inv_scale_factors(), 380.0, 700.0)
    seen += np.bincount(reason, minlength=len(M.REASONS))
    # |deltaR| > 1 cannot happen: bestincR is a strict minimum, so with a = d1 - d2 > 0 and b = d3 - d2 >= 0,
    # |deltaR| = |a - b| / (2 (a + b)) <= 1/2
    for r in M.REASONS:
        if r != "delta":
            assert seen[M.REASONS.index(r)] > 0, r
    assert seen[M.REASONS.index("delta")] == 0

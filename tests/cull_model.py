"""LocalMapping::KeyFrameCulling over the observation graph (orbgpu_covis_keyframe_culling, orbgpu_covis_observations,
orbgpu_covis_graph_set_keypoints) restated twice, in plain Python -- test infrastructure, like covis_model.py, which both
restatements extend.

1. `CullGraph`: covis_model.CovisGraph with V1's attribute byte per slot, MapPoint::Observations() for a list of ids and
   convention V8 (include/orbgpu.h).  It is what the device is compared with, entry for entry.
2. `CullPointerMap`: covis_model.PointerMap whose key frames carry mvKeysUn octaves, mvuRight, mvDepth, mThDepth and
   mbNotErase and whose map points carry the weighted nObs (MapPoint.cc:105-108, :119-122).  KeyFrameCulling is written
   statement by statement from LocalMapping.cc:632-698 and calls KeyFrame::SetBadFlag as covis_model restates it, so the
   cascade -- EraseObservation per slot, MapPoint::SetBadFlag at nObs <= 2 -- is the reference's and not V8's."""
import numpy as np

import covis_model as M
from covis_model import Refused  # noqa: F401

MAX_LEVELS = 16
KP_OCTAVE = 0x0F
KP_STEREO = 0x40
KP_FAR = 0x80
KP_RESERVED = 0x30
MAX_CANDIDATES = 1 << 16
MAX_CALL = 1 << 20


def pack_keypoint(octave, stereo, far):
    """V1's attribute byte"""
    assert 0 <= octave < MAX_LEVELS
    return octave | (KP_STEREO if stereo else 0) | (KP_FAR if far else 0)


class CullGraph(M.CovisGraph):
    def clear(self):
        super().clear()
        self.kp = {}  # key frame id -> one byte per slot

    def add_keyframe(self, kf_id, n_slots, mp_ids=None):
        super().add_keyframe(kf_id, n_slots, mp_ids)
        self.kp[int(kf_id)] = [0] * int(n_slots)

    def set_keypoints(self, kf_id, kp):
        kf_id = int(kf_id)
        kp = [] if kp is None else [int(b) for b in kp]
        row = self.row_of.get(kf_id)
        if row is None or len(kp) != len(row.slots) or any(b & KP_RESERVED or not 0 <= b <= 255 for b in kp):
            raise Refused("set_keypoints")
        if not row.bad:
            self.kp[kf_id] = kp

    def _weight(self, row, i):
        return 2 if self.kp[row.id][i] & KP_STEREO else 1

    def observations(self, mp_ids):
        """(n_obs, n_slots) per id: MapPoint::Observations() under V2 and the unweighted number of slots"""
        ids = [int(p) for p in mp_ids]
        if len(ids) > MAX_CALL or any(p < -1 for p in ids):
            raise Refused("observations")
        obs, cnt = {}, {}
        for row in self.rows:
            if row.bad:
                continue
            for i, p in enumerate(row.slots):
                if p >= 0:
                    obs[p] = obs.get(p, 0) + self._weight(row, i)
                    cnt[p] = cnt.get(p, 0) + 1
        return (np.array([obs.get(p, 0) for p in ids], np.int32), np.array([cnt.get(p, 0) for p in ids], np.int32))

    def keyframe_culling(self, kf_ids, not_erase=None, th_obs=3, order_free=False):
        """V8.  order_free=True evaluates every candidate on the relation at the start of the call (what a parallel
        evaluation would do; the tests show that it differs)."""
        ids = [int(k) for k in kf_ids]
        ne = [0] * len(ids) if not_erase is None else [int(b) for b in not_erase]
        if len(ids) > MAX_CANDIDATES or len(ne) != len(ids) or not 1 <= int(th_obs) <= 255 or any(k < 0 for k in ids):
            raise Refused("keyframe_culling")
        th = int(th_obs)
        live = {}  # S: (row id, idx) -> point, per point the set of its slots
        slots_of = {}
        obs = {}
        for row in self.rows:
            if row.bad:
                continue
            for i, p in enumerate(row.slots):
                if p >= 0:
                    live[(row.id, i)] = p
                    slots_of.setdefault(p, set()).add((row.id, i))
                    obs[p] = obs.get(p, 0) + self._weight(row, i)
        query = set()
        for k in ids:
            row = self.row_of.get(k)
            if k != 0 and row is not None and not row.bad:
                query.update(p for p in row.slots if p >= 0)
        culled, bad_points = set(), set()
        verdict, n_mps, n_red = [], [], []
        for k, keep in zip(ids, ne):
            row = self.row_of.get(k)
            if k == 0 or row is None or row.bad or k in culled:
                verdict.append(-1), n_mps.append(0), n_red.append(0)
                continue
            kp = self.kp[k]
            mps = red = 0
            for i in range(len(row.slots)):
                p = live.get((k, i))
                if p is None or kp[i] & KP_FAR:
                    continue
                mps += 1
                if obs[p] > th:
                    others = sum(1 for (k2, j) in slots_of[p] if k2 != k and (self.kp[k2][j] & KP_OCTAVE) <= (kp[i] & KP_OCTAVE) + 1)
                    if others >= th:
                        red += 1
            n_mps.append(mps), n_red.append(red)
            if not float(red) > 0.9 * float(mps):
                verdict.append(0)
            elif keep:
                verdict.append(2)
            else:
                verdict.append(1)
                if order_free:
                    continue
                culled.add(k)
                touched = set()
                for i in range(len(row.slots)):
                    p = live.pop((k, i), None)
                    if p is not None:
                        slots_of[p].discard((k, i))
                        obs[p] -= self._weight(row, i)
                        touched.add(p)
                for p in touched:
                    if obs[p] <= 2:  # MapPoint.cc:130
                        bad_points.add(p)
                        for s in slots_of.pop(p):
                            del live[s]
        return dict(verdict=np.array(verdict, np.int8), n_mps=np.array(n_mps, np.int32), n_redundant=np.array(n_red, np.int32),
                    bad_point_ids=np.array(sorted(bad_points), np.int64), n_culled=verdict.count(1), n_to_be_erased=verdict.count(2),
                    n_skipped=verdict.count(-1), n_points_bad=len(bad_points), n_query_points=len(query))

    def predicted(self, kf_ids, res):
        """the slot lists V8 predicts after the caller has run SetBadFlag on the verdict-1 key frames: {id: slots} of the
        rows that are not bad"""
        gone = {int(k) for k, v in zip(kf_ids, res["verdict"]) if v == 1}
        dead = set(int(p) for p in res["bad_point_ids"])
        return {r.id: [-1 if p in dead else p for p in r.slots] for r in self.rows if not r.bad and r.id not in gone}

    def state(self):
        return {r.id: list(r.slots) for r in self.rows if not r.bad}


class CullPointerMap(M.PointerMap):
    """key frames with mvKeysUn[i].octave (`octave`), mvuRight, mvDepth, mThDepth, mbNotErase, mbToBeErased; the weighted nObs"""

    def __init__(self, hooks=None, mbMonocular=False, **kw):
        super().__init__(hooks, **kw)
        self.mbMonocular = mbMonocular
        self.mpCurrentKeyFrame = None

    def AddKeyFrame(self, kf_id, n, octave=None, mvuRight=None, mvDepth=None, mThDepth=40.0):
        kf = super().AddKeyFrame(kf_id, n)
        kf.octave = [0] * n if octave is None else [int(o) for o in octave]
        kf.mvuRight = [-1.0] * n if mvuRight is None else [float(u) for u in mvuRight]
        kf.mvDepth = [-1.0] * n if mvDepth is None else [float(d) for d in mvDepth]
        kf.mThDepth = float(mThDepth)
        kf.mbNotErase = False
        kf.mbToBeErased = False
        self.hooks.set_keypoints(kf_id, self.keypoint_bytes(kf))  # KeyFrame's constructor hook
        return kf

    def keypoint_bytes(self, kf):
        """CovisibilityGraphT::SetKeyPoints"""
        return [pack_keypoint(kf.octave[i], kf.mvuRight[i] >= 0,
                              not self.mbMonocular and (kf.mvDepth[i] > kf.mThDepth or kf.mvDepth[i] < 0)) for i in range(kf.N)]

    @staticmethod
    def _w(kf, idx):
        return 2 if kf.mvuRight[idx] >= 0 else 1  # MapPoint.cc:105-108

    def AddObservations(self, kf, pairs):
        done = []
        for idx, mp in pairs:
            if kf in mp.mObservations or kf.mvpMapPoints[idx] is not None or mp.mbBad or kf.mbBad:
                continue
            kf.mvpMapPoints[idx] = mp
            mp.mObservations[kf] = idx
            mp.nObs += self._w(kf, idx)
            done.append((idx, mp.mnId))
        if done:
            self.hooks.set_slots([kf.mnId] * len(done), [d[0] for d in done], [d[1] for d in done])

    def _erase_observation(self, mp, kf):
        """MapPoint::EraseObservation (MapPoint.cc:111-137)"""
        bad = False
        if kf in mp.mObservations:
            mp.nObs -= self._w(kf, mp.mObservations[kf])
            del mp.mObservations[kf]
            if mp.nObs <= 2:
                bad = True
        if bad:
            self.SetBadFlagMapPoint(mp)

    def Replace(self, mp, other):
        raise NotImplementedError("not part of the culling tests")

    def SetBadFlagKeyFrame(self, kf):
        """KeyFrame::SetBadFlag with its mbNotErase branch (KeyFrame.cc:495-501)"""
        if kf.mnId == 0:
            return
        if kf.mbNotErase:
            kf.mbToBeErased = True
            return
        super().SetBadFlagKeyFrame(kf)

    def KeyFrameCulling(self, vpLocalKeyFrames, thObs=3, apply=True):
        """LocalMapping.cc:632-698 over vpLocalKeyFrames = mpCurrentKeyFrame->GetVectorCovisibleKeyFrames().  Returns the
        per-candidate (verdict, nMPs, nRedundantObservations) with V8's verdict codes and the ids of the points the run
        turned bad.  (A key frame that is bad already is passed over, as V8 does: the reference's covisible list holds
        none.)"""
        bad_before = {p.mnId for p in self.mps.values() if p.mbBad}
        out = []
        for pKF in vpLocalKeyFrames:
            if pKF is None or pKF.mnId == 0 or pKF.mbBad:
                out.append((-1, 0, 0))
                continue
            vpMapPoints = list(pKF.mvpMapPoints)
            nRedundantObservations = 0
            nMPs = 0
            for i in range(len(vpMapPoints)):
                pMP = vpMapPoints[i]
                if pMP is not None:
                    if not pMP.isBad():
                        if not self.mbMonocular:
                            if pKF.mvDepth[i] > pKF.mThDepth or pKF.mvDepth[i] < 0:
                                continue
                        nMPs += 1
                        if pMP.nObs > thObs:
                            scaleLevel = pKF.octave[i]
                            nObs = 0
                            for pKFi, idx in pMP.GetObservations():
                                if pKFi is pKF:
                                    continue
                                scaleLeveli = pKFi.octave[idx]
                                if scaleLeveli <= scaleLevel + 1:
                                    nObs += 1
                                    if nObs >= thObs:
                                        break
                            if nObs >= thObs:
                                nRedundantObservations += 1
            if nRedundantObservations > 0.9 * nMPs:
                if pKF.mbNotErase:
                    out.append((2, nMPs, nRedundantObservations))
                else:
                    out.append((1, nMPs, nRedundantObservations))
                if apply:
                    self.SetBadFlagKeyFrame(pKF)
            else:
                out.append((0, nMPs, nRedundantObservations))
        bad_now = {p.mnId for p in self.mps.values() if p.mbBad}
        return out, sorted(bad_now - bad_before)


# ---- scenes (shared by the tests, tools/fuzz_cull.py and tools/bench_cull.py) ------------------------------------------
OCTAVES = (0, 1, 2, 3, 4, 5, 6, 7, 15)


def random_map(rng, pm, n_kf=12, n_pts=60, first_kf=None, first_mp=None, sizes=None, share=0.75):
    """plants key frames with random octaves, stereo and far flags over a common pool of points; returns the key frames"""
    first_kf = int(rng.integers(0, 3)) if first_kf is None else first_kf
    first_mp = int(rng.choice([0, 2 ** 33])) if first_mp is None else first_mp
    mps = [pm.NewMapPoint(first_mp + 3 * i) for i in range(n_pts)]
    kfs = []
    kf_id = first_kf
    for _ in range(n_kf):
        n = int(rng.choice(M.SLOT_SIZES if sizes is None else sizes)) if rng.random() < 0.6 else int(rng.integers(0, 140))
        narrow = rng.random() < 0.5  # octaves close together: redundancy is likely
        octave = rng.choice(OCTAVES[:3] if narrow else OCTAVES, size=n)
        stereo = rng.random(n) < rng.choice([0.0, 0.5, 1.0])
        depth = np.where(stereo, rng.uniform(0.5, 60.0, n), -1.0)
        if rng.random() < 0.3:
            depth = np.where(stereo, rng.uniform(0.5, 30.0, n), depth)  # all stereo points close
        kf = pm.AddKeyFrame(kf_id, n, octave, np.where(stereo, 100.0, -1.0), depth, 40.0)
        kf_id += int(rng.integers(1, 4))
        take = rng.permutation(n)[:int(n * rng.uniform(0.3, 1.0))]
        chosen = rng.permutation(n_pts)[:len(take)] if len(take) <= n_pts else rng.integers(0, n_pts, len(take))
        pairs = [(int(i), mps[int(c)] if rng.random() < share else mps[int(rng.integers(n_pts))]) for i, c in zip(take, chosen)]
        pm.AddObservations(kf, pairs)
        kfs.append(kf)
    return kfs


def random_candidates(rng, kfs, n=None):
    """a covisible list: live key frames in random order, now and then id 0, an unknown id, a bad one or a duplicate"""
    live = [k.mnId for k in kfs if not k.mbBad]
    n = int(rng.integers(0, len(live) + 1)) if n is None else min(n, len(live))
    ids = [live[int(i)] for i in rng.permutation(len(live))[:n]]
    for extra in (0, 10 ** 12 + 7):
        if rng.random() < 0.3:
            ids.insert(int(rng.integers(len(ids) + 1)), extra)
    if ids and rng.random() < 0.4:
        ids.insert(int(rng.integers(len(ids) + 1)), ids[int(rng.integers(len(ids)))])
    bad = [k.mnId for k in kfs if k.mbBad]
    if bad and rng.random() < 0.4:
        ids.insert(int(rng.integers(len(ids) + 1)), bad[int(rng.integers(len(bad)))])
    keep = {k: int(rng.random() < 0.2) for k in set(ids)}  # mbNotErase belongs to the key frame
    not_erase = [keep[k] for k in ids]
    return ids, not_erase

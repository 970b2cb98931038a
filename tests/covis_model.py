"""The observation graph (orb_slam2_map_amd/csrc/covis.hip, orbgpu_covis_*) restated twice, in plain Python -- test
infrastructure, like kfdb_model.py.

1. `CovisGraph`: the table as conventions V1-V7 (include/orbgpu.h) define it: rows in add order with
   slot lists of map point ids, a bad flag, a parent id and up to 10 covisible ids; the vote, the local map and the
   connection counter.  It is what the device is compared with, entry for entry.
2. `PointerMap`: the reference's pointer graph -- KeyFrame and MapPoint objects with `mObservations` dicts, `mvpMapPoints`
   lists, `mspChildrens` sets and `mnTrackReferenceForFrame` -- with Tracking::UpdateLocalKeyFrames / UpdateLocalPoints
   (Tracking.cc:1509-1643) and KeyFrame::UpdateConnections (KeyFrame.cc:327-417) statement by statement.  Containers the
   reference iterates by address are iterated by id (V4).  Its edits (AddObservation, EraseObservation, SetBadFlag of
   points and key frames, Replace, UpdateConnections) call the library's hooks on whatever `hooks` object it is given: the
   table model, a device graph, or both (tools/fuzz_covis.py).

The stated deviation of V2 -- a bad key frame's slots are cleared -- is a switch of the pointer graph
(`clear_bad_keyframe_slots`); with it off the pointer graph is the reference and lists the stale points of a bad parent.
KeyFrame::SetBadFlag's re-parenting is restated by its fall-back branch only (KeyFrame.cc:568-573: the children go to the
bad key frame's parent); the spanning-tree search above it chooses among the same hooks."""
import numpy as np

MAX_SLOTS = 65536
MAX_COVISIBLES = 10
MAX_LOCAL_KFS = 80  # Tracking.cc:1589
INT_MAX = 2 ** 31 - 1


class Refused(ValueError):
    """the call the device answers with EINVAL; nothing has changed"""


class _Row:
    def __init__(self, kf_id, slots):
        self.id = kf_id
        self.slots = slots
        self.bad = False
        self.parent = -1
        self.nb = []
        self.stamp = 0


class CovisGraph:
    def __init__(self):
        self.clear()

    def clear(self):
        self.rows = []     # add order
        self.row_of = {}   # id -> _Row
        self.covis = {}    # lists set for ids that are not rows yet
        self.parents = {}  # parents set for ids that are not rows yet
        self.stamp = 0

    def size(self):
        bad = sum(1 for r in self.rows if r.bad)
        return len(self.rows) - bad, bad

    # ---- edits ----------------------------------------------------------------------------------------------------------
    def add_keyframe(self, kf_id, n_slots, mp_ids=None):
        kf_id, n_slots = int(kf_id), int(n_slots)
        slots = [-1] * n_slots if mp_ids is None else [int(x) for x in mp_ids]
        if kf_id < 0 or kf_id in self.row_of or not 0 <= n_slots <= MAX_SLOTS or len(slots) != n_slots or any(x < -1 for x in slots):
            raise Refused("add_keyframe")
        row = _Row(kf_id, slots)
        row.nb = self.covis.pop(kf_id, [])
        row.parent = self.parents.pop(kf_id, -1)
        self.rows.append(row)
        self.row_of[kf_id] = row

    def set_slots(self, kf_ids, idx, mp_ids):
        entries = [(int(k), int(i), int(p)) for k, i, p in zip(kf_ids, idx, mp_ids)]
        for k, i, p in entries:  # every refusal before any change
            if p < -1 or (k in self.row_of and not 0 <= i < len(self.row_of[k].slots)):
                raise Refused("set_slots")
        known = 0
        for k, i, p in entries:
            row = self.row_of.get(k)
            if row is None:
                continue
            known += 1
            if not row.bad:
                row.slots[i] = p
        return known

    def set_bad(self, kf_ids):
        known = 0
        for k in kf_ids:
            row = self.row_of.get(int(k))
            if row is None:
                continue
            known += 1
            row.bad = True
            row.slots = [-1] * len(row.slots)
            row.nb = []
        return known

    def set_parent(self, kf_id, parent_id):
        kf_id, parent_id = int(kf_id), int(parent_id)
        if kf_id < 0 or parent_id < -1:
            raise Refused("set_parent")
        if kf_id in self.row_of:
            self.row_of[kf_id].parent = parent_id
        else:
            self.parents[kf_id] = parent_id

    def set_covisibles(self, kf_id, ids):
        kf_id, ids = int(kf_id), [int(x) for x in ids]
        if kf_id < 0 or len(ids) > MAX_COVISIBLES or any(x < 0 for x in ids):
            raise Refused("set_covisibles")
        row = self.row_of.get(kf_id)
        if row is None:
            self.covis[kf_id] = ids
        elif not row.bad:
            row.nb = ids

    # ---- V5 ---------------------------------------------------------------------------------------------------------------
    def vote(self, q, exclude=None):
        """count per row id, for the rows with a vote"""
        mult = {}
        for p in q:
            if p >= 0:
                mult[int(p)] = mult.get(int(p), 0) + 1
        out = {}
        for row in self.rows:
            if row.bad or row is exclude:
                continue
            c = sum(mult.get(p, 0) for p in row.slots if p >= 0)
            if c > 0:
                out[row.id] = min(c, INT_MAX)
        return out

    def children(self, kf_id):
        """V3"""
        return sorted(r.id for r in self.rows if r.parent == kf_id)

    # ---- V6 ---------------------------------------------------------------------------------------------------------------
    def local_map(self, kp_ids, prev_kf_ids=()):
        kp_ids = [int(x) for x in kp_ids]
        if len(kp_ids) > MAX_SLOTS:
            raise Refused("local_map")
        prev = [int(x) for x in prev_kf_ids]
        self.stamp += 1
        cur = self.stamp
        count = self.vote(kp_ids)
        k1 = sorted(count)
        res = dict(ref_kf=-1, max_votes=0, n_voted=len(k1), kept_previous=0,
                   n_unknown_previous=sum(1 for k in prev if k not in self.row_of))
        if not k1:
            res["kept_previous"] = 1
            kfs = [k for k in prev if k in self.row_of]
        else:
            for k in k1:
                if count[k] > res["max_votes"]:
                    res["max_votes"], res["ref_kf"] = count[k], k
                self.row_of[k].stamp = cur
            kfs = list(k1)
            for k in k1:
                if len(kfs) > MAX_LOCAL_KFS:
                    break
                row = self.row_of[k]
                for n in row.nb:
                    r2 = self.row_of.get(n)
                    if r2 is not None and not r2.bad and r2.stamp != cur:
                        kfs.append(n)
                        r2.stamp = cur
                        break
                for c in self.children(k):
                    r2 = self.row_of[c]
                    if not r2.bad and r2.stamp != cur:
                        kfs.append(c)
                        r2.stamp = cur
                        break
                r2 = self.row_of.get(row.parent)
                if r2 is not None and r2.stamp != cur:
                    kfs.append(row.parent)
                    r2.stamp = cur
                    break  # Tracking.cc:1632: the outer loop
        seen, pts = set(), []
        for k in kfs:
            for p in self.row_of[k].slots:
                if p >= 0 and p not in seen:
                    seen.add(p)
                    pts.append(p)
        res.update(kf_ids=np.array(kfs, np.int64), point_ids=np.array(pts, np.int64), n_kfs=len(kfs), n_points=len(pts))
        return res

    # ---- V7 ---------------------------------------------------------------------------------------------------------------
    def connections(self, kf_id, th=15):
        row = self.row_of.get(int(kf_id))
        ids, counts, ordered = [], [], []
        if row is not None and not row.bad:
            count = self.vote(row.slots, exclude=row)
            ids = sorted(count)
            counts = [count[k] for k in ids]
            nmax, kmax = 0, -1
            for k, c in zip(ids, counts):
                if c > nmax:
                    nmax, kmax = c, k
                if c >= th:
                    ordered.append((c, k))
            if not ordered and ids:
                ordered.append((nmax, kmax))
            ordered.sort(reverse=True)
        return dict(n=len(ids), n_ordered=len(ordered), ids=np.array(ids, np.int64), counts=np.array(counts, np.int32),
                    ordered_ids=np.array([k for _, k in ordered], np.int64), ordered_weights=np.array([c for c, _ in ordered], np.int32))


# ======================================================================================================================
# The pointer graph
# ======================================================================================================================
class MapPoint:
    def __init__(self, mp_id):
        self.mnId = mp_id
        self.mObservations = {}  # KeyFrame -> index; iterated by mnId (V4)
        self.nObs = 0
        self.mbBad = False
        self.mpReplaced = None
        self.mnTrackReferenceForFrame = -1

    def isBad(self):
        return self.mbBad

    def GetObservations(self):
        return sorted(self.mObservations.items(), key=lambda kv: kv[0].mnId)


class KeyFrame:
    def __init__(self, kf_id, n):
        self.mnId = kf_id
        self.N = n
        self.mvpMapPoints = [None] * n
        self.mbBad = False
        self.mpParent = None
        self.mspChildrens = set()
        self.mConnectedKeyFrameWeights = {}
        self.mvpOrderedConnectedKeyFrames = []
        self.mvOrderedWeights = []
        self.mbFirstConnection = True
        self.mnTrackReferenceForFrame = -1

    def isBad(self):
        return self.mbBad

    def GetBestCovisibilityKeyFrames(self, n):
        return self.mvpOrderedConnectedKeyFrames[:n]

    def GetChilds(self):
        return sorted(self.mspChildrens, key=lambda k: k.mnId)


class NoHooks:
    def __getattr__(self, name):
        return lambda *a, **k: None


class PointerMap:
    """the reference's objects; every edit calls the hook INTEGRATION.md section 2o places at that line"""

    def __init__(self, hooks=None, clear_bad_keyframe_slots=True):
        self.hooks = hooks if hooks is not None else NoHooks()
        self.clear_bad_keyframe_slots = clear_bad_keyframe_slots
        self.kfs = {}
        self.mps = {}
        self.frame_id = 0
        self.mvpLocalKeyFrames = []
        self.mvpLocalMapPoints = []
        self.mpReferenceKF = None

    # ---- edits ----------------------------------------------------------------------------------------------------------
    def AddKeyFrame(self, kf_id, n):
        kf = self.kfs[kf_id] = KeyFrame(kf_id, n)
        self.hooks.add_keyframe(kf_id, n, None)
        return kf

    def NewMapPoint(self, mp_id):
        mp = self.mps[mp_id] = MapPoint(mp_id)
        return mp

    def AddObservations(self, kf, pairs):
        """pKF->AddMapPoint(pMP, idx); pMP->AddObservation(pKF, idx) for every (idx, pMP), one batched hook call"""
        done = []
        for idx, mp in pairs:
            if kf in mp.mObservations or kf.mvpMapPoints[idx] is not None or mp.mbBad or kf.mbBad:
                continue  # (MapPoint::AddObservation's guard; the driver does not create what V2 does not represent)
            kf.mvpMapPoints[idx] = mp
            mp.mObservations[kf] = idx
            mp.nObs += 1
            done.append((idx, mp.mnId))
        if done:
            self.hooks.set_slots([kf.mnId] * len(done), [d[0] for d in done], [d[1] for d in done])

    def EraseObservation(self, kf, mp):
        """pKF->EraseMapPointMatch(pMP); pMP->EraseObservation(pKF)  (Optimizer.cc:754-755)"""
        idx = mp.mObservations.get(kf, -1)
        if idx >= 0:
            kf.mvpMapPoints[idx] = None
            self.hooks.set_slots([kf.mnId], [idx], [-1])
        self._erase_observation(mp, kf)

    def _erase_observation(self, mp, kf):
        """MapPoint::EraseObservation (MapPoint.cc:111-149)"""
        bad = False
        if kf in mp.mObservations:
            del mp.mObservations[kf]
            mp.nObs -= 1
            if mp.nObs <= 2:
                bad = True
        if bad:
            self.SetBadFlagMapPoint(mp)

    def SetBadFlagMapPoint(self, mp):
        """MapPoint::SetBadFlag (MapPoint.cc:151-168)"""
        obs = mp.GetObservations()
        mp.mObservations = {}
        mp.mbBad = True
        for kf, idx in obs:
            kf.mvpMapPoints[idx] = None  # pKF->EraseMapPointMatch(mit->second)
        if obs:
            self.hooks.set_slots([kf.mnId for kf, _ in obs], [idx for _, idx in obs], [-1] * len(obs))

    def Replace(self, mp, other):
        """MapPoint::Replace (MapPoint.cc:177-215)"""
        if other.mnId == mp.mnId:
            return
        obs = mp.GetObservations()
        mp.mObservations = {}
        mp.mbBad = True
        mp.mpReplaced = other
        out = []
        for kf, idx in obs:
            if kf not in other.mObservations:
                kf.mvpMapPoints[idx] = other  # ReplaceMapPointMatch
                other.mObservations[kf] = idx
                other.nObs += 1
                out.append((kf.mnId, idx, other.mnId))
            else:
                kf.mvpMapPoints[idx] = None  # EraseMapPointMatch
                out.append((kf.mnId, idx, -1))
        if out:
            self.hooks.set_slots([o[0] for o in out], [o[1] for o in out], [o[2] for o in out])

    def SetBadFlagKeyFrame(self, kf):
        """KeyFrame::SetBadFlag (KeyFrame.cc:491-583), re-parenting by the fall-back branch"""
        if kf.mnId == 0 or kf.mbBad:
            return
        for other in sorted(kf.mConnectedKeyFrameWeights, key=lambda k: k.mnId):
            self._erase_connection(other, kf)
        for mp in kf.mvpMapPoints:
            if mp is not None:
                self._erase_observation(mp, kf)
        kf.mConnectedKeyFrameWeights = {}
        kf.mvpOrderedConnectedKeyFrames = []
        kf.mvOrderedWeights = []
        for child in kf.GetChilds():
            child.mpParent = kf.mpParent  # ChangeParent
            if kf.mpParent is not None:
                kf.mpParent.mspChildrens.add(child)
            self.hooks.set_parent(child.mnId, kf.mpParent.mnId if kf.mpParent is not None else -1)
        kf.mspChildrens = set()
        if kf.mpParent is not None:
            kf.mpParent.mspChildrens.discard(kf)
        kf.mbBad = True
        if self.clear_bad_keyframe_slots:  # V2's deviation
            kf.mvpMapPoints = [None] * kf.N
        self.hooks.set_bad([kf.mnId])

    # ---- KeyFrame's connection lists ------------------------------------------------------------------------------------
    def _update_best_covisibles(self, kf):
        """KeyFrame::UpdateBestCovisibles (KeyFrame.cc:176-195)"""
        pairs = sorted(((w, k.mnId, k) for k, w in kf.mConnectedKeyFrameWeights.items()), key=lambda t: (t[0], t[1]))
        kf.mvpOrderedConnectedKeyFrames = [t[2] for t in reversed(pairs)]
        kf.mvOrderedWeights = [t[0] for t in reversed(pairs)]
        self.hooks.set_covisibles(kf.mnId, [k.mnId for k in kf.mvpOrderedConnectedKeyFrames[:MAX_COVISIBLES]])

    def _add_connection(self, kf, other, weight):
        """KeyFrame::AddConnection (KeyFrame.cc:161-174)"""
        if kf.mConnectedKeyFrameWeights.get(other) == weight:
            return
        kf.mConnectedKeyFrameWeights[other] = weight
        self._update_best_covisibles(kf)

    def _erase_connection(self, kf, other):
        """KeyFrame::EraseConnection (KeyFrame.cc:591-605)"""
        if other in kf.mConnectedKeyFrameWeights:
            del kf.mConnectedKeyFrameWeights[other]
            self._update_best_covisibles(kf)

    def UpdateConnections(self, kf, th=15):
        """KeyFrame::UpdateConnections (KeyFrame.cc:327-417).  Returns (counter as [(id, n)], ordered ids, ordered weights)."""
        KFcounter = {}
        vpMP = list(kf.mvpMapPoints)
        for pMP in vpMP:
            if pMP is None:
                continue
            if pMP.isBad():
                continue
            for okf, _ in pMP.GetObservations():
                if okf.mnId == kf.mnId:
                    continue
                KFcounter[okf] = KFcounter.get(okf, 0) + 1
        if not KFcounter:
            return [], [], []
        nmax, pKFmax = 0, None
        vPairs = []
        for okf in sorted(KFcounter, key=lambda k: k.mnId):
            n = KFcounter[okf]
            if n > nmax:
                nmax, pKFmax = n, okf
            if n >= th:
                vPairs.append((n, okf.mnId, okf))
                self._add_connection(okf, kf, n)
        if not vPairs:
            vPairs.append((nmax, pKFmax.mnId, pKFmax))
            self._add_connection(pKFmax, kf, nmax)
        vPairs.sort(key=lambda t: (t[0], t[1]))
        lKFs, lWs = [], []
        for n, _, okf in vPairs:
            lKFs.insert(0, okf)
            lWs.insert(0, n)
        kf.mConnectedKeyFrameWeights = dict(KFcounter)
        kf.mvpOrderedConnectedKeyFrames = lKFs
        kf.mvOrderedWeights = lWs
        self.hooks.set_covisibles(kf.mnId, [k.mnId for k in lKFs[:MAX_COVISIBLES]])
        if kf.mbFirstConnection and kf.mnId != 0:
            kf.mpParent = lKFs[0]
            kf.mpParent.mspChildrens.add(kf)
            kf.mbFirstConnection = False
            self.hooks.set_parent(kf.mnId, kf.mpParent.mnId)
        return ([(k.mnId, KFcounter[k]) for k in sorted(KFcounter, key=lambda k: k.mnId)], [k.mnId for k in lKFs], list(lWs))

    # ---- Tracking -------------------------------------------------------------------------------------------------------
    def frame_kp_ids(self, frame_points):
        """what the caller hands the library: the frame's map points per key point, bad ones cleared (Tracking.cc:1552)"""
        return [-1 if mp is None or mp.isBad() else mp.mnId for mp in frame_points]

    def UpdateLocalMap(self, frame_points):
        """Tracking::UpdateLocalKeyFrames + UpdateLocalPoints for a frame whose mvpMapPoints is `frame_points` (changed in
        place as the reference does).  Returns dict(kf_ids, point_ids, ref_kf, max_votes, n_voted, kept_previous)."""
        self.frame_id += 1
        fid = self.frame_id
        out = self._update_local_keyframes(frame_points, fid)
        # UpdateLocalPoints
        self.mvpLocalMapPoints = []
        for pKF in self.mvpLocalKeyFrames:
            for pMP in pKF.mvpMapPoints:
                if pMP is None:
                    continue
                if pMP.mnTrackReferenceForFrame == fid:
                    continue
                if not pMP.isBad():
                    self.mvpLocalMapPoints.append(pMP)
                    pMP.mnTrackReferenceForFrame = fid
        out.update(kf_ids=[k.mnId for k in self.mvpLocalKeyFrames], point_ids=[p.mnId for p in self.mvpLocalMapPoints])
        return out

    def _update_local_keyframes(self, frame_points, fid):
        keyframeCounter = {}
        for i in range(len(frame_points)):
            if frame_points[i] is not None:
                pMP = frame_points[i]
                if not pMP.isBad():
                    for kf, _ in pMP.GetObservations():
                        keyframeCounter[kf] = keyframeCounter.get(kf, 0) + 1
                else:
                    frame_points[i] = None
        out = dict(ref_kf=-1, max_votes=0, n_voted=0, kept_previous=0)
        if not keyframeCounter:
            out["kept_previous"] = 1
            return out
        mx, pKFmax = 0, None
        self.mvpLocalKeyFrames = []
        for pKF in sorted(keyframeCounter, key=lambda k: k.mnId):
            if pKF.isBad():
                continue
            if keyframeCounter[pKF] > mx:
                mx, pKFmax = keyframeCounter[pKF], pKF
            self.mvpLocalKeyFrames.append(pKF)
            pKF.mnTrackReferenceForFrame = fid
        out["n_voted"] = len(self.mvpLocalKeyFrames)
        for pKF in list(self.mvpLocalKeyFrames):  # itEndKF is taken before the loop
            if len(self.mvpLocalKeyFrames) > MAX_LOCAL_KFS:
                break
            for pNeighKF in pKF.GetBestCovisibilityKeyFrames(10):
                if not pNeighKF.isBad():
                    if pNeighKF.mnTrackReferenceForFrame != fid:
                        self.mvpLocalKeyFrames.append(pNeighKF)
                        pNeighKF.mnTrackReferenceForFrame = fid
                        break
            for pChildKF in pKF.GetChilds():
                if not pChildKF.isBad():
                    if pChildKF.mnTrackReferenceForFrame != fid:
                        self.mvpLocalKeyFrames.append(pChildKF)
                        pChildKF.mnTrackReferenceForFrame = fid
                        break
            pParent = pKF.mpParent
            if pParent is not None:
                if pParent.mnTrackReferenceForFrame != fid:
                    self.mvpLocalKeyFrames.append(pParent)
                    pParent.mnTrackReferenceForFrame = fid
                    break
        if pKFmax is not None:
            self.mpReferenceKF = pKFmax
            out["ref_kf"], out["max_votes"] = pKFmax.mnId, mx
        return out


class Tee:
    """hooks that go to several graphs (the table model and a device graph)"""

    def __init__(self, *targets):
        self.targets = targets

    def __getattr__(self, name):
        def call(*a, **k):
            for t in self.targets:
                getattr(t, name)(*a, **k)
        return call


# ---- scenes (shared by the tests, tools/fuzz_covis.py and tools/bench_covis.py) ---------------------------------------
SLOT_SIZES = (0, 1, 63, 64, 65, 130)


def random_edit(rng, pm, next_ids):
    """one random consistent edit of the pointer map; next_ids = [next key frame id, next map point id]"""
    u = rng.random()
    kfs = [k for k in pm.kfs.values() if not k.mbBad]
    mps = [m for m in pm.mps.values() if not m.mbBad]
    if u < 0.18 or len(kfs) < 3:
        n = int(rng.choice(SLOT_SIZES)) if rng.random() < 0.5 else int(rng.integers(0, 140))
        kf = pm.AddKeyFrame(next_ids[0], n)
        next_ids[0] += int(rng.integers(1, 4))
        pairs = []
        for idx in rng.permutation(n)[:int(rng.integers(0, n + 1))]:
            if mps and rng.random() < 0.7:
                mp = mps[int(rng.integers(len(mps)))]
            else:
                mp = pm.NewMapPoint(next_ids[1])
                next_ids[1] += 1
                mps.append(mp)
            pairs.append((int(idx), mp))
        pm.AddObservations(kf, pairs)
        pm.UpdateConnections(kf, th=int(rng.choice([1, 2, 15])))  # LocalMapping::ProcessNewKeyFrame: the parent is older
        kf.mbFirstConnection = False  # (a key frame that found no parent now stays a root: no cycles in the spanning tree)
        return "add_keyframe"
    if u < 0.45 and mps:
        kf = kfs[int(rng.integers(len(kfs)))]
        if kf.N:
            pm.AddObservations(kf, [(int(rng.integers(kf.N)), mps[int(rng.integers(len(mps)))]) for _ in range(int(rng.integers(1, 6)))])
        return "add_observation"
    if u < 0.55 and mps:
        mp = mps[int(rng.integers(len(mps)))]
        if mp.mObservations:
            kf = mp.GetObservations()[int(rng.integers(len(mp.mObservations)))][0]
            pm.EraseObservation(kf, mp)
        return "erase_observation"
    if u < 0.62 and mps:
        pm.SetBadFlagMapPoint(mps[int(rng.integers(len(mps)))])
        return "point_bad"
    if u < 0.70 and len(mps) >= 2:
        a, b = rng.choice(len(mps), size=2, replace=False)
        pm.Replace(mps[int(a)], mps[int(b)])
        return "replace"
    if u < 0.76:
        pm.SetBadFlagKeyFrame(kfs[int(rng.integers(len(kfs)))])
        return "keyframe_bad"
    pm.UpdateConnections(kfs[int(rng.integers(len(kfs)))], th=int(rng.choice([1, 2, 5, 15])))
    return "update_connections"


def random_frame(rng, pm, n=None):
    """a frame's mvpMapPoints: points of a few key frames (so that the vote finds rows), some bad ones, some twice"""
    mps = list(pm.mps.values())
    n = int(rng.integers(0, 80)) if n is None else n
    kfs = [k for k in pm.kfs.values() if not k.mbBad and k.N]
    near = []
    for kf in (kfs[i] for i in rng.permutation(len(kfs))[:3]):
        near += [m for m in kf.mvpMapPoints if m is not None]
    out = []
    for _ in range(n):
        u = rng.random()
        if u < 0.2 or not mps:
            out.append(None)
        elif u < 0.8 and near:
            out.append(near[int(rng.integers(len(near)))])
        else:
            out.append(mps[int(rng.integers(len(mps)))])
    return out

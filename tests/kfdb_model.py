"""KeyFrameDatabase restated statement by statement (reference src/KeyFrameDatabase.cc:33-309) together with
L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68): the definition the device database
(orb_slam2_map_amd/csrc/kfdb.hip) is compared with.  Plain Python and numpy -- test infrastructure, like sim3_model.py
and pose_model.py.  The DBoW2 boundary is not pinned by a reference binary.

The inverted file is the literal one: a Python list per word, `append` on add, remove-first-match on erase.  A key
frame carries the fields the reference writes into the KeyFrame object: query stamp, word count, loop score, reloc
score.  Conventions K1-K9: DESIGN.md section 2.

Two things the reference leaves to its callers are fixed here (and on the device):
  * a key frame that is erased and added again is a NEW entry: new add sequence number, reloc score register 0.0f
    (the reference never re-adds: erase is called from KeyFrame::SetBadFlag only);
  * every query has a stamp of its own (the reference stamps with KeyFrame::mnId / Frame::mnId, which are unique)."""
import math

import numpy as np

MAX_NEIGHBOURS = 10  # GetBestCovisibilityKeyFrames(10), KeyFrameDatabase.cc:151 / :265
F32 = np.float32


def l1_score(ids1, vals1, ids2, vals2):
    """L1Scoring::score(v1, v2) as a double: the two-iterator walk with lower_bound jumps (ScoringObject.cpp:23-68)"""
    i, j, n1, n2 = 0, 0, len(ids1), len(ids2)
    score = 0.0
    while i < n1 and j < n2:
        vi, wi = float(vals1[i]), float(vals2[j])
        if ids1[i] == ids2[j]:
            score += math.fabs(vi - wi) - math.fabs(vi) - math.fabs(wi)
            i += 1
            j += 1
        elif ids1[i] < ids2[j]:
            i = int(np.searchsorted(ids1, ids2[j], side="left"))  # v1.lower_bound(v2_it->first)
        else:
            j = int(np.searchsorted(ids2, ids1[i], side="left"))
    score = -score / 2.0
    return score


def min_common_words(max_common_words):
    """int minCommonWords = maxCommonWords*0.8f;  (K3: float product, truncation)"""
    return int(F32(max_common_words) * F32(0.8))


def valid_vector(n_words, ids, vals):
    """K8: word ids strictly ascending inside [0, n_words), values finite"""
    ids = np.asarray(ids, np.int64)
    vals = np.asarray(vals, np.float64)
    if len(ids) != len(vals):
        return False
    if len(ids) == 0:
        return True
    return bool(ids[0] >= 0 and ids[-1] < n_words and np.all(np.diff(ids) > 0) and np.all(np.isfinite(vals)))


class _KF:
    def __init__(self, kf_id, ids, vals, seq):
        self.id = int(kf_id)
        self.ids = np.array(ids, np.int64)
        self.vals = np.array(vals, np.float64)
        self.seq = seq
        self.loop_query = self.reloc_query = -1  # mnLoopQuery / mnRelocQuery
        self.loop_words = self.reloc_words = 0   # mnLoopWords / mnRelocWords
        self.loop_score = F32(0)                 # mLoopScore
        self.reloc_score = F32(0)                # mRelocScore: K5's register, 0.0f before its first write


class Refused(ValueError):
    """the call the device answers with EINVAL; nothing has changed"""


class KeyFrameDatabase:
    def __init__(self, n_words):
        self.n_words = int(n_words)
        self.clear()

    def clear(self):
        """KeyFrameDatabase::clear (:69-73); the key frames, their neighbour lists and the sequence restart as well"""
        self.inverted = {}   # word -> list of _KF in add order (mvInvertedFile, sparse)
        self.kfs = {}        # id -> _KF of the key frames in the database
        self.covis = {}      # id -> neighbour ids (K7), kept for ids that are not in the database yet; erase drops it
        self.seq = 0
        self.stamp = 0
        self.last = []

    def size(self):
        return len(self.kfs)

    def set_covisibles(self, kf_id, neighbours):
        neighbours = [int(x) for x in neighbours]
        if kf_id < 0 or len(neighbours) > MAX_NEIGHBOURS or any(x < 0 for x in neighbours):
            raise Refused("neighbours")
        self.covis[int(kf_id)] = neighbours

    def add(self, kf_id, ids, vals):
        """KeyFrameDatabase::add (:40-46)"""
        if kf_id < 0 or kf_id in self.kfs or not valid_vector(self.n_words, ids, vals):
            raise Refused("add")
        kf = _KF(kf_id, ids, vals, self.seq)
        self.seq += 1
        self.kfs[kf.id] = kf
        for w in kf.ids:
            self.inverted.setdefault(int(w), []).append(kf)

    def erase(self, kf_ids):
        """KeyFrameDatabase::erase (:48-67) per id; unknown ids are ignored.  Returns how many were known."""
        known = 0
        for kf_id in kf_ids:
            kf = self.kfs.pop(int(kf_id), None)
            if kf is None:
                continue
            known += 1
            self.covis.pop(kf.id, None)  # K7: the list goes with the key frame
            for w in kf.ids:
                lst = self.inverted[int(w)]
                for k, other in enumerate(lst):
                    if other is kf:
                        del lst[k]
                        break
        return known

    def score(self, q_ids, q_vals, kf_ids):
        """LoopClosing.cc:128-139: mpORBVocabulary->score(CurrentBowVec, BowVec) as the float the caller keeps"""
        if not valid_vector(self.n_words, q_ids, q_vals):
            raise Refused("query")
        out = np.full(len(kf_ids), np.nan, np.float32)
        for k, kf_id in enumerate(kf_ids):
            kf = self.kfs.get(int(kf_id))
            if kf is not None:
                out[k] = F32(l1_score(q_ids, q_vals, kf.ids, kf.vals))
        return out

    # ---- K1, second formulation --------------------------------------------------------------------------------------
    def sharing_by_sort(self, q_ids, connected=()):
        """lKFsSharingWords without the inverted file: rows ordered by (first common word, add sequence number)"""
        q = set(int(w) for w in q_ids)
        conn = set(int(c) for c in connected)
        rows = []
        for kf in self.kfs.values():
            if kf.id in conn:
                continue
            common = [int(w) for w in kf.ids if int(w) in q]
            if common:
                rows.append((min(common), kf.seq, kf.id, len(common)))
        rows.sort()
        return [(r[2], r[3], r[0]) for r in rows]  # (id, words, first common word)

    def _neighbours(self, kf):
        """GetBestCovisibilityKeyFrames(10) resolved when the query runs (K7): ids that are not in the database drop out"""
        return [self.kfs[n] for n in self.covis.get(kf.id, ()) if n in self.kfs]

    # ---- KeyFrameDatabase::DetectLoopCandidates (:76-197) ------------------------------------------------------------
    def detect_loop(self, q_ids, q_vals, connected, min_score):
        if not valid_vector(self.n_words, q_ids, q_vals) or not math.isfinite(float(min_score)):
            raise Refused("query")
        min_score = F32(min_score)
        self.stamp += 1
        query = self.stamp  # pKF->mnId
        connected = set(int(c) for c in connected)  # spConnectedKeyFrames
        sharing, first = [], {}
        for w in q_ids:
            for kfi in self.inverted.get(int(w), ()):
                if kfi.loop_query != query:
                    kfi.loop_words = 0
                    if kfi.id not in connected:
                        kfi.loop_query = query
                        sharing.append(kfi)
                        first[kfi.id] = int(w)
                kfi.loop_words += 1
        rec = {kf.id: dict(id=kf.id, words=kf.loop_words, first_word=first[kf.id], score=F32(np.nan), acc=F32(np.nan), best_id=-1)
               for kf in sharing}
        self.last = [rec[kf.id] for kf in sharing]
        if not sharing:
            return []
        max_common = 0
        for kf in sharing:
            if kf.loop_words > max_common:
                max_common = kf.loop_words
        min_common = min_common_words(max_common)
        score_and_match = []
        for kfi in sharing:
            if kfi.loop_words > min_common:
                si = F32(l1_score(q_ids, q_vals, kfi.ids, kfi.vals))
                kfi.loop_score = si
                rec[kfi.id]["score"] = si
                if si >= min_score:
                    score_and_match.append((si, kfi))
        if not score_and_match:
            return []
        acc_and_match = []
        best_acc = min_score
        for si, kfi in score_and_match:
            best_score, acc, best_kf = si, si, kfi
            for kf2 in self._neighbours(kfi):
                if kf2.loop_query == query and kf2.loop_words > min_common:
                    acc = F32(acc + kf2.loop_score)
                    if kf2.loop_score > best_score:
                        best_kf = kf2
                        best_score = kf2.loop_score
            acc_and_match.append((acc, best_kf))
            rec[kfi.id]["acc"], rec[kfi.id]["best_id"] = acc, best_kf.id
            if acc > best_acc:
                best_acc = acc
        return self._retain(acc_and_match, best_acc)

    # ---- KeyFrameDatabase::DetectRelocalizationCandidates (:199-309) -------------------------------------------------
    def detect_reloc(self, q_ids, q_vals):
        if not valid_vector(self.n_words, q_ids, q_vals):
            raise Refused("query")
        self.stamp += 1
        query = self.stamp  # F->mnId
        sharing, first = [], {}
        for w in q_ids:
            for kfi in self.inverted.get(int(w), ()):
                if kfi.reloc_query != query:
                    kfi.reloc_words = 0
                    kfi.reloc_query = query
                    sharing.append(kfi)
                    first[kfi.id] = int(w)
                kfi.reloc_words += 1
        rec = {kf.id: dict(id=kf.id, words=kf.reloc_words, first_word=first[kf.id], score=F32(np.nan), acc=F32(np.nan), best_id=-1)
               for kf in sharing}
        self.last = [rec[kf.id] for kf in sharing]
        if not sharing:
            return []
        max_common = 0
        for kf in sharing:
            if kf.reloc_words > max_common:
                max_common = kf.reloc_words
        min_common = min_common_words(max_common)
        score_and_match = []
        for kfi in sharing:
            if kfi.reloc_words > min_common:
                si = F32(l1_score(q_ids, q_vals, kfi.ids, kfi.vals))
                kfi.reloc_score = si
                rec[kfi.id]["score"] = si
                score_and_match.append((si, kfi))
        if not score_and_match:
            return []
        acc_and_match = []
        best_acc = F32(0)
        for si, kfi in score_and_match:
            best_score, acc, best_kf = si, si, kfi
            for kf2 in self._neighbours(kfi):
                if kf2.reloc_query != query:
                    continue
                acc = F32(acc + kf2.reloc_score)  # a row this query did not score: the score an EARLIER query left (K5)
                if kf2.reloc_score > best_score:
                    best_kf = kf2
                    best_score = kf2.reloc_score
            acc_and_match.append((acc, best_kf))
            rec[kfi.id]["acc"], rec[kfi.id]["best_id"] = acc, best_kf.id
            if acc > best_acc:
                best_acc = acc
        return self._retain(acc_and_match, best_acc)

    @staticmethod
    def _retain(acc_and_match, best_acc):
        min_to_retain = F32(F32(0.75) * best_acc)
        already, out = set(), []
        for acc, kf in acc_and_match:
            if acc > min_to_retain:
                if kf.id not in already:
                    out.append(kf.id)
                    already.add(kf.id)
        return out

    def last_query(self):
        """the sharing list of the most recent detect call in K1 order, as dicts of numpy-comparable columns"""
        cols = dict(id=np.array([r["id"] for r in self.last], np.int64), words=np.array([r["words"] for r in self.last], np.int32),
                    first_word=np.array([r["first_word"] for r in self.last], np.int32),
                    score=np.array([r["score"] for r in self.last], np.float32), acc=np.array([r["acc"] for r in self.last], np.float32),
                    best_id=np.array([r["best_id"] for r in self.last], np.int64))
        return cols


# ---- scenes (shared by the tests, tools/fuzz_kfdb.py and tools/bench_kfdb.py) -----------------------------------------
def random_vector(rng, n_words, n, normalise=True):
    """a BoW vector of n distinct words: ascending ids, positive weights, L1-normalised like DBoW2's transform"""
    n = min(int(n), int(n_words))
    ids = np.sort(rng.choice(n_words, size=n, replace=False)).astype(np.int32)
    vals = rng.uniform(0.05, 1.0, size=n)
    if normalise and n:
        vals = vals / vals.sum()
    return ids, vals.astype(np.float64)


def vector_from(rng, base_ids, base_vals, keep, n_words, extra):
    """a vector sharing `keep` of the base's words (same values, jittered) plus `extra` words outside it"""
    keep = min(int(keep), len(base_ids))
    sel = np.sort(rng.choice(len(base_ids), size=keep, replace=False)) if keep else np.zeros(0, np.int64)
    ids = [int(base_ids[k]) for k in sel]
    vals = [float(base_vals[k]) * float(rng.uniform(0.5, 1.5)) for k in sel]
    taken = set(int(w) for w in base_ids)
    while len(ids) < keep + extra and len(taken) < n_words:
        w = int(rng.integers(0, n_words))
        if w not in taken:
            taken.add(w)
            ids.append(w)
            vals.append(float(rng.uniform(0.05, 1.0)))
    order = np.argsort(ids)
    ids = np.array(ids, np.int32)[order]
    vals = np.array(vals, np.float64)[order]
    if len(vals):
        vals = vals / np.abs(vals).sum()
    return ids, vals

"""Randomised comparison of the device observation graph (orbgpu_covis_*) with the CPU model (tests/covis_model.py).

usage: python tools/fuzz_covis.py SECONDS SEED

Each round creates a graph (initial rows and slots drawn, sometimes with the vote's query forced through global memory)
and drives the model's pointer map through random consistent edits -- add key frame, add / erase observation, point and
key frame set bad with re-parenting, replace, UpdateConnections -- whose hooks go to the device and to the table model
alike; refused calls are mixed in and must be refused by both.  Every output of orbgpu_covis_local_map and
orbgpu_covis_connections must equal the model's.  Exit status 1 on any mismatch."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import covis_model as M  # noqa: E402
from orb_slam2_map_amd import lib as G  # noqa: E402

LOCAL_MAP_FIELDS = ("ref_kf", "n_kfs", "n_points", "max_votes", "n_voted", "kept_previous", "n_unknown_previous")


class Pair:
    """one device graph and one table model fed the same calls; every call returns '' or a description of the difference"""

    def __init__(self, initial_rows=0, initial_slots=0):
        self.dev = G.CovisibilityGraph(initial_rows=initial_rows, initial_slots=initial_slots)
        self.model = M.CovisGraph()

    def close(self):
        self.dev.close()

    def _both(self, name, dev_call, model_call):
        try:
            want, refused_m = model_call(), False
        except M.Refused:
            want, refused_m = None, True
        try:
            got, refused_g = dev_call(), False
        except G.OrbGpuError as e:
            if e.status != G.EINVAL:
                raise
            got, refused_g = None, True
        if refused_m != refused_g:
            return "%s: refused by %s only" % (name, "the model" if refused_m else "the device"), None, None
        return "", got, want

    def _edit(self, name, *args):
        err, got, want = self._both(name, lambda: getattr(self.dev, name)(*args), lambda: getattr(self.model, name)(*args))
        if not err and got != want:
            err = "%s: %s, model %s" % (name, got, want)
        return err

    # the hooks (tests/covis_model.py PointerMap calls them; a mismatch raises, so that the pointer map stops there)
    def add_keyframe(self, kf_id, n_slots, mp_ids=None):
        return self._raise(self._edit("add_keyframe", kf_id, n_slots, mp_ids))

    def set_slots(self, kf_ids, idx, mp_ids):
        return self._raise(self._edit("set_slots", kf_ids, idx, mp_ids))

    def set_bad(self, kf_ids):
        return self._raise(self._edit("set_bad", kf_ids))

    def set_parent(self, kf_id, parent_id):
        return self._raise(self._edit("set_parent", kf_id, parent_id))

    def set_covisibles(self, kf_id, ids):
        return self._raise(self._edit("set_covisibles", kf_id, ids))

    @staticmethod
    def _raise(err):
        if err:
            raise AssertionError(err)
        return ""

    def clear(self):
        self.dev.clear()
        self.model.clear()
        return self.size()

    def size(self):
        return "" if self.dev.size() == self.model.size() else "size %s, model %s" % (self.dev.size(), self.model.size())

    def local_map(self, kp_ids, prev=(), kf_capacity=None, point_capacity=None):
        err, got, want = self._both("local_map", lambda: self.dev.local_map(kp_ids, prev, kf_capacity, point_capacity),
                                    lambda: self.model.local_map(kp_ids, prev))
        if err or want is None:
            return err
        for k in LOCAL_MAP_FIELDS:
            if got[k] != want[k]:
                return "local_map %s: %s, model %s" % (k, got[k], want[k])
        for k, cap in (("kf_ids", kf_capacity), ("point_ids", point_capacity)):
            w = want[k] if cap is None else want[k][:cap]
            if not np.array_equal(got[k], w):
                return "local_map %s: %s, model %s" % (k, got[k][:12], w[:12])
        return ""

    def connections(self, kf_id, th=15, capacity=None, ordered_capacity=None):
        err, got, want = self._both("connections", lambda: self.dev.connections(kf_id, th, capacity, ordered_capacity),
                                    lambda: self.model.connections(kf_id, th))
        if err or want is None:
            return err
        if got["n"] != want["n"] or got["n_ordered"] != want["n_ordered"]:
            return "connections: %d / %d entries, model %d / %d" % (got["n"], got["n_ordered"], want["n"], want["n_ordered"])
        for k, cap in (("ids", capacity), ("counts", capacity), ("ordered_ids", ordered_capacity), ("ordered_weights", ordered_capacity)):
            w = want[k] if cap is None else want[k][:cap]
            if not np.array_equal(got[k], w):
                return "connections %s: %s, model %s" % (k, got[k][:12], w[:12])
        return ""


def refused_call(rng, pair, pm):
    """a call both sides must refuse (or, for an unknown key frame, ignore) -- and that changes nothing"""
    kfs = list(pm.kfs.values())
    kf = kfs[int(rng.integers(len(kfs)))]
    kind = int(rng.integers(7))
    if kind == 0:
        return pair._edit("add_keyframe", kf.mnId, 3, None)
    if kind == 1:
        return pair._edit("add_keyframe", -5, 3, None)
    if kind == 2:
        return pair._edit("add_keyframe", 10 ** 9, M.MAX_SLOTS + 1, None)
    if kind == 3:
        return pair._edit("set_slots", [kf.mnId, kf.mnId], [0, kf.N], [7, 7])
    if kind == 4:
        return pair._edit("set_covisibles", kf.mnId, list(range(11)))
    if kind == 5:
        return pair._edit("set_slots", [10 ** 9 + 1], [5], [7])  # unknown: ignored by both, 0 known
    return pair._edit("set_slots", [kf.mnId] * min(kf.N, 1), [0] * min(kf.N, 1), [-2] * min(kf.N, 1)) if kf.N else ""


def one_round(rng, counts):
    lds = rng.random() < 0.3
    if lds:
        os.environ["ORBGPU_DEBUG_COVIS_LDS_IDS"] = str(int(rng.choice([0, 1, 5])))
    else:
        os.environ.pop("ORBGPU_DEBUG_COVIS_LDS_IDS", None)
    pair = Pair(initial_rows=int(rng.choice([0, 2, 2, 16])), initial_slots=int(rng.choice([0, 8, 64])))
    pm = M.PointerMap(pair)
    next_ids = [int(rng.integers(0, 3)), int(rng.choice([0, 2 ** 33]))]
    errs = []
    try:
        for step in range(int(rng.integers(20, 160))):
            u = rng.random()
            try:
                if u < 0.60 or len(pm.kfs) < 3:
                    op, err = M.random_edit(rng, pm, next_ids), ""
                elif u < 0.66:
                    op, err = "refused", refused_call(rng, pair, pm)
                elif u < 0.67:
                    op, err = "clear", pair.clear()
                    pm = M.PointerMap(pair)
                elif u < 0.85:
                    frame = M.random_frame(rng, pm)
                    prev = [k.mnId for k in pm.mvpLocalKeyFrames] + ([10 ** 9] if rng.random() < 0.2 else [])
                    caps = (None, None) if rng.random() < 0.7 else (int(rng.integers(0, 5)), int(rng.integers(0, 30)))
                    op, err = "local_map", pair.local_map(pm.frame_kp_ids(frame), prev, *caps)
                    pm.UpdateLocalMap(frame)  # (the previous list of the next query)
                else:
                    ids = list(pm.kfs) + [10 ** 9]
                    caps = (None, None) if rng.random() < 0.7 else (int(rng.integers(0, 4)), int(rng.integers(0, 3)))
                    op, err = "connections", pair.connections(ids[int(rng.integers(len(ids)))], int(rng.choice([1, 3, 15])), *caps)
            except AssertionError as e:
                op, err = "hook", str(e)
            counts[op] = counts.get(op, 0) + 1
            if err:
                errs.append("step %d (%s): %s" % (step, op, err))
                break
    finally:
        pair.close()
        os.environ.pop("ORBGPU_DEBUG_COVIS_LDS_IDS", None)
    return errs


def run(seconds, seed):
    rng = np.random.default_rng(seed)
    counts, errs, rounds = {}, [], 0
    t_end = time.time() + seconds
    while True:
        errs += one_round(rng, counts)
        rounds += 1
        if errs or time.time() >= t_end:
            return rounds, counts, errs


def main():
    seconds, seed = float(sys.argv[1]), int(sys.argv[2])
    t0 = time.time()
    rounds, counts, errs = run(seconds, seed)
    for e in errs[:20]:
        print("MISMATCH " + e)
    q = counts.get("local_map", 0) + counts.get("connections", 0)
    print("%s %d rounds, %d queries, %d refused calls, %d edits in %.1f s (seed %d; vs tests/covis_model.py, exact equality)" % (
        "fuzz FAILED" if errs else "fuzz ok", rounds, q, counts.get("refused", 0),
        sum(v for k, v in counts.items() if k not in ("local_map", "connections", "refused")), time.time() - t0, seed))
    sys.exit(1 if errs else 0)


if __name__ == "__main__":
    main()

"""Randomised comparison of the device KeyFrameDatabase (orbgpu_keyframe_db_*) with the CPU model (tests/kfdb_model.py)
-- vs CPU restatement; DBoW2 boundary unpinned.

usage: python tools/fuzz_kfdb.py SECONDS SEED

Each round creates a database (vocabulary size, initial rows drawn) and applies a random sequence of add / erase /
set_covisibles / clear / score / detect_loop / detect_reloc calls, refused ones included, to the device and to the model.
Candidate lists must be equal and in order, the records of the sharing list equal with scores and sums BIT-equal, and a
refused call must be refused by both.  Exit status 1 on any mismatch."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kfdb_model as M  # noqa: E402
from orb_slam2_map_amd import lib as G  # noqa: E402

FLOAT_COLS = ("score", "acc")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan_a, nan_b = np.isnan(a), np.isnan(b)  # a NaN is "not scored": its payload is not part of the contract
    return a.shape == b.shape and np.array_equal(nan_a, nan_b) and np.array_equal(a[~nan_a].view(np.uint32), b[~nan_b].view(np.uint32))


def last_query_diff(dev, model):
    """'' if the device's sharing list equals the model's (K1 order; scores and sums bit for bit), else what differs"""
    g, m = dev.last_query(), model.last_query()
    for k in ("id", "words", "first_word", "best_id"):
        if not np.array_equal(g[k], m[k]):
            return "last_query %s: %s, model %s" % (k, g[k][:12], m[k][:12])
    for k in FLOAT_COLS:
        if not same_bits(g[k], m[k]):
            w = [i for i in range(len(m[k])) if not same_bits(g[k][i:i + 1], m[k][i:i + 1])]
            return "last_query %s differs at %s: %r, model %r" % (k, w[:5], g[k][w[0]], m[k][w[0]])
    return ""


class Pair:
    """one device database and one model fed the same calls; every call returns '' or a description of the difference"""

    def __init__(self, n_words, initial_rows=0):
        self.dev = G.KeyFrameDatabase(n_words, initial_rows=initial_rows)
        self.model = M.KeyFrameDatabase(n_words)

    def close(self):
        self.dev.close()

    def _both(self, name, dev_call, model_call):
        """runs the call on both sides; ('refused', None, None) if both refuse, else ('', got, want) or a mismatch"""
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

    def add(self, kf_id, ids, vals):
        return self._both("add", lambda: self.dev.add(kf_id, ids, vals), lambda: self.model.add(kf_id, ids, vals))[0]

    def set_covisibles(self, kf_id, nb):
        return self._both("set_covisibles", lambda: self.dev.set_covisibles(kf_id, nb), lambda: self.model.set_covisibles(kf_id, nb))[0]

    def erase(self, kf_ids):
        err, got, want = self._both("erase", lambda: self.dev.erase(kf_ids), lambda: self.model.erase(kf_ids))
        if not err and got != want:
            err = "erase: %s known, model %s" % (got, want)
        return err or self.size()

    def clear(self):
        self.dev.clear()
        self.model.clear()
        return self.size()

    def size(self):
        return "" if self.dev.size() == self.model.size() else "size %d, model %d" % (self.dev.size(), self.model.size())

    def score(self, ids, vals, kf_ids):
        err, got, want = self._both("score", lambda: self.dev.score(ids, vals, kf_ids), lambda: self.model.score(ids, vals, kf_ids))
        if not err and want is not None and not same_bits(got, want):
            err = "score: %s, model %s" % (got[:8], want[:8])
        return err

    def loop(self, ids, vals, connected, min_score):
        err, got, want = self._both("detect_loop", lambda: self.dev.DetectLoopCandidates(ids, vals, connected, min_score),
                                    lambda: self.model.detect_loop(ids, vals, connected, min_score))
        if not err and want is not None and list(got) != list(want):
            err = "detect_loop: %s, model %s" % (list(got)[:12], list(want)[:12])
        return err or (last_query_diff(self.dev, self.model) if want is not None else "")

    def reloc(self, ids, vals):
        err, got, want = self._both("detect_reloc", lambda: self.dev.DetectRelocalizationCandidates(ids, vals),
                                    lambda: self.model.detect_reloc(ids, vals))
        if not err and want is not None and list(got) != list(want):
            err = "detect_reloc: %s, model %s" % (list(got)[:12], list(want)[:12])
        return err or (last_query_diff(self.dev, self.model) if want is not None else "")


def draw_len(rng, n_words):
    n = int(rng.choice([1, 5, 63, 64, 65, 200]) if rng.random() < 0.5 else rng.integers(1, 260))
    return min(n, n_words)


def draw_vector(rng, n_words, bases):
    """mostly a vector that overlaps an earlier one (so that queries find rows), sometimes a fresh or a broken one"""
    u = rng.random()
    if bases and u < 0.7:
        b = bases[int(rng.integers(len(bases)))]
        keep = int(rng.integers(0, len(b[0]) + 1))
        v = M.vector_from(rng, b[0], b[1], keep, n_words, int(rng.integers(0, 40)))
    else:
        v = M.random_vector(rng, n_words, draw_len(rng, n_words))
    if u > 0.97 and len(v[0]) >= 2:  # K8: broken vectors are refused by both sides
        ids, vals = v[0].copy(), v[1].copy()
        kind = int(rng.integers(3))
        if kind == 0:
            ids[1] = ids[0]
        elif kind == 1:
            ids[-1] = n_words
        else:
            vals[int(rng.integers(len(vals)))] = [np.nan, np.inf, -np.inf][int(rng.integers(3))]
        return ids, vals
    return v


def one_round(rng, counts):
    n_words = int(rng.choice([300, 1000, 100000]))
    pair = Pair(n_words, initial_rows=int(rng.choice([0, 2, 2, 16])))
    bases = [M.random_vector(rng, n_words, draw_len(rng, n_words)) for _ in range(3)]
    id_pool = int(rng.choice([8, 40, 400]))
    errs = []
    try:
        for step in range(int(rng.integers(10, 120))):
            u = rng.random()
            kf_id = int(rng.integers(0, id_pool))
            if u < 0.40:
                v = draw_vector(rng, n_words, bases)
                err = pair.add(kf_id, *v)
                if len(bases) < 12 and M.valid_vector(n_words, *v) and len(v[0]):
                    bases.append(v)
                op = "add"
            elif u < 0.55:
                nb = rng.integers(0, id_pool, size=int(rng.integers(0, 12))).tolist()
                err, op = pair.set_covisibles(kf_id, nb), "set_covisibles"
            elif u < 0.65:
                err, op = pair.erase(rng.integers(0, id_pool + 3, size=int(rng.integers(1, 4))).tolist()), "erase"
            elif u < 0.67:
                err, op = pair.clear(), "clear"
            elif u < 0.72:
                q = draw_vector(rng, n_words, bases)
                err, op = pair.score(q[0], q[1], rng.integers(0, id_pool + 3, size=int(rng.integers(0, 20))).tolist()), "score"
            else:
                q = draw_vector(rng, n_words, bases)
                if rng.random() < 0.5:
                    conn = rng.integers(0, id_pool, size=int(rng.integers(0, 6))).tolist()
                    ms = float(rng.choice([0.0, 0.01, 0.05, 0.3]))
                    err, op = pair.loop(q[0], q[1], conn, ms), "loop"
                else:
                    err, op = pair.reloc(*q), "reloc"
            counts[op] = counts.get(op, 0) + 1
            if err:
                errs.append("step %d (%s, n_words %d): %s" % (step, op, n_words, err))
                break
    finally:
        pair.close()
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
    q = counts.get("loop", 0) + counts.get("reloc", 0)
    print("%s %d rounds, %d queries, %d scores, %d edits in %.1f s (seed %d; vs CPU restatement; DBoW2 boundary unpinned)" % (
        "fuzz FAILED" if errs else "fuzz ok", rounds, q, counts.get("score", 0),
        sum(v for k, v in counts.items() if k not in ("loop", "reloc", "score")), time.time() - t0, seed))
    sys.exit(1 if errs else 0)


if __name__ == "__main__":
    main()

"""Randomised comparison of orbgpu_covis_graph_compact and orbgpu_keyframe_db_compact with tests/compact_model.py.

usage: python tools/fuzz_compact.py SECONDS SEED

Runs the rounds of tools/fuzz_covis.py, fuzz_cull.py, fuzz_refresh.py and fuzz_kfdb.py in turn -- their random edits, refused
calls and queries, drawn as those tools draw them -- on pairs that compact device and model at random points: after any
call of a round, edits inside the pointer map's SetBadFlag cascade included, with a probability drawn per round and from a
generator of its own; some compactions are preceded by a set_parent that names a bad row, so that C1 has rows to keep.
Every field of the result structure must equal the model's, and so must every query that follows (C1-C7, D1-D4 of
include/orbgpu.h).  Exit status 1 on any mismatch."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import compact_model as XM  # noqa: E402
import fuzz_covis  # noqa: E402
import fuzz_cull  # noqa: E402
import fuzz_kfdb  # noqa: E402
import fuzz_refresh  # noqa: E402


class Points:
    """where the compactions fall: a generator apart from the rounds' own, and what they did"""
    rng = np.random.default_rng(0)
    p = 0.1
    stats = dict(compactions=0, no_ops=0, rows_dropped=0, slots_freed=0, bad_kept=0)

    @classmethod
    def record(cls, res):
        s = cls.stats
        s["compactions" if res["compacted"] else "no_ops"] += 1
        s["rows_dropped"] += res["rows_before"] - res["rows_after"]
        s["slots_freed"] += res["slots_before"] - res["slots_after"]
        s["bad_kept"] += res["rows_bad_kept"] if res["compacted"] else 0


class CompactingPair:
    """mix-in for fuzz_covis.Pair and the pairs that extend it: the model is its compacting form (tests/compact_model.py), and
    every call of a round may be followed by a compaction of both sides"""

    def __init__(self, initial_rows=0, initial_slots=0):
        super().__init__(initial_rows, initial_slots)
        self.model = XM.compacting(type(self.model))(initial_rows, initial_slots)

    def compact(self):
        """'' or what differs"""
        got, want = self.dev.compact(), self.model.compact()
        Points.record(got)
        for k in XM.RESULT_FIELDS:
            if k in ("row_capacity", "slot_capacity") and want["row_capacity"] == 0:
                continue  # the model binds with the first key frame, the device may have done so for a query
            if got[k] != want[k]:
                return "compact %s: %s, model %s" % (k, got, want)
        return self.size()

    def name_bad_parent(self):
        """C1's other half: the pointer map re-parents the children before a key frame goes bad, so no round leaves a bad
        parent behind; now and then a live row is given one here, on both sides, before the compaction"""
        live = [r.id for r in self.model.rows if not r.bad]
        bad = [r.id for r in self.model.rows if r.bad]
        if not live or not bad or Points.rng.random() >= 0.3:
            return ""
        return self._edit("set_parent", live[int(Points.rng.integers(len(live)))], bad[int(Points.rng.integers(len(bad)))])

    busy = False

    def _both(self, name, dev_call, model_call):
        out = super()._both(name, dev_call, model_call)
        if not out[0] and not self.busy and Points.rng.random() < Points.p:
            self.busy = True
            try:
                err = self.name_bad_parent() or self.compact()
            finally:
                self.busy = False
            if err:
                return err, None, None
        return out


class CompactCovisPair(CompactingPair, fuzz_covis.Pair):
    pass


class CompactCullPair(CompactingPair, fuzz_cull.CullPair):
    pass


class CompactRefreshPair(CompactingPair, fuzz_refresh.RefreshPair):
    pass


class CompactKfdbPair(fuzz_kfdb.Pair):
    """fuzz_kfdb.Pair with compactions: the database model has no dead rows (D2), so the result structure is checked against
    what the model holds and the rules of D3"""

    def __init__(self, n_words, initial_rows=0):
        super().__init__(n_words, initial_rows)
        self.model = XM.CompactKeyFrameDatabase(n_words)
        self.rows0 = initial_rows if initial_rows > 0 else 1024

    def compact(self):
        got = self.dev.compact()
        self.model.compact()
        Points.record(got)
        want = dict(rows_after=self.model.size(), slots_after=self.model.pool_used(), rows_bad_kept=0)
        if got["compacted"]:
            want.update(row_capacity=XM.fresh_capacity(1, self.rows0, want["rows_after"]),
                        slot_capacity=XM.fresh_capacity(1024, min(self.rows0 * 512, 1 << 22), want["slots_after"]))
        else:
            want.update(rows_before=got["rows_after"], slots_before=got["slots_after"])
        for k, v in want.items():
            if got[k] != v:
                return "compact %s: %s, model %s" % (k, got, want)
        if got["rows_before"] < got["rows_after"] or got["slots_before"] < got["slots_after"]:
            return "compact grew the database: %s" % got
        return self.size() or fuzz_kfdb.last_query_diff(self.dev, self.model)  # D2: n = 0 on both sides

    def _both(self, name, dev_call, model_call):
        out = super()._both(name, dev_call, model_call)
        if not out[0] and Points.rng.random() < Points.p:
            err = self.compact()
            if err:
                return err, None, None
        return out


def refresh_refused_call(rng, pair, kf_ids):
    """fuzz_refresh.refused_call reads the model's row of the key frame it draws: it draws among the ids that are still rows"""
    rows = [k for k in kf_ids if k in pair.model.row_of]
    return _refresh_refused_call(rng, pair, rows) if rows else ""


_refresh_refused_call = fuzz_refresh.refused_call
ROUNDS = (("covis", fuzz_covis, "Pair", CompactCovisPair), ("cull", fuzz_cull, "CullPair", CompactCullPair),
          ("refresh", fuzz_refresh, "RefreshPair", CompactRefreshPair), ("kfdb", fuzz_kfdb, "Pair", CompactKfdbPair))
QUERIES = ("local_map", "connections", "culling", "reference_culling", "observations", "refresh", "table_refresh", "score", "loop",
           "reloc")


def one_round(rng, which, counts):
    """a round of the `which`-th fuzzer with its pair class replaced by the compacting one"""
    name, module, attr, cls = ROUNDS[which]
    Points.p = float(Points.rng.choice([0.02, 0.1, 0.3]))
    saved = getattr(module, attr)
    setattr(module, attr, cls)
    fuzz_refresh.refused_call = refresh_refused_call
    try:
        return ["%s round: %s" % (name, e) for e in module.one_round(rng, counts)]
    finally:
        setattr(module, attr, saved)
        fuzz_refresh.refused_call = _refresh_refused_call


def run(seconds, seed):
    rng = np.random.default_rng(seed)
    Points.rng = np.random.default_rng([seed, 0xC0])
    Points.stats = dict.fromkeys(Points.stats, 0)
    counts, errs, rounds = {}, [], 0
    t_end = time.time() + seconds
    while True:
        errs += one_round(rng, rounds % len(ROUNDS), counts)
        rounds += 1
        if errs or time.time() >= t_end:
            return rounds, counts, errs


def main():
    seconds, seed = float(sys.argv[1]), int(sys.argv[2])
    t0 = time.time()
    rounds, counts, errs = run(seconds, seed)
    for e in errs[:20]:
        print("MISMATCH " + e)
    s = Points.stats
    print("%s %d rounds, %d compactions, %d rows dropped, %d queries compared, %d compact calls with nothing to do, %d bad rows kept, "
          "%d slots freed, %d other calls in %.1f s (seed %d; vs tests/compact_model.py, exact equality)" % (
              "fuzz FAILED" if errs else "fuzz ok", rounds, s["compactions"], s["rows_dropped"], sum(counts.get(q, 0) for q in QUERIES),
              s["no_ops"], s["bad_kept"], s["slots_freed"], sum(v for k, v in counts.items() if k not in QUERIES), time.time() - t0, seed))
    sys.exit(1 if errs else 0)


if __name__ == "__main__":
    main()

"""Compaction of the observation graph and the key-frame database (orbgpu_covis_graph_compact, orbgpu_keyframe_db_compact)
restated in plain Python -- test infrastructure, like covis_model.py, whose graph it extends.  It is the definition of
conventions C1-C5 and D1-D2 (include/orbgpu.h): the device's result structure and every query after
a compaction are compared with it, entry for entry.

`Compacting` is a mix-in for covis_model.CovisGraph and the models that extend it (cull_model.CullGraph,
refresh_model.RefreshGraph): `CompactGraph`, `CompactCullGraph` and `CompactRefreshGraph` below.  Besides compact() it
keeps what the result structure reports and the plain models have no notion of: which rows own pool space, and the row
and pool capacity the doubling rules give (they outlive clear(), as the device's buffers do)."""
import covis_model as M
import cull_model as CM
import kfdb_model as KM
import refresh_model as RM

RESULT_FIELDS = ("compacted", "rows_before", "rows_after", "rows_bad_kept", "row_capacity", "slots_before", "slots_after",
                 "slot_capacity")


def grow(cap, base, want):
    """the doubling rule of cv_grow_rows / cv_grow_pool (and the database's): capacity `cap` asked for `want`"""
    if want <= cap:
        return cap
    cap = max(cap, base)
    while cap < want:
        cap *= 2
    return cap


def fresh_capacity(base, initial, want):
    """C5 / D3: a fresh handle created for `initial` that has since been asked for `want`"""
    return grow(grow(0, base, initial), base, want)


def graph_initial(initial_rows, initial_slots):
    """what the first call of a graph allocates for"""
    rows0 = initial_rows if initial_rows > 0 else 1024
    return rows0, initial_slots if initial_slots > 0 else min(rows0 * 1024, 1 << 22)


class Compacting:
    def __init__(self, initial_rows=0, initial_slots=0):
        self.rows0, self.slots0 = graph_initial(int(initial_rows), int(initial_slots))
        self.row_cap = self.pool_cap = 0  # 0: the device is not bound yet
        self.no_pool = set()              # kept bad rows (their _Row objects) that a compaction left without pool space
        super().__init__()

    def clear(self):
        super().clear()
        self.no_pool = set()

    def _bind(self):
        self.row_cap = grow(self.row_cap, 1, self.rows0)
        self.pool_cap = grow(self.pool_cap, 1024, self.slots0)

    def pool_used(self):
        return sum(len(r.slots) for r in self.rows if r not in self.no_pool)

    def add_keyframe(self, kf_id, n_slots, mp_ids=None):
        super().add_keyframe(kf_id, n_slots, mp_ids)
        self._bind()
        self.row_cap = grow(self.row_cap, 1, len(self.rows))
        self.pool_cap = grow(self.pool_cap, 1024, self.pool_used())

    def keep_set(self):
        """C1: the rows a compaction keeps, in add order"""
        named = {r.parent for r in self.rows if not r.bad}
        return [r for r in self.rows if not r.bad or r.id in named]

    def compact(self):
        before_rows, before_slots = len(self.rows), self.pool_used()
        kept = self.keep_set()
        kept_ids = {r.id for r in kept}
        res = dict(compacted=0, rows_before=before_rows, rows_after=before_rows, rows_bad_kept=sum(1 for r in self.rows if r.bad),
                   row_capacity=self.row_cap, slots_before=before_slots, slots_after=before_slots, slot_capacity=self.pool_cap)
        after_slots = sum(len(r.slots) for r in kept if not r.bad)
        if len(kept) == before_rows and after_slots == before_slots:  # C6
            return res
        for r in self.rows:  # C2: a dropped id is an unknown id; whatever the extended models keep per id goes with it
            if r.id not in kept_ids:
                del self.row_of[r.id]
                for per_id in ("kp", "desc", "centre"):
                    getattr(self, per_id, {}).pop(r.id, None)
        self.rows = kept  # C3: the row objects stay what they were (slots, parent, covisibles, stamp)
        self.no_pool = {r for r in kept if r.bad}
        self.row_cap = fresh_capacity(1, self.rows0, len(kept))      # C5
        self.pool_cap = fresh_capacity(1024, self.slots0, after_slots)
        res.update(compacted=1, rows_after=len(kept), rows_bad_kept=len(self.no_pool), row_capacity=self.row_cap,
                   slots_after=after_slots, slot_capacity=self.pool_cap)
        return res


class CompactGraph(Compacting, M.CovisGraph):
    pass


class CompactCullGraph(Compacting, CM.CullGraph):
    pass


class CompactRefreshGraph(Compacting, RM.RefreshGraph):
    pass


def compacting(model_class):
    """the compacting form of covis_model.CovisGraph or of a model that extends it"""
    return type("Compact" + model_class.__name__, (Compacting, model_class), {})


class CompactKeyFrameDatabase(KM.KeyFrameDatabase):
    """D2: the model has no dead rows, so a compaction is invisible -- but for last_query, which starts over"""

    def compact(self):
        self.last = []

    def pool_used(self):
        """the entries the live key frames hold (what the device reports as slots_after)"""
        return sum(len(kf.ids) for kf in self.kfs.values())

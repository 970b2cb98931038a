"""MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:242-307) and MapPoint::UpdateNormalAndDepth (:330-371) over the
observation graph (orbgpu_covis_refresh_points, orbgpu_mappoint_table_refresh) restated in numpy / plain Python -- test
infrastructure, like cull_model.py, whose graph it extends.  It is the definition of conventions R1-R8 (include/orbgpu.h,
DESIGN.md section 2): the device is compared with it bit for bit, floats as their 32-bit patterns.  Every float operation
below is one IEEE operation on np.float32 or np.float64 scalars, in the order R5 / R6 give."""
import numpy as np

import cull_model as CM
from covis_model import Refused  # noqa: F401

DESCRIPTOR, NORMAL_DEPTH = 1, 2
NO_OBS, OVERFLOW, NO_DESC, NO_CENTRE, NO_REF, UNKNOWN, BAD = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40
MAX_OBS = 1024
MAX_POINTS = 1 << 20
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def median_choice(desc):
    """R4 over the ordered group desc [N][32]: the index of the row with the least median Hamming distance to all rows
    (itself included), the median being the sorted distance row at (N - 1) >> 1; the first minimum wins"""
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    n = len(d)
    dist = POPCOUNT[d[:, None, :] ^ d[None, :, :]].sum(axis=2, dtype=np.int32)
    med = np.sort(dist, axis=1)[:, (n - 1) >> 1]
    return int(np.argmin(med))  # (argmin returns the first minimum)


def direction(P, Ow):
    """R5's term of one observation and R6's distance: (d * inv [3] float32, (float)nrm)"""
    f32, f64 = np.float32, np.float64
    with np.errstate(all="ignore"):
        d = [f32(f32(P[c]) - f32(Ow[c])) for c in range(3)]
        nrm = np.sqrt((f64(d[0]) * f64(d[0]) + f64(d[1]) * f64(d[1])) + f64(d[2]) * f64(d[2]))
        inv = f32(f64(1.0) / nrm)
        return [f32(d[c] * inv) for c in range(3)], f32(nrm)


class RefreshGraph(CM.CullGraph):
    def clear(self):
        super().clear()
        self.desc = {}     # key frame id -> uint8 [n_slots][32]
        self.centre = {}   # key frame id -> float32 [3]
        self.scale = None  # float32 [n_levels]

    def set_scale_factors(self, scale_factors):
        sf = np.array(scale_factors, np.float32).reshape(-1)
        if not 1 <= len(sf) <= CM.MAX_LEVELS or not np.all(np.isfinite(sf)) or not np.all(sf > 0):
            raise Refused("set_scale_factors")
        self.scale = sf

    def set_descriptors(self, kf_id, desc):
        kf_id = int(kf_id)
        d = np.array(np.zeros((0, 32), np.uint8) if desc is None else desc, np.uint8).reshape(-1, 32)
        row = self.row_of.get(kf_id)
        if row is None or len(d) != len(row.slots):
            raise Refused("set_descriptors")
        if not row.bad and len(d):
            self.desc[kf_id] = d

    def set_centres(self, kf_ids, centres):
        c = np.array(centres, np.float32).reshape(-1, 3)
        known = 0
        for k, ow in zip(kf_ids, c):
            row = self.row_of.get(int(k))
            if row is None:
                continue
            known += 1
            if not row.bad:
                self.centre[int(k)] = ow.copy()
        return known

    def observations_of(self, p):
        """R1: [(key frame id, slot index)] in ascending (id, index)"""
        out = []
        for row in self.rows:
            if not row.bad:
                out += [(row.id, i) for i, q in enumerate(row.slots) if q == p]
        return sorted(out)

    def refresh(self, mp_ids, ref_kf_ids, world_pos, what=DESCRIPTOR | NORMAL_DEPTH, initial=None, pre=None):
        """dict of normal, min_dist, max_dist, desc (in/out: they start from `initial[name]`, zeros otherwise), desc_kf,
        desc_idx, n_slots, status and the fields of orbgpu_covis_refresh_result.  pre (the table form): per point UNKNOWN, BAD
        or 0."""
        ids = [int(p) for p in mp_ids]
        refs = [int(k) for k in ref_kf_ids]
        n = len(ids)
        if n > MAX_POINTS or len(refs) != n or what == 0 or what & ~3 or any(p < 0 for p in ids) or len(set(ids)) != n:
            raise Refused("refresh")
        pos = np.array(world_pos, np.float32).reshape(n, 3)
        initial = initial or {}
        out = dict(normal=np.array(initial.get("normal", np.zeros((n, 3))), np.float32).reshape(n, 3),
                   min_dist=np.array(initial.get("min_dist", np.zeros(n)), np.float32).reshape(n),
                   max_dist=np.array(initial.get("max_dist", np.zeros(n)), np.float32).reshape(n),
                   desc=np.array(initial.get("desc", np.zeros((n, 32))), np.uint8).reshape(n, 32),
                   desc_kf=np.full(n, -1, np.int64), desc_idx=np.full(n, -1, np.int32), n_slots=np.zeros(n, np.int32),
                   status=np.zeros(n, np.uint8))
        res = dict(n_descriptors=0, n_normals=0, n_entries=0)
        for i, p in enumerate(ids):
            obs = self.observations_of(p)
            N = out["n_slots"][i] = len(obs)
            st = 0
            if pre is not None and pre[i]:
                st = int(pre[i])
            elif N == 0:
                st = NO_OBS  # R2
            elif N > MAX_OBS:
                st = OVERFLOW  # R3
            if st:
                out["status"][i] = st
                continue
            res["n_entries"] += N
            if what & DESCRIPTOR:  # R4
                if any(k not in self.desc for k, _ in obs):
                    st |= NO_DESC
                else:
                    best = median_choice(np.stack([self.desc[k][j] for k, j in obs]))
                    k, j = obs[best]
                    out["desc"][i], out["desc_kf"][i], out["desc_idx"][i] = self.desc[k][j], k, j
                    res["n_descriptors"] += 1
            if what & NORMAL_DEPTH:  # R5, R6
                if any(k not in self.centre for k, _ in obs):
                    st |= NO_CENTRE
                ref_slots = [j for k, j in obs if k == refs[i]]
                level = self.kp[refs[i]][ref_slots[0]] & CM.KP_OCTAVE if ref_slots else -1
                if not ref_slots or self.scale is None or level >= len(self.scale):
                    st |= NO_REF
                if not st & (NO_CENTRE | NO_REF):
                    acc = [np.float32(0.0)] * 3
                    with np.errstate(all="ignore"):
                        for k, _ in obs:
                            term, _ = direction(pos[i], self.centre[k])
                            acc = [np.float32(acc[c] + term[c]) for c in range(3)]
                        inv_n = np.float32(np.float64(1.0) / np.float64(N))
                        out["normal"][i] = [np.float32(acc[c] * inv_n) for c in range(3)]
                        _, dist = direction(pos[i], self.centre[refs[i]])
                        mx = np.float32(dist * self.scale[level])
                        out["max_dist"][i] = mx
                        out["min_dist"][i] = np.float32(mx / self.scale[len(self.scale) - 1])
                    res["n_normals"] += 1
            out["status"][i] = st
        s = out["status"]
        res.update(n_no_obs=int(np.sum(s & NO_OBS != 0)), n_overflow=int(np.sum(s & OVERFLOW != 0)),
                   n_no_desc=int(np.sum(s & NO_DESC != 0)), n_no_centre=int(np.sum(s & NO_CENTRE != 0)),
                   n_no_ref=int(np.sum(s & NO_REF != 0)), n_unknown=int(np.sum(s & UNKNOWN != 0)), n_bad=int(np.sum(s & BAD != 0)),
                   max_obs=int(out["n_slots"].max()) if n else 0)
        out.update(res)
        return out


FLOAT_FIELDS = ("normal", "min_dist", "max_dist")
EXACT_FIELDS = ("desc", "desc_kf", "desc_idx", "n_slots", "status")
COUNT_FIELDS = ("n_descriptors", "n_normals", "n_no_obs", "n_overflow", "n_no_desc", "n_no_centre", "n_no_ref", "n_unknown", "n_bad",
                "max_obs", "n_entries")


def compare(got, want, fields=None):
    """"" if the device's dict equals the model's in every field both hold: floats as their 32-bit patterns; else a message"""
    for name in fields or FLOAT_FIELDS + EXACT_FIELDS + COUNT_FIELDS:
        if name not in got or name not in want:
            continue
        a, b = got[name], want[name]
        if name in FLOAT_FIELDS:
            a, b = np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32)
        a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
        if a.shape != b.shape or not np.array_equal(a, b):
            where = np.argwhere(a != b)[:4].tolist() if a.shape == b.shape else "shapes %s / %s" % (a.shape, b.shape)
            return "%s differs at %s: %s, model %s" % (name, where, np.asarray(got[name]).reshape(-1)[:8].tolist(),
                                                        np.asarray(want[name]).reshape(-1)[:8].tolist())
    return ""


def junk(rng, n):
    """in/out arrays to start a refresh from: what the rules leave untouched must come back as these bytes"""
    return dict(normal=rng.normal(size=(n, 3)).astype(np.float32), min_dist=rng.random(n).astype(np.float32),
                max_dist=rng.random(n).astype(np.float32), desc=rng.integers(0, 256, (n, 32)).astype(np.uint8))


# ---- the scene the GPU tests and tools/fuzz_refresh.py share; g is a RefreshGraph or a pair of it and a device graph ----
PATTERNS = np.random.default_rng(20261021).integers(0, 256, (8, 32)).astype(np.uint8)


def base_scene(rng, g, n_kf=12, n_slots=64, n_pts=150, max_obs=12, first_kf=1000, n_levels=3, descriptors=True, centres=True,
               scale=True):
    """n_kf key frames of n_slots slots, ids descending from first_kf + 7 * n_kf (rows are not in id order); point p in
    [0, n_pts) is held by 1 .. max_obs key frames; descriptors from PATTERNS (median ties), octaves below n_levels, centres in
    the unit cube, points 2 to 6 units away.  Returns (kf ids, point ids, world positions, reference key frame per point)."""
    kf_ids = [first_kf + 7 * (n_kf - i) for i in range(n_kf)]
    slots = {k: [-1] * n_slots for k in kf_ids}
    free = {k: list(rng.permutation(n_slots)) for k in kf_ids}
    ref = []
    for p in range(n_pts):
        want = min(max_obs, 1 + int((max_obs - 0.01) * rng.random() ** 3))  # a third of max_obs on average: the slots suffice
        holders = [k for k in (kf_ids[int(j)] for j in rng.permutation(n_kf)) if free[k]][:want]
        for k in holders:
            slots[k][int(free[k].pop())] = p
        ref.append(holders[int(rng.integers(len(holders)))] if holders else kf_ids[0])
    for k in kf_ids:
        g.add_keyframe(k, n_slots, slots[k])
        g.set_keypoints(k, rng.integers(0, n_levels, n_slots).astype(np.uint8))
        if descriptors:
            g.set_descriptors(k, PATTERNS[rng.integers(0, len(PATTERNS), n_slots)])
    if centres:
        g.set_centres(kf_ids, rng.random((n_kf, 3)).astype(np.float32))
    if scale:
        g.set_scale_factors(np.float32(1.2) ** np.arange(n_levels, dtype=np.float32))
    v = rng.normal(size=(n_pts, 3))
    pos = (0.5 + v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(2.0, 6.0, (n_pts, 1))).astype(np.float32)
    return kf_ids, list(range(n_pts)), pos, ref

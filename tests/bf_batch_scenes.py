"""Scenes of the batched matcher tests (test_gpu_matcher_batch.py, test_bf_batch_scenes.py); the device-side packing
is tools/bf_batch_pack.py, which tools/fuzz_bf.py uses too.

A problem is one (A, B) pair with the parameters it is matched under.  The parameters (threshold, ratio, rotation check,
whether a validity mask is passed) are arguments of a CALL, not of a pair, so `run` issues one call per distinct
parameter set over the whole batch and keeps, from each call, the pairs that belong to it.

The conflict scene is low_entropy() of test_gpu_matcher_bf.py: few base descriptors, 2 % byte noise, so that more than
four A rows share their four nearest B rows and the later ones, finding their cached list claimed, are decided by the
exact full scan.  `outside_four_nearest` counts those decisions in a result of the oracle."""
import os
import sys
from types import SimpleNamespace

import numpy as np

from test_gpu_matcher_bf import low_entropy

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from bf_batch_pack import pack, run  # noqa: E402,F401  the device side, shared with tools/fuzz_bf.py

SETTINGS = [(10.0, 256), (2.0, 100), (0.7, 50)]  # (nnratio, th_low)
_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.uint8)


def hamming_matrix(a, b):
    return _POP[a[:, None, :] ^ b[None, :, :]].sum(-1, dtype=np.int64)


def conflict(seed, na, nb, pool, ratio, th, ori, masked):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (pool, 32), dtype=np.uint8)
    a, b = low_entropy(rng, na, base), low_entropy(rng, nb, base)
    aa, ab = (rng.random(na) * 360).astype(np.float32), (rng.random(nb) * 360).astype(np.float32)
    valid = (rng.random(na) < 0.9).astype(np.uint8) if masked else None
    return SimpleNamespace(a=a, b=b, aa=aa, ab=ab, valid=valid, node_a=None, node_b=None, ratio=float(ratio), th=int(th),
                           ori=bool(ori), seed=seed)


def with_nodes(pr, ids=(3, 7, 8, 20, 21, 40), none_frac=0.1):
    """Labels the rows of a conflict scene with vocabulary nodes (-1: not in the feature vector).  Labels and
    descriptors are independent, so every node holds rows of every base descriptor: the conflicts stay inside it."""
    rng = np.random.default_rng(pr.seed + 50000)
    for side, n in (("node_a", len(pr.a)), ("node_b", len(pr.b))):
        lab = np.asarray(ids, np.int32)[rng.integers(0, len(ids), n)]
        lab[rng.random(n) < none_frac] = -1
        setattr(pr, side, lab)
    return pr


def feature_vector(labels):
    """The FeatureVector of orbgpu_bow_transform as CSR: nodes ascending, items ascending inside a node, -1 left out."""
    live = np.nonzero(labels >= 0)[0]
    order = live[np.argsort(labels[live], kind="stable")]
    nodes, counts = np.unique(labels[live], return_counts=True)
    start = np.concatenate([[0], np.cumsum(counts)])
    return {"fv_nodes": nodes.astype(np.int32), "fv_start": start.astype(np.int32), "fv_items": order.astype(np.int32)}


def expected(oracle, pr, claims=False):
    """(nmatches, match_b[:nb]) of the oracle; cached on the problem (computed once, never modified).
    claims=True: before the rotation check, i.e. every decision of the greedy pass."""
    slot, ori = ("claimed", False) if claims else ("want", pr.ori)
    if getattr(pr, slot, None) is None:
        if pr.node_a is not None:
            n, m = oracle.search_by_bow(pr.a, pr.aa, pr.valid, feature_vector(pr.node_a), pr.b, pr.ab,
                                        feature_vector(pr.node_b), pr.th, pr.ratio, ori)
        else:
            n, m = oracle.match_bf(pr.a, pr.aa, pr.b, pr.ab, valid_a=pr.valid, th_low=pr.th, nnratio=pr.ratio,
                                   check_orientation=ori)
        m.setflags(write=False)
        setattr(pr, slot, (int(n), m))
    return getattr(pr, slot)


def outside_four_nearest(pr, match_b):
    """Matches (i, j) of `match_b` whose j is not among the four smallest (distance, index) keys of row i over the B
    rows it may match (all of them, or those of its node): each was decided by the full scan."""
    if len(pr.a) == 0 or len(pr.b) == 0:
        return 0
    key = hamming_matrix(pr.a, pr.b) * 4096 + np.arange(len(pr.b))
    if pr.node_a is not None:
        key[pr.node_a[:, None] != pr.node_b[None, :]] = 1 << 40
    count = 0
    for j in np.nonzero(match_b >= 0)[0]:
        i = match_b[j]
        count += int(key[i, j] not in np.sort(key[i])[:4])
    return count


# ---- the committed problem sets -------------------------------------------------------------------------------------
def _masked(p):
    return ((p + 1) // 2) % 2 == 1  # pairs 1, 2, 5, 6: every second pair, not in step with the rotation check


def _cycle(seed0, shapes):
    """Pair p: settings p % 3, rotation check on odd pairs, a validity mask on every second pair.  A shape may name
    its seed (the ratio-0.7 pairs: chosen so that the oracle accepts something, test_bf_batch_scenes.py)."""
    return [conflict(sh[3] if len(sh) > 3 else seed0 + p, sh[0], sh[1], sh[2], *SETTINGS[p % 3], ori=p % 2 == 1,
                     masked=_masked(p)) for p, sh in enumerate(shapes)]


_sets = {}


def problems(name):
    if name not in _sets:
        _sets[name] = _BUILD[name]()
    return _sets[name]


_BUILD = {
    # (na, nb, pool); cap 320
    "split": lambda: _cycle(9100, [(300, 300, 40), (200, 256, 20), (300, 300, 40, 9113), (257, 129, 12), (320, 320, 20),
                                   (129, 257, 40, 9127), (256, 320, 20), (320, 64, 12), (65, 320, 40, 9108)]),
    "ragged": lambda: _cycle(9200, [(0, 300, 12), (300, 0, 12), (1, 1, 12), (1, 320, 12), (320, 1, 12), (255, 63, 12),
                                    (256, 64, 12), (257, 65, 12), (320, 5, 12)]),
    "unstaged": lambda: [conflict(9300, 300, 300, 40, 10.0, 256, False, False),
                         conflict(9301, 300, 300, 40, 2.0, 100, True, True)],
    # cap 704
    "threads": lambda: _cycle(9400, [(700, 700, 40), (300, 300, 20), (257, 257, 40, 9110)]),
    "nodes": lambda: [with_nodes(conflict(9500 + p, na, nb, 12, ratio, th, ori, True))
                      for p, (na, nb) in enumerate([(300, 300), (320, 257), (200, 320)])
                      for ratio, th, ori in ((0.95, 50, True), (10.0, 256, False))],
    "nodes_empty": lambda: [with_nodes(conflict(9600 + p, na, nb, 12, 10.0, 256, p == 1, True))
                            for p, (na, nb) in enumerate([(0, 100), (300, 300), (100, 0)])],
}

"""Device-side packing for the batched matchers (BatchMatcher.match / search_by_bow), shared by tools/fuzz_bf.py and
tests/bf_batch_scenes.py.  A problem is any object with a, b ([n,32] uint8), aa, ab (float32 angles), valid (uint8 mask
or None), node_a, node_b (int32 labels or None) and the call parameters th, ratio, ori.  Threshold, ratio, rotation
check and the mask pointer are arguments of a CALL, so `run` issues one call per distinct parameter set over the whole
batch and keeps, from each call, the pairs that belong to it."""
from types import SimpleNamespace

import numpy as np


def pack(prs, cap, seed=1):
    """[pairs][cap] device arrays of the problems.  Everything behind a pair's row count is seeded random bytes
    (descriptors, angles, validity); node garbage is drawn from the pair's own live node ids, so a kernel that reads
    behind the count finds plausible candidates there.  Pairs without a mask get an all-ones one."""
    import torch
    rng = np.random.default_rng(seed)
    P = len(prs)
    raw = lambda *shape: rng.integers(0, 256, shape, dtype=np.uint8)
    h = dict(desc_a=raw(P, cap, 32), desc_b=raw(P, cap, 32), ang_a=raw(P, cap, 4).view(np.float32).reshape(P, cap),
             ang_b=raw(P, cap, 4).view(np.float32).reshape(P, cap), valid=raw(P, cap),
             na=np.array([len(q.a) for q in prs], np.int32), nb=np.array([len(q.b) for q in prs], np.int32))
    nodes = prs[0].node_a is not None
    if nodes:
        h["node_a"], h["node_b"] = np.full((P, cap), -1, np.int32), np.full((P, cap), -1, np.int32)
    for p, q in enumerate(prs):
        na, nb = len(q.a), len(q.b)
        h["desc_a"][p, :na], h["desc_b"][p, :nb] = q.a, q.b
        h["ang_a"][p, :na], h["ang_b"][p, :nb] = q.aa, q.ab
        h["valid"][p, :na] = 1 if q.valid is None else q.valid
        if nodes:
            live = np.concatenate([q.node_a[q.node_a >= 0], q.node_b[q.node_b >= 0]])
            for key, lab, n in (("node_a", q.node_a, na), ("node_b", q.node_b, nb)):
                h[key][p, :n] = lab
                if len(live):
                    h[key][p, n:] = live[rng.integers(0, len(live), cap - n)]
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in h.items()}
    d["match_b"] = torch.empty((P, cap), dtype=torch.int32, device="cuda")
    d["nm"] = torch.empty(P, dtype=torch.int32, device="cuda")
    return SimpleNamespace(cap=cap, pairs=P, nodes=nodes, **d)


def run(bm, prs, cap, seed=1):
    """Every problem through the batched entry (one call per distinct parameter set, all pairs in every call).
    Returns per pair (nmatches, match_b[:nb], match_b[nb:cap], sweeps) and the list of last_launch() dicts."""
    import torch
    d = pack(prs, cap, seed)
    stream = torch.cuda.current_stream().cuda_stream
    out, launches = [None] * len(prs), []
    for key in sorted({(q.th, q.ratio, q.ori, q.valid is not None) for q in prs}):
        th, ratio, ori, masked = key
        d.match_b.fill_(-7)
        d.nm.fill_(-7)
        args = [d.pairs, cap, d.desc_a.data_ptr(), d.ang_a.data_ptr(), d.valid.data_ptr() if masked else None]
        tail = [d.na.data_ptr(), d.desc_b.data_ptr(), d.ang_b.data_ptr()]
        if d.nodes:
            bm.search_by_bow(*args, d.node_a.data_ptr(), *tail, d.node_b.data_ptr(), d.nb.data_ptr(), 4, th, ratio, ori,
                             d.match_b.data_ptr(), d.nm.data_ptr(), stream)
        else:
            bm.match(*args, *tail, d.nb.data_ptr(), 4, th, ratio, ori, d.match_b.data_ptr(), d.nm.data_ptr(), stream)
        torch.cuda.synchronize()
        mb, nm, sweeps = d.match_b.cpu().numpy(), d.nm.cpu().numpy(), bm.last_sweeps(d.pairs)
        launches.append(bm.last_launch())
        for p, q in enumerate(prs):
            if (q.th, q.ratio, q.ori, q.valid is not None) == key:
                nb = len(q.b)
                out[p] = (int(nm[p]), mb[p, :nb].copy(), mb[p, nb:].copy(), int(sweeps[p]))
    return out, launches

"""Randomised parity sweep of the brute-force / vocabulary-guided matchers against the oracle: descriptor sets drawn
from small pools (many near-duplicates -> long claim chains), random sizes, thresholds, ratios, validity masks and
node labels.  Every second draw goes through the device-resident batched entry instead of the host call: 1-9 pairs of
the drawn family in one BatchMatcher, sized for exactly these pairs or for 64, with the row stride at the largest count
or at 3264 (no B descriptors in LDS), random bytes behind every row count.
    python tools/fuzz_bf.py [seconds] [seed]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from orb_slam2_map_amd import lib as G
from oracle import oracle_py as O
from types import SimpleNamespace
import bf_batch_pack as S

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
t0, n, n_ori, n_batch = time.time(), 0, 0, 0
while time.time() - t0 < budget:
    na, nb = int(rng.integers(1, 1300)), int(rng.integers(1, 1300))
    pool = int(rng.choice([4, 20, 100, 1000]))
    flip = float(rng.choice([0.0, 0.01, 0.03, 0.1]))
    base = rng.integers(0, 256, (pool, 32), dtype=np.uint8)

    def draw(m):
        d = base[rng.integers(0, pool, m)].copy()
        bits = np.unpackbits(d, axis=1)
        bits ^= (rng.random(bits.shape) < flip).astype(np.uint8)
        return np.packbits(bits, axis=1)
    ratio, th = float(rng.choice([0.6, 0.7, 0.9, 10.0])), int(rng.choice([30, 50, 100, 256]))
    ori = bool(rng.integers(0, 2))
    p_valid = rng.choice([0.5, 0.9, 1.0])

    def problem(na, nb):
        return SimpleNamespace(a=draw(na), b=draw(nb), aa=(rng.random(na) * 360).astype(np.float32),
                               ab=(rng.random(nb) * 360).astype(np.float32),
                               valid=(rng.random(na) < p_valid).astype(np.uint8), node_a=None, node_b=None, ratio=ratio,
                               th=th, ori=ori)

    def expected(q):
        return O.match_bf(q.a, q.aa, q.b, q.ab, valid_a=q.valid, th_low=th, nnratio=ratio, check_orientation=ori)
    if n % 2 == 0:
        q = problem(na, nb)
        ng, mg = G.ORBmatcher(ratio, ori).MatchBruteForce(q.a, q.aa, q.b, q.ab, valid_a=q.valid, th_low=th)
        no, mo = expected(q)
        bad = ng != no or not np.array_equal(mg, mo)
    else:
        pairs = int(rng.integers(1, 10))
        prs = [problem(na, nb)] + [problem(int(rng.integers(0, 1300)), int(rng.integers(0, 1300))) for _ in range(pairs - 1)]
        cap = int(rng.choice([max(max(len(q.a), len(q.b)) for q in prs), 3264]))
        bm = G.BatchMatcher(int(rng.choice([pairs, 64])), cap)
        out, _ = S.run(bm, prs, cap, seed=int(rng.integers(1 << 30)))
        bm.close()
        bad = False
        for q, (ng, mg, behind, _) in zip(prs, out):
            no, mo = expected(q)
            if ng != no or not np.array_equal(mg, mo) or np.any(behind != -1):
                bad, na, nb = True, len(q.a), len(q.b)
                break
        n_batch += 1
    if bad:
        print("FAIL bf", dict(na=na, nb=nb, pool=pool, flip=flip, ratio=ratio, th=th, ori=ori), ng, no)
        sys.exit(1)
    n += 1
    n_ori += ori
print("fuzz ok: %d matches, %d with the rotation check on uniform random angles, %d through the batched entry, in %.0f s" %
      (n, n_ori, n_batch, time.time() - t0))

"""Throughput and latency of the stereo stage (orbgpu_stereo_matches_batch_device / orbgpu_compute_stereo_matches) at
the reference's stereo operating point (KITTI: 1241 x 376, 2000 features, 8 levels, 1.2).

usage: python tools/stereo_bench.py [--reps N]

For B = 64 and 256 pairs: one extraction of 2B frames on one handle, then the stereo call, timed with HIP events on
one stream; prints pairs/s of extraction + stereo and the stereo stage's share.  Then the latency of one pair through
the host entry point (the key points already on the host, as Frame's constructor has them)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orb_slam2_map_amd import lib as G  # noqa: E402
from orb_slam2_map_amd.synth import StereoStream  # noqa: E402


def main():
    import torch
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
    st = StereoStream(1241, 376, 2024)
    w, h = st.w, st.h
    frames = [st.frame(t) for t in range(16)]
    out = {"size": [w, h], "nfeatures": 2000}
    for B in (64, 256):
        L = np.stack([frames[i % 16][0] for i in range(B)])
        R = np.stack([frames[i % 16][1] for i in range(B)])
        imgs = torch.from_numpy(np.concatenate([L, R])).cuda()
        ext = G.ORBextractor(2000, max_batch=2 * B)
        cap = ext.max_keypoints(w, h)
        k = torch.zeros((2 * B, cap, 7), dtype=torch.float32, device="cuda")
        d = torch.zeros((2 * B, cap, 32), dtype=torch.uint8, device="cuda")
        n = torch.zeros(2 * B, dtype=torch.int32, device="cuda")
        u = torch.zeros((B, cap), dtype=torch.float32, device="cuda")
        z = torch.zeros((B, cap), dtype=torch.float32, device="cuda")
        ns = torch.zeros(B, dtype=torch.int32, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        t_ext, t_st = [], []
        for r in range(reps + 3):
            ev[0].record()
            ext.extract_batch_device(imgs.data_ptr(), 2 * B, w, h, w, w * h, k.data_ptr(), d.data_ptr(), cap, n.data_ptr(), 0)
            ev[1].record()
            G.stereo_matches_batch_device(ext, 0, ext, B, B, cap, k.data_ptr(), n.data_ptr(), d.data_ptr(),
                                          k[B:].data_ptr(), n[B:].data_ptr(), d[B:].data_ptr(), st.bf, st.fx,
                                          u.data_ptr(), z.data_ptr(), ns.data_ptr(), 0)
            ev[2].record()
            torch.cuda.synchronize()
            if r >= 3:
                t_ext.append(ev[0].elapsed_time(ev[1]))
                t_st.append(ev[1].elapsed_time(ev[2]))
        me, ms = float(np.median(t_ext)), float(np.median(t_st))
        out["B%d" % B] = {"extract_2B_ms": round(me, 3), "stereo_ms": round(ms, 3),
                          "pairs_per_s": round(B / ((me + ms) / 1e3), 1), "stereo_share": round(ms / (me + ms), 4),
                          "matches_per_pair": float(ns.float().mean().item())}
        del ext
    el, er = G.ORBextractor(2000), G.ORBextractor(2000)
    left, right, _ = frames[0]
    kl, dl = el(left)
    kr, dr = er(right)
    lat = []
    for r in range(reps * 5 + 5):
        t0 = time.perf_counter()
        G.compute_stereo_matches(el, er, kl, dl, kr, dr, st.bf, st.fx)
        if r >= 5:
            lat.append((time.perf_counter() - t0) * 1e3)
    out["host_entry_one_pair_ms"] = {"median": round(float(np.median(lat)), 3), "p90": round(float(np.percentile(lat, 90)), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

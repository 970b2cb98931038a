"""Device time of Optimizer::OptimizeSim3 (orbgpu_sim3_optimize_batch_device) per call.

usage: python tools/bench_sim3opt.py [--reps N]

One candidate and 16 candidates per call at N = 30, 100 and 300 correspondences (seeded scenes of
tests/sim3opt_model.py, 30 % gross outliers, so that the second stage runs its 10 iterations), HIP events around the
call on one stream, 5 warm-up calls, median of the repetitions.  The iteration / trial counts of the result records are
reported so that a time can be read per LM trial.  There is no earlier implementation to compare with, and the CPU model
is not a baseline.  Writes profiles/sim3opt_bench.json and prints it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import fuzz_sim3opt as F  # noqa: E402
import sim3opt_model as M  # noqa: E402
from orb_slam2_map_amd import lib as G  # noqa: E402


def main():
    import torch
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 50
    s = torch.cuda.current_stream().cuda_stream
    out = {"threads_per_problem": 256, "reps": reps, "outlier_frac": 0.3}
    for n in (30, 100, 300):
        for B in (1, 16):
            scenes = [M.make_scene(n, 7000 + 31 * n + i, outlier_frac=0.3) for i in range(B)]
            ups = [F.upload(torch, sc) for sc in scenes]
            problems = [u[0] for u in ups]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ms = []
            for r in range(reps + 5):
                ev[0].record()
                G.sim3_optimize_batch_device(problems, stream=s)
                ev[1].record()
                torch.cuda.synchronize()
                if r >= 5:
                    ms.append(ev[0].elapsed_time(ev[1]))
            res = [F.download(u[1], len(sc["valid"]))[1] for u, sc in zip(ups, scenes)]
            med = float(np.median(ms))
            out["N%d_B%d" % (n, B)] = {
                "ms_per_call": round(med, 4), "ms_p90": round(float(np.percentile(ms, 90)), 4),
                "stages_min": int(min(r["stages"] for r in res)),
                "iterations_mean": float(np.mean([r["iterations"] for r in res])),
                "trials_mean": float(np.mean([r["trials"] for r in res])), "trials_max": int(max(r["trials"] for r in res)),
                "us_per_trial_of_slowest_problem": round(1e3 * med / max(r["trials"] for r in res), 3),
                "us_per_iteration_of_slowest_problem": round(1e3 * med / max(r["iterations"] for r in res), 3),
                "spilled_problems": G.sim3_opt_last_spills()}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sim3opt_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Device time of Optimizer::PoseOptimization (orbgpu_pose_optimization_batch_device) per call.

usage: python tools/bench_pose.py [--reps N]

One problem and 128 problems per call at N ~ 300 and N ~ 1500 edges (seeded scenes of tests/pose_model.py, 20 % gross
outliers, mixed mono / stereo), HIP events around the call on one stream, 5 warm-up calls, median of the repetitions.
The iteration / trial counts of the result structs are reported so that a time can be read per LM trial.  Writes
profiles/pose_bench.json and prints it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import fuzz_pose as F  # noqa: E402
import pose_model as M  # noqa: E402
from orb_slam2_map_amd import lib as G  # noqa: E402


def main():
    import torch
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 50
    s = torch.cuda.current_stream().cuda_stream
    out = {"threads_per_problem": 256, "reps": reps}
    for n_kp, label in ((375, "N300"), (1875, "N1500")):
        for B in (1, 128):
            scenes = [M.make_scene(n_kp, 7000 + i) for i in range(B)]
            ups = [F.upload(torch, sc) for sc in scenes]
            problems = [u[0] for u in ups]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ms = []
            for r in range(reps + 5):
                ev[0].record()
                G.pose_optimization_batch_device(problems, stream=s)
                ev[1].record()
                torch.cuda.synchronize()
                if r >= 5:
                    ms.append(ev[0].elapsed_time(ev[1]))
            res = [F.download(u[1], sc["n"])[1] for u, sc in zip(ups, scenes)]
            trials = float(np.mean([r["trials"] for r in res]))
            med = float(np.median(ms))
            out["%s_B%d" % (label, B)] = {
                "edges_mean": float(np.mean([r["n_initial"] for r in res])), "ms_per_call": round(med, 4),
                "ms_p90": round(float(np.percentile(ms, 90)), 4), "iterations_mean": float(np.mean([r["iterations"] for r in res])),
                "trials_mean": trials, "trials_max": int(max(r["trials"] for r in res)),
                "us_per_trial_of_slowest_problem": round(1e3 * med / max(r["trials"] for r in res), 3),
                "spilled_problems": G.pose_last_spills()}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pose_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

import os, sys, json; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from orb_slam2_map_amd import workloads
r = workloads.c4(); r.pop("per_keyframe")
print(json.dumps(r))

"""The learning curve of the five-arm RL2 model of tests/test_gpu_wide_meta.py, three seeds: the mean trial
reward on 4,096 fresh trials after every period -> profiles/wide_meta_learning.json.

    python scripts/wide_meta_learning.py [periods]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import relearn_amd as ra
import test_gpu_wide_meta as W
periods = int(sys.argv[1]) if len(sys.argv) > 1 else 60
eng = ra.Engine(0)
c = W.LEARNING
out = {"config": dict(c, periods=periods, bar=5.0, memoryless=2.0, arms_in_turn=8.0), "curves": {}, "seconds": {}}
for seed in (40, 50, 60):
    curve = []
    t0 = time.perf_counter()
    W.learn(eng, c["lanes"], c["episodes_per_trial"], c["trials_per_period"], c["hidden"], periods, seed, c["arms"], curve)
    out["seconds"][str(seed)] = time.perf_counter() - t0
    out["curves"][str(seed)] = curve
    first = next((i + 1 for i in range(len(curve)) if all(v > 5.0 for v in curve[i:])), None)
    print("seed %d: above 5.0 and staying from period %s; %.1f s with an evaluation per period" % (seed, first, out["seconds"][str(seed)]), flush=True)
    print(" ".join("%.2f" % v for v in curve), flush=True)
json.dump(out, open(os.path.join(ROOT, "profiles", "wide_meta_learning.json"), "w"), indent=1)

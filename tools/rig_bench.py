"""Time the rig self-calibration per iteration (64 and 1024 frames, 4 views, 15 joints) -> profiles/rig_refine_b64.json.

    python tools/rig_bench.py [--rounds 30] [--out profiles/rig_refine_b64.json]

One process.  Operands: the `noisy`-style scene of tests/rig_statement.py (the syn rig with cameras 1..3 tilted by 0.03 rad, random
points, 0.1 px of noise).  egr_rig_refine_f32 runs 1 + 2 (iterations + 1) launches, so its time at 4 and at 12 iterations gives the time
of one iteration - one accumulate launch plus one step launch - as (t12 - t4) / 8, and the rest (the ray pass, the first evaluation, the
output) as t4 - 4 iterations.  Next to it egr_triangulate_f32 on the same operands: the nearest yardstick, because an accumulate launch
contains a triangulation.  Method: every call is captured into a hipGraph of its own so that its kernels run back to back without the
host's enqueue time between them; the graphs are replayed in turn `rounds` times, each replay between two device events.  No target
was set for these numbers: they are reported as measured, with the ratio."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FRAMES, V, J = (64, 1024), 4, 15
THR, MIN_DET, HM = 0.5, 1e-6, 64
COUNTS = (4, 8, 12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rig_refine_b64.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rig_bench: needs the GPU (nothing is measured without one)")
    import rig_statement as RS
    from egorear_amd import hip
    dev = "cuda:0"
    res = {"views": V, "joints": J, "threshold": THR, "min_det_ratio": MIN_DET, "rounds": a.rounds, "device": hip.device_arch(),
           "library": hip.version(), "method": "one call per hipGraph, graphs replayed in turn, device events around each replay",
           "frames": {}}
    for B in FRAMES:
        sc = RS.scene(B, V, J, False, 0.03, 0.1, 7)
        coords, conf, rec = sc["coords"].to(dev), sc["conf"].to(dev), sc["rec"].to(dev)
        calls = {f"egr_rig_refine_f32 x{k}": (lambda k=k: hip.rig_refine(coords, conf, rec, None, None, 1.0 / HM, 1.0 / HM, THR, MIN_DET, 0.0, k))
                 for k in COUNTS}
        calls["egr_triangulate_f32"] = lambda: hip.triangulate(coords, conf, rec, None, 1.0 / HM, 1.0 / HM, THR, MIN_DET)
        graphs, keep = {}, []
        for name, fn in calls.items():
            for _ in range(3):             # warm-up: code objects loaded
                out = fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                keep.append(fn())
            graphs[name] = g
        fit = hip.rig_refine(coords, conf, rec, None, None, 1.0 / HM, 1.0 / HM, THR, MIN_DET, 0.0, 8)
        torch.cuda.synchronize()
        for g in graphs.values():
            g.replay()
        torch.cuda.synchronize()
        times = {name: [] for name in calls}
        for _ in range(a.rounds):
            for name, g in graphs.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                g.replay()
                e.record()
                e.synchronize()
                times[name].append(s.elapsed_time(e) * 1e3)          # us per call
        med = {name: statistics.median(t) for name, t in times.items()}
        per_iteration = (med["egr_rig_refine_f32 x12"] - med["egr_rig_refine_f32 x4"]) / 8.0
        row = {"pairs": B * J, "pairs_counted": int(fit[5]), "steps_of_8": int(fit[6]), "valid": bool(fit[8]),
               "calls": {name: {"median_us": round(med[name], 2), "min_us": round(min(times[name]), 2)} for name in calls},
               "per_iteration_us": round(per_iteration, 2), "outside_the_iterations_us": round(med["egr_rig_refine_f32 x4"] - 4 * per_iteration, 2),
               "iteration_over_triangulate": round(per_iteration / med["egr_triangulate_f32"], 2)}
        res["frames"][str(B)] = row
        for name in calls:
            print(f"{B:5d} frames  {name:26s} median {med[name]:9.2f} us  min {min(times[name]):9.2f} us")
        print(f"{B:5d} frames  one iteration {per_iteration:.2f} us = {row['iteration_over_triangulate']:.2f} x egr_triangulate_f32")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

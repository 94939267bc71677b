"""Time the soft-argmax launches against the arg-max kernel on the serving shape (64, 4, 15, 64, 64) -> profiles/soft_argmax_b64.json.

    python tools/soft_argmax_bench.py [--inputs 6] [--rounds 30] [--out profiles/soft_argmax_b64.json]

Four launches, one process: egr_soft_argmax_f32 (mode 0, beta 100), egr_soft_argmax_bwd_f32, decode.decode_joints_2d and
egr_argmax_rows_f32 (the yardstick: it reads what the forward reads).  Each rotates over `inputs` distinct tensors of 63 MB (6: 377 MB,
beyond the 256 MiB last-level cache; the backward writes as many gradients), the same rotation for all four.  One rotation of each launch
is captured into a hipGraph, so the kernels run back to back without the host's enqueue time between them; the four graphs are replayed
in turn, `rounds` times, each replay between two events.  Reported per launch: median and minimum over the rounds, the ratio to the
arg-max kernel in the same run, and algorithmic bytes over time."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPE = (64, 4, 15, 64, 64)
BETA = 100.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "soft_argmax_b64.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("soft_argmax_bench: needs the GPU (nothing is measured without one)")
    from egorear_amd import decode, hip
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    B, V, J, H, W = SHAPE
    rows = B * V * J
    xs, ys = torch.arange(W, device=dev).view(1, 1, W), torch.arange(H, device=dev).view(1, H, 1)
    hms, fwd, seeds = [], [], []
    for _ in range(a.inputs):      # a unit bump at a random centre plus noise: the data the decode sees, not zeros
        cx, cy = torch.rand(rows, 1, 1, device=dev, generator=gen) * (W - 1), torch.rand(rows, 1, 1, device=dev, generator=gen) * (H - 1)
        h = torch.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / 32.0) + 0.05 * torch.randn(rows, H, W, device=dev, generator=gen)
        hms.append(h.view(SHAPE).contiguous())
        fwd.append(hip.soft_argmax(hms[-1], BETA, 0))
        seeds.append(torch.randn(rows, 2, device=dev, generator=gen))
    grads = [torch.empty_like(h) for h in hms]
    map_bytes = 4.0 * rows * H * W
    launches = {
        "egr_argmax_rows_f32": (lambda i: hip.argmax_rows(hms[i], 0.5), map_bytes + 17.0 * rows),
        "egr_soft_argmax_f32": (lambda i: hip.soft_argmax(hms[i], BETA, 0, False, 0.5), map_bytes + 25.0 * rows),
        "egr_soft_argmax_bwd_f32": (lambda i: hip.soft_argmax_bwd(hms[i], fwd[i][4], fwd[i][0], fwd[i][2], seeds[i], None, BETA, 0, out=grads[i]),
                                    2.0 * map_bytes + 36.0 * rows),
        "decode_joints_2d": (lambda i: decode.decode_joints_2d(hms[i], BETA, 0.5), map_bytes + 25.0 * rows),
    }
    graphs, keep = {}, []
    for name, (fn, _) in launches.items():
        for i in range(a.inputs):      # warm-up: code objects loaded, every input touched
            fn(i)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            keep.append([fn(i) for i in range(a.inputs)])
        graphs[name] = g
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    times = {name: [] for name in launches}
    for _ in range(a.rounds):
        for name, g in graphs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            g.replay()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / a.inputs)      # us per launch
    base = statistics.median(times["egr_argmax_rows_f32"])
    targets = {"egr_soft_argmax_f32": 1.5, "egr_soft_argmax_bwd_f32": 3.0}
    res = {"shape": list(SHAPE), "beta": BETA, "mode": 0, "inputs": a.inputs, "rounds": a.rounds,
           "working_set_mb": round(a.inputs * map_bytes / 1e6, 1), "device": hip.device_arch(), "library": hip.version(),
           "method": "one rotation over the inputs per hipGraph, graphs replayed in turn, device events around each replay", "launches": {}}
    for name, (_, nbytes) in launches.items():
        med, mn = statistics.median(times[name]), min(times[name])
        row = {"median_us": round(med, 2), "min_us": round(mn, 2), "ratio_to_argmax": round(med / base, 3),
               "algorithmic_bytes": int(nbytes), "gb_per_s": round(nbytes / med / 1e3, 1)}
        if name in targets:
            row["target_ratio"] = targets[name]
            row["target_met"] = bool(med / base <= targets[name])
        res["launches"][name] = row
        print(f"{name:28s} median {med:8.2f} us  min {mn:8.2f} us  x{med / base:5.2f} of arg-max  {row['gb_per_s']:8.1f} GB/s")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""Time the volumetric fusion on the serving shape (64 frames, 4 views, 15 joints, 64 x 64 maps) -> profiles/volume_b64.json.

    python tools/volume_bench.py [--inputs 4] [--rounds 20] [--out profiles/volume_b64.json]

One process: egr_volume_fuse_f32 and egr_volume_fuse_bwd_f32 at grid 16 and grid 32 (a 40 cm cube around the triangulated pose of bumps
rendered at the projections of random points, weighted by the maps' maxima), and decode.decode_joints_3d_volumetric (soft-argmax,
triangulation, fusion: three launches) next to decode.decode_joints_3d (the first two) on the same maps.  The method is
tools/triangulate_bench.py's: each launch rotates over `inputs` distinct inputs, one rotation is captured into a hipGraph so that the
kernels run back to back without the host's enqueue time between them, the graphs are replayed in turn `rounds` times, each replay
between two device events.  Nothing here is a target: the numbers are reported as measured, with the projections per second they
amount to (pairs x grid^3 x views over the median time)."""
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
BETA, THR, MIN_DET, CUBE = 100.0, 0.5, 1e-6, 40.0
GRIDS = (16, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "volume_b64.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("volume_bench: needs the GPU (nothing is measured without one)")
    from egorear_amd import decode, hip
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    B, V, J, H, W = SHAPE
    rec = decode._ray_records("ego4view_syn", None, torch.device(dev))
    xs, ys = torch.arange(W, device=dev).view(1, 1, 1, 1, W), torch.arange(H, device=dev).view(1, 1, 1, H, 1)
    hms, coarse, seeds = [], [], []
    for _ in range(a.inputs):      # unit bumps (sigma 1) at the rig's own projections of random points, plus 0.02 noise
        r = torch.rand(B, J, 3, device=dev, generator=gen)
        pts = torch.stack((r[..., 0] * 120 - 60, r[..., 1] * 120 - 40, r[..., 2] * 135 + 15), -1)
        centre = torch.empty(B, V, J, 2, device=dev)
        for v in range(V):         # each camera on its own: flip, offset, then the W2C polynomial (un-chained)
            f = -1.0 if float(rec[v, 26]) != 0.0 else 1.0
            p = pts * torch.tensor([f, f, 1.0], device=dev) + rec[v, 27:30]
            norm = torch.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2)
            theta = torch.atan(-p[..., 2] / norm)
            rho = sum(rec[v, 5 + i] * theta ** i for i in range(12))
            centre[:, v, :, 0] = (p[..., 0] / norm * rho + rec[v, 1]) / rec[v, 3] * W
            centre[:, v, :, 1] = (p[..., 1] / norm * rho + rec[v, 2]) / rec[v, 4] * H
        h = torch.exp(-((xs - centre[..., 0, None, None]) ** 2 + (ys - centre[..., 1, None, None]) ** 2) / 2.0)
        hms.append((h + 0.02 * torch.randn(SHAPE, device=dev, generator=gen)).contiguous())
        tri, j2 = decode.decode_joints_3d(hms[-1], "ego4view_syn", None, BETA, THR, MIN_DET)
        coarse.append((j2.maxvals.contiguous(), tri.pose.contiguous(), tri.valid.view(torch.uint8).contiguous()))
        seeds.append((torch.randn(B, J, 3, device=dev, generator=gen), torch.randn(B, J, device=dev, generator=gen)))
    pairs = B * J
    map_bytes = 4.0 * B * V * J * H * W
    launches = {}
    for G in GRIDS:
        launches[f"egr_volume_fuse_f32 grid {G}"] = (
            lambda i, G=G: hip.volume_fuse(hms[i], coarse[i][0], coarse[i][1], rec, None, coarse[i][2], G, CUBE, BETA, THR),
            map_bytes + pairs * (V * 4.0 + 38.0), pairs * G ** 3 * V)
        launches[f"egr_volume_fuse_bwd_f32 grid {G}"] = (
            lambda i, G=G: hip.volume_fuse_bwd(hms[i], coarse[i][0], coarse[i][1], rec, None, coarse[i][2], seeds[i][0], seeds[i][1], G, CUBE,
                                               BETA, THR),
            2.0 * map_bytes + pairs * (V * 4.0 + 28.0), 2 * pairs * G ** 3 * V)
    launches["decode_joints_3d"] = (lambda i: decode.decode_joints_3d(hms[i], "ego4view_syn", None, BETA, THR, MIN_DET),
                                    map_bytes + 25.0 * B * V * J + pairs * (V * 16.0 + 17.0), 0)
    for G in GRIDS:
        launches[f"decode_joints_3d_volumetric grid {G}"] = (
            lambda i, G=G: decode.decode_joints_3d_volumetric(hms[i], "ego4view_syn", None, G, CUBE, BETA, BETA, THR, MIN_DET),
            2.0 * map_bytes + 25.0 * B * V * J + pairs * (V * 20.0 + 55.0), pairs * G ** 3 * V)
    ok = hip.volume_fuse(hms[0], coarse[0][0], coarse[0][1], rec, None, coarse[0][2], 16, CUBE, BETA, THR)[4]
    graphs, keep = {}, []
    for name, (fn, _, _) in launches.items():
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
            times[name].append(s.elapsed_time(e) * 1e3 / a.inputs)      # us per call
    res = {"shape": list(SHAPE), "cube_cm": CUBE, "beta": BETA, "threshold": THR, "inputs": a.inputs, "rounds": a.rounds, "pairs": pairs,
           "pairs_ok": int(ok.sum()), "device": hip.device_arch(), "library": hip.version(),
           "method": "one rotation over the inputs per hipGraph, graphs replayed in turn, device events around each replay", "launches": {}}
    for name, (_, nbytes, proj) in launches.items():
        med, mn = statistics.median(times[name]), min(times[name])
        res["launches"][name] = {"median_us": round(med, 2), "min_us": round(mn, 2), "algorithmic_bytes": int(nbytes)}
        if proj:
            res["launches"][name]["projections"] = int(proj)
            res["launches"][name]["projections_per_us_at_median"] = round(proj / med, 1)
        print(f"{name:40s} median {med:10.2f} us  min {mn:10.2f} us")
    d3 = res["launches"]["decode_joints_3d"]["median_us"]
    for G in GRIDS:
        dv = res["launches"][f"decode_joints_3d_volumetric grid {G}"]["median_us"]
        res[f"volumetric_grid_{G}_over_decode_3d"] = round(dv / d3, 2)
        print(f"decode_joints_3d_volumetric grid {G} / decode_joints_3d = {dv / d3:.2f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

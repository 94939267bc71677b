"""Time the robust decoder's launches on the serving shape (64 frames, 4 views, 15 joints) -> profiles/robust_decode_b64.json.

    python tools/robust_decode_bench.py [--inputs 6] [--rounds 30] [--out profiles/robust_decode_b64.json]

Six timings, one process: egr_peaks_f32 next to egr_soft_argmax_f32 (both read the same 63 MB of maps once), egr_consensus_f32 next to
egr_triangulate_f32 (both are latency-bound launches over the 960 (frame, joint) pairs), and the chains decode.decode_joints_3d_robust
(three launches) and decode.decode_joints_3d (two) on the same maps: (64, 4, 15, 64, 64) unit bumps at the syn rig's projections of
random points plus 0.02 noise, with a distractor bump of height 1.2 in one view per joint.  The method is tools/triangulate_bench.py's:
each launch rotates over `inputs` distinct inputs, one rotation is captured into a hipGraph so that the kernels run back to back
without the host's enqueue time between them, the graphs are replayed in turn `rounds` times, each replay between two events.  There
is no target: the numbers are reported as measured."""
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
K, RN, R, BETA, THR, TAU, MIN_VIEWS, MIN_DET = 3, 1, 2, 100.0, 0.5, 2.0, 2, 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "robust_decode_b64.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("robust_decode_bench: needs the GPU (nothing is measured without one)")
    from egorear_amd import decode, hip
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    B, V, J, H, W = SHAPE
    rec = decode._ray_records("ego4view_syn", None, torch.device(dev))
    xs, ys = torch.arange(W, device=dev).view(1, 1, 1, 1, W), torch.arange(H, device=dev).view(1, 1, 1, H, 1)
    hms, peaks, joints, agreed = [], [], [], []
    for _ in range(a.inputs):
        r = torch.rand(B, J, 3, device=dev, generator=gen)
        pts = torch.stack((r[..., 0] * 120 - 60, r[..., 1] * 120 - 40, r[..., 2] * 135 + 15), -1)
        # (each camera on its own: flip, offset, then the W2C polynomial - the triangulation's convention, un-chained)
        centre = torch.empty(B, V, J, 2, device=dev)
        for v in range(V):
            f = -1.0 if float(rec[v, 26]) != 0.0 else 1.0
            p = pts * torch.tensor([f, f, 1.0], device=dev) + rec[v, 27:30]
            norm = torch.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2)
            theta = torch.atan(-p[..., 2] / norm)
            rho = sum(rec[v, 5 + i] * theta ** i for i in range(12))
            centre[:, v, :, 0] = (p[..., 0] / norm * rho + rec[v, 1]) / rec[v, 3] * W
            centre[:, v, :, 1] = (p[..., 1] / norm * rho + rec[v, 2]) / rec[v, 4] * H
        h = torch.exp(-((xs - centre[..., 0, None, None]) ** 2 + (ys - centre[..., 1, None, None]) ** 2) / 2.0)
        # the distractor: one view per joint, at the true spot mirrored through the map's centre when that is more than 10 px away,
        # else 20 px to the side
        view = torch.randint(0, V, (B, 1, J), device=dev, generator=gen)
        spot = torch.tensor([W - 1.0, H - 1.0], device=dev) - centre
        near = (spot - centre).norm(dim=-1, keepdim=True) <= 10.0
        spot = torch.where(near, (centre + torch.tensor([20.0, 0.0], device=dev)) % torch.tensor([W - 1.0, H - 1.0], device=dev), spot)
        on = (torch.arange(V, device=dev).view(1, V, 1) == view).float()
        h = h + 1.2 * on[..., None, None] * torch.exp(-((xs - spot[..., 0, None, None]) ** 2 + (ys - spot[..., 1, None, None]) ** 2) / 2.0)
        hms.append((h + 0.02 * torch.randn(SHAPE, device=dev, generator=gen)).contiguous())
        j2 = decode.decode_joints_2d(hms[-1], BETA, THR)
        joints.append((j2.soft.contiguous(), j2.maxvals.contiguous()))
        pk = decode.find_peaks_2d(hms[-1], K, RN, R, BETA, THR)
        peaks.append(pk)
        agreed.append(decode.select_consistent(pk, "ego4view_syn", None, (H, W), TAU, MIN_VIEWS, MIN_DET))
    torch.cuda.synchronize()
    rob, con, pk = decode.decode_joints_3d_robust(hms[0], "ego4view_syn", None, K, RN, R, BETA, THR, TAU, MIN_VIEWS, MIN_DET)
    map_bytes = 4.0 * B * V * J * H * W
    rows, pairs = B * V * J, B * J
    peak_bytes, con_bytes, tri_bytes = map_bytes + rows * (16.0 * K + 4.0), pairs * (V * (16.0 * K + 16.0) + 12.0), pairs * (V * 16.0 + 17.0)
    launches = {
        "egr_peaks_f32": (lambda i: hip.find_peaks(hms[i], K, RN, R, BETA, THR), peak_bytes),
        "egr_soft_argmax_f32": (lambda i: hip.soft_argmax(hms[i], BETA, 0, False, THR), map_bytes + 25.0 * rows),
        "egr_consensus_f32": (lambda i: hip.consensus(peaks[i].coords, peaks[i].score, peaks[i].index, rec, None, 1.0 / W, 1.0 / H, TAU,
                                                      MIN_VIEWS, MIN_DET), con_bytes),
        "egr_triangulate_f32": (lambda i: hip.triangulate(agreed[i].coords, agreed[i].conf, rec, None, 1.0 / W, 1.0 / H, THR, MIN_DET),
                                tri_bytes),
        "decode_joints_3d_robust": (lambda i: decode.decode_joints_3d_robust(hms[i], "ego4view_syn", None, K, RN, R, BETA, THR, TAU,
                                                                             MIN_VIEWS, MIN_DET), peak_bytes + con_bytes + tri_bytes),
        "decode_joints_3d": (lambda i: decode.decode_joints_3d(hms[i], "ego4view_syn", None, BETA, THR, MIN_DET),
                             map_bytes + 25.0 * rows + tri_bytes),
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
            times[name].append(s.elapsed_time(e) * 1e3 / a.inputs)      # us per launch (per chain for the two chains)
    res = {"shape": list(SHAPE), "k": K, "nms_radius": RN, "refine_radius": R, "beta": BETA, "threshold": THR, "max_reproj": TAU,
           "min_views": MIN_VIEWS, "min_det_ratio": MIN_DET, "inputs": a.inputs, "rounds": a.rounds, "pairs": pairs,
           "pairs_valid": int(rob.valid.sum()), "pairs_with_four_inliers": int((con.inliers == V).sum()),
           "maps_with_two_peaks_or_more": int((pk.count >= 2).sum()), "device": hip.device_arch(), "library": hip.version(),
           "method": "one rotation over the inputs per hipGraph, graphs replayed in turn, device events around each replay", "launches": {}}
    for name, (_, nbytes) in launches.items():
        med, mn = statistics.median(times[name]), min(times[name])
        res["launches"][name] = {"median_us": round(med, 2), "min_us": round(mn, 2), "algorithmic_bytes": int(nbytes)}
        print(f"{name:28s} median {med:8.2f} us  min {mn:8.2f} us")
    L = res["launches"]
    res["peaks_over_soft_argmax"] = round(L["egr_peaks_f32"]["median_us"] / L["egr_soft_argmax_f32"]["median_us"], 3)
    res["consensus_over_triangulate"] = round(L["egr_consensus_f32"]["median_us"] / L["egr_triangulate_f32"]["median_us"], 3)
    res["robust_over_decode_3d"] = round(L["decode_joints_3d_robust"]["median_us"] / L["decode_joints_3d"]["median_us"], 3)
    print(f"peaks / soft-argmax = {res['peaks_over_soft_argmax']:.3f}, consensus / triangulate = {res['consensus_over_triangulate']:.3f}, "
          f"robust chain / decode_joints_3d = {res['robust_over_decode_3d']:.3f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

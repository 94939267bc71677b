"""Time the skeleton fit on the serving shape (64 frames, 4 views, 15 joints) -> profiles/skeleton_fit_b64.json, and measure what it
buys -> profiles/skeleton_accuracy.json.

    python tools/skeleton_fit_bench.py [--inputs 6] [--rounds 30] [--out profiles/skeleton_fit_b64.json]
                                       [--accuracy-out profiles/skeleton_accuracy.json]

Timings, one process: egr_skeleton_fit_f32 at 16 and at 48 iterations next to egr_triangulate_f32 on the same operands (all three are
latency-bound launches over the 64 frames), and the chain decode.decode_joints_3d_skeleton (three launches) next to
decode.decode_joints_3d (two) on the same maps: (64, 4, 15, 64, 64) unit bumps (sigma 1) at the syn rig's projections of random
15-joint skeletons (bones 10 to 35 cm) plus 0.02 noise.  The method is tools/robust_decode_bench.py's: each launch rotates over `inputs`
distinct inputs, one rotation is captured into a hipGraph so that the kernels run back to back without the host's enqueue time
between them, the graphs are replayed in turn `rounds` times, each replay between two events.  There is no target: the numbers are
reported as measured.

Accuracy, on the same maps with the true bone lengths, for the four views and for the front pair: the mean joint error of
decode_joints_3d, of decode_joints_3d followed by resize_skeleton, and of decode_joints_3d_skeleton (bone_weight 1, 48 iterations)."""
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
BETA, THR, MIN_DET, NOISE, BONE_WEIGHT = 100.0, 0.5, 1e-6, 0.02, 1.0


def skeletons(B, parents, gen, torch):
    """(B, J, 3) float64 poses of a tree whose bones - (J), the same in every frame - are 10 to 35 cm, inside the box the other decode
    benches draw their points from."""
    J = len(parents)
    lengths = torch.rand(J, generator=gen, dtype=torch.float64) * 25 + 10
    lengths[0] = 0.0
    lo, hi = torch.tensor([-60.0, -40.0, 15.0], dtype=torch.float64), torch.tensor([60.0, 80.0, 150.0], dtype=torch.float64)
    pts = torch.zeros(B, J, 3, dtype=torch.float64)
    r = torch.rand(B, 3, generator=gen, dtype=torch.float64)
    pts[:, 0] = torch.stack((r[:, 0] * 60 - 30, r[:, 1] * 60 - 10, r[:, 2] * 67 + 47), -1)
    for j in range(1, J):
        u = torch.randn(B, 3, generator=gen, dtype=torch.float64)
        u = u / u.norm(dim=-1, keepdim=True)
        child = pts[:, parents[j]] + lengths[j] * u
        u = torch.where((child < lo) | (child > hi), -u, u)
        pts[:, j] = pts[:, parents[j]] + lengths[j] * u
    return pts, lengths


def render(pts, rec, H, W, gen, torch):
    """(B, V, J, H, W) fp32 bumps at the projections of pts (each camera on its own: flip, offset, then the W2C polynomial)."""
    B, J, _ = pts.shape
    V = rec.shape[0]
    rec = rec.double().cpu()
    centre = torch.empty(B, V, J, 2, dtype=torch.float64)
    for v in range(V):
        f = -1.0 if float(rec[v, 26]) != 0.0 else 1.0
        p = pts * torch.tensor([f, f, 1.0], dtype=torch.float64) + rec[v, 27:30]
        norm = torch.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2)
        theta = torch.atan(-p[..., 2] / norm)
        rho = sum(rec[v, 5 + i] * theta ** i for i in range(12))
        centre[:, v, :, 0] = (p[..., 0] / norm * rho + rec[v, 1]) / rec[v, 3] * W
        centre[:, v, :, 1] = (p[..., 1] / norm * rho + rec[v, 2]) / rec[v, 4] * H
    xs, ys = torch.arange(W, dtype=torch.float64).view(1, 1, 1, 1, W), torch.arange(H, dtype=torch.float64).view(1, 1, 1, H, 1)
    h = torch.exp(-((xs - centre[..., 0, None, None]) ** 2 + (ys - centre[..., 1, None, None]) ** 2) / 2.0)
    return (h + NOISE * torch.randn(h.shape, generator=gen, dtype=torch.float64)).float().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "skeleton_fit_b64.json"))
    ap.add_argument("--accuracy-out", default=os.path.join(REPO, "profiles", "skeleton_accuracy.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("skeleton_fit_bench: needs the GPU (nothing is measured without one)")
    from egorear_amd import decode, hip
    from egorear_amd.camera import FishEyeCameraCalibratedModel
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    B, V, J, H, W = SHAPE
    parents = list(decode.HEATMAP_PARENTS_15)
    cams = [FishEyeCameraCalibratedModel("ego4view_syn", decode._PKG_CALIB, n) for n in decode._CAMERA_NAMES]
    rec = decode._ray_records(cams, None, torch.device(dev))
    hms, joints, starts, truth = [], [], [], []
    for _ in range(a.inputs):
        pts, _ = skeletons(B, parents, gen, torch)
        truth.append(pts)
        hms.append(render(pts, rec, H, W, gen, torch).to(dev))
        j2 = decode.decode_joints_2d(hms[-1], BETA, THR)
        joints.append((j2.soft.contiguous(), j2.maxvals.contiguous()))
        p3, _, _, ok = hip.triangulate(joints[-1][0], joints[-1][1], rec, None, 1.0 / W, 1.0 / H, THR, MIN_DET)
        starts.append((p3, ok))
    torch.cuda.synchronize()
    # every input has its own skeleton; the timed fits take each input's true lengths per frame
    Ls = [(t - t[:, parents]).norm(dim=-1).float().to(dev).contiguous() for t in truth]
    pairs = B * J
    map_bytes = 4.0 * B * V * J * H * W
    tri_bytes, fit_bytes = pairs * (V * 16.0 + 17.0), B * (J * (V * 12.0 + 42.0) + 16.0)
    fit = lambda i, n: hip.skeleton_fit(joints[i][0], joints[i][1], rec, None, parents, Ls[i], starts[i][0], starts[i][1], 1.0 / W, 1.0 / H, THR,
                                        MIN_DET, BONE_WEIGHT, 0.0, n)
    launches = {
        "egr_skeleton_fit_f32 (16 iterations)": (lambda i: fit(i, 16), fit_bytes),
        "egr_skeleton_fit_f32 (48 iterations)": (lambda i: fit(i, 48), fit_bytes),
        "egr_triangulate_f32": (lambda i: hip.triangulate(joints[i][0], joints[i][1], rec, None, 1.0 / W, 1.0 / H, THR, MIN_DET), tri_bytes),
        "decode_joints_3d_skeleton (16 iterations)": (lambda i: decode.decode_joints_3d_skeleton(hms[i], cams, Ls[i], iterations=16),
                                                      map_bytes + 25.0 * B * V * J + tri_bytes + fit_bytes),
        "decode_joints_3d": (lambda i: decode.decode_joints_3d(hms[i], cams, None, BETA, THR, MIN_DET), map_bytes + 25.0 * B * V * J + tri_bytes),
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
    out16, out48 = fit(0, 16), fit(0, 48)
    res = {"shape": list(SHAPE), "parents": parents, "beta": BETA, "threshold": THR, "min_det_ratio": MIN_DET, "map_noise": NOISE,
           "bone_weight": BONE_WEIGHT, "prior_weight": 0.0, "inputs": a.inputs, "rounds": a.rounds, "frames": B,
           "joints_valid": int(out48[3].sum()), "steps_kept_of_16": [int(out16[7].min()), int(out16[7].max())],
           "steps_kept_of_48": [int(out48[7].min()), int(out48[7].max())],
           "largest_grad_after_16": float(out16[6].max()), "largest_grad_after_48": float(out48[6].max()),
           "device": hip.device_arch(), "library": hip.version(),
           "method": "one rotation over the inputs per hipGraph, graphs replayed in turn, device events around each replay", "launches": {}}
    for name, (_, nbytes) in launches.items():
        med, mn = statistics.median(times[name]), min(times[name])
        res["launches"][name] = {"median_us": round(med, 2), "min_us": round(mn, 2), "algorithmic_bytes": int(nbytes)}
        print(f"{name:44s} median {med:8.2f} us  min {mn:8.2f} us")
    L = res["launches"]
    res["fit16_over_triangulate"] = round(L["egr_skeleton_fit_f32 (16 iterations)"]["median_us"] / L["egr_triangulate_f32"]["median_us"], 3)
    res["fit48_over_triangulate"] = round(L["egr_skeleton_fit_f32 (48 iterations)"]["median_us"] / L["egr_triangulate_f32"]["median_us"], 3)
    res["us_per_iteration"] = round((L["egr_skeleton_fit_f32 (48 iterations)"]["median_us"] -
                                     L["egr_skeleton_fit_f32 (16 iterations)"]["median_us"]) / 32.0, 3)
    res["skeleton_chain_over_decode_3d"] = round(L["decode_joints_3d_skeleton (16 iterations)"]["median_us"] / L["decode_joints_3d"]["median_us"], 3)
    print(f"fit(16) / triangulate = {res['fit16_over_triangulate']:.3f}, fit(48) / triangulate = {res['fit48_over_triangulate']:.3f}, "
          f"{res['us_per_iteration']:.3f} us an iteration, skeleton chain / decode_joints_3d = {res['skeleton_chain_over_decode_3d']:.3f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)

    # ---- accuracy: what the bones buy, on the same maps
    acc = {"shape": list(SHAPE), "inputs": a.inputs, "map_noise": NOISE, "bone_weight": BONE_WEIGHT, "iterations": 48, "unit": "cm",
           "bone_length": "the true lengths of every frame's skeleton", "views": {}}
    for label, views in (("four views", [0, 1, 2, 3]), ("front pair", [0, 1])):
        sums = {"decode_joints_3d": 0.0, "decode_joints_3d + resize_skeleton": 0.0, "decode_joints_3d_skeleton": 0.0}
        worst = dict.fromkeys(sums, 0.0)
        count = 0
        for i in range(a.inputs):
            hm = hms[i][:, views].contiguous()
            sub = [cams[v] for v in views]
            fit3, tri, _ = decode.decode_joints_3d_skeleton(hm, sub, Ls[i], bone_weight=BONE_WEIGHT, iterations=48)
            moved = decode.resize_skeleton(tri.pose, tri.valid, Ls[i])
            ok = (tri.valid & fit3.valid).cpu()
            for name, pose in (("decode_joints_3d", tri.pose), ("decode_joints_3d + resize_skeleton", moved), ("decode_joints_3d_skeleton", fit3.pose)):
                err = (pose.double().cpu() - truth[i]).norm(dim=-1)[ok]
                sums[name] += float(err.sum())
                worst[name] = max(worst[name], float(err.max()))
            count += int(ok.sum())
        acc["views"][label] = {"joints": count, "mean_error": {k: round(v / count, 4) for k, v in sums.items()},
                               "largest_error": {k: round(v, 4) for k, v in worst.items()}}
        print(label, acc["views"][label])
    with open(a.accuracy_out, "w") as f:
        json.dump(acc, f, indent=1)
        f.write("\n")
    print("wrote", a.accuracy_out)


if __name__ == "__main__":
    main()

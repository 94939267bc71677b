"""Time the temporal trajectory smoother -> profiles/trajectory_b64.json, and measure what it buys on a rendered clip ->
profiles/trajectory_accuracy.json.

    python tools/trajectory_bench.py [--inputs 4] [--rounds 30] [--out profiles/trajectory_b64.json]
                                     [--accuracy-out profiles/trajectory_accuracy.json]

Timings, one process, J = 15: egr_trajectory_smooth_f32 in its plain form and with huber 1 cm, K = 4, and egr_trajectory_smooth_bwd_f32,
on clips of (N, T) = (1, 64), (1, 1024) and (64, 64) - random walks with 30 % of the frames dropped - and the chain decode.decode_clip_3d
(three launches) next to decode.decode_joints_3d (two) on the same 64 frames of (4, 15, 64, 64) maps.  The method is
tools/skeleton_fit_bench.py's: each launch rotates over `inputs` distinct inputs, one rotation is captured into a hipGraph so that the
kernels run back to back without the host's enqueue time between them, the graphs are replayed in turn `rounds` times, each replay
between two events.  The kernel is bound by the latency of a dependent fp64 chain of T steps per sweep (2 (K + 1) sweeps), so the time per
step and sweep is reported next to each launch.  There is no target: the numbers are reported as measured.

Accuracy: one clip of T = 64 frames of a moving 15-joint skeleton, rendered as sigma-1 bumps (tests/fisheye_statement.py) at the syn
rig's projections with 0.3 px of noise on every bump's centre; 15 % of the (frame, joint) pairs keep one view only, which the
triangulation gives up; 8 pairs are rendered 40 cm off in every view for one frame (a consistent glitch, as a left / right swap is).
For per-frame decode_joints_3d, the plain smoother and the Huber smoother (1 cm, K = 4): the mean joint error, the mean
|x_{t+1} - 2 x_t + x_{t-1}| and the share of (frame, joint) pairs with a valid pose."""
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

J = 15
CLIPS = ((1, 64), (1, 1024), (64, 64))
ACCEL, VEL, HUBER, K, MAX_GAP = 10.0, 0.0, 1.0, 4, 8
BETA, THR, MIN_DET = 100.0, 0.5, 1e-6
PIXEL_NOISE, DROPPED, GLITCHES, GLITCH_CM = 0.3, 0.15, 8, 40.0


def random_clip(N, T, gen, torch):
    """(pose (N, T, J, 3) fp32, weight (N, T, J) fp32 with 30 % zeros): a random walk of 1 cm steps about a place in the working volume."""
    place = torch.rand(N, 1, J, 3, generator=gen) * 100.0 - 50.0
    pose = place + torch.randn(N, T, J, 3, generator=gen).cumsum(1) + 0.5 * torch.randn(N, T, J, 3, generator=gen)
    weight = 0.5 + 0.5 * torch.rand(N, T, J, generator=gen)
    weight[torch.rand(N, T, J, generator=gen) < 0.3] = 0.0
    return pose.contiguous(), weight.contiguous()


def moving_skeleton(T, parents, gen, torch):
    """(T, J, 3) float64: a tree with bones of 10 to 30 cm whose root wanders by a few cm while the body turns about the vertical axis
    and every joint swings a little - well inside what the four cameras see."""
    import math
    n = len(parents)
    rest = torch.zeros(n, 3, dtype=torch.float64)
    for j in range(1, n):
        u = torch.randn(3, generator=gen, dtype=torch.float64)
        rest[j] = rest[parents[j]] + (10.0 + 20.0 * float(torch.rand(1, generator=gen))) * u / u.norm()
    rest = rest.clamp(-35.0, 35.0)
    t = torch.arange(T, dtype=torch.float64)
    ang = 0.6 * torch.sin(2.0 * math.pi * t / 90.0)
    c, s = torch.cos(ang).view(T, 1), torch.sin(ang).view(T, 1)
    turned = torch.stack((c * rest[:, 0] - s * rest[:, 1], s * rest[:, 0] + c * rest[:, 1], rest[:, 2].expand(T, n)), -1)
    root = torch.stack((8.0 * torch.sin(2.0 * math.pi * t / 50.0), 20.0 + 6.0 * torch.cos(2.0 * math.pi * t / 70.0),
                        80.0 + 5.0 * torch.sin(2.0 * math.pi * t / 40.0)), -1).view(T, 1, 3)
    phase = 2.0 * math.pi * torch.rand(1, n, 3, generator=gen, dtype=torch.float64)
    swing = 2.0 * torch.sin(2.0 * math.pi * t.view(T, 1, 1) / 30.0 + phase)
    return root + turned + swing


def rendered_clip(T, parents, rec, gen, torch, FS):
    """The accuracy clip (tools/ray_track_bench.py renders the same one): truth (T, J, 3) float64, maps (T, 4, J, HM, HM) fp32 on the
    host, glitch and dropped (T, J) bool - sigma-1 bumps at the syn rig's projections with PIXEL_NOISE on every centre, GLITCHES pairs
    rendered GLITCH_CM off in every view, DROPPED of the other pairs keeping one view."""
    truth = moving_skeleton(T, parents, gen, torch)
    shown = truth.clone()
    glitch = torch.zeros(T, J, dtype=torch.bool)
    while int(glitch.sum()) < GLITCHES:
        t, j = int(torch.randint(2, T - 2, (1,), generator=gen)), int(torch.randint(0, J, (1,), generator=gen))
        if not bool(glitch[max(t - 2, 0):t + 3, j].any()):
            glitch[t, j] = True
            u = torch.randn(3, generator=gen, dtype=torch.float64)
            u[2] = 0.0                                                                 # (sideways: it stays in front of the cameras)
            shown[t, j] += GLITCH_CM * u / u.norm()
    x, y, _ = FS.heatmap_coords(shown.unsqueeze(1).unsqueeze(3), rec, None, FS.HM, FS.HM)
    x = x.squeeze(-1) + PIXEL_NOISE * torch.randn(T, 4, J, generator=gen, dtype=torch.float64)
    y = y.squeeze(-1) + PIXEL_NOISE * torch.randn(T, 4, J, generator=gen, dtype=torch.float64)
    maps = FS.render(x, y, FS.HM, FS.HM).float()
    dropped = (torch.rand(T, J, generator=gen) < DROPPED) & ~glitch
    for t, j in dropped.nonzero().tolist():
        keep = int(torch.randint(0, 4, (1,), generator=gen))
        for v in range(4):
            if v != keep:
                maps[t, v, j] = 0.0
    return truth, maps, glitch, dropped


def graph_times(launches, inputs, rounds, torch):
    graphs, keep = {}, []
    for name, fn in launches.items():
        for i in range(inputs):        # warm-up: code objects loaded, every input touched
            fn(i)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            keep.append([fn(i) for i in range(inputs)])
        graphs[name] = g
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    times = {name: [] for name in launches}
    for _ in range(rounds):
        for name, g in graphs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            g.replay()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / inputs)        # us per launch (per chain for the chains)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trajectory_b64.json"))
    ap.add_argument("--accuracy-out", default=os.path.join(REPO, "profiles", "trajectory_accuracy.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("trajectory_bench: needs the GPU (nothing is measured without one)")
    import fisheye_statement as FS
    from egorear_amd import decode, hip
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    cams = FS.rig()
    rec = FS.records(cams)
    parents = list(decode.HEATMAP_PARENTS_15)

    # ---- the rendered clip (also the chain's maps)
    T = 64
    truth, maps, glitch, dropped = rendered_clip(T, parents, rec, gen, torch, FS)
    maps = maps.contiguous().to(dev)
    chain_maps = [maps] + [(maps + 0.01 * torch.randn(maps.shape, generator=gen).to(dev)).contiguous() for _ in range(a.inputs - 1)]

    # ---- timings
    launches, meta = {}, {}
    for N, T_ in CLIPS:
        data = [tuple(t.to(dev) for t in random_clip(N, T_, gen, torch)) for _ in range(a.inputs)]
        grads = [torch.randn(N, T_, J, 3, generator=gen).to(dev) for _ in range(a.inputs)]
        tag = f"N {N}, T {T_}"
        launches[f"egr_trajectory_smooth_f32 plain ({tag})"] = (
            lambda i, d=data: hip.trajectory_smooth(d[i][0], d[i][1], None, VEL, ACCEL, 0.0, 0, MAX_GAP))
        launches[f"egr_trajectory_smooth_f32 huber K {K} ({tag})"] = (
            lambda i, d=data: hip.trajectory_smooth(d[i][0], d[i][1], None, VEL, ACCEL, HUBER, K, MAX_GAP))
        launches[f"egr_trajectory_smooth_bwd_f32 ({tag})"] = (
            lambda i, d=data, g=grads: hip.trajectory_smooth_bwd(d[i][0], d[i][1], None, g[i], VEL, ACCEL))
        meta[f"egr_trajectory_smooth_f32 plain ({tag})"] = (N, T_, 2)
        meta[f"egr_trajectory_smooth_f32 huber K {K} ({tag})"] = (N, T_, 2 * (K + 1))
        meta[f"egr_trajectory_smooth_bwd_f32 ({tag})"] = (N, T_, 2)
    launches["decode_clip_3d (T 64, plain)"] = lambda i: decode.decode_clip_3d(chain_maps[i], cams, None, BETA, THR, MIN_DET, None, ACCEL, VEL)
    launches[f"decode_clip_3d (T 64, huber K {K})"] = lambda i: decode.decode_clip_3d(chain_maps[i], cams, None, BETA, THR, MIN_DET, None, ACCEL,
                                                                                     VEL, HUBER, K)
    launches["decode_joints_3d (64 frames)"] = lambda i: decode.decode_joints_3d(chain_maps[i], cams, None, BETA, THR, MIN_DET)
    times = graph_times(launches, a.inputs, a.rounds, torch)
    res = {"joints": J, "accel_weight": ACCEL, "vel_weight": VEL, "huber_cm": HUBER, "reweights": K, "max_gap": MAX_GAP, "dropped_frames": 0.3,
           "chain_maps": [T, 4, J, FS.HM, FS.HM], "inputs": a.inputs, "rounds": a.rounds, "device": hip.device_arch(), "library": hip.version(),
           "method": "one rotation over the inputs per hipGraph, graphs replayed in turn, device events around each replay", "launches": {}}
    for name in launches:
        med, mn = statistics.median(times[name]), min(times[name])
        entry = {"median_us": round(med, 2), "min_us": round(mn, 2)}
        if name in meta:
            N, T_, sweeps = meta[name]
            entry.update(tracks=N * J, waves=(N * J + 63) // 64, sweeps=sweeps, ns_per_step_and_sweep=round(med * 1e3 / (T_ * sweeps), 2))
        res["launches"][name] = entry
        print(f"{name:56s} median {med:9.2f} us  min {mn:9.2f} us" + (f"  {entry['ns_per_step_and_sweep']:8.2f} ns a step and sweep" if name in meta else ""))
    L = res["launches"]
    res["clip_chain_over_decode_3d"] = round(L["decode_clip_3d (T 64, plain)"]["median_us"] / L["decode_joints_3d (64 frames)"]["median_us"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)

    # ---- accuracy: what the time axis buys, on the rendered clip
    per_frame, _ = decode.decode_joints_3d(maps, cams, None, BETA, THR, MIN_DET)
    _, plain = decode.decode_clip_3d(maps, cams, None, BETA, THR, MIN_DET, None, ACCEL, VEL, 0.0, 0, MAX_GAP)
    _, robust = decode.decode_clip_3d(maps, cams, None, BETA, THR, MIN_DET, None, ACCEL, VEL, HUBER, K, MAX_GAP)
    torch.cuda.synchronize()

    def figures(pose, valid):
        pose, valid = pose.double().cpu(), valid.cpu()
        err = (pose - truth).norm(dim=-1)
        acc = (pose[2:] - 2.0 * pose[1:-1] + pose[:-2]).norm(dim=-1)
        run = valid[2:] & valid[1:-1] & valid[:-2]
        return {"mean_error_cm": round(float(err[valid].mean()), 4), "largest_error_cm": round(float(err[valid].max()), 4),
                "mean_error_at_glitches_cm": round(float(err[glitch & valid].mean()), 4) if bool((glitch & valid).any()) else None,
                "mean_error_in_dropped_pairs_cm": round(float(err[dropped & valid].mean()), 4) if bool((dropped & valid).any()) else None,
                "mean_second_difference_cm": round(float(acc[run].mean()), 4), "valid_share": round(float(valid.float().mean()), 4)}

    acc = {"clip": [T, 4, J, FS.HM, FS.HM], "unit": "cm", "pixel_noise": PIXEL_NOISE, "dropped_pairs": int(dropped.sum()), "glitches": GLITCHES,
           "glitch_cm": GLITCH_CM, "accel_weight": ACCEL, "vel_weight": VEL, "huber_cm": HUBER, "reweights": K, "max_gap": MAX_GAP,
           "truth_mean_second_difference_cm": round(float((truth[2:] - 2.0 * truth[1:-1] + truth[:-2]).norm(dim=-1).mean()), 4),
           "second_difference": "mean |x[t+1] - 2 x[t] + x[t-1]| over the triples of valid frames",
           "methods": {"decode_joints_3d (per frame)": figures(per_frame.pose, per_frame.valid),
                       "decode_clip_3d (plain)": figures(plain.pose, plain.valid),
                       f"decode_clip_3d (huber {HUBER} cm, K {K})": figures(robust.pose, robust.valid)}}
    for name, fig in acc["methods"].items():
        print(name, fig)
    with open(a.accuracy_out, "w") as f:
        json.dump(acc, f, indent=1)
        f.write("\n")
    print("wrote", a.accuracy_out)


if __name__ == "__main__":
    main()

"""Time the ray-space clip smoother -> profiles/ray_track_b64.json, and measure what fitting the rays directly buys on the rendered clip
of tools/trajectory_bench.py -> profiles/ray_track_accuracy.json.

    python tools/ray_track_bench.py [--inputs 4] [--rounds 30] [--out profiles/ray_track_b64.json]
                                    [--accuracy-out profiles/ray_track_accuracy.json]

Timings, one process, J = 15, V = 4: egr_ray_track_f32 (its two kernels) in its plain form and with huber 1 cm, K = 4, on clips of
(N, T) = (1, 64), (64, 64) and (1, 1024) - random walks seen by the syn rig, 30 % of the rays dropped - next to
egr_trajectory_smooth_f32 at the same (N, T, J), and the chain decode.decode_clip_3d_rays (soft-argmax + the fit) next to
decode.decode_clip_3d (soft-argmax + triangulation + smoother) on the same 64 frames of (4, 15, 64, 64) maps.  The method is
tools/trajectory_bench.py's (its graph_times): each launch rotates over `inputs` distinct inputs, one rotation is captured into a
hipGraph, the graphs are replayed in turn `rounds` times, each replay between two events.  Both kernels are bound by the latency of a
dependent fp64 chain of T steps per sweep, so the time per step and sweep is reported next to each launch, and the ratio of the two.
There is no target: the numbers are reported as measured.

Accuracy: the rendered clip of tools/trajectory_bench.py (T = 64, 0.3 px of noise, 15 % of the pairs down to one view, 8 pairs rendered
40 cm off in every view for a frame).  decode_clip_3d against decode_clip_3d_rays, plain and Huber (1 cm, K = 4), with the four views
and with the front pair alone: the mean joint error over the valid poses, at the glitches, in the pairs one camera sees, and the
share of (frame, joint) pairs with a valid pose - at the default accel_weight, then the mean errors of both over a sweep of it, and `range_bias`: the pull toward the
rig that explains the sweep, measured on the float64 statements."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

J, V = 15, 4
CLIPS = ((1, 64), (64, 64), (1, 1024))
ACCEL, VEL, HUBER, K, MAX_GAP = 10.0, 0.0, 1.0, 4, 8
BETA, THR, MIN_DET = 100.0, 0.5, 1e-6
SWEEP = (0.01, 0.1, 1.0, 10.0, 100.0)                   # accel_weight, both methods (accuracy only)


def random_clip(N, T, rec, gen, torch, FS):
    """(coords (N, T, V, J, 2) fp32 in heat-map pixels, conf (N, T, V, J) fp32 with 30 % of the rays at 0, pose (N, T, J, 3) fp32 and
    weight (N, T, J) fp32 for the scalar smoother): random walks of 0.3 cm steps about places in the working volume, projected."""
    place = FS.random_points(N, J, gen).unsqueeze(1)
    pose = place + 0.3 * torch.randn(N, T, J, 3, generator=gen, dtype=torch.float64).cumsum(1)
    coords = FS.project(pose.view(N * T, J, 3), rec, None, 1.0 / FS.HM, 1.0 / FS.HM).view(N, T, V, J, 2)
    coords = coords + 0.3 * torch.randn(N, T, V, J, 2, generator=gen, dtype=torch.float64)
    conf = 0.5 + 0.5 * torch.rand(N, T, V, J, generator=gen)
    conf[torch.rand(N, T, V, J, generator=gen) < 0.3] = 0.0
    weight = 0.5 + 0.5 * torch.rand(N, T, J, generator=gen)
    weight[torch.rand(N, T, J, generator=gen) < 0.3] = 0.0
    return coords.float().contiguous(), conf.contiguous(), (pose + 0.5 * torch.randn(N, T, J, 3, generator=gen)).float().contiguous(), weight.contiguous()


def range_bias(torch, FS):
    """Why the ray fit loses as the track stiffens, on the float64 statements (CPU): 15 joints on straight lines, T = 64, the front
    pair, every ray used, 0.3 px of noise - per accel_weight the mean error and the mean of |x| - |truth| of the ray-fitted track and of
    the triangulated points, smoothed.  The ray distance in cm is smaller nearer the rig; a track can follow that, a frame cannot."""
    import ray_track_statement as RS
    import trajectory_statement as TS
    g = torch.Generator().manual_seed(3)
    T, views = 64, 2
    rec = FS.records(FS.rig()[:views])
    vel = 0.3 * torch.randn(1, J, 3, generator=g, dtype=torch.float64)
    t = torch.arange(T, dtype=torch.float64).view(1, T, 1, 1) - (T - 1) / 2
    truth = FS.random_points(1, J, g).unsqueeze(1) + vel.unsqueeze(1) * t
    sx = sy = 1.0 / FS.HM
    coords = FS.project(truth.view(T, J, 3), rec, None, sx, sy).view(1, T, views, J, 2)
    coords = coords + 0.3 * torch.randn(1, T, views, J, 2, generator=g, dtype=torch.float64)
    conf = torch.full((1, T, views, J), 0.9, dtype=torch.float64)
    tri, _, _, ok = FS.statement(coords.view(T, views, J, 2), conf.view(T, views, J), rec, None, sx, sy)
    far = truth.norm(dim=-1)
    rows = {}
    for accel in (0.01, 1.0, 100.0, 10000.0):
        fit = RS.fit(coords, conf, rec, None, sx, sy, lv=0.0, la=accel)["pose"]
        smooth = TS.smooth(tri.view(1, T, J, 3), None, ok.view(1, T, J), 0.0, accel)["pose"]
        rows[f"accel_weight {accel}"] = {
            name: {"mean_error_cm": round(float((x - truth).norm(dim=-1).mean()), 4), "mean_range_bias_cm": round(float((x.norm(dim=-1) - far).mean()), 4)}
            for name, x in (("rays fitted", fit), ("triangulated, smoothed", smooth))}
        print("noisy lines, front pair | accel_weight", accel, rows[f"accel_weight {accel}"])
    return {"scene": "15 joints on straight lines, T 64, front pair, every ray used, 0.3 px noise; float64 statements on the CPU",
            "per_frame_triangulation_range_bias_cm": round(float((tri.norm(dim=-1) - far[0]).mean()), 4), "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ray_track_b64.json"))
    ap.add_argument("--accuracy-out", default=os.path.join(REPO, "profiles", "ray_track_accuracy.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ray_track_bench: needs the GPU (nothing is measured without one)")
    import fisheye_statement as FS
    import trajectory_bench as TB
    from egorear_amd import decode, hip
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    cams = FS.rig()
    rec = FS.records(cams)
    parents = list(decode.HEATMAP_PARENTS_15)

    # ---- the rendered clip (also the chains' maps): the first draws of the generator, as in tools/trajectory_bench.py
    T = 64
    truth, maps, glitch, dropped = TB.rendered_clip(T, parents, rec, gen, torch, FS)
    maps = maps.contiguous().to(dev)
    chain_maps = [maps] + [(maps + 0.01 * torch.randn(maps.shape, generator=gen).to(dev)).contiguous() for _ in range(a.inputs - 1)]

    # ---- timings
    cam_rec = rec.to(dev)
    sx = sy = 1.0 / FS.HM
    launches, meta = {}, {}
    for N, T_ in CLIPS:
        data = [tuple(t.to(dev) for t in random_clip(N, T_, rec, gen, torch, FS)) for _ in range(a.inputs)]
        tag = f"N {N}, T {T_}"
        launches[f"egr_ray_track_f32 plain ({tag})"] = (
            lambda i, d=data: hip.ray_track(d[i][0], d[i][1], cam_rec, None, sx, sy, THR, VEL, ACCEL, 0.0, 0, MAX_GAP))
        launches[f"egr_ray_track_f32 huber K {K} ({tag})"] = (
            lambda i, d=data: hip.ray_track(d[i][0], d[i][1], cam_rec, None, sx, sy, THR, VEL, ACCEL, HUBER, K, MAX_GAP))
        launches[f"egr_trajectory_smooth_f32 plain ({tag})"] = (
            lambda i, d=data: hip.trajectory_smooth(d[i][2], d[i][3], None, VEL, ACCEL, 0.0, 0, MAX_GAP))
        launches[f"egr_trajectory_smooth_f32 huber K {K} ({tag})"] = (
            lambda i, d=data: hip.trajectory_smooth(d[i][2], d[i][3], None, VEL, ACCEL, HUBER, K, MAX_GAP))
        for kind in ("egr_ray_track_f32", "egr_trajectory_smooth_f32"):
            meta[f"{kind} plain ({tag})"] = (N, T_, 2)
            meta[f"{kind} huber K {K} ({tag})"] = (N, T_, 2 * (K + 1))
    launches["decode_clip_3d_rays (T 64, plain)"] = lambda i: decode.decode_clip_3d_rays(chain_maps[i], cams, None, BETA, THR, ACCEL, VEL)
    launches[f"decode_clip_3d_rays (T 64, huber K {K})"] = lambda i: decode.decode_clip_3d_rays(chain_maps[i], cams, None, BETA, THR, ACCEL, VEL,
                                                                                               HUBER, K)
    launches["decode_clip_3d (T 64, plain)"] = lambda i: decode.decode_clip_3d(chain_maps[i], cams, None, BETA, THR, MIN_DET, None, ACCEL, VEL)
    launches[f"decode_clip_3d (T 64, huber K {K})"] = lambda i: decode.decode_clip_3d(chain_maps[i], cams, None, BETA, THR, MIN_DET, None, ACCEL,
                                                                                     VEL, HUBER, K)
    times = TB.graph_times(launches, a.inputs, a.rounds, torch)
    res = {"joints": J, "views": V, "accel_weight": ACCEL, "vel_weight": VEL, "huber_cm": HUBER, "reweights": K, "max_gap": MAX_GAP,
           "dropped_rays": 0.3, "chain_maps": [T, 4, J, FS.HM, FS.HM], "inputs": a.inputs, "rounds": a.rounds, "device": hip.device_arch(),
           "library": hip.version(),
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
    res["ray_track_over_trajectory_smooth"] = {
        f"{form} (N {N}, T {T_})": round(L[f"egr_ray_track_f32 {form} (N {N}, T {T_})"]["median_us"] /
                                        L[f"egr_trajectory_smooth_f32 {form} (N {N}, T {T_})"]["median_us"], 3)
        for N, T_ in CLIPS for form in ("plain", f"huber K {K}")}
    res["rays_chain_over_clip_chain"] = {form: round(L[f"decode_clip_3d_rays (T 64, {form})"]["median_us"] /
                                                     L[f"decode_clip_3d (T 64, {form})"]["median_us"], 3) for form in ("plain", f"huber K {K}")}
    print("ray track / scalar smoother:", res["ray_track_over_trajectory_smooth"])
    print("rays chain / clip chain:", res["rays_chain_over_clip_chain"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)

    # ---- accuracy: the rays fitted directly against triangulate-then-smooth, on the rendered clip
    def figures(pose, valid):
        pose, valid = pose.double().cpu(), valid.cpu()
        err = (pose - truth).norm(dim=-1)
        mean = lambda m: round(float(err[m & valid].mean()), 4) if bool((m & valid).any()) else None
        return {"mean_error_cm": mean(torch.ones_like(valid)), "largest_error_cm": round(float(err[valid].max()), 4),
                "mean_error_at_glitches_cm": mean(glitch), "mean_error_in_one_view_pairs_cm": mean(dropped),
                "mean_error_elsewhere_cm": mean(~glitch & ~dropped), "valid_share": round(float(valid.float().mean()), 4)}

    acc = {"clip": [T, 4, J, FS.HM, FS.HM], "unit": "cm", "pixel_noise": TB.PIXEL_NOISE, "one_view_pairs": int(dropped.sum()), "glitches": TB.GLITCHES,
           "glitch_cm": TB.GLITCH_CM, "accel_weight": ACCEL, "vel_weight": VEL, "huber_cm": HUBER, "reweights": K, "max_gap": MAX_GAP, "rigs": {}}
    for rig, views in (("four views", 4), ("front pair", 2)):
        hm, cc = maps[:, :views].contiguous(), cams[:views]
        methods = {}
        for form, huber, k in (("plain", 0.0, 0), (f"huber {HUBER} cm, K {K}", HUBER, K)):
            _, old = decode.decode_clip_3d(hm, cc, None, BETA, THR, MIN_DET, None, ACCEL, VEL, huber, k, MAX_GAP)
            _, new = decode.decode_clip_3d_rays(hm, cc, None, BETA, THR, ACCEL, VEL, huber, k, MAX_GAP)
            torch.cuda.synchronize()
            methods[f"decode_clip_3d ({form})"] = figures(old.pose, old.valid)
            methods[f"decode_clip_3d_rays ({form})"] = figures(new.pose, new.valid)
        acc["rigs"][rig] = methods
        for name, fig in methods.items():
            print(rig, "|", name, fig)
        # the two data terms weigh a frame differently - 1 a frame there, the rays' own normal equations here, a few hundredths along
        # rays that are nearly parallel - so one accel_weight is not the same amount of smoothing in both: each method over a sweep of it
        sweep = {}
        for accel in SWEEP:
            row = {}
            for form, huber, k in (("plain", 0.0, 0), (f"huber {HUBER} cm, K {K}", HUBER, K)):
                _, old = decode.decode_clip_3d(hm, cc, None, BETA, THR, MIN_DET, None, accel, VEL, huber, k, MAX_GAP)
                _, new = decode.decode_clip_3d_rays(hm, cc, None, BETA, THR, accel, VEL, huber, k, MAX_GAP)
                torch.cuda.synchronize()
                for name, track in ((f"decode_clip_3d ({form})", old), (f"decode_clip_3d_rays ({form})", new)):
                    fig = figures(track.pose, track.valid)
                    row[name] = {key: fig[key] for key in ("mean_error_cm", "mean_error_at_glitches_cm", "mean_error_in_one_view_pairs_cm")}
            sweep[f"accel_weight {accel}"] = row
            print(rig, "| accel_weight", accel, {name: fig["mean_error_cm"] for name, fig in row.items()})
        acc["accel_weight_sweep"] = dict(acc.get("accel_weight_sweep", {}), **{rig: sweep})
    acc["range_bias_on_noisy_lines"] = range_bias(torch, FS)
    with open(a.accuracy_out, "w") as f:
        json.dump(acc, f, indent=1)
        f.write("\n")
    print("wrote", a.accuracy_out)


if __name__ == "__main__":
    main()

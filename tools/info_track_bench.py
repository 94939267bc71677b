"""Time the information-weighted clip smoother -> profiles/info_track_b64.json, and measure what the 3 x 3 weights buy on the rendered clip
of tools/trajectory_bench.py -> profiles/info_track_accuracy.json.

    python tools/info_track_bench.py [--inputs 4] [--rounds 30] [--out profiles/info_track_b64.json]
                                     [--accuracy-out profiles/info_track_accuracy.json]

Timings, one process, J = 15, V = 4: egr_joint_info_f32 and egr_info_track_f32 (plain, and huber 2 px with K = 4) on the clips of
tools/ray_track_bench.py - (N, T) = (1, 64), (64, 64) and (1, 1024), random walks seen by the syn rig, 30 % of the frames dropped -
next to egr_trajectory_smooth_f32 and egr_ray_track_f32 at the same (N, T, J) in the same run, with the ratios, and the chain
decode.decode_clip_3d_info (five launches) next to decode.decode_clip_3d (three) on the same 64 frames of (4, 15, 64, 64) maps.  The
method is tools/trajectory_bench.py's graph_times.  There is no target: the numbers are reported as measured.

Accuracy: the rendered clip of tools/trajectory_bench.py (T = 64, 0.3 px of noise, 15 % of the pairs down to one view, 8 pairs rendered
40 cm off in every view for a frame), the four views and the front pair.  decode_clip_3d, decode_clip_3d_rays, decode_clip_3d_info and
the variant of the last with the matrices taken at the triangulated points instead of the smoothed track, plain and Huber, over a sweep
of accel_weight (each smoother's own: the data terms have different units) - the mean joint error over the valid poses and at the
glitches - then best against best and at the defaults."""
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
ACCEL, VEL, HUBER_CM, HUBER_PX, K, MAX_GAP = 10.0, 0.0, 1.0, 2.0, 4, 8
BETA, THR, MIN_DET = 100.0, 0.5, 1e-6
# accel_weight: the five decades the other clip tools sweep and two more - the scalar smoother's best on the front pair lies past 100
SWEEP = (0.01, 0.1, 1.0, 10.0, 100.0, 1000.0, 10000.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "info_track_b64.json"))
    ap.add_argument("--accuracy-out", default=os.path.join(REPO, "profiles", "info_track_accuracy.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("info_track_bench: needs the GPU (nothing is measured without one)")
    import fisheye_statement as FS
    import ray_track_bench as RB
    import trajectory_bench as TB
    from egorear_amd import decode, hip
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    cams = FS.rig()
    rec = FS.records(cams)
    parents = list(decode.HEATMAP_PARENTS_15)
    info_accel = decode.INFO_ACCEL_WEIGHT

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
        data = []
        for _ in range(a.inputs):
            coords, conf, pose, weight = (t.to(dev) for t in RB.random_clip(N, T_, rec, gen, torch, FS))
            info = hip.joint_info(pose.view(N * T_, J, 3), conf.view(N * T_, V, J), cam_rec, None, sx, sy, THR, MIN_DET)[0].view(N, T_, J, 6)
            data.append((coords, conf, pose, weight, info.contiguous(), (weight > 0).to(torch.uint8).contiguous()))
        tag = f"N {N}, T {T_}"
        launches[f"egr_joint_info_f32 ({tag})"] = (
            lambda i, d=data, B=N * T_: hip.joint_info(d[i][2].view(B, J, 3), d[i][1].view(B, V, J), cam_rec, None, sx, sy, THR, MIN_DET))
        launches[f"egr_info_track_f32 plain ({tag})"] = lambda i, d=data: hip.info_track(d[i][2], d[i][4], d[i][5], VEL, info_accel, 0.0, 0, MAX_GAP)
        launches[f"egr_info_track_f32 huber K {K} ({tag})"] = (
            lambda i, d=data: hip.info_track(d[i][2], d[i][4], d[i][5], VEL, info_accel, HUBER_PX, K, MAX_GAP))
        launches[f"egr_trajectory_smooth_f32 plain ({tag})"] = lambda i, d=data: hip.trajectory_smooth(d[i][2], d[i][3], None, VEL, ACCEL, 0.0, 0, MAX_GAP)
        launches[f"egr_trajectory_smooth_f32 huber K {K} ({tag})"] = (
            lambda i, d=data: hip.trajectory_smooth(d[i][2], d[i][3], None, VEL, ACCEL, HUBER_CM, K, MAX_GAP))
        launches[f"egr_ray_track_f32 plain ({tag})"] = lambda i, d=data: hip.ray_track(d[i][0], d[i][1], cam_rec, None, sx, sy, THR, VEL, ACCEL, 0.0, 0, MAX_GAP)
        launches[f"egr_ray_track_f32 huber K {K} ({tag})"] = (
            lambda i, d=data: hip.ray_track(d[i][0], d[i][1], cam_rec, None, sx, sy, THR, VEL, ACCEL, HUBER_CM, K, MAX_GAP))
        for kind in ("egr_info_track_f32", "egr_trajectory_smooth_f32", "egr_ray_track_f32"):
            meta[f"{kind} plain ({tag})"] = (N, T_, 2)
            meta[f"{kind} huber K {K} ({tag})"] = (N, T_, 2 * (K + 1))
    launches["decode_clip_3d_info (T 64, plain)"] = lambda i: decode.decode_clip_3d_info(chain_maps[i], cams, None, BETA, THR, MIN_DET, ACCEL, info_accel, VEL)
    launches[f"decode_clip_3d_info (T 64, huber K {K})"] = lambda i: decode.decode_clip_3d_info(chain_maps[i], cams, None, BETA, THR, MIN_DET, ACCEL,
                                                                                               info_accel, VEL, HUBER_PX, K)
    launches["decode_clip_3d (T 64, plain)"] = lambda i: decode.decode_clip_3d(chain_maps[i], cams, None, BETA, THR, MIN_DET, None, ACCEL, VEL)
    launches[f"decode_clip_3d (T 64, huber K {K})"] = lambda i: decode.decode_clip_3d(chain_maps[i], cams, None, BETA, THR, MIN_DET, None, ACCEL,
                                                                                     VEL, HUBER_CM, K)
    times = TB.graph_times(launches, a.inputs, a.rounds, torch)
    res = {"joints": J, "views": V, "info_accel_weight": info_accel, "accel_weight": ACCEL, "vel_weight": VEL, "huber_px": HUBER_PX,
           "huber_cm": HUBER_CM, "reweights": K, "max_gap": MAX_GAP, "dropped_frames": 0.3, "chain_maps": [T, 4, J, FS.HM, FS.HM], "inputs": a.inputs,
           "rounds": a.rounds, "device": hip.device_arch(), "library": hip.version(),
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
    ratio = lambda top, bottom: round(L[top]["median_us"] / L[bottom]["median_us"], 3)
    forms = ("plain", f"huber K {K}")
    res["info_track_over_trajectory_smooth"] = {f"{f} (N {N}, T {T_})": ratio(f"egr_info_track_f32 {f} (N {N}, T {T_})", f"egr_trajectory_smooth_f32 {f} (N {N}, T {T_})")
                                                for N, T_ in CLIPS for f in forms}
    res["info_track_over_ray_track"] = {f"{f} (N {N}, T {T_})": ratio(f"egr_info_track_f32 {f} (N {N}, T {T_})", f"egr_ray_track_f32 {f} (N {N}, T {T_})")
                                        for N, T_ in CLIPS for f in forms}
    res["info_chain_over_clip_chain"] = {f: ratio(f"decode_clip_3d_info (T 64, {f})", f"decode_clip_3d (T 64, {f})") for f in forms}
    for key in ("info_track_over_trajectory_smooth", "info_track_over_ray_track", "info_chain_over_clip_chain"):
        print(key, res[key])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)

    # ---- accuracy on the rendered clip
    def figures(pose, valid):
        pose, valid = pose.double().cpu(), valid.cpu()
        err = (pose - truth).norm(dim=-1)
        mean = lambda m: round(float(err[m & valid].mean()), 4) if bool((m & valid).any()) else None
        return {"mean_error_cm": mean(torch.ones_like(valid)), "mean_error_at_glitches_cm": mean(glitch), "mean_error_elsewhere_cm": mean(~glitch & ~dropped),
                "valid_share": round(float(valid.float().mean()), 4)}

    def at_triangulated(hm, cc, accel, huber, k):
        """The variant the issue refutes: the same five launches, the matrices taken at the frame's own triangulated point."""
        j3, j2 = decode.decode_joints_3d(hm, cc, None, BETA, THR, MIN_DET)
        info = decode.joint_information(j3.pose.detach(), j2.maxvals, cc, None, (FS.HM, FS.HM), THR, MIN_DET)
        return decode.smooth_trajectory_info(j3.pose.detach(), info.info, j3.valid, accel, VEL, huber, k, MAX_GAP)

    def methods(hm, cc, accel_cm, accel_px):
        row = {}
        for form, h_cm, h_px, k in (("plain", 0.0, 0.0, 0), ("huber", HUBER_CM, HUBER_PX, K)):
            _, old = decode.decode_clip_3d(hm, cc, None, BETA, THR, MIN_DET, None, accel_cm, VEL, h_cm, k, MAX_GAP)
            _, ray = decode.decode_clip_3d_rays(hm, cc, None, BETA, THR, accel_cm, VEL, h_cm, k, MAX_GAP)
            _, _, new = decode.decode_clip_3d_info(hm, cc, None, BETA, THR, MIN_DET, ACCEL, accel_px, VEL, h_px, k, MAX_GAP)
            bad = at_triangulated(hm, cc, accel_px, h_px, k)
            torch.cuda.synchronize()
            for name, track in (("decode_clip_3d", old), ("decode_clip_3d_rays", ray), ("decode_clip_3d_info", new),
                                ("matrices at the triangulated points", bad)):
                row[f"{name} ({form})"] = figures(track.pose, track.valid)
        return row

    acc = {"clip": [T, 4, J, FS.HM, FS.HM], "unit": "cm", "pixel_noise": TB.PIXEL_NOISE, "one_view_pairs": int(dropped.sum()), "glitches": TB.GLITCHES,
           "glitch_cm": TB.GLITCH_CM, "defaults": {"accel_weight": ACCEL, "info_accel_weight": info_accel, "linearise_accel_weight": ACCEL},
           "vel_weight": VEL, "huber_cm": HUBER_CM, "huber_px": HUBER_PX, "reweights": K, "max_gap": MAX_GAP, "sweep": list(SWEEP), "rigs": {}}
    for rig, views in (("four views", 4), ("front pair", 2)):
        hm, cc = maps[:, :views].contiguous(), cams[:views]
        out = {"at_the_defaults": methods(hm, cc, ACCEL, info_accel), "accel_weight_sweep": {}}
        for name, fig in out["at_the_defaults"].items():
            print(rig, "| defaults |", name, fig)
        for accel in SWEEP:
            row = methods(hm, cc, accel, accel)
            out["accel_weight_sweep"][f"accel_weight {accel}"] = row
            print(rig, "| accel_weight", accel, {name: (fig["mean_error_cm"], fig["mean_error_at_glitches_cm"]) for name, fig in row.items()})
        best = {}
        for name in out["at_the_defaults"]:
            accel = min(SWEEP, key=lambda s: out["accel_weight_sweep"][f"accel_weight {s}"][name]["mean_error_cm"])
            fig = out["accel_weight_sweep"][f"accel_weight {accel}"][name]
            best[name] = {"accel_weight": accel, "at_the_edge_of_the_sweep": accel in (SWEEP[0], SWEEP[-1]), "mean_error_cm": fig["mean_error_cm"],
                          "mean_error_at_glitches_cm": fig["mean_error_at_glitches_cm"]}
            print(rig, "| best |", name, best[name])
        out["best_against_best"] = best
        acc["rigs"][rig] = out
    with open(a.accuracy_out, "w") as f:
        json.dump(acc, f, indent=1)
        f.write("\n")
    print("wrote", a.accuracy_out)


if __name__ == "__main__":
    main()

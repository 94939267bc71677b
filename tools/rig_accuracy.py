"""What the rig self-calibration buys on rendered heat maps -> profiles/rig_accuracy.json (the table of DESIGN.md 5t).

    python tools/rig_accuracy.py [--out profiles/rig_accuracy.json]

The syn rig with cameras 1..3 tilted by a random vector with entries in +-0.03 rad (tests/rig_statement.py `scene`), 64 and 1024 frames
of 15 random points, rendered as sigma-1 bumps on 64 x 64 maps through the TILTED cameras (FS.bumps).  `decode_joints_3d` with the
nominal rig is the error before; `calibrate_rig` on the same maps (8 iterations, view 0 held), then `decode_joints_3d` with its
coord_trans_mat, the error after; next to them the recovered rotations against the truth, and the same decode with the true matrices -
what the 64 x 64 maps allow at the best.  The soft-argmax at beta 100 of a sigma-1 bump is the bump's nearest pixel to within a
quarter of a pixel, and the ray-distance objective is biased by coordinate noise - noise makes every ray miss, and rays that meet closer
to the cameras miss by less, so the minimiser tilts the cameras towards each other by about 0.8 rad per squared pixel of noise, however
many frames it sees.  The second table therefore sweeps the noise: the same rig, 64 frames, exact projections plus Gaussian noise of
0.02 to 0.25 px, `refine_rig` and `triangulate_joints` before and after.  Errors are Euclidean, in cm.  Needs the GPU."""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FRAMES, V, J, HM, ANG, ITERATIONS = (64, 1024), 4, 15, 64, 0.03, 8
NOISE_PX = (0.02, 0.05, 0.1, 0.25)


def stats(err):
    import torch
    return {"mean": round(float(err.mean()), 3), "p95": round(float(torch.quantile(err, 0.95)), 3), "max": round(float(err.max()), 3),
            "n": int(err.numel())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rig_accuracy.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rig_accuracy: needs the GPU")
    import fisheye_statement as FS
    import rig_statement as RS
    from egorear_amd import decode, hip
    dev = "cuda:0"
    res = {"views": V, "joints": J, "maps": [HM, HM], "tilt_rad": ANG, "iterations": ITERATIONS, "device": hip.device_arch(),
           "library": hip.version(), "frames": {}}
    for B in FRAMES:
        sc = RS.scene(B, V, J, False, ANG, 0.0, 31)
        pts, true = sc["pts"], sc["true"]
        # (64 frames at a time: the float64 renderer's temporaries are large)
        hm = torch.cat([FS.bumps(pts[b:b + 64], sc["rec"], true, HM, HM).float() for b in range(0, B, 64)]).to(dev)
        before, _ = decode.decode_joints_3d(hm, sc["cams"])
        fit, _ = decode.calibrate_rig(hm, sc["cams"], iterations=ITERATIONS)
        after, _ = decode.decode_joints_3d(hm, sc["cams"], fit.coord_trans_mat)
        best, _ = decode.decode_joints_3d(hm, sc["cams"], true.float().expand(B, V, 4, 4).contiguous().to(dev))
        torch.cuda.synchronize()
        err = lambda j3: (j3.pose.double().cpu() - pts).norm(dim=-1)[j3.valid.cpu()]
        rot = (fit.rotation.double().cpu() - sc["vec"]).abs()
        row = {"valid": bool(fit.valid), "pairs": int(fit.pairs), "steps": int(fit.steps), "grad": float(fit.grad),
               "rms_ray_distance_cm": [round(float(fit.cost0) ** 0.5, 4), round(float(fit.cost) ** 0.5, 4)],
               "error_nominal_rig_cm": stats(err(before)), "error_calibrated_rig_cm": stats(err(after)), "error_true_rig_cm": stats(err(best)),
               "rotation_error_rad": {"max": float(rot.max()), "per_camera": [round(float(v), 6) for v in rot.amax(1)]},
               "tilt_rad_per_camera": [round(float(v), 6) for v in sc["vec"].norm(dim=1)]}
        res["frames"][str(B)] = row
        print(f"| {B} | {row['error_nominal_rig_cm']['mean']:.2f} | {row['error_calibrated_rig_cm']['mean']:.2f} | "
              f"{row['error_true_rig_cm']['mean']:.2f} | {row['rotation_error_rad']['max']:.2e} | "
              f"{row['rms_ray_distance_cm'][0]:.2f} -> {row['rms_ray_distance_cm'][1]:.2f} | {row['steps']} |")
    res["noise_sweep_64_frames"] = {}
    for noise in NOISE_PX:
        B = 64
        sc = RS.scene(B, V, J, False, ANG, noise, 31)
        coords, conf, pts = sc["coords"].to(dev), sc["conf"].to(dev), sc["pts"]
        fit = decode.refine_rig(coords, conf, sc["cams"], iterations=ITERATIONS)
        tri = [decode.triangulate_joints(coords, conf, sc["cams"], m) for m in
               (None, fit.coord_trans_mat, sc["true"].float().expand(B, V, 4, 4).contiguous().to(dev))]
        torch.cuda.synchronize()
        err = lambda j3: (j3.pose.double().cpu() - pts).norm(dim=-1)[j3.valid.cpu()]
        rot = float((fit.rotation.double().cpu() - sc["vec"]).abs().max())
        row = {"rms_ray_distance_cm": [round(float(fit.cost0) ** 0.5, 4), round(float(fit.cost) ** 0.5, 4)], "steps": int(fit.steps),
               "error_nominal_rig_cm": stats(err(tri[0])), "error_calibrated_rig_cm": stats(err(tri[1])), "error_true_rig_cm": stats(err(tri[2])),
               "rotation_error_rad_max": rot}
        res["noise_sweep_64_frames"][str(noise)] = row
        print(f"| {noise} px | {row['error_nominal_rig_cm']['mean']:.2f} | {row['error_calibrated_rig_cm']['mean']:.2f} | "
              f"{row['error_true_rig_cm']['mean']:.2f} | {rot:.2e} | {row['rms_ray_distance_cm'][0]:.2f} -> {row['rms_ray_distance_cm'][1]:.2f} |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

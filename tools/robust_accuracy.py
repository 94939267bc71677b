"""Error of the top-1 and of the robust 3-D decoder on heat maps with a distractor -> profiles/robust_accuracy_float64.json, or with
--device profiles/robust_accuracy_device.json (the table of DESIGN.md 5p).

    python tools/robust_accuracy.py [--frames 10] [--device] [--out ...]

The bumps of the triangulation's round-trip test (sigma 1 on 64 x 64 maps at the syn rig's projections of random points, seed 77, 15
joints a frame) plus, in one view per joint - and, in a second table, in two - an extra bump of height 1.2 at a random spot more than 10
px from the true one (tests/robust_statement.py builds the scene).  Decoders: the whole-map soft-argmax of every view + triangulation
(`decode_joints_3d`), and top-3 peaks per view + consensus + triangulation (`decode_joints_3d_robust`) with the window refinement at
beta 100 and at beta 10 (5 x 5 window), with four views and with the two front cameras.  Without --device the float64 statements of
tests/ are evaluated on the CPU (imported, not restated); with --device the kernels run.  Errors are Euclidean, in cm: mean, 95th
percentile, maximum over the joints with a valid pose; `valid` counts them."""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

K, RN, R, THR, TAU = 3, 1, 2, 0.5, 2.0
BETAS = (100.0, 10.0)


def stats(err, ok):
    import torch
    err = err[ok]
    if err.numel() == 0:
        return {"mean": None, "p95": None, "max": None, "valid": 0, "n": int(ok.numel())}
    return {"mean": round(float(err.mean()), 3), "p95": round(float(torch.quantile(err, 0.95)), 3), "max": round(float(err.max()), 3),
            "valid": int(ok.sum()), "n": int(ok.numel())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import robust_statement as RS
    out = a.out or os.path.join(REPO, "profiles", "robust_accuracy_device.json" if a.device else "robust_accuracy_float64.json")
    if a.device:
        if not torch.cuda.is_available():
            raise SystemExit("robust_accuracy --device: needs the GPU")
        from egorear_amd import decode
    res = {"frames": a.frames, "joints": 15, "maps": [RS.HM, RS.HM], "k": K, "nms_radius": RN, "refine_radius": R, "threshold": THR,
           "max_reproj": TAU, "min_views": 2, "distractor_height": 1.2,
           "arithmetic": "kernels on the device" if a.device else "float64 statements on the CPU", "rows": {}}
    for views in ((0, 1, 2, 3), (0, 1)):
        V = len(views)
        for distract in (1, 2):
            scene = RS.distractor_scene(a.frames, views, distract=distract)
            pts, rec, hm = scene["pts"], scene["rec"], scene["hm"]
            rows = {}
            if a.device:
                dhm = hm.to("cuda:0")
                tri, _ = decode.decode_joints_3d(dhm, scene["cams"], None, 100.0, THR)
                rows["top-1 peak per view + triangulation"] = stats((tri.pose.double().cpu() - pts).norm(dim=-1), tri.valid.cpu())
                for beta in BETAS:
                    rob, con, _ = decode.decode_joints_3d_robust(dhm, scene["cams"], None, K, RN, R, beta, THR, TAU, 2)
                    torch.cuda.synchronize()
                    rows[f"top-{K} peaks + consensus + triangulation, beta {beta:g}"] = stats((rob.pose.double().cpu() - pts).norm(dim=-1),
                                                                                             rob.valid.cpu())
            else:
                pose, ok = RS.top1_chain(hm.double(), rec)
                rows["top-1 peak per view + triangulation"] = stats((pose - pts).norm(dim=-1), ok)
                for beta in BETAS:
                    pose, ok, con, _ = RS.robust_chain(hm.double(), rec, None, K, RN, R, beta, THR, TAU, 2)
                    s = stats((pose - pts).norm(dim=-1), ok)
                    win = con["score"]
                    # the winner's lead over the best qualifying hypothesis with another selection, relative
                    differs = (con["all_choice"] != con["choice"].long().permute(0, 2, 1).unsqueeze(2)).any(-1) & con["all_ok"]
                    rival = torch.where(differs, con["all_score"], torch.zeros_like(con["all_score"])).max(-1)[0]
                    s["min_relative_lead"] = round(float(((win - rival) / win)[con["hyp"] >= 0].min()), 4)
                    rows[f"top-{K} peaks + consensus + triangulation, beta {beta:g}"] = s
            res["rows"][f"{V} views, {distract} distractor view{'s' if distract > 1 else ''}"] = rows
            for name, s in rows.items():
                print(f"| {V} views, {distract} distractor | {name} | {s['mean']} | {s['p95']} | {s['max']} | {s['valid']}/{s['n']} |")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()

"""What the causal fixed-lag trajectory filter buys on the rendered clip of profiles/trajectory_accuracy.json ->
profiles/trajectory_filter_accuracy.json.

    python tools/trajectory_filter_accuracy.py [--out profiles/trajectory_filter_accuracy.json]

The clip is tools/trajectory_bench.py's, from the same generator: T = 64 frames of a moving 15-joint skeleton as sigma-1 bumps at the
syn rig's projections with 0.3 px of noise on every centre, 15 % of the (frame, joint) pairs keeping one view, 8 pairs rendered 40 cm off
in every view for one frame.  With the four views and with the front pair alone, the clip is fed through decode.decode_stream_3d as one
stream at lag 0 / 2 / 4 / 8 / 16 with the gate off and at 1 / 2 / 5 cm; every frame is taken as it came out - from the arrival `lag` frames
later, the last `lag` from decode.filter_tail - and compared with the truth: the mean joint error over the valid poses, at the
glitches, in the pairs one camera sees, and the share of valid poses, next to per-frame decode_joints_3d and both forms of
decode_clip_3d (which see the whole clip).  Reported as measured, losses included."""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

J = 15
LAGS = (0, 2, 4, 8, 16)
GATES = (0.0, 1.0, 2.0, 5.0)
ACCEL, VEL, HUBER, K, MAX_GAP = 10.0, 0.0, 1.0, 4, 8
BETA, THR, MIN_DET = 100.0, 0.5, 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trajectory_filter_accuracy.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("trajectory_filter_accuracy: needs the GPU (nothing is measured without one)")
    import fisheye_statement as FS
    import trajectory_bench as TB
    from egorear_amd import decode
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    cams = FS.rig()
    T = 64
    truth, maps, glitch, dropped = TB.rendered_clip(T, list(decode.HEATMAP_PARENTS_15), FS.records(cams), gen, torch, FS)
    maps = maps.contiguous().to(dev)

    def figures(pose, valid):
        pose, valid = pose.double().cpu(), valid.cpu()
        err = (pose - truth).norm(dim=-1)
        mean = lambda m: round(float(err[m & valid].mean()), 4) if bool((m & valid).any()) else None
        return {"mean_error_cm": mean(torch.ones_like(valid)), "largest_error_cm": round(float(err[valid].max()), 4),
                "mean_error_at_glitches_cm": mean(glitch), "mean_error_in_one_view_pairs_cm": mean(dropped),
                "mean_error_elsewhere_cm": mean(~glitch & ~dropped), "valid_share": round(float(valid.float().mean()), 4)}

    acc = {"clip": [T, 4, J, FS.HM, FS.HM], "unit": "cm", "pixel_noise": TB.PIXEL_NOISE, "one_view_pairs": int(dropped.sum()),
           "glitches": TB.GLITCHES, "glitch_cm": TB.GLITCH_CM, "accel_weight": ACCEL, "vel_weight": VEL, "huber_cm": HUBER, "reweights": K,
           "max_gap": MAX_GAP, "filter": "every frame as it came out: from the arrival `lag` frames later, the last `lag` from the tail",
           "rigs": {}}
    for rig, views in (("four views", 4), ("front pair", 2)):
        hm, cc = maps[:, :views].contiguous(), cams[:views]
        per_frame, _ = decode.decode_joints_3d(hm, cc, None, BETA, THR, MIN_DET)
        _, plain = decode.decode_clip_3d(hm, cc, None, BETA, THR, MIN_DET, None, ACCEL, VEL, 0.0, 0, MAX_GAP)
        _, robust = decode.decode_clip_3d(hm, cc, None, BETA, THR, MIN_DET, None, ACCEL, VEL, HUBER, K, MAX_GAP)
        methods = {"decode_joints_3d (per frame)": figures(per_frame.pose, per_frame.valid),
                   "decode_clip_3d (plain, whole clip)": figures(plain.pose, plain.valid),
                   f"decode_clip_3d (huber {HUBER} cm, K {K}, whole clip)": figures(robust.pose, robust.valid)}
        for lag in LAGS:
            for gate in GATES:
                state = decode.new_track_filter(1, J, lag, dev, ACCEL, VEL, gate, MAX_GAP)
                _, step = decode.decode_stream_3d(state, hm.unsqueeze(0), cc, None, BETA, THR, MIN_DET)
                rest = decode.filter_tail(state)
                torch.cuda.synchronize()
                pose = torch.cat((step.pose[0, lag:], rest.pose[0]), 0)
                valid = torch.cat((step.valid[0, lag:], rest.valid[0]), 0)
                frame = torch.cat((step.frame[0, lag:], rest.frame[0]), 0)
                assert frame.tolist() == list(range(T))
                methods[f"filter lag {lag}, gate {'off' if gate == 0 else f'{gate:g} cm'}"] = figures(pose, valid)
        acc["rigs"][rig] = methods
        for name, fig in methods.items():
            print(rig, "|", name, fig)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(acc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

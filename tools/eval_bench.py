#!/usr/bin/env python3
"""What a validation step costs next to its forward (egorear_amd.evaluate), at batch 64, config 3 (HeatmapMVFEX) and config 4 (pose3d):
  (a) the forward replayed alone (runner.GraphedForward), (b) step() = forward + metrics + accumulation as one graph,
  (c) the heat-map metric launch alone, with its bytes (S + 1) * B * V * J * H * W * 4 -> GB/s, beside the read-only streaming
      rate of this box taken the way tools/hbm_probe.py takes it (torch's sum over 2 GiB), in the same run,
  (d) the reference's host-loop formulation of `evaluate` (heatmap_mvf_ex.py:263-316: `.cpu()` per sample, boolean indexing)
      restated with torch ops on the same device tensors, for the calls one step makes.
HIP-event medians.  One JSON line.     python tools/eval_bench.py [--batch 64] [--reps 30] [--out profiles/eval_step_b64.json]"""
import argparse
import copy
import json
import os
import socket
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from egorear_amd import configs, evaluate, metrics, synth  # noqa: E402
from egorear_amd.estimator import EgoPoseFormerHeatmapMVFEX, EgoPoseFormerMVFEX  # noqa: E402
from egorear_amd.runner import GraphedForward  # noqa: E402


def median_ms(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def reference_evaluate(pred, gt, threshold=1.0):
    """heatmap_mvf_ex.py:263-316 restated op for op on device tensors (host loop, one `.cpu()` per sample and view)."""
    B, V = pred.shape[:2]
    xs = [pred[:, i].reshape(B, -1) for i in range(V)]
    ys = [gt[:, i].reshape(B, -1) for i in range(V)]
    pos = [y > 0 for y in ys]
    err = sum(torch.abs(x - y) for x, y in zip(xs, ys)).sum(dim=1).reshape(B).detach().cpu()
    pos_err = torch.tensor([sum(torch.abs(x[i][ind[i]] - y[i][ind[i]]).sum().detach().cpu() for x, y, ind in zip(xs, ys, pos)) for i in range(B)])
    mse = torch.nn.functional.mse_loss(pred, gt)

    def pts(h):
        m, idx = h.reshape(*h.shape[:3], -1).max(-1)
        return torch.stack([(idx % h.shape[-1]).float(), (idx // h.shape[-1]).float()], -1), m >= threshold
    pp, _ = pts(pred)
    gp, valid = pts(gt)
    mse_pts = torch.nn.functional.mse_loss(pp * valid.unsqueeze(-1), gp * valid.unsqueeze(-1))
    return err, pos_err, mse, mse_pts


def hbm_read_gbs():
    a = torch.empty(1 << 29, device="cuda")        # 2 GiB, tools/hbm_probe.py's read-only leg
    a.fill_(1.0)
    ms = median_ms(lambda: a.sum(), 10, warmup=2)
    return 4 * a.numel() / ms / 1e6


def leg(name, cls, cfg, batch, reps, gt_hm):
    net = cls(**copy.deepcopy(cfg)).eval()
    synth.load_synth(net, 42)
    net = net.cuda()
    img = synth.synth_images(batch, 4, seed=1234).cuda()
    fwd = GraphedForward(net)
    out = fwd(img)
    a = median_ms(lambda: fwd(img), reps)
    ev = evaluate.evaluator_for(net)
    gt = gt_hm if name == "config3_heatmap_mvfex" else synth.synth_gt_pose(batch).double().cuda()
    ev.step(img, gt, "val")
    b = median_ms(lambda: ev.step(img, gt, "val"), reps)
    rec = {"forward_replay_ms": round(a, 4), "step_ms": round(b, 4), "step_minus_forward_us": round((b - a) * 1e3, 1),
           "step_minus_forward_share_of_forward": round((b - a) / a, 5), "eval_class": type(ev).__name__, "keys": len(ev.keys("val"))}
    hms = out[0] if name == "config3_heatmap_mvfex" else out[1]
    hms = [h.clone() for h in hms]
    return rec, hms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: needs a GPU (nothing is measured without one)")
    from oracle import train_oracle as TO
    B = args.batch
    gt_hm = TO.synth_gt_heatmap(B).cuda()
    res = {"tool": "tools/eval_bench.py", "box": socket.gethostname(), "device": torch.cuda.get_device_properties(0).name, "batch": B,
           "reps": args.reps, "timing": "HIP events, median"}
    res["config3_heatmap_mvfex"], hms = leg("config3_heatmap_mvfex", EgoPoseFormerHeatmapMVFEX, configs.heatmap_mvfex_cfg(), B, args.reps, gt_hm)
    res["config4_pose3d"], _ = leg("config4_pose3d", EgoPoseFormerMVFEX, configs.pose3d_cfg("ego4view_syn"), B, args.reps, gt_hm)
    # (c) the heat-map metric launch alone: two sets, two view groups - what one stage-2 step issues
    sets, groups = [hms[0], hms[-1]], [(0, 2), (2, 4)]
    c = median_ms(lambda: metrics.heatmap_metrics(sets, gt_hm, view_groups=groups), args.reps)
    nbytes = (len(sets) + 1) * gt_hm.numel() * 4
    hbm = hbm_read_gbs()
    res["metric_launch"] = {"sets": len(sets), "view_groups": groups, "ms": round(c, 4), "bytes": nbytes, "gb_per_s": round(nbytes / c / 1e6, 1),
                            "hbm_probe_read_only_gb_per_s": round(hbm, 1), "fraction_of_hbm_probe": round(nbytes / c / 1e6 / hbm, 4),
                            "note": "the 189 MB working set fits the 256 MiB Infinity Cache: repeated launches on the same tensors may be served on-die"}
    # (d) the reference's formulation: the four `evaluate` calls of one stage-2 validation step
    def host_loop():
        for p in sets:
            for v0, v1 in groups:
                reference_evaluate(p[:, v0:v1], gt_hm[:, v0:v1])
    d = median_ms(host_loop, max(3, args.reps // 10), warmup=1)
    extra = res["config3_heatmap_mvfex"]["step_ms"] - res["config3_heatmap_mvfex"]["forward_replay_ms"]
    res["reference_host_loop"] = {"calls": len(sets) * len(groups), "ms": round(d, 3), "over_step_minus_forward": round(d / extra, 1) if extra > 0 else None}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

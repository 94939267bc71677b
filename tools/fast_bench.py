#!/usr/bin/env python3
"""The opt-in fast policy (hip.LaunchPolicy.fast()) against the shipped one, in ONE process on the same weights:

    python tools/fast_bench.py [--out profiles/fast_policy_b64.json] [--steps 60] [--repeats 3]

Two modules hold the same seeded weights, one per policy (engine.set_policy - the way bench.py's exact leg coexists with the headline).
Per policy: frames/s at batch 64 through runner.PipelinedForward (two lanes, as bench.py's headline), `repeats` timed windows of
`steps` steps each, the two policies ALTERNATING window by window (other work shares the machine: a difference counts only beyond the
spread of the repeats); and the summed time of the conv2d launches the role-split kernel carries, from HIP events around every launch
of an eager one-lane forward (best of 5 per launch, tools/kernel_times.py's method - a profile of its own, never inside a timed window).
Also the heat-map error of both policies against the reference's golden vectors at batch 2 (what tests/test_gpu_fast_policy.py takes
its bound from).  No CPU path: without a GPU this fails."""
import argparse, copy, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from egorear_amd import configs, engine, hip, synth
from egorear_amd.estimator import EgoPoseFormerHeatmap, EgoPoseFormerMVFEX
from egorear_amd.runner import PipelinedForward

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fast_policy_b64.json"))
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=60, help="steps per timed window (about half a second at batch 64)")
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--repeats", type=int, default=3)
a = ap.parse_args()
assert hip.POLICY.w_format == "f16x2", "the comparison is against the shipped policy: unset EGR_W_FORMAT"
POLICIES = {"shipped": None, "fast": hip.POLICY.fast()}


def build(cls, cfg, pol):
    net = cls(**copy.deepcopy(cfg)).eval()
    synth.load_synth(net, 42)
    net = net.cuda()
    engine.set_policy(net, pol)
    return net


def window(pipe, img, steps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        pipe(img)
    pipe.wait()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


out = {"batch": a.batch, "steps_per_window": a.steps, "warmup_steps": a.warmup, "repeats": a.repeats, "lanes": 2, "device": hip.device_arch(),
       "what": "one process, two modules on the same weights (engine.set_policy), windows alternating between the policies"}
img = synth.synth_images(a.batch, 4, seed=1234).cuda()
nets = {n: build(EgoPoseFormerMVFEX, configs.pose3d_cfg(), p) for n, p in POLICIES.items()}
with torch.no_grad():
    # ---- role-split launches of one eager forward, per policy: events around every launch, best of 5
    for n, net in nets.items():
        net(img); torch.cuda.synchronize()
        hip.PLAN_LOG = []
        net(img); torch.cuda.synchronize()
        plans, hip.PLAN_LOG = hip.PLAN_LOG, None
        runs = []
        for _ in range(5):
            hip.PROFILE = []
            net(img); torch.cuda.synchronize()
            prof, hip.PROFILE = hip.PROFILE, None
            runs.append([(name, s.elapsed_time(e), tag) for name, s, e, _f, _b, tag in prof])
        best = [(runs[0][i][0], min(r[i][1] for r in runs), runs[0][i][2]) for i in range(len(runs[0]))]
        convs = [(t, ms) for name, ms, t in best if name == "egr_conv2d_nhwc_f32" and "masked" not in t]
        assert len(convs) == len(plans), (len(convs), len(plans))
        tapx = [(t, ms, p) for (t, ms), (_t, p) in zip(convs, plans) if p.route == hip.ROUTE_TAPX]
        out[n] = {"forward_ms_one_lane_eager_sum_of_launches": round(sum(ms for _, ms, _ in best), 4), "launches": len(best),
                  "role_split_launches": len(tapx), "role_split_one_product_launches": sum(1 for *_, p in tapx if p.planes == 1),
                  "role_split_ms": round(sum(ms for _, ms, _ in tapx), 4),
                  "role_split_3x3_ms": round(sum(ms for t, ms, _ in tapx if " k3s" in t), 4),
                  "role_split_detail": [{"tag": t, "ms": round(ms, 4), "planes": p.planes, "variant": p.variant, "tile": [p.bm, p.bn]} for t, ms, p in tapx]}
        print(f"[{n}] role-split launches {len(tapx)} ({out[n]['role_split_one_product_launches']} one-product): {out[n]['role_split_ms']:.3f} ms "
              f"(3x3: {out[n]['role_split_3x3_ms']:.3f} ms) of {out[n]['forward_ms_one_lane_eager_sum_of_launches']:.3f} ms over {len(best)} launches", flush=True)
    # ---- throughput: two lanes, windows alternating between the policies
    pipes = {n: PipelinedForward(net, lanes=2, copy_inputs=False) for n, net in nets.items()}
    for n, p in pipes.items():
        p.prime(img)
    # (a capture under one policy drops no pack of the other module, but engine.GENERATION is process-wide: capture both, THEN warm up)
    for n, p in pipes.items():
        window(p, img, a.warmup)
    ms = {n: [] for n in pipes}
    for r in range(a.repeats):
        for n, p in pipes.items():
            ms[n].append(window(p, img, a.steps))
            print(f"[{n}] window {r + 1}/{a.repeats}: {ms[n][-1]:.4f} ms/step, {a.batch / ms[n][-1] * 1e3:.1f} frames/s", flush=True)
    for n in pipes:
        fps = [a.batch / m * 1e3 for m in ms[n]]
        out[n].update({"ms_per_step": [round(m, 4) for m in ms[n]], "frames_per_s": [round(f, 1) for f in fps],
                       "frames_per_s_median": round(float(np.median(fps)), 1), "frames_per_s_spread": round(max(fps) - min(fps), 1)})
    spread = max(out["shipped"]["frames_per_s_spread"], out["fast"]["frames_per_s_spread"])
    gain = out["fast"]["frames_per_s_median"] - out["shipped"]["frames_per_s_median"]
    out["fast_over_shipped"] = round(out["fast"]["frames_per_s_median"] / out["shipped"]["frames_per_s_median"], 4)
    out["fast_beats_shipped_beyond_spread"] = bool(gain > spread)
    out["role_split_ms_fast_over_shipped"] = round(out["fast"]["role_split_ms"] / out["shipped"]["role_split_ms"], 4)
    print(f"fast / shipped: {out['fast_over_shipped']:.4f} in frames/s (gain {gain:.1f}, spread {spread:.1f}), {out['role_split_ms_fast_over_shipped']:.4f} in role-split time", flush=True)
    del pipes, nets
    # ---- the heat-map estimator at batch 2 against the reference's golden vectors, role-split kernel from one tile up
    hip.lib.egr_conv_set_tapx(1, 1, 256)
    try:
        hnets = {n: build(EgoPoseFormerHeatmap, configs.heatmap_cfg(), p) for n, p in POLICIES.items()}
        err = {n: {} for n in hnets}
        for seed in (0, 1):
            g = np.load(os.path.join(REPO, "tests", "golden", f"heatmap_s{seed}.npz"))["hm_sl"]
            x = synth.synth_images(2, 2, seed=seed).cuda()
            for n, net in hnets.items():
                err[n][f"s{seed}"] = float(np.abs(net(x).float().cpu()[:, :, :, ::8, ::8].numpy() - g).max())
            err.setdefault("golden_max", {})[f"s{seed}"] = float(np.abs(g).max())
    finally:
        hip.lib.egr_conv_set_tapx(1, 256, 256)
    out["heatmap_golden_err"] = dict(err["fast"], shipped=err["shipped"], golden_max=err["golden_max"],
                                     what="max |heat map - reference golden| on the golden's sub-sampled grid, EgoPoseFormerHeatmap B 2 V 2, seeds 0 / 1")
    print("heat-map error against the golden:", json.dumps(out["heatmap_golden_err"]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
json.dump(out, open(a.out, "w"), indent=1)
print(f"-> {a.out}")

#!/usr/bin/env python3
"""The half-precision training policy (hip.LaunchPolicy.fast_training()) against the default one, in ONE process:

    python tools/fast_train_bench.py [--out profiles/fast_train_b32.json] [--steps 40] [--repeats 3]

Two trainers hold copies of the same seeded weights, one per policy (`hip.use_policy` around everything a trainer does).  Per policy:
  * ms per stage-3 step at batch 32 with the step replayed as one hipGraph, `repeats` timed windows of `steps` steps between device
    events, the two policies ALTERNATING window by window after a warm-up of their own (other work shares the machine: a difference
    counts only beyond the spread of the windows);
  * the per-family sums of one instrumented EAGER step on one stream (events around every launch, best of 3 per launch - a profile of
    its own, never inside a timed window): role-split forward / data-gradient conv launches, the other conv launches, the weight
    gradients by kernel, everything else;
  * the deviation of the first update's loss and gradient from the default trainer's (same weights, same batch), beside the same
    figures for exact() - the distance between two arithmetics that both hold the parity contract;
  * a one-batch overfit at batch 2 (30 updates, warmup_iters=1): the loss curve of each policy.
The parity contract does not apply to fast_training().  No CPU path: without a GPU this fails."""
import argparse, copy, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from egorear_amd import configs, hip, synth, train
from egorear_amd.estimator import EgoPoseFormerMVFEX
from egorear_amd.metrics import generate_target

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fast_train_b32.json"))
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--steps", type=int, default=40, help="steps per timed window (about a second at batch 32)")
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--overfit-updates", type=int, default=30)
a = ap.parse_args()
assert hip.POLICY.w_format == "f16x2", "the comparison is against the default policy: unset EGR_W_FORMAT"
POLICIES = {"default": hip.LaunchPolicy(), "fast_training": hip.LaunchPolicy.fast_training()}
DEV = "cuda:0"

seed_net = EgoPoseFormerMVFEX(**copy.deepcopy(configs.pose3d_cfg("ego4view_rw")))
synth.load_synth(seed_net, 42)


def batch(B):
    return (synth.synth_images(B, 4, seed=1234).to(DEV), synth.synth_coord_trans_mat(B).to(DEV), synth.synth_gt_pose(B).to(DEV),
            generate_target(synth.synth_joint_px(B).to(DEV)).contiguous())


def trainer(pol, **kw):
    with hip.use_policy(pol):
        return train.Trainer(copy.deepcopy(seed_net).to(DEV), **kw)


def first_update(pol, args):
    """(trainer, loss terms, flat gradient, per-tensor gradients) of the first eager update under `pol`."""
    tr = trainer(pol, use_graph=True)
    with hip.use_policy(pol):
        S, _ = tr._run(*args, update=True)
        tr._eager_done += 1
        tr._invalidate()
    torch.cuda.synchronize()
    return tr, S.loss_terms.double().cpu(), tr.opt.flat_g.clone(), {k: tr.opt.gviews[k].clone() for k in S.pgrads}


def deviation(ref, got):
    (_, l0, g0, p0), (_, l1, g1, p1) = ref, got
    per = sorted(((float((p1[k].double() - p0[k].double()).norm() / float(p0[k].double().norm())), k) for k in p0
                  if k in p1 and float(p0[k].abs().max()) > 0), reverse=True)
    return {"loss_rel": abs(float(l1.sum()) - float(l0.sum())) / abs(float(l0.sum())),
            "flat_grad_rel": float((g1.double() - g0.double()).norm() / g0.double().norm()),
            "worst_tensor_rel": per[0][0], "worst_tensor": per[0][1], "median_tensor_rel": per[len(per) // 2][0]}


def families(tr, pol, args):
    """One instrumented eager step on one stream, best of 3 per launch: ms per family."""
    orig, overlap = hip.conv2d_wgrad, train.OVERLAP
    runs = []
    try:
        train.OVERLAP = False
        for _ in range(3):
            wg = []

            def spy(*x, **k):
                r = orig(*x, **k)
                wg.append((hip.lib.egr_wgrad_last_kernel(), hip.lib.egr_wgrad_last_planes()))
                return r
            hip.conv2d_wgrad, hip.PROFILE, hip.PLAN_LOG = spy, [], []
            with hip.use_policy(pol):
                tr._run(*args, update=True)
                tr._invalidate()
            torch.cuda.synchronize()
            prof, plans = hip.PROFILE, hip.PLAN_LOG
            hip.PROFILE = hip.PLAN_LOG = None
            runs.append(([(n, s.elapsed_time(e), t) for n, s, e, _f, _b, t in prof], plans, wg))
    finally:
        hip.conv2d_wgrad, train.OVERLAP, hip.PROFILE, hip.PLAN_LOG = orig, overlap, None, None
    prof, plans, wg = runs[0]
    best = [(prof[i][0], min(r[0][i][1] for r in runs), prof[i][2]) for i in range(len(prof))]
    convs = [i for i, (n, _, _) in enumerate(best) if n == "egr_conv2d_nhwc_f32"]
    wgs = [i for i, (n, _, _) in enumerate(best) if n == "egr_conv2d_wgrad_f32"]
    assert len(convs) == len(plans) and len(wgs) == len(wg), (len(convs), len(plans), len(wgs), len(wg))
    fam = {}

    def add(key, ms, one):
        cur = fam.setdefault(key, {"ms": 0.0, "launches": 0, "one_product": 0})
        cur["ms"] += ms
        cur["launches"] += 1
        cur["one_product"] += int(one)
    seen = set(convs) | set(wgs)
    for i, (tag, p) in zip(convs, plans):
        if p.route == hip.ROUTE_TAPX:
            add("role_split_data_gradient" if (best[i][2].startswith("T ") or "masked" in best[i][2]) else "role_split_forward", best[i][1], p.planes == 1)
        else:
            add("conv_other", best[i][1], False)
    for i, (kern, planes) in zip(wgs, wg):
        add(f"wgrad_kernel_{kern}", best[i][1], planes == 1)
    for i, (n, ms, t) in enumerate(best):
        if i not in seen:
            add("everything_else", ms, False)
    for v in fam.values():
        v["ms"] = round(v["ms"], 4)
    fam["sum_of_launches_ms"] = round(sum(ms for _, ms, _ in best), 4)
    return fam


def window(tr, pol, args, steps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with hip.use_policy(pol):
        s.record()
        for _ in range(steps):
            tr.step(*args)
        e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


out = {"batch": a.batch, "steps_per_window": a.steps, "warmup_steps": a.warmup, "repeats": a.repeats, "device": hip.device_arch(),
       "what": "one process, two trainers on copies of the same seeded weights (hip.use_policy), stage-3 step replayed as one hipGraph, "
               "windows alternating between the policies; the parity contract does not apply to fast_training"}
args = batch(a.batch)
first = {n: first_update(p, args) for n, p in POLICIES.items()}
ex = first_update(hip.LaunchPolicy().exact(), args)
out["deviation_from_default_b%d" % a.batch] = {"fast_training": deviation(first["default"], first["fast_training"]),
                                                "exact": deviation(first["default"], ex)}
print("deviation:", json.dumps(out["deviation_from_default_b%d" % a.batch]), flush=True)
del ex
trs = {n: f[0] for n, f in first.items()}
del first
torch.cuda.empty_cache()
for n, tr in trs.items():
    out[n] = {"families_eager_one_stream": families(tr, POLICIES[n], args)}
    print(f"[{n}] families:", json.dumps(out[n]["families_eager_one_stream"]), flush=True)
for n, tr in trs.items():           # capture (the third step on) and warm up, per policy
    window(tr, POLICIES[n], args, a.warmup)
    assert tr.graph is not None, f"[{n}] capture of the step was refused"
ms = {n: [] for n in trs}
for r in range(a.repeats):
    for n, tr in trs.items():
        ms[n].append(window(tr, POLICIES[n], args, a.steps))
        print(f"[{n}] window {r + 1}/{a.repeats}: {ms[n][-1]:.3f} ms/step", flush=True)
for n in trs:
    v = sorted(ms[n])
    out[n].update({"ms_per_step": [round(m, 4) for m in ms[n]], "ms_per_step_median": round(v[len(v) // 2], 4), "ms_per_step_spread": round(v[-1] - v[0], 4)})
spread = max(out[n]["ms_per_step_spread"] for n in trs)
gain = out["default"]["ms_per_step_median"] - out["fast_training"]["ms_per_step_median"]
out["fast_training_over_default_ms"] = round(out["fast_training"]["ms_per_step_median"] / out["default"]["ms_per_step_median"], 4)
out["fast_training_not_slower_beyond_spread"] = bool(-gain <= spread)
out["fast_training_faster_beyond_spread"] = bool(gain > spread)
print(f"fast_training / default: {out['fast_training_over_default_ms']:.4f} in ms/step (gain {gain:.3f} ms, spread {spread:.3f} ms)", flush=True)
del trs
torch.cuda.empty_cache()
# ---- one-batch overfit at batch 2
args2 = batch(2)
out["overfit_b2"] = {"updates": a.overfit_updates, "warmup_iters": 1}
for n, pol in POLICIES.items():
    tr = trainer(pol, warmup_iters=1, use_graph=True)
    with hip.use_policy(pol):
        out["overfit_b2"][n] = [round(float(tr.step(*args2)[0].sum()), 6) for _ in range(a.overfit_updates + 1)]
    print(f"[{n}] overfit: {out['overfit_b2'][n][0]:.4f} -> {out['overfit_b2'][n][-1]:.4f}", flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
json.dump(out, open(a.out, "w"), indent=1)
print(f"-> {a.out}")

"""Training-step timing and per-kernel breakdown (config 5: ego4view_rw_pose3d, batch 32 per GPU).

    python tools/train_bench.py [--batch 32] [--steps 5]
    python tools/train_bench.py --graph --accumulate 8      # gradient accumulation: ms per micro-step and per optimizer update
    python tools/train_bench.py --graph --policy fast_training     # the half-precision training policy (tags say h1)
"""
import argparse
import collections
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from egorear_amd import configs, hip, synth, train  # noqa: E402
from egorear_amd.estimator import EgoPoseFormerMVFEX  # noqa: E402
from egorear_amd.metrics import generate_target  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--graph", action="store_true", help="replay the step as one hipGraph")
    ap.add_argument("--dump", default="", help="write every launch of the instrumented step (order, us, name, tag) to this file")
    ap.add_argument("--accumulate", type=int, default=1, help="micro-batches per optimizer update (--steps / --warmup then count updates)")
    ap.add_argument("--json", default="", help="with --accumulate: also write the figures to this file")
    ap.add_argument("--policy", choices=["default", "fast_training"], default="default",
                    help="launch policy of the step: the process default, or hip.LaunchPolicy.fast_training() (outside the parity contract)")
    a = ap.parse_args()
    with hip.use_policy(hip.LaunchPolicy.fast_training() if a.policy == "fast_training" else None):
        run(a)


def run(a):
    dev = "cuda:0"
    net = EgoPoseFormerMVFEX(**copy.deepcopy(configs.pose3d_cfg("ego4view_rw")))
    synth.load_synth(net, 42)
    net = net.to(dev)
    tr = train.Trainer(net, use_graph=a.graph, accumulate=a.accumulate)
    B = a.batch
    img = synth.synth_images(B, 4, seed=1234).to(dev)
    ctm = synth.synth_coord_trans_mat(B).to(dev)
    gt_pose = synth.synth_gt_pose(B).to(dev)
    gt_hm = generate_target(synth.synth_joint_px(B).to(dev)).contiguous()
    if a.accumulate > 1:
        return accumulate_leg(a, tr, (img, ctm, gt_pose, gt_hm))
    for _ in range(a.warmup):
        terms, _ = tr.step(img, ctm, gt_pose, gt_hm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = 0.0
    for _ in range(a.steps):
        h0 = time.perf_counter()
        terms, _ = tr.step(img, ctm, gt_pose, gt_hm)
        host += time.perf_counter() - h0          # time the host needs to ENQUEUE a step (no sync inside)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    print(f"host enqueue time {host / a.steps * 1e3:.2f} ms/step")
    print(f"policy {a.policy}, batch {B}: {dt * 1e3:.2f} ms/step, {B / dt:.1f} frames/s, loss {float(terms.sum()):.4f}, mem {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
    # per-kernel breakdown of one step
    # eager and instrumented even when the timed steps were graph replays - and on ONE stream: with the two-stream reverse pass a
    # launch's event pair would also time whatever the other stream runs beside it
    overlap, train.OVERLAP = train.OVERLAP, False
    hip.PROFILE = []
    tr._run(img, ctm, gt_pose, gt_hm, update=True)
    torch.cuda.synchronize()
    prof, hip.PROFILE = hip.PROFILE, None
    train.OVERLAP = overlap
    if a.dump:
        with open(a.dump, "w") as f:
            for i, (name, s, e, fl, nb, tag) in enumerate(prof):
                us = s.elapsed_time(e) * 1e3
                f.write(f"{i:4d} {us:9.1f} us  {fl / us / 1e6 if fl > 0 else 0:7.1f} TF  {nb / us / 1e3 if nb > 0 else 0:7.0f} GB/s  {name:30s} {tag}\n")
    agg = collections.OrderedDict()
    for name, s, e, fl, nb, tag in prof:
        key = name
        if name == "egr_conv2d_nhwc_f32":
            key = name + (" [dgrad]" if False else "")
        ms = s.elapsed_time(e)
        cur = agg.setdefault(key, [0.0, 0, 0.0])
        cur[0] += ms
        cur[1] += 1
        cur[2] += fl
    tot = sum(v[0] for v in agg.values())
    print(f"instrumented step: {tot:.2f} ms inside {len(prof)} egr launches")
    for k, (ms, n, fl) in sorted(agg.items(), key=lambda kv: -kv[1][0]):
        tf = f"{fl / ms / 1e9:7.1f} TF" if fl > 0 else ""
        print(f"  {k:32s} {ms:8.3f} ms  {n:5d} launches {tf}")
    # the slowest conv launches
    by_tag = collections.OrderedDict()
    for name, s, e, fl, nb, tag in prof:
        if "conv2d" in name:
            cur = by_tag.setdefault((name.replace("egr_", "").replace("_f32", ""), tag), [0.0, 0, 0.0])
            cur[0] += s.elapsed_time(e)
            cur[1] += 1
            cur[2] += fl
    for (name, tag), (ms, n, fl) in sorted(by_tag.items(), key=lambda kv: -kv[1][0])[:60]:
        print(f"    {ms:7.3f} ms x{n:3d} {fl / ms / 1e9 if ms > 0 else 0:7.1f} TF  {name:14s} {tag}")


def accumulate_leg(a, tr, args):
    """Device time per micro-step (event pairs on the step's stream), split into the ones that only accumulate and the one that
    also clips and updates, and the wall time per optimizer update."""
    K = a.accumulate
    for _ in range(a.warmup * K):
        tr.step(*args)
    assert tr.pending_micro_steps() == 0
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps * K + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(a.steps * K):
        terms, _ = tr.step(*args)
        marks[i + 1].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / a.steps
    ms = [marks[i].elapsed_time(marks[i + 1]) for i in range(a.steps * K)]
    plain = [t for i, t in enumerate(ms) if (i + 1) % K]
    upd = [t for i, t in enumerate(ms) if (i + 1) % K == 0]
    res = {"batch": a.batch, "accumulate": K, "graph": bool(a.graph and tr.graph is not None), "updates_timed": a.steps,
           "ms_micro_step_accumulating": sum(plain) / len(plain), "ms_micro_step_updating": sum(upd) / len(upd),
           "ms_per_optimizer_update": wall * 1e3, "optimizer_updates": tr.opt.steps, "loss": float(terms.sum()),
           "mem_gib": torch.cuda.max_memory_allocated() / 2**30}
    print(f"batch {a.batch} x accumulate {K}: {res['ms_micro_step_accumulating']:.2f} ms per accumulating micro-step, "
          f"{res['ms_micro_step_updating']:.2f} ms per updating micro-step, {res['ms_per_optimizer_update']:.2f} ms per optimizer update "
          f"({a.batch * K / wall:.1f} frames/s), mem {res['mem_gib']:.1f} GiB")
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

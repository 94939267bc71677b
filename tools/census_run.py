#!/usr/bin/env python3
"""A long parity census (oracle/census.py) as evidence for profiles/: N frames through the HIP path at batch 64 under the shipped launch
policy against the CPU oracle - all arg-maxes of both heat-map sets, valid masks, four pose sets, tie exposure, float64 referee.
    python tools/census_run.py --frames 2048 --out census.json        (one line of progress per GPU batch)
    python tools/census_run.py --frames 512 --policies shipped,exact,f32 --referee f64 --out referee.json
    python tools/census_run.py --frames 512 --policy shipped,fast,bf16x3 --out 'profiles/fast_policy_census_512_{policy}.json'
                                              (one file per policy in the single-policy layout, same seeds, the oracle computed once)
Test infrastructure (imports oracle/): not part of the product or of bench.py's timed region."""
import argparse, copy, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from egorear_amd import configs, hip, synth
from egorear_amd.estimator import EgoPoseFormerMVFEX
from oracle import census
from oracle import egorear_oracle as O
from oracle import referee as R

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=2048)
ap.add_argument("--seed0", type=int, default=100)
ap.add_argument("--out", default="")
ap.add_argument("--weight-seed", type=int, default=42, help="seed of the synthetic weights (egorear_amd/synth.py); the tests and bench.py use 42")
ap.add_argument("--camera", default="ego4view_syn", choices=["ego4view_syn", "ego4view_rw"], help="camera model / config family (rw: with coord_trans_mat)")
ap.add_argument("--policies", "--policy", default="shipped", help="comma-separated launch policies the GPU forwards run under, on one module "
                "(shipped = the process default, exact = bf16x3 = six products, f32 = fp32 matrix cores, fast = the opt-in one-product "
                "policy of DESIGN.md 5k, whose counts are reported and never gated); the oracle is computed once")
ap.add_argument("--referee", default="", choices=["", "f64"], help="f64: every map is also put before the float64 oracle (oracle/referee.py)")
a = ap.parse_args()
torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
net = EgoPoseFormerMVFEX(**copy.deepcopy(configs.pose3d_cfg(a.camera))).eval()
synth.load_synth(net, a.weight_seed)
sd = {k: v.clone() for k, v in net.state_dict().items()}
net = net.to("cuda:0")
cams = O.make_cameras(a.camera, os.path.join(os.path.dirname(os.path.abspath(synth.__file__)), "calib", "ego4view"))
assert hip.H2 and hip.X6_MIN_ROWS > 0
POLICIES = {"shipped": None, "exact": hip.POLICY.exact(), "bf16x3": hip.POLICY.exact(), "fast": hip.POLICY.fast(),
            "f32": hip.POLICY.replace(w_format="f32", h2=False, layer_h2=False, wgrad_x6=False)}
names = a.policies.split(",")
assert names and all(n in POLICIES for n in names), a.policies
acc, ref, t0 = {n: None for n in names}, {n: None for n in names}, time.time()


def referee_merge(r, part):
    """Additive float64-referee counts of one chunk: arg-max disagreements and valid flips per set (hip and f32), the largest heat-map
    and joint distances from float64."""
    if r is None:
        r = {"sets": [{"maps": 0, "hip_disagreements": 0, "f32_disagreements": 0, "outside_rounding": 0, "valid_flips": 0, "f32_valid_flips": 0,
                       "flips_outside": 0, "max_f64_gap_to_hip": 0.0, "min_f64_to_threshold_of_flips": None} for _ in part],
             "max_heatmap_err_f64": 0.0, "max_joint_err_cm_f64": 0.0}
    for acc_s, p in zip(r["sets"], part):
        for k in ("maps", "hip_disagreements", "f32_disagreements", "outside_rounding", "f32_valid_flips", "flips_outside"):
            acc_s[k] += p[k]
        acc_s["valid_flips"] += len(p["valid_flips"])
        for d in p["disagreements"]:
            acc_s["max_f64_gap_to_hip"] = max(acc_s["max_f64_gap_to_hip"], d["f64_gap_to_hip"])
        for f in p["valid_flips"]:
            m = acc_s["min_f64_to_threshold_of_flips"]
            acc_s["min_f64_to_threshold_of_flips"] = f["f64_to_threshold"] if m is None else min(m, f["f64_to_threshold"])
    return r


nb = a.frames // 64
f32_ref = None
for i in range(nb):
    scale = (1.0, 0.35, 0.6, 1.5)[i % 4]
    img = synth.synth_images(64, 4, seed=a.seed0 + i, scale=scale)
    ctm = synth.synth_coord_trans_mat(64, seed=500 + i) if a.camera == "ego4view_rw" else None
    gpu = {}
    for n in names:
        with hip.use_policy(POLICIES[n]):
            gpu[n] = census.gpu_outputs(net, img.to("cuda:0"), ctm.to("cuda:0") if ctm is not None else None)
    for lo in range(0, 64, 8):
        hi = lo + 8
        o = census.oracle_outputs(sd, cams, img[lo:hi], O, ctm[lo:hi] if ctm is not None else None)
        e = R.reference_outputs(sd, cams, img[lo:hi], ctm[lo:hi] if ctm is not None else None, dtype=torch.float64) if a.referee else None
        if e is not None:
            f32_ref = referee_merge(f32_ref, R.argmax_vs_referee(o["hms"], e["hms"], o["hms"]))
            f32_ref["max_heatmap_err_f64"] = max(f32_ref["max_heatmap_err_f64"], max(float((h.double() - f).abs().max()) for h, f in zip(o["hms"], e["hms"])))
            f32_ref["max_joint_err_cm_f64"] = max(f32_ref["max_joint_err_cm_f64"],
                                                  max(float((p.double() - e["stages"][f"pose_{k}"]).abs().max()) for k, p in enumerate(o["preds"])))
        for n in names:
            g = census._slice(gpu[n], lo, hi)
            part = census.compare_chunk(g, o, sd, img[lo:hi], O, first_frame=i * 64 + lo)
            for d in part["mismatch_detail"]:
                d["batch"], d["seed"], d["scale"] = i, a.seed0 + i, scale
            acc[n] = census.merge(acc[n], part)
            if e is not None:
                r = ref[n] = referee_merge(ref[n], R.argmax_vs_referee(g["hms"], e["hms"], o["hms"]))
                r["max_heatmap_err_f64"] = max(r["max_heatmap_err_f64"], max(float((h.double() - f).abs().max()) for h, f in zip(g["hms"], e["hms"])))
                r["max_joint_err_cm_f64"] = max(r["max_joint_err_cm_f64"],
                                                max(float((p.double() - e["stages"][f"pose_{k}"]).abs().max()) for k, p in enumerate(g["preds"])))
    for n in names:
        c = acc[n]
        extra = ""
        if a.referee:
            extra = ", vs float64: " + " / ".join(f"set {k} {s['hip_disagreements']} ({s['outside_rounding']} outside)" for k, s in enumerate(ref[n]["sets"]))
        print(f"[{n}] batch {i + 1}/{nb} (seed {a.seed0 + i}, scale {scale}): {c['frames']} frames, {c['argmax_mismatches']} mismatches "
              f"({c['argmax_mismatches_outside_rounding']} outside rounding), valid flips {c['valid_mask_mismatches']}, "
              f"max joint err {c['max_joint_err_cm']:.2e} cm{extra}, {time.time() - t0:.0f} s", flush=True)
for n in names:
    acc[n]["policy"] = "shipped (fp16 scheme by size), batch 64" if n == "shipped" else f"{n}, batch 64"
    acc[n]["weight_seed"], acc[n]["camera"] = a.weight_seed, a.camera
    acc[n]["seeds"] = [a.seed0, a.seed0 + nb - 1]
    acc[n]["image_scales"] = [1.0, 0.35, 0.6, 1.5]
if names == ["shipped"] and not a.referee:
    out = acc["shipped"]                                    # (the single-policy layout of the earlier census profiles)
else:
    out = {"policies": acc, "frames": nb * 64}
    if a.referee:
        # (the float32 oracle's own counts against float64: its sets carry no second evaluation, hence no hip_ / f32_ prefixes)
        for st in f32_ref["sets"]:
            st["disagreements"], st["valid_flips_count"] = st.pop("hip_disagreements"), st.pop("valid_flips")
            st["max_f64_gap_to_choice"] = st.pop("max_f64_gap_to_hip")
            del st["f32_disagreements"], st["f32_valid_flips"]
        out["referee_f64"] = {"hip": ref, "f32_oracle": f32_ref, "rounding_gap": census.ROUNDING_GAP}
print(json.dumps(out))
if "{policy}" in a.out:
    for n in names:
        json.dump(acc[n], open(a.out.replace("{policy}", n), "w"), indent=1)
elif a.out:
    json.dump(out, open(a.out, "w"), indent=1)

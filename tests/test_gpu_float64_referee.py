"""The whole inference path against a float64 referee (oracle/referee.py), stage by stage, under three launch policies.

The kernel tests hold every implicit-GEMM launch to "no further from fp64 than the fp32 launch, x1.5 + 1e-7"; the end-to-end tests only
compare with the float32 oracle, at bars 25-100x above the measured error.  Here the drop-in EgoPoseFormerMVFEX (synthetic weights,
seed 42) runs three 64-frame device batches - the benchmarked size, so the role-split / persistent / chained launches are the ones
measured - and a spread of frames of each is compared with the CPU oracle evaluated in float32 and in float64:
  (a) exact / shipped policies: per stage, rms(hip - f64) <= 1.5 rms(hip_f32 - f64) + 1e-7 and max <= 2 max + 1e-7 (relative to the
      f64 values), hip_f32 = the same network under the f32 policy - the kernel tests' bar; the fp16 scheme needs no looser bound;
  (b) f32 policy (fp32 matrix cores everywhere, the stem included): against the float32 CPU oracle, per stage, at rho, the smallest
      ratio by which the backbone's 3x3 fp32 launches one by one already sit further from float64 than the CPU's float32
      convolutions (measured in the same run, fp32_launches);
  (c) every policy: no arg-max disagreement with float64 where float64's own gap between the two positions is >= census.ROUNDING_GAP,
      no `valid` flip where the float64 maximum is >= 1e-6 from 0.5;
  (d) at least 90 % of the compared frames enter every stage (their discrete decisions agree in all three evaluations).
Policies are switched on the SAME module: ambient `hip.use_policy` for one transition, `engine.set_policy` for another (the packs are
keyed by the policy they were made under: egorear_amd.engine.State).  A second test checks that switch launch by launch and bit for bit."""
import copy
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCH = 64
PICK = [0, 5, 13, 22, 31, 38, 46, 55, 63]                               # the compared frames of every batch: first, last and a spread
PLAN = [("ego4view_syn", 21, 1.0), ("ego4view_syn", 22, 0.35), ("ego4view_rw", 23, 1.0)]     # (camera, image seed, image scale)
CONV = ("egr_conv2d_nhwc_f32", "egr_conv1x1_chain_f32")


def _policies():
    from egorear_amd import hip
    return {"shipped": hip.POLICY, "exact": hip.POLICY.exact(),
            "f32": hip.POLICY.replace(w_format="f32", h2=False, layer_h2=False, wgrad_x6=False)}


def _net(camera):
    from egorear_amd import configs, synth
    from egorear_amd.estimator import EgoPoseFormerMVFEX
    net = EgoPoseFormerMVFEX(**copy.deepcopy(configs.pose3d_cfg(camera))).eval()
    synth.load_synth(net, 42)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    return net.to(DEV), sd


def _tags(profile):
    conv = [t for name, *_, t in profile if name in CONV]
    layer = [t for name, *_, t in profile if name == "egr_joint_layer_f32"]
    return {"h2": sum(t.startswith("h2 ") for t in conv), "x6": sum(t.startswith("x6 ") for t in conv), "conv": len(conv),
            "layer_h2": sum(t.startswith("h2") for t in layer), "layer_plain": sum(t.startswith("plain") for t in layer),
            # the stem: split operands (bf16x3 or the fp16 scheme) or the fp32 matrix cores
            "stem_split": sum(name == "egr_stem_conv7x7_x6_f32" for name, *_ in profile),
            "stem_f32": sum(name in ("egr_stem_conv7x7_f32", "egr_stem_conv7x7_pool_f32") for name, *_ in profile)}


@pytest.fixture(scope="module")
def runs(calib_dir):
    """{policy: (hip outputs of the PICK frames of all batches, launch tags per batch)}, the float32 and float64 oracle on the same frames."""
    from egorear_amd import engine, hip, synth
    from oracle import egorear_oracle as O
    from oracle import referee as R
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    pols = _policies()
    nets = {}
    got = {k: [] for k in pols}
    tags = {k: [] for k in pols}
    f32, f64 = [], []
    for camera, seed, scale in PLAN:
        if camera not in nets:
            nets[camera] = _net(camera)
        net, sd = nets[camera]
        img = synth.synth_images(BATCH, 4, seed=seed, scale=scale)
        ctm = synth.synth_coord_trans_mat(BATCH, seed=seed + 500) if camera == "ego4view_rw" else None
        dev_img, dev_ctm = img.to(DEV), (ctm.to(DEV) if ctm is not None else None)

        def forward(name):
            hip.PROFILE = []
            try:
                got[name].append(R.hip_outputs(net, dev_img, dev_ctm, frames=PICK))
                torch.cuda.synchronize()
                tags[name].append(_tags(hip.PROFILE))
            finally:
                hip.PROFILE = None
        # on ONE module: the process default, then exact through the ambient route, then f32 held by the module itself
        forward("shipped")
        with hip.use_policy(pols["exact"]):
            forward("exact")
        engine.set_policy(net, pols["f32"])
        try:
            forward("f32")
        finally:
            engine.set_policy(net, None)
        cams = O.make_cameras(camera, calib_dir)
        sub_ctm = ctm[PICK] if ctm is not None else None
        f32.append(R.reference_outputs(sd, cams, img[PICK], sub_ctm, dtype=torch.float32))
        f64.append(R.reference_outputs(sd, cams, img[PICK], sub_ctm, dtype=torch.float64))
    out = {k: R.concat(v) for k, v in got.items()}
    return {"hip": out, "tags": tags, "f32": R.concat(f32), "f64": R.concat(f64)}


@pytest.fixture(scope="module")
def tables(runs):
    from oracle import referee as R
    res = {}
    for pol, h in runs["hip"].items():
        res[pol] = (R.stage_distances(h, runs["f32"], runs["f64"]), R.argmax_vs_referee(h["hms"], runs["f64"]["hms"], runs["f32"]["hms"]))
    # policy x stage x (rms ratio, max ratio, frames compared, arg-max disagreements hip / f32 vs float64)
    print("\nfloat64 referee: %d frames (%d per batch x %d batches); ratios = distance of the HIP path / of the float32 oracle from float64"
          % (len(PICK) * len(PLAN), len(PICK), len(PLAN)))
    print("%-8s %-13s %10s %10s %12s %12s %7s %s" % ("policy", "stage", "rms ratio", "max ratio", "rms hip", "max hip", "frames", "arg-max hip/f32"))
    for pol, (t, am) in res.items():
        for s in R.STAGES:
            r = t[s]
            sets = {"hm_init": 0, "hm_refined": 1}
            a = "%d/%d" % (am[sets[s]]["hip_disagreements"], am[sets[s]]["f32_disagreements"]) if s in sets else "-"
            if "rms_hip" in r:
                print("%-8s %-13s %10.3f %10.3f %12.3e %12.3e %7d %s" % (pol, s, r["ratio_rms"], r["ratio_max"], r["rms_hip"], r["max_hip"], r["frames"], a))
            else:
                print("%-8s %-13s %10s %10s %12s %12s %7d %s" % (pol, s, "-", "-", "-", "-", r["frames"], a))
        for a in am:
            print("%-8s set %d: %d hip / %d f32 arg-max disagreements with float64 (%d outside rounding), %d hip / %d f32 valid flips (%d outside 1e-6)"
                  % (pol, a["set"], a["hip_disagreements"], a["f32_disagreements"], a["outside_rounding"], len(a["valid_flips"]),
                     a["f32_valid_flips"], a["flips_outside"]))
    return res


def test_shipped_policy_is_the_fp16_scheme(runs):
    from egorear_amd import hip
    assert hip.POLICY.w_format == "f16x2" and hip.H2 and hip.POLICY.layer_h2 and hip.X6_MIN_ROWS > 0 and hip.X6_MIN_FLOPS > 0, \
        "the shipped leg is a statement about the default launch policy"
    for t in runs["tags"]["shipped"]:
        assert t["h2"] >= 35 and t["x6"] <= 3 and t["layer_plain"] == 0 and t["layer_h2"] >= 4 and t["stem_split"] >= 1, t
    for t in runs["tags"]["exact"]:
        assert t["h2"] == 0 and t["x6"] >= 35 and t["layer_h2"] == 0 and t["layer_plain"] >= 4 and t["stem_split"] >= 1, t
    for t in runs["tags"]["f32"]:      # fp32 matrix cores everywhere, the stem included
        assert t["h2"] == 0 and t["x6"] == 0 and t["layer_h2"] == 0 and t["layer_plain"] >= 4 and t["stem_split"] == 0 and t["stem_f32"] >= 1, t


# The backbone's convolutions one launch at a time: the fp32-matrix-core launch and the CPU's float32 F.conv2d (the oracle's), both
# against float64, on ReLU-like activations and He-scaled weights at the trunk's shapes (n, h = w, cin, cout, k, stride).
BACKBONE_LAUNCHES = [(16, 64, 64, 64, 3, 1), (16, 64, 64, 128, 3, 2), (16, 32, 128, 128, 3, 1), (16, 16, 256, 256, 3, 1),
                     (16, 8, 512, 512, 3, 1), (16, 64, 64, 128, 1, 1)]


@pytest.fixture(scope="module")
def fp32_launches():
    """{shape: (rms, max) of the fp32 launch's distance from float64 over the CPU float32 conv's}, relative to the float64 output."""
    import torch.nn.functional as F
    from egorear_amd import hip
    from egorear_amd.engine import pack_conv_weight
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    ws = torch.empty(16 << 20, device=DEV, dtype=torch.float32)
    g = torch.Generator().manual_seed(3)
    out = {}
    for n, h, cin, cout, k, stride in BACKBONE_LAUNCHES:
        x = torch.rand(n, cin, h, h, generator=g)
        w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        pad = k // 2
        ref = F.conv2d(x.double(), w.double(), stride=stride, padding=pad)
        cpu = F.conv2d(x, w, stride=stride, padding=pad).double()
        with hip.use_policy(_policies()["f32"]):
            y = hip.conv2d(hip.Img(x.permute(0, 2, 3, 1).contiguous().to(DEV)), pack_conv_weight(w).to(DEV), cout, k, k, stride, pad, workspace=ws)
        dev = y.t.permute(0, 3, 1, 2).double().cpu()
        rms_r, max_r = float(ref.pow(2).mean().sqrt()), float(ref.abs().max())
        e = [(float((t - ref).pow(2).mean().sqrt()) / rms_r, float((t - ref).abs().max()) / max_r) for t in (dev, cpu)]
        out[(n, h, cin, cout, k, stride)] = (e[0][0] / e[1][0], e[0][1] / e[1][1])
        print("fp32 launch %-26s rms %.2e (cpu %.2e, ratio %.2f)  max %.2e (cpu %.2e, ratio %.2f)"
              % ((n, h, cin, cout, k, stride), e[0][0], e[1][0], e[0][0] / e[1][0], e[0][1], e[1][1], e[0][1] / e[1][1]))
    return out


def test_f32_policy_vs_the_float32_oracle(tables, fp32_launches):
    """The f32 policy against the float32 CPU oracle.  The backbone's 3x3 fp32 launches one by one already sit further from float64
    than the CPU's float32 convolutions - their error grows with K like a sequential fp32 chain (measured: rms ratio ~2 at K = 576 to
    ~5 at K = 4608), the CPU's does not.  The whole network may not exceed the SMALLEST of those launch ratios (rho, measured in this
    run, no margin on top): rms <= rho_rms x the oracle's + 1e-7, max <= rho_max x the oracle's + 1e-7."""
    from oracle import referee as R
    three = [v for key, v in fp32_launches.items() if key[4] == 3]
    rho_rms, rho_max = min(r for r, _ in three), min(m for _, m in three)
    assert rho_rms >= 1.0 and rho_max >= 1.0, fp32_launches
    t = tables["f32"][0]
    for s in R.STAGES:
        r = t[s]
        assert "rms_hip" in r, (s, r)
        assert r["rms_hip"] <= rho_rms * r["rms_f32"] + 1e-7, (s, r, rho_rms)
        assert r["max_hip"] <= rho_max * r["max_f32"] + 1e-7, (s, r, rho_max)


@pytest.mark.parametrize("pol", ["exact", "shipped"])
def test_stages_no_further_from_float64_than_the_fp32_launches(tables, pol):
    """The kernel tests' bar carried to the whole network: per stage, no further from float64 than the same network on the fp32 matrix
    cores (the f32 policy), rms x 1.5 + 1e-7 and max x 2 + 1e-7.  The fp16 scheme (shipped) meets it without a looser bound."""
    from oracle import referee as R
    t, ref = tables[pol][0], tables["f32"][0]
    for s in R.STAGES:
        r, f = t[s], ref[s]
        assert "rms_hip" in r and "rms_hip" in f, (pol, s, r)
        assert r["rms_hip"] <= 1.5 * f["rms_hip"] + 1e-7, (pol, s, r, f)
        assert r["max_hip"] <= 2.0 * f["max_hip"] + 1e-7, (pol, s, r, f)


@pytest.mark.parametrize("pol", ["exact", "f32", "shipped"])
def test_discrete_decisions_agree_with_float64(tables, runs, pol):
    from oracle import census
    t, am = tables[pol]
    for a in am:
        assert a["outside_rounding"] == 0, (pol, a)
        assert a["flips_outside"] == 0, (pol, a)
        for d in a["disagreements"]:
            assert d["f64_gap_to_hip"] < census.ROUNDING_GAP, d
    n = len(PICK) * len(PLAN)
    for s, r in t.items():
        assert r["frames"] >= 0.9 * n, (pol, s, r)


def test_policy_switch_on_one_module_matches_fresh_modules():
    """default -> use_policy(exact) -> default -> use_policy(f32) on ONE module: every forward runs its policy's kernels (conv and fused
    layer tags) and computes, bit for bit, what a fresh module forwarded only under that policy computes."""
    from egorear_amd import hip, synth
    pols = _policies()
    img = synth.synth_images(16, 4, seed=5).to(DEV)

    def run(net, pol):
        hip.PROFILE = []
        try:
            with hip.use_policy(pol), torch.no_grad():
                p, h = net(img)
            torch.cuda.synchronize()
            return [x.clone() for x in p] + [x.clone() for x in h], _tags(hip.PROFILE)
        finally:
            hip.PROFILE = None
    net, _ = _net("ego4view_syn")
    seq = [("shipped", None), ("exact", pols["exact"]), ("shipped", None), ("f32", pols["f32"])]
    outs = [(name,) + run(net, pol) for name, pol in seq]
    del net
    for name, pol in (("shipped", None), ("exact", pols["exact"]), ("f32", pols["f32"])):
        fresh, _ = _net("ego4view_syn")
        ref, rtags = run(fresh, pol)
        del fresh
        for n, o, t in outs:
            if n != name:
                continue
            assert t == rtags, (name, t, rtags)
            assert all(torch.equal(a, b) for a, b in zip(o, ref)), name
        if name == "shipped":
            assert rtags["h2"] >= 30 and rtags["layer_plain"] == 0 and rtags["layer_h2"] >= 4, rtags
        else:
            assert rtags["h2"] == 0 and rtags["layer_h2"] == 0 and rtags["layer_plain"] >= 4, rtags
            assert (rtags["x6"] >= 30) if name == "exact" else (rtags["x6"] == 0), rtags

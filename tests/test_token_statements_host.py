"""oracle/token_statements.py on the CPU: the plain statements of the three fused token kernels are (a) the oracle's own arithmetic,
to 1e-10 in float64, on the synthetic network's weights, and (b) evaluated on inputs that expose every term - each deliberate error
(token_statements.MUTATIONS) moves the float64 result by more than 100 x the float32-vs-float64 distance in every kernel-test case
in which the term occurs.  The GPU comparison (tests/test_gpu_token_kernels_f64.py) rests on both."""
import copy
import os

import pytest
import torch

from oracle import egorear_oracle as O
from oracle import referee as R
from oracle import token_statements as T

REFINER = "heatmap_estimator.heatmap_refiner_front_left"
POSE3D = "pose3d_estimator"


@pytest.fixture(scope="module")
def sd():
    from egorear_amd import configs, synth
    from egorear_amd.estimator import EgoPoseFormerMVFEX
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    net = EgoPoseFormerMVFEX(**copy.deepcopy(configs.pose3d_cfg("ego4view_syn"))).eval()
    return {k: v.clone() for k, v in synth.load_synth(net, 42).items()}


def _f64(sd, prefix, skip=()):
    return {k: v.double() for k, v in sd.items() if k.startswith(prefix) and v.is_floating_point() and not any(s in k for s in skip)}


def _same(got, ref, what):
    scale = float(ref.abs().max())
    assert got.shape == ref.shape, what
    err = float((got - ref).abs().max())
    assert scale > 0 and err <= 1e-10 * scale, f"{what}: {err:.3e} of {scale:.3e}"


def _layer_weights(sdd, p, pre_w, pre_b):
    """The layer's parameters under the descriptor's names, float64, one query set; w_fold / c_fold as engine.pack_layers folds them."""
    ca, sa = p + ".cross_attn", p + ".spatial_attn"
    Wv, bv = sdd[ca + ".value_proj.weight"], sdd[ca + ".value_proj.bias"]
    Wp = pre_w.reshape(pre_w.shape[0], -1)
    u = lambda t: t.unsqueeze(0)                                               # noqa: E731
    return {"w_fold": u(Wv @ Wp), "c_fold": u(Wv @ pre_b + bv), "w_out": u(sdd[ca + ".output_proj.weight"]), "b_out": u(sdd[ca + ".output_proj.bias"]),
            "w_fuse": u(sdd[p + ".fuse_mlp.weight"]), "b_fuse": u(sdd[p + ".fuse_mlp.bias"]),
            "ln1_g": u(sdd[p + ".norm_cross.weight"]), "ln1_b": u(sdd[p + ".norm_cross.bias"]),
            "w_qkv": u(torch.cat([sdd[f"{sa}.{n}_proj.weight"] for n in "qkv"], 0)), "b_qkv": u(torch.cat([sdd[f"{sa}.{n}_proj.bias"] for n in "qkv"], 0)),
            "w_mo": u(sdd[sa + ".out_proj.weight"]), "b_mo": u(sdd[sa + ".out_proj.bias"]),
            "ln2_g": u(sdd[p + ".norm_spatial.weight"]), "ln2_b": u(sdd[p + ".norm_spatial.bias"]),
            "w_f0": u(sdd[p + ".ffn.layers.0.0.weight"]), "b_f0": u(sdd[p + ".ffn.layers.0.0.bias"]),
            "w_f1": u(sdd[p + ".ffn.layers.1.weight"]), "b_f1": u(sdd[p + ".ffn.layers.1.bias"]),
            "ln3_g": u(sdd[p + ".norm_ffn.weight"]), "ln3_b": u(sdd[p + ".norm_ffn.bias"])}


@pytest.mark.parametrize("which", ["refiner", "lifting"])
def test_layer_statement_is_the_oracles_transformer_layer(sd, which):
    """Refiner 0's layer (C = 256, positional table) and the lifting head's first layer (C = 128) on an 8 x 8 memory: the sampled
    operands g / sigma / e come from the oracle's own msda_core on the UN-projected features, a ones map and the projected positions;
    the statement on them and the folded weights is O.joint_transformer_layer on the projected memory."""
    B, V, H, Wd = 2, 4, 8, 8
    gen = torch.Generator().manual_seed(5)
    if which == "refiner":
        p, pre, C, J = REFINER + ".transformer_layers.0", REFINER + ".frame_feat_multi_view_proj", 256, 15
        sdd = _f64(sd, REFINER)
        pos = sdd[REFINER + ".frame_feat_multi_view_pos_embed"][:, :, :H * Wd].contiguous()           # (1, V, HW, C)
    else:
        p, pre, C, J = POSE3D + ".layers.0", POSE3D + ".feat_proj", 128, 16
        sdd = _f64(sd, POSE3D, skip=("mlp_pred.0", "mlp_pred.1"))
        pos = None
    heads, P, dh = 4, 16, C // 4
    f = torch.randn(B, V, H * Wd, 128, generator=gen, dtype=torch.float64)
    x = torch.randn(B, J, C, generator=gen, dtype=torch.float64)
    anchors = torch.rand(B, V, J, 2, generator=gen, dtype=torch.float64)
    valid = torch.rand(B, V, J, generator=gen) > 0.3
    assert valid.any() and not valid.all()
    pre_w, pre_b = sdd[pre + ".weight"], sdd[pre + ".bias"]
    mem = f @ pre_w.reshape(C, 128).t() + pre_b
    if pos is not None:
        mem = mem + pos
    ref = O.joint_transformer_layer(sdd, p, x, mem, anchors, valid, H, Wd)
    # the kernel's sampled operands, by the oracle's sampler
    ca = p + ".cross_attn"
    off = O._lin(sdd, ca + ".sampling_offsets", x).view(B, J, heads, P, 2)
    aw = torch.softmax(O._lin(sdd, ca + ".attention_weights", x).view(B, J, heads, P), -1)
    Wv = sdd[ca + ".value_proj.weight"]
    g, sg, e = [], [], []
    for v in range(V):
        loc = anchors[:, v][:, :, None, None, :] + off / torch.tensor([Wd, H], dtype=torch.float64)
        g.append(O.msda_core(f[:, v][:, :, None, :].expand(B, H * Wd, heads, 128), H, Wd, loc, aw).view(B, J, heads, 128))
        sg.append(O.msda_core(torch.ones(B, H * Wd, heads, 1, dtype=torch.float64), H, Wd, loc, aw).view(B, J, heads))
        if pos is not None:
            e.append(O.msda_core((pos[0, v] @ Wv.t()).view(1, H * Wd, heads, dh).expand(B, -1, -1, -1), H, Wd, loc, aw))
    g = torch.stack(g, 2).reshape(B * J * V, heads, 128)
    sigma = torch.stack(sg, 2).permute(3, 0, 1, 2).reshape(1, heads, B * J * V)
    e = torch.stack(e, 2).reshape(B * J * V, C) if e else None
    rowmask = valid.permute(0, 2, 1).reshape(-1).to(torch.uint8)
    assert float(sigma.min()) < 0.999 and float(sigma.max()) > 0.5               # some samples fall off the map, most do not
    got = T.joint_layer(x.reshape(B * J, C), g, e, sigma, rowmask, _layer_weights(sdd, p, pre_w, pre_b), B, J, V, C, 1)
    _same(got["x_out"].view(B, J, C), ref, which + " layer")


def _recording_lin(monkeypatch):
    """O._lin with its calls recorded: {parameter prefix: [(input, output), ...]}"""
    calls = {}
    real = O._lin

    def lin(sd_, p, x):
        y = real(sd_, p, x)
        calls.setdefault(p, []).append((x, y))
        return y
    monkeypatch.setattr(O, "_lin", lin)
    return calls


def test_jqa_statement_is_the_oracles_query(sd, monkeypatch):
    """O.heatmap_mvf's JQA query (cap["query"]) and the offsets / logits its transformer layer derives from it, against the statement
    on t = ReLU(heatmap_proj[0](heat map)) and the stride-32 features in NHWC."""
    B, V, J, H, Wd = 2, 4, 15, 64, 64
    gen = torch.Generator().manual_seed(6)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)         # noqa: E731
    sdd = _f64(sd, REFINER)
    calls = _recording_lin(monkeypatch)
    cap = {}
    s32 = torch.relu(rn(B, 512, 3, 5))
    with torch.no_grad():
        O.heatmap_mvf(sdd, REFINER, rn(B, J, H, Wd), rn(B, 128, H, Wd), rn(B, V, 128, H, Wd), torch.rand(B, V, J, 2, generator=gen, dtype=torch.float64),
                      torch.rand(B, V, J, generator=gen) > 0.3, s32, cap=cap)
    t = calls[REFINER + ".heatmap_proj.2"][0][0]                               # = ReLU(heatmap_proj[0](.)), (B, J, C)
    ca = REFINER + ".transformer_layers.0.cross_attn"
    assert calls[ca + ".sampling_offsets"][0][0] is cap["query"]
    ol = torch.cat([calls[ca + ".sampling_offsets"][0][1], calls[ca + ".attention_weights"][0][1]], -1)
    u = lambda k: sdd[REFINER + k].unsqueeze(0)                                 # noqa: E731
    W = {"w_hp2": u(".heatmap_proj.2.weight"), "b_hp2": u(".heatmap_proj.2.bias"), "w_bfb": u(".fc_bfb.weight"), "b_bfb": u(".fc_bfb.bias"),
         "embed": u(".joint_query_embed.weight"), "w_q": u(".fc_query.0.weight"), "b_q": u(".fc_query.0.bias"),
         "w_ol": torch.cat([sdd[ca + ".sampling_offsets.weight"], sdd[ca + ".attention_weights.weight"]], 0).unsqueeze(0),
         "b_ol": torch.cat([sdd[ca + ".sampling_offsets.bias"], sdd[ca + ".attention_weights.bias"]], 0).unsqueeze(0)}
    got = T.jqa_query(t.reshape(B * J, -1), s32.permute(0, 2, 3, 1).contiguous(), W, B, J, 1)
    _same(got["x"].view(B, J, -1), cap["query"], "query")
    _same(got["ol"].view(B, J, -1), ol, "offsets / logits")


@pytest.mark.parametrize("camera", ["ego4view_syn", "ego4view_rw"])
def test_pose_statement_is_the_oracles_lifting_head(sd, calib_dir, camera):
    """The lines of O.pose3d_forward between mlp_pred[1] and the first decoder layer (mlp_pred[2], the reprojection with its in-place
    chain in syn mode, the joint index column, query_gen_mlp) and the first layer's offsets / logits, piece by piece as that function
    calls them, against the statement."""
    from egorear_amd import synth
    B, J, p = 3, 16, POSE3D
    sdd = _f64(sd, POSE3D, skip=("mlp_pred.0", "mlp_pred.1"))
    gen = torch.Generator().manual_seed(7)
    h1 = torch.randn(B, 128, generator=gen, dtype=torch.float64)
    # body-like proposals instead of the synthetic bias (whose joints sit within centimetres of the optical axes' origin)
    sdd[p + ".mlp_pred.2.bias"] = (torch.rand(3 * J, generator=gen, dtype=torch.float64) * 60 - 30) + torch.tensor([0.0, 10.0, 90.0], dtype=torch.float64).repeat(J)
    sdd[p + ".mlp_pred.2.bias"][5::24] -= 200.0                                # (z of joints 1 and 9: behind the cameras)
    ctm = synth.synth_coord_trans_mat(B).double() if camera == "ego4view_rw" else None
    cams = O.make_cameras(camera, calib_dir)
    camd = R.cameras_as(cams, torch.float64)
    mlp_pred = O._lin(sdd, p + ".mlp_pred.2", h1).reshape(B, -1, 3)
    anchors_3d = mlp_pred.clone().detach()
    anchors_2d, anchors_valid = O.reproject_3d_to_2d(camd, anchors_3d, ctm)
    joint_inds = (torch.arange(1, J + 1).to(torch.float64).reshape(1, J, 1).repeat(B, 1, 1)) / float(J)
    q = torch.cat((joint_inds, anchors_3d), dim=-1)
    q = torch.relu(O._lin(sdd, p + ".query_gen_mlp.0", q))
    q = torch.relu(O._lin(sdd, p + ".query_gen_mlp.2", q))
    x = O._lin(sdd, p + ".query_gen_mlp.4", q)
    ca = p + ".layers.0.cross_attn"
    ol = torch.cat([O._lin(sdd, ca + ".sampling_offsets", x), O._lin(sdd, ca + ".attention_weights", x)], -1)
    W = {"w_m2": sdd[p + ".mlp_pred.2.weight"], "b_m2": sdd[p + ".mlp_pred.2.bias"],
         "w_ol": torch.cat([sdd[ca + ".sampling_offsets.weight"], sdd[ca + ".attention_weights.weight"]], 0),
         "b_ol": torch.cat([sdd[ca + ".sampling_offsets.bias"], sdd[ca + ".attention_weights.bias"]], 0)}
    for i in (0, 2, 4):
        W[f"w_qg{i}"], W[f"b_qg{i}"] = sdd[f"{p}.query_gen_mlp.{i}.weight"], sdd[f"{p}.query_gen_mlp.{i}.bias"]
    got = T.pose_query(h1, ctm, cams, W, B, J)
    _same(got["pred"], mlp_pred, "proposal")
    _same(got["anchors_3d"], anchors_3d, "anchors_3d")
    _same(got["anchors_2d"], anchors_2d, "anchors_2d")
    assert torch.equal(got["valid"], anchors_valid) and anchors_valid.any() and not anchors_valid.all()
    _same(got["x"].view(B, J, -1), x, "decoder query")
    _same(got["ol"].view(B, J, -1), ol, "offsets / logits")
    if camera == "ego4view_syn":                                               # F7: the four chained offsets leave (+12, 0, 0)
        _same(got["anchors_3d"] - got["pred"], torch.tensor([12.0, 0.0, 0.0], dtype=torch.float64).expand(B, J, 3), "chain")
    else:
        assert torch.equal(got["anchors_3d"], got["pred"])
    uv = T.unclamped_uv(h1, ctm, cams, W, B, J)
    assert torch.equal(uv.clamp(0.0, 1.0), anchors_2d)


# --------------------------------------------------------------------------- the kernel tests' inputs expose every term

def _layer_names(pred):
    return [n for n, (C, G, B, J, kw) in T.LAYER_CASES.items() if pred(C, G, B, J, kw)]


# mutation -> the kernel-test cases whose result contains the term (a frame that is entirely masked shows nothing of the sampled rows;
# one token has a trivial softmax)
SHOWS = {
    "no_c_fold_sigma": ("layer", _layer_names(lambda C, G, B, J, kw: B > 1)),
    "no_e": ("layer", _layer_names(lambda C, G, B, J, kw: B > 1 and kw.get("e"))),
    "mask_before_bias": ("layer", list(T.LAYER_CASES)),
    "views_reversed": ("layer", _layer_names(lambda C, G, B, J, kw: B > 1)),
    "wrong_c_scale": ("layer", _layer_names(lambda C, G, B, J, kw: J > 1)),
    "tanh_gelu": ("layer", list(T.LAYER_CASES)),
    "no_bfb": ("jqa", list(T.JQA_CASES)),
    "no_chain": ("pose", [n for n, (B, ol_n, rw) in T.POSE_CASES.items() if not rw]),
    "align_corners_false": ("layer", _layer_names(lambda C, G, B, J, kw: kw.get("head"))),
}


@pytest.fixture(scope="module")
def evaluated(calib_dir):
    """{(kind, case): (case, float64 statement, float32 statement, runner(dtype, mutate))} of every unit-scale kernel-test case"""
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    out = {}
    for n in T.LAYER_CASES:
        c = T.layer_case(n)
        out["layer", n] = (c, lambda dt, mu=(), c=c: T.layer_statement(c, dt, mu))
    for n in T.JQA_CASES:
        c = T.jqa_case(n)
        out["jqa", n] = (c, lambda dt, mu=(), c=c: T.jqa_statement(c, dt, mu))
    for n in T.POSE_CASES:
        c = T.pose_case(n)
        cams = O.make_cameras(c["camera"], calib_dir)
        out["pose", n] = (c, lambda dt, mu=(), c=c, cams=cams: T.pose_statement(c, cams, dt, mu))
    return {k: (c, run(torch.float64), run(torch.float32), run) for k, (c, run) in out.items()}


def test_the_case_tables_cover_the_mutations():
    assert set(SHOWS) == set(T.MUTATIONS) and all(names for _, names in SHOWS.values())
    assert len(SHOWS["no_e"][1]) >= 3 and len(SHOWS["align_corners_false"][1]) == 3 and len(SHOWS["no_chain"][1]) == 2


@pytest.mark.parametrize("mutation", T.MUTATIONS)
def test_every_deliberate_error_moves_the_statement_by_100_float32_distances(evaluated, mutation):
    kind, names = SHOWS[mutation]
    for n in names:
        _, f64, f32, run = evaluated[kind, n]
        mut = run(torch.float64, (mutation,))
        ratios = {}
        for k, ref in f64.items():
            if ref.dtype == torch.bool:
                continue
            ratios[k] = T.distances(mut[k], ref)[0] / max(T.distances(f32[k], ref)[0], 1e-300)     # (the rms measure E of the kernel test)
        assert max(ratios.values()) > 100.0, (mutation, kind, n, ratios)


def test_float32_and_float64_agree_wherever_nothing_was_changed(evaluated):
    """(sanity of the yardstick: the float32 statement sits at rounding distance from the float64 one at unit scale)"""
    for (kind, n), (_, f64, f32, _) in evaluated.items():
        for k, ref in f64.items():
            if ref.dtype != torch.bool:
                e, m = T.distances(f32[k], ref)
                assert e < 1e-5 and m < 1e-4, (kind, n, k, e, m)


@pytest.mark.parametrize("name", list(T.POSE_CASES))
def test_pose_case_flags_are_decided_clear_of_the_image_border(evaluated, calib_dir, name):
    """What the kernel test's treatment of `valid` rests on: at most 2 % of a case's flags lie within 1e-4 of the border in float64,
    float32 agrees with float64 on all the others, both values occur, and no joint sits on an optical axis (x = y = 0: atan(z / 0))."""
    c, f64, f32, _ = evaluated["pose", name]
    cams = O.make_cameras(c["camera"], calib_dir)
    uv = T.pose_uv(c, cams, torch.float64)
    keep = torch.minimum(uv.abs(), (uv - 1).abs()).amin(-1) >= 1e-4
    assert float((~keep).float().mean()) <= 0.02
    assert torch.equal(f64["valid"][keep], f32["valid"][keep])
    assert torch.equal(f64["valid"], ((uv > 0) & (uv < 1)).all(-1))
    assert f64["valid"].any() and not f64["valid"].all()
    for b in range(c["B"]):
        assert f64["valid"][b].any() and not f64["valid"][b].all()
    for out in (f64, f32):
        assert torch.isfinite(out["anchors_2d"]).all()
    if c["ctm"] is None:
        # the in-place chain visits (x + 6, y), (x, y), (-x - 6, 37 - y), (x + 12, y): none of them on an axis
        x, y = f64["pred"][..., 0], f64["pred"][..., 1]
        for px, py in ((x + 6, y), (x, y), (-x - 6, 37 - y), (x + 12, y)):
            assert float(torch.sqrt(px * px + py * py).min()) > 1.0

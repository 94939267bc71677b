"""Plain statements of what the fused token kernels compute (egr_joint_layer_f32, egr_jqa_query_f32, egr_pose_query_f32), in the
operand layout of include/egorear_hip.h.  TEST INFRASTRUCTURE ONLY (oracle/ header rule).

Each function takes the kernels' operands as plain row-major CPU tensors (no packing, no state dict), works in the dtype of its
inputs (float32 or float64) and returns a dict of outputs.  They are written from the descriptor comments of include/egorear_hip.h
(egr_layer_desc, egr_jqa_query_desc, egr_pose_query_desc) and the reference lines quoted there, and are tied to the oracle
(egorear_oracle.joint_transformer_layer, heatmap_mvf, pose3d_forward) in float64 by tests/test_token_statements_host.py - so a
kernel test that compares with them compares with the reference's own arithmetic, not with a transcription of the kernel.

`mutate`: names of deliberate errors (MUTATIONS).  The host test evaluates the float64 statement with each of them on the inputs of
make_*_case and requires the result to move by more than 100 x the float32-vs-float64 distance: inputs on which a kernel with
that error would pass are not test inputs.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch
import torch.nn.functional as F

from . import egorear_oracle as O
from .referee import cameras_as

MUTATIONS = ("no_c_fold_sigma", "no_e", "mask_before_bias", "views_reversed", "wrong_c_scale", "tanh_gelu", "no_bfb", "no_chain",
             "align_corners_false")
# The seed of make_*_case.  Chosen on the CPU among 0..39 for the host test's conditions: every deliberate error shows at more than
# 100 float32 distances in every case that contains its term (the closest one, tanh- for erf-GELU, at 213 with this seed; 35 - 194 with
# the others, every other error far above), and float32 and float64 agree on every `valid` flag of the pose cases.
SEED = 21
V, HEADS, CF, FFN, KB, HN = 4, 4, 128, 512, 512, 64


def _lin(x, w, b):
    """x (G, rows, k), w (G, n, k), b (G, n) -> (G, rows, n)"""
    return torch.matmul(x, w.transpose(-1, -2)) + b[:, None, :]


def _ln(x, g, b):
    """LayerNorm over the last dim, eps 1e-5, per-group affine (G, c) on x (G, rows, c)"""
    return F.layer_norm(x, (x.shape[-1],), None, None, 1e-5) * g[:, None, :] + b[:, None, :]


def _gelu(x, mutate):
    return F.gelu(x, approximate="tanh" if "tanh_gelu" in mutate else "none")


def joint_layer(x, g, e, sigma, rowmask, W: Dict[str, torch.Tensor], B: int, J: int, V: int, C: int, G: int, ol: Optional[dict] = None,
                post: Optional[dict] = None, reg: Optional[dict] = None, head: Optional[dict] = None, *, mutate: Sequence[str] = ()):
    """egr_layer_desc.  x (G*B*J, C); g (G*B*J*V, 4, 128), e (G*B*J*V, C) | None, sigma (G, 4, B*J*V), rowmask (B*J*V) with sampled rows
    ordered (frame, joint, view); W: (G, out, in) weights, (G, out) vectors under the descriptor's names; ol = {"w", "b"},
    post = {"g", "b"}, reg = {"w0", "b0", "w2", "b2", "anchors"}, head = {"w" (G, 64, J), "b" (G, 64)}.
    -> {"x_out", "ol", "xn", "pred", "h0"} (the tails that were asked for)."""
    dh = C // HEADS
    rows = B * J * V
    gg = g.reshape(G, rows, HEADS, CF)
    # value projection per head on the sampled features, the folded bias weighted by the in-bounds mass, the sampled positions
    wf = W["w_fold"].reshape(G, HEADS, dh, CF)
    a = torch.einsum("grhk,ghdk->grhd", gg, wf)
    if "no_c_fold_sigma" not in mutate:
        a = a + W["c_fold"].reshape(G, 1, HEADS, dh) * sigma.reshape(G, HEADS, rows).transpose(1, 2)[..., None]
    a = a.reshape(G, rows, C)
    if e is not None and "no_e" not in mutate:
        a = a + e.reshape(G, rows, C)
    keep = (rowmask.reshape(1, rows, 1) != 0)
    zero = torch.zeros((), dtype=x.dtype)
    if "mask_before_bias" in mutate:
        o = torch.where(keep, torch.matmul(a, W["w_out"].transpose(-1, -2)), zero) + W["b_out"][:, None, :]
    else:
        o = torch.where(keep, _lin(a, W["w_out"], W["b_out"]), zero)           # masked_fill(~valid) behind output_proj: the bias goes too
    o = o.reshape(G, B * J, V, C)
    if "views_reversed" in mutate:
        o = o.flip(2)
    x0 = x.reshape(G, B * J, C)
    t = _ln(x0 + _lin(o.reshape(G, B * J, V * C), W["w_fuse"], W["b_fuse"]), W["ln1_g"], W["ln1_b"])
    # joint-to-joint attention, 4 heads over the J tokens of a frame
    qkv = _lin(t, W["w_qkv"], W["b_qkv"]).reshape(G, B, J, 3, HEADS, dh)
    q, k, v = (qkv[:, :, :, i].permute(0, 1, 3, 2, 4) for i in range(3))     # (G, B, heads, J, dh)
    scale = ((384 - C) // HEADS if "wrong_c_scale" in mutate else dh) ** -0.5
    att = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * scale, dim=-1)
    m = torch.matmul(att, v).permute(0, 1, 3, 2, 4).reshape(G, B * J, C)
    t = _ln(t + _lin(m, W["w_mo"], W["b_mo"]), W["ln2_g"], W["ln2_b"])
    f = _lin(_gelu(_lin(t, W["w_f0"], W["b_f0"]), mutate), W["w_f1"], W["b_f1"])
    xo = _ln(t + f, W["ln3_g"], W["ln3_b"])
    out = {"x_out": xo.reshape(G * B * J, C)}
    if ol is not None:
        out["ol"] = _lin(xo, ol["w"], ol["b"]).reshape(G * B * J, -1)
    if post is not None:
        xn = _ln(xo, post["g"], post["b"])
        out["xn"] = xn.reshape(G * B * J, C)
        if reg is not None:
            h = _gelu(_lin(xn, reg["w0"], reg["b0"]), mutate)
            out["pred"] = (_lin(h, reg["w2"], reg["b2"]) + reg["anchors"].reshape(G, B * J, 3)).reshape(G * B * J, 3)
        if head is not None:
            s = int(round(C ** 0.5))
            img = xn.reshape(G, B, J, s * s)                                  # the joints are the channels of an s x s image
            h0 = torch.relu(torch.einsum("gbjp,gnj->gbnp", img, head["w"]) + head["b"][:, None, :, None])
            h0 = F.interpolate(h0.reshape(G * B, -1, s, s), scale_factor=2, mode="bilinear", align_corners="align_corners_false" not in mutate)
            out["h0"] = h0.permute(0, 2, 3, 1).contiguous()                   # NHWC (G*B, 2s, 2s, 64)
    return out


def jqa_query(t, s32, W: Dict[str, torch.Tensor], B: int, J: int, G: int, *, mutate: Sequence[str] = ()):
    """egr_jqa_query_desc.  t (G*B*J, C) = ReLU(heatmap_proj[0](heat map)); s32 (G*B, h, w, 512) NHWC; W: w_hp2, b_hp2, w_bfb, b_bfb,
    embed (G, J, C), w_q, b_q, w_ol, b_ol.  -> {"x", "ol"}."""
    C = t.shape[-1]
    hm_embed = _lin(t.reshape(G, B * J, C), W["w_hp2"], W["b_hp2"]).reshape(G, B, J, C)
    pooled = s32.reshape(G, B, -1, s32.shape[-1]).mean(dim=2)                 # adaptive_avg_pool2d(., (1, 1))
    bfb = _lin(pooled, W["w_bfb"], W["b_bfb"])[:, :, None, :]
    q = W["embed"][:, None]
    if "no_bfb" not in mutate:
        q = q + bfb
    q = (q + hm_embed).reshape(G, B * J, C)
    x = torch.relu(_lin(q, W["w_q"], W["b_q"]))
    return {"x": x.reshape(G * B * J, C), "ol": _lin(x, W["w_ol"], W["b_ol"]).reshape(G * B * J, -1)}


def pose_query(h1, ctm, cams: Sequence[O.FishEye], W: Dict[str, torch.Tensor], B: int, J: int, *, mutate: Sequence[str] = ()):
    """egr_pose_query_desc.  h1 (B, C); ctm (B, 4, 4, 4) | None; cams: the oracle's four FishEye cameras of the mode (syn: ctm None);
    W: w_m2 (3 J, C), b_m2, w_qg0 (C, 4), b_qg0, w_qg2, b_qg2, w_qg4, b_qg4, w_ol, b_ol.
    -> {"pred", "anchors_3d", "anchors_2d", "valid", "x", "ol"}."""
    dt = h1.dtype
    camd = cameras_as(cams, dt)
    pred = F.linear(h1, W["w_m2"], W["b_m2"]).reshape(B, J, 3)
    a3 = pred.clone()
    m = ctm.to(dt) if ctm is not None else None
    if "no_chain" in mutate and ctm is None:                                  # every camera from the untouched proposal
        parts = [c.world2camera(pred.clone(), None) for c in camd]
        a2, ok = torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1)
    else:
        a2, ok = O.reproject_3d_to_2d(camd, a3, m)                            # syn: mutates a3 through the four chained offsets (F7)
    idx = (torch.arange(1, J + 1, dtype=dt).reshape(1, J, 1).repeat(B, 1, 1)) / float(J)
    q = torch.cat((idx, a3), dim=-1)
    q = torch.relu(F.linear(q, W["w_qg0"], W["b_qg0"]))
    q = torch.relu(F.linear(q, W["w_qg2"], W["b_qg2"]))
    x = F.linear(q, W["w_qg4"], W["b_qg4"])
    return {"pred": pred, "anchors_3d": a3, "anchors_2d": a2, "valid": ok, "x": x.reshape(B * J, -1),
            "ol": F.linear(x, W["w_ol"], W["b_ol"]).reshape(B * J, -1)}


def unclamped_uv(h1, ctm, cams: Sequence[O.FishEye], W: Dict[str, torch.Tensor], B: int, J: int) -> torch.Tensor:
    """(B, 4, J, 2): pose_query's projections BEFORE the clamp to [0, 1] - the quantity `valid` is decided on (utils/camera_models.py:
    70-101 behind FishEye.camera_relative, which carries the in-place chain in syn mode).  The kernel tests compare a flag only where
    this, in float64, is clear of 0 and 1."""
    dt = h1.dtype
    a3 = F.linear(h1, W["w_m2"], W["b_m2"]).reshape(B, J, 3).clone()
    uv = []
    for i, cam in enumerate(cameras_as(cams, dt)):
        p = cam.camera_relative(a3, ctm[:, i].to(dt) if ctm is not None else None)
        x, y, z = p[..., 0], p[..., 1], p[..., 2]
        norm = torch.sqrt(x * x + y * y)
        theta = torch.atan(-z / norm)
        rho = sum(a * theta ** k for k, a in enumerate(cam.poly))
        uv.append(torch.stack(((x / norm * rho + cam.image_center[0]) / cam.image_size[1],
                               (y / norm * rho + cam.image_center[1]) / cam.image_size[0]), dim=-1))
    return torch.stack(uv, dim=1)


# --------------------------------------------------------------------------- distances

def distances(v: torch.Tensor, ref64: torch.Tensor):
    """E = rms(v - ref) / rms(ref), M = max|v - ref| / max|ref| in float64 (0 / 0 = 0)."""
    r = ref64.double()
    d = v.double().cpu() - r
    rms, mx = float(r.pow(2).mean().sqrt()), float(r.abs().max())
    e, m = float(d.pow(2).mean().sqrt()), float(d.abs().max())
    return (e / rms if rms > 0 else e), (m / mx if mx > 0 else m)


# --------------------------------------------------------------------------- inputs of the kernel tests

# The smallest shapes at which the kernels' indexing differs (tests/test_gpu_token_kernels_f64.py runs them, the host test checks
# that their inputs expose every term).  Layer: (C, G, B, J, make_layer_case keywords).
_HEAD = dict(e=True, post=True, head=True)
LAYER_CASES = {
    "lift_all_tails": (128, 1, 1, 16, dict(ol_n=192, post=True, reg=True)),       # one frame, entirely masked
    "lift_ol_only": (128, 1, 3, 16, dict(ol_n=192)),
    "refiner_xcd_map": (256, 4, 2, 15, _HEAD),                                     # G * B = 8: query sets mapped to XCDs
    "refiner_plain_map": (256, 4, 3, 15, _HEAD),                                   # G * B = 12: the plain mapping with G > 1
    "refiner_no_tail": (256, 2, 4, 15, dict(e=True)),
    "seven_joints": (128, 2, 1, 7, dict(ol_n=16, post=True, reg=True)),            # 28 sampled rows: the second half is empty; ol_n < 16 * waves
    "one_joint": (256, 1, 2, 1, _HEAD),
}
SCALED = ("refiner_xcd_map", "refiner_plain_map", "lift_all_tails")                # also at the off-unit scales (x, g) below
SCALES = ((3e4, 1e5), (1e-6, 1e-7))
# (G, B, J, s32 (h, w), ol_n)
JQA_CASES = {
    "four_sets": (4, 2, 15, (8, 8), 192),
    "pool_tail": (2, 3, 15, (3, 5), 16),                                           # 15 pooled positions: one group of 8 and the scalar tail
    "one_pixel": (1, 1, 16, (1, 1), 192),
    "one_joint": (1, 1, 1, (1, 1), 16),
}
# (B, ol_n, rw)
POSE_CASES = {"syn_b1": (1, 192, False), "syn_b5": (5, 16, False), "rw_b1": (1, 16, True), "rw_b5": (5, 192, True)}


def layer_case(name: str, scale=None) -> dict:
    C, G, B, J, kw = LAYER_CASES[name]
    xs, gs = scale if scale is not None else (1.0, 1.0)
    return make_layer_case(C, G, B, J, xs=xs, gs=gs, **kw)


def jqa_case(name: str) -> dict:
    G, B, J, hw, ol_n = JQA_CASES[name]
    return make_jqa_case(G, B, J, hw, ol_n)


def pose_case(name: str) -> dict:
    B, ol_n, rw = POSE_CASES[name]
    return make_pose_case(B, ol_n, rw)


class _Rnd:
    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def __call__(self, *shape, scale=1.0):
        return (torch.rand(*shape, generator=self.g) * 2 - 1) * scale


def _frame_mask(r: _Rnd, B: int, per_frame: int) -> torch.Tensor:
    """frame 0 all zero, frame 1 (where there is one) all ones, the rest mixed"""
    m = (r(B, per_frame) > -0.4).to(torch.uint8)
    m[0] = 0
    if B > 1:
        m[1] = 1
    return m


def make_layer_case(C: int, G: int, B: int, J: int, *, e: bool = False, ol_n: int = 0, post: bool = False, reg: bool = False,
                    head: bool = False, xs: float = 1.0, gs: float = 1.0, seed: int = SEED) -> dict:
    """Operands of one egr_joint_layer_f32 launch, float32 on the CPU, unit scale: weights uniform in +-0.1, LayerNorm gains 1 +- 0.1,
    one row of w_out x 1e-5 and one of w_f0 x 300 (per-row scales of the fp16 scheme); frame 0 entirely masked, frame 1 entirely
    valid, the rest mixed; every 11th sampled row has sigma == 0 and g == 0 (a sample that fell outside the map).  xs / gs scale the
    layer input and the sampled features."""
    r = _Rnd(seed)
    w = lambda *s: r(*s, scale=0.1)                                           # noqa: E731
    W = {"w_fold": w(G, C, CF), "c_fold": w(G, C), "w_out": w(G, C, C), "b_out": w(G, C), "w_fuse": w(G, C, V * C), "b_fuse": w(G, C),
         "ln1_g": w(G, C) + 1, "ln1_b": w(G, C), "w_qkv": w(G, 3 * C, C), "b_qkv": w(G, 3 * C), "w_mo": w(G, C, C), "b_mo": w(G, C),
         "ln2_g": w(G, C) + 1, "ln2_b": w(G, C), "w_f0": w(G, FFN, C), "b_f0": w(G, FFN), "w_f1": w(G, C, FFN), "b_f1": w(G, C),
         "ln3_g": w(G, C) + 1, "ln3_b": w(G, C)}
    W["w_out"][0, 5] *= 1e-5
    W["w_f0"][0, 9] *= 300.0
    rows = B * J * V
    case = {"C": C, "G": G, "B": B, "J": J, "V": V, "W": W, "x": r(G * B * J, C, scale=xs), "g": r(G * rows, HEADS, CF, scale=gs),
            "e": r(G * rows, C, scale=gs) if e else None, "sigma": r(G, HEADS, rows).abs() * 0.5 + 0.25,
            "rowmask": _frame_mask(r, B, J * V).reshape(rows), "ol": None, "post": None, "reg": None, "head": None}
    out = torch.arange(rows) % 11 == 3
    case["g"].reshape(G, rows, HEADS, CF)[:, out] = 0
    case["sigma"][:, :, out] = 0
    if ol_n:
        case["ol"] = {"w": w(G, ol_n, C), "b": w(G, ol_n)}
    if post:
        case["post"] = {"g": w(G, C) + 1, "b": w(G, C)}
    if reg:
        case["reg"] = {"w0": w(G, C, C), "b0": w(G, C), "w2": w(G, 3, C), "b2": w(G, 3), "anchors": r(G * B * J, 3, scale=10.0)}
    if head:
        case["head"] = {"w": r(G, HN, J, scale=0.3), "b": w(G, HN)}
    return case


def layer_statement(case: dict, dtype, mutate: Sequence[str] = ()) -> dict:
    c = _cast(case, dtype)
    return joint_layer(c["x"], c["g"], c["e"], c["sigma"], case["rowmask"], c["W"], case["B"], case["J"], case["V"], case["C"], case["G"],
                       ol=c["ol"], post=c["post"], reg=c["reg"], head=c["head"], mutate=mutate)


def make_jqa_case(G: int, B: int, J: int, hw, ol_n: int, *, C: int = 256, seed: int = SEED) -> dict:
    """Operands of one egr_jqa_query_f32 launch: t and s32 non-negative (both sit behind a ReLU), unit scale."""
    r = _Rnd(seed + 1)
    w = lambda *s: r(*s, scale=0.1)                                           # noqa: E731
    W = {"w_hp2": w(G, C, C), "b_hp2": w(G, C), "w_bfb": w(G, C, KB), "b_bfb": w(G, C), "embed": r(G, J, C), "w_q": w(G, C, C),
         "b_q": w(G, C), "w_ol": w(G, ol_n, C), "b_ol": w(G, ol_n)}
    return {"C": C, "G": G, "B": B, "J": J, "W": W, "t": torch.relu(r(G * B * J, C)), "s32": torch.relu(r(G * B, hw[0], hw[1], KB))}


def jqa_statement(case: dict, dtype, mutate: Sequence[str] = ()) -> dict:
    c = _cast(case, dtype)
    return jqa_query(c["t"], c["s32"], c["W"], case["B"], case["J"], case["G"], mutate=mutate)


def make_pose_case(B: int, ol_n: int, rw: bool, *, C: int = 128, J: int = 16, seed: int = SEED) -> dict:
    """Operands of one egr_pose_query_f32 launch.  The proposal is b_m2 + a small w_m2 . h1: joints at body-like positions, tens of
    centimetres in x and y and about a metre along z.  The fisheye model sees theta = atan(-z / |xy|) < 0, i.e. z > 0 (at z = -100
    every projection lands outside the image), so most joints sit at z ~ +100 and are valid in most views; every fourth one is far off
    to the side (the fisheye still sees it) and two are at z ~ -100, so that both values of `valid` occur in every frame.  rw: with synthetic camera matrices."""
    from egorear_amd import synth
    r = _Rnd(seed + 2)
    w = lambda *s: r(*s, scale=0.1)                                           # noqa: E731
    pos = torch.stack((r(J, scale=35.0), r(J, scale=35.0) + 15.0, r(J, scale=25.0) + 100.0), dim=-1)
    pos[3::4, 0] += 400.0 * torch.sign(pos[3::4, 0])
    pos[1::8, 2] -= 200.0
    W = {"w_m2": r(3 * J, C, scale=0.02), "b_m2": pos.reshape(3 * J), "w_qg0": w(C, 4), "b_qg0": w(C), "w_qg2": w(C, C), "b_qg2": w(C),
         "w_qg4": w(C, C), "b_qg4": w(C), "w_ol": w(ol_n, C), "b_ol": w(ol_n)}
    W["w_qg0"][:, 1:] *= 0.1                                                  # (the point is in centimetres)
    return {"C": C, "B": B, "J": J, "W": W, "h1": r(B, C), "ctm": synth.synth_coord_trans_mat(B, seed=seed + 500) if rw else None,
            "camera": "ego4view_rw" if rw else "ego4view_syn"}


def pose_statement(case: dict, cams, dtype, mutate: Sequence[str] = ()) -> dict:
    c = _cast(case, dtype)
    return pose_query(c["h1"], c["ctm"], cams, c["W"], case["B"], case["J"], mutate=mutate)


def pose_uv(case: dict, cams, dtype) -> torch.Tensor:
    c = _cast(case, dtype)
    return unclamped_uv(c["h1"], c["ctm"], cams, c["W"], case["B"], case["J"])


def _cast(v, dtype):
    if isinstance(v, dict):
        return {k: _cast(t, dtype) for k, t in v.items()}
    if isinstance(v, torch.Tensor) and v.is_floating_point():
        return v.to(dtype)
    return v

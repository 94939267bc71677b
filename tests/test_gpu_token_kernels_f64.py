"""The fused token kernels of egr_layer.hip, each on its own, against a float64 statement of their math (`-m gpu`).

egr_joint_layer_f32 (joint_layer_kernel<C, H2>, joint_layer_p_kernel<C>), egr_jqa_query_f32 and egr_pose_query_f32 through their
wrappers, at the smallest shapes at which their indexing differs (oracle/token_statements.py: LAYER_CASES, JQA_CASES, POSE_CASES -
fewer than 15 joints down to one, an empty second half of sampled rows, a frame that is entirely masked, sampled rows with
sigma == 0, plain weights at C = 256, 16 offset / logit columns, a pooling window that is no multiple of 8, both block-to-(set, frame)
mappings), every returned tensor against oracle/token_statements.py evaluated in float64.  That statement is tied to the oracle on
the CPU and its inputs are shown to expose every term by tests/test_token_statements_host.py.

The yardstick is the same statement evaluated in float32 on the CPU - the same precision class in another summation order: per
tensor E(v) = rms(v - f64) / rms(f64), M(v) = max|v - f64| / max|f64| and
    E(hip) <= rho E(cpu32) + 1e-7,   M(hip) <= rho_max M(cpu32) + 1e-7
with one (rho, rho_max) per arithmetic (RHO below): twice the largest ratio observed on the MI355X over every (case, tensor), rounded
up to one significant digit (the table is in DESIGN.md 5i; every test prints its ratios).  The 1e-7 floor is
test_gpu_float64_referee.py's.  In the same launches: w_packed = 1 gives the bits of w_packed = 0, the split-in-loop kernel the bits
of the split-once kernel, the head tail's abs-max record bounds its output, everything is finite."""
import os

import numpy as np
import pytest
import torch

from oracle import egorear_oracle as O
from oracle import token_statements as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 1e-7
# (rho, rho_max) per arithmetic; a ratio above 8 (fp32 matrix cores) or 16 (fp16 scheme: 22 bits per operand, 4 x a float32 rounding
# per product) would be a finding about the kernel, not a reason for a larger constant
RHO = {
    "f32": (5.0, 6.0),       # fp32 matrix cores: largest observed 2.16 (E) / 2.77 (M), both egr_jqa_query_f32 at J = 1
    "h2": (4.0, 4.0),        # fp16 scheme: largest observed 1.64 (E) / 1.53 (M), the same case
}
PACKED = {"f32": 0, "h2": 2}
LAYER_MATS = ("w_fold", "w_out", "w_fuse", "w_qkv", "w_mo", "w_f0", "w_f1")


@pytest.fixture(scope="module")
def hip():
    from egorear_amd import hip as h
    assert torch.cuda.is_available()
    assert "gfx950" in h.device_arch()
    return h


@pytest.fixture(scope="module")
def statements(calib_dir):
    """key -> (case, float64 statement, float32 statement), each evaluated once"""
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    cache = {}

    def get(kind, name, scale=None):
        key = (kind, name, scale)
        if key not in cache:
            if kind == "layer":
                case = T.layer_case(name, scale)
                run = lambda dt: T.layer_statement(case, dt)                    # noqa: E731
            elif kind == "jqa":
                case = T.jqa_case(name)
                run = lambda dt: T.jqa_statement(case, dt)                      # noqa: E731
            else:
                case = T.pose_case(name)
                cams = O.make_cameras(case["camera"], calib_dir)
                case["uv64"] = T.pose_uv(case, cams, torch.float64)
                run = lambda dt: T.pose_statement(case, cams, dt)               # noqa: E731
            with torch.no_grad():
                cache[key] = (case, run(torch.float64), run(torch.float32))
        return cache[key]
    return get


def _packer(hip, packed):
    return {0: lambda w: w, 1: hip.pack_layer_w, 2: hip.pack_layer_wh2}[packed]


def _flag(packed):
    return {0: False, 1: True, 2: 2}[packed]


def _dev(v):
    if isinstance(v, dict):
        return {k: _dev(t) for k, t in v.items()}
    return v.to(DEV).contiguous() if isinstance(v, torch.Tensor) else v


def _compare(tag, got, f64, f32, select=None):
    """Every tensor of `got` (arithmetic -> {name: tensor}) against the float64 statement under the float32 yardstick; prints the ratios."""
    bad = []
    for arith, outs in got.items():
        rho, rho_max = RHO[arith]
        assert set(outs) == {k for k in f64 if f64[k].dtype != torch.bool}, (tag, arith, sorted(outs))
        for k, v in outs.items():
            assert torch.isfinite(v).all(), (tag, arith, k)
            pick = (lambda t: t[select[k]]) if select and k in select else (lambda t: t)
            e_h, m_h = T.distances(pick(v.cpu()), pick(f64[k]))
            e_c, m_c = T.distances(pick(f32[k]), pick(f64[k]))
            re, rm = e_h / e_c if e_c > 0 else float("inf"), m_h / m_c if m_c > 0 else float("inf")
            print("ratio | %-34s %-10s %-3s | E hip %.3e cpu32 %.3e ratio %7.3f | M hip %.3e cpu32 %.3e ratio %7.3f%s"
                  % (tag, k, arith, e_h, e_c, re, m_h, m_c, rm, "  (under the floor)" if e_h <= FLOOR and m_h <= FLOOR else ""))
            if not (e_h <= rho * e_c + FLOOR and m_h <= rho_max * m_c + FLOOR):
                bad.append((tag, arith, k, e_h, e_c, m_h, m_c))
    assert not bad, bad


# --------------------------------------------------------------------------- the layer

def _launch_layer(hip, case, packed):
    pk = _packer(hip, packed)
    d = _dev({k: case[k] for k in ("x", "g", "e", "sigma", "rowmask", "W", "ol", "post", "reg", "head")})
    W = {k: (pk(v) if k in LAYER_MATS else v) for k, v in d["W"].items()}
    W["packed"] = _flag(packed)
    ol = dict(d["ol"], w=pk(d["ol"]["w"])) if d["ol"] else None
    reg = dict(d["reg"], w0=pk(d["reg"]["w0"])) if d["reg"] else None              # (w_r2 stays plain)
    head = dict(d["head"], amax=torch.zeros(64, dtype=torch.int32, device=DEV)) if d["head"] else None
    x_out, ol_out, xn, pred = hip.joint_layer(d["x"], d["g"], d["e"], d["sigma"], d["rowmask"], W, case["B"], case["J"], case["V"], case["C"],
                                              case["G"], ol=ol, post=d["post"], reg=reg, want_xn=d["post"] is not None, head=head)
    torch.cuda.synchronize()
    out = {"x_out": x_out, "ol": ol_out, "xn": xn, "pred": pred, "h0": head["out"] if head else None}
    return {k: v for k, v in out.items() if v is not None}, (head["amax"] if head else None)


LAYER_RUNS = [(n, None) for n in T.LAYER_CASES] + [(n, s) for n in T.SCALED for s in T.SCALES]


@pytest.mark.parametrize("name,scale", LAYER_RUNS, ids=[n if s is None else "%s-x%g-g%g" % ((n,) + s) for n, s in LAYER_RUNS])
def test_joint_layer_against_the_float64_statement(hip, statements, name, scale):
    case, f64, f32 = statements("layer", name, scale)
    tag = name if scale is None else "%s x%g g%g" % ((name,) + scale)
    plain, _ = _launch_layer(hip, case, 0)
    # fragment-ordered fp32 weights: only the address pattern of the loads differs
    ordered, _ = _launch_layer(hip, case, 1)
    assert set(ordered) == set(plain)
    for k in plain:
        assert torch.equal(plain[k], ordered[k]), (tag, k)
    # fp16 scheme: the kernel that splits its tiles once and the one that splits inside the product loop - same scales, same products
    # in the same order
    old = hip.lib.egr_layer_set_planes(1)
    try:
        h2, amax = _launch_layer(hip, case, 2)
        hip.lib.egr_layer_set_planes(0)
        in_loop, amax0 = _launch_layer(hip, case, 2)
    finally:
        hip.lib.egr_layer_set_planes(old)
    assert set(in_loop) == set(h2) == set(plain)
    for k in h2:
        assert torch.equal(h2[k], in_loop[k]), (tag, k)
    if amax is not None:
        for rec, outs in ((amax, h2), (amax0, in_loop)):
            assert float(rec.view(torch.float32).max()) >= float(outs["h0"].abs().max()) > 0.0
    _compare(tag, {"f32": plain, "h2": h2}, f64, f32)


# --------------------------------------------------------------------------- the two query kernels

def _launch_jqa(hip, case, packed):
    pk = _packer(hip, packed)
    d = _dev({k: case[k] for k in ("t", "s32", "W")})
    W = {k: (pk(v) if k in ("w_hp2", "w_bfb", "w_q", "w_ol") else v) for k, v in d["W"].items()}
    W["packed"] = _flag(packed)
    x, ol = hip.jqa_query(d["t"], d["s32"], W, case["B"], case["J"], case["C"], case["G"])
    torch.cuda.synchronize()
    return {"x": x, "ol": ol}


@pytest.mark.parametrize("name", list(T.JQA_CASES))
def test_jqa_query_against_the_float64_statement(hip, statements, name):
    case, f64, f32 = statements("jqa", name)
    plain, ordered, h2 = (_launch_jqa(hip, case, p) for p in (0, 1, 2))
    for k in plain:
        assert torch.equal(plain[k], ordered[k]), (name, k)
    assert float(f64["x"].min()) == 0.0 < float(f64["x"].max())                    # (the ReLU cuts)
    _compare("jqa " + name, {"f32": plain, "h2": h2}, f64, f32)


def _launch_pose(hip, case, packed, cams):
    pk = _packer(hip, packed)
    d = _dev({k: case[k] for k in ("h1", "ctm", "W")})
    W = {k: (pk(v) if k in ("w_m2", "w_qg2", "w_qg4", "w_ol") else v) for k, v in d["W"].items()}       # (w_qg0 (C, 4) stays plain)
    W["packed"] = _flag(packed)
    pred, a3, a2, valid, x, ol = hip.pose_query(d["h1"], d["ctm"], cams, W, case["B"], case["J"], case["C"])
    torch.cuda.synchronize()
    return {"pred": pred, "anchors_3d": a3, "anchors_2d": a2, "x": x, "ol": ol}, valid


@pytest.mark.parametrize("name", list(T.POSE_CASES))
def test_pose_query_against_the_float64_statement(hip, statements, calib_dir, name):
    """`valid` and the clamped anchors_2d of a (frame, view, joint) are compared where the float64 projection is at least 1e-4 from 0
    and from 1 in both coordinates - at most 2 % of a case's flags are left out (on the CPU: none, test_token_statements_host.py)."""
    from egorear_amd.camera import FishEyeCameraCalibratedModel as Cam
    case, f64, f32 = statements("pose", name)
    cams = torch.from_numpy(np.stack([Cam(case["camera"], calib_dir, n).packed() for n in O.CAMERAS])).to(DEV)
    uv = case["uv64"]
    keep = torch.minimum(uv.abs(), (uv - 1).abs()).amin(-1) >= 1e-4                  # (B, 4, J)
    assert float((~keep).float().mean()) <= 0.02
    assert f64["valid"][keep].any() and not f64["valid"][keep].all()
    assert torch.equal(f32["valid"][keep], f64["valid"][keep])
    got = {}
    for arith, packed in PACKED.items():
        got[arith], valid = _launch_pose(hip, case, packed, cams)
        assert valid.shape == f64["valid"].shape
        assert torch.equal(valid.cpu().bool()[keep], f64["valid"][keep]), (name, arith)
    ordered, valid1 = _launch_pose(hip, case, 1, cams)
    for k in ordered:
        assert torch.equal(ordered[k], got["f32"][k]), (name, k)
    if case["ctm"] is None:                                                       # F7: the chained in-place offsets leave (+12, 0, 0)
        assert float((got["f32"]["anchors_3d"] - got["f32"]["pred"]).cpu().sub(torch.tensor([12.0, 0.0, 0.0])).abs().max()) < 1e-4
    else:
        assert torch.equal(got["f32"]["anchors_3d"], got["f32"]["pred"])
    _compare("pose " + name, got, f64, f32, select={"anchors_2d": keep})

"""The one-product form of conv_tapx_kernel (EGR_W_F16X1 beside EGR_W_F16X2): the role-split kernel multiplying the HIGH
planes only - a = f16(x s_a), w = f16(w s_w[co]), one v_mfma_f32_32x32x16_f16 per fragment pair, fp32 accumulation.  Forced from one
tile up with fewer workgroups than tiles (as tests/test_gpu_conv_tapx.py), on the smallest shapes that reach every tile form, a walk of
several tiles per workgroup, groups, residuals and a ragged last round.

Both bounds are derived, none is fitted to what the kernel gives:
  (2) against the float64 conv y_q of the operands rounded the way the kernel rounds them (torch's round-to-nearest-even fp16 of the
      pre-scaled value): |y - y_q| <= (K + 8) 2^-24 S_q + 2^-28 max|a| sum|w_q| - the worst case of an fp32 accumulation of K products
      plus the epilogue's few operations, S_q = conv(|a_q|, |w_q|) plus the absolute epilogue terms; the second term covers operands
      whose scaled value is an fp16 subnormal, kept or flushed;
  (3) against the float64 conv y64 of the unrounded operands: each operand carries a relative rounding error of at most 2^-11, so
      |y - y64| <= (2 2^-11 + 2^-22) S + bound (2), S = conv(|a|, |w|) carried through the epilogue's channel scale (shift and
      residual enter unrounded).
"""
import math

import pytest
import torch

from test_gpu_conv_h2 import DEV, _epilogue_kw, _reference, check, record_value
from test_gpu_conv_x6 import pack_w, rnd

pytestmark = pytest.mark.gpu

CASES = [
    # stride (0: 1x1), n, h(=w, input), cin, cout, groups, epilogue
    (1, 2, 64, 64, 64, 1, "res_before"),          # 256 x 64 tile, residual before ReLU
    (1, 8, 32, 128, 128, 2, "scale_relu"),        # 256 x 128 / 128 x 128, grouped, affine
    (1, 6, 32, 64, 128, 1, "plain"),              # 24 tiles on 5 workgroups: ragged walk
    (1, 128, 8, 128, 128, 1, "plain"),            # a tile of four whole images
    (2, 16, 32, 128, 256, 2, "scale_relu"),       # stride-2 loader, grouped
    (2, 6, 32, 96, 256, 1, "plain"),              # six chunks, 12 tiles
    (0, 4, 32, 256, 256, 1, "scale_relu"),        # 1x1: 128 x 256 / 128 x 128 tiles
    (0, 4, 32, 256, 128, 1, "res_after"),         # 1x1: 128 x 128 tiles only
]


@pytest.fixture(params=[2, 3], ids=["w32", "w64"])
def tapx(request):
    """egr_conv_set_tapx's wave-tile mode in force (2: 128 x 32, 3: 128 x 64), from one tile up, five workgroups."""
    from egorear_amd import hip
    hip.lib.egr_conv_set_tapx(request.param, 1, 5)
    saved = hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS, hip.PLAN_LOG
    hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = 0, 0.0
    yield hip, request.param
    hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS, hip.PLAN_LOG = saved
    hip.lib.egr_conv_set_tapx(1, 256, 256)


def _prescale(rec: torch.Tensor) -> float:
    """act_prescale (egr_conv_shared.h): the power of two that puts the recorded abs-max into [2^14, 2^15), exponent clamped to +-60."""
    e = int(rec.cpu().view(torch.float32).max().view(torch.int32)) >> 23
    return 2.0 ** max(-60, min(60, 141 - e))


def _f16(t: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """f16(t s) / s, round to nearest even, in float64 (s: powers of two, so both scalings are exact)."""
    return (t.double() * s).to(torch.float16).double() / s


@pytest.mark.parametrize("case", CASES, ids=[f"s{c[0]}-n{c[1]}-hw{c[2]}-{c[3]}to{c[4]}-g{c[5]}-{c[6]}" for c in CASES])
def test_one_product_launch(tapx, case):
    hip, mode = tapx
    stride, n, hw, cin, cout, G, extra = case
    k, pad, st = (1, 0, 1) if stride == 0 else (3, 1, stride)
    ho = hw // st
    x = rnd(G * n, hw, hw, cin, seed=700)
    wts = [rnd(cout, cin, k, k, seed=701 + g, scale=1.0 / math.sqrt(k * k * cin)) for g in range(G)]
    wp = (torch.stack([pack_w(t) for t in wts]) if G > 1 else pack_w(wts[0])).to(DEV)
    npad = wp.shape[-2]
    kw, res, sc, sh = _epilogue_kw(hip, extra, G, n, ho, ho, cout, npad, 705)
    w6 = hip.add_wh2(hip.pack_w6(wp))
    xd = x.to(DEV)
    rec_x = hip.absmax_record(xd, torch.zeros(64, dtype=torch.int32, device=DEV))

    def launch(one):
        rec = torch.zeros(64, dtype=torch.int32, device=DEV)
        hip.PLAN_LOG = []
        y = hip.conv2d(hip.Img(xd, amax=rec_x), w6, cout, k, k, st, pad, amax_out=rec, one_product=one, **kw)
        (tag, plan), = hip.PLAN_LOG
        hip.PLAN_LOG = None
        return y.t.permute(0, 3, 1, 2).double().cpu(), plan, hip.lib.egr_conv_last_kernel(), record_value(rec)

    # 1. the plan of the call, and the kernel that ran
    y, plan, kern, rec = launch(True)
    y3, plan3, kern3, rec3 = launch(False)
    wide_only = stride == 0 and mode == 3 and cout % 256 != 0       # (the 128 x 64 wave tile forced, only 128 x 128 tiles exist: test_gpu_conv_tapx.py)
    if wide_only:
        assert plan.planes == 2 and kern == 1 and torch.equal(y, y3), "outside the role-split kernel's cover the bit is absent"
        return
    assert (plan.route, plan.planes, kern) == (hip.ROUTE_TAPX, 1, 6), (plan.route, plan.planes, kern)
    assert (plan3.route, plan3.planes, kern3, plan3.variant + 1000) == (hip.ROUTE_TAPX, 2, 6, plan.variant)
    assert (plan.bm, plan.bn, plan.grid_x, plan.persistent) == (plan3.bm, plan3.bn, plan3.grid_x, plan3.persistent)

    # 2. against the conv of the operands as the kernel rounds them
    s_a = _prescale(rec_x)
    ds = w6.h2_ds.cpu().double().view(G, npad)[:, :cout]
    assert torch.all(torch.frexp(ds)[0] == 0.5)
    a_q = _f16(x, torch.tensor(s_a, dtype=torch.float64))
    w_q = [_f16(wts[g], (1.0 / ds[g]).view(-1, 1, 1, 1)) for g in range(G)]
    absd = lambda t: None if t is None else t.abs()
    y_q = _reference(a_q, w_q, G, n, st, pad, extra, res, sc, sh, cout)
    S_q = _reference(a_q.abs(), [w.abs() for w in w_q], G, n, st, pad, extra, absd(res), absd(sc), absd(sh), cout)
    K = k * k * cin
    wsum = torch.cat([w.abs().sum((1, 2, 3)) for w in w_q]).view(G, 1, cout, 1, 1).expand(G, n, cout, 1, 1).reshape(G * n, cout, 1, 1)
    bound2 = (K + 8) * 2.0 ** -24 * S_q + 2.0 ** -28 * float(x.abs().max()) * wsum
    err2 = (y - y_q).abs()
    print(f"{case} mode {mode}: max |y - y_q| / bound {float((err2 / bound2.clamp_min(1e-300)).max()):.4f}")
    assert torch.all(err2 <= bound2), (case, float((err2 - bound2).max()))

    # 3. against the conv of the unrounded operands
    xa = x.double()
    y64 = _reference(xa, [w.double() for w in wts], G, n, st, pad, extra, res, sc, sh, cout)
    sc1 = None if sc is None else sc.abs()
    plain = "scale_relu" if extra == "scale_relu" else "plain"          # S: the channel scale only - no shift, no residual
    S = _reference(xa.abs(), [w.double().abs() for w in wts], G, n, st, pad, plain, None, sc1, None if sc is None else torch.zeros_like(sc), cout)
    bound3 = (2 * 2.0 ** -11 + 2.0 ** -22) * S + bound2
    err3 = (y - y64).abs()
    print(f"{case} mode {mode}: max |y - y64| / bound {float((err3 / bound3.clamp_min(1e-300)).max()):.4f}, / max|y64| {float(err3.max() / y64.abs().max()):.3e}")
    assert torch.all(err3 <= bound3), (case, float((err3 - bound3).max()))

    # 4. the same call without the bit is the three-product launch (the existing bar), and the two differ
    a32 = hip.conv2d(hip.Img(xd), wp, cout, k, k, st, pad, **kw).t.permute(0, 3, 1, 2).double().cpu()
    saved = hip.H2
    hip.H2 = False
    try:
        b6 = hip.conv2d(hip.Img(xd), w6, cout, k, k, st, pad, **kw).t.permute(0, 3, 1, 2).double().cpu()
    finally:
        hip.H2 = saved
    check(a32, b6, y3, y64, None, f"three products {case}")
    assert rec3 == float(y3.abs().max())
    assert not torch.equal(y, y3), "the one-product launch must not be the three-product one"

    # 5. the record it leaves: an upper bound of what it stored, within one binade of the three-product launch's
    assert rec >= float(y.abs().max()) and rec == float(y.float().abs().max())
    assert 0.5 * rec3 <= rec <= 2.0 * rec3, (rec, rec3)

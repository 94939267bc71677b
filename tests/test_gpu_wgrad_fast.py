"""The one-product form of the split weight-gradient kernels (EGR_W_F16X1 beside EGR_W_BF16X3 | EGR_W_F16X2 on egr_conv2d_wgrad_ex_f32;
DESIGN.md 5l): both operands staged as their HIGH fp16 plane only - dy_q = f16(dy s_dy) / s_dy, x_q = f16(x s_x) / s_x, the powers of
two s from the abs-max records by wg_prescale's rule - one v_mfma_f32_32x32x16_f16 per fragment pair, fp32 accumulation, the slabs of the
pixel splits summed in fp32.  Forced split launches (x6="force") with records from an AmaxArena, one_product=True against False, on
the kernels 1 (both output-tile widths), 2 and 3 (16- and 8-pixel stages), ragged K and M, groups and stride 2.

Both bounds are derived, none is fitted to what the kernels give (M = pixels of a group, the reduction length):
  (2) against the float64 gradient dW_q of the operands rounded the way the kernel rounds them:
      |dW - dW_q| <= (M + splits + 8) 2^-24 S_q + 2^-28 (max|dy| sum_m |x_q| + max|x| sum_m |dy_q|),  S_q = sum_m |dy_q| |x_q|.
      First term: every product of two fp16 numbers is exact in fp32; the worst case of an fp32 accumulation of M of them, in whatever
      order, is M 2^-24 S_q to first order; the slab sums add `splits` more fp32 additions of partial sums bounded by S_q, the descale is
      a power of two, and 8 covers the optional accumulation onto dw and the second-order terms at these M.  `splits` is taken as the
      launch rule's ceiling, min(512, ceil(M / 64)) (at least four stages of >= 16 pixels per split).  Second term: an operand more
      than 2^28 below its tensor's maximum is an fp16 subnormal after the pre-scale - kept (as the reference keeps it) or flushed, an
      absolute error of at most 2^-28 max|.| on that operand, times the other operand, summed over the pixels;
  (3) against the float64 gradient dW64 of the unrounded operands: each operand carries a relative rounding error of at most 2^-11, so
      |dW - dW64| <= (2 2^-11 + 2^-22) S + bound (2),  S = sum_m |dy| |x|.
The bias gradient is a sum of fp32 dy on both launches: bit-equal."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_fast import _f16, _prescale
from test_gpu_conv_h2 import DEV
from test_gpu_conv_x6 import WGRAD_CASES, WGRAD_KERNEL, rnd

pytestmark = pytest.mark.gpu

CASES = [
    # n, h, w, cin, cout, k, stride, groups
    (8, 32, 32, 64, 64, 3, 1, 1),        # kernel 2 (64 channels x 2 chunks), 16-pixel stages
    (8, 32, 32, 64, 128, 3, 2, 2),       # kernel 1, 128-wide output tile, stride 2, grouped
    (2, 32, 32, 128, 128, 1, 1, 1),      # kernel 1, 1x1
    (9, 32, 32, 32, 96, 3, 1, 1),        # kernel 1: cout not a multiple of 32, ragged K tile (9 chunks)
    (3, 61, 45, 64, 128, 3, 1, 1),       # kernel 1: odd sizes, pixel count not a multiple of the stage
    (2, 16, 32, 128, 128, 3, 1, 3),      # kernel 3 (128 channels x 1 chunk), h != w, three groups
    (6, 8, 8, 256, 128, 3, 1, 1),        # kernel 3, 8-pixel-wide images: a stage is two rows
    (5, 8, 8, 64, 64, 3, 1, 2),          # kernel 2, 8-pixel-wide images, grouped
    (2, 20, 12, 32, 64, 3, 1, 1),        # kernel 1 with the 64-wide output tile (width neither 8 nor a multiple of 16)
]


def _kernel(case) -> int:
    """The kernel a forced split launch takes (egr_conv2d_wgrad_ex_f32's rule; WGRAD_KERNEL of test_gpu_conv_x6.py where it lists the case)."""
    n, h, w, cin, cout, k, s, G = case
    kern = 1
    if k == 3 and s == 1 and (w % 16 == 0 or (w == 8 and h % 2 == 0)):
        kern = 3 if cout % 128 == 0 else (2 if cout % 64 == 0 and cin % 64 == 0 else 1)
    if case in WGRAD_CASES:
        assert kern == WGRAD_KERNEL[WGRAD_CASES.index(case)]
    return kern


def _wgrad64(x, dy, cin, cout, k, s, pad):
    """sum_m dy[m, co] im2col(x)[m, (ci, kh, kw)] in float64, OIHW.  x (n, cin, h, w), dy (n, cout, ho, wo)."""
    wt = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(F.conv2d(x, wt, None, s, pad), wt, dy)
    return g


@pytest.mark.parametrize("case", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_one_product_weight_gradient(case):
    from egorear_amd import hip
    from egorear_amd.engine import unpack_conv_weight
    n, h, w, cin, cout, k, s, G = case
    pad = k // 2
    x = rnd(G * n, cin, h, w, seed=821)
    ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    dy = rnd(G * n, cout, ho, wo, seed=822) * 3e-3
    # a few operands far below their tensor's maximum: the subnormal term of the bounds
    x.view(-1)[::97] *= 2.0 ** -30
    dy.view(-1)[::89] *= 2.0 ** -29
    ws = torch.empty(1 << 24, device=DEV)
    xt, dyt = x.permute(0, 2, 3, 1).contiguous().to(DEV), dy.permute(0, 2, 3, 1).contiguous().to(DEV)
    arena = hip.AmaxArena(torch.device(DEV), records=4)
    arena.begin()
    xi, dyi = hip.Img(xt), hip.Img(dyt)
    saved = hip.H2
    hip.H2 = True
    try:
        dw1, db1 = hip.conv2d_wgrad(xi, dyi, k, k, s, pad, ws, want_bias=True, groups=G, x6="force", amax_arena=arena, one_product=True)
        kern1, planes1, h2_1 = hip.lib.egr_wgrad_last_kernel(), hip.lib.egr_wgrad_last_planes(), hip.lib.egr_wgrad_last_h2()
        assert arena.k == 2 and xi.amax is not None and dyi.amax is not None
        dw3, db3 = hip.conv2d_wgrad(xi, dyi, k, k, s, pad, ws, want_bias=True, groups=G, x6="force", amax_arena=arena, one_product=False)
        kern3, planes3 = hip.lib.egr_wgrad_last_kernel(), hip.lib.egr_wgrad_last_planes()
        # accumulate=True adds the same one-product gradient onto a preset dw / db
        pre_w, pre_b = rnd(*dw1.shape, seed=823).to(DEV) * 0.5, rnd(*db1.shape, seed=824).to(DEV)
        acc_w, acc_b = pre_w.clone(), pre_b.clone()
        hip.conv2d_wgrad(xi, dyi, k, k, s, pad, ws, want_bias=True, groups=G, x6="force", amax_arena=arena, one_product=True,
                         dw=acc_w, db=acc_b, accumulate=True)
        assert hip.lib.egr_wgrad_last_planes() == 1
        torch.cuda.synchronize()
    finally:
        hip.H2 = saved
    assert kern1 == kern3 == _kernel(case), (kern1, kern3, _kernel(case))
    assert (planes1, planes3, h2_1) == (1, 2, 1)
    assert torch.equal(db1, db3), "the bias gradient is a sum of fp32 dy on both launches"
    assert not torch.equal(dw1, dw3), "the one-product launch must not be the three-product one"
    assert float((acc_w - (pre_w + dw1)).abs().max()) <= 2.0 ** -22 * float((pre_w.abs() + dw1.abs()).max())
    assert float((acc_b - (pre_b + db1)).abs().max()) <= 2.0 ** -22 * float((pre_b.abs() + db1.abs()).max())

    s_x, s_dy = _prescale(xi.amax), _prescale(dyi.amax)
    x_q, dy_q = _f16(x, torch.tensor(s_x, dtype=torch.float64)), _f16(dy, torch.tensor(s_dy, dtype=torch.float64))
    M = n * ho * wo
    splits = min(512, (M + 63) // 64)
    mx, mdy = float(x.abs().max()), float(dy.abs().max())
    worst2 = worst3 = 0.0
    for g in range(G):
        sl = slice(g * n, (g + 1) * n)
        got = unpack_conv_weight((dw1[g] if G > 1 else dw1).cpu(), cin, k, k).double()
        args = (cin, cout, k, s, pad)
        dW_q = _wgrad64(x_q[sl], dy_q[sl], *args)
        S_q = _wgrad64(x_q[sl].abs(), dy_q[sl].abs(), *args)
        sum_x = _wgrad64(x_q[sl].abs(), torch.ones_like(dy_q[sl]), *args)
        sum_dy = _wgrad64(torch.ones_like(x_q[sl]), dy_q[sl].abs(), *args)
        bound2 = (M + splits + 8) * 2.0 ** -24 * S_q + 2.0 ** -28 * (mdy * sum_x + mx * sum_dy)
        err2 = (got - dW_q).abs()
        worst2 = max(worst2, float((err2 / bound2.clamp_min(1e-300)).max()))
        assert torch.all(err2 <= bound2), (case, g, float((err2 - bound2).max()))
        dW64 = _wgrad64(x[sl].double(), dy[sl].double(), *args)
        S = _wgrad64(x[sl].double().abs(), dy[sl].double().abs(), *args)
        bound3 = (2 * 2.0 ** -11 + 2.0 ** -22) * S + bound2
        err3 = (got - dW64).abs()
        worst3 = max(worst3, float((err3 / bound3.clamp_min(1e-300)).max()))
        assert torch.all(err3 <= bound3), (case, g, float((err3 - bound3).max()))
        db64 = dy[sl].double().sum((0, 2, 3))
        gb = (db1[g] if G > 1 else db1).cpu().double()
        assert float((gb - db64).abs().max()) <= 1e-5 * float(dy[sl].abs().sum((0, 2, 3)).max())
    print(f"{case}: kernel {kern1}, max |dW - dW_q| / bound {worst2:.4f}, max |dW - dW64| / bound {worst3:.4f}")


def test_the_policy_selects_it_and_only_fp16_scheme_launches_take_it():
    """one_product=None follows LaunchPolicy.train_one_product; a split launch outside the fp16 scheme (no records) ignores the request."""
    from egorear_amd import hip
    x, dy = rnd(8, 32, 32, 64, seed=831).to(DEV), rnd(8, 32, 32, 64, seed=832).to(DEV)
    ws = torch.empty(1 << 24, device=DEV)

    def run(**kw):
        arena = hip.AmaxArena(torch.device(DEV), records=4)
        arena.begin()
        dw, _ = hip.conv2d_wgrad(hip.Img(x.clone()), hip.Img(dy.clone()), 3, 3, 1, 1, ws, x6="force", **dict(dict(amax_arena=arena), **kw))
        return dw.clone(), hip.lib.egr_wgrad_last_planes()

    dw_d, p_d = run()
    with hip.use_policy(hip.LaunchPolicy.fast()):
        dw_f, p_f = run()
    with hip.use_policy(hip.LaunchPolicy.fast_training()):
        dw_t, p_t = run()
        dw_n, p_n = run(amax_arena=None)                  # no records: the bf16 scheme, whatever the policy asks for
    dw_1, p_1 = run(one_product=True)
    assert (p_d, p_f, p_t, p_n, p_1) == (2, 2, 1, 3, 1)
    assert torch.equal(dw_d, dw_f) and torch.equal(dw_t, dw_1) and not torch.equal(dw_t, dw_d)
    assert float((dw_n - dw_d).abs().max()) <= 4e-6 * float(dw_d.abs().max())

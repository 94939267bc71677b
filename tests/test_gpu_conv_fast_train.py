"""The one-product forms of conv_tapx_kernel's TRAINING launches (EGR_W_F16X1T beside EGR_W_F16X2 | EGR_W_F16X1): the
statistics epilogue (variants 1100, 1101, 1103, 1105), the masked stride-1 data gradient (1201, 1203, 1211, 1213) and the plain data
gradient - a forward one-product variant on the transposed weight image.  a = f16(x s_a), w = f16(w s_w[co]), one
v_mfma_f32_32x32x16_f16 per fragment pair, fp32 accumulation; slabs, mask quads, residual, hand-over and record are the shared code.
Forced from one tile up with five workgroups on both wave-tile modes, as tests/test_gpu_conv_fast.py.

The bounds are (2) and (3) of tests/test_gpu_conv_fast.py's docstring, elementwise, carried through the epilogue of these launches:
  (2) |y - y_q| <= (K + 8) 2^-24 S_q + 2^-28 max|a| sum|w_q| against the float64 result of the operands rounded the way the kernel
      rounds them, S_q = conv(|a_q|, |w_q|) + |residual|;
  (3) |y - y64| <= (2 2^-11 + 2^-22) S + bound (2) against the float64 result of the unrounded operands, S = conv(|a|, |w|);
the residual (the gradient accumulated so far) enters unrounded, and the ReLU mask is the sign of a given activation tensor - exact - so
reference, S_q, S and both bounds are multiplied by it.  None of this is fitted to what the kernel gives."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_fast import _f16, _prescale
from test_gpu_conv_h2 import DEV, _reference, record_value
from test_gpu_conv_x6 import pack_w, pack_w_dgrad, rnd

pytestmark = pytest.mark.gpu

BN_CASES = [
    # n, h(=w), cin, cout, stride, groups
    (8, 32, 64, 64, 1, 2),                     # 256 x 64 tiles, grouped: 1103
    (4, 32, 128, 128, 1, 1),                   # 128 x 128 tiles (1101) / 256 x 128 on the wide wave tile (1100)
    (8, 32, 64, 128, 2, 2),                    # stride 2, grouped: 1105
]
DGRAD_CASES = [
    # groups, n, h(=w), forward cin, forward cout, mode
    (1, 4, 64, 64, 64, "masked"),              # 256 x 64 tiles, mask only: 1203
    (1, 4, 64, 64, 64, "masked_res"),          # ... + the gradient accumulated so far: 1213
    (1, 8, 32, 128, 128, "masked"),            # 128 x 128 tiles: 1201
    (2, 8, 32, 128, 128, "masked_res"),        # grouped: 1211
    (1, 6, 32, 64, 128, "masked_res"),         # 24 tiles on 5 workgroups: ragged walk
    (2, 32, 8, 512, 512, "plain"),             # plain data gradient, two 8 x 8 images per tile: 1000 / 1001 on the transposed image
    (1, 16, 64, 128, 64, "res"),               # accumulated, no mask: 1010 / 1011
]
NEW_VARIANTS = {1100, 1101, 1103, 1105, 1201, 1203, 1211, 1213}
SEEN, RAN = set(), []        # variants launched over the file; (test, case, mode) that ran
REFS = {}                    # per case: the float64 references and bounds (the same for both wave-tile modes)


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


def _launch(hip, fn):
    """fn() under a fresh PLAN_LOG: (result, the one plan it logged, the route that ran)."""
    hip.PLAN_LOG = []
    try:
        out = fn()
        (tag, plan), = hip.PLAN_LOG
    finally:
        hip.PLAN_LOG = None
    return out, tag, plan, hip.lib.egr_conv_last_kernel()


def _check_plans(hip, plan, kern, tag, plan3, kern3, tag3):
    assert (plan.route, plan.planes, kern) == (hip.ROUTE_TAPX, 1, 6), (plan.route, plan.planes, kern)
    assert (plan3.route, plan3.planes, kern3, plan3.variant + 1000) == (hip.ROUTE_TAPX, 2, 6, plan.variant)
    assert (plan.bm, plan.bn, plan.grid_x, plan.persistent) == (plan3.bm, plan3.bn, plan3.grid_x, plan3.persistent)
    assert tag.startswith("h1 ") and tag3.startswith("h2 ") and tag[3:] == tag3[3:], (tag, tag3)
    SEEN.add(plan.variant)


def _check_bounds(y, refs, what):
    y_q, bound2, y64, bound3 = refs
    err2, err3 = (y - y_q).abs(), (y - y64).abs()
    print(f"{what}: max |y - y_q| / bound {float((err2 / bound2.clamp_min(1e-300)).max()):.4f}, "
          f"max |y - y64| / bound {float((err3 / bound3.clamp_min(1e-300)).max()):.4f}, / max|y64| {float(err3.max() / y64.abs().max()):.3e}")
    assert torch.all(err2 <= bound2), (what, float((err2 - bound2).max()))
    assert torch.all(err3 <= bound3), (what, float((err3 - bound3).max()))


@pytest.mark.parametrize("case", BN_CASES, ids=[f"n{c[0]}-hw{c[1]}-{c[2]}to{c[3]}-s{c[4]}-g{c[5]}" for c in BN_CASES])
def test_one_product_statistics_epilogue(tapx, case):
    from egorear_amd import hip_train as T
    hip, mode = tapx
    n, hw, cin, cout, st, G = case
    x = rnd(G * n, hw, hw, cin, seed=531)
    x[:, :, :, 3] += 7.0                       # (a channel far from zero mean on the input side)
    wts = [rnd(cout, cin, 3, 3, seed=532 + g, scale=1.0 / math.sqrt(9 * cin)) for g in range(G)]
    wp = (torch.stack([pack_w(t) for t in wts]) if G > 1 else pack_w(wts[0])).to(DEV)
    npad = wp.shape[-2]
    w6 = hip.add_wh2(hip.pack_w6(wp))
    xd = x.to(DEV)
    rec_x = hip.absmax_record(xd, torch.zeros(64, dtype=torch.int32, device=DEV))
    ws = T.bn_workspace(DEV)

    def run(one):
        rec, slabs = torch.zeros(64, dtype=torch.int32, device=DEV), []
        y, tag, plan, kern = _launch(hip, lambda: hip.conv2d(hip.Img(xd, amax=rec_x), w6, cout, 3, 3, st, 1, groups=G, amax_out=rec,
                                                             bn_ws=ws, bn_slabs=slabs, one_product=one).t)
        # the slabs finalise right behind the launch that left them (the next launch reuses the workspace)
        gamma, beta = (rnd(G, cout, seed=535) + 1.5).to(DEV), rnd(G, cout, seed=536).to(DEV)
        fin = []
        for sl in (slabs[0], None):            # the epilogue's slabs / a statistics pass over the same stored tensor
            r = torch.zeros(64, dtype=torch.int32, device=DEV)
            rm, rv = torch.zeros(G, cout, device=DEV), torch.ones(G, cout, device=DEV)
            _, ctx = T.bn_train(y, gamma, beta, rm, rv, G, ws, relu=True, amax_out=r, slabs=sl)
            fin.append((ctx.mean.clone(), ctx.invstd.clone(), ctx.xhat_max.clone(), r.clone()))
        torch.cuda.synchronize()
        return y, tag, plan, kern, record_value(rec), slabs[0], fin

    y_dev, tag, plan, kern, rec, nslabs, fin = run("train")
    y3_dev, tag3, plan3, kern3, rec3, nslabs3, _ = run(False)
    RAN.append(("bn", case, mode))
    # 1. the plan of the call, and the kernel that ran
    _check_plans(hip, plan, kern, tag, plan3, kern3, tag3)
    assert plan.variant // 100 == 11 and nslabs == nslabs3 == plan.bn_slabs == plan3.bn_slabs
    # 2. the bounds
    y, y3 = y_dev.permute(0, 3, 1, 2).double().cpu(), y3_dev.permute(0, 3, 1, 2).double().cpu()
    if case not in REFS:
        s_a = _prescale(rec_x)
        ds = w6.h2_ds.cpu().double().view(G, npad)[:, :cout]
        a_q = _f16(x, torch.tensor(s_a, dtype=torch.float64))
        w_q = [_f16(wts[g], (1.0 / ds[g]).view(-1, 1, 1, 1)) for g in range(G)]
        y_q = _reference(a_q, w_q, G, n, st, 1, "plain", None, None, None, cout)
        S_q = _reference(a_q.abs(), [w.abs() for w in w_q], G, n, st, 1, "plain", None, None, None, cout)
        wsum = torch.cat([w.abs().sum((1, 2, 3)) for w in w_q]).view(G, 1, cout, 1, 1).expand(G, n, cout, 1, 1).reshape(G * n, cout, 1, 1)
        bound2 = (9 * cin + 8) * 2.0 ** -24 * S_q + 2.0 ** -28 * float(x.abs().max()) * wsum
        y64 = _reference(x.double(), [w.double() for w in wts], G, n, st, 1, "plain", None, None, None, cout)
        S = _reference(x.double().abs(), [w.double().abs() for w in wts], G, n, st, 1, "plain", None, None, None, cout)
        REFS[case] = (y_q, bound2, y64, (2 * 2.0 ** -11 + 2.0 ** -22) * S + bound2)
    _check_bounds(y, REFS[case], f"statistics {case} mode {mode}")
    # 3. not the three-product launch
    assert not torch.equal(y, y3), "the one-product launch must not be the three-product one"
    # 4. the record: the maximum of what was stored, within one binade of the three-product launch's
    assert rec == float(y.abs().max()) and rec3 == float(y3.abs().max())
    assert 0.5 * rec3 <= rec <= 2.0 * rec3, (rec, rec3)
    # 5. the slabs finalise to the statistics of the stored tensor; the extremes are those of a pass over it
    yv = y_dev.double().view(G, -1, cout)
    (mean, invstd, xmax, r), (mean_p, invstd_p, xmax_p, r_p) = fin
    assert float((mean.double().view(G, cout) - yv.mean(1)).abs().max()) <= 1e-6 * float(yv.abs().max())
    assert float((mean - mean_p).abs().max()) <= 2e-6 * float(mean_p.abs().max())
    assert float((invstd - invstd_p).abs().max()) <= 2e-6 * float(invstd_p.abs().max())
    assert torch.equal(xmax, xmax_p) and torch.equal(r, r_p)


@pytest.mark.parametrize("case", DGRAD_CASES, ids=[f"g{c[0]}-n{c[1]}-hw{c[2]}-{c[3]}to{c[4]}-{c[5]}" for c in DGRAD_CASES])
def test_one_product_data_gradient(tapx, case):
    hip, mode = tapx
    G, n, hw, cin, cout, how = case            # forward conv cin -> cout; the gradient maps dy (cout channels) to dx (cin)
    dy = rnd(G * n, hw, hw, cout, seed=481)
    xs, prev = rnd(G * n, hw, hw, cin, seed=482), rnd(G * n, hw, hw, cin, seed=483)
    wts = [rnd(cout, cin, 3, 3, seed=484 + g, scale=1.0 / math.sqrt(9 * cin)) for g in range(G)]
    wt = (torch.stack([pack_w_dgrad(w) for w in wts]) if G > 1 else pack_w_dgrad(wts[0])).to(DEV)
    npad = wt.shape[-2]
    w6 = hip.add_wh2(hip.pack_w6(wt))
    kw = dict(transposed_out_hw=(hw, hw), groups=G)
    if "res" in how:
        kw.update(res=hip.Img(prev.to(DEV)), res_mode=hip.RES_BEFORE_ACT)
    if "masked" in how:
        kw.update(mask=hip.Img(xs.to(DEV)))
    dyd = dy.to(DEV)
    rec_dy = hip.absmax_record(dyd, torch.zeros(64, dtype=torch.int32, device=DEV))

    def run(one):
        rec = torch.zeros(64, dtype=torch.int32, device=DEV)
        o, tag, plan, kern = _launch(hip, lambda: hip.conv2d(hip.Img(dyd, amax=rec_dy), w6, cin, 3, 3, 1, 1, amax_out=rec, one_product=one, **kw).t)
        torch.cuda.synchronize()
        return o.double().cpu(), tag, plan, kern, record_value(rec)

    dx, tag, plan, kern, rec = run("train")
    dx3, tag3, plan3, kern3, rec3 = run(False)
    RAN.append(("dgrad", case, mode))
    # 1. the plan of the call, and the kernel that ran
    _check_plans(hip, plan, kern, tag, plan3, kern3, tag3)
    assert plan.variant // 100 == (12 if "masked" in how else 10) and (plan.variant // 10) % 10 == (1 if "res" in how else 0)
    # a forward request alone leaves a data gradient on three products (the plan it has without the bit)
    _, _, plan_f, _ = _launch(hip, lambda: hip.conv2d(hip.Img(dyd, amax=rec_dy), w6, cin, 3, 3, 1, 1, one_product=True, **kw))
    assert all(getattr(plan_f, f) == getattr(plan3, f) for f, _ in hip.ConvPlan._fields_)
    # 2. the bounds
    if case not in REFS:
        def grad(dyv, ws_):
            out = []
            for g in range(G):
                xr = torch.zeros(n, cin, hw, hw, dtype=torch.float64, requires_grad=True)
                (r,) = torch.autograd.grad(F.conv2d(xr, ws_[g], None, 1, 1), xr, dyv[g * n:(g + 1) * n].permute(0, 3, 1, 2))
                out.append(r.permute(0, 2, 3, 1))
            return torch.cat(out)
        s_a = _prescale(rec_dy)
        ds = w6.h2_ds.cpu().double().view(G, npad)[:, :cin]            # per OUTPUT channel of the launch: the forward conv's input channel
        assert torch.all(torch.frexp(ds)[0] == 0.5)
        a_q = _f16(dy, torch.tensor(s_a, dtype=torch.float64))
        w_q = [_f16(wts[g], (1.0 / ds[g]).view(1, -1, 1, 1)) for g in range(G)]
        keep = (xs > 0).double() if "masked" in how else torch.ones_like(xs, dtype=torch.float64)
        resv = prev.double() if "res" in how else torch.zeros_like(prev, dtype=torch.float64)
        y_q = (grad(a_q, w_q) + resv) * keep
        S_q = (grad(a_q.abs(), [w.abs() for w in w_q]) + resv.abs()) * keep
        wsum = torch.cat([w.abs().sum((0, 2, 3)) for w in w_q]).view(G, 1, 1, 1, cin).expand(G, n, 1, 1, cin).reshape(G * n, 1, 1, cin)
        bound2 = ((9 * cout + 8) * 2.0 ** -24 * S_q + 2.0 ** -28 * float(dy.abs().max()) * wsum) * keep
        y64 = (grad(dy.double(), [w.double() for w in wts]) + resv) * keep
        S = grad(dy.double().abs(), [w.double().abs() for w in wts]) * keep
        REFS[case] = (y_q, bound2, y64, (2 * 2.0 ** -11 + 2.0 ** -22) * S + bound2)
    _check_bounds(dx, REFS[case], f"data gradient {case} mode {mode}")
    # 3. not the three-product launch
    assert not torch.equal(dx, dx3), "the one-product launch must not be the three-product one"
    # 4. the record: the maximum of what was stored, within one binade of the three-product launch's
    assert rec == float(dx.abs().max()) and rec3 == float(dx3.abs().max())
    assert 0.5 * rec3 <= rec <= 2.0 * rec3, (rec, rec3)


def test_every_new_variant_was_launched():
    """Over both wave-tile modes the cases above reach all eight new variants and the forward ones on the transposed image.  (Judged
    when the whole file ran: a selection of its cases reaches a subset.)"""
    if len(RAN) != 2 * (len(BN_CASES) + len(DGRAD_CASES)):
        pytest.skip(f"only {len(RAN)} of the file's {2 * (len(BN_CASES) + len(DGRAD_CASES))} cases ran: the variant census needs all of them")
    assert NEW_VARIANTS <= SEEN, sorted(NEW_VARIANTS - SEEN)
    assert SEEN & {1000, 1001} and SEEN & {1010, 1011}, sorted(SEEN)

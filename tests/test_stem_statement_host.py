"""The float64 statement of the stem kernels (tests/stem_statement.py) held against torch: F.conv2d / F.max_pool2d / autograd in
float64, the documented view selection, and the condition the statement has to meet before a kernel is judged by it - a float32
evaluation of the same inputs, the reference alone, lies inside the bounds test_gpu_stem_walk.py asserts for the fp32 kernel.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import stem_statement as S

C_F32 = (147 + 3) * 2.0 ** -24       # test_gpu_stem_walk.py's bound for the fp32 kernel: a chain over the 147 taps + the epilogue


def _torch_ref(img, view0, nviews, w, scale, shift, groups, pool, dt=torch.float64):
    B = img.shape[0]
    out = []
    for g in range(groups):
        v0 = view0 + g * nviews
        x = torch.stack([img[b, v0 + v] for v in range(nviews) for b in range(B)]).to(dt)         # n = v*B + b
        y = F.conv2d(x, w[g].to(dt), None, 2, 3)
        if scale is not None:
            y = F.relu(y * scale[g].to(dt).view(1, -1, 1, 1) + shift[g].to(dt).view(1, -1, 1, 1))
        if pool:
            y = F.max_pool2d(y, 3, 2, 1)
        out.append(y.permute(0, 2, 3, 1))
    return torch.cat(out, 0)


@pytest.mark.parametrize("B,V,H,W,view0,nviews,groups", [(2, 4, 18, 26, 1, 1, 3), (1, 5, 32, 64, 0, 2, 2)])
def test_statement_is_torchs_conv_pool_and_autograd(B, V, H, W, view0, nviews, groups):
    img, w, scale, shift = S.stem_inputs(B, V, H, W, groups, seed=300)
    for sc, sh, pool in ((None, None, False), (scale, shift, False), (scale, shift, True), (None, None, True)):
        got = S.stem_ref(img, view0, nviews, w, sc, sh, groups, pool)
        ref = _torch_ref(img, view0, nviews, w, sc, sh, groups, pool)
        mag = S.stem_mag(img, view0, nviews, w, sc, sh, groups, pool)
        assert got.dtype == torch.float64 and got.shape == ref.shape == mag.shape
        # two float64 evaluations in different orders: within 300 roundings of the sum of magnitudes
        assert torch.all((got - ref).abs() <= 300 * 2.0 ** -53 * mag)
    # the magnitude is the same convolution over |img| and |w|
    assert torch.equal(S.stem_mag(img, view0, nviews, w, None, None, groups, False),
                       S.stem_ref(img.abs(), view0, nviews, w.abs(), None, None, groups, False))
    # the weight gradient against autograd
    n = nviews * B
    dy = S.rnd(groups * n, (H + 1) // 2, (W + 1) // 2, 64, seed=304)
    dw, dmag = S.stem_wgrad_ref(img, view0, nviews, dy, groups)
    wd = w.double().requires_grad_(True)
    auto, = torch.autograd.grad(_torch_ref(img, view0, nviews, wd, None, None, groups, False), wd, dy.double())
    assert dw.shape == dmag.shape == (groups, 64, 3, 7, 7) and dw.dtype == torch.float64
    assert torch.all((dw - auto).abs() <= (n * dy.shape[1] * dy.shape[2] + 2) * 2.0 ** -53 * dmag)
    assert torch.equal(dmag, S.stem_wgrad_ref(img.abs(), view0, nviews, dy.abs(), groups)[0])


def test_view_selection_is_the_documented_one():
    """Every view of every batch element a distinct constant, every filter its group's number at the centre tap of input channel 1: output
    image g*nviews*B + v*B + b must hold (g + 1) * the constant of (b, view0 + g*nviews + v)."""
    B, V, H, W, view0, nviews, groups = 3, 6, 8, 12, 1, 2, 2
    const = (torch.arange(B * V, dtype=torch.float32) + 1).view(B, V)
    img = const.view(B, V, 1, 1, 1).expand(B, V, 3, H, W).contiguous()
    img[:, :, 0] += 0.25      # the other input channels do not reach the output
    w = torch.zeros(groups, 64, 3, 7, 7)
    for g in range(groups):
        w[g, :, 1, 3, 3] = g + 1
    y = S.stem_ref(img, view0, nviews, w, None, None, groups, False)
    assert y.shape == (groups * nviews * B, H // 2, W // 2, 64)
    for g in range(groups):
        for v in range(nviews):
            for b in range(B):
                want = (g + 1) * float(const[b, view0 + g * nviews + v])
                assert torch.all(y[g * nviews * B + v * B + b] == want), (g, v, b)
    # the weight gradient takes the same views: dy = 1 on one image only -> dw's centre tap = pixels * that image's constant
    dy = torch.zeros(groups * nviews * B, H // 2, W // 2, 64)
    g, v, b = 1, 1, 2
    dy[g * nviews * B + v * B + b] = 1.0
    dw, _ = S.stem_wgrad_ref(img, view0, nviews, dy, groups)
    assert torch.all(dw[g, :, 1, 3, 3] == (H // 2) * (W // 2) * float(const[b, view0 + g * nviews + v]))
    assert torch.all(dw[0] == 0)


BOUND_CASES = ([S.WALK_CASES["main"], S.WALK_CASES["single"], S.VIEW_CASE]
               + sorted({S.edge_case(*hw) for fam in S.EDGE_SHAPES.values() for hw in fam.values()}))


@pytest.mark.parametrize("case", BOUND_CASES, ids=lambda c: "%dx%d-G%d" % (c[2], c[3], c[4]))
def test_a_float32_evaluation_lies_inside_the_bounds(case):
    """The condition on the reference alone, on every input of test_gpu_stem_walk.py: torch's float32 convolution deviates from the float64
    statement by less than both bounds that file asserts, per element, raw and in eval mode - (147 + 3) * 2^-24 of the magnitude (the fp32
    kernel) and 1e-6 / 1.2e-6 (the split launches).  A kernel that misses its bound is then wrong, not the bound or the statement."""
    B, V, H, W, groups, seed, view0, nviews = case
    img, w, scale, shift = S.stem_inputs(B, V, H, W, groups, seed)
    conv, mag = S.stem_conv(img, view0, nviews, w, groups), S.stem_conv(img, view0, nviews, w, groups, magnitude=True)
    for sc, sh, c_split in ((None, None, 1e-6), (scale, shift, 1.2e-6)):
        ref, m = S.stem_epilogue(conv, sc, sh, groups, False), S.mag_epilogue(mag, sc, sh, groups, False)
        y32 = _torch_ref(img, view0, nviews, w, sc, sh, groups, False, dt=torch.float32)
        assert y32.dtype == torch.float32
        err = (y32.double() - ref).abs()
        r = float((err / m.clamp_min(1e-300)).max())
        print(f"{H}x{W} G{groups} {'raw' if sc is None else 'eval'}: float32 conv2d max err / mag {r:.3e}  (bounds {c_split:.1e}, {C_F32:.3e})")
        assert torch.all(err <= C_F32 * m) and torch.all(err <= c_split * m)

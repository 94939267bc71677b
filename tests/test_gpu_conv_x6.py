"""The split-bf16 launch of egr_conv2d_nhwc_f32 (EGR_W_BF16X3: fp32 operands as exact sums of three bf16, six partial products
on the bf16 matrix cores, fp32 accumulate) against the fp32-matrix-core launch of the same problem and against an fp64
reference: every mode the model and the training step use (3x3 / 1x1, strides, every tile configuration, grouped, split-K,
transposed data gradient incl. the stride-2 parity classes, masked epilogue, residual modes, channel-major output).
The bar: the split launch is as close to the fp64 result as the fp32 launch is (its error may not exceed 1.5x the fp32
launch's + 1e-7 of the result's magnitude), and both are within 2e-5."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def pack_w(w):
    from egorear_amd.engine import pack_conv_weight
    w2 = pack_conv_weight(w)
    npad = (w.shape[0] + 31) // 32 * 32
    out = torch.zeros(npad, w2.shape[1])
    out[:w.shape[0]] = w2
    return out


def pack_w_dgrad(w):
    return pack_w(w.transpose(0, 1).contiguous())


def both(hip, x, wp, *args, **kw):
    """The same launch with the fp32 matrix and with its split image."""
    wp = wp.to(DEV)
    a = hip.conv2d(x, wp, *args, **kw)
    if kw.get("out") is not None or kw.get("out_nchw") is not None:
        raise AssertionError("use fresh outputs here")
    # the shipped size rule would send these small problems back to the fp32 kernel: force the split launch
    saved = hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS
    hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = 0, 0.0
    try:
        prof, hip.PROFILE = hip.PROFILE, []
        b = hip.conv2d(x, hip.pack_w6(wp), *args, **kw)
        tags = [t for name, *_, t in hip.PROFILE if name == "egr_conv2d_nhwc_f32"]
        assert tags and ("x6 " in tags[-1]), "the second launch must be the split-bf16 one"
    finally:
        hip.PROFILE = prof
        hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = saved
    return a, b


def judge(a, b, ref, what=""):
    ref = ref.double()
    scale = max(float(ref.abs().max()), 1e-6)
    ea = float((a.double().cpu() - ref).abs().max()) / scale
    eb = float((b.double().cpu() - ref).abs().max()) / scale
    assert ea <= 2e-5 and eb <= 2e-5, (what, ea, eb)
    # (+4e-7: small 1x1 fp32 launches sum K as four quarter chains - linear_small_kernel - and land below 2e-7 themselves)
    assert eb <= 1.5 * ea + 4e-7, (what, "split launch less accurate than the fp32 launch", ea, eb)
    return ea, eb


def test_pack_w6_is_an_exact_three_way_split(hip=None):
    from egorear_amd import hip
    npad, K = 96, 9 * 64
    w = rnd(2, npad, K, seed=3, scale=0.3)
    w[0, 5, 7] = 1.0
    w[1, 0, 0] = 3.0e-30
    w[1, 1, 1] = -2.5e20
    w6 = hip.pack_w6(w.to(DEV))
    assert w6.gstride == 4 * (K // 32) * 3072 and w6.img.numel() == 2 * w6.gstride
    img = w6.img.float().cpu().view(2, 4, K // 32, 2, 3, 64, 8)    # [g][frag][chunk][step][plane][lane][j]
    recon = img.double().sum(4)                                     # hi + mid + lo, exact in fp64
    lanes = torch.arange(64)
    for g in range(2):
        for cf in range(4):
            for step in range(2):
                cols = cf * 32 + (lanes & 31)
                for ch in (0, K // 32 - 1, 7):
                    k0 = ch * 32 + step * 16 + 8 * (lanes >> 5)
                    kk = k0[:, None] + torch.arange(8)[None]
                    want = torch.zeros(64, 8, dtype=torch.float64) if cf == 3 else w[g][cols[:, None].expand(64, 8), kk].double()
                    assert torch.equal(recon[g, cf, ch, step], want), (g, cf, ch, step)


CONV_CASES = [
    # n, h, w, cin, cout, k, stride, act, res_mode, bn, cfg
    (2, 16, 16, 64, 64, 3, 1, 1, 1, True, -1),
    (2, 16, 16, 64, 128, 3, 2, 1, 0, True, -1),
    (2, 16, 16, 64, 128, 1, 2, 0, 0, True, -1),
    (3, 8, 8, 512, 128, 1, 1, 1, 0, False, -1),
    (1, 64, 64, 128, 256, 3, 2, 1, 0, False, -1),
    (5, 64, 64, 32, 128, 3, 1, 1, 2, False, -1),     # 128x128 tiles
    (5, 64, 64, 64, 64, 3, 1, 1, 0, True, -1),       # N = 64 -> 64x64 tiles
    (5, 64, 64, 128, 192, 1, 1, 0, 0, False, -1),
    (2, 32, 32, 128, 15, 1, 1, 0, 0, False, -1),     # 15 channels: 128x32 tiles
    (37, 1, 1, 256, 48, 1, 1, 2, 0, False, -1),      # linear + GELU, ragged rows
    (5, 64, 64, 64, 64, 3, 1, 1, 0, True, 1),        # forced 256x64 (two staging units per thread)
    (5, 64, 64, 64, 64, 3, 1, 1, 0, True, 4),        # forced 128x64
    (3, 33, 17, 96, 160, 3, 1, 0, 0, False, 0),      # odd sizes, 3 channel chunks, ragged tiles in both directions (128x128)
    (3, 33, 17, 96, 160, 3, 2, 1, 0, False, 2),      # the same on 64x64 tiles, stride 2
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_forward_modes(case):
    from egorear_amd import hip
    n, h, w, cin, cout, k, stride, act, res_mode, bn, cfg = case
    pad = k // 2
    x = rnd(n, h, w, cin, seed=1)
    wt = rnd(cout, cin, k, k, seed=2, scale=1.0 / math.sqrt(cin * k * k))
    scale = (rnd(cout, seed=3) * 0.4 + 1.0) if bn else None
    shift = rnd(cout, seed=4)
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    res = rnd(n, ho, wo, cout, seed=5) if res_mode else None
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), wt.double(), None, stride, pad)
    if scale is not None:
        ref = ref * scale.double().view(1, -1, 1, 1)
    ref = ref + shift.double().view(1, -1, 1, 1)
    if res_mode == 1:
        ref = ref + res.permute(0, 3, 1, 2).double()
    ref = F.relu(ref) if act == 1 else (F.gelu(ref) if act == 2 else ref)
    if res_mode == 2:
        ref = ref + res.permute(0, 3, 1, 2).double()
    hip.conv_force_config(cfg)
    try:
        a, b = both(hip, hip.Img(x.to(DEV)), pack_w(wt), cout, k, k, stride, pad, scale=scale.to(DEV) if scale is not None else None,
                    shift=shift.to(DEV), act=act, res=hip.Img(res.to(DEV)) if res is not None else None, res_mode=res_mode)
    finally:
        hip.conv_force_config(-1)
    judge(a.t.permute(0, 3, 1, 2), b.t.permute(0, 3, 1, 2), ref, str(case))


def test_grouped_and_split_k():
    from egorear_amd import hip
    G, n, h, cin, cout, k = 3, 2, 16, 64, 96, 3
    x = rnd(G * n, h, h, cin, seed=21)
    wts = [rnd(cout, cin, k, k, seed=30 + g, scale=1 / 24) for g in range(G)]
    wp = torch.stack([pack_w(w) for w in wts])
    a, b = both(hip, hip.Img(x.to(DEV)), wp, cout, k, k, 1, 1, groups=G)
    ref = torch.cat([F.conv2d(x[g * n:(g + 1) * n].permute(0, 3, 1, 2).double(), wts[g].double(), None, 1, 1) for g in range(G)])
    judge(a.t.permute(0, 3, 1, 2), b.t.permute(0, 3, 1, 2), ref, "grouped")
    # skinny linear with long K through split-K (explicit and automatic) with row scale / mask
    m, K, n_out = 6, 4096, 96
    xl, wl, bl, rs = rnd(m, K, seed=11), rnd(n_out, K, seed=12, scale=1 / 64), rnd(n_out, seed=13), rnd(m, seed=14)
    mask = torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.uint8)
    ref = (xl.double() @ wl.double().t() + bl.double()[None] * rs.double()[:, None]) * mask.double()[:, None]
    ws = torch.empty(1 << 22, device=DEV)
    for split in (1, 0, 7):
        a, b = both(hip, hip.Img(xl.to(DEV).view(m, 1, 1, K)), wl, n_out, 1, 1, 1, 0, shift=bl.to(DEV), rowscale=rs.to(DEV),
                    rowmask=mask.to(DEV), workspace=ws, split_k=split)
        judge(a.t.view(m, n_out), b.t.view(m, n_out), ref, f"split {split}")


DGRAD_CASES = [
    (2, 16, 16, 64, 64, 3, 1), (2, 32, 32, 64, 128, 3, 2), (3, 16, 16, 64, 128, 1, 2), (2, 8, 8, 128, 32, 1, 1),
    (5, 64, 64, 32, 64, 3, 2), (2, 15, 17, 32, 64, 3, 2), (1, 8, 8, 512, 256, 3, 2),
]


@pytest.mark.parametrize("case", DGRAD_CASES)
def test_data_gradient_modes(case):
    from egorear_amd import hip
    n, h, w, cin, cout, k, s = case
    pad = k // 2
    x = rnd(n, cin, h, w, seed=1).double().requires_grad_(True)
    wt = rnd(cout, cin, k, k, seed=2, scale=1.0 / math.sqrt(cin * k * k))
    y = F.conv2d(x, wt.double(), None, s, pad)
    dy = rnd(*y.shape, seed=3)
    (dx_ref,) = torch.autograd.grad(y, x, dy.double())
    dy_nhwc = hip.Img(dy.permute(0, 2, 3, 1).contiguous().to(DEV))
    a, b = both(hip, dy_nhwc, pack_w_dgrad(wt), cin, k, k, s, pad, transposed_out_hw=(h, w))
    judge(a.t.permute(0, 3, 1, 2), b.t.permute(0, 3, 1, 2), dx_ref, str(case))
    # masked epilogue with an accumulated gradient (the ReLU backward fused into the launch)
    if cin % 4 == 0:
        act_fwd, prev = rnd(n, h, w, cin, seed=5), rnd(n, h, w, cin, seed=6)
        a, b = both(hip, dy_nhwc, pack_w_dgrad(wt), cin, k, k, s, pad, transposed_out_hw=(h, w), res=hip.Img(prev.to(DEV)),
                    res_mode=hip.RES_BEFORE_ACT, mask=hip.Img(act_fwd.to(DEV)))
        ref = (dx_ref.permute(0, 2, 3, 1) + prev.double()) * (act_fwd > 0)
        judge(a.t, b.t, ref, "masked " + str(case))


def test_channel_major_output_and_upsampled_residual():
    from egorear_amd import hip
    n, h, w, cin, cout = 4, 16, 16, 64, 32
    x = rnd(n, h, w, cin, seed=7).to(DEV)
    wt = rnd(cout, cin, 1, 1, seed=8, scale=0.1)
    ref = F.conv2d(x.permute(0, 3, 1, 2).cpu().double(), wt.double())
    plane = cout * h * w
    outs = []
    for wop in (pack_w(wt).to(DEV), hip.pack_w6(pack_w(wt).to(DEV))):
        out = torch.zeros(2, 2, cout, h, w, device=DEV)
        hip.conv2d(hip.Img(x), wop, cout, 1, 1, 1, 0, out_nchw=out, ymap=hip.NMap(2, 2 * plane, plane))
        outs.append(out.permute(1, 0, 2, 3, 4).reshape(n, cout, h, w))
    judge(outs[0], outs[1], ref, "nchw")
    lo = rnd(n, h // 2, w // 2, cout, seed=9)
    up = F.interpolate(lo.permute(0, 3, 1, 2).double(), scale_factor=2, mode="bilinear", align_corners=True)
    a, b = both(hip, hip.Img(x), pack_w(wt), cout, 1, 1, 1, 0, res=hip.Img(lo.to(DEV)), res_mode=hip.RES_UP2_BEFORE_ACT, act=hip.ACT_RELU)
    judge(a.t.permute(0, 3, 1, 2), b.t.permute(0, 3, 1, 2), F.relu(ref + up), "up2 residual")


def test_wide_dynamic_range_and_zero_padding_rows():
    """Operands spanning many binades (the split is exact at every magnitude) and an input with exact zeros / tiny values."""
    from egorear_amd import hip
    n, h, cin, cout = 2, 16, 64, 64
    g = torch.Generator().manual_seed(5)
    x = rnd(n, h, h, cin, seed=1) * torch.exp2(torch.randint(-20, 20, (n, h, h, cin), generator=g).float())
    x[0, :4] = 0.0
    wt = rnd(cout, cin, 3, 3, seed=2) * torch.exp2(torch.randint(-12, 4, (cout, cin, 3, 3), generator=g).float())
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), wt.double(), None, 1, 1)
    a, b = both(hip, hip.Img(x.to(DEV)), pack_w(wt), cout, 3, 3, 1, 1)
    judge(a.t.permute(0, 3, 1, 2), b.t.permute(0, 3, 1, 2), ref, "dynamic range")


TAP_CASES = [
    # n, h(=w), cin, cout, groups, extras
    (2, 64, 64, 64, 1, "res_before"),          # layer1 geometry: 64-channel tile, residual + ReLU
    (8, 32, 128, 128, 2, "scale_relu"),        # layer2 geometry, grouped, BatchNorm affine + ReLU
    (32, 16, 32, 192, 1, "plain"),             # wo = 16 (a fragment spans two image rows), 32 channels = two chunks, Npad = 192 -> 64-wide tiles
    (4, 64, 96, 256, 1, "res_after"),          # three 32-channel blocks, residual behind the activation
    (9, 32, 64, 60, 1, "nchw"),                # cout not a multiple of 32; channel-major planes out; image count odd
    (32, 64, 64, 128, 1, "scale_relu"),        # enough tiles for the 128 x 128 configuration
    (64, 64, 64, 64, 1, "res_before"),         # 64 output channels, enough tiles for the 256 x 64 configuration (four image rows per tile)
    (256, 16, 64, 192, 1, "scale_relu"),       # 256 x 64 tiles = one whole 16 x 16 image each, three column tiles
    (128, 8, 128, 128, 1, "plain"),            # 8 x 8 images: a 128-pixel tile is two whole images
    (512, 8, 64, 64, 2, "res_after"),          # 8 x 8 images, grouped, 64-wide tiles
]


@pytest.mark.parametrize("case", TAP_CASES)
def test_tap_sharing_forward_kernel(case):
    """conv_igemm_tap_kernel (3x3 / stride 1 / pad 1, tiles of whole image rows, input rows split once per 16-channel chunk and the
    nine taps read as shifted LDS windows) against fp64 and against the generic split kernel (same operands, same products: the
    two differ only in the order the accumulator receives the taps' products)."""
    from egorear_amd import hip
    n, hw, cin, cout, G, extra = case
    x = rnd(G * n, hw, hw, cin, seed=70)
    wts = [rnd(cout, cin, 3, 3, seed=71 + g, scale=1.0 / math.sqrt(9 * cin)) for g in range(G)]
    wp = torch.stack([pack_w(t) for t in wts]) if G > 1 else pack_w(wts[0])
    npad = wp.shape[-2]
    kw = dict(groups=G)
    res = None
    if extra in ("res_before", "res_after"):
        res = rnd(G * n, hw, hw, cout, seed=75)
        kw.update(res=hip.Img(res.to(DEV)), res_mode=hip.RES_BEFORE_ACT if extra == "res_before" else hip.RES_AFTER_ACT, act=hip.ACT_RELU)
    sc = sh = None
    if extra == "scale_relu":
        sc, sh = rnd(G, npad, seed=76) * 0.2 + 1.0, rnd(G, npad, seed=77)
        if G == 1:
            sc, sh = sc[0], sh[0]
        kw.update(scale=sc.to(DEV), shift=sh.to(DEV), act=hip.ACT_RELU)
    saved = hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS
    hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = 0, 0.0
    try:
        outs = {}
        for tap in (1, 0):
            hip.lib.egr_conv_set_tap(tap)
            if extra == "nchw":
                planes = torch.full((n, cout, hw, hw), 7.0, device=DEV)
                hip.conv2d(hip.Img(x.to(DEV)), hip.pack_w6(wp.to(DEV)), cout, 3, 3, 1, 1, out_nchw=planes, ymap=hip.NMap(n, cout * hw * hw, 0), **kw)
                outs[tap] = planes
            else:
                outs[tap] = hip.conv2d(hip.Img(x.to(DEV)), hip.pack_w6(wp.to(DEV)), cout, 3, 3, 1, 1, **kw).t.permute(0, 3, 1, 2)
            assert hip.lib.egr_conv_last_kernel() == (2 if tap else 1)
    finally:
        hip.lib.egr_conv_set_tap(1)
        hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = saved
    refs = []
    for g in range(G):
        r = F.conv2d(x[g * n:(g + 1) * n].permute(0, 3, 1, 2).double(), wts[g].double(), None, 1, 1)
        if extra == "scale_relu":
            s_, b_ = (sc[g], sh[g]) if G > 1 else (sc, sh)
            r = F.relu(r * s_[:cout].double().view(1, -1, 1, 1) + b_[:cout].double().view(1, -1, 1, 1))
        if extra == "res_before":
            r = F.relu(r + res[g * n:(g + 1) * n].permute(0, 3, 1, 2).double())
        if extra == "res_after":
            r = F.relu(r) + res[g * n:(g + 1) * n].permute(0, 3, 1, 2).double()
        refs.append(r)
    ref = torch.cat(refs)
    judge(outs[0], outs[1], ref, f"tap {case}")
    assert float((outs[0] - outs[1]).abs().max()) <= 4e-6 * float(ref.abs().max())


@pytest.mark.parametrize("case", [(1, 2, 64, 64, 64, False), (2, 8, 32, 128, 128, True), (1, 32, 16, 256, 96, True)])
def test_tap_sharing_data_gradient(case):
    """The same kernel in data-gradient mode (mirrored tap windows), plain and with the fused ReLU mask + accumulated gradient."""
    from egorear_amd import hip
    G, n, hw, cin, cout, masked = case          # forward conv cin -> cout; the gradient maps dy (cout) to dx (cin)
    dy = rnd(G * n, hw, hw, cout, seed=81)
    xs, prev = rnd(G * n, hw, hw, cin, seed=82), rnd(G * n, hw, hw, cin, seed=83)
    wts = [rnd(cout, cin, 3, 3, seed=84 + g, scale=1.0 / math.sqrt(9 * cin)) for g in range(G)]
    wt = (torch.stack([pack_w_dgrad(w) for w in wts]) if G > 1 else pack_w_dgrad(wts[0])).to(DEV)
    kw = dict(transposed_out_hw=(hw, hw), groups=G)
    if masked:
        kw.update(res=hip.Img(prev.to(DEV)), res_mode=hip.RES_BEFORE_ACT, mask=hip.Img(xs.to(DEV)))
    saved = hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS
    hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = 0, 0.0
    try:
        outs = {}
        for tap in (1, 0):
            hip.lib.egr_conv_set_tap(tap)
            outs[tap] = hip.conv2d(hip.Img(dy.to(DEV)), hip.pack_w6(wt), cin, 3, 3, 1, 1, **kw).t.clone()
            assert hip.lib.egr_conv_last_kernel() == (2 if tap else 1)
    finally:
        hip.lib.egr_conv_set_tap(1)
        hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = saved
    refs = []
    for g in range(G):
        xr = torch.zeros(n, cin, hw, hw, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(xr, wts[g].double(), None, 1, 1)
        (dx_ref,) = torch.autograd.grad(y, xr, dy[g * n:(g + 1) * n].permute(0, 3, 1, 2).double())
        r = dx_ref.permute(0, 2, 3, 1)
        if masked:
            r = (r + prev[g * n:(g + 1) * n].double()) * (xs[g * n:(g + 1) * n] > 0)
        refs.append(r)
    ref = torch.cat(refs)
    judge(outs[0], outs[1], ref, f"tap dgrad {case}")
    assert float((outs[0] - outs[1]).abs().max()) <= 4e-6 * float(ref.abs().max())


def test_tap_sharing_randomised_geometry():
    """Seeded sweep over tap-eligible shapes (image sizes 8-64, 1-3 input chunks, 64-256 output channels, groups, forward and data
    gradient, every tile configuration the dispatcher can pick): the tap-sharing launch must agree with the generic split launch of
    the same problem to fp32 rounding (same operands, same products), and the tap-sharing weight gradient with the generic one."""
    from egorear_amd import hip
    from egorear_amd.engine import unpack_conv_weight
    g = torch.Generator().manual_seed(4321)

    def pick(options):
        return options[int(torch.randint(len(options), (1,), generator=g))]

    saved = hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS
    hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = 0, 0.0
    ws = torch.empty(1 << 25, device=DEV)
    seen = set()
    try:
        for it in range(14):
            hw = pick([8, 16, 32, 64])
            G = pick([1, 1, 2])
            cin, cout = pick([32, 64, 96, 128]), pick([64, 128, 192, 256])
            n = max(1, (8192 * pick([1, 2, 3])) // (hw * hw))          # >= 8192 rows per group, also odd multiples of the tile
            transposed = pick([False, False, True])
            x = rnd(G * n, hw, hw, cout if transposed else cin, seed=900 + it)
            wts = [rnd(cout, cin, 3, 3, seed=950 + it * 2 + q, scale=1.0 / math.sqrt(9 * cin)) for q in range(G)]
            packer = pack_w_dgrad if transposed else pack_w
            wp = (torch.stack([packer(t) for t in wts]) if G > 1 else packer(wts[0])).to(DEV)
            kw = dict(groups=G, transposed_out_hw=(hw, hw)) if transposed else dict(groups=G, act=hip.ACT_RELU)
            outs = {}
            n_launch = cin if transposed else cout                      # output channels of the launch
            eligible = ((n_launch + 31) // 32 * 32) % 64 == 0            # the tap-sharing tiles are 64 / 128 channels wide
            for tap in (1, 0):
                hip.lib.egr_conv_set_tap(tap)
                outs[tap] = hip.conv2d(hip.Img(x.to(DEV)), hip.pack_w6(wp), n_launch, 3, 3, 1, 1, **kw).t.clone()
                assert hip.lib.egr_conv_last_kernel() == (2 if (tap and eligible) else 1), (it, hw, cin, cout, n, G, transposed)
            scale = float(outs[0].abs().max())
            assert float((outs[1] - outs[0]).abs().max()) <= 4e-6 * scale, ("tap vs generic", it, hw, cin, cout, n, G, transposed)
            if eligible:
                seen.add((hw, transposed))
            # weight gradient of the same layer
            if it % 2 == 0 and cin % 32 == 0:
                xa = rnd(G * n, cin, hw, hw, seed=1000 + it)
                dy = rnd(G * n, cout, hw, hw, seed=1100 + it)
                xi, dyi = hip.Img(xa.permute(0, 2, 3, 1).contiguous().to(DEV)), hip.Img(dy.permute(0, 2, 3, 1).contiguous().to(DEV))
                import os as _os
                d1, _ = hip.conv2d_wgrad(xi, dyi, 3, 3, 1, 1, ws, groups=G, x6="force")
                k1 = hip.lib.egr_wgrad_last_kernel()
                d1 = d1.clone()
                d0, _ = hip.conv2d_wgrad(xi, dyi, 3, 3, 1, 1, ws, groups=G, x6=False)
                assert hip.lib.egr_wgrad_last_kernel() == 0
                expect = 3 if cout % 128 == 0 else (2 if (cout % 64 == 0 and cin % 64 == 0) else 1)
                assert k1 == expect, (k1, expect, cin, cout, hw)
                sc = float(d0.abs().max())
                assert float((d1 - d0).abs().max()) <= 2e-5 * sc, ("wgrad", it, hw, cin, cout, n, G)
        assert len({h for h, _ in seen}) >= 3
    finally:
        hip.lib.egr_conv_set_tap(1)
        hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = saved


TAP2_CASES = [
    # n, h(=w, input), cin, cout, groups, extras
    (8, 64, 64, 128, 1, "scale_relu"),         # layer2 entry: 64 -> 32 pixels, four output rows per tile
    (16, 32, 128, 256, 2, "scale_relu"),       # layer3 entry, grouped: 16 x 16 outputs, a tile is half an image
    (64, 16, 256, 512, 1, "plain"),            # layer4 entry: 8 x 8 outputs, a tile is two whole images; enough tiles for 128 x 128
    (32, 32, 32, 192, 1, "res_after"),         # two chunks only, Npad = 192 -> 64-wide tiles, residual behind the ReLU
    (9 * 2, 32, 96, 60, 1, "plain"),           # cout not a multiple of 32 (Npad 64), three 32-channel blocks
    (128, 64, 64, 128, 1, "plain"),            # many tiles: the 128 x 128 configuration on 32-pixel output rows
]


@pytest.mark.parametrize("case", TAP2_CASES)
def test_tap_sharing_stride2_kernel(case):
    """conv_igemm_tap2_kernel (3x3 / stride 2 / pad 1 on even images: the input rows of a tile are staged once per 16-channel chunk
    as four parity-class planes, the nine taps read them as shifted LDS windows) against fp64 and the generic split kernel."""
    from egorear_amd import hip
    n, hw, cin, cout, G, extra = case
    ho = hw // 2
    x = rnd(G * n, hw, hw, cin, seed=170)
    wts = [rnd(cout, cin, 3, 3, seed=171 + g, scale=1.0 / math.sqrt(9 * cin)) for g in range(G)]
    wp = torch.stack([pack_w(t) for t in wts]) if G > 1 else pack_w(wts[0])
    npad = wp.shape[-2]
    kw = dict(groups=G)
    res = sc = sh = None
    if extra == "res_after":
        res = rnd(G * n, ho, ho, cout, seed=175)
        kw.update(res=hip.Img(res.to(DEV)), res_mode=hip.RES_AFTER_ACT, act=hip.ACT_RELU)
    if extra == "scale_relu":
        sc, sh = rnd(G, npad, seed=176) * 0.2 + 1.0, rnd(G, npad, seed=177)
        if G == 1:
            sc, sh = sc[0], sh[0]
        kw.update(scale=sc.to(DEV), shift=sh.to(DEV), act=hip.ACT_RELU)
    saved = hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS
    hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = 0, 0.0
    try:
        outs = {}
        for tap in (1, 0):
            hip.lib.egr_conv_set_tap(tap)
            outs[tap] = hip.conv2d(hip.Img(x.to(DEV)), hip.pack_w6(wp.to(DEV)), cout, 3, 3, 2, 1, **kw).t.permute(0, 3, 1, 2).clone()
            assert hip.lib.egr_conv_last_kernel() == (3 if tap else 1)
    finally:
        hip.lib.egr_conv_set_tap(1)
        hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = saved
    refs = []
    for g in range(G):
        r = F.conv2d(x[g * n:(g + 1) * n].permute(0, 3, 1, 2).double(), wts[g].double(), None, 2, 1)
        if extra == "scale_relu":
            s_, b_ = (sc[g], sh[g]) if G > 1 else (sc, sh)
            r = F.relu(r * s_[:cout].double().view(1, -1, 1, 1) + b_[:cout].double().view(1, -1, 1, 1))
        if extra == "res_after":
            r = F.relu(r) + res[g * n:(g + 1) * n].permute(0, 3, 1, 2).double()
        refs.append(r)
    ref = torch.cat(refs)
    judge(outs[0], outs[1], ref, f"tap2 {case}")
    assert float((outs[0] - outs[1]).abs().max()) <= 4e-6 * float(ref.abs().max())


PW_CASES = [
    # n, h, w, cin, cout, groups, extras
    (16, 64, 64, 128, 128, 1, "scale_relu"),       # K = N = 128: the FPN / head 1x1 layers
    (8, 64, 64, 128, 256, 2, "plain"),             # two channel tiles per group (weights of one tile per workgroup), grouped
    (16, 64, 64, 64, 128, 1, "res_after"),         # cin = 64 (four k steps), residual behind the ReLU
    (32, 32, 64, 128, 64, 1, "res_before"),        # 64 output channels (two fragments), non-square image
    (19, 60, 60, 128, 60, 1, "scale_relu"),        # image size not a power of two, ragged last tile, cout not a multiple of 32
    (16, 64, 64, 128, 128, 1, "up2"),              # FPN top-down: half-resolution residual up-sampled in the epilogue
    (8, 64, 64, 64, 64, 2, "up2"),                 # the same, grouped, 64 channels
    (5, 128, 128, 64, 192, 1, "plain"),            # Npad = 192 -> 64-channel tiles, three of them
    (64, 64, 64, 64, 128, 1, "stride2_scale"),     # 1x1 / stride 2 (the residual blocks' down-sampling convs), BatchNorm affine, no ReLU
    (37, 62, 62, 128, 256, 2, "stride2_scale"),    # the same: odd-sized output grid (31 x 31), grouped, ragged last tile
    (457, 12, 12, 64, 64, 1, "up2"),               # up-sampled residual on an image that is no power of two (the decode divides), ragged last tile
    (457, 12, 12, 64, 64, 1, "res_before"),        # the same image with a residual of the output's shape
]


@pytest.mark.parametrize("case", PW_CASES)
def test_streaming_1x1_kernel(case):
    """conv_pw_x6_kernel (1x1 / stride 1, cin 64 / 128, many pixels: weights stationary in LDS, a lane owns a pixel, activations
    go global -> registers -> MFMA, stores from the accumulator registers) against fp64 and the tiled split kernel."""
    from egorear_amd import hip
    n, h, w, cin, cout, G, extra = case
    stride = 2 if extra.startswith("stride2") else 1
    x = rnd(G * n, h, w, cin, seed=270)
    wts = [rnd(cout, cin, 1, 1, seed=271 + g, scale=1.0 / math.sqrt(cin)) for g in range(G)]
    wp = torch.stack([pack_w(t) for t in wts]) if G > 1 else pack_w(wts[0])
    npad = wp.shape[-2]
    kw = dict(groups=G)
    res = sc = sh = None
    if extra in ("res_before", "res_after"):
        res = rnd(G * n, h, w, cout, seed=275)
        kw.update(res=hip.Img(res.to(DEV)), res_mode=hip.RES_BEFORE_ACT if extra == "res_before" else hip.RES_AFTER_ACT, act=hip.ACT_RELU)
    if extra == "up2":
        res = rnd(G * n, h // 2, w // 2, cout, seed=275)
        kw.update(res=hip.Img(res.to(DEV)), res_mode=hip.RES_UP2_BEFORE_ACT, act=hip.ACT_RELU)
    if extra in ("scale_relu", "stride2_scale"):
        sc, sh = rnd(G, npad, seed=276) * 0.2 + 1.0, rnd(G, npad, seed=277)
        if G == 1:
            sc, sh = sc[0], sh[0]
        kw.update(scale=sc.to(DEV), shift=sh.to(DEV), act=hip.ACT_RELU if extra == "scale_relu" else hip.ACT_NONE)
    saved = hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS
    hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = 0, 0.0
    try:
        outs = {}
        for tap in (1, 0):
            hip.lib.egr_conv_set_tap(tap)
            outs[tap] = hip.conv2d(hip.Img(x.to(DEV)), hip.pack_w6(wp.to(DEV)), cout, 1, 1, stride, 0, **kw).t.permute(0, 3, 1, 2).clone()
            assert hip.lib.egr_conv_last_kernel() == (4 if tap else 1)
    finally:
        hip.lib.egr_conv_set_tap(1)
        hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = saved
    refs = []
    for g in range(G):
        r = F.conv2d(x[g * n:(g + 1) * n].permute(0, 3, 1, 2).double(), wts[g].double(), None, stride, 0)
        rg = res[g * n:(g + 1) * n].permute(0, 3, 1, 2).double() if res is not None else None
        if extra in ("scale_relu", "stride2_scale"):
            s_, b_ = (sc[g], sh[g]) if G > 1 else (sc, sh)
            r = r * s_[:cout].double().view(1, -1, 1, 1) + b_[:cout].double().view(1, -1, 1, 1)
            if extra == "scale_relu":
                r = F.relu(r)
        if extra == "res_before":
            r = F.relu(r + rg)
        if extra == "res_after":
            r = F.relu(r) + rg
        if extra == "up2":
            r = F.relu(r + F.interpolate(rg, scale_factor=2, mode="bilinear", align_corners=True))
        refs.append(r)
    ref = torch.cat(refs)
    judge(outs[0], outs[1], ref, f"streaming 1x1 {case}")
    assert float((outs[0] - outs[1]).abs().max()) <= 4e-6 * float(ref.abs().max())


def test_tap_sharing_stride2_operand_placement():
    """The stride-2 tap-sharing kernel with the input as a channel slice of a wider tensor stored frame-major behind a
    (view, frame) -> (frame, view) image map, 8 x 8 outputs (a tile spans two images), the output into a channel slice."""
    from egorear_amd import hip
    V, B, h, cin, cout = 4, 8, 16, 64, 128            # n = v * B + b = 32 images of 16 x 16 -> 8 x 8: 2048 output pixels
    n = V * B
    x = rnd(n, h, h, cin, seed=411)                                       # launch order (view-major)
    stored = torch.zeros(B, V, h, h, 2 * cin)
    stored[..., cin:] = x.view(V, B, h, h, cin).permute(1, 0, 2, 3, 4)
    stored[..., :cin] = 9.0
    stored = stored.to(DEV)
    wt = rnd(cout, cin, 3, 3, seed=412, scale=1.0 / math.sqrt(9 * cin))
    ref = F.relu(F.conv2d(x.permute(0, 3, 1, 2).double(), wt.double(), None, 2, 1))
    img = h * h * 2 * cin
    saved = hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS
    hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = 0, 0.0
    try:
        cat = torch.full((n, h // 2, h // 2, 2 * cout), 5.0, device=DEV)
        hip.conv2d(hip.Img(stored.view(n, h, h, 2 * cin)[..., cin:]), hip.pack_w6(pack_w(wt).to(DEV)), cout, 3, 3, 2, 1, act=hip.ACT_RELU,
                   xmap=hip.NMap(B, V * img, img), out=hip.Img(cat[..., cout:]))
        assert hip.lib.egr_conv_last_kernel() == 3
    finally:
        hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = saved
    err = float((cat[..., cout:].permute(0, 3, 1, 2).double().cpu() - ref).abs().max()) / float(ref.abs().max())
    assert err <= 2e-5, err
    assert float((cat[..., :cout] - 5.0).abs().max()) == 0


def test_streaming_1x1_kernel_operand_placement():
    """The streaming kernel with every operand placed the way the engine places them: input and residual as channel slices of wider
    tensors (row stride > channels), the output written into a channel slice of a wider buffer (its neighbours untouched), and a
    (view, frame) -> (frame, view) image map on the input and the output."""
    from egorear_amd import hip
    V, B, h, cin, cout = 4, 4, 64, 128, 128           # n = v * B + b; 65536 pixels
    n = V * B
    wide = rnd(n, h, h, 2 * cin, seed=401).to(DEV)                      # the conv reads channels cin .. 2 cin
    reswide = rnd(n, h, h, cout + 64, seed=402).to(DEV)                 # the residual is channels 32 .. 32 + cout
    wt = rnd(cout, cin, 1, 1, seed=403, scale=1.0 / math.sqrt(cin))
    sh = rnd(cout, seed=404).to(DEV)
    ref = F.relu(F.conv2d(wide[..., cin:].permute(0, 3, 1, 2).cpu().double(), wt.double()) + sh.cpu().double().view(1, -1, 1, 1)
                 + reswide[..., 32:32 + cout].permute(0, 3, 1, 2).cpu().double())
    saved = hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS
    hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = 0, 0.0
    try:
        cat = torch.full((n, h, h, 3 * cout), 5.0, device=DEV)
        hip.conv2d(hip.Img(wide[..., cin:]), hip.pack_w6(pack_w(wt).to(DEV)), cout, 1, 1, 1, 0, shift=sh, act=hip.ACT_RELU,
                   res=hip.Img(reswide[..., 32:32 + cout]), res_mode=hip.RES_BEFORE_ACT, out=hip.Img(cat[..., cout:2 * cout]))
        assert hip.lib.egr_conv_last_kernel() == 4
        err = float((cat[..., cout:2 * cout].permute(0, 3, 1, 2).double().cpu() - ref).abs().max()) / float(ref.abs().max())
        assert err <= 2e-5, err
        assert float((cat[..., :cout] - 5.0).abs().max()) == 0 and float((cat[..., 2 * cout:] - 5.0).abs().max()) == 0
        # image maps: the input batch is stored frame-major (b, v), the launch enumerates view-major (n = v * B + b) and writes view-major
        xbv = wide[..., cin:].reshape(V, B, h, h, cin).permute(1, 0, 2, 3, 4).contiguous()      # (B, V, ...)
        img = h * h * cin
        out = torch.zeros(n, h, h, cout, device=DEV)
        hip.conv2d(hip.Img(xbv.view(n, h, h, cin)), hip.pack_w6(pack_w(wt).to(DEV)), cout, 1, 1, 1, 0, shift=sh,
                   xmap=hip.NMap(B, V * img, img), out=hip.Img(out))
        assert hip.lib.egr_conv_last_kernel() == 4
        ref2 = F.conv2d(wide[..., cin:].permute(0, 3, 1, 2).cpu().double(), wt.double()) + sh.cpu().double().view(1, -1, 1, 1)
        err = float((out.permute(0, 3, 1, 2).double().cpu() - ref2).abs().max()) / float(ref2.abs().max())
        assert err <= 2e-5, err
    finally:
        hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = saved


@pytest.mark.parametrize("case", [(1, 16, 64, 128, 128, True), (2, 8, 64, 64, 128, True), (1, 16, 64, 128, 64, False)])
def test_streaming_1x1_data_gradient(case):
    """The streaming kernel as the data gradient of a 1x1 convolution (the same launch with the transposed matrix), plain and with the
    fused ReLU mask + accumulated gradient of the training step."""
    from egorear_amd import hip
    G, n, hw, cin, cout, masked = case          # forward conv cin -> cout; the gradient maps dy (cout) to dx (cin)
    dy = rnd(G * n, hw, hw, cout, seed=281)
    xs, prev = rnd(G * n, hw, hw, cin, seed=282), rnd(G * n, hw, hw, cin, seed=283)
    wts = [rnd(cout, cin, 1, 1, seed=284 + g, scale=1.0 / math.sqrt(cin)) for g in range(G)]
    wt = (torch.stack([pack_w_dgrad(w) for w in wts]) if G > 1 else pack_w_dgrad(wts[0])).to(DEV)
    kw = dict(transposed_out_hw=(hw, hw), groups=G)
    if masked:
        kw.update(res=hip.Img(prev.to(DEV)), res_mode=hip.RES_BEFORE_ACT, mask=hip.Img(xs.to(DEV)))
    saved = hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS
    hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = 0, 0.0
    try:
        outs = {}
        for tap in (1, 0):
            hip.lib.egr_conv_set_tap(tap)
            outs[tap] = hip.conv2d(hip.Img(dy.to(DEV)), hip.pack_w6(wt), cin, 1, 1, 1, 0, **kw).t.clone()
            assert hip.lib.egr_conv_last_kernel() == (4 if tap else 1)
    finally:
        hip.lib.egr_conv_set_tap(1)
        hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = saved
    refs = []
    for g in range(G):
        r = torch.einsum("nhwo,oi->nhwi", dy[g * n:(g + 1) * n].double(), wts[g][:, :, 0, 0].double())
        if masked:
            r = (r + prev[g * n:(g + 1) * n].double()) * (xs[g * n:(g + 1) * n] > 0)
        refs.append(r)
    ref = torch.cat(refs)
    judge(outs[0], outs[1], ref, f"streaming 1x1 dgrad {case}")
    assert float((outs[0] - outs[1]).abs().max()) <= 4e-6 * float(ref.abs().max())


WGRAD_CASES = [
    # n, h, w, cin, cout, k, stride, groups
    (8, 32, 32, 64, 64, 3, 1, 1),        # 64-wide output tile (BCO = 64), 8192 pixels
    (8, 32, 32, 64, 128, 3, 2, 2),       # stride 2, grouped
    (4, 64, 64, 128, 128, 1, 1, 1),      # 1x1
    (9, 32, 32, 32, 96, 3, 1, 1),        # cout not a multiple of 32, ragged K tile (9 chunks)
    (2, 64, 64, 256, 256, 3, 1, 1),      # deeper K: several K tiles
    (3, 61, 45, 64, 128, 3, 1, 1),       # odd sizes: pixel count not a multiple of the stage
    (4, 48, 48, 64, 64, 3, 1, 2),        # tap-sharing kernel, 64 x 2 chunks: width not a power of two, grouped
    (2, 16, 32, 128, 128, 3, 1, 3),      # tap-sharing kernel, 128 x 1 chunk: h != w, three groups
    (3, 16, 16, 128, 64, 3, 1, 1),       # 64 output channels, two input-chunk tiles
    (1, 16, 16, 64, 256, 3, 1, 1),       # two output-channel tiles x two input chunks, one image
    (6, 8, 8, 256, 128, 3, 1, 1),        # 8-pixel-wide images: a stage is two rows (layer4's geometry)
    (5, 8, 8, 64, 64, 3, 1, 2),
]
# kernel egr_wgrad_last_kernel() must report for the forced split launch of each case (1 generic, 2 / 3 tap-sharing)
WGRAD_KERNEL = [2, 1, 1, 1, 3, 1, 2, 3, 2, 3, 3, 2]


@pytest.mark.parametrize("case", WGRAD_CASES)
def test_weight_gradient_split_launch(case):
    """conv_wgrad_x6_kernel (both operands split on the fly, transposing LDS reads) against the fp32 kernel and fp64 autograd."""
    from egorear_amd import hip
    from egorear_amd.engine import unpack_conv_weight
    n, h, w, cin, cout, k, s, G = case
    pad = k // 2
    x = rnd(G * n, cin, h, w, seed=21)
    ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    dy = rnd(G * n, cout, ho, wo, seed=22)
    ws = torch.empty(1 << 25, device=DEV)
    xi, dyi = hip.Img(x.permute(0, 2, 3, 1).contiguous().to(DEV)), hip.Img(dy.permute(0, 2, 3, 1).contiguous().to(DEV))
    out = {}
    for fmt in (False, "force"):
        dw, db = hip.conv2d_wgrad(xi, dyi, k, k, s, pad, ws, want_bias=True, groups=G, x6=fmt)
        out[bool(fmt)] = (dw.clone(), db.clone())
        assert hip.lib.egr_wgrad_last_kernel() == (WGRAD_KERNEL[WGRAD_CASES.index(case)] if fmt else 0)
    for g in range(G):
        wt = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x[g * n:(g + 1) * n].double(), wt, b, s, pad)
        dw_ref, db_ref = torch.autograd.grad(y, (wt, b), dy[g * n:(g + 1) * n].double())
        dwa = out[False][0][g] if G > 1 else out[False][0]
        dwb = out[True][0][g] if G > 1 else out[True][0]
        judge(unpack_conv_weight(dwa, cin, k, k), unpack_conv_weight(dwb, cin, k, k), dw_ref, f"dw {case} g{g}")


def test_randomised_shapes_split_vs_fp32_launches():
    """Seeded sweep over shapes the fixed cases do not hit (ragged tiles in both directions, 5x5 kernels, three groups, every
    tile configuration, forward and data-gradient mode, stride 2 with odd and even sizes): the split launch (forced on at any
    size) must agree with the fp32 launch of the same problem to fp32 rounding, and the split weight gradient with the fp32 one."""
    from egorear_amd import hip
    g = torch.Generator().manual_seed(1234)

    def pick(options):
        return options[int(torch.randint(len(options), (1,), generator=g))]

    saved = hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS
    hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = 0, 0.0
    ws = torch.empty(1 << 24, device=DEV)
    try:
        for it in range(48):
            G = pick([1, 1, 2, 3])
            n, h, w = pick([1, 2, 3, 5]), pick([5, 8, 13, 16, 33]), pick([4, 8, 11, 16, 32])
            cin, cout = pick([32, 64, 96, 160]), pick([8, 15, 32, 48, 64, 100, 128, 200])
            k, s = pick([1, 3, 3, 5]), pick([1, 1, 2])
            pad = k // 2
            cfg = pick([-1, -1, 0, 1, 2, 3, 4])
            transposed = pick([False, False, True])
            ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
            wts = [rnd(cout, cin, k, k, seed=100 + it * 4 + q, scale=1.0 / math.sqrt(cin * k * k)) for q in range(G)]
            hip.conv_force_config(cfg)
            try:
                if not transposed:
                    x = rnd(G * n, h, w, cin, seed=it)
                    wp = torch.stack([pack_w(t) for t in wts]) if G > 1 else pack_w(wts[0])
                    a, b = both(hip, hip.Img(x.to(DEV)), wp, cout, k, k, s, pad, groups=G, workspace=ws, split_k=pick([1, 0]))
                    ref = torch.cat([F.conv2d(x[q * n:(q + 1) * n].permute(0, 3, 1, 2).double(), wts[q].double(), None, s, pad) for q in range(G)])
                    judge(a.t.permute(0, 3, 1, 2), b.t.permute(0, 3, 1, 2), ref, f"fwd it{it} G{G} n{n} {h}x{w} {cin}->{cout} k{k}s{s} cfg{cfg}")
                else:
                    if cout % 32:
                        continue        # the data gradient's K side is the forward cout: padded to 32 by the caller in the model
                    dy = rnd(G * n, ho, wo, cout, seed=it)
                    wp = torch.stack([pack_w_dgrad(t) for t in wts]) if G > 1 else pack_w_dgrad(wts[0])
                    a, b = both(hip, hip.Img(dy.to(DEV)), wp, cin, k, k, s, pad, groups=G, transposed_out_hw=(h, w))
                    refs = []
                    for q in range(G):
                        xr = torch.zeros(n, cin, h, w, dtype=torch.float64, requires_grad=True)
                        y = F.conv2d(xr, wts[q].double(), None, s, pad)
                        refs.append(torch.autograd.grad(y, xr, dy[q * n:(q + 1) * n].permute(0, 3, 1, 2).double())[0])
                    judge(a.t.permute(0, 3, 1, 2), b.t.permute(0, 3, 1, 2), torch.cat(refs), f"dgrad it{it} G{G} n{n} {h}x{w} {cin}->{cout} k{k}s{s} cfg{cfg}")
            finally:
                hip.conv_force_config(-1)
            # weight gradient of the same layer (cout must be a multiple of 4 there)
            if cout % 4 == 0 and it % 2 == 0:
                from egorear_amd.engine import unpack_conv_weight
                x = rnd(G * n, cin, h, w, seed=it + 500)
                dyw = rnd(G * n, cout, ho, wo, seed=it + 600)
                xi, dyi = hip.Img(x.permute(0, 2, 3, 1).contiguous().to(DEV)), hip.Img(dyw.permute(0, 2, 3, 1).contiguous().to(DEV))
                d0, _ = hip.conv2d_wgrad(xi, dyi, k, k, s, pad, ws, groups=G, x6=False)
                d0 = d0.clone()
                d1, _ = hip.conv2d_wgrad(xi, dyi, k, k, s, pad, ws, groups=G, x6="force")
                for q in range(G):
                    wt = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
                    y = F.conv2d(x[q * n:(q + 1) * n].double(), wt, None, s, pad)
                    (dw_ref,) = torch.autograd.grad(y, wt, dyw[q * n:(q + 1) * n].double())
                    judge(unpack_conv_weight(d0[q] if G > 1 else d0, cin, k, k), unpack_conv_weight(d1[q] if G > 1 else d1, cin, k, k), dw_ref,
                          f"wgrad it{it} G{G} n{n} {h}x{w} {cin}->{cout} k{k}s{s}")
    finally:
        hip.X6_MIN_ROWS, hip.X6_MIN_FLOPS = saved


def test_pack_many_equals_single_launches():
    from egorear_amd import hip
    ws = [rnd(64, 9 * 32, seed=1).to(DEV), rnd(3, 160, 128, seed=2).to(DEV), rnd(32, 4096, seed=3).to(DEV), rnd(2, 96, 64, seed=4).to(DEV)]
    single = [hip.pack_w6(w) for w in ws]
    many = [hip.pack_w6(w) for w in ws]
    for w6 in many:
        w6.img.zero_()
    hip.W6Table(many).run()
    for a, b in zip(single, many):
        assert torch.equal(a.img.view(torch.int16), b.img.view(torch.int16))


# --------------------------------------------------------------------------- corner cases of the split

def _corner_case(hip, x, cin=64, cout=64, seed=11):
    w = rnd(cout, cin, 3, 3, seed=seed, scale=0.2)
    wp = pack_w(w)
    a, b = both(hip, hip.Img(x.to(DEV)), wp, cout, 3, 3, 1, 1)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), padding=1).permute(0, 2, 3, 1)
    return a.t.cpu(), b.t.cpu(), ref


def test_split_launch_with_an_infinite_operand_pins_the_documented_behaviour():
    """An Inf operand: the fp32 matrix cores return +-Inf (or NaN where +Inf and -Inf meet), the split launch returns NaN there
    (mid = bf16(Inf - Inf)).  Documented difference; what both must guarantee: every output whose receptive field
    holds the Inf is non-finite - never a finite wrong number - and every other output is untouched."""
    from egorear_amd import hip
    x = rnd(2, 16, 16, 64, seed=1)
    x[1, 5, 7, 9] = float("inf")
    a, b, ref = _corner_case(hip, x)
    hit = torch.zeros(2, 16, 16, dtype=torch.bool)
    hit[1, 4:7, 6:9] = True
    assert not torch.isfinite(a[hit]).any() and not torch.isfinite(b[hit]).any()
    assert torch.isnan(b[hit]).all()                              # the split launch: NaN, as documented
    fin = ~hit
    scale = float(ref[fin].abs().max())
    assert torch.isfinite(a[fin]).all() and torch.isfinite(b[fin]).all()
    assert float((b[fin].double() - ref[fin]).abs().max()) <= 2e-5 * scale


def test_split_launch_propagates_nan_like_the_fp32_launch():
    from egorear_amd import hip
    x = rnd(1, 16, 16, 64, seed=2)
    x[0, 0, 0, 0] = float("nan")
    a, b, ref = _corner_case(hip, x)
    hit = torch.zeros(1, 16, 16, dtype=torch.bool)
    hit[0, 0:2, 0:2] = True
    assert torch.isnan(a[hit]).all() and torch.isnan(b[hit]).all()
    assert torch.isfinite(b[~hit]).all()


def test_split_launch_on_subnormal_and_tiny_operands_stays_within_the_documented_bound():
    """Operands below ~2^-110 lose their mid / lo planes to bf16 underflow: the split is then no longer exact, but the ABSOLUTE
    error stays far below anything representable next to normal activations (documented: < 2^-126 per product; here the bound is
    checked on the accumulated result)."""
    from egorear_amd import hip
    for mag, bound in ((2.0 ** -112, 2.0 ** -112), (1e-40, 1e-38)):     # tiny normals, subnormals
        x = rnd(1, 16, 16, 64, seed=3) * mag
        a, b, ref = _corner_case(hip, x)
        assert torch.isfinite(b).all() and torch.isfinite(a).all()
        assert float((b.double() - ref).abs().max()) <= bound, mag      # absolute, not relative
    # and a mix: tiny values next to normal ones do not disturb the normal ones
    x = rnd(1, 16, 16, 64, seed=4)
    x[..., ::2] *= 2.0 ** -115
    a, b, ref = _corner_case(hip, x)
    judge(a, b, ref, "tiny next to normal")


# --------------------------------------------------------------------------- persistent launches (short-K layers)

@pytest.mark.parametrize("cin,cout,k,res_mode", [(128, 128, 1, 0), (128, 128, 1, 1), (64, 128, 1, 0), (128, 256, 1, 2), (64, 256, 1, 0),
                                                 (32, 128, 3, 0), (256, 128, 1, 1)])
def test_persistent_split_launches_match_fp64(cin, cout, k, res_mode):
    """The persistent variant of the split kernel (a workgroup walks several tiles; the next tile's row table is decoded and its
    first operands requested under the current tile's stores): forced onto small problems with 8 workgroup slots, so that every
    workgroup walks many tiles incl. a ragged last round."""
    from egorear_amd import hip
    n, h, w = 3, 20, 44                              # M = 2640 rows: 21 tiles of 128 (the last one ragged), 2 column tiles for cout 256
    x = rnd(n, h, w, cin, seed=cin + cout)
    wt = rnd(cout, cin, k, k, seed=7, scale=0.2)
    sc, sh = torch.rand(cout) + 0.5, rnd(cout, seed=9)
    res = rnd(n, h, w, cout, seed=10) if res_mode else None
    hip.conv_set_persist(8, 16)
    try:
        a, b = both(hip, hip.Img(x.to(DEV)), pack_w(wt), cout, k, k, 1, k // 2, scale=sc.to(DEV), shift=sh.to(DEV), act=1,
                    res=hip.Img(res.to(DEV)) if res_mode else None, res_mode=res_mode, split_k=1)
    finally:
        hip.conv_set_persist(512, 4)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), wt.double(), padding=k // 2).permute(0, 2, 3, 1) * sc.double() + sh.double()
    if res_mode == 1:
        ref = ref + res.double()
    ref = ref.clamp_min(0)
    if res_mode == 2:
        ref = ref + res.double()
    judge(a.t, b.t, ref, f"persistent cin{cin} cout{cout} k{k} res{res_mode}")

"""egr_conv_aux.in_mode = EGR_IN_UP2_RELU on the GPU: the streaming 1x1 kernel that interpolates ReLU(up2(x)) from the half-resolution
x as it loads it - and, asked to, writes that operand out - against egr_upsample2x_nhwc_f32(relu = 1) followed by the plain launch.
Same interpolated fp32 values, same fp16 planes, same product order: every comparison here is for EQUAL BITS, none has a tolerance.
Host-side decisions (plans, refusals): tests/test_up2_on_load_host.py."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CIN = 128


def _rand(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _record(x: torch.Tensor, factor: float = 1.0) -> torch.Tensor:
    """The abs-max record a producing launch would leave for x (64 int32 slots of float bits), optionally `factor` too large."""
    rec = torch.zeros(64, dtype=torch.int32)
    rec[5] = torch.tensor([float(x.abs().max()) * factor], dtype=torch.float32).view(torch.int32)[0]
    return rec.to(DEV)


def _both(hip, n, hs, ws, groups, cout, seed, factor=1.0, side=True):
    """(plain: up-sampling launch + conv, fused: the conv in the input mode) -> ((y, record, operand), (y, record, operand), plan)."""
    x = _rand(n, hs, ws, CIN, seed=seed).to(DEV)                       # both signs: the ReLU acts on about half of the operand
    npad = (cout + 31) // 32 * 32
    wshape = (groups, npad, CIN) if groups > 1 else (npad, CIN)
    w6 = hip.add_wh2(hip.pack_w6((_rand(*wshape, seed=seed + 1) * 0.05).to(DEV)))
    shift = (_rand(*wshape[:-1], seed=seed + 2) * 0.1).to(DEV)
    rec = _record(x, factor)
    kw = dict(shift=shift, act=hip.ACT_RELU, groups=groups)
    r0 = torch.zeros(64, dtype=torch.int32, device=DEV)
    full = hip.upsample2x(hip.Img(x, amax=rec), relu=True)
    y0 = hip.conv2d(full, w6, cout, 1, 1, 1, 0, amax_out=r0, **kw)
    assert hip.lib.egr_conv_last_kernel() == hip.ROUTE_STREAM_1X1
    r1 = torch.zeros(64, dtype=torch.int32, device=DEV)
    op = hip.Img(torch.full((n, 2 * hs, 2 * ws, CIN), float("nan"), device=DEV)) if side else None
    hip.PLAN_LOG = []
    try:
        y1 = hip.conv2d(hip.Img(x, amax=rec), w6, cout, 1, 1, 1, 0, amax_out=r1, up2_in=True, up2_out=op, **kw)
        plan = hip.PLAN_LOG[-1][1]
    finally:
        hip.PLAN_LOG = None
    assert y1 is not None, "the library refused the launch in the input mode"
    assert hip.lib.egr_conv_last_kernel() == hip.ROUTE_STREAM_1X1
    torch.cuda.synchronize()
    return (y0.t, r0, full), (y1.t, r1, op), plan


# (images, source height, source width, groups, cout): 65 536 output pixels each - the smallest launch the streaming route accepts;
# a wave's 32 pixels are half an output row (32 x 32 source), a quarter (16 x 64) or a whole one (64 x 16: the 17-pixel window starts
# at column 0 of every row); one and four groups, two and four 32-column fragments per workgroup
CASES = [(16, 32, 32, 1, 64), (16, 32, 32, 1, 128), (16, 16, 64, 1, 64), (16, 64, 16, 1, 128), (16, 32, 32, 4, 64), (16, 32, 32, 4, 128)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_%dx%d_g%d_c%d" % c)
def test_input_mode_equals_upsample_then_conv(case):
    from egorear_amd import hip
    n, hs, ws, groups, cout = case
    (y0, r0, full), (y1, r1, op), plan = _both(hip, n, hs, ws, groups, cout, seed=11 + cout + groups)
    assert plan.variant == 2000 + 800 + (20 if cout == 64 else 40) and plan.planes == 2
    assert float((full.t == 0).float().mean()) > 0.2 and float((full.t > 0).float().mean()) > 0.2      # the ReLU acted
    assert torch.equal(op.t.view(torch.int32), full.t.view(torch.int32)), "operand written out differs from egr_upsample2x_nhwc_f32"
    assert torch.equal(y1.view(torch.int32), y0.view(torch.int32)), "conv output differs"
    assert torch.equal(r1, r0) and int(r0.max()) > 0, "abs-max record differs"
    assert op.amax is not None and full.amax is not None and op.amax.data_ptr() == full.amax.data_ptr()   # the source's record rides on


@pytest.mark.parametrize("cout", [64, 128])
def test_input_mode_without_the_operand_written_out(cout):
    from egorear_amd import hip
    (y0, r0, _), (y1, r1, op), plan = _both(hip, 16, 32, 32, 1, cout, seed=3, side=False)
    assert op is None and plan.variant == 1000 + 800 + (20 if cout == 64 else 40)
    assert torch.equal(y1.view(torch.int32), y0.view(torch.int32)) and torch.equal(r1, r0)


def test_record_too_large_by_64():
    """A record 2^6 above the tensor's true abs-max (any upper bound serves): both paths take the same, smaller pre-scale."""
    from egorear_amd import hip
    (y0, r0, full), (y1, r1, op), _ = _both(hip, 16, 32, 32, 1, 64, seed=5, factor=64.0)
    assert torch.equal(op.t.view(torch.int32), full.t.view(torch.int32))
    assert torch.equal(y1.view(torch.int32), y0.view(torch.int32)) and torch.equal(r1, r0)


def test_refused_launch_returns_none_and_launches_nothing():
    """Below the streaming route's row count the library has no kernel for the mode: hip.conv2d reports it, the caller up-samples."""
    from egorear_amd import hip
    x = _rand(8, 32, 32, CIN, seed=1).to(DEV)
    w6 = hip.add_wh2(hip.pack_w6((_rand(64, CIN, seed=2) * 0.05).to(DEV)))
    hip.PROFILE = []
    try:
        y = hip.conv2d(hip.Img(x, amax=_record(x)), w6, 64, 1, 1, 1, 0, act=hip.ACT_RELU, up2_in=True)
        launched = [e[0] for e in hip.PROFILE]
    finally:
        hip.PROFILE = None
    assert y is None and not [nm for nm in launched if "conv" in nm or "upsample" in nm]


@pytest.fixture(scope="module")
def net_img():
    from egorear_amd import configs, synth
    from egorear_amd.estimator import EgoPoseFormerMVFEX
    net = EgoPoseFormerMVFEX(**copy.deepcopy(configs.pose3d_cfg("ego4view_syn"))).eval()
    synth.load_synth(net, 42)
    # batch 4: 16 images of 64 x 64 = the 65 536 rows from which conv_frame_feat[0] is a streaming launch (batch 2 stays below:
    # there the field changes nothing)
    net, img = net.to(DEV), synth.synth_images(4, 4, seed=7).to(DEV)
    with torch.no_grad():
        net(img)                 # the first forward packs the weights: the launch lists compared below are those of later ones
    torch.cuda.synchronize()
    return net, img


def _forward(hip, net, img, on: bool):
    hip.PROFILE = []
    try:
        with torch.no_grad(), hip.use_policy(hip.POLICY.replace(up2_on_load=on)):
            preds, hms = net(img)
        torch.cuda.synchronize()
        names = [e[0] for e in hip.PROFILE]
    finally:
        hip.PROFILE = None
    return [p.clone() for p in preds], [h.clone() for h in hms], names


def test_whole_network_policy_on_equals_off(net_img):
    from egorear_amd import hip
    net, img = net_img
    p_on, h_on, n_on = _forward(hip, net, img, True)
    p_off, h_off, n_off = _forward(hip, net, img, False)
    assert len(p_on) == len(p_off) and len(h_on) == len(h_off) == 2
    for a, b in zip(p_on + h_on, p_off + h_off):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the full-resolution up-sampling launches of the forward: the refined features' own goes, nothing else changes
    up = "egr_upsample2x_nhwc_f32"
    assert n_off.count(up) == n_on.count(up) + 1 and len(n_off) == len(n_on) + 1
    assert sorted(n_off) == sorted(n_on + [up])


def test_heatmap_estimator_still_returns_the_refined_features(net_img):
    """heatmap_mvfex_forward_api hands feat_refined to its caller: it keeps the materialising path whatever the field says, and what
    it returns is what the pose forward's heat maps were computed from."""
    from egorear_amd import hip
    net, img = net_img
    outs = {}
    for on in (True, False):
        hip.PROFILE = []
        try:
            with torch.no_grad(), hip.use_policy(hip.POLICY.replace(up2_on_load=on)):
                hms, feats = net.heatmap_estimator(img)
            torch.cuda.synchronize()
            names = [e[0] for e in hip.PROFILE]
        finally:
            hip.PROFILE = None
        outs[on] = ([h.clone() for h in hms], [f.clone() for f in feats], names)
    assert outs[True][2] == outs[False][2]
    for a, b in zip(outs[True][0] + outs[True][1], outs[False][0] + outs[False][1]):
        assert torch.equal(a, b)
    _, h_on, _ = _forward(hip, net, img, True)
    assert torch.equal(h_on[1], outs[False][0][1])        # refined heat maps: computed from the operand the lifting conv wrote out

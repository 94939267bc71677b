"""Soft-argmax decoding on the GPU (egr_soft_argmax_f32 / egr_soft_argmax_bwd_f32 / egr_coord_l1_f32, egorear_amd/decode.py, the
coordinate loss of train.HeatmapTrainer) against a float64 statement of the two reference functions written here.

The yardstick of every comparison with float64: the HIP result may deviate from the float64 statement (evaluated on the same fp32
inputs) by at most 8 x the deviation of torch's own fp32 CPU evaluation of that statement on those inputs - computed in the test, per
case, and printed next to the HIP figure.  The margin covers the hardware exp and a different, but fixed, summation order."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 8.0

# (rows, H, W): the product shape 2*2*15 maps on the register path; fewer elements than one wave pass and rows % 4 != 0; W not a
# power of two; H*W % 4 != 0 (unaligned maps, scalar path); above 4096 elements (two-read path)
SHAPES = [(60, 64, 64), (5, 8, 12), (1, 64, 48), (7, 7, 9), (3, 96, 96)]
CASES = [(mode, beta, normalize) for mode in (0, 1) for beta in (1.0, 100.0) for normalize in (False, True)]


# --------------------------------------------------------------------------- the statement

def statement(h, beta, mode, normalize):
    """What get_max_preds_soft_pytorch (beta 1, mode 0) and integrate_tensor_2d (beta = multiplier, mode 0 softmax / 1 relu) compute,
    for maps h (rows, H, W) in h's own dtype: coordinates (rows, 2) = (x, y), the weights (rows, H, W), the maxima (rows,)."""
    rows, H, W = h.shape
    z = (h * beta).reshape(rows, H * W)
    w = (torch.softmax(z, dim=1) if mode == 0 else torch.relu(z)).reshape(rows, H, W)
    x = (w.sum(dim=1) * torch.arange(W, dtype=h.dtype)).sum(dim=1)
    y = (w.sum(dim=2) * torch.arange(H, dtype=h.dtype)).sum(dim=1)
    if mode == 1:
        mass = w.sum(dim=(1, 2))
        x, y = x / mass, y / mass
    if normalize:
        x, y = x / W, y / H
    return torch.stack((x, y), dim=1), w, h.reshape(rows, -1).max(dim=1)[0]


def bumps(rows, H, W, seed):
    """A unit Gaussian bump at a random sub-pixel centre plus 0.05 Gaussian noise."""
    g = torch.Generator().manual_seed(seed)
    cx = torch.rand(rows, 1, 1, generator=g, dtype=torch.float64) * (W - 1)
    cy = torch.rand(rows, 1, 1, generator=g, dtype=torch.float64) * (H - 1)
    xs, ys = torch.arange(W, dtype=torch.float64).view(1, 1, W), torch.arange(H, dtype=torch.float64).view(1, H, 1)
    sigma = max(1.0, min(H, W) / 16.0)
    h = torch.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2 * sigma * sigma)) + 0.05 * torch.randn(rows, H, W, generator=g, dtype=torch.float64)
    return h.float().contiguous()


_CACHE = {}


def case_data(shape):
    """Inputs and the CPU references of one shape, computed once and shared by the tests (never modified)."""
    if shape not in _CACHE:
        rows, H, W = shape
        h = bumps(rows, H, W, seed=1000 + rows)
        g = torch.Generator().manual_seed(7 + rows)
        gc, gm = torch.randn(rows, 2, generator=g), torch.randn(rows, generator=g)
        ref = {}
        for mode, beta, normalize in CASES:
            out = {}
            for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
                hh = h.clone().to(dt).requires_grad_()
                c, w, m = statement(hh, beta, mode, normalize)
                (gh,) = torch.autograd.grad([c, m], [hh], [gc.to(dt), gm.to(dt)])
                out[name] = (c.detach(), w.detach(), gh)
            ref[(mode, beta, normalize)] = out
        _CACHE[shape] = (h, gc, gm, ref)
    return _CACHE[shape]


def dev64(a, b):
    return float((a.double().cpu() - b.double()).abs().max())


# --------------------------------------------------------------------------- forward

@pytest.mark.parametrize("shape", SHAPES)
def test_forward_against_the_float64_statement(shape):
    from egorear_amd import hip
    h, _, _, ref = case_data(shape)
    hd = h.to(DEV)
    ratios = []
    for mode, beta, normalize in CASES:
        c64, w64, _ = ref[(mode, beta, normalize)]["f64"]
        c32, w32, _ = ref[(mode, beta, normalize)]["f32"]
        coords, maxvals, index, valid, stat, probs = hip.soft_argmax(hd, beta, mode, normalize, 0.0, want_probs=True)
        torch.cuda.synchronize()
        own, got = dev64(c32, c64), dev64(coords, c64)
        p_own, p_got = dev64(w32, w64), dev64(probs, w64)
        print(f"{shape} mode {mode} beta {beta:g} normalize {normalize}: coords |hip - f64| {got:.3e}, |torch fp32 - f64| {own:.3e}, "
              f"ratio {got / own if own else float('inf'):.2f}; weights {p_got:.3e} vs {p_own:.3e}")
        ratios.append(((mode, beta, normalize), got, own, p_got, p_own))
        if mode == 0:      # the weights are a distribution: they sum to 1 as closely as torch's own fp32 softmax does
            s_own = float((w32.double().sum(dim=(1, 2)) - 1).abs().max())
            s_got = float((probs.double().sum(dim=(1, 2)) - 1).abs().max())
            print(f"    sum of weights - 1: hip {s_got:.3e}, torch fp32 {s_own:.3e}")
            ratios[-1] += (s_got, s_own)
    for r in ratios:
        assert r[1] <= MARGIN * r[2], ("coords", shape) + r
        assert r[3] <= MARGIN * r[4], ("weights", shape) + r
        if len(r) > 5:
            assert r[5] <= MARGIN * r[6], ("sum of weights", shape) + r


@pytest.mark.parametrize("shape", SHAPES)
def test_hard_decode_outputs_are_exact(shape):
    from egorear_amd import hip
    h, _, _, _ = case_data(shape)
    rows, H, W = shape
    hd = h.to(DEV)
    mx, ix = h.reshape(rows, -1).max(dim=1)                        # torch returns the first maximum
    thr = float(mx.median())
    for mode, beta in ((0, 100.0), (1, 1.0)):
        for want_probs in (False, True):
            _, maxvals, index, valid, stat, _ = hip.soft_argmax(hd, beta, mode, False, thr, want_probs=want_probs)
            assert torch.equal(maxvals.cpu(), mx) and torch.equal(index.cpu().long(), ix)
            assert torch.equal(valid.cpu().bool(), mx >= thr) and 0 < int(valid.sum()) <= rows
            assert torch.equal(stat[:, 0].cpu(), mx * beta)           # the max of z, not of h
            if (H * W) % 4 == 0:                                      # egr_argmax_rows_f32 takes these shapes only
                _, a_max, a_valid, a_idx = hip.argmax_rows(hd, thr)
                assert torch.equal(maxvals, a_max) and torch.equal(index, a_idx) and torch.equal(valid, a_valid)


def test_edge_rows_against_hand_derived_values():
    from egorear_amd import decode, hip
    for H, W in ((64, 64), (8, 12), (7, 9), (96, 96)):
        flat = torch.full((3, H, W), 0.25, device=DEV)             # beta * 0.25 is exact: every weight is exactly 1
        for mode, beta in ((0, 1.0), (0, 100.0), (1, 100.0)):
            coords, maxvals, index, _, _, _ = hip.soft_argmax(flat, beta, mode)
            assert torch.equal(coords.cpu(), torch.tensor([[(W - 1) / 2, (H - 1) / 2]] * 3)), (H, W, mode, beta, coords)
            assert torch.equal(index.cpu(), torch.zeros(3, dtype=torch.int32)) and float(maxvals.min()) == 0.25
    # the maximum twice, in two different lanes' elements: the first is the index; coordinates from the closed form
    for (H, W), (i0, i1) in (((64, 64), (5, 700)), ((7, 9), (3, 40))):
        m = torch.zeros(2, H, W)
        m.view(2, -1)[1, [i0, i1]] = 2.0
        coords, maxvals, index, _, _, _ = hip.soft_argmax(m.to(DEV), 1.0, 0)
        assert int(index[1]) == i0 and float(maxvals[1]) == 2.0 and int(index[0]) == 0
        import math
        e = math.exp(-2.0)
        den = H * W * e + 2 * (1 - e)
        x = (e * H * W * (W - 1) / 2 + (1 - e) * (i0 % W + i1 % W)) / den
        y = (e * H * W * (H - 1) / 2 + (1 - e) * (i0 // W + i1 // W)) / den
        assert abs(float(coords[1, 0]) - x) < 1e-4 and abs(float(coords[1, 1]) - y) < 1e-4, (coords[1], x, y)
    # a map peaking at 50 under beta 100: z reaches 5000, nothing overflows, the decode is the peak's pixel
    for H, W, at in ((64, 64, 64 * 41 + 13), (7, 9, 9 * 4 + 7), (96, 96, 96 * 95 + 1)):
        m = torch.zeros(1, 1, H, W)
        m.view(-1)[at] = 50.0
        hm = m.to(DEV).requires_grad_()
        coords, probs = decode.integrate_tensor_2d(hm)
        assert torch.equal(coords.detach().cpu().view(-1), torch.tensor([float(at % W), float(at // W)]))
        assert bool(torch.isfinite(probs).all()) and float(probs.sum()) == 1.0 and float(probs.view(-1)[at]) == 1.0
        (g,) = torch.autograd.grad(coords.sum(), hm)
        assert bool(torch.isfinite(g).all())
    # mode 1 without positive mass: NaN coordinates like the reference's 0 / 0, a zero gradient (the documented deviation)
    for H, W in ((64, 64), (7, 9)):
        hm = (-torch.rand(2, 1, H, W) - 0.1)
        hm[1, 0, 2, 3] = 0.5                                         # the second map has mass: its results are ordinary
        hm = hm.to(DEV).requires_grad_()
        coords, _ = decode.integrate_tensor_2d(hm, softmax=False)
        assert bool(torch.isnan(coords[0]).all()) and torch.equal(coords[1].detach().cpu().view(-1), torch.tensor([3.0, 2.0]))
        (g,) = torch.autograd.grad(coords, hm, torch.ones_like(coords))
        assert float(g[0].abs().max()) == 0.0 and bool(torch.isfinite(g).all())


# --------------------------------------------------------------------------- backward

@pytest.mark.parametrize("shape", SHAPES)
def test_backward_against_float64_autograd(shape):
    from egorear_amd import decode
    h, gc, gm, ref = case_data(shape)
    res = []
    for mode, beta, normalize in CASES:
        g64, g32 = ref[(mode, beta, normalize)]["f64"][2], ref[(mode, beta, normalize)]["f32"][2]
        hd = h.to(DEV).requires_grad_()
        coords, maxvals, _, _, _, _ = decode.soft_argmax_op(hd, beta, mode, normalize, 0.0, False)
        (g,) = torch.autograd.grad([coords, maxvals], [hd], [gc.to(DEV), gm.to(DEV)])
        torch.cuda.synchronize()
        own, got = dev64(g32, g64), dev64(g, g64)
        print(f"{shape} mode {mode} beta {beta:g} normalize {normalize}: g_hm |hip - f64| {got:.3e}, |torch fp32 - f64| {own:.3e}, "
              f"ratio {got / own if own else float('inf'):.2f}, largest entry {float(g64.abs().max()):.3g}")
        res.append(((mode, beta, normalize), got, own))
    for r in res:
        assert r[1] <= MARGIN * r[2], (shape,) + r


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_accumulates_and_repeats_bit_for_bit(shape):
    from egorear_amd import hip
    h, gc, gm, _ = case_data(shape)
    hd, gcd, gmd = h.to(DEV), gc.to(DEV), gm.to(DEV)
    for mode in (0, 1):
        coords, _, index, _, stat, _ = hip.soft_argmax(hd, 100.0, mode)
        g = hip.soft_argmax_bwd(hd, stat, coords, index, gcd, gmd, 100.0, mode)
        again = hip.soft_argmax_bwd(hd, stat, coords, index, gcd, gmd, 100.0, mode)
        coords2, _, _, _, stat2, _ = hip.soft_argmax(hd, 100.0, mode)
        assert torch.equal(g, again) and torch.equal(coords, coords2) and torch.equal(stat, stat2)
        prior = torch.randn(h.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
        buf = prior.clone()
        assert hip.soft_argmax_bwd(hd, stat, coords, index, gcd, gmd, 100.0, mode, out=buf, accumulate=True) is buf
        assert torch.equal(buf, g + prior)
        no_max = hip.soft_argmax_bwd(hd, stat, coords, index, gcd, None, 100.0, mode)       # g_maxvals lands on the arg-max alone
        d = (g - no_max).reshape(shape[0], -1)
        assert int((d != 0).sum()) <= shape[0] and torch.allclose(d.gather(1, index.long().view(-1, 1)).view(-1), gmd, atol=1e-5)


# --------------------------------------------------------------------------- placement and replay

def test_a_map_decodes_to_the_same_bits_alone_and_inside_the_batch():
    from egorear_amd import hip
    h, gc, gm, _ = case_data(SHAPES[0])
    hd, gcd, gmd = h.to(DEV), gc.to(DEV), gm.to(DEV)
    for mode, beta in ((0, 100.0), (0, 1.0), (1, 100.0)):
        full = hip.soft_argmax(hd, beta, mode, want_probs=True)
        one = hip.soft_argmax(hd[17:18], beta, mode, want_probs=True)
        for a, b in zip(full, one):
            assert torch.equal(a[17:18], b)
        g_full = hip.soft_argmax_bwd(hd, full[4], full[0], full[2], gcd, gmd, beta, mode)
        g_one = hip.soft_argmax_bwd(hd[17:18], one[4], one[0], one[2], gcd[17:18].contiguous(), gmd[17:18].contiguous(), beta, mode)
        assert torch.equal(g_full[17:18], g_one)


def test_graph_replay_gives_the_eager_bits():
    from egorear_amd import hip
    h, gc, gm, _ = case_data(SHAPES[0])
    hd, gcd, gmd = h.to(DEV), gc.to(DEV), gm.to(DEV)
    eager = hip.soft_argmax(hd, 100.0, 0, want_probs=True)
    g_eager = hip.soft_argmax_bwd(hd, eager[4], eager[0], eager[2], gcd, gmd, 100.0, 0)
    torch.cuda.synchronize()
    static = hd.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                    # one stream, no parallel branches
        out = hip.soft_argmax(static, 100.0, 0, want_probs=True)
        g = hip.soft_argmax_bwd(static, out[4], out[0], out[2], gcd, gmd, 100.0, 0)
    static.copy_(torch.zeros_like(hd))
    graph.replay()
    static.copy_(hd)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(a, b)
    assert torch.equal(g_eager, g)


def test_public_functions_return_the_reference_shapes():
    from egorear_amd import decode, hip
    h, _, _, ref = case_data(SHAPES[0])
    hm = h.view(2, 2, 15, 64, 64).to(DEV)
    out = decode.decode_joints_2d(hm, beta=100.0, threshold=0.5)
    _, a_max, a_valid, a_idx = hip.argmax_rows(hm, 0.5)
    assert out.soft.shape == out.hard.shape == (2, 2, 15, 2) and torch.equal(out.maxvals.view(-1), a_max)
    assert torch.equal(out.valid.view(-1), a_valid.bool())
    assert torch.equal(out.hard.view(-1, 2)[:, 0].long(), a_idx.long() % 64) and torch.equal(out.hard.view(-1, 2)[:, 1].long(), a_idx.long() // 64)
    assert float((out.soft - out.hard).abs().max()) < 4.0        # a sharp softmax sits next to the arg-max (0.05 noise is 5 in z)
    preds, maxvals = decode.get_max_preds_soft(hm.view(4, 15, 64, 64), normalize=True)
    assert preds.shape == (4, 15, 2) and maxvals.shape == (4, 15, 1)
    c64 = ref[(0, 1.0, True)]["f64"][0]
    assert dev64(preds.view(-1, 2), c64) <= MARGIN * dev64(ref[(0, 1.0, True)]["f32"][0], c64)
    coords, w = decode.integrate_tensor_2d(hm.view(4, 15, 64, 64).requires_grad_())
    assert coords.shape == (4, 15, 2) and w.shape == (4, 15, 64, 64) and coords.requires_grad and not w.requires_grad
    assert torch.equal(coords.detach().view(-1, 2), out.soft.view(-1, 2))


def test_coordinate_l1_loss_and_seed():
    from egorear_amd import hip
    g = torch.Generator().manual_seed(5)
    for rows, W in ((60, 64), (3, 9), (700, 64)):                    # fewer maps than threads; more than one pass of the workgroup
        coords = (torch.rand(rows, 2, generator=g) * W).float()
        index = torch.randint(0, W * W, (rows,), generator=g, dtype=torch.int32)
        valid = (torch.rand(rows, generator=g) < 0.7).to(torch.uint8)
        coords[0] = torch.tensor([float(index[0] % W), 5.25])        # an exact hit: sign(0) = 0
        valid[0] = 1
        loss = torch.full((1,), 7.0, dtype=torch.float64, device=DEV)
        gc = hip.coord_l1(coords.to(DEV), index.to(DEV), valid.to(DEV), W, 0.3, loss)
        tgt = torch.stack((index % W, index // W), 1).double()
        d = coords.double() - tgt
        n = max(int(valid.sum()), 1)
        w = float(torch.tensor(0.3, dtype=torch.float32))
        want = w / n * float((d.abs().sum(1) * valid).sum())
        assert abs(float(loss) - want) <= 1e-12 * max(want, 1.0), (float(loss), want)
        want_g = (torch.sign(d) * valid.view(-1, 1) * (w / n)).float()
        assert torch.equal(gc.cpu(), want_g)
    none = torch.zeros(4, dtype=torch.uint8, device=DEV)             # no valid map: loss 0, no division by zero
    loss = torch.ones(1, dtype=torch.float64, device=DEV)
    gc = hip.coord_l1(torch.rand(4, 2, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV), none, 8, 1.0, loss)
    assert float(loss) == 0.0 and float(gc.abs().max()) == 0.0


def test_bad_launches_are_refused():
    from egorear_amd import hip
    hm = torch.zeros(2, 8, 8, device=DEV)
    for beta, mode in ((0.0, 0), (-1.0, 0), (float("inf"), 0), (float("nan"), 1), (1.0, 2)):
        with pytest.raises(hip.LaunchError) as e:
            hip.soft_argmax(hm, beta, mode)
        assert e.value.code == hip.EINVAL


# --------------------------------------------------------------------------- the trainer's coordinate loss

W_COORD, BETA, THR = 0.1, 100.0, 1.0


def _heatmap_net():
    from egorear_amd import configs, synth
    from egorear_amd.estimator import EgoPoseFormerHeatmap
    net = EgoPoseFormerHeatmap(**copy.deepcopy(configs.heatmap_cfg()))
    synth.load_synth(net, 42)
    return net.to(DEV)


def _heatmap_data(seed, B=2):
    from egorear_amd import synth
    from egorear_amd.metrics import generate_target
    return synth.synth_images(B, 2, seed=seed).to(DEV), generate_target(synth.synth_joint_px(B, seed=40 + seed).to(DEV)).contiguous()


def _coord_loss(hm, gt, beta=BETA, thr=THR):
    """The trainer's coordinate term, as a drop-in user writes it: torch autograd through decode.integrate_tensor_2d."""
    from egorear_amd import decode
    B, V, J, H, W = hm.shape
    g = gt[:, :V].reshape(B * V, J, H * W)
    mx, ix = g.max(dim=2)
    valid = (mx >= thr).to(hm.dtype)
    tgt = torch.stack((ix % W, torch.div(ix, W, rounding_mode="floor")), -1).to(hm.dtype)
    coords = decode.integrate_tensor_2d(hm.reshape(B * V, J, H, W), multiplier=beta)[0]
    return ((coords - tgt).abs().sum(-1) * valid).sum() / valid.sum().clamp(min=1)


@pytest.fixture(scope="module")
def first_step():
    """The first update of HeatmapTrainer(w_coord=0.1) on fixed data: loss terms, heat maps and gradients, shared by the tests below."""
    from egorear_amd import train
    tr = train.HeatmapTrainer(_heatmap_net(), w_coord=W_COORD, coord_beta=BETA, coord_threshold=THR)
    img, gt = _heatmap_data(0)
    terms, hm = tr.step(img, gt)
    torch.cuda.synchronize()
    return {"terms": terms.clone(), "hm": hm.detach().clone(), "grads": {k: v.clone() for k, v in tr.opt.gviews.items()}, "img": img, "gt": gt,
            "w_heatmap": tr.w_heatmap}


def test_trainer_default_is_bit_identical_to_no_coordinate_loss():
    from egorear_amd import train
    a, b = train.HeatmapTrainer(_heatmap_net()), train.HeatmapTrainer(_heatmap_net(), w_coord=0.0)
    for t in range(2):
        ta, _ = a.step(*_heatmap_data(t))
        tb, _ = b.step(*_heatmap_data(t))
        assert ta.shape == tb.shape == (1,)
        assert abs(float(ta) - float(tb)) <= 1e-12 * float(ta)       # (the MSE term is a sum by double atomics: order-dependent last bits)
    torch.cuda.synchronize()
    assert torch.equal(a.opt.flat_p, b.opt.flat_p) and torch.equal(a.opt.flat_g, b.opt.flat_g)


def test_trainer_gradients_agree_with_the_drop_in_autograd_flow(first_step):
    net = _heatmap_net()
    net.train()
    hm = net(first_step["img"])
    V = hm.shape[1]
    mse = first_step["w_heatmap"] * V * torch.nn.functional.mse_loss(hm, first_step["gt"][:, :V])
    (mse + W_COORD * _coord_loss(hm, first_step["gt"])).backward()
    torch.cuda.synchronize()
    assert first_step["terms"].shape == (2,)
    checked = 0
    for k, p in net.named_parameters():
        g = first_step["grads"][k]
        if p.grad is None:
            assert float(g.abs().max()) == 0.0, k
            continue
        frac = float(((p.grad - g).abs() > 2e-4).float().mean())
        assert frac < 0.02, (k, frac, float((p.grad - g).abs().max()))
        checked += 1
    assert checked > 20
    # and the coordinate term is in them: the MSE term alone gives other gradients
    other = _heatmap_net()
    other.train()
    h2 = other(first_step["img"])
    (first_step["w_heatmap"] * V * torch.nn.functional.mse_loss(h2, first_step["gt"][:, :V])).backward()
    moved = max(float((p.grad - first_step["grads"][k]).abs().max()) for k, p in other.named_parameters() if p.grad is not None)
    print(f"largest gradient entry the coordinate term moved: {moved:.3e}")
    assert moved > 2e-3


def test_trainer_coordinate_term_is_the_float64_statement(first_step):
    hm, gt, terms = first_step["hm"].cpu(), first_step["gt"].cpu(), first_step["terms"].cpu()
    B, V, J, H, W = hm.shape
    g = gt[:, :V].reshape(B * V * J, H * W)
    mx, ix = g.max(dim=1)
    valid = (mx >= THR).double()
    assert 0 < float(valid.sum())
    tgt = torch.stack((ix % W, ix // W), 1).double()
    maps = hm.reshape(B * V * J, H, W)
    c64 = statement(maps.double(), BETA, 0, False)[0]
    c32 = statement(maps, BETA, 0, False)[0]

    def loss(c):
        return float(((c.double() - tgt).abs().sum(1) * valid).sum() / valid.sum())
    want, own = W_COORD * loss(c64), abs(W_COORD * loss(c32) - W_COORD * loss(c64))
    got = abs(float(terms[1]) - want)
    print(f"coordinate term {float(terms[1]):.9g} vs float64 {want:.9g}: |hip - f64| {got:.3e}, |torch fp32 - f64| {own:.3e}")
    assert float(terms[1]) > 0 and got <= MARGIN * own


def test_graphed_trainer_follows_the_eager_one_with_the_coordinate_loss():
    from egorear_amd import train
    eager = train.HeatmapTrainer(_heatmap_net(), w_coord=W_COORD)
    graphed = train.HeatmapTrainer(_heatmap_net(), w_coord=W_COORD, use_graph=True)
    for t in range(4):
        args = _heatmap_data(t)
        le, _ = eager.step(*args)
        lg, _ = graphed.step(*args)
        torch.cuda.synchronize()
        assert le.shape == lg.shape == (2,)
        for a, b in zip(le.tolist(), lg.tolist()):
            assert abs(a - b) <= 1e-5 * abs(a), (t, le, lg)
    assert graphed.graph is not None, "capture was refused"
    for (k, p), (_, q) in zip(eager.net.named_parameters(), graphed.net.named_parameters()):
        assert float(((p - q).abs() > 2e-4).float().mean()) < 0.02, k


def test_trainer_accumulates_with_the_coordinate_loss():
    from egorear_amd import train
    tr = train.HeatmapTrainer(_heatmap_net(), w_coord=W_COORD, accumulate=2)
    one = train.HeatmapTrainer(_heatmap_net(), w_coord=W_COORD)
    t0, _ = tr.step(*_heatmap_data(0))
    g0 = tr.opt.flat_g.clone()
    r0, _ = one.step(*_heatmap_data(0))
    torch.cuda.synchronize()
    assert t0.shape == (2,) and tr.opt.steps == 0 and tr.pending_micro_steps() == 1
    for a, b in zip(t0.tolist(), r0.tolist()):                     # the terms are reported un-scaled, the seeds carry 1/2
        assert abs(a - b) <= 1e-5 * abs(b)
    n2, n1 = float(g0.double().norm()), float(one.opt.flat_g.double().norm())
    assert abs(2.0 * n2 - n1) <= 1e-4 * n1, (n2, n1)
    tr.step(*_heatmap_data(1))
    torch.cuda.synchronize()
    assert tr.opt.steps == 1 and tr.pending_micro_steps() == 0

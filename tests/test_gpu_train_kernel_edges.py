"""Training-step kernels (egr_train.hip, egr_msda_bwd.hip, egr_attn.hip) at the branches and layouts the per-op file
test_gpu_train_kernels.py never launches: entry points reached only through the assembled step (mse_loss, nhwc_to_planes, adamw_dev,
the per-head colsum, the padded row-norm loss), untested template instantiations (MSDA cf 64 / 256 and heads != 4, LayerNorm 64 / 512,
BatchNorm 256 / 1024), ragged / tiny slabs, non-square maps, the grid-stride tails behind the clamped reduction grids and the
accumulate paths.  Every reference is plain torch on the CPU in float64 (autograd through the textbook formulation, or explicit
indexing); every shape is the smallest that still reaches its branch.

The unmarked tests at the top run without a GPU: they check the hand-written references against an independent torch statement
(1e-12) and show, by perturbing the REFERENCE, that the chosen inputs tell a kernel's likely layout mistakes apart by more than 10x
the bound the GPU test applies."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
DEV = "cuda:0"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def relerr(got, ref):
    ref = ref.detach().double()
    return float((got.detach().double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)


def close(got, ref, rel=2e-5, what=""):
    ref = ref.detach().double()
    tol = rel * max(float(ref.abs().max()), 1e-6)
    err = float((got.double().cpu() - ref).abs().max())
    assert err <= tol, f"{what} max err {err:.3e} > tol {tol:.3e}"


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# =========================================================================== references (float64, CPU)

def msda_sample_ref(value, H, W, loc, attn):
    """Single-level deformable sampling by explicit indexing.  value (N, H*W, nh, D); loc (N, Lq, nh, P, 2) normalised (x, y);
    attn (N, Lq, nh, P) -> (N, Lq, nh*D).  pixel = loc * size - 0.5; a point counts iff -1 < h, w and h < H, w < W; each of its four
    corners counts iff it lies inside the map (zero padding)."""
    N, _, nh, D = value.shape
    Lq = loc.shape[1]
    w_im, h_im = loc[..., 0] * W - 0.5, loc[..., 1] * H - 0.5
    inside = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
    h0, w0 = torch.floor(h_im), torch.floor(w_im)
    lh, lw = h_im - h0, w_im - w0
    h0, w0 = h0.long(), w0.long()
    ni = torch.arange(N).view(N, 1, 1, 1)
    hi = torch.arange(nh).view(1, 1, nh, 1)
    out = 0
    for dy in (0, 1):
        for dx in (0, 1):
            y, x = h0 + dy, w0 + dx
            ok = inside & (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
            wgt = (lh if dy else 1 - lh) * (lw if dx else 1 - lw) * ok.to(value.dtype) * attn
            rows = value[ni, y.clamp(0, H - 1) * W + x.clamp(0, W - 1), hi]          # (N, Lq, nh, P, D)
            out = out + (wgt[..., None] * rows).sum(3)
    return out.reshape(N, Lq, nh * D)


MSDA_BWD_SHAPES = [(64, 2, 32), (128, 4, 16), (256, 8, 32), (128, 1, 64)]       # (cf, heads, dh)


@functools.lru_cache(maxsize=None)
def msda_case(cf, heads, dh, H, W, groups, with_pos, B=1, V=2, J=3):
    """Inputs of one gather launch (float32, never modified): a corner anchor, a far-corner anchor whose x and y differ, offsets of
    several pixels so that some samples leave the map, and one invalid (b, v, j)."""
    C = heads * dh
    feat = rnd(V, B, H * W, cf, seed=1)
    pos = rnd(groups, V, H * W, C, seed=2) if with_pos else None
    ol = rnd(groups * B * J, heads * 48, seed=3)
    ol[:, :heads * 32] *= 6.0
    anchors = rnd(B, V, J, 2, seed=4) * 0.5 + 0.5
    anchors[0, 0, 0] = torch.tensor([0.0, 0.0])
    anchors[B - 1, V - 1, J - 1] = torch.tensor([(W - 0.5) / W, (H - 0.5) / H])      # centre of the last pixel: x != y
    valid = torch.ones(B, V, J, dtype=torch.uint8)
    valid[0, 1, 1] = 0
    Wfold = rnd(groups, C, cf, seed=5, scale=1 / math.sqrt(cf))
    cfold = rnd(groups, C, seed=6)
    da = rnd(groups, B * J * V, C, seed=7)
    return dict(B=B, V=V, J=J, heads=heads, dh=dh, cf=cf, C=C, H=H, W=W, groups=groups, feat=feat, pos=pos, ol=ol, anchors=anchors,
                valid=valid, Wfold=Wfold, cfold=cfold, da=da)


def msda_dense(c, feat, pos, ol, swap_hw=False):
    """Project every token, then sample (the dense statement the sample-then-project kernels replace).  feat / pos / ol: float64
    (leaves of the caller's graph).  -> (groups, rows (b, j, v), C); rows of an invalid (b, v, j) are zero.
    swap_hw: the offsets normalised by [H, W] instead of [W, H] - the perturbation of the sensitivity test."""
    B, V, J, heads, dh, H, W, groups = (c[k] for k in ("B", "V", "J", "heads", "dh", "H", "W", "groups"))
    size = torch.tensor([H, W] if swap_hw else [W, H], dtype=torch.float64)
    outs = []
    for g in range(groups):
        o_g = ol[g * B * J:(g + 1) * B * J]
        off = o_g[:, :heads * 32].reshape(B, J, heads, 16, 2)
        aw = o_g[:, heads * 32:].reshape(B, J, heads, 16).softmax(-1)
        per_view = []
        for v in range(V):
            value = feat[v] @ c["Wfold"][g].double().t() + c["cfold"][g].double()
            if pos is not None:
                value = value + pos[g, v]
            loc = c["anchors"][:, v].double()[:, :, None, None, :] + off / size
            a = msda_sample_ref(value.reshape(B, H * W, heads, dh), H, W, loc, aw)
            per_view.append(a * c["valid"][:, v, :, None].double())
        outs.append(torch.stack(per_view, dim=2).reshape(B * J * V, c["C"]))
    return torch.stack(outs)


def msda_grads(c, swap_hw=False):
    feat = c["feat"].double().requires_grad_(True)
    pos = c["pos"].double().requires_grad_(True) if c["pos"] is not None else None
    ol = c["ol"].double().requires_grad_(True)
    out = msda_dense(c, feat, pos, ol, swap_hw)
    wanted = (ol, feat) + ((pos,) if pos is not None else ())
    return out.detach(), torch.autograd.grad(out, wanted, c["da"].double())


def row_index(rows, d, inner, ld):
    """Flat offsets of the d floats of row r in a padded buffer: (r // inner) * ld + (r % inner) * d + [0, d)."""
    r = torch.arange(rows)
    return ((r // inner) * ld + (r % inner) * d)[:, None] + torch.arange(d)[None]


def rownorm_ref(pred, gt, rows, d, inner, ld_pred, ld_gt, weight):
    """weight * mean_rows ||gt_r - pred_r||_2 over rows gathered from padded buffers by explicit offsets (pred: float64, may require
    grad: autograd then leaves zeros in the padding, and torch's norm gives a zero-length row a zero subgradient)."""
    p = pred.reshape(-1)[row_index(rows, d, inner, ld_pred)]
    g = gt.double().reshape(-1)[row_index(rows, d, inner, ld_gt)]
    return weight * torch.linalg.norm(g - p, dim=-1, ord=2).sum() / rows


def mse_ref(pred, gt, weight):
    return weight * ((pred.double() - gt.double()) ** 2).sum() / pred.numel()


def colsum_ref(x, ld, rows, c, scale, groups, gx, gs, cps, sstride, head_shift=0):
    """out[g, ch] = sum_r scale[g*gs + (ch // cps)*sstride + r] * x[g*gx + r*ld + ch] by explicit flat indexing.
    head_shift: take the scale vector of another head (sensitivity test)."""
    xf, sf = x.double().reshape(-1), scale.double().reshape(-1)
    nvec = (c + cps - 1) // cps
    g, r, ch = torch.arange(groups)[:, None, None], torch.arange(rows)[None, :, None], torch.arange(c)[None, None, :]
    vec = (ch // cps + head_shift) % nvec
    return (sf[g * gs + vec * sstride + r] * xf[g * gx + r * ld + ch]).sum(1)


def plane_index(n, c, hw, nmap, base=0, image_shift=0):
    """Flat offsets (n, c, hw) of image img's (c, hw) planes: base + (img % n_inner)*stride_inner + (img // n_inner)*stride_outer."""
    n_inner, s_in, s_out = nmap
    img = (torch.arange(n) + image_shift) % n
    start = base + (img % n_inner) * s_in + (img // n_inner) * s_out
    return start[:, None, None] + torch.arange(c)[None, :, None] * hw + torch.arange(hw)[None, None, :]


def planes_ref(x, numel, c, nmap, base=0, sentinel=-7.0, image_shift=0):
    """x (n, hw, cpad) channels-last -> its first c channels as planes inside a flat buffer pre-filled with the sentinel."""
    n, hw, _ = x.shape
    out = torch.full((numel,), sentinel, dtype=x.dtype)
    out[plane_index(n, c, hw, nmap, base, image_shift)] = x[:, :, :c].permute(0, 2, 1)
    return out


# the three NMap forms of the training step, scaled down: (name, n, hw, c, cpad, nmap, base, numel)
def _plane_cases():
    B, V, J, hw = 3, 2, 5, 6
    return [
        # view-major (image n = v*B + b) into a (B, V, J + 1, hw) tensor: the last plane of every (b, v) is not addressed
        ("view_major", V * B, hw, J, 8, (B, V * (J + 1) * hw, (J + 1) * hw), 0, B * V * (J + 1) * hw),
        # zero outer stride, c < cpad (tokens <- the joints-as-channels image), from an offset into a larger buffer
        ("zero_outer", 4, 16, 3, 8, (4, 3 * 16, 0), 4, 4 + 4 * 3 * 16 + 5),
        # hw = 1 (vectors), view-major with one unaddressed float behind every image
        ("hw1", V * B, 1, 10, 12, (B, V * 11, 11), 0, B * V * 11),
    ]


PLANE_CASES = _plane_cases()


def mha_ref(qkv, dout, B, J, heads, d, dtype):
    """d qkv of softmax(q k^T / sqrt(d)) v with a max-subtracted softmax, in `dtype`; also returns the largest |logit|."""
    C = heads * d
    t = qkv.to(dtype).requires_grad_(True)
    q, k, v = (t[:, i * C:(i + 1) * C].reshape(B, J, heads, d).permute(0, 2, 1, 3) for i in range(3))
    s = (q @ k.transpose(-2, -1)) * torch.tensor(d ** -0.5, dtype=dtype)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    out = ((e / e.sum(-1, keepdim=True)) @ v).permute(0, 2, 1, 3).reshape(B * J, C)
    g, = torch.autograd.grad(out, t, dout.to(dtype))
    return g, float(s.detach().abs().max())


# =========================================================================== CPU tier: the references themselves

def test_reference_losses_match_torch_statements():
    B, J = 5, 15
    for pred, gt, inner, ldp, ldg in ((rnd(B, 64, seed=1), rnd(B, 45, seed=2), J, 64, 45), (rnd(B * J, 4, seed=3), rnd(B * J, 3, seed=4), 1, 4, 3)):
        mine = rownorm_ref(pred.double(), gt, B * J, 3, inner, ldp, ldg, 10.0)
        rows_p = pred.double()[:, :45].reshape(B * J, 3) if inner == J else pred.double()[:, :3]
        stated = 10.0 * ((gt.double().reshape(B * J, 3) - rows_p) ** 2).sum(-1).sqrt().mean()     # rows by slicing, the norm spelled out
        assert abs(float(mine - stated)) <= 1e-12 * abs(float(stated))
    p, g = rnd(257, 4, seed=5), rnd(257, 4, seed=6)
    stated = 3.5 * F.mse_loss(p.double(), g.double())
    assert abs(float(mse_ref(p, g, 3.5) - stated)) <= 1e-12 * abs(float(stated))


def test_reference_colsum_matches_einsum():
    G, rows, heads, dh = 2, 37, 4, 64
    C = heads * dh
    da, sig = rnd(G, rows, C, seed=1), rnd(G, heads, rows, seed=2)
    mine = colsum_ref(da, C, rows, C, sig, G, rows * C, heads * rows, dh, rows)
    stated = torch.einsum("ghr,grhd->ghd", sig.double(), da.double().view(G, rows, heads, dh)).reshape(G, C)
    assert relerr(mine, stated) <= 1e-12
    x, sc = rnd(21, 48, seed=3), rnd(4, 21, seed=4)                        # c = 40 of ld = 48, 10 columns per scale vector
    mine = colsum_ref(x, 48, 21, 40, sc, 1, 0, 0, 10, 21)
    stated = torch.einsum("vr,rvk->vk", sc.double(), x.double()[:, :40].reshape(21, 4, 10)).reshape(1, 40)
    assert relerr(mine, stated) <= 1e-12


def test_reference_plane_layouts_match_permute():
    B, V, J, hw = 3, 2, 5, 6
    _, n, _, c, cpad, nmap, base, numel = PLANE_CASES[0]
    x = rnd(n, hw, cpad, seed=1)
    mine = planes_ref(x, numel, c, nmap, base).view(B, V, J + 1, hw)
    assert torch.equal(mine[:, :, :J], x.view(V, B, hw, cpad)[..., :J].permute(1, 0, 3, 2))
    assert bool((mine[:, :, J] == -7.0).all())
    _, n, hw, c, cpad, nmap, base, numel = PLANE_CASES[1]
    x = rnd(n, hw, cpad, seed=2)
    mine = planes_ref(x, numel, c, nmap, base)
    assert torch.equal(mine[base:base + n * c * hw].view(n, c, hw), x[..., :c].transpose(1, 2))
    assert bool((mine[:base] == -7.0).all()) and bool((mine[base + n * c * hw:] == -7.0).all())
    _, n, hw, c, cpad, nmap, base, numel = PLANE_CASES[2]
    x = rnd(n, hw, cpad, seed=3)
    mine = planes_ref(x, numel, c, nmap, base).view(B, V, 11)
    assert torch.equal(mine[..., :10], x.view(V, B, cpad)[..., :10].permute(1, 0, 2)) and bool((mine[..., 10] == -7.0).all())


def test_reference_msda_on_a_non_square_map():
    from oracle.egorear_oracle import msda_core
    H, W, nh, D = 8, 16, 2, 3
    value = rnd(1, H * W, nh, D, seed=1).double()
    # one hand-placed sample for head 1: pixel (x, y) = (10.25, 5.75) -> corners x 10 / 11, y 5 / 6, weights by hand
    loc = torch.zeros(1, 1, nh, 1, 2, dtype=torch.float64)
    loc[0, 0, :, 0] = torch.tensor([(10.25 + 0.5) / W, (5.75 + 0.5) / H])
    attn = torch.ones(1, 1, nh, 1, dtype=torch.float64)
    got = msda_sample_ref(value, H, W, loc, attn).view(nh, D)
    v = value[0].view(H, W, nh, D)
    hand = 0.25 * 0.75 * v[5, 10] + 0.25 * 0.25 * v[5, 11] + 0.75 * 0.75 * v[6, 10] + 0.75 * 0.25 * v[6, 11]
    assert float((got - hand).abs().max()) <= 1e-12
    # a point half a pixel outside the right edge keeps its two left corners only; one beyond -1 contributes nothing
    loc[0, 0, :, 0] = torch.tensor([(15.5 + 0.5) / W, (2.0 + 0.5) / H])
    got = msda_sample_ref(value, H, W, loc, attn).view(nh, D)
    assert float((got - 0.5 * v[2, 15]).abs().max()) <= 1e-12
    loc[0, 0, :, 0] = torch.tensor([(-1.0 + 0.5) / W, (2.0 + 0.5) / H])
    assert float(msda_sample_ref(value, H, W, loc, attn).abs().max()) == 0.0
    # and the whole dense statement against the oracle's sampling core on the inputs of the GPU test
    for H, W in ((8, 16), (16, 8)):
        c = msda_case(128, 4, 32, H, W, 1, True)
        mine = msda_dense(c, c["feat"].double(), c["pos"].double(), c["ol"].double())
        B, V, J, heads = c["B"], c["V"], c["J"], c["heads"]
        off = c["ol"].double()[:, :heads * 32].reshape(B, J, heads, 16, 2)
        aw = c["ol"].double()[:, heads * 32:].reshape(B, J, heads, 16).softmax(-1)
        per_view = []
        for vw in range(V):
            val = c["feat"][vw].double() @ c["Wfold"][0].double().t() + c["cfold"][0].double() + c["pos"][0, vw].double()
            loc = c["anchors"][:, vw].double()[:, :, None, None, :] + off / torch.tensor([W, H], dtype=torch.float64)
            per_view.append(msda_core(val.reshape(B, H * W, heads, -1), H, W, loc, aw) * c["valid"][:, vw, :, None].double())
        stated = torch.stack(per_view, dim=2).reshape(1, B * J * V, -1)
        assert relerr(mine, stated) <= 1e-12


# --------------------------------------------------------------------------- CPU tier: can the inputs tell the mistakes apart?
# Each test perturbs the REFERENCE the way a kernel would most likely be wrong and requires the result to move by more than 10x the
# bound the GPU test applies.  The measured margins (relative to max |ref|, as `close` measures) are written beside each assert.

def test_sensitivity_swapped_height_and_width():
    for H, W in ((8, 16), (16, 8)):
        c = msda_case(128, 4, 32, H, W, 1, True)
        out, _ = msda_grads(c)
        out_s, _ = msda_grads(c, swap_hw=True)
        assert relerr(out_s, out) > 10 * 3e-5              # forward, bound 3e-5: measured 0.56 (8 x 16), 0.59 (16 x 8)
    for cf, heads, dh in MSDA_BWD_SHAPES:
        c = msda_case(cf, heads, dh, 8, 16, 2, True)
        _, grads = msda_grads(c)
        _, grads_s = msda_grads(c, swap_hw=True)
        for a, b in zip(grads_s, grads):
            assert relerr(a, b) > 10 * 5e-5                # d offsets/logits, d feat, d pos, bound 5e-5: measured 0.88 .. 2.4


def test_sensitivity_row_strides_of_the_padded_loss():
    B, J = 5, 15
    for pred, gt, inner, ldp, ldg in ((rnd(B, 64, seed=1), rnd(B, 45, seed=2), J, 64, 45), (rnd(B * J, 4, seed=3), rnd(B * J, 3, seed=4), 1, 4, 3)):
        pr = pred.double().requires_grad_(True)
        loss = rownorm_ref(pr, gt, B * J, 3, inner, ldp, ldg, 10.0)
        g, = torch.autograd.grad(loss, pr)
        ps = torch.cat([pred.double().reshape(-1), torch.zeros(64, dtype=torch.float64)]).requires_grad_(True)   # (room for the wrong stride)
        loss_s = rownorm_ref(ps, torch.cat([gt.reshape(-1), torch.zeros(64)]), B * J, 3, inner, ldg, ldg, 10.0)  # ld_gt where ld_pred belongs
        g_s, = torch.autograd.grad(loss_s, ps)
        assert abs(float(loss_s.detach() - loss.detach())) > 10 * 1e-5 * abs(float(loss.detach()))      # bound 1e-5: measured 0.088 (B x 64), 0.063 (B*J x 4)
        assert relerr(g_s[:pred.numel()], g.reshape(-1)) > 10 * 1e-5         # bound 1e-5: measured 1.4, 1.7


def test_sensitivity_scale_vector_of_the_neighbouring_head():
    G, rows, heads, dh = 2, 37, 4, 64
    C = heads * dh
    da, sig = rnd(G, rows, C, seed=1), rnd(G, heads, rows, seed=2)
    ref = colsum_ref(da, C, rows, C, sig, G, rows * C, heads * rows, dh, rows)
    assert relerr(colsum_ref(da, C, rows, C, sig, G, rows * C, heads * rows, dh, rows, head_shift=1), ref) > 10 * 1e-5   # measured 1.3
    x, sc = rnd(21, 48, seed=3), rnd(4, 21, seed=4)
    ref = colsum_ref(x, 48, 21, 40, sc, 1, 0, 0, 10, 21)
    assert relerr(colsum_ref(x, 48, 21, 40, sc, 1, 0, 0, 10, 21, head_shift=1), ref) > 10 * 1e-5                          # measured 1.5
    # a scale vector chosen per 16-lane group instead of per 10 columns: columns 10..15 and 20..31 would take the wrong one
    wrong = colsum_ref(x, 48, 21, 40, sc, 1, 0, 0, 16, 21)
    assert relerr(wrong, ref) > 10 * 1e-5                                                                                 # measured 1.5


def test_sensitivity_plane_shifted_by_one_image():
    for i, (_, n, hw, c, cpad, nmap, base, numel) in enumerate(PLANE_CASES):
        x = rnd(n, hw, cpad, seed=10 + i)
        ref, shifted = planes_ref(x, numel, c, nmap, base), planes_ref(x, numel, c, nmap, base, image_shift=1)
        addressed = ref != -7.0
        # the GPU test demands equality (tolerance 0): every addressed float differs (measured: 90 / 90, 192 / 192, 60 / 60)
        assert int((ref != shifted).sum()) == int(addressed.sum()) == n * c * hw


# =========================================================================== GPU tier

@gpu
@pytest.mark.parametrize("with_pos", [True, False])
@pytest.mark.parametrize("dh", [32, 64])
@pytest.mark.parametrize("H,W", [(8, 16), (16, 8)])
def test_msda_gather_forward_non_square(H, W, dh, with_pos):
    """egr_msda_gather_f32 on a map with hgt != wid: a_h = Wfold_h g_h + cfold_h sigma_h + e_h (assembled in float64 from the kernel's
    g, e, sigma) against the dense statement.  3e-5 is the bound test_gpu_kernels.py applies to the same comparison.  dh = 64 with the
    positional table takes the quarter-wave reads, dh = 32 one corner per instruction."""
    from egorear_amd import hip
    c = msda_case(128, 4, dh, H, W, 1, with_pos)
    B, V, J, heads, dh, cf, C = (c[k] for k in ("B", "V", "J", "heads", "dh", "cf", "C"))
    ref = msda_dense(c, c["feat"].double(), c["pos"].double() if with_pos else None, c["ol"].double())
    g, e, sigma, rowmask = hip.msda_gather(c["feat"].to(DEV), c["pos"].to(DEV) if with_pos else None, c["ol"].to(DEV), c["anchors"].to(DEV),
                                           c["valid"].to(DEV), B, V, J, heads, dh, H, W)
    rows = B * J * V
    assert torch.equal(rowmask.cpu().view(B, J, V), c["valid"].permute(0, 2, 1))
    a = torch.einsum("rhc,hdc->rhd", g[0].double().cpu(), c["Wfold"][0].double().view(heads, dh, cf))
    a = a + sigma[0].double().cpu().t()[:, :, None] * c["cfold"][0].double().view(1, heads, dh)
    if with_pos:
        a = a + e[0].double().cpu().view(rows, heads, dh)
    m = c["valid"].permute(0, 2, 1).reshape(rows, 1).double()
    close(a.reshape(rows, C) * m, ref[0], rel=3e-5)


@gpu
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("with_pos", [True, False])
@pytest.mark.parametrize("cf,heads,dh", MSDA_BWD_SHAPES)
def test_msda_gather_backward_non_square(cf, heads, dh, with_pos, groups):
    """egr_msda_gather_bwd_f32 on an 8 x 16 map: the cf 64 / 256 instantiations, heads 1 / 2 (a block of fewer than four waves) and
    heads 8 (two heads per wave), against autograd through the dense statement."""
    from egorear_amd import hip_train as T
    H, W = 8, 16
    c = msda_case(cf, heads, dh, H, W, groups, with_pos)
    B, V, J, C = c["B"], c["V"], c["J"], c["C"]
    _, grads = msda_grads(c)
    da_m = c["da"].double() * c["valid"].permute(0, 2, 1).reshape(1, B * J * V, 1).double()      # masked rows carry no gradient
    dg = torch.einsum("grhd,ghdc->grhc", da_m.reshape(groups, -1, heads, dh), c["Wfold"].double().reshape(groups, heads, dh, cf)).float()
    dfeat = T.zeros(c["feat"].shape, DEV)
    dpos = T.zeros(c["pos"].shape, DEV) if with_pos else None
    dol = T.msda_gather_bwd(c["feat"].to(DEV), c["pos"].to(DEV) if with_pos else None, c["ol"].to(DEV), c["anchors"].to(DEV),
                            c["valid"].to(DEV), B, V, J, heads, dh, H, W, dg.contiguous().to(DEV),
                            da_m.float().reshape(-1, C).contiguous().to(DEV), c["cfold"].to(DEV), dfeat, dpos, groups)
    close(T.fold_rows(dol, V), grads[0], rel=5e-5, what="d offsets/logits")
    close(dfeat, grads[1], rel=5e-5, what="d feat")
    if with_pos:
        close(dpos, grads[2], rel=5e-5, what="d pos")


@gpu
@pytest.mark.parametrize("c,groups,rpg", [(64, 3, 5), (512, 1, 7)])
def test_layernorm_narrowest_and_widest(c, groups, rpg):
    from egorear_amd import hip, hip_train as T
    rows = groups * rpg
    x, res = rnd(rows, c, seed=1), rnd(rows, c, seed=2)
    gamma, beta = rnd(groups, c, seed=3) + 1.2, rnd(groups, c, seed=4)
    dy = rnd(rows, c, seed=5)
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    pre = xr + res.double()
    y = torch.cat([F.layer_norm(pre[g * rpg:(g + 1) * rpg], (c,), gr[g], br[g], 1e-5) for g in range(groups)])
    dx_ref, dg_ref, db_ref = torch.autograd.grad(y, (xr, gr, br), dy.double())
    pre_d = T.add(x.to(DEV), res.to(DEV))
    ds, dgam, dbet = T.layernorm_bwd(dy.to(DEV), pre_d, gamma.reshape(-1).to(DEV), groups)
    close(ds, dx_ref, rel=2e-5, what="ds")
    close(dgam.view(groups, c), dg_ref, rel=2e-5, what="dgamma")
    close(dbet.view(groups, c), db_ref, rel=2e-5, what="dbeta")
    yk = hip.layernorm(x.to(DEV), gamma.reshape(-1).to(DEV), beta.reshape(-1).to(DEV), res=res.to(DEV), groups=groups)   # accepts 64 and 512
    close(yk, y.detach(), rel=2e-5, what="y")


def _ptr(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


@gpu
def test_layernorm_backward_refuses_other_widths():
    from egorear_amd import hip, hip_train as T
    rows, c = 8, 96
    dy, pre, gamma = rnd(rows, c, seed=1).to(DEV), rnd(rows, c, seed=2).to(DEV), rnd(c, seed=3).to(DEV)
    with pytest.raises(RuntimeError) as ei:
        T.layernorm_bwd(dy, pre, gamma)
    assert ei.value.code == -1                                   # EGR_EINVAL from the entry point, not a device error
    out = torch.zeros(rows * c + 2 * c + 2 * rows, device=DEV)
    p = [_ptr(t) for t in (dy, pre, gamma, out, out[rows * c:], out[rows * c + c:], out[rows * c + 2 * c:])]
    assert hip.lib.egr_layernorm_bwd_f32(*p, rows, c, 1e-5, 0, None) == -1
    assert float(out.abs().max()) == 0.0                         # nothing was launched


def _bn_inputs(c, groups, n, h, w):
    x = rnd(groups * n, c, h, w, seed=1) * 2 + 0.3
    res = rnd(groups * n, c, h, w, seed=2)
    gamma, beta = rnd(groups, c, seed=3) + 1.5, rnd(groups, c, seed=4)
    rm, rv = rnd(groups, c, seed=5), rnd(groups, c, seed=6) + 2
    dy = rnd(groups * n, c, h, w, seed=7)
    return x, res, gamma, beta, rm, rv, dy


BN_SHAPES = [(64, 2, 3, 7, 5),       # 105 rows per group in 3 slabs of 35 rows over 16 row lanes: ragged
             (256, 1, 2, 6, 6),      # 72 rows, 4 row lanes
             (1024, 2, 2, 3, 3),     # one row lane: no LDS reduction
             (64, 1, 1, 1, 5)]       # 5 rows for 16 row lanes


@gpu
@pytest.mark.parametrize("c,groups,n,h,w", BN_SHAPES)
def test_batchnorm_train_ragged_and_wide(c, groups, n, h, w):
    from egorear_amd import hip_train as T
    ws = T.bn_workspace(DEV)
    x, res, gamma, beta, rm, rv, dy = _bn_inputs(c, groups, n, h, w)
    # reference: each group is its own BatchNorm2d in training mode, followed by +res, ReLU
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rr = res.double().requires_grad_(True)
    rms, rvs, ys = [], [], []
    for g in range(groups):
        m, v = rm[g].double().clone(), rv[g].double().clone()
        ys.append(F.relu(F.batch_norm(xr[g * n:(g + 1) * n], m, v, gr[g], br[g], True, 0.1, 1e-5) + rr[g * n:(g + 1) * n]))
        rms.append(m)
        rvs.append(v)
    yref = torch.cat(ys)
    dx_ref, dg_ref, db_ref, dres_ref = torch.autograd.grad(yref, (xr, gr, br, rr), dy.double())
    rm_d, rv_d = rm.to(DEV).contiguous(), rv.to(DEV).contiguous()
    y, ctx = T.bn_train(nhwc(x).to(DEV), gamma.to(DEV), beta.to(DEV), rm_d, rv_d, groups, ws, res=nhwc(res).to(DEV), relu=True)
    close(y.permute(0, 3, 1, 2), yref, what="y")
    close(rm_d, torch.stack(rms), rel=1e-6, what="running_mean")
    close(rv_d, torch.stack(rvs), rel=1e-6, what="running_var")
    dx, dgam, dbet, dz = T.bn_backward(ctx, nhwc(dy).to(DEV), y, ws, want_dz=True)
    close(dx.permute(0, 3, 1, 2), dx_ref, rel=1e-4, what="dx")
    close(dgam, dg_ref, rel=1e-4, what="dgamma")
    close(dbet, db_ref, rel=1e-4, what="dbeta")
    close(dz.permute(0, 3, 1, 2), dres_ref, what="dres")
    # plain: no ReLU, no residual
    y2, ctx2 = T.bn_train(nhwc(x).to(DEV), gamma.to(DEV), beta.to(DEV), None, None, groups, ws, relu=False)
    y2ref = torch.cat([F.batch_norm(xr[g * n:(g + 1) * n], None, None, gr[g], br[g], True, 0.1, 1e-5) for g in range(groups)])
    close(y2.permute(0, 3, 1, 2), y2ref, what="y2")
    dx2_ref, dg2_ref, db2_ref = torch.autograd.grad(y2ref, (xr, gr, br), dy.double())
    dx2, dgam2, dbet2, _ = T.bn_backward(ctx2, nhwc(dy).to(DEV), None, ws)
    close(dx2.permute(0, 3, 1, 2), dx2_ref, rel=1e-4, what="dx2")
    close(dgam2, dg2_ref, rel=1e-4, what="dgamma2")
    close(dbet2, db2_ref, rel=1e-4, what="dbeta2")


@gpu
def test_batchnorm_records_on_ragged_slabs():
    """The abs-max records (egr_bn_stats_ex_f32 / egr_bn_backward_ex_f32) with slabs of unequal length: never below the true maximum,
    at most 4x (output) and 6x (gradient) above it, the conditions of test_batchnorm_records_are_upper_bounds_from_the_batch_extremes."""
    from egorear_amd import hip, hip_train as T
    c, groups, n, h, w = BN_SHAPES[0]
    ws = T.bn_workspace(DEV)
    x = (rnd(groups * n, h, w, c, seed=11) * 2 + 0.3).to(DEV)
    res = rnd(groups * n, h, w, c, seed=12).to(DEV)
    gamma, beta = (rnd(groups, c, seed=13) + 1.5).to(DEV), rnd(groups, c, seed=14).to(DEV)
    dy = rnd(groups * n, h, w, c, seed=17).to(DEV)
    arena = hip.AmaxArena(torch.device(DEV), records=8)
    arena.begin()
    hip.absmax_record(res, arena.new())
    rec_value = lambda rec: float(rec.cpu().view(torch.float32).max())      # noqa: E731
    for with_res in (True, False):
        rec = arena.new()
        y, ctx = T.bn_train(x, gamma, beta, None, None, groups, ws, res=res if with_res else None, relu=True, amax_out=rec)
        true = float(y.abs().max())
        print(f"bn record: res={with_res} max|y|={true:.4f} record={rec_value(rec):.4f}")
        assert y._egr_amax is rec and true <= rec_value(rec) <= 4.0 * true, (with_res, true, rec_value(rec))
        assert ctx.xhat_max is not None
        xh = ((x.view(groups, -1, c) - ctx.mean.view(groups, 1, c)) * ctx.invstd.view(groups, 1, c)).abs().amax(1)
        assert float((ctx.xhat_max / xh).min()) >= 1.0 - 1e-5 and float((ctx.xhat_max / xh).max()) <= 1.0 + 1e-4
        rdx = arena.new()
        dx, _, _, _ = T.bn_backward(ctx, dy, y, ws, want_dz=with_res, amax_dx=rdx)
        true = float(dx.abs().max())
        print(f"bn record: res={with_res} max|dx|={true:.4f} record={rec_value(rdx):.4f}")
        assert dx._egr_amax is rdx and true <= rec_value(rdx) <= 6.0 * true, (with_res, true, rec_value(rdx))


@gpu
@pytest.mark.parametrize("c", [32, 96])
def test_batchnorm_refuses_other_channel_counts(c):
    from egorear_amd import hip_train as T
    ws = T.bn_workspace(DEV)
    x = rnd(2, 3, 3, c, seed=1).to(DEV)
    gamma, beta = torch.ones(1, c, device=DEV), torch.zeros(1, c, device=DEV)
    with pytest.raises(RuntimeError) as ei:
        T.bn_train(x, gamma, beta, None, None, 1, ws)
    assert ei.value.code == -1                                   # EGR_EINVAL: refused before any launch


@functools.lru_cache(maxsize=None)
def _long_vectors(n):
    return rnd(n, seed=1), rnd(n, seed=2)


MSE_SIZES = [4, 1028, 2 * 2 ** 20 + 1028]     # one quad; one block and a bit; past the 2048-block clamp (the grid-stride loop runs twice)


@gpu
@pytest.mark.parametrize("want_grad", [True, False])
@pytest.mark.parametrize("n", MSE_SIZES)
def test_mse_loss(n, want_grad):
    """egr_mse_loss_f32: loss += weight * mean (pred - gt)^2 onto a non-zero scalar, dpred = 2 weight (pred - gt) / n.  Bounds 1e-6:
    the difference, its square's operand and coef = weight / n are one fp32 rounding (2^-24) each, the sum is in double."""
    from egorear_amd import hip_train as T
    pred, gt = _long_vectors(n)
    weight, start = 3.7, 0.75
    term = float(mse_ref(pred, gt, weight))
    loss = torch.full((1,), start, dtype=torch.float64, device=DEV)
    dp = T.mse_loss(pred.to(DEV), gt.to(DEV), weight, loss, want_grad=want_grad)
    got = float(loss)
    print(f"mse n={n}: loss {got!r} ref {start + term!r}")
    assert abs(got - (start + term)) <= 1e-6 * abs(term)
    if want_grad:
        close(dp, 2.0 * weight * (pred.double() - gt.double()) / n, rel=1e-6, what="dpred")
    else:
        assert dp is None


@gpu
def test_rownorm_loss_past_the_grid_clamp():
    """4099 rows: the grid stops at 1024 blocks of 4 rows, rows 4096.. go round the grid-stride loop; rows % 4 != 0."""
    from egorear_amd import hip_train as T
    d, rows = 3, 4099
    pred, gt = rnd(rows, d, seed=1), rnd(rows, d, seed=2)
    gt[4097] = pred[4097]                                  # zero norm (in the tail): a zero subgradient, as torch's norm backward
    gt[3] = pred[3]
    pr = pred.double().requires_grad_(True)
    loss_ref = torch.mean(torch.linalg.norm(gt.double() - pr, dim=-1, ord=2)) * 10.0
    g_ref, = torch.autograd.grad(loss_ref, pr)
    loss = torch.full((1,), 0.5, dtype=torch.float64, device=DEV)
    dp = T.rownorm_loss(pred.to(DEV), gt.to(DEV), d, 10.0, loss)
    assert abs(float(loss) - 0.5 - float(loss_ref.detach())) <= 1e-5 * abs(float(loss_ref.detach()))
    close(dp, g_ref, rel=1e-5)
    assert float(dp[4097].abs().max()) == 0.0 and float(dp[3].abs().max()) == 0.0


@gpu
@pytest.mark.parametrize("form", ["rows_of_B", "rows_of_BJ"])
def test_rownorm_loss_padded_layouts(form):
    """Both padded call forms of the pose loss: pred (B, 64) holding J x 3 floats per row against gt (B, J*3), and pred (B*J, 4)
    against gt (B*J, 3).  dpred has pred's layout: the used columns match autograd on the gathered rows, the padding is exactly 0."""
    from egorear_amd import hip_train as T
    B, J = 5, 15
    if form == "rows_of_B":
        pred, gt, inner, ldp, ldg = rnd(B, 64, seed=1), rnd(B, 45, seed=2), J, 64, 45
        pred[2, 6:9] = gt[2, 6:9]                          # one zero-norm row
    else:
        pred, gt, inner, ldp, ldg = rnd(B * J, 4, seed=3), rnd(B * J, 3, seed=4), 1, 4, 3
        pred[7, :3] = gt[7]
    pr = pred.double().requires_grad_(True)
    loss_ref = rownorm_ref(pr, gt, B * J, 3, inner, ldp, ldg, 10.0)
    g_ref, = torch.autograd.grad(loss_ref, pr)             # zero in the padding by construction
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    dp = T.rownorm_loss(pred.to(DEV), gt.to(DEV), 3, 10.0, loss, rows=B * J, inner=inner, ld_pred=ldp, ld_gt=ldg)
    assert abs(float(loss) - float(loss_ref.detach())) <= 1e-5 * abs(float(loss_ref.detach()))
    assert dp.shape == pred.shape
    close(dp, g_ref, rel=1e-5)
    used = torch.zeros(pred.numel(), dtype=torch.bool)
    used[row_index(B * J, 3, inner, ldp).reshape(-1)] = True
    pad = dp.cpu().reshape(-1)[~used]
    assert pad.numel() == pred.numel() - B * J * 3 and bool((pad == 0.0).all())


@gpu
def test_sumsq_past_the_grid_clamp_and_accumulating():
    """egr_sumsq_f32: n past the 2048-block clamp (1e-6: products and sum are in double), and accumulate=True twice onto one scalar."""
    from egorear_amd import hip_train as T
    g, g2 = _long_vectors(MSE_SIZES[-1])
    ref = float((g.double() ** 2).sum())
    out = torch.full((1,), 123.0, dtype=torch.float64, device=DEV)
    T.sumsq(g.to(DEV), out)                                # overwrites
    assert abs(float(out) - ref) <= 1e-6 * ref
    a, b = g[:4100] * 3, g2[:1028]
    acc = torch.full((1,), 0.5, dtype=torch.float64, device=DEV)
    T.sumsq(a.to(DEV), acc, accumulate=True)
    T.sumsq(b.to(DEV), acc, accumulate=True)
    ref2 = 0.5 + float((a.double() ** 2).sum()) + float((b.double() ** 2).sum())
    assert abs(float(acc) - ref2) <= 1e-6 * ref2


@gpu
@pytest.mark.parametrize("accumulate", [False, True])
def test_colsum_per_head_scale(accumulate):
    """egr_colsum_f32 with cols_per_scale / scale_stride / gs as the gather backward calls it (dcfold: one sigma vector per head), and
    with c = 40, 10 columns per scale vector: not a multiple of the 16 channel lanes, a scale block straddling a 16-lane group."""
    from egorear_amd import hip_train as T
    G, rows, heads, dh = 2, 37, 4, 64
    C = heads * dh
    da, sig = rnd(G, rows, C, seed=1), rnd(G, heads, rows, seed=2)
    out0 = rnd(G, C, seed=3)
    ref = colsum_ref(da, C, rows, C, sig, G, rows * C, heads * rows, dh, rows) + (out0.double() if accumulate else 0)
    got = T.colsum(da.to(DEV), C, rows, C, scale=sig.to(DEV), out=out0.clone().to(DEV) if accumulate else None, accumulate=accumulate,
                   groups=G, gx=rows * C, gs=heads * rows, cols_per_scale=dh, scale_stride=rows)
    close(got, ref, rel=1e-5, what="per-head")
    x, sc = rnd(21, 48, seed=3), rnd(4, 21, seed=4)
    out1 = rnd(1, 40, seed=5)
    ref = colsum_ref(x, 48, 21, 40, sc, 1, 0, 0, 10, 21) + (out1.double() if accumulate else 0)
    got = T.colsum(x.to(DEV), 48, 21, 40, scale=sc.to(DEV), out=out1.clone().to(DEV) if accumulate else None, accumulate=accumulate,
                   cols_per_scale=10, scale_stride=21)
    close(got, ref, rel=1e-5, what="c = 40")


@gpu
@pytest.mark.parametrize("case", PLANE_CASES, ids=[c[0] for c in PLANE_CASES])
def test_nhwc_to_planes_maps(case):
    """egr_nhwc_to_planes_f32 for the three NMap forms of the step: copies, so equality; what the map does not address keeps the
    sentinel; planes_to_nhwc of the result returns the first c channels with zero padding."""
    from egorear_amd import hip_train as T
    from egorear_amd.hip import NMap
    _, n, hw, c, cpad, nmap, base, numel = case
    x = rnd(n, hw, cpad, seed=21)
    planes = torch.full((numel,), -7.0, device=DEV)
    T.nhwc_to_planes(x.to(DEV), planes, NMap(*nmap), c, base_offset=base)
    assert torch.equal(planes.cpu(), planes_ref(x, numel, c, nmap, base))
    back = T.planes_to_nhwc(planes, NMap(*nmap), n, c, hw, cpad, base_offset=base).cpu()
    assert torch.equal(back[..., :c], x[..., :c]) and (c == cpad or float(back[..., c:].abs().max()) == 0.0)


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _hyper(lr, b1, b2, t):
    """What egr_adamw_f32 derives from (lr, beta1, beta2, step): the betas arrive as C floats, the bias corrections are computed in
    double from those and cast to float."""
    return torch.tensor([lr, 1.0 - _f32(b1) ** t, math.sqrt(1.0 - _f32(b2) ** t)], dtype=torch.float64).float()


@gpu
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("clipping", ["active", "inactive", "none"])
@pytest.mark.parametrize("n", [4, 4100])
def test_adamw_clip_situations(n, clipping, wd):
    """egr_adamw_f32 over one quad and over 17 blocks (the last one partial), two steps against torch.optim.AdamW with
    clip_grad_norm_: the clip coefficient below 1, at 1, and no gradient norm given at all.
    The parameters are held to torch's AdamW with betas (0.9, 0.999).  The moments are held to AdamW with the betas the entry point
    receives: they cross the C interface as floats, and float(0.999) = 0.999 + 1.3e-8 moves 1 - beta2, and with it every v, by 1.3e-5
    of its value (measured: v off by exactly that against the un-rounded betas; p is not affected, the bias correction is formed from
    the same rounded beta2)."""
    from egorear_amd import hip_train as T
    p0, g1, g2 = rnd(n, seed=1), rnd(n, seed=2) * 3, rnd(n, seed=3) * 0.01
    clip = {"active": 0.004, "inactive": 1e3, "none": 1.0}[clipping]
    ref, ref32 = torch.nn.Parameter(p0.clone()), torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=1e-3, weight_decay=wd)
    opt32 = torch.optim.AdamW([ref32], lr=1e-3, weight_decay=wd, betas=(_f32(0.9), _f32(0.999)))
    p, m, v = p0.clone().to(DEV), T.zeros((n,), DEV), T.zeros((n,), DEV)
    ss = torch.zeros(1, dtype=torch.float64, device=DEV)
    for step, g in enumerate((g1, g2), 1):
        for r, o in ((ref, opt), (ref32, opt32)):
            r.grad = g.clone()
            if clipping != "none":
                total = float(torch.nn.utils.clip_grad_norm_([r], clip))
                assert (total > clip) == (clipping == "active")
            o.step()
        gd = g.to(DEV)
        if clipping != "none":
            T.sumsq(gd, ss)
        T.adamw(p, gd, m, v, 1e-3, 0.9, 0.999, 1e-8, wd, step, ss if clipping != "none" else None, clip)
        close(p, ref.detach(), rel=2e-6, what=f"step {step}")
        close(p, ref32.detach(), rel=2e-6, what=f"step {step}, float betas")
        close(m, opt32.state[ref32]["exp_avg"], rel=2e-6, what=f"m, step {step}")
        # (own scale, not close()'s 1e-6 floor: clipped gradients leave v near 1e-9)
        v_ref = opt32.state[ref32]["exp_avg_sq"].double()
        assert float((v.double().cpu() - v_ref).abs().max()) <= 2e-6 * float(v_ref.abs().max()), f"v, step {step}"


@gpu
@pytest.mark.parametrize("n", [4, 4100])
def test_adamw_dev_equals_adamw(n):
    """egr_adamw_dev_f32 (the update of every graphed step) reads {lr, 1 - b1^t, sqrt(1 - b2^t)} from device memory: given the floats
    the host entry derives, the same kernel runs on the same values - p, m, v are bit-identical; both match torch.optim.AdamW.
    The Trainer writes the bias corrections from the un-rounded betas (a few ulp away): that form is held to torch's 2e-6 as well."""
    from egorear_amd import hip_train as T
    lr, b1, b2, eps, wd, clip = 1e-3, 0.9, 0.999, 1e-8, 5e-4, 0.004
    p0, g1, g2 = rnd(n, seed=1), rnd(n, seed=2) * 3, rnd(n, seed=3) * 0.01
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=lr, weight_decay=wd)
    sets = [[p0.clone().to(DEV), T.zeros((n,), DEV), T.zeros((n,), DEV)] for _ in range(3)]
    ss = torch.zeros(1, dtype=torch.float64, device=DEV)
    for step, g in enumerate((g1, g2), 1):
        ref.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([ref], clip)
        opt.step()
        gd = g.to(DEV)
        T.sumsq(gd, ss)
        T.adamw(sets[0][0], gd, sets[0][1], sets[0][2], lr, b1, b2, eps, wd, step, ss, clip)
        T.adamw_dev(sets[1][0], gd, sets[1][1], sets[1][2], _hyper(lr, b1, b2, step).to(DEV), b1, b2, eps, wd, ss, clip)
        trainer_form = torch.zeros(4, device=DEV)
        T.set4(trainer_form, lr, 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step))
        T.adamw_dev(sets[2][0], gd, sets[2][1], sets[2][2], trainer_form, b1, b2, eps, wd, ss, clip)
        for a, b, what in zip(sets[0], sets[1], "pmv"):
            assert torch.equal(a, b), f"{what} differs at step {step}"
        print(f"adamw_dev n={n} step {step}: bias corrections from un-rounded betas move {int((sets[2][0] != sets[0][0]).sum())} of {n} parameters")
        for s in sets:
            close(s[0], ref.detach(), rel=2e-6, what=f"step {step}")


@gpu
@pytest.mark.parametrize("J,heads,d", [(1, 1, 8), (7, 2, 24), (16, 1, 64)])
def test_joint_mha_backward_small_and_odd(J, heads, d):
    from egorear_amd import hip_train as T
    B, C = 2, heads * d
    qkv, dout = rnd(B * J, 3 * C, seed=1), rnd(B * J, C, seed=2)
    ref, _ = mha_ref(qkv, dout, B, J, heads, d, torch.float64)
    got = T.joint_mha_bwd(qkv.to(DEV), dout.to(DEV), B, J, heads, d, d ** -0.5)
    close(got, ref, rel=3e-5)


@gpu
def test_joint_mha_backward_large_logits():
    """q and k scaled so the largest logit passes 100: exp() of it overflows fp32 unless the row maximum is subtracted first.  fp32
    logit error grows with |logit|, so the bound is 4x what the same math in float32 on the CPU (max-subtracted softmax) loses
    against float64, floored at the 3e-5 of the other cases."""
    from egorear_amd import hip_train as T
    B, J, heads, d = 2, 16, 4, 64
    C = heads * d
    qkv, dout = rnd(B * J, 3 * C, seed=1), rnd(B * J, C, seed=2)
    qkv[:, :2 * C] *= 12.0
    ref, top = mha_ref(qkv, dout, B, J, heads, d, torch.float64)
    assert top > 100.0, top                                        # measured: largest |logit| 169.1
    f32, _ = mha_ref(qkv, dout, B, J, heads, d, torch.float32)
    cpu_err = relerr(f32, ref)                                     # measured: 4.7e-6 (4x = 1.9e-5) -> the floor applies, bound 3e-5
    bound = max(4.0 * cpu_err, 3e-5)
    got = T.joint_mha_bwd(qkv.to(DEV), dout.to(DEV), B, J, heads, d, d ** -0.5)
    assert bool(torch.isfinite(got).all())
    print(f"large logits: max |logit| {top:.1f}, float32 CPU error {cpu_err:.2e}, bound {bound:.2e}, kernel error {relerr(got, ref):.2e}")
    close(got, ref, rel=bound)


@gpu
@pytest.mark.parametrize("J,d", [(17, 64), (16, 65)])
def test_joint_mha_backward_refuses_what_does_not_fit(J, d):
    from egorear_amd import hip_train as T
    B, heads = 2, 1
    qkv, dout = rnd(B * J, 3 * heads * d, seed=1).to(DEV), rnd(B * J, heads * d, seed=2).to(DEV)
    with pytest.raises(RuntimeError) as ei:
        T.joint_mha_bwd(qkv, dout, B, J, heads, d, d ** -0.5)
    assert ei.value.code == -1                                     # EGR_EINVAL: the LDS tiles hold 16 tokens of 64 floats


@gpu
def test_gelu_in_saturation():
    from egorear_amd import hip_train as T
    z = torch.cat([torch.tensor([30.0, -30.0, 0.0, -0.0, 6.0, -6.0, 9.0, -9.0]), rnd(56, seed=3) * 4])
    dh = rnd(64, seed=4)
    zr = z.double().requires_grad_(True)
    h = F.gelu(zr)
    dz_ref, = torch.autograd.grad(h, zr, dh.double())
    hk, dzk = T.gelu(z.to(DEV)), T.gelu_bwd(dh.to(DEV), z.to(DEV))
    assert bool(torch.isfinite(hk).all()) and bool(torch.isfinite(dzk).all())
    # the random values and the saturated ones each against their own scale (30 in the maximum would hide an error of 6e-5 elsewhere)
    close(hk[8:], h.detach()[8:], rel=2e-6, what="gelu")
    close(dzk[8:], dz_ref[8:], rel=2e-6, what="gelu_bwd")
    close(hk[:8], h.detach()[:8], rel=2e-6, what="gelu, saturated")
    close(dzk[:8], dz_ref[:8], rel=2e-6, what="gelu_bwd, saturated")
    assert float(hk[1]) == 0.0 and float(hk[2]) == 0.0 and float(dzk[1]) == 0.0        # -30 -> -0 * ..., exactly nothing
    assert float(hk[0]) == 30.0 and float(dzk[0]) == float(dh[0])


@gpu
@pytest.mark.parametrize("k,s,p,h,w,c", [(2, 2, 1, 7, 5, 4), (5, 3, 2, 9, 11, 8), (3, 1, 1, 4, 4, 4)])
def test_maxpool_odd_geometries(k, s, p, h, w, c):
    """One channel quad, non-square odd sizes, padded 2 x 2 windows, 5 x 5 windows (slots up to 24), overlapping stride-1 windows;
    planted ties: the first maximum in scan order gets the gradient, as in torch."""
    from egorear_amd import hip, hip_train as T
    x = rnd(2, c, h, w, seed=1)
    x[:, :, ::3, ::2] = 0.25
    x[:, :, 1, 1] = 0.25
    xr = x.double().requires_grad_(True)
    y = F.max_pool2d(xr, k, s, p)
    dy = rnd(*y.shape, seed=2)
    dx_ref, = torch.autograd.grad(y, xr, dy.double())
    yi, slot = T.maxpool_train(hip.Img(nhwc(x).to(DEV)), k, s, p)
    close(yi.t.permute(0, 3, 1, 2), y.detach(), rel=1e-7)
    dx = T.maxpool_bwd(nhwc(dy).to(DEV), slot, (h, w), k, s, p)
    close(dx.permute(0, 3, 1, 2), dx_ref, rel=1e-6)

"""Float64 statement of the stem kernels (egr_stem.hip, egr_stem_x6.hip): the 7x7 / stride 2 / pad 3 convolution of selected views with
per-group filters, the optional BatchNorm(eval) scale / shift + ReLU, the optional MaxPool2d(3, 2, 1), and the weight gradient of the bare
convolution - each written out as sums over the 49 taps (strided slices of the padded image, one matrix product per group), not taken
from torch's convolution or autograd, which tests/test_stem_statement_host.py holds it against.  Plain torch on the CPU, computing in
float64 whatever it is given; no import of the HIP library.  Shared by test_stem_statement_host.py and test_gpu_stem_walk.py.

View selection, as hip.stem documents it: img is (B, V, 3, H, W); group g takes the views view0 + g*nviews ... view0 + (g+1)*nviews - 1
with its own filters w[g]; its output images are view-major, n = v*B + b, and the groups' outputs follow each other: image
g*nviews*B + v*B + b of the (groups*nviews*B, H/2, W/2, 64) NHWC result."""
import torch


def _views(img, view0, nviews, g):
    """(nviews*B, 3, H, W) float64: the images of group g, n = v*B + b."""
    B, V, C, H, W = img.shape
    v0 = view0 + g * nviews
    assert C == 3 and 0 <= v0 and v0 + nviews <= V
    return img[:, v0:v0 + nviews].permute(1, 0, 2, 3, 4).reshape(nviews * B, 3, H, W).double()


def _patches(x):
    """x (n, 3, H, W) -> (n, 147, H/2 * W/2): column k = ci*49 + kh*7 + kw of output pixel (oy, ox) is the zero-padded input at
    (ci, 2*oy + kh - 3, 2*ox + kw - 3)."""
    n, _, H, W = x.shape
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.zeros(n, 3, H + 6, W + 6, dtype=x.dtype)
    xp[:, :, 3:3 + H, 3:3 + W] = x
    taps = [xp[:, :, kh:kh + 2 * ho - 1:2, kw:kw + 2 * wo - 1:2] for kh in range(7) for kw in range(7)]
    return torch.stack(taps, 2).reshape(n, 147, ho * wo), ho, wo


def stem_conv(img, view0, nviews, w, groups, magnitude=False):
    """The bare convolution, NHWC (groups*nviews*B, H/2, W/2, 64) float64.  magnitude=True: the same sums over |img| and |w| - the sum of
    the magnitudes of every output's 147 terms, what a rounding-error bound of the sum is stated against."""
    assert tuple(w.shape) == (groups, 64, 3, 7, 7)
    out = []
    for g in range(groups):
        x, wg = _views(img, view0, nviews, g), w[g].double().reshape(64, 147)
        if magnitude:
            x, wg = x.abs(), wg.abs()
        cols, ho, wo = _patches(x)
        out.append(torch.matmul(cols.transpose(1, 2), wg.t()).reshape(-1, ho, wo, 64))
    return torch.cat(out, 0)


def maxpool_3_2_1(y):
    """MaxPool2d(3, 2, 1) of an NHWC tensor, as the largest of nine strided slices of the -inf padded tensor."""
    n, h, w, c = y.shape
    ph, pw = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    yp = torch.full((n, h + 2, w + 2, c), float("-inf"), dtype=y.dtype)
    yp[:, 1:1 + h, 1:1 + w] = y
    out = None
    for dy in range(3):
        for dx in range(3):
            s = yp[:, dy:dy + 2 * ph - 1:2, dx:dx + 2 * pw - 1:2]
            out = s.clone() if out is None else torch.maximum(out, s)
    return out


def stem_epilogue(conv, scale, shift, groups, pool):
    """What follows the convolution: relu(conv * scale[g] + shift[g]) per group when scale / shift (groups, 64) are given (both or
    neither), then the max-pool when asked for."""
    assert (scale is None) == (shift is None)
    y = conv
    if scale is not None:
        n = conv.shape[0] // groups
        sc = scale.double().reshape(groups, 1, 1, 1, 64)
        sh = shift.double().reshape(groups, 1, 1, 1, 64)
        y = torch.clamp_min(conv.reshape(groups, n, *conv.shape[1:]) * sc + sh, 0.0).reshape(conv.shape)
    return maxpool_3_2_1(y) if pool else y


def stem_ref(img, view0, nviews, w, scale, shift, groups, pool):
    """The stem in float64: NHWC (groups*nviews*B, H/2, W/2, 64), or (.., H/4, W/4, 64) with pool."""
    return stem_epilogue(stem_conv(img, view0, nviews, w, groups), scale, shift, groups, pool)


def mag_epilogue(mag, scale, shift, groups, pool):
    """The magnitude an error of stem_ref's output is judged against, from the convolution's (stem_conv(.., magnitude=True)):
    mag * |scale| + |shift| in eval mode (the scale multiplies the sum's error, the shift adds one rounding of its own size; ReLU does not
    increase a difference), and its max-pool for the pooled output (|max a - max b| <= max |a - b| over the window)."""
    m = mag
    if scale is not None:
        n = mag.shape[0] // groups
        m = (mag.reshape(groups, n, *mag.shape[1:]) * scale.double().abs().reshape(groups, 1, 1, 1, 64)
             + shift.double().abs().reshape(groups, 1, 1, 1, 64)).reshape(mag.shape)
    return maxpool_3_2_1(m) if pool else m


def stem_mag(img, view0, nviews, w, scale, shift, groups, pool):
    """stem_ref's companion: per output element the sum of the magnitudes of its terms (see mag_epilogue)."""
    return mag_epilogue(stem_conv(img, view0, nviews, w, groups, magnitude=True), scale, shift, groups, pool)


def stem_wgrad_ref(img, view0, nviews, dy, groups):
    """Weight gradient of the bare convolution: dy (groups*nviews*B, H/2, W/2, 64) NHWC -> (dw, mag), both (groups, 64, 3, 7, 7) float64:
    dw[g, co, ci, kh, kw] = sum over the group's images and output pixels of dy[n, oy, ox, co] * padded input(n, ci, 2*oy + kh - 3,
    2*ox + kw - 3), and mag the same sum over |dy| and |img|."""
    B = img.shape[0]
    n = nviews * B
    assert dy.shape[0] == groups * n and dy.shape[3] == 64
    dw, mag = [], []
    for g in range(groups):
        cols, ho, wo = _patches(_views(img, view0, nviews, g))
        d = dy[g * n:(g + 1) * n].double().reshape(n, ho * wo, 64)
        dw.append(torch.matmul(cols, d).sum(0).t().reshape(64, 3, 7, 7))
        mag.append(torch.matmul(cols.abs(), d.abs()).sum(0).t().reshape(64, 3, 7, 7))
    return torch.stack(dw), torch.stack(mag)


# ----------------------------------------------------------------------------------------------- the inputs of the stem tests

def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def stem_inputs(B, V, H, W, groups, seed):
    """float32 inputs with the dynamic range the fp16 scheme's per-tile pre-scale has to cope with (test_gpu_kernels.py's h2 case), spread so
    that consecutive tiles of a persistent workgroup's walk carry different pre-scales: every image has an amplitude of its own
    (0.05 * 3.7^k, k = 0..4 - not powers of two), one image starts with a black band of tile height, another holds a single outlier
    pixel 900 times its neighbours; two output channels of every group are scaled by 1e-4 and by 300.
    -> img (B, V, 3, H, W), w (groups, 64, 3, 7, 7), scale, shift (groups, 64)."""
    img = rnd(B, V, 3, H, W, seed=seed)
    amp = 0.05 * 3.7 ** ((torch.arange(B * V) * 3) % 5).double()
    img = (img * amp.float().view(B, V, 1, 1, 1)).contiguous()
    img[0, 0, :, :min(32, H), :] = 0.0
    img[-1, -1, 1, min(H - 1, H // 2 + 8), 17] = 900.0 * float(amp[-1])
    if B * V > 3:
        img[B // 2, (V - 1) // 2] = 0.0                              # a whole black image inside a walk
        img[B // 2, (V - 1) // 2, 2, H - 1, W - 1] = -3.0            # ... but for its last pixel
    w = rnd(groups, 64, 3, 7, 7, seed=seed + 1, scale=0.1)
    w[:, 5] *= 1e-4
    w[:, 9] *= 300.0
    scale = rnd(groups, 64, seed=seed + 2) * 0.3 + 1.0
    shift = rnd(groups, 64, seed=seed + 3) * 0.02                    # small beside the sums: ReLU and the max-pool see the image
    return img, w, scale, shift


def pack_w(w):
    """(groups, 64, 3, 7, 7) -> the (groups, 64, 148) rows the stem entry points take (k = ci*49 + kh*7 + kw, last column 0)."""
    wp = torch.zeros(w.shape[0], 64, 148)
    wp[:, :, :147] = w.reshape(w.shape[0], 64, 147)
    return wp


# The geometries of test_gpu_stem_walk.py, here so that test_stem_statement_host.py holds the reference to its condition on the same inputs.
# name: (B, V, H, W, groups, seed, view0, nviews)
WALK_CASES = {"main": (2, 64, 96, 192, 64, 564, 0, 1),          # 64 groups: 4 (x6 / h2) and 8 (fp32, weight gradient) workgroups per group
              "single": (2, 300, 32, 128, 300, 800, 0, 1)}      # 300 groups: one workgroup per group
EDGE_SHAPES = {   # per kernel family: a single tile, seams in rows only, seams in columns only (B = 2, two views, one group)
    "f32": {"one tile": (16, 64), "row seams": (32, 64), "column seams": (16, 128)},
    "x6": {"one tile": (32, 64), "row seams": (64, 64), "column seams": (32, 128)},
}


def edge_case(H, W):
    return (2, 2, H, W, 1, 600 + H + W, 0, 2)


VIEW_CASE = (2, 6, 64, 128, 2, 700, 1, 2)                       # first view skipped, group stride (2 views) unlike the view stride


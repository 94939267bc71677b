"""Multi-peak heat-map decoding on the GPU (egr_peaks_f32, egorear_amd/decode.py) against the float64 statement of
tests/robust_statement.py.  `index`, `count` and `score` rest on exact fp32 comparisons and copies: they must equal the statement's.
`coords` meet the yardstick of fisheye_statement.py: at most 8 x the deviation of torch's fp32 CPU evaluation of the statement from
its float64 evaluation - per case, printed - with a floor of 4 fp32 ulp of the largest coordinate."""
import pytest
import torch

import robust_statement as RS
from fisheye_statement import yardstick

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BETA, THR = 100.0, 0.5
# (B, V, J, H, W, K, nms_radius, refine_radius): the product's maps; a non-square map with the widest windows; one peak, no window;
# a map smaller than the windows whose 35 pixels are no multiple of 64 (nor of 4: the scalar-load path)
SHAPES = [(2, 4, 3, 64, 64, 3, 1, 2), (1, 2, 1, 16, 12, 4, 2, 3), (3, 3, 2, 32, 32, 1, 1, 0), (1, 1, 1, 5, 7, 4, 3, 3)]
CASES = ("bumps", "noise", "quantised", "constant", "below", "borders", "nonfinite")


def make_case(case, shape, g):
    """(N, H, W) float32 maps.  Noise stays within [0.6, 1.2): beta * (h - m) <= 60 wherever a window is wider than the suppression
    radius, so that torch's fp32 evaluation of exp - the yardstick - does not overflow."""
    B, V, J, H, W = shape[:5]
    N = B * V * J
    ys, xs = torch.arange(H, dtype=torch.float64).view(1, H, 1), torch.arange(W, dtype=torch.float64).view(1, 1, W)
    if case == "bumps":                  # a unit bump and a distractor of height 1.2 somewhere else, both off the pixel grid
        c = torch.rand(N, 2, 2, generator=g, dtype=torch.float64) * torch.tensor([W - 1.0, H - 1.0], dtype=torch.float64)
        hm = sum(a * torch.exp(-((xs - c[:, i, 0].view(N, 1, 1)) ** 2 + (ys - c[:, i, 1].view(N, 1, 1)) ** 2) / 2.0) for i, a in ((0, 1.0), (1, 1.2)))
    elif case == "noise":                # far more than K peaks
        hm = 0.6 + 0.6 * torch.rand(N, H, W, generator=g, dtype=torch.float64)
    elif case == "quantised":            # multiples of 1/8: exact ties and plateaus everywhere
        hm = 0.625 + torch.floor(torch.rand(N, H, W, generator=g, dtype=torch.float64) * 5) / 8
    elif case == "constant":
        hm = torch.full((N, H, W), 0.75, dtype=torch.float64)
    elif case == "below":
        hm = 0.5 * torch.rand(N, H, W, generator=g, dtype=torch.float64)            # rand < 1: every pixel < 0.5; one sits exactly on it
        hm[:, H // 2, W // 2] = 0.5                                                   # (h > threshold is strict)
    elif case == "borders":              # the four corners and the middles of the four borders; two pairs of equal heights
        hm = 0.3 * torch.rand(N, H, W, generator=g, dtype=torch.float64)
        spots = [(0, 0, 0.9), (0, W - 1, 0.95), (H - 1, 0, 0.9), (H - 1, W - 1, 1.0), (0, W // 2, 0.8), (H // 2, 0, 0.85), (H - 1, W // 2, 0.8),
                 (H // 2, W - 1, 0.7)]
        for y, x, a in spots:
            hm[:, y, x] = a
    else:                                # NaN, +inf and -inf sprinkled over the noise
        hm = 0.6 + 0.6 * torch.rand(N, H, W, generator=g, dtype=torch.float64)
        r = torch.rand(N, H, W, generator=g)
        hm[r < 0.04], hm[(r >= 0.04) & (r < 0.07)], hm[(r >= 0.07) & (r < 0.10)] = float("nan"), float("inf"), float("-inf")
    return hm.float().contiguous()


_CACHE = {}


def shape_data(shape):
    """Per case the maps and the statement in float64 and in float32, computed once."""
    if shape in _CACHE:
        return _CACHE[shape]
    K, rn, r = shape[5:]
    g = torch.Generator().manual_seed(sum(shape))
    out = {}
    for case in CASES:
        hm = make_case(case, shape, g)
        out[case] = (hm, RS.peaks_statement(hm.double(), K, rn, r, BETA, THR), RS.peaks_statement(hm, K, rn, r, BETA, THR))
    _CACHE[shape] = out
    return out


def launch(hm, shape):
    from egorear_amd import decode
    B, V, J, H, W, K, rn, r = shape
    p = decode.find_peaks_2d(hm.view(B, V, J, H, W).to(DEV), K, rn, r, BETA, THR)
    N = B * V * J
    return p.coords.view(N, K, 2), p.score.view(N, K), p.index.view(N, K), p.count.view(N)


@pytest.mark.parametrize("shape", SHAPES)
def test_peaks_against_the_float64_statement(shape):
    d = shape_data(shape)
    B, V, J, H, W, K, rn, r = shape
    bad = []
    for case in CASES:
        hm, f64, f32 = d[case]
        coords, score, index, count = launch(hm, shape)
        torch.cuda.synchronize()
        print(f"{shape} {case}: peaks kept per map {sorted(set(f64[3].tolist()))}")
        assert torch.equal(index.cpu(), f64[2]), (shape, case)
        assert torch.equal(count.cpu(), f64[3]), (shape, case)
        assert torch.equal(score.cpu().double(), f64[1]), (shape, case)                   # the peak's own value, copied
        assert torch.equal(f32[2], f64[2]) and torch.equal(f32[3], f64[3])                # (fp32 comparisons are exact in either)
        err, allowed = yardstick("coords", coords, f32[0], f64[0])
        if not err <= allowed:
            bad.append((shape, case, err, allowed))
        empty = (f64[2] < 0)
        assert float(coords.cpu()[empty].abs().sum()) == 0.0 and float(score.cpu()[empty].abs().sum()) == 0.0
        # what the cases are for
        if case == "noise" and H * W >= 64:
            assert int(f64[3].min()) == K
        if case == "quantised" and H * W >= 64:
            s = f64[1]
            assert bool((s[:, 0] == 1.125).any()) and (K == 1 or bool((s[:, 0] == s[:, 1]).any()))       # ties among the kept
        if case == "constant":
            assert index.cpu()[:, 0].tolist() == [0] * (B * V * J) and count.cpu().tolist() == [1] * (B * V * J)
        if case == "below":
            assert int(count.sum()) == 0 and bool((index == -1).all())
        if case == "borders":
            assert index.cpu()[:, 0].tolist() == [(H - 1) * W + W - 1] * (B * V * J)                         # the highest: a corner
            if K >= 4 and min(H, W) > 4 * rn:                                                               # 1.0, 0.95, then 0.9 twice
                assert index.cpu()[0].tolist() == [(H - 1) * W + W - 1, W - 1, 0, (H - 1) * W]              # ties: the smaller index first
        if case == "nonfinite":
            assert bool(torch.isfinite(coords).all()) and bool(torch.isfinite(score).all())
    assert not bad, bad


@pytest.mark.parametrize("shape", SHAPES)
def test_two_runs_agree_and_a_map_alone_gives_its_bits_in_the_batch(shape):
    d = shape_data(shape)
    B, V, J, H, W, K, rn, r = shape
    from egorear_amd import decode
    for case in ("quantised", "nonfinite", "bumps"):
        hm = d[case][0]
        first, again = launch(hm, shape), launch(hm, shape)
        for a, b in zip(first, again):
            assert torch.equal(a, b), (shape, case)
        N = B * V * J
        for n in sorted({0, N // 2, N - 1}):
            one = decode.find_peaks_2d(hm[n].view(1, 1, 1, H, W).to(DEV), K, rn, r, BETA, THR)
            for a, b in zip(first, one):
                assert torch.equal(a[n], b.view(a[n].shape)), (shape, case, n)
    torch.cuda.synchronize()


def test_the_entry_refuses_what_it_does_not_support():
    from egorear_amd import hip
    hm = torch.zeros(2, 8, 8, device=DEV)
    out = (torch.empty(2, 4, 2, device=DEV), torch.empty(2, 4, device=DEV), torch.empty(2, 4, dtype=torch.int32, device=DEV),
           torch.empty(2, dtype=torch.int32, device=DEV))
    ptrs = [t.data_ptr() for t in out]
    ok = dict(rows=2, hgt=8, wid=8, K=3, rn=1, r=2, beta=100.0, thr=0.5)
    for change in ({"K": 0}, {"K": 5}, {"rn": 0}, {"rn": 4}, {"r": -1}, {"r": 4}, {"beta": 0.0}, {"beta": float("inf")}, {"thr": float("nan")},
                   {"hgt": 64, "wid": 65}, {"hgt": 0}, {"rows": 0}):
        a = dict(ok, **change)
        rc = hip.lib.egr_peaks_f32(hm.data_ptr(), a["rows"], a["hgt"], a["wid"], a["K"], a["rn"], a["r"], a["beta"], a["thr"], *ptrs, None)
        assert rc == hip.EINVAL, (change, rc)
    assert hip.lib.egr_peaks_f32(None, 2, 8, 8, 3, 1, 2, 100.0, 0.5, *ptrs, None) == hip.ENULL

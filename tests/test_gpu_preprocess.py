"""Frame pre-processing at its edge shapes: every kernel of egr_preprocess.hip (LDS, aligned-dword and generic horizontal pass,
vertical pass, fused) against the numpy restatement of Pillow and against Pillow's own committed answers, bit for bit, with
egr_preprocess_last_kernel() saying which kernel ran.  No comparison here has a tolerance.

Kernels and the cases that reach them:
  LDS horizontal pass (0): five two-pass shapes, the pattern set at (36,40)->(48,64), placement offset 0, non-contiguous input, the
                           leading dimensions, every fused shape again in two passes, the fall-back of the one over the LDS limit;
  aligned-dword (1):       three two-pass shapes, the pattern set at (35,44)->(40,64), placement offset 4;
  generic (2):             three two-pass shapes, the pattern set at (33,47)->(24,20), placement offset 1, frames[1:] of an odd-sized batch;
  fused (3):               six fused shapes, the pattern set at (64,128)->(80,256);
  vertical pass:           every two-pass case above (ksize_v 5 .. 23).
"""
import numpy as np
import pytest
import torch

from oracle import preprocess_oracle as O
from oracle import preprocess_patterns as P

LDS, DWORD, GENERIC, FUSED = range(4)      # the codes of egr_preprocess_last_kernel() (hip.PRE_ROUTE_*)

# in_hw, out_hw, kernel of the horizontal pass, ksize_h, ksize_v
TWO_PASS = [
    ((36, 40), (48, 64), LDS, 5, 5),          # up-sampling both ways: 5 taps, windows clipped at both borders
    ((200, 64), (40, 320), LDS, 5, 21),       # ow > 256: a second trip of the kernel's column loop
    ((88, 72), (16, 24), LDS, 13, 23),        # the longest vertical window the launch accepts, ow < 64
    ((100, 24), (20, 8), LDS, 13, 21),        # ow = 8
    ((48, 64), (48, 64), LDS, 5, 5),          # equal sizes: Pillow's bicubic is the identity
    ((35, 44), (24, 20), DWORD, 11, 7),       # odd h
    ((35, 44), (40, 64), DWORD, 5, 5),        # up-sampling
    ((36, 45), (24, 20), DWORD, 11, 7),       # 135-byte row pitch: every row starts at another byte misalignment
    ((33, 47), (24, 20), GENERIC, 11, 7),     # odd total byte count
    ((64, 330), (16, 64), GENERIC, 23, 17),   # the longest horizontal window the launch accepts
    ((96, 100), (20, 24), GENERIC, 19, 21),
]
# in_hw, out_hw, inside the fused kernel's limits, ksize_h, ksize_v, rows of the largest band, LDS bytes of the launch
FUSED_CASES = [
    ((64, 128), (80, 256), True, 5, 5, None, None),           # up-sampling both ways, oh % 32 = 16
    ((60, 64), (100, 256), True, 5, 5, None, None),           # 4 bands, the last one of 4 rows
    ((100, 512), (40, 256), True, 9, 11, None, None),         # two bands
    ((44, 256), (30, 256), True, 5, 7, 44, None),             # one partial band, horizontal identity, h % 8 = 4
    ((500, 400), (100, 256), True, 9, 21, 175, 144064),       # close to the 153 600-byte LDS limit
    ((532, 400), (100, 256), True, 9, 23, 186, 152512),       # the last height under it, and the longest vertical window
    ((536, 400), (100, 256), False, 9, 23, 188, 154048),      # the first height over it: two passes (LDS kernel) by itself
]
# (560, 400) -> (100, 256) would be 196 rows and 160 192 bytes, but its vertical window has 25 taps: no launch takes it (refusals below)
assert tuple((i, o) for i, o, *_ in TWO_PASS) == P.TWO_PASS_SHAPES and tuple((i, o) for i, o, *_ in FUSED_CASES) == P.FUSED_SHAPES

_id = lambda v: "%dx%d" % v if isinstance(v, tuple) else None


def _f32(u8):
    """ToTensor + Normalize of (n, oh, ow, 3) uint8 images: what O.preprocess_frames makes of them."""
    return np.stack([O.to_tensor_normalize(f) for f in u8])


def _pre(in_hw, out_hw, fused=False):
    from egorear_amd.preprocess import FramePreprocessor
    pre = FramePreprocessor(in_hw=in_hw, out_hw=out_hw)
    pre.fused = fused
    return pre


def _route():
    from egorear_amd import hip
    return hip.lib.egr_preprocess_last_kernel()


def _park_route(away_from):
    """Leave another code in egr_preprocess_last_kernel() than the one the next launch must report: a stale value cannot pass."""
    if away_from == GENERIC:
        _pre((4, 4), (4, 4))(torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device="cuda"))
        assert _route() == LDS
    else:
        _pre((3, 3), (4, 4))(torch.zeros(1, 3, 3, 3, dtype=torch.uint8, device="cuda"))     # 27 bytes per frame: byte loads
        assert _route() == GENERIC


def _run(pre, frames, route):
    """Launch on a device tensor; (fp32, uint8) as numpy and the assertion that `route` ran."""
    _park_route(route)
    x, u8 = pre(frames, return_u8=True)
    assert _route() == route
    return x.cpu().numpy(), u8.cpu().numpy()


def _check(x, u8, ref_u8):
    assert x.dtype == np.float32 and x.shape == ref_u8.shape[:-3] + (3,) + ref_u8.shape[-3:-1]
    assert np.array_equal(u8, ref_u8)
    assert np.array_equal(x.reshape((-1,) + x.shape[-3:]), _f32(ref_u8.reshape((-1,) + ref_u8.shape[-3:])))


@pytest.fixture(scope="module")
def golden_edges(golden_dir):
    import os
    return np.load(os.path.join(golden_dir, "preprocess_pil_edges.npz"))


def _check_golden(golden, pattern, in_hw, out_hw, u8):
    for i in range(P.FRAMES):
        P.check_against_golden(golden, P.key(pattern, in_hw, out_hw, i), u8[i])


# ------------------------------------------------------------------ the fixture's own claims (host only)
def test_the_shape_tables_pin_what_they_say():
    """Window lengths, band rows and LDS bytes named in the tables are the ones the resampling tables give."""
    from egorear_amd import hip
    assert (hip.PRE_ROUTE_LDS, hip.PRE_ROUTE_DWORD, hip.PRE_ROUTE_GENERIC, hip.PRE_ROUTE_FUSED) == (LDS, DWORD, GENERIC, FUSED)
    for in_hw, out_hw, _, kh, kv in TWO_PASS:
        assert (O.precompute_coeffs(in_hw[1], out_hw[1])[2], O.precompute_coeffs(in_hw[0], out_hw[0])[2]) == (kh, kv), (in_hw, out_hw)
        assert kh <= 24 and kv <= 24 and out_hw[1] % 4 == 0
    assert max(c[3] for c in TWO_PASS) == 23 and max(c[4] for c in TWO_PASS) == 23        # the accepted maximum: ksize is odd
    # ksize is the row length of the weight table; a window holds at most ksize - 1 taps.  The longest ones that run, all non-zero:
    for (i, o), taps in (((88, 16), 22), ((330, 64), 21), ((532, 100), 22)):
        b, c, _ = O.precompute_coeffs(i, o)
        assert int(b[:, 1].max()) == taps and any(c[r, 0] != 0 and c[r, taps - 1] != 0 for r in np.where(b[:, 1] == taps)[0])
    for in_hw, out_hw, inside, kh, kv, rows, lds in FUSED_CASES:
        bv, _, kv2 = O.precompute_coeffs(in_hw[0], out_hw[0])
        assert (O.precompute_coeffs(in_hw[1], out_hw[1])[2], kv2) == (kh, kv), (in_hw, out_hw)
        band = max(int(bv[min(o + 32, out_hw[0]) - 1].sum() - bv[o, 0]) for o in range(0, out_hw[0], 32))
        need = ((8 * in_hw[1] * 3 + 64 + 15) & ~15) + band * out_hw[1] * 3
        assert rows in (None, band) and lds in (None, need)
        assert (need <= 150 * 1024) == inside and out_hw[1] == 256 and kh <= 16 and in_hw[0] % 4 == 0 and (in_hw[1] * 12) % 16 == 0
    u8 = P.oracle_u8("random", (33, 47), (24, 20))
    assert np.array_equal(_f32(u8), O.preprocess_frames(P.frames("random", (33, 47)), 24, 20))      # _f32 is preprocess_frames' tail


def _preclip(img, bounds, coeffs, axis):
    """(acc + 2^21) >> 22 of one pass before the clip, and the pass's (clipped) uint8 image."""
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    rows = []
    for o in range(bounds.shape[0]):
        lo, cnt = int(bounds[o, 0]), int(bounds[o, 1])
        k = coeffs[o, :cnt].astype(np.int64)
        rows.append(((src[lo:lo + cnt] * k[:, None, None]).sum(axis=0) + (1 << 21)) >> 22)
    pre = np.moveaxis(np.stack(rows), 0, axis)
    return pre, np.clip(pre, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("in_hw,out_hw", [((36, 40), (48, 64)), ((35, 44), (40, 64)), ((64, 128), (80, 256))], ids=_id)
def test_the_binary_pattern_reaches_both_clips_in_both_passes(in_hw, out_hw):
    """A condition on the fixture: at least 5 % of the accumulators of each pass fall below 0 and at least 5 % above 255, so a
    kernel that clipped once only, or rounded negative accumulators another way, cannot pass the binary case."""
    bh, ch, _ = O.precompute_coeffs(in_hw[1], out_hw[1])
    bv, cv, _ = O.precompute_coeffs(in_hw[0], out_hw[0])
    for f, ref in zip(P.frames("binary", in_hw), P.oracle_u8("binary", in_hw, out_hw)):
        ph, tmp = _preclip(f, bh, ch, 1)
        pv, out = _preclip(tmp, bv, cv, 0)
        assert np.array_equal(out, ref)                                     # the same arithmetic as the oracle's
        for p in (ph, pv):
            assert (p < 0).mean() >= 0.05 and (p > 255).mean() >= 0.05, ((p < 0).mean(), (p > 255).mean())


# ------------------------------------------------------------------ two passes
@pytest.mark.gpu
@pytest.mark.parametrize("in_hw,out_hw,route,kh,kv", TWO_PASS, ids=_id)
def test_two_pass_edge_shapes_equal_pillow(golden_edges, in_hw, out_hw, route, kh, kv):
    pre = _pre(in_hw, out_hw)
    assert (pre.kh, pre.kv) == (kh, kv)
    frames = P.frames("random", in_hw)
    x, u8 = _run(pre, torch.from_numpy(frames).cuda(), route)
    _check(x, u8, P.oracle_u8("random", in_hw, out_hw))
    _check_golden(golden_edges, "random", in_hw, out_hw, u8)
    if in_hw == out_hw:
        assert np.array_equal(u8, frames)                                   # a known answer that needs no oracle


# ------------------------------------------------------------------ one launch
@pytest.mark.gpu
@pytest.mark.parametrize("in_hw,out_hw,inside,kh,kv,rows,lds", FUSED_CASES, ids=_id)
def test_fused_edge_shapes_equal_pillow(golden_edges, in_hw, out_hw, inside, kh, kv, rows, lds):
    pre = _pre(in_hw, out_hw, fused=True)
    assert (pre.kh, pre.kv) == (kh, kv) and rows in (None, pre.band_rows)
    frames = torch.from_numpy(P.frames("random", in_hw)).cuda()
    x, u8 = _run(pre, frames, FUSED if inside else LDS)
    assert pre.fused is inside                                              # over the limit: refused, two passes from then on
    ref = P.oracle_u8("random", in_hw, out_hw)
    _check(x, u8, ref)
    _check_golden(golden_edges, "random", in_hw, out_hw, u8)
    x2, u82 = _run(_pre(in_hw, out_hw), frames, LDS)                        # every fused shape is an LDS shape in two passes
    assert np.array_equal(x2, x) and np.array_equal(u82, u8)


# ------------------------------------------------------------------ saturating patterns, one shape per kernel
@pytest.mark.gpu
@pytest.mark.parametrize("in_hw,out_hw,route", [((36, 40), (48, 64), LDS), ((35, 44), (40, 64), DWORD), ((33, 47), (24, 20), GENERIC),
                                                 ((64, 128), (80, 256), FUSED)], ids=_id)
def test_saturating_patterns_equal_pillow(golden_edges, in_hw, out_hw, route):
    """Constant, checkerboard, block and random-binary frames: accumulators far outside [0, 255] after either pass (the clip of the
    uint8 intermediate and the clip of the result), negative ones included."""
    assert (in_hw, out_hw) in P.PATTERN_SHAPES
    pre = _pre(in_hw, out_hw, fused=route == FUSED)
    for pattern in P.PATTERNS[1:]:
        x, u8 = _run(pre, torch.from_numpy(P.frames(pattern, in_hw)).cuda(), route)
        _check(x, u8, P.oracle_u8(pattern, in_hw, out_hw))
        _check_golden(golden_edges, pattern, in_hw, out_hw, u8)
        if pattern in ("zeros", "ones"):
            assert (u8 == (255 if pattern == "ones" else 0)).all(), pattern      # the weights sum to 2^22 only approximately
    assert pre.fused is (route == FUSED)


# ------------------------------------------------------------------ where the operands lie
@pytest.mark.gpu
def test_src_at_any_byte_offset_gives_the_same_bytes():
    """The frames inside a flat buffer whose other bytes are 255: 16-byte aligned (LDS kernel), 4-byte aligned (aligned-dword
    kernel), odd (generic kernel).  Same result each time, the oracle's: neither the address nor the bytes around the frames count."""
    in_hw, out_hw = (36, 40), (48, 64)
    frames = P.frames("random", in_hw)
    ref = P.oracle_u8("random", in_hw, out_hw)
    pre = _pre(in_hw, out_hw)
    got = []
    for off, route in ((0, LDS), (4, DWORD), (1, GENERIC)):
        buf = torch.full((16 + off + frames.size + 64,), 255, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        view = buf[16 + off:16 + off + frames.size].view(frames.shape)
        view.copy_(torch.from_numpy(frames))
        assert view.data_ptr() % 16 == off and view.is_contiguous()
        x, u8 = _run(pre, view, route)
        _check(x, u8, ref)
        got.append((x, u8))
        rest = torch.cat([buf[:16 + off], buf[16 + off + frames.size:]])
        assert bool((rest == 255).all()) and np.array_equal(view.cpu().numpy(), frames)    # the launch wrote nothing here
    assert all(np.array_equal(g[0], got[0][0]) and np.array_equal(g[1], got[0][1]) for g in got[1:])


@pytest.mark.gpu
def test_a_batch_slice_of_odd_sized_frames_is_accepted():
    """frames[1:] of (33, 47) frames starts 4653 bytes into the allocation: byte loads take it (it was refused before)."""
    in_hw, out_hw = (33, 47), (24, 20)
    frames = torch.from_numpy(P.frames("random", in_hw, n=3)).cuda()
    part = frames[1:]
    assert part.is_contiguous() and part.data_ptr() % 4 != 0
    x, u8 = _run(_pre(in_hw, out_hw), part, GENERIC)
    _check(x, u8, P.oracle_u8("random", in_hw, out_hw, n=2, seed=1))


@pytest.mark.gpu
def test_non_contiguous_frames_equal_their_contiguous_copy():
    in_hw, out_hw = (36, 40), (48, 64)
    frames = P.frames("random", in_hw)
    ref = P.oracle_u8("random", in_hw, out_hw)
    pre = _pre(in_hw, out_hw)
    base, base8 = _run(pre, torch.from_numpy(frames).cuda(), LDS)
    chw = torch.from_numpy(np.ascontiguousarray(frames.transpose(0, 3, 1, 2))).cuda().permute(0, 2, 3, 1)       # HWC view of CHW data
    doubled = torch.from_numpy(np.repeat(frames[:, None], 2, axis=1).copy()).cuda()
    doubled[:, 1] = 255
    for view, lead in ((chw, (2,)), (doubled[:, ::2], (2, 1))):
        assert not view.is_contiguous()
        x, u8 = _run(pre, view, LDS)
        assert x.shape == lead + (3,) + out_hw and u8.shape == lead + out_hw + (3,)
        _check(x.reshape(base.shape), u8.reshape(base8.shape), ref)
        assert np.array_equal(x.reshape(base.shape), base) and np.array_equal(u8.reshape(base8.shape), base8)


@pytest.mark.gpu
def test_leading_dimensions_from_none_to_three():
    in_hw, out_hw = (36, 40), (48, 64)
    frames = P.frames("random", in_hw, n=4)
    ref = P.oracle_u8("random", in_hw, out_hw, n=4)
    pre = _pre(in_hw, out_hw)
    x, u8 = _run(pre, torch.from_numpy(frames[3]).cuda(), LDS)
    assert x.shape == (3,) + out_hw and u8.shape == out_hw + (3,)
    _check(x[None], u8[None], ref[3:])
    x, u8 = _run(pre, torch.from_numpy(frames.reshape((2, 1, 2) + frames.shape[1:])).cuda(), LDS)
    assert x.shape == (2, 1, 2, 3) + out_hw and u8.shape == (2, 1, 2) + out_hw + (3,)
    _check(x, u8, ref.reshape((2, 1, 2) + ref.shape[1:]))


# ------------------------------------------------------------------ refusals
@pytest.mark.gpu
@pytest.mark.parametrize("in_hw,out_hw,kh,kv", [((36, 40), (24, 18), 11, 7),        # ow % 4 != 0: the vertical pass writes four columns per thread
                                                 ((120, 16), (16, 8), 9, 31),         # ksize_v > 24
                                                 ((560, 400), (100, 256), 9, 25)],    # the first window length over the accepted 23
                         ids=_id)
def test_unsupported_shapes_are_refused_and_leave_the_route_alone(in_hw, out_hw, kh, kv):
    good = _pre((36, 40), (48, 64))
    frames = torch.from_numpy(P.frames("random", (36, 40))).cuda()
    ref = P.oracle_u8("random", (36, 40), (48, 64))
    for fused, parked in ((False, GENERIC), (True, GENERIC), (False, LDS)):
        pre = _pre(in_hw, out_hw, fused=fused)
        assert (pre.kh, pre.kv) == (kh, kv)
        _park_route(LDS if parked == GENERIC else GENERIC)
        assert _route() == parked
        with pytest.raises(RuntimeError, match="EGR_EINVAL"):
            pre(torch.zeros((2,) + in_hw + (3,), dtype=torch.uint8, device="cuda"))
        assert _route() == parked
        torch.cuda.synchronize()
    x, u8 = _run(good, frames, LDS)                                         # and the next launch is as right as ever
    _check(x, u8, ref)

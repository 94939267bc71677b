"""The stem kernels' persistent tile walk and pooling seams against the float64 statement (tests/stem_statement.py), on a real MI355X.

stem_kernel (egr_stem.hip), stem_x6_kernel<POOL, 3 | 2> (egr_stem_x6.hip) and stem_wgrad_kernel start a workgroup at tile blockIdx.x and
walk tile += gridDim.x, fetching the next tile's patch under the current tile's products and parking it in the other half of a two-deep
LDS buffer.  The grid is GRID / groups workgroups per group, clamped to the tile count - so the stem cases of test_gpu_kernels.py and
test_gpu_train_kernels.py (one or two groups) run ONE tile per workgroup and never walk.  Here many groups shrink the grid: every walking
case computes its tile and workgroup counts from the constants below and asserts, before it launches, that some workgroup takes three
tiles or more, that the walks are uneven, that a walk crosses from one image into the next (and, for the main case, goes border tile ->
interior tile -> border tile).  A change of the grid rule makes these assertions say that the case no longer walks.

Per launch kind (fp32 MFMA `f32`, split-bf16 `x6`, fp16 scheme `h2`; raw, eval, pooled):
 (a) every element against float64: |y - ref| <= c * mag (raw), c * (mag |scale| + |shift|) (eval; pooled: the window's largest bound),
     mag = the sum of the magnitudes of the element's 147 terms;  c = 1e-6 raw / 1.2e-6 eval for x6 and h2 (what
     test_stem_h2_matches_torch_and_pools_bit_for_bit asserts), (147 + 3) * 2^-24 for the fp32 kernel (a chain over the taps + epilogue);
 (b) group g, image i of the walking launch == the launch of that image alone with groups = 1 (one tile per workgroup), bit for bit;
 (c) pooled == unpooled + hip.maxpool(3, 2, 1), bit for bit, into a buffer of the test's own filled with 1e30, twice;
 (d) the abs-max record of the pooled x6 / h2 launches == max |pooled output| exactly.
A failure names the (group, workgroup, step of its walk) of the offending tiles.

Largest measured err / mag (MI355X) over all cases of this file, printed by every test beside its bound:
   f32   raw 8.9e-07   eval 9.4e-07   pooled 6.2e-07      (bound 8.94e-06)
   x6    raw 5.9e-07   eval 5.1e-07   pooled 4.4e-07      (bounds 1e-06 raw, 1.2e-06 eval / pooled)
   h2    raw 6.7e-07   eval 5.8e-07   pooled 5.8e-07      (the same)
   weight gradient 4.8e-07 (one workgroup per group), 4.0e-08 (eight)   (bounds 1.2e-04 / 5.5e-04; from the order of accumulation 3.1e-05 / 1.9e-05)
torch's float32 convolution of the same inputs sits at 2.4e-07 ... 8.9e-07 (test_stem_statement_host.py).
"""
import pytest
import torch

import stem_statement as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE = {"f32": (8, 32), "x6": (16, 32), "h2": (16, 32)}      # conv pixels of a tile (rows, columns): egr_stem.hip / egr_stem_x6.hip TH, TW
GRID = {"f32": 512, "x6": 256, "h2": 256}                     # workgroups shared by the groups of a launch (stem_wgrad_kernel: as f32)
KINDS = ("f32", "x6", "h2")
C_RAW = {"f32": (147 + 3) * 2.0 ** -24, "x6": 1e-6, "h2": 1e-6}
C_EVAL = {"f32": (147 + 3) * 2.0 ** -24, "x6": 1.2e-6, "h2": 1.2e-6}

# The geometries live in stem_statement.py (WALK_CASES: nviews = 1, V = groups views; "main" also walks border -> interior -> border,
# "single" has one workgroup per group; EDGE_SHAPES; VIEW_CASE), where the host test holds the reference to its condition on the same inputs.


@pytest.fixture(scope="module")
def hip():
    from egorear_amd import hip as h
    assert torch.cuda.is_available()
    assert "gfx950" in h.device_arch()
    return h


class Geo:
    """Tiles and workgroups of a launch, from the constants above (the rule of the entry points: GRID / groups, at least 1, at most the
    group's tiles)."""

    def __init__(self, kind, B, H, W, groups, nviews=1):
        self.th, self.tw = TILE[kind]
        self.n, self.groups = nviews * B, groups
        self.ty, self.tx = (H // 2) // self.th, (W // 2) // self.tw
        self.tpi = self.ty * self.tx
        self.tiles = self.n * self.tpi
        self.blocks = max(1, min(GRID[kind] // groups, self.tiles))

    def border(self, t):
        y, x = (t % self.tpi) // self.tx, (t % self.tpi) % self.tx
        return y in (0, self.ty - 1) or x in (0, self.tx - 1)

    def assert_walks(self, name):
        t, b = self.tiles, self.blocks
        assert -(-t // b) >= 3, f"{name}: no workgroup takes three tiles ({t} tiles on {b} workgroups): the case no longer covers the walk"
        if name == "single":
            assert b == 1, f"{name}: {b} workgroups per group, one expected"
        else:
            assert t % b != 0, f"{name}: {t} tiles on {b} workgroups: the walks are all of one length"
        assert any(i // self.tpi != (i + b) // self.tpi for i in range(t - b)), f"{name}: no walk crosses an image boundary"
        if name == "main":
            assert any(self.border(i) and not self.border(i + b) and self.border(i + 2 * b) for i in range(t - 2 * b)), \
                f"{name}: no walk goes border tile -> interior tile -> border tile"

    def one_tile_each(self):
        return self.tiles <= self.blocks

    def where(self, bad, pooled=False):
        """bad: bool (groups*n, h, w, 64) -> the offending tiles as 'g<group> wg<workgroup> step<k>' (k-th tile of that workgroup's walk)."""
        idx = bad.nonzero()[:, :3]
        if idx.numel() == 0:
            return "none"
        f = 2 if pooled else 1
        img = idx[:, 0] % self.n
        t = img * self.tpi + (idx[:, 1] * f // self.th) * self.tx + idx[:, 2] * f // self.tw
        key = torch.unique((idx[:, 0] // self.n) * self.tiles + t)
        out = [f"g{int(k) // self.tiles} wg{int(k) % self.tiles % self.blocks} step{int(k) % self.tiles // self.blocks}" for k in key[:12]]
        return f"{bad.sum().item()} elements in {key.numel()} tiles: " + ", ".join(out) + (" ..." if key.numel() > 12 else "")


class Bank:
    """A launch's operands on the device: the image batch, the filters in the three kernels' formats, scale / shift."""

    def __init__(self, hip, img, w, scale, shift):
        self.hip = hip
        self.img = img.to(DEV)
        self.wp = S.pack_w(w).to(DEV)
        self.w6 = hip.pack_stem_w6(self.wp)
        self.wh2, self.wds = hip.pack_stem_wh2(self.wp)
        self.scale, self.shift = scale.to(DEV), shift.to(DEV)
        self.groups = w.shape[0]

    def only(self, g, b, v):
        """The bank of group g alone with image (b, v) as a batch of one."""
        o = object.__new__(Bank)
        o.hip, o.groups = self.hip, 1
        o.img = self.img[b:b + 1, v:v + 1].contiguous()
        o.wp, o.w6, o.wh2, o.wds = self.wp[g:g + 1], self.w6[g:g + 1], self.wh2[g:g + 1], self.wds[g:g + 1]
        o.scale, o.shift = self.scale[g:g + 1], self.shift[g:g + 1]
        return o

    def run(self, kind, mode, view0=0, nviews=1):
        """mode raw / eval / pool through the Python wrappers -> the output tensor."""
        hip, sc, sh = self.hip, None if mode == "raw" else self.scale, None if mode == "raw" else self.shift
        if kind == "f32":
            f = hip.stem_pool if mode == "pool" else hip.stem
            return f(self.img, view0, nviews, self.wp, sc, sh, groups=self.groups).t
        kw = dict(w_descale=self.wds) if kind == "h2" else {}
        return hip.stem_x6(self.img, view0, nviews, self.wh2 if kind == "h2" else self.w6, sc, sh, groups=self.groups,
                           pool=mode == "pool", **kw).t

    def pool_into(self, kind, y, view0=0, nviews=1, rec=None):
        """The pooled launch through the C entry point itself, into the caller's buffer y (and abs-max record rec)."""
        hip = self.hip
        B, V, _, H, W = self.img.shape
        p, n = hip._p, nviews * B
        base = self.img.reshape(-1)[view0 * 3 * H * W:]
        xmap = hip.NMap(B, V * 3 * H * W, 3 * H * W)
        assert view0 >= 0 and view0 + self.groups * nviews <= V
        assert y.is_contiguous() and tuple(y.shape) == (self.groups * n, H // 4, W // 4, 64) and y.dtype == torch.float32
        if kind == "f32":
            assert rec is None
            hip._launch("egr_stem_conv7x7_pool_f32", hip.lib.egr_stem_conv7x7_pool_f32, p(base), xmap, n, H, W, p(self.wp), p(self.scale),
                        p(self.shift), p(y), self.groups, nviews * 3 * H * W, hip._stream())
        elif kind == "x6":
            hip._launch("egr_stem_conv7x7_x6_ex_f32", hip.lib.egr_stem_conv7x7_x6_ex_f32, p(base), xmap, n, H, W, p(self.w6, torch.uint8),
                        p(self.scale), p(self.shift), p(y), 1, self.groups, nviews * 3 * H * W, p(rec, torch.int32), hip._stream())
        else:
            hip._launch("egr_stem_conv7x7_h2_f32", hip.lib.egr_stem_conv7x7_h2_f32, p(base), xmap, n, H, W, p(self.wh2, torch.uint8),
                        p(self.wds), p(self.scale), p(self.shift), p(y), 1, self.groups, nviews * 3 * H * W, p(rec, torch.int32),
                        hip._stream())


class Case:
    """Inputs, device operands and the float64 statement (convolution and magnitude once; eval / pooled forms derived) of one geometry."""

    def __init__(self, hip, B, V, H, W, groups, seed, view0, nviews):
        self.B, self.V, self.H, self.W, self.groups, self.view0, self.nviews = B, V, H, W, groups, view0, nviews
        self.img, self.w, self.scale, self.shift = S.stem_inputs(B, V, H, W, groups, seed)
        self.bank = Bank(hip, self.img, self.w, self.scale, self.shift)
        self.conv = S.stem_conv(self.img, view0, nviews, self.w, groups)
        self.mag = S.stem_conv(self.img, view0, nviews, self.w, groups, magnitude=True)
        self._memo = {}

    def ref_and_bound(self, kind, mode):
        """(float64 reference, per-element bound c * magnitude) of a mode; the reference is computed once and never written."""
        if mode not in self._memo:
            sc, sh = (None, None) if mode == "raw" else (self.scale, self.shift)
            self._memo[mode] = (S.stem_epilogue(self.conv, sc, sh, self.groups, mode == "pool"),
                                S.mag_epilogue(self.mag, sc, sh, self.groups, mode == "pool"))
        ref, mag = self._memo[mode]
        return ref, mag, (C_RAW if mode == "raw" else C_EVAL)[kind]

    def geo(self, kind):
        return Geo(kind, self.B, self.H, self.W, self.groups, self.nviews)

    def run(self, kind, mode):
        return self.bank.run(kind, mode, self.view0, self.nviews)

    def check_a(self, kind, mode, y, label):
        ref, mag, c = self.ref_and_bound(kind, mode)
        assert y.shape == ref.shape, (y.shape, ref.shape)
        err = (y.double().cpu() - ref).abs()
        ratio = float((err / mag.clamp_min(1e-300)).max())
        print(f"{label} {kind} {mode}: max err / mag {ratio:.3e}  (bound {c:.3e})")
        bad = ~(err <= c * mag)          # (a NaN is bad)
        assert not bool(bad.any()), f"{label} {kind} {mode}: err / mag {ratio:.3e} > {c:.3e}; {self.geo(kind).where(bad, mode == 'pool')}"

    def check_c(self, kind, label, rec=False):
        """(c), and (d) when rec: the pooled launch into a 1e30-filled buffer of the test's own == unpooled + maxpool, twice."""
        hip = self.bank.hip
        two = hip.maxpool(hip.Img(self.run(kind, "eval")), 3, 2, 1).t
        y = torch.full_like(two, 1e30)
        for turn in range(2):
            r = torch.zeros(64, dtype=torch.int32, device=DEV) if rec else None
            self.bank.pool_into(kind, y, self.view0, self.nviews, r)
            bad = y != two
            assert torch.equal(y, two), f"{label} {kind} pooled (turn {turn}) != unpooled + maxpool; {self.geo(kind).where(bad.cpu(), True)}"
            if rec:
                assert float(r.view(torch.float32).max()) == float(two.abs().max()) > 0.0, f"{label} {kind}: abs-max record"
            y.fill_(1e30)


@pytest.fixture(scope="module", params=list(S.WALK_CASES))
def walk(request, hip):
    case = Case(hip, *S.WALK_CASES[request.param])
    case.name = request.param
    yield case
    del case
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind", KINDS)
def test_walking_launch_matches_float64(walk, kind):
    """(a) for the raw, eval and pooled launch of a walking grid."""
    walk.geo(kind).assert_walks(walk.name)
    for mode in ("raw", "eval", "pool"):
        walk.check_a(kind, mode, walk.run(kind, mode), f"walk {walk.name}")


@pytest.mark.parametrize("kind", KINDS)
def test_walking_launch_is_the_single_image_launch_bit_for_bit(walk, kind):
    """(b): the pre-scale of a tile depends on its patch only and the order of accumulation inside a tile is fixed, so what a workgroup
    computed before (or fetches next) must not reach a tile's bits."""
    geo, G, n = walk.geo(kind), walk.groups, walk.B
    geo.assert_walks(walk.name)
    pairs = [(0, 0), (G - 1, n - 1), (G // 2, n - 1), (1, n // 2), (G - 2, 0)]      # first / last group, images reached late in a walk
    for mode in ("raw", "eval", "pool"):
        big = walk.run(kind, mode)
        for g, i in pairs:
            one = walk.bank.only(g, i, g)
            assert Geo(kind, 1, walk.H, walk.W, 1).one_tile_each()
            alone = one.run(kind, mode)
            got = big[g * n + i:g * n + i + 1]
            if not torch.equal(got, alone):
                bad = torch.zeros(big.shape, dtype=torch.bool)
                bad[g * n + i] = (got != alone).cpu()[0]
                pytest.fail(f"walk {walk.name} {kind} {mode}: group {g} image {i} differs from its launch alone; {geo.where(bad, mode == 'pool')}")


@pytest.mark.parametrize("kind", KINDS)
def test_walking_pooled_launch_is_stem_then_maxpool_and_keeps_its_record(walk, kind):
    """(c) and (d) on a walking grid: the exchange area of the pooling epilogue shares the patch buffers with the prefetched patch, the
    abs-max record accumulates over a workgroup's tiles."""
    walk.geo(kind).assert_walks(walk.name)
    walk.check_c(kind, f"walk {walk.name}", rec=kind != "f32")


def test_weight_gradient_on_a_walking_grid(walk, hip):
    """stem_wgrad_kernel sums a workgroup's tiles in its accumulators (per wave a chain over the 64 pixels of its two tile rows, tile after
    tile of the walk), the four waves through LDS, the workgroups' slabs in four interleaved partial sums of slab order.  Against
    stem_wgrad_ref: within one rounding (2^-24 of the summed magnitudes) per summed term, n * ho * wo of them, and within the tighter bound
    that this order gives - the longest chain has 64 * walk + 3 + ceil(blocks / 4) + 2 additions.  The workspace is groups * blocks slabs
    of 64 x 160 floats, filled with 1e30 here (every slab is written whole); one float fewer is refused on the host."""
    from egorear_amd import hip_train as T
    geo = walk.geo("f32")
    geo.assert_walks(walk.name)
    G, n, ho, wo = walk.groups, walk.B, walk.H // 2, walk.W // 2
    dy = S.rnd(G * n, ho, wo, 64, seed=77)
    dy[:, :, :, 3] *= 1e-3
    dy[n:2 * n] *= 50.0
    ws = torch.full((G * geo.blocks * 64 * 160,), 1e30, device=DEV)
    dw = T.stem_wgrad(walk.bank.img, 0, 1, dy.to(DEV), ws, groups=G)
    ref, mag = S.stem_wgrad_ref(walk.img, 0, 1, dy, G)
    err = (dw.double().cpu() - ref).abs()
    ratio = float((err / mag.clamp_min(1e-300)).max())
    c = n * ho * wo * 2.0 ** -24
    walk_len = -(-geo.tiles // geo.blocks)
    c_chain = (64 * walk_len + 3 + -(-geo.blocks // 4) + 2) * 2.0 ** -24
    print(f"walk {walk.name} wgrad: max err / mag {ratio:.3e}  (bound {c:.3e}; from the order of accumulation {c_chain:.3e})")
    assert torch.all(err <= c * mag), (ratio, c)
    assert torch.all(err <= c_chain * mag), (ratio, c_chain)
    with pytest.raises(hip.LaunchError) as e:
        T.stem_wgrad(walk.bank.img, 0, 1, dy.to(DEV), ws[:-1], groups=G)
    assert e.value.code == hip.EWORKSPACE


# ---------------------------------------------------------------------------------------------------- edge geometries, one tile per workgroup

@pytest.mark.parametrize("shape", ["one tile", "row seams", "column seams"])
@pytest.mark.parametrize("kind", KINDS)
def test_edge_geometries(hip, kind, shape):
    """(a) and (c) where all four image borders, or the seams of one direction only, meet in a launch."""
    H, W = S.EDGE_SHAPES["f32" if kind == "f32" else "x6"][shape]
    case = Case(hip, *S.edge_case(H, W))
    geo = case.geo(kind)
    assert geo.one_tile_each() and (geo.ty, geo.tx) == {"one tile": (1, 1), "row seams": (2, 1), "column seams": (1, 2)}[shape]
    for mode in ("raw", "eval", "pool"):
        case.check_a(kind, mode, case.run(kind, mode), f"{H}x{W} ({shape})")
    case.check_c(kind, f"{H}x{W} ({shape})", rec=kind != "f32")


@pytest.mark.parametrize("kind", ["x6", "h2"])
def test_first_view_skipped_and_group_stride_unlike_view_stride(hip, kind):
    """view0 = 1, nviews = 2, groups = 2 on six views: group g takes the views 1 + 2g and 2 + 2g, view 0 and view 5 are not read."""
    case = Case(hip, *S.VIEW_CASE)
    assert case.geo(kind).one_tile_each()
    for mode in ("raw", "eval", "pool"):
        case.check_a(kind, mode, case.run(kind, mode), "view0 = 1")
    case.check_c(kind, "view0 = 1", rec=True)

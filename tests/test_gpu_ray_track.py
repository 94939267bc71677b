"""The ray-space clip smoother on the GPU (egr_ray_track_f32, egorear_amd/decode.py) against the float64 statement of
tests/ray_track_statement.py.

Yardstick: fisheye_statement's - a HIP output may deviate from the float64 statement (on the same fp32 operands) by at most MARGIN = 8 x
the deviation of the float32 evaluation of that statement, with a floor of 4 ulp (fp32) of the output's largest magnitude.  Where the
float32 evaluation does not factor or is not finite the floor alone holds; the kernel eliminates in fp64 and can meet it.  The
solvability flags of both evaluations are the float64 ones.

Shapes (N, T, V, J): T = 1..5 are the band's corners (no, one and two sub-diagonals, the first full row); 8 and 9 end a chunk of the
backward sweep's prefetch and start the next; (4, 5, 2, 16) fills a wave with 64 tracks and (5, 9, 4, 13) spills one track into a
second workgroup; (3, 64, 4, 15) is a clip of the serving path."""
import itertools

import pytest
import torch

import fisheye_statement as FS
import ray_track_statement as RS
import trajectory_statement as TS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1, 2, 1), (2, 2, 3, 3), (1, 3, 4, 2), (2, 4, 4, 15), (4, 5, 2, 16), (1, 8, 3, 4), (5, 9, 4, 13), (3, 64, 4, 15)]
LAMBDAS = [(0.0, 10.0), (1.0, 0.0), (0.5, 100.0), (0.0, 1000.0)]          # (lambda_v, lambda_a): the trajectory test's pairs
MODES = [(0.0, 0), (1.0, 1), (1.0, 4)]                                     # (huber, K)
OUTPUTS = ("pose", "residual", "weight", "energy")
NAMES = ("pose", "valid", "residual", "weight", "rays", "energy")
_SCENES, _REFS = {}, {}


def scene(shape, case, rw):
    if (shape, case, rw) not in _SCENES:
        _SCENES[shape, case, rw] = RS.scene(*shape, case, rw)
    return _SCENES[shape, case, rw]


def reference(shape, case, rw, lam, mode, gap):
    """The statement in float64 and float32 on the case's fp32 operands, computed once and shared (never modified); "f32" is the float64
    one where the float32 evaluation does not factor or is not finite: its own deviation is then 0 and the floor alone holds."""
    key = (shape, case, rw, lam, mode, gap)
    if key not in _REFS:
        sc = scene(shape, case, rw)
        args = (sc["coords"], sc["conf"], sc["rec"], sc["ctm"], sc["sx"], sc["sy"])
        kw = dict(lv=lam[0], la=lam[1], huber=mode[0], reweights=mode[1], max_gap=gap)
        f64 = RS.fit(*args, **kw)
        f32 = RS.try_fit(*args, dt=torch.float32, **kw)
        _REFS[key] = {"f64": f64, "f32": f64 if f32 is None else f32, "f32_failed": f32 is None}
    return _REFS[key]


def dev(t):
    return None if t is None else t.to(DEV)


def launch(sc, lam, mode, gap, coords=None):
    from egorear_amd import hip
    out = hip.ray_track(dev(sc["coords"] if coords is None else coords), dev(sc["conf"]), dev(sc["rec"]), dev(sc["ctm"]), sc["sx"], sc["sy"], 0.5,
                        lam[0], lam[1], mode[0], mode[1], gap)
    torch.cuda.synchronize()
    return dict(zip(NAMES, (t.cpu() for t in out)))


def combos(shape):
    """(lambda, mode, max_gap, rw): every pair of penalties meets every mode on the small shapes; the clip of 64 frames, whose dense
    float64 and float32 statements take a second a solve, meets every penalty once and every mode."""
    N, T, V, J = shape
    every = list(itertools.product(LAMBDAS, MODES))
    if N * T * J > 1000:
        every = [(LAMBDAS[i], MODES[i % 3]) for i in range(4)]
    return [(lam, mode, (0, 3, T)[(i + i // 3) % 3], bool((i + i // 3) % 2)) for i, (lam, mode) in enumerate(every)]


@pytest.mark.parametrize("case", RS.CASES)
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_statement(shape, case):
    N, T, V, J = shape
    bad = []
    for lam, mode, gap, rw in combos(shape):
        sc = scene(shape, case, rw)
        ref = reference(shape, case, rw, lam, mode, gap)
        got = launch(sc, lam, mode, gap)
        f64 = ref["f64"]
        print(f"{shape} {case} {'ctm' if rw else 'syn'} lambda {lam} huber {mode[0]} K {mode[1]} max_gap {gap}: cond(A) {f64['cond']:.3e}, "
              f"{int(f64['ok'].sum())} of {N * J} tracks solvable, {int(f64['valid'].sum())} of {N * T * J} frames valid"
              f"{', float32 evaluation failed' if ref['f32_failed'] else ''}")
        assert torch.equal(got["valid"].bool(), f64["valid"]), (shape, case, rw, lam, mode, gap)
        assert torch.equal(got["rays"], f64["rays"]), (shape, case, rw, lam, mode, gap)
        for name in OUTPUTS:
            assert bool(torch.isfinite(got[name]).all()), (shape, case, rw, lam, mode, name)
            err, allowed = FS.yardstick(name, got[name], ref["f32"][name], f64[name])
            if not err <= allowed:
                bad.append((shape, case, rw, lam, mode, name, err, allowed))
        dead = ~f64["ok"]                                                              # a track that is not solvable gives zeros
        assert float(got["pose"].transpose(1, 2)[dead].abs().sum()) == 0.0 and float(got["energy"][dead].abs().sum()) == 0.0
        for name in ("residual", "weight"):
            assert float(got[name].permute(0, 3, 1, 2)[dead].abs().sum()) == 0.0
        assert not bool(got["valid"].transpose(1, 2)[dead].any()) and int(got["rays"].transpose(1, 2)[dead].sum()) == 0
        unused = ~((sc["conf"] >= 0.5) & (sc["conf"] > 0))
        assert float(got["residual"][unused].abs().sum()) == 0.0 and float(got["weight"][unused].abs().sum()) == 0.0
    assert not bad, bad


@pytest.mark.parametrize("shape", [(2, 4, 4, 15), (5, 9, 4, 13), (3, 64, 4, 15)])
def test_hubers_energy_does_not_increase_with_the_rounds(shape):
    """K = 0 is the plain solve, whose rho is the square >= Huber's; every further round is a majorise-minimise step.  The energies are
    fp64 sums rounded to fp32 once: a round may appear to rise by the two roundings, one ulp of the energy, and no more."""
    bad = []
    for lam, rw in zip(LAMBDAS, (False, True, True, False)):
        sc = scene(shape, "glitch", rw)
        before = None
        for K in range(7):
            got = launch(sc, lam, (0.0, 0) if K == 0 else (1.0, K), 8)["energy"].double()
            print(f"{shape} {'ctm' if rw else 'syn'} lambda {lam} K {K}: energy {float(got.sum()):.6f}")
            assert bool(torch.isfinite(got).all())
            if before is not None:
                ulp = torch.tensor([[FS.ulp32(float(v)) for v in row] for row in before], dtype=torch.float64)
                if not bool((got <= before + ulp).all()):
                    bad.append((shape, lam, K, float((got - before).max())))
            before = got
    assert not bad, bad


@pytest.mark.parametrize("shape", SHAPES)
def test_what_is_planted_in_an_unused_ray_reaches_no_output(shape):
    for rw in (False, True):
        sc = scene(shape, "gaps", rw)
        unused = ~((sc["conf"] >= 0.5) & (sc["conf"] > 0))
        planted = sc["coords"].clone()
        values = torch.tensor([float("nan"), float("inf"), float("-inf"), 3.0e38, -1.0e30])
        pick = torch.randint(0, 5, sc["coords"].shape, generator=torch.Generator().manual_seed(3))
        planted[unused] = values[pick][unused]
        assert int(unused.sum()) > 0
        for lam, mode in ((LAMBDAS[0], MODES[0]), (LAMBDAS[2], MODES[2]), (LAMBDAS[1], MODES[1])):
            clean, dirty = launch(sc, lam, mode, 3), launch(sc, lam, mode, 3, coords=planted)
            for name in NAMES:
                assert bool(torch.isfinite(dirty[name].float()).all()), (shape, rw, lam, mode, name)
                assert torch.equal(clean[name], dirty[name]), (shape, rw, lam, mode, name)


def test_bits_do_not_depend_on_the_batch_the_run_or_a_graph_replay():
    from egorear_amd import hip
    for case, rw, lam, mode in (("gaps", False, (0.0, 10.0), (0.0, 0)), ("glitch", True, (0.5, 100.0), (1.0, 4)), ("oneview", True, (1.0, 0.0), (0.0, 0))):
        sc = scene((3, 64, 4, 15), case, rw)
        c, f, r, m = dev(sc["coords"]), dev(sc["conf"]), dev(sc["rec"]), dev(sc["ctm"])
        run = lambda cc, ff, mm: hip.ray_track(cc, ff, r, mm, sc["sx"], sc["sy"], 0.5, lam[0], lam[1], mode[0], mode[1], 3)
        cut = lambda t, n: None if t is None else t[n:n + 1].contiguous()
        eager, again = run(c, f, m), run(c, f, m)
        for a, b in zip(eager, again):
            assert torch.equal(a, b)
        for n in range(3):                                                             # a clip alone and inside the batch of three
            for a, b in zip(eager, run(cut(c, n), cut(f, n), cut(m, n))):
                assert torch.equal(a[n:n + 1], b)
        torch.cuda.synchronize()
        static = c.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                                  # one stream, no parallel branches
            out = run(static, f, m)
        static.copy_(torch.zeros_like(c))
        graph.replay()
        static.copy_(c)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, out):
            assert torch.equal(a, b)
        assert bool(eager[1].any()) and float(eager[5].max()) > 0.0


@pytest.fixture(scope="module")
def clip_maps():
    """Gaussian bumps (sigma 1, 64 x 64) at the projections of a moving 15-joint skeleton, N = 2 clips of T = 6 frames, V = 4, on the syn
    rig; a few joints lose three of their views for a frame or two: one ray is left, which the triangulation gives up."""
    g = torch.Generator().manual_seed(91)
    cams = FS.rig()
    rec = FS.records(cams)
    pts = TS.motion(2, 6, 15, g)
    hm = FS.bumps(pts.view(12, 15, 3), rec, None, FS.HM, FS.HM).float().view(2, 6, 4, 15, FS.HM, FS.HM).contiguous()
    lost = ((0, 2, 3), (0, 3, 3), (1, 0, 7), (1, 5, 14), (0, 4, 0))
    for n, t, j in lost:
        hm[n, t, 1:, j] = 0.0
    return {"cams": cams, "pts": pts, "hm": hm, "lost": lost}


def test_decode_clip_3d_rays_is_its_launches(clip_maps):
    from egorear_amd import decode, hip
    hm, cams = clip_maps["hm"].to(DEV), clip_maps["cams"]
    kw = dict(accel_weight=10.0, vel_weight=0.5, huber_cm=1.0, reweights=2, max_gap=2)
    decode.decode_clip_3d_rays(hm, cams, **kw)                                         # (warms the record cache)
    hip.PROFILE = []
    try:
        joints, track = decode.decode_clip_3d_rays(hm, cams, **kw)
        torch.cuda.synchronize()
        names = [e[0] for e in hip.PROFILE]
    finally:
        hip.PROFILE = None
    assert names == ["egr_soft_argmax_f32", "egr_ray_track_f32"], names                # (the entry issues the ray pass and the solve)
    # the pieces, called one by one
    flat = decode.decode_joints_2d(hm.view(12, 4, 15, FS.HM, FS.HM))
    by_hand = decode.fit_ray_tracks(flat.soft.view(2, 6, 4, 15, 2), flat.maxvals.view(2, 6, 4, 15), cams, None, (FS.HM, FS.HM), **kw)
    for a, b in zip(track, by_hand):
        assert torch.equal(a, b)
    for a, b in zip(joints, flat):
        assert torch.equal(a.reshape(b.shape), b)
    assert joints.soft.shape == (2, 6, 4, 15, 2) and track.pose.shape == (2, 6, 15, 3) and track.residual.shape == (2, 6, 4, 15)
    assert track.valid.dtype == torch.bool and track.rays.dtype == torch.uint8
    for n, t, j in clip_maps["lost"]:                                                  # one ray is a measurement here, not a hole
        assert int(track.rays[n, t, j]) == 1 and bool(track.valid[n, t, j]) and float(track.weight[n, t, 0, j]) > 0.0
    err = (track.pose.double().cpu() - clip_maps["pts"]).norm(dim=-1)
    print(f"mean error {float(err.mean()):.4e} cm, at the frames with one ray {[round(float(err[i]), 4) for i in clip_maps['lost']]}")
    assert bool(torch.isfinite(err).all())
    one_j, one_t = decode.decode_clip_3d_rays(hm[1], cams, **kw)                       # (T, V, J, H, W): one clip, the same bits
    assert one_t.pose.shape == (6, 15, 3) and one_j.soft.shape == (6, 4, 15, 2)
    for a, b in zip(one_t, track):
        assert torch.equal(a, b[1])
    for a, b in zip(one_j, joints):
        assert torch.equal(a, b[1])
    alone = decode.fit_ray_tracks(joints.soft[1], joints.maxvals[1], cams, None, (FS.HM, FS.HM), **kw)
    for a, b in zip(alone, track):
        assert torch.equal(a, b[1])


def test_inputs_that_require_grad_give_outputs_that_do_not(clip_maps):
    from egorear_amd import decode
    sc = scene((2, 4, 4, 15), "dense", True)
    c, f, m = dev(sc["coords"]).requires_grad_(), dev(sc["conf"]).requires_grad_(), dev(sc["ctm"]).requires_grad_()
    for kw in ({}, {"huber_cm": 1.0, "reweights": 2}):
        track = decode.fit_ray_tracks(c, f, sc["cams"], m, **kw)
        assert not any(t.requires_grad for t in track)
        with pytest.raises(RuntimeError):
            track.pose.sum().backward()
    maps = clip_maps["hm"].to(DEV).requires_grad_()
    joints, track = decode.decode_clip_3d_rays(maps, clip_maps["cams"])
    assert joints.soft.requires_grad and not any(t.requires_grad for t in track)


def test_bad_launches_are_refused():
    from egorear_amd import hip
    sc = scene((2, 4, 4, 15), "dense", False)
    c, f, r = dev(sc["coords"]), dev(sc["conf"]), dev(sc["rec"])
    good = dict(sx=sc["sx"], sy=sc["sy"], threshold=0.5, vel_weight=0.0, accel_weight=10.0, huber=0.0, reweights=0, max_gap=8, min_pivot_ratio=1e-10)
    for kw in ({"vel_weight": -1.0}, {"accel_weight": 0.0}, {"huber": 1.0}, {"reweights": 2}, {"huber": 1.0, "reweights": 17}, {"max_gap": -1},
               {"accel_weight": float("nan")}, {"min_pivot_ratio": 1.0}, {"sx": 0.0}):
        with pytest.raises(ValueError):
            hip.ray_track(c, f, r, None, **dict(good, **kw))
    with pytest.raises(ValueError):
        hip.ray_track(c, f[:, :3], r, None, **good)
    with pytest.raises(ValueError):
        hip.ray_track(c.transpose(0, 1), f.transpose(0, 1), r, None, **good)
    with pytest.raises(ValueError):
        hip.ray_track(c, f, r[:3], None, **good)

"""The information-weighted clip smoother on the GPU (egr_joint_info_f32, egr_info_track_f32, egorear_amd/decode.py)
against the float64 statements of tests/info_track_statement.py.

Yardstick: fisheye_statement's - a HIP output may deviate from the float64 statement (on the same fp32 operands) by at most MARGIN = 8 x
the deviation of the float32 evaluation of that statement, with a floor of 4 ulp (fp32) of the output's largest magnitude.  Where the
float32 evaluation does not factor or is not finite the floor alone holds; the kernels compute in fp64 and can meet it.  The discrete
outputs (views, valid, the solvability) are the float64 ones.

Shapes of the smoother (N, T, J), as test_gpu_ray_track.py explains them: T = 1..5 are the band's corners; 8 and 9 end a chunk of the
sweeps' prefetch and start the next; (4, 5, 16) fills a wave with 64 tracks and (5, 9, 13) spills one track into a second workgroup;
(3, 64, 15) is a clip of the serving path.  Shapes of the matrix (B, V, J): one thread, a few, a frame's worth, and (64, 4, 16) - 1024
threads, eight full workgroups of 128 - next to (3, 4, 15), whose only workgroup is partial."""
import itertools

import pytest
import torch

import fisheye_statement as FS
import info_track_statement as IS
import trajectory_statement as TS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1, 1), (2, 2, 3), (1, 3, 2), (2, 4, 15), (4, 5, 16), (1, 8, 4), (5, 9, 13), (3, 64, 15)]
INFO_SHAPES = [(1, 2, 1), (2, 3, 3), (3, 4, 15), (64, 4, 16)]
LAMBDAS = [(0.0, 10.0), (1.0, 0.0), (0.5, 100.0), (0.0, 1000.0)]          # (lambda_v, lambda_a): the trajectory test's pairs
MODES = [(0.0, 0), (1.0, 1), (1.0, 4)]                                     # (huber in pixels, K)
OUTPUTS = ("pose", "residual", "weight", "energy")
NAMES = ("pose", "valid", "residual", "weight", "energy")
INFO_NAMES = ("info", "views", "sigma", "valid")
INFO_CASES = ("every", "emptied", "behind", "axis", "nan")
_SCENES, _REFS, _POINTS = {}, {}, {}


def dev(t):
    return None if t is None else t.to(DEV)


# --------------------------------------------------------------------------- the information matrix

def points_scene(shape, case, rw):
    """Points in the working volume seen by the rig, fp32: `every` view confident; `emptied` views below the threshold, at 0 and at NaN,
    some joints down to one view and to none; `behind` points behind the rig (z < 0: the polynomial still gives a pixel); `axis` a
    joint a frame exactly on a camera's optical axis, in front of it and behind (the syn rig: its offsets are fp32 integers, so the
    camera-frame x and y are exact zeros on both sides); `nan` points with a NaN or an infinity."""
    key = (shape, case, rw)
    if key in _POINTS:
        return _POINTS[key]
    B, V, J = shape
    g = torch.Generator().manual_seed(17 * B + 5 * V + J + 1000 * INFO_CASES.index(case) + (500 if rw else 0))
    cams = FS.rig("ego4view_rw" if rw else "ego4view_syn")[:V]
    rec = FS.records(cams)
    pts = FS.random_points(B, J, g).float()
    conf = (0.6 + 0.4 * torch.rand(B, V, J, generator=g)).float()
    ctm = FS.random_ctm(B, V, cams, g) if rw else None
    if case == "emptied":
        kind = torch.randint(0, 6, (B, V, J), generator=g)
        conf[kind == 0] = 0.3
        conf[kind == 1] = 0.0
        conf[kind == 2] = float("nan")
        conf[0, 1:, 0] = 0.0                                                            # one view
        conf[B - 1, :, J - 1] = 0.2                                                     # none
    elif case == "behind":
        pts[..., 2] = -pts[..., 2]
    elif case == "axis":
        for b in range(B):
            v, j = b % V, b % J
            off = rec[v, 27:30]
            fl = -1.0 if float(rec[v, 26]) != 0 else 1.0
            pts[b, j] = torch.tensor([-fl * float(off[0]), -fl * float(off[1]), 60.0 if b % 2 == 0 else -60.0])
    elif case == "nan":
        bad = torch.tensor([float("nan"), float("inf"), float("-inf")])
        hit = torch.rand(B, J, generator=g) < 0.3
        hit[0, 0] = True
        for b, j in hit.nonzero().tolist():
            pts[b, j, (b + j) % 3] = bad[(b + 2 * j) % 3]
    _POINTS[key] = {"points": pts.contiguous(), "conf": conf.contiguous(), "rec": rec, "ctm": ctm, "cams": cams, "sx": 1.0 / FS.HM, "sy": 1.0 / FS.HM}
    return _POINTS[key]


def info_launch(sc, points=None, conf=None, ctm=None):
    from egorear_amd import hip
    out = hip.joint_info(dev(sc["points"] if points is None else points), dev(sc["conf"] if conf is None else conf), dev(sc["rec"]),
                         dev(sc["ctm"] if ctm is None else ctm), sc["sx"], sc["sy"], 0.5, 1e-6)
    torch.cuda.synchronize()
    return dict(zip(INFO_NAMES, (t.cpu() for t in out)))


@pytest.mark.parametrize("case", INFO_CASES)
@pytest.mark.parametrize("shape", INFO_SHAPES)
def test_joint_info_against_the_statement(shape, case):
    bad = []
    for rw in (False, True):
        if case == "axis" and rw:                   # (exactly on an axis is an fp32 statement only where the extrinsics are exact: the syn rig)
            continue
        sc = points_scene(shape, case, rw)
        args = (sc["rec"], sc["ctm"], sc["sx"], sc["sy"])
        f64 = IS.information(sc["points"].double(), sc["conf"].double(), *args)
        f32 = IS.information(sc["points"], sc["conf"], *args)
        got = info_launch(sc)
        print(f"{shape} {case} {'ctm' if rw else 'syn'}: views {sorted(set(f64['views'].flatten().tolist()))}, {int(f64['valid'].sum())} of "
              f"{shape[0] * shape[2]} matrices valid")
        assert torch.equal(got["views"], f64["views"]), (shape, case, rw)
        assert torch.equal(got["valid"].bool(), f64["valid"]), (shape, case, rw)
        for name in ("info", "sigma"):
            assert bool(torch.isfinite(got[name]).all()), (shape, case, rw, name)
            err, allowed = FS.yardstick(name, got[name], f32[name], f64[name])
            if not err <= allowed:
                bad.append((shape, case, rw, name, err, allowed))
        none = f64["views"] == 0                                                        # no view: exact zeros
        assert float(got["info"][none].abs().sum()) == 0.0 and float(got["sigma"][~f64["valid"]].abs().sum()) == 0.0
        if case == "axis":
            assert int((f64["views"] < shape[1]).sum()) == shape[0]                     # the joint on an axis lost exactly that view
        if case == "nan":
            assert int(none.sum()) > 0
    assert not bad, bad


@pytest.mark.parametrize("shape", INFO_SHAPES)
def test_what_is_planted_in_an_excluded_view_reaches_no_output(shape):
    B, V, J = shape
    values = torch.tensor([float("nan"), float("inf"), float("-inf"), 3.0e38, -1.0e30])
    sc = points_scene(shape, "emptied", True)
    conf, ctm = sc["conf"].clone(), sc["ctm"].clone()
    conf[0, V - 1, :] = 0.1                                                             # a whole view of a frame excluded: its matrix is not read
    clean = info_launch(sc, conf=conf)
    planted_ctm = ctm.clone()
    planted_ctm[0, V - 1] = values[torch.randint(0, 5, (4, 4), generator=torch.Generator().manual_seed(3))]
    excluded = ~((conf >= 0.5) & (conf > 0))
    planted_conf = conf.clone()
    planted_conf[excluded] = torch.tensor([float("nan"), 0.0, -1.0, 0.49, float("-inf")])[torch.randint(0, 5, conf.shape, generator=torch.Generator().manual_seed(4))][excluded]
    assert int(excluded.sum()) > 0
    dirty = info_launch(sc, conf=planted_conf, ctm=planted_ctm)
    for name in INFO_NAMES:
        assert bool(torch.isfinite(dirty[name].float()).all()), (shape, name)
        assert torch.equal(clean[name], dirty[name]), (shape, name)
    nan = points_scene(shape, "nan", False)                                             # what stands in a point that is not finite
    other = nan["points"].clone()
    broken = ~torch.isfinite(other).all(-1)
    other[broken] = torch.tensor([float("inf"), 1.0, float("nan")])
    for a, b in zip(info_launch(nan).values(), info_launch(nan, points=other).values()):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------- the smoother

def scene(shape, case, rw):
    if (shape, case, rw) not in _SCENES:
        N, T, J = shape
        _SCENES[shape, case, rw] = IS.scene(N, T, 2 + (T + J) % 3, J, case, rw)
    return _SCENES[shape, case, rw]


def reference(shape, case, rw, lam, mode, gap):
    """The statement in float64 and float32 on the case's fp32 operands, computed once and shared (never modified); "f32" is the float64
    one where the float32 evaluation does not factor or is not finite: its own deviation is then 0 and the floor alone holds."""
    key = (shape, case, rw, lam, mode, gap)
    if key not in _REFS:
        sc = scene(shape, case, rw)
        kw = dict(lv=lam[0], la=lam[1], huber=mode[0], reweights=mode[1], max_gap=gap)
        f64 = IS.fit(sc["pose"], sc["info"], sc["obs"], **kw)
        f32 = IS.try_fit(sc["pose"], sc["info"], sc["obs"], dt=torch.float32, **kw)
        _REFS[key] = {"f64": f64, "f32": f64 if f32 is None else f32, "f32_failed": f32 is None}
    return _REFS[key]


def launch(sc, lam, mode, gap, pose=None, info=None):
    from egorear_amd import hip
    out = hip.info_track(dev(sc["pose"] if pose is None else pose), dev(sc["info"] if info is None else info), dev(sc["obs"]), lam[0], lam[1],
                         mode[0], mode[1], gap)
    torch.cuda.synchronize()
    return dict(zip(NAMES, (t.cpu() for t in out)))


def combos(shape):
    """(lambda, mode, max_gap, rw): every pair of penalties meets every mode on the small shapes; the clip of 64 frames, whose dense
    float64 and float32 statements take a second a solve, meets every penalty once and every mode."""
    N, T, J = shape
    every = list(itertools.product(LAMBDAS, MODES))
    if N * T * J > 1000:
        every = [(LAMBDAS[i], MODES[i % 3]) for i in range(4)]
    return [(lam, mode, (0, 3, T)[(i + i // 3) % 3], bool((i + i // 3) % 2)) for i, (lam, mode) in enumerate(every)]


@pytest.mark.parametrize("case", IS.CASES)
@pytest.mark.parametrize("shape", SHAPES)
def test_info_track_against_the_statement(shape, case):
    N, T, J = shape
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
        for name in OUTPUTS:
            assert bool(torch.isfinite(got[name]).all()), (shape, case, rw, lam, mode, name)
            err, allowed = FS.yardstick(name, got[name], ref["f32"][name], f64[name])
            if not err <= allowed:
                bad.append((shape, case, rw, lam, mode, name, err, allowed))
        dead = ~f64["ok"]                                                              # a track that is not solvable gives zeros
        assert float(got["pose"].transpose(1, 2)[dead].abs().sum()) == 0.0 and float(got["energy"][dead].abs().sum()) == 0.0
        for name in ("residual", "weight"):
            assert float(got[name].transpose(1, 2)[dead].abs().sum()) == 0.0
        assert not bool(got["valid"].transpose(1, 2)[dead].any())
        unused = ~IS.used_frames(sc["pose"], sc["info"], sc["obs"])
        assert float(got["residual"][unused].abs().sum()) == 0.0 and float(got["weight"][unused].abs().sum()) == 0.0
    assert not bad, bad


@pytest.mark.parametrize("shape", [(2, 4, 15), (5, 9, 13), (3, 64, 15)])
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
def test_what_is_planted_in_a_frame_that_is_not_used_reaches_no_output(shape):
    values = torch.tensor([float("nan"), float("inf"), float("-inf"), 3.0e38, -1.0e30, 0.0, 7.0])
    planted = 0
    for rw in (False, True):
        sc = scene(shape, "gaps", rw)
        gap = sc["obs"] == 0                                                            # (a frame with obs = 1 is read: that is how it is refused)
        planted += int(gap.sum())                                                       # (the one frame of (1, 1, 1) is a gap on one rig only)
        pose, info = sc["pose"].clone(), sc["info"].clone()
        pose[gap] = values[torch.randint(0, 7, pose.shape, generator=torch.Generator().manual_seed(3))][gap]
        info[gap] = values[torch.randint(0, 7, info.shape, generator=torch.Generator().manual_seed(4))][gap]
        for lam, mode in ((LAMBDAS[0], MODES[0]), (LAMBDAS[2], MODES[2]), (LAMBDAS[1], MODES[1])):
            clean, dirty = launch(sc, lam, mode, 3), launch(sc, lam, mode, 3, pose=pose, info=info)
            for name in NAMES:
                assert bool(torch.isfinite(dirty[name].float()).all()), (shape, rw, lam, mode, name)
                assert torch.equal(clean[name], dirty[name]), (shape, rw, lam, mode, name)
    assert planted > 0


def test_bits_do_not_depend_on_the_batch_the_run_or_a_graph_replay():
    from egorear_amd import hip
    for case, rw, lam, mode in (("gaps", False, (0.0, 10.0), (0.0, 0)), ("glitch", True, (0.5, 100.0), (1.0, 4)), ("oneview", True, (1.0, 0.0), (0.0, 0))):
        sc = scene((3, 64, 15), case, rw)
        z, w, o = dev(sc["pose"]), dev(sc["info"]), dev(sc["obs"])
        run = lambda zz, ww, oo: hip.info_track(zz, ww, oo, lam[0], lam[1], mode[0], mode[1], 3)
        cut = lambda t, n: None if t is None else t[n:n + 1].contiguous()
        eager, again = run(z, w, o), run(z, w, o)
        for a, b in zip(eager, again):
            assert torch.equal(a, b)
        for n in range(3):                                                             # a clip alone and inside the batch of three
            for a, b in zip(eager, run(cut(z, n), cut(w, n), cut(o, n))):
                assert torch.equal(a[n:n + 1], b)
        torch.cuda.synchronize()
        static = z.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                                  # one stream, no parallel branches
            out = run(static, w, o)
        static.copy_(torch.zeros_like(z))
        graph.replay()
        static.copy_(z)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, out):
            assert torch.equal(a, b)
        assert bool(eager[1].any()) and float(eager[4].max()) > 0.0
    # ---- the matrix: a frame alone and inside the batch, twice, and replayed
    sc = points_scene((64, 4, 16), "emptied", True)
    p, f, r, m = dev(sc["points"]), dev(sc["conf"]), dev(sc["rec"]), dev(sc["ctm"])
    run = lambda pp, ff, mm: hip.joint_info(pp, ff, r, mm, sc["sx"], sc["sy"], 0.5, 1e-6)
    eager, again = run(p, f, m), run(p, f, m)
    for a, b in zip(eager, again):
        assert torch.equal(a, b)
    for b_ in (0, 31, 63):
        for a, b in zip(eager, run(p[b_:b_ + 1].contiguous(), f[b_:b_ + 1].contiguous(), m[b_:b_ + 1].contiguous())):
            assert torch.equal(a[b_:b_ + 1], b)
    torch.cuda.synchronize()
    static = p.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(static, f, m)
    static.copy_(torch.zeros_like(p))
    graph.replay()
    static.copy_(p)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(a, b)
    assert bool(eager[3].any())


@pytest.fixture(scope="module")
def clip_maps():
    """Gaussian bumps (sigma 1, 64 x 64) at the projections of a moving 15-joint skeleton, N = 2 clips of T = 6 frames, V = 4, on the syn
    rig; a few joints lose three of their views for a frame or two: the triangulation gives those frames up and the smoothers fill them."""
    g = torch.Generator().manual_seed(91)
    cams = FS.rig()
    rec = FS.records(cams)
    pts = TS.motion(2, 6, 15, g)
    hm = FS.bumps(pts.view(12, 15, 3), rec, None, FS.HM, FS.HM).float().view(2, 6, 4, 15, FS.HM, FS.HM).contiguous()
    lost = ((0, 2, 3), (0, 3, 3), (1, 0, 7), (1, 5, 14), (0, 4, 0))
    for n, t, j in lost:
        hm[n, t, 1:, j] = 0.0
    return {"cams": cams, "pts": pts, "hm": hm, "lost": lost}


def test_decode_clip_3d_info_is_its_five_launches(clip_maps):
    from egorear_amd import decode, hip
    hm, cams = clip_maps["hm"].to(DEV), clip_maps["cams"]
    kw = dict(accel_weight=2.0, vel_weight=0.05, huber_px=1.0, reweights=2, max_gap=2)
    decode.decode_clip_3d_info(hm, cams, linearise_accel_weight=5.0, **kw)             # (warms the record cache)
    hip.PROFILE = []
    try:
        joints, coarse, fine = decode.decode_clip_3d_info(hm, cams, linearise_accel_weight=5.0, **kw)
        torch.cuda.synchronize()
        names = [e[0] for e in hip.PROFILE]
    finally:
        hip.PROFILE = None
    assert names == ["egr_soft_argmax_f32", "egr_triangulate_f32", "egr_trajectory_smooth_f32", "egr_joint_info_f32", "egr_info_track_f32"], names
    # the first two results are decode_clip_3d's with the same arguments
    old_joints, old_track = decode.decode_clip_3d(hm, cams, accel_weight=5.0, max_gap=2)
    for a, b in zip(joints, old_joints):
        assert torch.equal(a, b)
    for a, b in zip(coarse, old_track):
        assert torch.equal(a, b)
    # the pieces, called one by one
    j3, j2 = decode.decode_joints_3d(hm.view(12, 4, 15, FS.HM, FS.HM), cams)
    smooth = decode.smooth_trajectory(j3.pose.view(2, 6, 15, 3), None, j3.valid.view(2, 6, 15), 5.0, 0.0, 0.0, 0, 2)
    information = decode.joint_information(smooth.pose.reshape(12, 15, 3), j2.maxvals, cams, None, (FS.HM, FS.HM))
    by_hand = decode.smooth_trajectory_info(j3.pose.view(2, 6, 15, 3), information.info.view(2, 6, 15, 6), j3.valid.view(2, 6, 15), **kw)
    for a, b in zip(fine, by_hand):
        assert torch.equal(a, b)
    for a, b in zip(coarse, smooth):
        assert torch.equal(a, b)
    assert fine.pose.shape == (2, 6, 15, 3) and fine.residual.shape == fine.weight.shape == (2, 6, 15) and fine.energy.shape == (2, 15)
    assert fine.valid.dtype == torch.bool and information.views.dtype == torch.uint8 and information.valid.dtype == torch.bool
    for n, t, j in clip_maps["lost"]:                                                  # one view is no triangulated point: a gap, filled
        assert not bool(joints.valid[n, t, j]) and bool(fine.valid[n, t, j]) and float(fine.weight[n, t, j]) == 0.0
        assert int(information.views.view(2, 6, 15)[n, t, j]) == 1
    err = (fine.pose.double().cpu() - clip_maps["pts"]).norm(dim=-1)
    old = (coarse.pose.double().cpu() - clip_maps["pts"]).norm(dim=-1)
    print(f"mean error {float(err.mean()):.4e} cm (the linearisation track {float(old.mean()):.4e}), at the filled frames "
          f"{[round(float(err[i]), 4) for i in clip_maps['lost']]}")
    assert bool(torch.isfinite(err).all())
    one = decode.decode_clip_3d_info(hm[1], cams, linearise_accel_weight=5.0, **kw)    # (T, V, J, H, W): one clip, the same bits
    assert one[2].pose.shape == (6, 15, 3) and one[0].pose.shape == (6, 15, 3) and one[2].energy.shape == (15,)
    for got, want in zip(one, (joints, coarse, fine)):
        for a, b in zip(got, want):
            assert torch.equal(a, b[1])
    alone = decode.smooth_trajectory_info(j3.pose.view(2, 6, 15, 3)[1], information.info.view(2, 6, 15, 6)[1], j3.valid.view(2, 6, 15)[1], **kw)
    for a, b in zip(alone, fine):
        assert torch.equal(a, b[1])


def test_inputs_that_require_grad_give_outputs_that_do_not(clip_maps):
    from egorear_amd import decode
    sc = scene((2, 4, 15), "dense", True)
    z, w = dev(sc["pose"]).requires_grad_(), dev(sc["info"]).requires_grad_()
    for kw in ({}, {"huber_px": 1.0, "reweights": 2}):
        track = decode.smooth_trajectory_info(z, w, **kw)
        assert not any(t.requires_grad for t in track)
        with pytest.raises(RuntimeError):
            track.pose.sum().backward()
    ps = points_scene((3, 4, 15), "every", True)
    got = decode.joint_information(dev(ps["points"]).requires_grad_(), dev(ps["conf"]).requires_grad_(), ps["cams"], dev(ps["ctm"]).requires_grad_())
    assert not any(t.requires_grad for t in got)
    with pytest.raises(RuntimeError):
        got.info.sum().backward()
    maps = clip_maps["hm"].to(DEV).requires_grad_()
    joints, coarse, fine = decode.decode_clip_3d_info(maps, clip_maps["cams"])
    assert joints.pose.requires_grad and coarse.pose.requires_grad and not any(t.requires_grad for t in fine)


def test_bad_launches_are_refused():
    from egorear_amd import decode, hip
    sc = scene((2, 4, 15), "dense", False)
    z, w = dev(sc["pose"]), dev(sc["info"])
    good = dict(vel_weight=0.0, accel_weight=1.0, huber=0.0, reweights=0, max_gap=8, min_pivot_ratio=1e-10)
    for kw in ({"vel_weight": -1.0}, {"accel_weight": 0.0}, {"huber": 1.0}, {"reweights": 2}, {"huber": 1.0, "reweights": 17}, {"max_gap": -1},
               {"accel_weight": float("nan")}, {"min_pivot_ratio": 1.0}):
        with pytest.raises(ValueError):
            hip.info_track(z, w, None, **dict(good, **kw))
    with pytest.raises(ValueError):
        hip.info_track(z, w[:, :3], None, **good)
    with pytest.raises(ValueError):
        hip.info_track(z.transpose(0, 1), w.transpose(0, 1), None, **good)
    with pytest.raises(ValueError):
        hip.info_track(z, w, torch.ones(2, 4, 14, dtype=torch.uint8, device=DEV), **good)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.info_track(z.cpu(), w.cpu(), None, **good)
    ps = points_scene((3, 4, 15), "every", False)
    p, f, r = dev(ps["points"]), dev(ps["conf"]), dev(ps["rec"])
    for kw in ({"sx": 0.0}, {"threshold": float("nan")}, {"min_det_ratio": -1.0}):
        with pytest.raises(ValueError):
            hip.joint_info(p, f, r, None, **dict(dict(sx=ps["sx"], sy=ps["sy"], threshold=0.5, min_det_ratio=1e-6), **kw))
    with pytest.raises(ValueError):
        hip.joint_info(p, f[:, :3], r, None)
    with pytest.raises(ValueError):
        hip.joint_info(p, f, r[:3], None)
    with pytest.raises(ValueError):
        hip.joint_info(p[:, :14], f, r, None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.joint_info(p.cpu(), f.cpu(), r.cpu(), None)
    with pytest.raises(ValueError, match="no CPU path"):
        decode.smooth_trajectory_info(z.cpu(), w.cpu())

"""The temporal trajectory smoother on the GPU (egr_trajectory_smooth_f32, egr_trajectory_smooth_bwd_f32, egorear_amd/decode.py,
DESIGN.md 5s) against the float64 statement of tests/trajectory_statement.py.

Yardstick: fisheye_statement's - a HIP output may deviate from the float64 statement (on the same fp32 operands) by at most MARGIN = 8 x
the deviation of the float32 evaluation of that statement, with a floor of 4 ulp (fp32) of the output's largest magnitude.  Where the
float32 evaluation does not factor or is not finite the floor alone holds; the kernel eliminates in fp64 and can meet it.  cond(A) of
every case used is computed on the CPU and held below 1e10.

The binding check of the plain form is independent of the solver: at the returned fp32 pose  g = A x - W z  in float64 must satisfy
|g_i| <= MARGIN * sum_k |A_ik| * ulp32(max |x| of the track)  for every component of every solvable track - rounding the exact
minimiser to fp32 costs up to half that sum (the float64 statement rounded to fp32 measures 0.49 of it on the CPU)."""
import itertools

import pytest
import torch

import fisheye_statement as FS
import trajectory_statement as TS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = FS.MARGIN
# (N, T, J): the band is narrower than five where T < 5; 64 / 65 sit at a wave-length boundary of the time axis; 257 is the long chain
SHAPES = [(1, 1, 1), (2, 2, 3), (1, 3, 2), (2, 4, 15), (1, 5, 16), (3, 64, 15), (1, 65, 16), (2, 257, 5)]
LAMBDAS = [(0.0, 10.0), (1.0, 0.0), (0.5, 100.0), (0.0, 1000.0)]          # (lambda_v, lambda_a)
MODES = [(0.0, 0), (1.0, 1), (1.0, 4)]                                     # (huber, K)
OUTPUTS = ("pose", "residual", "weight", "energy")
_SCENES, _REFS, _COND = {}, {}, {}


def scene(shape, case):
    if (shape, case) not in _SCENES:
        _SCENES[shape, case] = TS.scene(*shape, case)
    return _SCENES[shape, case]


def reference(shape, case, lam, mode, gap):
    """The statement in float64 and float32 on the case's fp32 operands, computed once and shared (never modified); "f32" is the float64
    one where the float32 evaluation does not factor or is not finite: its own deviation is then 0 and the floor alone holds."""
    key = (shape, case, lam, mode, gap)
    if key not in _REFS:
        sc = scene(shape, case)
        f64 = TS.smooth(sc["pose"], sc["weight"], sc["obs"], lam[0], lam[1], mode[0], mode[1], gap)
        f32 = TS.try_smooth(sc["pose"], sc["weight"], sc["obs"], lam[0], lam[1], mode[0], mode[1], gap, dt=torch.float32)
        _REFS[key] = {"f64": f64, "f32": f64 if f32 is None else f32, "f32_failed": f32 is None}
    return _REFS[key]


def condition(shape, case, lam):
    if (shape, case, lam) not in _COND:
        sc = scene(shape, case)
        _COND[shape, case, lam] = TS.condition(sc["pose"], sc["weight"], sc["obs"], lam[0], lam[1])
    return _COND[shape, case, lam]


def dev(t):
    return None if t is None else t.to(DEV)


def launch(sc, lam, mode, gap):
    from egorear_amd import hip
    out = hip.trajectory_smooth(dev(sc["pose"]), dev(sc["weight"]), dev(sc["obs"]), lam[0], lam[1], mode[0], mode[1], gap)
    torch.cuda.synchronize()
    return dict(zip(("pose", "valid", "residual", "weight", "energy"), (t.cpu() for t in out)))


def held(bad, tag, name, got, ref):
    err, allowed = FS.yardstick(name, got, ref["f32"][name], ref["f64"][name])
    if not err <= allowed:
        bad.append(tag + (name, err, allowed))
    return allowed


@pytest.mark.parametrize("case", TS.CASES)
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_statement_and_stationary(shape, case):
    sc = scene(shape, case)
    N, T, J = shape
    bad = []
    for i, (lam, mode) in enumerate(itertools.product(LAMBDAS, MODES)):
        gap = (0, 3, T)[(i + i // 3) % 3]                                              # every lambda and every mode meets every max_gap
        cond = condition(shape, case, lam)
        ref = reference(shape, case, lam, mode, gap)
        got = launch(sc, lam, mode, gap)
        f64 = ref["f64"]
        print(f"{shape} {case} lambda {lam} huber {mode[0]} K {mode[1]} max_gap {gap}: cond(A) {cond:.3e}, {int(f64['ok'].sum())} of {N * J} "
              f"tracks solvable, {int(f64['valid'].sum())} of {N * T * J} frames valid{', float32 evaluation failed' if ref['f32_failed'] else ''}")
        assert cond <= 1e10, (shape, case, lam, cond)
        assert torch.equal(got["valid"].bool(), f64["valid"]), (shape, case, lam, mode, gap)
        for name in OUTPUTS:
            assert bool(torch.isfinite(got[name]).all()), (shape, case, lam, mode, name)
            held(bad, (shape, case, lam, mode), name, got[name], ref)
        dead = ~f64["ok"]                                                              # a track that is not solvable gives zeros
        for name in ("pose", "residual", "weight"):
            assert float(got[name].transpose(1, 2)[dead].abs().sum()) == 0.0
        assert float(got["energy"][dead].abs().sum()) == 0.0 and not bool(got["valid"].transpose(1, 2)[dead].any())
        unseen = TS.base_weights(sc["pose"], sc["weight"], sc["obs"])[0] == 0
        assert float(got["residual"][unseen].abs().sum()) == 0.0 and float(got["weight"][unseen].abs().sum()) == 0.0
        if mode[1] == 0:
            g, allowed, _ = TS.stationarity(got["pose"], sc["weight"], sc["obs"], sc["pose"], lam[0], lam[1])
            worst = g.abs().amax(-1)
            ratio = float(torch.where(allowed > 0, worst / allowed.clamp_min(1e-300), torch.zeros_like(worst)).max())
            own = TS.stationarity(f64["pose"].float(), sc["weight"], sc["obs"], sc["pose"], lam[0], lam[1])
            own_ratio = float(torch.where(own[1] > 0, own[0].abs().amax(-1) / own[1].clamp_min(1e-300), torch.zeros_like(worst)).max())
            print(f"    stationarity: largest |g_i| / allowance {ratio:.3g} (statement rounded to fp32: {own_ratio:.3g})")
            if not bool((worst <= MARGIN * allowed).all()):
                bad.append((shape, case, lam, "stationarity", ratio, MARGIN))
    assert not bad, bad


@pytest.mark.parametrize("shape", SHAPES)
def test_hubers_energy_does_not_increase_with_the_rounds(shape):
    sc = scene(shape, "glitch")
    bad = []
    for lam in LAMBDAS:
        before = None
        for mode in ((0.0, 0), (1.0, 1), (1.0, 2), (1.0, 4)):                          # K = 0: the plain solve, whose rho is the square >= Huber's
            ref = reference(shape, "glitch", lam, mode, 8)
            got = launch(sc, lam, mode, 8)
            allowed = held(bad, (shape, "glitch", lam, mode), "energy", got["energy"], ref)
            print(f"{shape} lambda {lam} K {mode[1]}: energy {float(got['energy'].double().sum()):.6f} (statement {float(ref['f64']['energy'].sum()):.6f})")
            if before is not None and not bool((got["energy"].double() <= before[0].double() + before[1] + allowed).all()):
                bad.append((shape, lam, mode, "energy rose", before[0].tolist(), got["energy"].tolist()))
            before = (got["energy"], allowed)
    assert not bad, bad


@pytest.mark.parametrize("shape", SHAPES)
def test_what_is_planted_in_a_gap_reaches_no_output(shape):
    sc = scene(shape, "nonfinite")
    for lam, mode in itertools.product(LAMBDAS, MODES):
        got, twin = launch(sc, lam, mode, 3), launch(sc["twin"], lam, mode, 3)
        for name in OUTPUTS + ("valid",):
            assert bool(torch.isfinite(got[name].float()).all()), (shape, lam, mode, name)
            assert torch.equal(got[name], twin[name]), (shape, lam, mode, name)


@pytest.mark.parametrize("case", ["dense", "gaps", "mask"])
@pytest.mark.parametrize("shape", SHAPES)
def test_gradients_of_the_plain_form(shape, case):
    from egorear_amd import decode
    sc = scene(shape, case)
    g_pose = torch.randn(sc["pose"].shape, generator=torch.Generator().manual_seed(17))
    bad = []
    for lam in LAMBDAS:
        grads = {}
        for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
            p = sc["pose"].detach().clone().to(dt).requires_grad_()               # (a leaf of its own: the scene is shared)
            w = None if sc["weight"] is None else sc["weight"].detach().clone().to(dt).requires_grad_()
            try:
                out = TS.smooth(p, w, sc["obs"], lam[0], lam[1], dt=dt)
                (out["pose"] * g_pose.to(dt)).sum().backward()
                grads[name] = {"g_pose": p.grad, "g_weight": None if w is None else w.grad}
                if not all(bool(torch.isfinite(v).all()) for v in grads[name].values() if v is not None):
                    grads[name] = grads["f64"]
            except RuntimeError:                                                       # (float32 only: float64 factors every case used)
                assert name == "f32"
                grads[name] = grads["f64"]
        p = dev(sc["pose"]).requires_grad_()
        w = None if sc["weight"] is None else dev(sc["weight"]).requires_grad_()
        track = decode.smooth_trajectory(p, w, dev(sc["obs"]), accel_weight=lam[1], vel_weight=lam[0])
        (track.pose * g_pose.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        print(f"{shape} {case} lambda {lam}:")
        for name, got in (("g_pose", p.grad), ("g_weight", None if w is None else w.grad)):
            if got is None:
                continue
            assert bool(torch.isfinite(got).all())
            err, allowed = FS.yardstick(name, got, grads["f32"][name], grads["f64"][name])
            if not err <= allowed:
                bad.append((shape, case, lam, name, err, allowed))
        ok = reference(shape, case, lam, (0.0, 0), 8)["f64"]["ok"]
        assert float(p.grad.cpu().transpose(1, 2)[~ok].abs().sum()) == 0.0             # a track that is not solvable gives zeros
    assert not bad, bad


def test_the_backward_of_the_huber_form_raises():
    from egorear_amd import decode
    sc = scene((2, 4, 15), "glitch")
    p, w = dev(sc["pose"]).requires_grad_(), dev(sc["weight"]).requires_grad_()
    track = decode.smooth_trajectory(p, w, None, huber_cm=1.0, reweights=2)
    assert not any(t.requires_grad for t in track)
    with pytest.raises(RuntimeError):
        track.pose.sum().backward()
    with pytest.raises(RuntimeError):
        track.energy.sum().backward()
    plain = decode.smooth_trajectory(p, w, None)                                      # the plain form's side outputs carry no gradient either
    assert plain.pose.requires_grad and not plain.residual.requires_grad and not plain.energy.requires_grad


def test_bits_do_not_depend_on_the_batch_the_run_or_a_graph_replay():
    from egorear_amd import hip
    for case, lam, mode in (("gaps", (0.0, 10.0), (0.0, 0)), ("glitch", (0.5, 100.0), (1.0, 4)), ("mask", (1.0, 0.0), (0.0, 0))):
        sc = scene((3, 64, 15), case)
        p, w, o = dev(sc["pose"]), dev(sc["weight"]), dev(sc["obs"])
        run = lambda pp, ww, oo: hip.trajectory_smooth(pp, ww, oo, lam[0], lam[1], mode[0], mode[1], 3)
        cut = lambda t, n: None if t is None else t[n:n + 1].contiguous()
        eager, again = run(p, w, o), run(p, w, o)
        for a, b in zip(eager, again):
            assert torch.equal(a, b)
        for n in range(3):                                                             # a clip alone and inside the batch of three
            for a, b in zip(eager, run(cut(p, n), cut(w, n), cut(o, n))):
                assert torch.equal(a[n:n + 1], b)
        if mode[1] == 0:
            g = torch.randn(p.shape, generator=torch.Generator().manual_seed(2)).to(DEV)
            first, second = hip.trajectory_smooth_bwd(p, w, o, g, lam[0], lam[1]), hip.trajectory_smooth_bwd(p, w, o, g, lam[0], lam[1])
            alone = hip.trajectory_smooth_bwd(cut(p, 1), cut(w, 1), cut(o, 1), cut(g, 1), lam[0], lam[1])
            for a, b, c in zip(first, second, alone):
                assert (a is None and b is None and c is None) or (torch.equal(a, b) and torch.equal(a[1:2], c))
        torch.cuda.synchronize()
        static = p.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                                  # one stream, no parallel branches
            out = run(static, w, o)
        static.copy_(torch.zeros_like(p))
        graph.replay()
        static.copy_(p)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, out):
            assert torch.equal(a, b)
        assert bool(eager[1].any()) and float(eager[4].min()) > 0.0


@pytest.fixture(scope="module")
def clip_maps():
    """Gaussian bumps (sigma 1, 64 x 64) at the projections of a moving 15-joint skeleton, N = 2 clips of T = 6 frames, V = 4, on the syn
    rig; a few joints lose three of their views for a frame or two, which the triangulation gives up."""
    g = torch.Generator().manual_seed(91)
    cams = FS.rig()
    rec = FS.records(cams)
    pts = TS.motion(2, 6, 15, g)
    hm = FS.bumps(pts.view(12, 15, 3), rec, None, FS.HM, FS.HM).float().view(2, 6, 4, 15, FS.HM, FS.HM).contiguous()
    for n, t, j in ((0, 2, 3), (0, 3, 3), (1, 0, 7), (1, 5, 14), (0, 4, 0)):
        hm[n, t, 1:, j] = 0.0
    return {"cams": cams, "pts": pts, "hm": hm, "lost": ((0, 2, 3), (0, 3, 3), (1, 0, 7), (1, 5, 14), (0, 4, 0))}


def test_decode_clip_3d_is_its_three_launches(clip_maps):
    from egorear_amd import decode, hip
    hm, cams = clip_maps["hm"].to(DEV), clip_maps["cams"]
    kw = dict(accel_weight=10.0, vel_weight=0.5, huber_cm=1.0, reweights=2, max_gap=2)
    decode.decode_clip_3d(hm, cams, **kw)                                              # (warms the record cache)
    hip.PROFILE = []
    try:
        joints, track = decode.decode_clip_3d(hm, cams, **kw)
        torch.cuda.synchronize()
        names = [e[0] for e in hip.PROFILE]
    finally:
        hip.PROFILE = None
    assert names == ["egr_soft_argmax_f32", "egr_triangulate_f32", "egr_trajectory_smooth_f32"], names
    # the pieces, called one by one
    flat, _ = decode.decode_joints_3d(hm.view(12, 4, 15, FS.HM, FS.HM), cams)
    by_hand = decode.smooth_trajectory(flat.pose.view(2, 6, 15, 3), None, flat.valid.view(2, 6, 15), **kw)
    for a, b in zip(track, by_hand):
        assert torch.equal(a, b)
    for a, b in zip(joints, flat):
        assert torch.equal(a.reshape(b.shape), b)
    assert joints.pose.shape == (2, 6, 15, 3) and joints.residual.shape == (2, 6, 4, 15) and track.valid.dtype == torch.bool
    for n, t, j in clip_maps["lost"]:                                                  # the holes of the triangulation are filled
        assert not bool(joints.valid[n, t, j]) and bool(track.valid[n, t, j]) and float(track.weight[n, t, j]) == 0.0
    err = (track.pose.double().cpu() - clip_maps["pts"]).norm(dim=-1)
    print(f"mean error {float(err.mean()):.4e} cm, in the filled holes {[round(float(err[i]), 4) for i in clip_maps['lost']]}")
    assert bool(torch.isfinite(err).all())
    one_j, one_t = decode.decode_clip_3d(hm[1], cams, **kw)                            # (T, V, J, H, W): one clip, the same bits
    assert one_t.pose.shape == (6, 15, 3) and torch.equal(one_t.pose, track.pose[1]) and torch.equal(one_j.valid, joints.valid[1])
    # in the plain form a temporal loss reaches the heat maps through the three backward operators
    maps = hm.clone().requires_grad_()
    _, plain = decode.decode_clip_3d(maps, cams, max_gap=2)
    (plain.pose[:, 2:] - 2.0 * plain.pose[:, 1:-1] + plain.pose[:, :-2]).square().sum().backward()
    assert bool(torch.isfinite(maps.grad).all()) and float(maps.grad.abs().max()) > 0.0


def test_bad_launches_are_refused():
    from egorear_amd import hip
    sc = scene((2, 4, 15), "dense")
    p, w = dev(sc["pose"]), dev(sc["weight"])
    for kw in ({"vel_weight": -1.0}, {"accel_weight": 0.0}, {"huber": 1.0}, {"reweights": 2}, {"huber": 1.0, "reweights": 17}, {"max_gap": -1},
               {"accel_weight": float("nan")}):
        with pytest.raises(ValueError):
            hip.trajectory_smooth(p, w, None, **dict(dict(vel_weight=0.0, accel_weight=10.0, huber=0.0, reweights=0, max_gap=8), **kw))
    with pytest.raises(ValueError):
        hip.trajectory_smooth(p, w[:, :3], None)
    with pytest.raises(ValueError):
        hip.trajectory_smooth(p.transpose(1, 2), None, None)

"""The bone-length-constrained skeleton fit on the GPU (egr_skeleton_fit_f32, egr_bone_lengths_f32, egr_skeleton_resize_f32,
egorear_amd/decode.py) against the statements of tests/skeleton_statement.py.

Yardstick: fisheye_statement's - a HIP output may deviate from the float64 statement (on the same fp32 inputs) by at most MARGIN = 8 x
the deviation of the float32 evaluation of that statement, with a floor of 4 ulp (fp32) of the output's largest magnitude.

The binding check is solver-independent: at the returned fp32 pose the float64 gradient g and exact Hessian H of the energy (autograd of
the three sums) must satisfy |g_i| <= MARGIN * sum_k |H_ik| * ulp32(max |pose|) for every active component - rounding the exact minimiser
to fp32 costs up to sum_k |H_ik| * ulp32 / 2.

ITERATIONS is the smallest multiple of 16 at which the float64 statement, rounded to fp32, meets an eighth of that allowance on the CPU
for every (shape, case, lambda) below: 176.  Most need 16 or 32; the slow ones are on the 15-joint scene at lambda = 10 - `nonfinite`
176, `free_bones` 144, `one_view` 128 (112 at lambda = 1) - where Gauss-Newton converges linearly: what it drops of a bone's curvature,
tension / length, is not small against the rays' stiffness along the viewing direction."""
import pytest
import torch

import fisheye_statement as FS
import skeleton_statement as SS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = FS.MARGIN
ITERATIONS = 176
# (B, V, J, rw, chain): the 15-joint tree; a chain on the front pair; one bone; the 16-joint tree on rw with per-frame lengths; no bone
SHAPES = [(3, 4, 15, False, False), (2, 2, 5, False, True), (1, 3, 2, False, False), (2, 4, 16, True, False), (1, 4, 1, False, False)]
BONED = SHAPES[:4]
_SCENES, _REFS = {}, {}


def scene(shape):
    if shape not in _SCENES:
        _SCENES[shape] = SS.scene(*shape)
    return _SCENES[shape]


def reference(shape, case, lam, iterations=ITERATIONS):
    """The statement in float64 and float32 on the case's fp32 operands, computed once and shared (never modified)."""
    key = (shape, case, lam, iterations)
    if key not in _REFS:
        sc = scene(shape)
        ops = SS.case_operands(sc, case)
        ref = {"ops": ops}
        for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
            pr = SS.problem(sc, ops, lam, dt)
            out, E0, grad, steps = SS.fit_statement(pr, iterations)
            out.update(energy0=E0, grad=grad, steps=steps)
            ref[name], ref["pr_" + name] = out, pr
        _REFS[key] = ref
    return _REFS[key]


def launch(shape, ops, lam, iterations=ITERATIONS):
    from egorear_amd import hip
    sc = scene(shape)
    ctm = None if sc["ctm"] is None else sc["ctm"].to(DEV)
    out = hip.skeleton_fit(ops["coords"].to(DEV), ops["conf"].to(DEV), sc["rec"].to(DEV), ctm, sc["parents"], ops["bone_length"].to(DEV),
                           ops["init"].to(DEV), ops["init_ok"].to(DEV), 1.0 / SS.HM, 1.0 / SS.HM, FS.THR, FS.MIN_DET, lam, ops["rho"], iterations)
    torch.cuda.synchronize()
    return dict(zip(("pose", "ray_cost", "bone", "valid", "energy0", "energy", "grad", "steps"), (t.cpu() for t in out)))


@pytest.mark.parametrize("case", SS.CASES)
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_statement_and_stationary(shape, case):
    bad = []
    for lam in SS.LAMBDAS:
        ref = reference(shape, case, lam)
        got = launch(shape, ref["ops"], lam)
        f64, f32, pr = ref["f64"], ref["f32"], ref["pr_f64"]
        print(f"{shape} {case} lambda {lam}: {int(f64['valid'].sum())} joints, {int(f64['bone_on'].sum())} bones, steps {got['steps'].tolist()} "
              f"(statement {f64['steps'].tolist()})")
        assert torch.equal(got["valid"].bool(), f64["valid"]), (shape, case, lam)
        assert torch.equal(got["bone"] > 0, f64["bone_on"]), (shape, case, lam)
        # (at lambda = 0 a joint that only its bone keeps in the fit is free along its one ray: every point of the ray minimises, and
        # where on it a run ends is rounding - its pose and the bones that touch it are compared nowhere, its ray_cost everywhere)
        fixed = torch.ones_like(f64["valid"]) if lam > 0.0 or ref["ops"]["rho"] > 0.0 else (pr.w > 0).sum(1) >= 2
        fixed_bone = fixed & fixed[:, list(scene(shape)["parents"])]
        for name in ("pose", "ray_cost", "bone", "energy0", "energy"):
            keep = {"pose": fixed.unsqueeze(-1), "bone": fixed_bone}.get(name)
            pick = (lambda t: t) if keep is None else (lambda t: torch.where(keep, t, torch.zeros_like(t)))
            err, allowed = FS.yardstick(name, pick(got[name]), pick(f32[name]), pick(f64[name]))
            if not err <= allowed:
                bad.append((shape, case, lam, name, err, allowed))
        # stationarity of the returned pose, and the kernel's own report of it
        ratio, g, m, allowed = SS.stationarity(pr, got["pose"])
        zero = torch.zeros_like(g)
        gmax, room = torch.where(m, g.abs(), zero).amax(1), torch.where(m, allowed, zero).amax(1)
        off = float(((got["grad"].double() - gmax).abs() - room).max())
        print(f"    stationarity: largest |g_i| / allowed {ratio:.3g} (statement rounded to fp32: "
              f"{SS.stationarity(pr, f64['pose'].float())[0]:.3g}); grad output {got['grad'].tolist()} against {gmax.tolist()}")
        if not ratio <= 1.0:
            bad.append((shape, case, lam, "stationarity", ratio, 1.0))
        if not off <= 0.0:
            bad.append((shape, case, lam, "grad", got["grad"].tolist(), gmax.tolist()))
        monotone(shape, ref["ops"], lam, got)
        dead = ~got["valid"].bool()
        assert float(got["pose"][dead].abs().sum()) == 0.0 and float(got["ray_cost"][dead].abs().sum()) == 0.0
        assert float(got["bone"][dead].abs().sum()) == 0.0 and float(got["bone"][:, 0].abs().sum()) == 0.0
        seen = (pr.w > 0).any(1)
        assert float(got["ray_cost"][~seen].abs().sum()) == 0.0
        for b in range(shape[0]):
            if not bool(got["valid"][b].any()):                                       # a frame without an active joint gives zeros
                assert float(got["energy0"][b]) == float(got["energy"][b]) == float(got["grad"][b]) == 0.0 and int(got["steps"][b]) == 0
    assert not bad, bad


def monotone(shape, ops, lam, got):
    """The issue's monotone check, made without the kernel's energy outputs: the three sums in float64 at the returned pose and at the
    start.  The kernel keeps no step that raises E at its fp64 point p; the pose is p rounded to fp32, which moves every coordinate by
    at most h = ulp32(max |pose|) / 2 and E by at most  sum_i |g_i| h + sum_ik |H_ik| h^2 / 2  (g and the exact H are taken at the
    pose, not at p: twice that is allowed).  Then the outputs themselves: energy0 and energy against those sums, energy <= energy0 up
    to an fp32 ulp (the two sums round on their own), and a pose that moved exactly where steps were kept."""
    pr = SS.problem(scene(shape), ops, lam, torch.float64)
    start, pose = pr.start(), got["pose"].double()
    E_start, E_pose = SS.energy(pr, start)[0], SS.energy(pr, pose)[0]
    g, H = SS.grad_hess(pr, pose)
    h = FS.ulp32(float(pose.abs().max())) / 2.0
    cost = 2.0 * (g.abs().sum(1) * h + 0.5 * H.abs().sum((1, 2)) * h * h)
    print(f"    E(start) {E_start.tolist()} -> E(pose) {E_pose.tolist()} (float64 at the returned pose; rounding may cost {cost.tolist()}), "
          f"outputs {got['energy0'].tolist()} -> {got['energy'].tolist()}, steps {got['steps'].tolist()}")
    assert bool((E_pose <= E_start + cost).all()), (shape, lam, E_start.tolist(), E_pose.tolist())
    ulp0 = torch.tensor([FS.ulp32(float(e)) for e in E_start], dtype=torch.float64)
    ulp1 = torch.tensor([FS.ulp32(float(e)) for e in E_pose], dtype=torch.float64)
    assert bool(((got["energy0"].double() - E_start).abs() <= 4.0 * ulp0).all())
    assert bool(((got["energy"].double() - E_pose).abs() <= cost + 4.0 * ulp1).all())
    assert bool((got["energy"].double() <= got["energy0"].double() + ulp0).all())
    moved, kept = (pose != start).flatten(1).any(1), got["steps"] > 0
    downhill = SS.gauss_newton_system(pr, start)[0].abs().amax((1, 2)) > 1e-3         # (a joint that only its prior holds starts at rest)
    assert not bool((moved & ~kept).any())                                            # no kept step: the pose is the init, bit for bit
    assert not bool((kept & downhill & ~moved).any())                                 # a kept step moved it
    assert bool((E_pose < E_start)[kept & downhill].all())                            # and lowered E


@pytest.mark.parametrize("shape", SHAPES)
def test_the_energy_never_increases_even_after_one_iteration(shape):
    for case, lam in (("full", 10.0), ("one_view", 1.0), ("unseen_prior", 1.0), ("nonfinite", 10.0)):
        ops = SS.case_operands(scene(shape), case)
        for iterations in (1, 3, 16):
            got = launch(shape, ops, lam, iterations)
            print(f"{shape} {case} lambda {lam}, {iterations} iteration(s):")
            monotone(shape, ops, lam, got)
            assert bool((got["steps"] <= iterations).all())
            assert bool(torch.isfinite(got["pose"]).all()) and bool(torch.isfinite(got["energy"]).all())
            if iterations == 1 and bool(got["valid"].any()) and case != "unseen_prior":
                # 3 cm off, mu = 1e-3: the first step is nearly the Gauss-Newton step and must be kept, in every frame with a joint
                assert bool((got["steps"][got["valid"].bool().any(1)] == 1).all())


@pytest.mark.parametrize("shape", SHAPES)
def test_without_bones_and_prior_it_is_the_triangulation(shape):
    from egorear_amd import hip
    sc = scene(shape)
    bad = []
    for case in ("full", "one_view", "nonfinite"):
        ops = SS.case_operands(sc, case)
        got = launch(shape, ops, 0.0)
        ctm = None if sc["ctm"] is None else sc["ctm"].to(DEV)
        pts, cost, _, ok = (t.cpu() for t in hip.triangulate(ops["coords"].to(DEV), ops["conf"].to(DEV), sc["rec"].to(DEV), ctm, 1.0 / SS.HM,
                                                             1.0 / SS.HM, FS.THR, FS.MIN_DET))
        keep = ok.bool() & ops["init_ok"].bool() & torch.isfinite(ops["init"]).all(-1)
        assert int(keep.sum()) > 0 or shape[2] <= 2
        assert bool(got["valid"].bool()[keep].all())
        f64 = FS.statement(ops["coords"].double(), ops["conf"].double(), sc["rec"], sc["ctm"], 1.0 / SS.HM, 1.0 / SS.HM)
        f32 = FS.statement(ops["coords"], ops["conf"], sc["rec"], sc["ctm"], 1.0 / SS.HM, 1.0 / SS.HM)
        print(f"{shape} {case}: {int(keep.sum())} triangulated joints")
        if int(keep.sum()) == 0:
            continue
        for name, mine, theirs, i in (("pose", got["pose"], pts, 0), ("ray_cost", got["ray_cost"], cost, 1)):
            for what, value in (("fit", mine), ("triangulate", theirs)):                # both launches against the one statement
                err, allowed = FS.yardstick(f"{name} ({what})", value[keep], f32[i][keep], f64[i][keep])
                if not err <= allowed:
                    bad.append((shape, case, name, what, err, allowed))
            err = float((mine.double() - theirs.double())[keep].abs().max())
            _, allowed = FS.yardstick(f"{name} (fit against triangulate)", mine[keep], f32[i][keep], f64[i][keep])
            if not err <= allowed:
                bad.append((shape, case, name, "difference", err, allowed))
    assert not bad, bad


@pytest.mark.parametrize("shape", BONED)
def test_a_joint_one_camera_sees_is_placed(shape):
    """Why the fit exists: the triangulation has nothing for a joint with one view; the fit places it by its ray and its bone, as close
    to the true point as the Newton referee gets on the same inputs, from the init, like the fit.  The ray meets the bone's sphere
    twice: in a frame where the two algorithms end in different minima (printed when it happens) the referee is run again from the
    statement's result, so that it referees the minimum the fit is in."""
    from egorear_amd import hip
    sc = scene(shape)
    leaf = SS.limb_joint(sc["parents"])
    for lam in (1.0, 10.0):
        ref = reference(shape, "one_view", lam)
        ops = ref["ops"]
        ctm = None if sc["ctm"] is None else sc["ctm"].to(DEV)
        ok = hip.triangulate(ops["coords"].to(DEV), ops["conf"].to(DEV), sc["rec"].to(DEV), ctm, 1.0 / SS.HM, 1.0 / SS.HM, FS.THR, FS.MIN_DET)[3]
        assert int(ok[:, leaf].sum()) == 0
        got = launch(shape, ops, lam)
        assert bool(got["valid"][:, leaf].all())
        pr = ref["pr_f64"]
        referee, gmax = SS.newton_referee(pr)
        parted = (referee - ref["f64"]["pose"]).abs().flatten(1).amax(1) > 1e-3
        if bool(parted.any()):           # another minimum: say so, and referee the basin the fit is in (the 15-joint scene at lambda 10)
            print(f"{shape} lambda {lam}: from the init the referee ends in another minimum in frames {parted.nonzero().flatten().tolist()}: "
                  f"E {SS.energy(pr, referee)[0].tolist()} against the statement's {ref['f64']['energy'].tolist()}")
            again, gmax2 = SS.newton_referee(pr, ref["f64"]["pose"])
            referee, gmax = torch.where(parted.view(-1, 1, 1), again, referee), torch.where(parted, gmax2, gmax)
        assert float(gmax.max()) < 1e-10
        truth = sc["pts"][:, leaf]
        mine = (got["pose"][:, leaf].double() - truth).norm(dim=-1)
        theirs = (referee[:, leaf] - truth).norm(dim=-1)
        err, allowed = FS.yardstick("the one-view joint", got["pose"][:, leaf], ref["f32"]["pose"][:, leaf], referee[:, leaf])
        print(f"{shape} lambda {lam}: distance from the true joint: fit {mine.tolist()} cm, referee {theirs.tolist()} cm")
        assert err <= allowed and bool((mine <= theirs + allowed).all())


def test_bits_do_not_depend_on_the_batch_the_run_or_a_graph_replay():
    from egorear_amd import hip
    shape = SHAPES[0]
    sc = scene(shape)
    ops = SS.case_operands(sc, "one_view")
    rec, L = sc["rec"].to(DEV), ops["bone_length"].to(DEV)
    c, w, q, k = ops["coords"].to(DEV), ops["conf"].to(DEV), ops["init"].to(DEV), ops["init_ok"].to(DEV)
    run = lambda cc, ww, qq, kk: hip.skeleton_fit(cc, ww, rec, None, sc["parents"], L, qq, kk, 1.0 / SS.HM, 1.0 / SS.HM, FS.THR, FS.MIN_DET, 10.0,
                                                  1e-3, 48)
    eager, again = run(c, w, q, k), run(c, w, q, k)
    for a, b in zip(eager, again):
        assert torch.equal(a, b)
    for f in range(3):                                                               # a frame alone and inside the batch of three
        one = run(c[f:f + 1].contiguous(), w[f:f + 1].contiguous(), q[f:f + 1].contiguous(), k[f:f + 1].contiguous())
        for a, b in zip(eager, one):
            assert torch.equal(a[f:f + 1], b)
    torch.cuda.synchronize()
    static = c.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                    # one stream, no parallel branches
        out = run(static, w, q, k)
    static.copy_(torch.zeros_like(c))
    graph.replay()
    static.copy_(c)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(a, b)
    assert int(eager[7].min()) > 0 and float(eager[4].min()) > 0.0


@pytest.mark.parametrize("B", [1, 7])
def test_the_small_launches_against_their_statements(B):
    from egorear_amd import hip
    g = torch.Generator().manual_seed(50 + B)
    parents = SS.parents_15()
    pts, lengths = SS.random_skeleton(B, 15, parents, g)
    pose = (pts + 0.8 * torch.randn(B, 15, 3, generator=g, dtype=torch.float64)).float()
    valid = (torch.rand(B, 15, generator=g) < 0.85).to(torch.uint8)
    valid[:, 14] = 0                                                                 # a bone that is never valid
    valid[B - 1, :8] = 1
    valid[B - 1, 2] = 0                                                              # and a frame whose invalid joint is mid-chain
    L = lengths.float()
    L[5] = 0.0                                                                       # one bone without a length keeps its vector
    length, spread, count = (t.cpu() for t in hip.bone_lengths(pose.to(DEV), valid.to(DEV), parents))
    l64, s64, c64 = SS.bone_lengths_statement(pose.double(), valid, parents)
    l32, s32, _ = SS.bone_lengths_statement(pose, valid, parents)
    assert torch.equal(count, c64) and int(count[14]) == 0 and float(length[14]) == 0.0 and float(length[0]) == 0.0
    bad = []
    for name, got, f32, f64 in (("length", length, l32, l64), ("spread", spread, s32, s64)):
        err, allowed = FS.yardstick(name, got, f32, f64)
        if not err <= allowed:
            bad.append((name, err, allowed))
    for table in (L, L.expand(B, 15).contiguous()):
        out = hip.skeleton_resize(pose.to(DEV), valid.to(DEV), table.to(DEV), parents).cpu()
        err, allowed = FS.yardstick("resize", out, SS.resize_statement(pose, valid, table, parents),
                                    SS.resize_statement(pose.double(), valid, table.double(), parents))
        if not err <= allowed:
            bad.append(("resize", err, allowed))
        keep = (valid == 0) | (valid[:, list(parents)] == 0)
        keep[:, 0] = True
        assert torch.equal(out[keep], pose[keep])                                     # they keep their place, bit for bit
        assert torch.equal(out[B - 1, 2], pose[B - 1, 2]) and torch.equal(out[B - 1, 4], pose[B - 1, 4])      # joint 4 hangs on joint 2
        # every rescaled bone has its length: each of the child's three coordinates rounds by half an ulp32 of the pose's largest
        # magnitude at most, which moves the length by less than one such ulp - 4 are allowed
        used = ~keep & (L > 0).unsqueeze(0)
        got_len = (out.double() - out.double()[:, list(parents)]).norm(dim=-1)
        off = float((got_len - L.double().unsqueeze(0))[used].abs().max())
        print(f"B {B}: {int(used.sum())} rescaled bones, largest |length - L| {off:.3e} cm, 4 ulp32 {4 * FS.ulp32(float(out.abs().max())):.3e}")
        assert int(used.sum()) > 0 and off <= 4 * FS.ulp32(float(out.abs().max()))
    assert torch.equal(hip.bone_lengths(pose.to(DEV), valid.to(DEV), parents)[0].cpu(), length)               # the same bits again
    assert not bad, bad


@pytest.fixture(scope="module")
def bump_maps():
    """Gaussian bumps (sigma 1, 64 x 64) at the projections of a 15-joint skeleton, B = 2, V = 4, on the syn rig (the fixture style of
    test_gpu_triangulate.bump_maps)."""
    g = torch.Generator().manual_seed(78)
    cams = FS.rig()
    rec = FS.records(cams)
    pts, lengths = SS.random_skeleton(2, 15, SS.parents_15(), g)
    return {"cams": cams, "rec": rec, "pts": pts, "lengths": lengths.float(), "hm": FS.bumps(pts, rec, None, SS.HM, SS.HM).float().contiguous()}


def test_decode_joints_3d_skeleton_on_rendered_bumps(bump_maps):
    from egorear_amd import decode, hip
    hm, cams, pts, L = bump_maps["hm"].to(DEV), bump_maps["cams"], bump_maps["pts"], bump_maps["lengths"].to(DEV)
    fit, tri, j2 = decode.decode_joints_3d_skeleton(hm, cams, L, iterations=48)
    plain, _ = decode.decode_joints_3d(hm, cams)
    torch.cuda.synchronize()
    assert fit.pose.shape == (2, 15, 3) and fit.valid.dtype == torch.bool and bool(fit.valid.all()) and torch.equal(tri.pose, plain.pose)
    # the three calls made by hand
    coords, maxvals, _, _, _, _ = hip.soft_argmax(hm, 100.0, 0, False, 0.5)
    coords, maxvals = coords.view(2, 4, 15, 2), maxvals.view(2, 4, 15)
    rec = bump_maps["rec"].to(DEV)
    p3, _, _, ok = hip.triangulate(coords, maxvals, rec, None, 1.0 / SS.HM, 1.0 / SS.HM, 0.5, 1e-6)
    by_hand = hip.skeleton_fit(coords, maxvals, rec, None, SS.parents_15(), L, p3, ok, 1.0 / SS.HM, 1.0 / SS.HM, 0.5, 1e-6, 1.0, 0.0, 48)
    for a, b in zip(fit, by_hand):
        assert torch.equal(a.view(torch.uint8) if a.dtype == torch.bool else a, b)
    keep = fit.valid.cpu()
    e_fit = float((fit.pose.double().cpu() - pts).norm(dim=-1)[keep].mean())
    e_tri = float((plain.pose.double().cpu() - pts).norm(dim=-1)[keep].mean())
    print(f"mean error over {int(keep.sum())} joints: decode_joints_3d {e_tri:.4e} cm, decode_joints_3d_skeleton {e_fit:.4e} cm; "
          f"energy {fit.energy0.tolist()} -> {fit.energy.tolist()}")
    assert e_fit <= e_tri
    # with a caller's init that leaves a joint out, that joint starts from the triangulated point
    init, init_ok = (tri.pose + 1.0).detach(), torch.ones(2, 15, dtype=torch.bool, device=DEV)
    init_ok[0, 3] = False
    mixed, _, _ = decode.decode_joints_3d_skeleton(hm, cams, L, init, init_ok, iterations=48)
    start = torch.where(init_ok.unsqueeze(-1), init, tri.pose)
    want = hip.skeleton_fit(coords, maxvals, rec, None, SS.parents_15(), L, start, torch.ones(2, 15, dtype=torch.uint8, device=DEV),
                            1.0 / SS.HM, 1.0 / SS.HM, 0.5, 1e-6, 1.0, 0.0, 48)
    assert torch.equal(mixed.pose, want[0]) and bool(mixed.valid.all())


def test_bad_launches_are_refused():
    from egorear_amd import hip
    sc = scene(SHAPES[2])
    ops = SS.case_operands(sc, "full")
    args = lambda **kw: dict(dict(parents=[0, 0], lam=1.0, rho=0.0, iterations=16), **kw)
    for kw in (args(parents=[0, 1]), args(parents=[1, 0]), args(lam=-1.0), args(rho=float("nan")), args(iterations=0), args(iterations=257)):
        with pytest.raises(ValueError):
            hip.skeleton_fit(ops["coords"].to(DEV), ops["conf"].to(DEV), sc["rec"].to(DEV), None, kw["parents"], ops["bone_length"].to(DEV),
                             ops["init"].to(DEV), ops["init_ok"].to(DEV), 1.0 / SS.HM, 1.0 / SS.HM, FS.THR, FS.MIN_DET, kw["lam"], kw["rho"],
                             kw["iterations"])

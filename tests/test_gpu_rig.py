"""The rig self-calibration on the GPU (egr_rig_refine_f32, egorear_amd/decode.py refine_rig / apply_rig_correction / calibrate_rig,
DESIGN.md 5t) against the statement of tests/rig_statement.py.

Yardstick: fisheye_statement's - a HIP output may deviate from the float64 statement (on the same fp32 inputs) by at most MARGIN = 8 x
the deviation of the float32 evaluation of that statement, with a floor of 4 ulp (fp32) of the output's largest magnitude.

The binding check is solver-independent: at the rotations the returned fp32 matrices encode, the float64 gradient g and exact Hessian H
of the reduced objective (autograd, the point of every pair eliminated in closed form) must satisfy |g_i| <= MARGIN * sum_k |H_ik| *
ulp32(1.0) for every free component - the matrices are what the decoders consume, and they are rounded at the scale of 1.

ITERATIONS is the smallest count at which the float64 statement, rounded to fp32, meets an eighth of that allowance on the CPU for
every (shape, case) below: 7.  The noise-free cases need 3 (Gauss-Newton converges quadratically where the rays can meet); with
0.1 px of noise the residuals do not vanish and the convergence is linear - (5, 2, 4) `noisy` needs 7, (1, 4, 15) `noisy` 5, the other
`noisy` and the `prior` cases 4."""
import pytest
import torch

import fisheye_statement as FS
import rig_statement as RS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = FS.MARGIN
ITERATIONS = 7
SHAPES = RS.SHAPES
_CASES, _REFS = {}, {}


def case(shape, name):
    if (shape, name) not in _CASES:
        _CASES[shape, name] = RS.case(shape, name)
    return _CASES[shape, name]


def reference(shape, name):
    """The statement in float64 and float32 on the case's fp32 operands, computed once and shared (never modified)."""
    if (shape, name) not in _REFS:
        sc, ops = case(shape, name)
        ref = {}
        for key, dt in (("f64", torch.float64), ("f32", torch.float32)):
            pr = RS.problem(sc, ops, dt)
            out = RS.refine_statement(pr, ITERATIONS)
            out["ctm"] = RS.apply_correction_f64(out["matrix"].double(), sc["rec"], sc["ctm"], True).expand(shape[0], shape[1], 4, 4)
            ref[key], ref["pr_" + key] = out, pr
        _REFS[shape, name] = ref
    return _REFS[shape, name]


def launch(sc, ops, iterations=ITERATIONS, ctm="own"):
    from egorear_amd import decode
    ctm = sc["ctm"] if isinstance(ctm, str) else ctm
    fit = decode.refine_rig(ops["coords"].to(DEV), ops["conf"].to(DEV), sc["cams"], None if ctm is None else ctm.to(DEV), (RS.HM, RS.HM),
                            FS.THR, FS.MIN_DET, ops["fixed"], ops["prior_weight"], iterations)
    torch.cuda.synchronize()
    return fit._replace(**{n: getattr(fit, n).cpu() for n in fit._fields})


@pytest.mark.parametrize("name", RS.CASES)
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_statement_and_stationary(shape, name):
    B, V, J, rw = shape
    sc, ops = case(shape, name)
    ref = reference(shape, name)
    f64, f32, pr = ref["f64"], ref["f32"], ref["pr_f64"]
    got = launch(sc, ops)
    print(f"{shape} {name}: {f64['pairs']} pairs, valid {f64['valid']}, steps {int(got.steps)} (statement {f64['steps']}), RMS ray distance "
          f"{RS.rms_cm(got.cost0):.3e} -> {RS.rms_cm(got.cost):.3e} cm, grad {float(got.grad):.3e}")
    assert bool(got.valid) == f64["valid"] == f32["valid"] and int(got.pairs) == f64["pairs"] == f32["pairs"]
    assert got.pairs.dtype == got.steps.dtype == torch.int32 and got.valid.dtype == torch.bool
    bad = []
    for what, mine in (("rotation", got.rotation), ("matrix", got.matrix), ("ctm", got.coord_trans_mat), ("cost0", got.cost0), ("cost", got.cost)):
        err, allowed = FS.yardstick(what, mine, torch.as_tensor(f32[what]), torch.as_tensor(f64[what] if what != "matrix" else f64["dR"]))
        if not err <= allowed:
            bad.append((what, err, allowed))
    nominal = RS.apply_correction(torch.eye(3).expand(V, 3, 3).contiguous(), sc["rec"], sc["ctm"], B)
    if not f64["valid"]:                                                              # `nothing`: identities, the given rig, zeros
        assert name == "nothing"
        assert float(got.rotation.abs().max()) == 0.0 and torch.equal(got.matrix, torch.eye(3).expand(V, 3, 3))
        assert torch.equal(got.coord_trans_mat, nominal)
        assert float(got.cost0) == float(got.cost) == float(got.grad) == 0.0 and int(got.steps) == int(got.pairs) == 0
        assert not bad, bad
        return
    assert name != "nothing" and 0 <= int(got.steps) <= ITERATIONS
    assert float(got.cost) <= float(got.cost0) and bool(torch.isfinite(got.coord_trans_mat).all())
    held = pr.fixed
    assert float(got.rotation[held].abs().max()) == 0.0 and torch.equal(got.matrix[held], torch.eye(3).expand(int(held.sum()), 3, 3))
    assert torch.equal(got.coord_trans_mat[:, held], nominal[:, held])

    # solver-independent: stationary at the returned matrices; the kernel's own report of it; no worse than the given rig
    ratio, g, allowed, free = RS.stationarity(pr, got.matrix)
    at_statement = RS.stationarity(pr, f64["matrix"])[0]
    print(f"    stationarity: largest |g_i| / allowed {ratio:.3g} (statement rounded to fp32: {at_statement:.3g})")
    if not ratio <= 1.0:
        bad.append(("stationarity", ratio, 1.0))
    if bool(free.any()):
        gmax, room = float(g[free].abs().max()), float(allowed[free].max())
        print(f"    grad output {float(got.grad):.3e} against the float64 gradient at the fp32 matrices {gmax:.3e} (rounding room {room:.3e})")
        if not abs(float(got.grad) - gmax) <= room:
            bad.append(("grad", float(got.grad), gmax))
    else:
        assert float(got.grad) == 0.0
    zero = torch.zeros(V, 3, dtype=torch.float64)
    E_id, E_got = float(pr.objective(zero)), float(pr.objective(zero, got.matrix.double()))
    _, H = pr.grad_hess(got.matrix.double())
    h = FS.ulp32(1.0) / 2.0                                                           # the rounding of the matrices: half an ulp of 1 a component
    cost = 2.0 * float((g.abs() * free).sum() * h + 0.5 * (H.abs() * free.unsqueeze(0) * free.unsqueeze(1)).sum() * h * h)
    print(f"    E(identity) {E_id:.6e} -> E(returned matrices) {E_got:.6e} (float64; rounding may cost {cost:.3e})")
    if not E_got <= E_id + cost:
        bad.append(("objective", E_got, E_id))

    if name == "calibrated":                                                          # nothing to find: the rotations stay at the rounding
        _, allowed = FS.yardstick("rotation (calibrated, against 0)", got.rotation, f32["rotation"], torch.zeros(V, 3))
        assert float(got.rotation.abs().max()) <= max(allowed, MARGIN * FS.ulp32(1.0))
    if name in ("rotated", "emptied"):                                                # the truth is recovered
        err = float((got.rotation.double() - sc["vec"]).abs().max())
        own = float((f64["rotation"] - sc["vec"]).abs().max())
        print(f"    max |rotation - truth| {err:.3e} rad (statement {own:.3e})")
        assert err <= MARGIN * max(own, FS.ulp32(0.03))
    if name == "all_fixed":
        assert int(got.steps) == 0 and float(got.cost) == float(got.cost0) > 0.0 and float(got.rotation.abs().max()) == 0.0
    assert not bad, bad


@pytest.mark.parametrize("shape", SHAPES)
def test_two_runs_are_bit_identical(shape):
    for name in ("rotated", "emptied", "noisy"):
        sc, ops = case(shape, name)
        a, b = launch(sc, ops), launch(sc, ops)
        for field in a._fields:
            assert torch.equal(getattr(a, field), getattr(b, field)), (shape, name, field)
        short = launch(sc, ops, 1)
        assert int(short.steps) <= 1 and float(short.cost) <= float(short.cost0) and float(short.cost0) == float(a.cost0)


def test_one_rig_for_the_clip_is_the_same_rig_in_every_frame():
    shape = (40, 4, 3, True)
    sc, ops = case(shape, "rotated")
    one = sc["ctm"][:1].contiguous()
    ops1 = dict(ops)
    a = launch(sc, ops1, ctm=one)
    b = launch(sc, ops1, ctm=one.expand(shape[0], 4, 4, 4).contiguous())
    for field in a._fields:
        assert torch.equal(getattr(a, field), getattr(b, field)), field
    assert a.coord_trans_mat.shape == (40, 4, 4, 4) and bool(a.valid)


@pytest.mark.parametrize("shape", SHAPES)
def test_the_corrected_rig_serves_the_decoders(shape):
    """The point of the feature: on `rotated`, `triangulate_joints` with the returned coord_trans_mat gives the statement's triangulation
    on those matrices, and a cost below the nominal rig's; `apply_rig_correction` does the same for other frames of the same rig."""
    from egorear_amd import decode
    B, V, J, rw = shape
    sc, ops = case(shape, "rotated")
    got = launch(sc, ops)
    bad = []

    def served(clip, coords, conf, corrected, nominal):
        tri = decode.triangulate_joints(coords.to(DEV), conf.to(DEV), sc["cams"], corrected.to(DEV))
        plain = decode.triangulate_joints(coords.to(DEV), conf.to(DEV), sc["cams"], None if nominal is None else nominal.to(DEV))
        f64 = FS.statement(coords.double(), conf.double(), sc["rec"], corrected, 1.0 / RS.HM, 1.0 / RS.HM)
        f32 = FS.statement(coords, conf, sc["rec"], corrected, 1.0 / RS.HM, 1.0 / RS.HM)
        assert torch.equal(tri.valid.cpu(), f64[3]) and bool(f64[3].all())
        for what, mine, i in (("pose", tri.pose, 0), ("cost", tri.cost, 1)):
            err, allowed = FS.yardstick(f"{clip} {what}", mine, f32[i], f64[i])
            if not err <= allowed:
                bad.append((clip, what, err, allowed))
        before, after = float(plain.cost.double().mean()), float(tri.cost.double().mean())
        miss = float((tri.pose.cpu().double() - pts).norm(dim=-1).mean()), float((plain.pose.cpu().double() - pts).norm(dim=-1).mean())
        print(f"    {clip}: mean cost {before:.3e} -> {after:.3e} cm^2, mean joint error {miss[1]:.3e} -> {miss[0]:.3e} cm")
        assert after < before and miss[0] < miss[1]

    pts = sc["pts"]
    served("the clip", ops["coords"], ops["conf"], got.coord_trans_mat, sc["ctm"])
    B2 = max(2, B // 2)
    nxt = RS.more_frames(sc, B2, 4242)
    pts = nxt["pts"]
    corrected = decode.apply_rig_correction(got.matrix.to(DEV), sc["cams"], None if nxt["ctm"] is None else nxt["ctm"].to(DEV), B2).cpu()
    assert torch.equal(corrected, RS.apply_correction(got.matrix, sc["rec"], nxt["ctm"], B2))
    # the kernel's composition and torch's give the same bits: fp32 times fp32 is exact in float64, three products added in index order
    mine = None if sc["ctm"] is None else sc["ctm"].to(DEV)
    assert torch.equal(decode.apply_rig_correction(got.matrix.to(DEV), sc["cams"], mine, B).cpu(), got.coord_trans_mat)
    served("the next clip", nxt["coords"], nxt["conf"], corrected, nxt["ctm"])
    assert not bad, bad


def test_calibrate_rig_is_the_two_calls():
    from egorear_amd import decode
    shape = (6, 4, 15, False)
    sc, ops = case(shape, "rotated")
    hm = FS.bumps(sc["pts"], sc["rec"], sc["true"].expand(6, 4, 4, 4), RS.HM, RS.HM).float().to(DEV)
    fit, j2 = decode.calibrate_rig(hm, sc["cams"], iterations=ITERATIONS)
    two = decode.decode_joints_2d(hm)
    again = decode.refine_rig(two.soft, two.maxvals, sc["cams"], iterations=ITERATIONS)
    torch.cuda.synchronize()
    for a, b in zip(tuple(fit) + tuple(j2), tuple(again) + tuple(two)):
        assert torch.equal(a, b)
    err = float((fit.rotation.cpu().double() - sc["vec"]).abs().max())
    print(f"calibrate_rig on sigma-1 bumps: RMS ray distance {RS.rms_cm(fit.cost0.cpu()):.3e} -> {RS.rms_cm(fit.cost.cpu()):.3e} cm, "
          f"max |rotation - truth| {err:.3e} rad, steps {int(fit.steps)}")
    assert bool(fit.valid) and int(fit.pairs) == 90 and float(fit.cost) < float(fit.cost0)

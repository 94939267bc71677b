"""CPU-side checks of the rig self-calibration (egorear_amd/decode.py refine_rig / apply_rig_correction / calibrate_rig):
the operator is registered with a fake implementation and no gradient, the public functions give the documented shapes and dtypes on
meta tensors, `calibrate_rig` traces under Dynamo as one graph, bad arguments and CPU tensors are refused before any launch, the library
exports the entry and refuses bad arguments itself - and the statement of tests/rig_statement.py, which the GPU test compares the kernels
with, is itself held to known answers here."""
import ctypes

import pytest
import torch

import fisheye_statement as FS
import rig_statement as RS

# (B, V, J, rw) of test_gpu_rig.py
META_SHAPES = tuple(RS.SHAPES)
FIELDS = ("rotation", "matrix", "coord_trans_mat", "cost0", "cost", "pairs", "steps", "grad", "valid")


def _meta(B, V, J, rw, clip=False):
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)
    return {"coords": m(B, V, J, 2), "conf": m(B, V, J), "cams": m(V, 30), "ctm": m(1 if clip else B, V, 4, 4) if rw else None}


def _op(decode, a, fixed=None, **kw):
    args = dict(sx=1 / 64, sy=1 / 64, threshold=0.5, min_det_ratio=1e-6, prior_weight=0.0, iterations=8)
    args.update(kw)
    V = a["coords"].shape[1]
    fixed = [int(v == 0) for v in range(V)] if fixed is None else fixed
    return decode.rig_refine_op(a["coords"], a["conf"], a["cams"], a["ctm"], fixed, args["sx"], args["sy"], args["threshold"],
                                args["min_det_ratio"], args["prior_weight"], args["iterations"])


def test_the_operator_is_registered_with_a_fake_implementation_and_no_gradient():
    from egorear_amd import decode
    assert hasattr(torch.ops.egorear_amd, "rig_refine")
    for B, V, J, rw in META_SHAPES:
        for clip in (False, True):
            a = _meta(B, V, J, rw, clip)
            a["coords"].requires_grad_()
            a["conf"].requires_grad_()
            out = _op(decode, a)
            rotation, matrix, ctm, cost0, cost, pairs, steps, grad, valid = out
            assert rotation.shape == (V, 3) and matrix.shape == (V, 3, 3) and ctm.shape == (B, V, 4, 4)
            assert cost0.shape == cost.shape == pairs.shape == steps.shape == grad.shape == valid.shape == (1,)
            assert pairs.dtype == steps.dtype == torch.int32 and valid.dtype == torch.uint8
            assert all(t.dtype == torch.float32 for t in (rotation, matrix, ctm, cost0, cost, grad))
            assert not any(t.requires_grad for t in out)


def test_public_functions_give_the_documented_shapes_on_meta():
    from egorear_amd import decode
    cams = FS.rig()
    for B, V, J, rw in META_SHAPES:
        for clip in (False, True):
            a = _meta(B, V, J, rw, clip)
            for kw in ({}, {"fixed": [True] * V}, {"fixed": torch.tensor([True] + [False] * (V - 1))}, {"prior_weight": 10.0, "iterations": 3}):
                fit = decode.refine_rig(a["coords"], a["conf"], cams[:V], a["ctm"], **kw)
                assert isinstance(fit, decode.RigFit) and fit._fields == FIELDS
                assert fit.rotation.shape == (V, 3) and fit.matrix.shape == (V, 3, 3) and fit.coord_trans_mat.shape == (B, V, 4, 4)
                assert all(getattr(fit, n).shape == () for n in FIELDS[3:])
                assert fit.pairs.dtype == fit.steps.dtype == torch.int32 and fit.valid.dtype == torch.bool
                assert all(getattr(fit, n).dtype == torch.float32 for n in ("rotation", "matrix", "coord_trans_mat", "cost0", "cost", "grad"))
            again = decode.apply_rig_correction(fit.matrix, cams[:V], a["ctm"], B)
            assert again.shape == (B, V, 4, 4) and again.dtype == torch.float32
            assert decode.apply_rig_correction(fit.matrix, cams[:V], a["ctm"], 1 if clip or not rw else B).shape[1:] == (V, 4, 4)
            hm = torch.empty(B, V, J, 64, 64, device="meta")
            fit2, j2 = decode.calibrate_rig(hm, cams[:V], a["ctm"], iterations=4)
            assert isinstance(fit2, decode.RigFit) and isinstance(j2, decode.Joints2D)
            assert fit2.coord_trans_mat.shape == (B, V, 4, 4) and j2.soft.shape == (B, V, J, 2)
            # the corrected matrices are what every decoder takes
            assert decode.triangulate_joints(a["coords"], a["conf"], cams[:V], fit.coord_trans_mat).pose.shape == (B, J, 3)


def test_calibrate_rig_traces_as_one_graph():
    import torch._dynamo as dynamo
    from egorear_amd import decode
    lin = torch.nn.Conv2d(4, 15, 1, device="meta")
    cams = FS.rig()

    def serving_side(feat):
        hm = lin(feat).view(2, 4, 15, 64, 64)
        fit, j2 = decode.calibrate_rig(hm, cams, iterations=6)
        pose = decode.triangulate_joints(j2.soft, j2.maxvals, cams, fit.coord_trans_mat).pose
        return fit.rotation, fit.valid, pose

    feat = torch.empty(8, 4, 64, 64, device="meta")
    rotation, valid, pose = serving_side(feat)                # (also warms the record cache: the upload is not part of a graph)
    assert rotation.shape == (4, 3) and not rotation.requires_grad and valid.dtype == torch.bool and pose.shape == (2, 15, 3)
    dynamo.reset()
    ex = dynamo.explain(serving_side)(feat)
    assert ex.graph_break_count == 0 and ex.graph_count == 1, ex
    targets = [str(nd.target) for g in ex.graphs for nd in g.graph.nodes if nd.op == "call_function"]
    for name in ("egorear_amd.soft_argmax", "egorear_amd.rig_refine", "egorear_amd.triangulate"):
        assert sum(name in t for t in targets) == 1, (name, targets)


def test_bad_arguments_are_refused_before_any_launch():
    from egorear_amd import decode
    cams = FS.rig()
    a = _meta(2, 4, 5, False)
    decode.refine_rig(a["coords"], a["conf"], cams)
    for kw in ({"fixed": [True, False, False]}, {"fixed": [True] * 5}, {"fixed": [0.5, 0, 0, 0]}, {"fixed": [2, 0, 0, 0]}, {"fixed": "tfff"},
               {"fixed": torch.tensor([True, False])}, {"fixed": torch.zeros(4)}, {"prior_weight": -1.0}, {"prior_weight": float("nan")},
               {"prior_weight": float("inf")}, {"iterations": 0}, {"iterations": -3}, {"iterations": 257}, {"iterations": 8.0},
               {"iterations": True}, {"min_det_ratio": -1.0}, {"heatmap_size": (0, 64)}):
        with pytest.raises(ValueError):
            decode.refine_rig(a["coords"], a["conf"], cams, **kw)
        if "heatmap_size" not in kw:
            with pytest.raises(ValueError):
                decode.calibrate_rig(torch.empty(2, 4, 5, 16, 16, device="meta"), cams, **kw)
        if "fixed" not in kw and "heatmap_size" not in kw and type(kw.get("iterations", 1)) is int:   # (the schema types its own arguments)
            with pytest.raises(ValueError):
                _op(decode, a, **kw)
    for fixed in ([1, 0, 0], [1, 0, 0, 0, 0], [2, 0, 0, 0]):
        with pytest.raises(ValueError):
            _op(decode, a, fixed)
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)
    for V in (1, 5):                                                                  # V outside 2..4
        with pytest.raises(ValueError):
            decode.refine_rig(m(2, V, 5, 2), m(2, V, 5), (cams + cams)[:V])
        with pytest.raises(ValueError):
            decode.rig_refine_op(m(2, V, 5, 2), m(2, V, 5), m(V, 30), None, [1] + [0] * (V - 1), 1 / 64, 1 / 64, 0.5, 1e-6, 0.0, 8)
        with pytest.raises(ValueError):
            decode.calibrate_rig(m(2, V, 5, 16, 16), (cams + cams)[:V])
    for bad in ({"conf": m(2, 4, 4)}, {"coords": m(2, 4, 5, 3)}, {"cams": m(4, 17)}, {"ctm": m(2, 3, 4, 4)}, {"ctm": m(3, 4, 4, 4)},
                {"ctm": m(2, 4, 4, 4, dtype=torch.float64)}, {"ctm": m(1, 4, 4, 4, dtype=torch.float64)}, {"coords": m(2, 4, 5, 2, dtype=torch.float64)}):
        with pytest.raises(ValueError):
            _op(decode, dict(a, **bad))
    good = m(4, 3, 3)
    for matrix, ctm, B in ((m(4, 3, 2), None, 2), (m(5, 3, 3), None, 2), (good.double(), None, 2), (good, m(3, 4, 4, 4), 2), (good, None, 0),
                           (good, None, 2.0), (good, m(2, 4, 4, 4, dtype=torch.float64), 2), (m(3, 3, 3), None, 2)):
        with pytest.raises(ValueError):
            decode.apply_rig_correction(matrix, cams, ctm, B)


def test_cpu_tensors_are_refused():
    from egorear_amd import decode, hip
    cams = FS.rig()
    coords, conf = torch.zeros(1, 4, 3, 2), torch.ones(1, 4, 3)
    with pytest.raises(ValueError, match="no CPU path"):
        decode.refine_rig(coords, conf, cams)
    with pytest.raises(ValueError, match="no CPU path"):
        decode.calibrate_rig(torch.zeros(1, 4, 3, 16, 16), cams)
    with pytest.raises(ValueError, match="no CPU path"):
        decode.apply_rig_correction(torch.eye(3).expand(4, 3, 3).contiguous(), cams, None, 1)
    with pytest.raises((NotImplementedError, RuntimeError)):                         # the operator itself: no CPU kernel, no fallback
        decode.rig_refine_op(coords, conf, torch.zeros(4, 30), None, [1, 0, 0, 0], 1 / 64, 1 / 64, 0.5, 1e-6, 0.0, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.rig_refine(coords, conf, torch.zeros(4, 30))


def test_the_library_exports_the_entry_and_refuses_bad_arguments_itself():
    from egorear_amd import hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ("egr_rig_refine_f32", "egr_rig_refine_workspace_bytes"):
        assert name in hip.EXPORTS and hasattr(lib, name), name
    size = hip.lib.egr_rig_refine_workspace_bytes
    assert size(6, 4, 15) > 6 * 15 * 4 * 4 * 8 and size(6, 4, 15) % 8 == 0 and size(700, 4, 3) > size(6, 4, 15)
    assert size(0, 4, 15) == size(6, 1, 15) == size(6, 5, 15) == size(6, 4, 0) == 0
    # the entry validates before it launches: with pointers that are never followed, every refusal is a return code
    p = ctypes.c_void_p(64)

    def refine(B=2, V=4, J=3, mask=1, pw=0.0, iterations=8, ws=p, nbytes=1 << 30, md=1e-6):
        return hip.lib.egr_rig_refine_f32(p, p, p, None, 0, B, V, J, 1.0, 1.0, 0.5, md, mask, pw, iterations, ws, nbytes, p, p, p, p, p, p, p, p, p,
                                          None)

    assert refine(ws=None) == hip.ENULL
    for kw in ({"V": 1}, {"V": 5}, {"B": 0}, {"J": 0}, {"mask": -1}, {"mask": 16}, {"V": 2, "mask": 4}, {"pw": -1.0}, {"pw": float("nan")},
               {"pw": float("inf")}, {"iterations": 0}, {"iterations": 257}, {"md": -1.0}):
        assert refine(**kw) == hip.EINVAL, kw
    assert refine(nbytes=size(2, 4, 3) - 8) == hip.EWORKSPACE


# --------------------------------------------------------------------------- the statement, held to known answers

TABLE_SHAPES = ((6, 4, 15, False), (5, 2, 4, False), (3, 3, 2, False))
STATEMENT_ITERATIONS = 6
# max |rotation - truth| (rad) of the float64 statement after STATEMENT_ITERATIONS on `rotated`, measured on the CPU: 4.43e-8, 4.85e-8,
# 1.63e-7 - what the fp32 rounding of the coordinates (2e-6 to 5e-6 cm of ray distance) leaves of the truth; the bound is 8 x that
ROTATION_ERROR = {(6, 4, 15, False): 8 * 4.43e-8, (5, 2, 4, False): 8 * 4.85e-8, (3, 3, 2, False): 8 * 1.63e-7}


@pytest.mark.parametrize("shape", TABLE_SHAPES)
def test_the_statement_converges_as_the_issue_measured(shape):
    """The first three rows of the convergence table of DESIGN.md 5t (pure Gauss-Newton from the nominal rig, 0.03 rad, noise-free; other
    random draws than these scenes): RMS ray distance 2.28 -> 1.9e-2 -> 7.9e-6 -> 4.9e-6 cm, 1.11 -> 1.5e-2 -> 1.4e-4 -> 1.9e-6,
    1.29 -> 3.5e-2 -> 1.4e-5 -> 2.6e-6.  With mu = 1e-4, 1e-5, .. the damped iteration is Gauss-Newton to four digits, so the table's
    pattern is required of it: a start between 0.3 and 3 cm (0.03 rad at 10 to 100 cm); quadratic convergence, e' <= e^2 in cm - every
    step of every row of the table satisfies it, the tightest (1.5e-2 -> 1.4e-4) at 0.62 e^2 - down to the fp32 rounding of the
    coordinates, below 1e-5 cm (twice the table's largest) and reached after four iterations at the latest; never rising; and the truth
    recovered to ROTATION_ERROR."""
    sc, ops = RS.case(shape, "rotated")
    pr = RS.problem(sc, ops, torch.float64)
    out = RS.refine_statement(pr, STATEMENT_ITERATIONS)
    rms = [c ** 0.5 for c in out["costs"]]
    err = float((out["rotation"] - sc["vec"]).abs().max())
    print(f"{shape}: {pr.pairs} pairs, RMS ray distance by iteration {['%.2e' % r for r in rms]} cm, steps {out['steps']}, "
          f"max rotation error {err:.3e} rad (bound {ROTATION_ERROR[shape]:.3e})")
    assert out["valid"] and out["pairs"] == shape[0] * shape[2]
    assert 0.3 < rms[0] < 3.0 and all(b <= max(a * a, 1e-5) for a, b in zip(rms, rms[1:])) and rms[4] < 1e-5
    assert all(b <= a for a, b in zip(rms, rms[1:]))
    assert float(out["cost"]) <= float(out["cost0"]) and abs(float(out["cost0"]) - rms[0] ** 2) < 1e-12
    assert err <= ROTATION_ERROR[shape]
    assert float((out["matrix"].double() - RS.expm(sc["vec"])).abs().max()) <= ROTATION_ERROR[shape] + FS.ulp32(1.0)
    assert float(out["rotation"][0].abs().max()) == 0.0                              # view 0 is held
    # stationary at the returned fp32 matrices, by the solver-independent check the GPU test applies
    ratio = RS.stationarity(pr, out["matrix"])[0]
    print(f"    stationarity at the fp32 matrices: {ratio:.3g} of the allowance")
    assert ratio <= 1.0 / 8.0


@pytest.mark.parametrize("shape", TABLE_SHAPES)
def test_with_every_camera_fixed_the_statement_returns_the_identity(shape):
    sc, ops = RS.case(shape, "all_fixed")
    for dt in (torch.float64, torch.float32):
        out = RS.refine_statement(RS.problem(sc, ops, dt), 4)
        assert out["valid"] and out["steps"] == 0 and float(out["cost"]) == float(out["cost0"]) > 0.0
        assert float(out["rotation"].abs().max()) == 0.0 and torch.equal(out["matrix"], torch.eye(3).expand(shape[1], 3, 3))
    sc, ops = RS.case(shape, "nothing")
    out = RS.refine_statement(RS.problem(sc, ops, torch.float64), 4)
    assert not out["valid"] and out["pairs"] == 0 and float(out["cost"]) == 0.0


@pytest.mark.parametrize("name", ("rotated", "prior", "emptied"))
@pytest.mark.parametrize("shape", TABLE_SHAPES)
def test_the_gradient_agrees_with_a_central_difference_of_the_objective(shape, name):
    """The statement's gradient (the formula the kernel uses) at the identity and at a rotation off it, against
    (E(+h) - E(-h)) / 2h with h = 1e-5 rad: the difference's own error is h^2 E''' / 6 - 1e-10 of the third derivative - plus the
    rounding of E over h, 1e-16 * E / 1e-5: together below 1e-6 of the largest gradient component.  At the truth of a noise-free scene
    the residuals vanish, so the Gauss-Newton matrix there is the exact Hessian (autograd) to rounding."""
    sc, ops = RS.case(shape, name)
    pr = RS.problem(sc, ops, torch.float64)
    V, h = shape[1], 1e-5
    g0 = torch.Generator().manual_seed(5)
    for base in (torch.eye(3, dtype=torch.float64).expand(V, 3, 3).contiguous(), RS.expm(0.02 * torch.randn(V, 3, generator=g0, dtype=torch.float64))):
        base = torch.where(pr.fixed.view(V, 1, 1), torch.eye(3, dtype=torch.float64), base)
        _, _, failed, g, H = pr.system(base)
        assert not failed
        fd = torch.zeros(3 * V, dtype=torch.float64)
        for i in range(3 * V):
            e = torch.zeros(3 * V, dtype=torch.float64)
            e[i] = h
            fd[i] = (pr.objective(e.view(V, 3), base) - pr.objective(-e.view(V, 3), base)) / (2 * h)
        free = pr.free
        err, scale = float((g - fd)[free].abs().max()), float(g[free].abs().max())
        print(f"{shape} {name}: |g - central difference| {err:.3e} against max |g| {scale:.3e}")
        assert scale > 0.0 and err <= 1e-6 * scale
        ga = pr.grad_hess(base)[0]
        assert float((g - ga)[free].abs().max()) <= 1e-9 * scale
    if name == "rotated":
        truth = RS.expm(sc["vec"])
        _, _, _, g, H = pr.system(truth)
        Ha = pr.grad_hess(truth)[1]
        free2 = free.unsqueeze(0) & free.unsqueeze(1)
        rel = float(((H - Ha) * free2).abs().max() / (Ha * free2).abs().max())
        print(f"    at the truth: |H_gn - H_exact| / max |H| {rel:.3e}, max |g| {float(g[free].abs().max()):.3e}")
        assert rel <= 1e-5                                                           # (the fp32 coordinates leave residuals of 5e-6 cm)


def test_the_composition_equals_left_multiplication():
    """`apply_rig_correction` on the CPU's meta device cannot compute; its torch composition is the statement's `apply_correction`,
    which is held to a plain matrix product here: for given matrices [dR 0; 0 1] M, and for the syn rig M as FS.random_ctm writes a
    camera's nominal pose - the flip on the diagonal, the offset in m."""
    g = torch.Generator().manual_seed(3)
    cams = FS.rig()
    rec = FS.records(cams)
    dR = RS.expm(0.05 * torch.randn(4, 3, generator=g, dtype=torch.float64)).float()
    ctm = FS.random_ctm(5, 4, cams, g)
    for given, B in ((ctm, 5), (ctm[:1], 5), (None, 3)):
        got = RS.apply_correction(dR, rec, given, B)
        assert got.shape == (B, 4, 4, 4) and got.dtype == torch.float32
        for b in range(B):
            for v in range(4):
                if given is None:
                    f = -1.0 if cams[v].flip_xy else 1.0
                    M = torch.eye(4, dtype=torch.float64)
                    M[0, 0] = M[1, 1] = f
                    M[:3, 3] = torch.tensor(cams[v].packed_rays()[27:30].astype("float64")) * 0.01
                else:
                    M = given[b if given.shape[0] > 1 else 0, v].double()
                left = torch.eye(4, dtype=torch.float64)
                left[:3, :3] = dR[v].double()
                assert float(((left @ M).float() - got[b, v]).abs().max()) <= FS.ulp32(1.0)
    # the syn rig as matrices is the syn rig: the statement's triangulation agrees on both
    sc, ops = RS.case((6, 4, 15, False), "calibrated")
    eye = torch.eye(3).expand(4, 3, 3).contiguous()
    as_ctm = RS.apply_correction(eye, sc["rec"], None, 6)
    a = FS.statement(ops["coords"].double(), ops["conf"].double(), sc["rec"], None, 1 / 64, 1 / 64)
    b = FS.statement(ops["coords"].double(), ops["conf"].double(), sc["rec"], as_ctm, 1 / 64, 1 / 64)
    assert torch.equal(a[3], b[3]) and float((a[0] - b[0]).abs().max()) < 1e-4


def test_the_decode_composition_is_the_statements():
    """The torch lines of `decode.apply_rig_correction`, run on CPU float tensors through its own arithmetic (the device check aside),
    give the statement's matrices bit for bit."""
    from egorear_amd import decode
    g = torch.Generator().manual_seed(4)
    cams = FS.rig()
    dR = RS.expm(0.05 * torch.randn(4, 3, generator=g, dtype=torch.float64)).float()
    ctm = FS.random_ctm(3, 4, cams, g)
    real = decode.hip._on_device
    decode.hip._on_device = lambda *a, **k: None
    try:
        for given, B in ((ctm, 3), (ctm[:1], 4), (None, 2)):
            assert torch.equal(decode.apply_rig_correction(dR, cams, given, B), RS.apply_correction(dR, FS.records(cams), given, B))
    finally:
        decode.hip._on_device = real

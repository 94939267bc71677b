"""Fisheye triangulation on the GPU (egr_triangulate_f32 / egr_triangulate_bwd_f32, egorear_amd/decode.py) against the float64
statement of its math in tests/fisheye_statement.py, in elementwise torch operations: ray by Newton to convergence, the normal equations,
a closed-form symmetric solve, the cost and the ray distances.  torch.autograd differentiates the statement; no LAPACK call is involved.

The yardstick (fisheye_statement.yardstick) is the one of test_gpu_soft_argmax.py: a HIP output or gradient may deviate from the
float64 statement (evaluated on the same fp32 inputs) by at most 8 x the deviation of torch's fp32 CPU evaluation of that statement - computed per case and printed next to
the HIP figure - with a floor of 4 ulp (fp32) of the output's largest magnitude for the cases where the fp32 evaluation is exact."""
import numpy as np
import pytest
import torch

from fisheye_statement import (HM, MARGIN, MIN_DET, THR, bumps, project, random_ctm, random_points, records, rig, soft_argmax_statement,
                               statement, ulp32, yardstick)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (B, V, J, rw): the product layout on the syn rig; the two front cameras; one pair; rw with a per-sample coord_trans_mat
SHAPES = [(4, 4, 15, False), (3, 2, 5, False), (1, 3, 1, False), (5, 4, 16, True)]
CASES = ("ones", "noisy", "dropped", "nan")


# --------------------------------------------------------------------------- data, computed once and shared (never modified)

_CACHE = {}


def evaluate(coords, conf, rec, ctm, sx, sy, g_pts, g_cost, thr=THR):
    """The statement and its autograd in float64 and in float32 on the same fp32 inputs."""
    out = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        c, w = coords.clone().to(dt).requires_grad_(), conf.clone().to(dt).requires_grad_()
        pts, cost, resid, ok = statement(c, w, rec, ctm, sx, sy, thr)
        gc, gw = torch.autograd.grad([pts, cost], [c, w], [g_pts.to(dt), g_cost.to(dt)], allow_unused=True)
        out[name] = {"pts": pts.detach(), "cost": cost.detach(), "resid": resid.detach(), "ok": ok,
                     "g_coords": torch.zeros_like(c) if gc is None else gc, "g_conf": torch.zeros_like(w) if gw is None else gw}
    return out


def shape_data(shape):
    if shape in _CACHE:
        return _CACHE[shape]
    B, V, J, rw = shape
    g = torch.Generator().manual_seed(100 * B + 10 * V + J)
    cams = rig("ego4view_rw" if rw else "ego4view_syn")[:V]
    rec = records(cams)
    ctm = random_ctm(B, V, cams, g) if rw else None
    pts = random_points(B, J, g)
    clean = (project(pts, rec, ctm) * HM).float()
    g_pts, g_cost = torch.randn(B, J, 3, generator=g), torch.randn(B, J, generator=g)
    cases = {}
    for case in CASES:
        coords, conf, thr = clean.clone(), torch.ones(B, V, J), THR
        if case == "noisy":              # every view counts, with its own weight (the threshold is below the smallest confidence)
            thr = 0.05
            conf = torch.rand(B, V, J, generator=g) * 0.9 + 0.1
            coords = coords + 0.05 * torch.randn(B, V, J, 2, generator=g)
        elif case == "dropped":          # pair k loses (k + 1) % (V + 1) of its views: V, ..., one, zero views are left
            conf = torch.rand(B, V, J, generator=g) * 0.4 + 0.6
            coords = coords + 0.05 * torch.randn(B, V, J, 2, generator=g)
            for k in range(B * J):
                for i in range((k + 1) % (V + 1)):
                    conf[k // J, (k + i) % V, k % J] = 0.3
        elif case == "nan":              # one view of every other pair has a NaN coordinate: that view alone is excluded
            conf = torch.rand(B, V, J, generator=g) * 0.4 + 0.6
            for k in range(0, B * J, 2):
                coords[k // J, k % V, k % J, k % 2] = float("nan")
        cases[case] = (coords.contiguous(), conf.contiguous(), thr, evaluate(coords, conf, rec, ctm, 1.0 / HM, 1.0 / HM, g_pts, g_cost, thr))
    _CACHE[shape] = {"cams": cams, "rec": rec, "ctm": ctm, "pts": pts, "g_pts": g_pts, "g_cost": g_cost, "cases": cases}
    return _CACHE[shape]


def launch(d, coords, conf, hm=HM, thr=THR):
    from egorear_amd import hip
    ctm = None if d["ctm"] is None else d["ctm"].to(DEV)
    return hip.triangulate(coords.to(DEV), conf.to(DEV), d["rec"].to(DEV), ctm, 1.0 / hm, 1.0 / hm, thr, MIN_DET)


# --------------------------------------------------------------------------- forward

@pytest.mark.parametrize("shape", SHAPES)
def test_forward_against_the_float64_statement(shape):
    d = shape_data(shape)
    B, V, J, _ = shape
    bad = []
    for case in CASES:
        coords, conf, thr, ref = d["cases"][case]
        pts, cost, resid, ok = launch(d, coords, conf, thr=thr)
        torch.cuda.synchronize()
        print(f"{shape} {case}:")
        assert torch.equal(ok.cpu().bool(), ref["f64"]["ok"]), (shape, case)
        for name, got in (("pts", pts), ("cost", cost), ("resid", resid)):
            err, allowed = yardstick(name, got, ref["f32"][name], ref["f64"][name])
            if not err <= allowed:
                bad.append((shape, case, name, err, allowed))
        used = ((conf >= thr) & torch.isfinite(coords).all(-1)).sum(1)
        assert torch.equal(ok.cpu().bool(), used >= 2), (shape, case)          # the rig's rays are never parallel
        dead = ~ok.cpu().bool()
        assert float(pts.cpu()[dead].abs().sum()) == 0.0 and float(cost.cpu()[dead].abs().sum()) == 0.0
        assert float(resid.cpu().permute(0, 2, 1)[dead].abs().sum()) == 0.0
        excluded = ~((conf >= thr) & torch.isfinite(coords).all(-1))
        assert float(resid.cpu()[excluded].abs().sum()) == 0.0                   # an excluded view reports no distance
        if case == "dropped" and B * J >= V + 1:
            assert sorted(set(used.view(-1).tolist())) == list(range(V + 1))     # V, ..., two, one and zero views all occur
        if case == "nan":
            assert bool(torch.isfinite(pts).all()) and int(used.min()) == V - 1 and int(used.max()) == (V if B * J > 1 else V - 1)
        if case in ("noisy", "dropped") and bool(ok.any()):
            assert float(cost.max()) > 1e-4 and float(resid.max()) > 1e-2      # the noise makes them non-trivial
    assert not bad, bad


@pytest.mark.parametrize("shape", SHAPES)
def test_round_trip_returns_the_projected_points(shape):
    d = shape_data(shape)
    coords, conf, _, ref = d["cases"]["ones"]
    pts, _, _, ok = launch(d, coords, conf)
    assert bool(ok.all())
    err, own = float((pts.double().cpu() - d["pts"]).abs().max()), float((ref["f32"]["pts"].double() - d["pts"]).abs().max())
    floor = 4.0 * ulp32(float(d["pts"].abs().max()))
    print(f"{shape}: |hip - projected points| {err:.3e} cm, |torch fp32 - projected points| {own:.3e} cm, floor {floor:.3e}")
    assert err <= max(MARGIN * own, floor)


def test_inverts_the_shipped_projection():
    """rw mode: the anchors of egr_fisheye_project2_f32 triangulate back to the points they were projected from."""
    from egorear_amd import hip
    d = shape_data(SHAPES[3])
    B, V, J, _ = SHAPES[3]
    pts = d["pts"].float().contiguous()
    cams17 = torch.from_numpy(np.stack([c.packed() for c in d["cams"]])).to(DEV)
    out = torch.empty(B, J, 3, device=DEV)
    anchors, valid, _ = hip.fisheye_project(pts.to(DEV), d["ctm"].to(DEV), cams17, out=out)
    conf = valid.float()
    got, _, _, ok = hip.triangulate(anchors, conf, d["rec"].to(DEV), d["ctm"].to(DEV), 1.0, 1.0, 0.5, MIN_DET)
    torch.cuda.synchronize()
    seen = valid.sum(1) >= 2
    assert int(seen.sum()) >= B * J // 2 and torch.equal(ok.bool(), seen)
    f32 = statement(anchors.cpu(), conf.cpu(), d["rec"], d["ctm"], 1.0, 1.0)[0]
    keep = seen.cpu()
    err = float((got.double().cpu() - pts.double())[keep].abs().max())
    own = float((f32.double() - pts.double())[keep].abs().max())
    floor = 4.0 * ulp32(float(pts.abs().max()))
    print(f"anchors of the shipped projection: |hip - points| {err:.3e} cm, |torch fp32 - points| {own:.3e} cm, floor {floor:.3e}, "
          f"{int(seen.sum())} of {B * J} joints seen by two views or more")
    assert err <= max(MARGIN * own, floor)


def test_a_point_on_the_optical_axis():
    """View 0 is given its image centre exactly (fp32): the ray is finite and the result meets the yardstick."""
    from egorear_amd import hip
    cams = rig()
    rec = records(cams)
    pts = torch.tensor([[[-6.0, 0.0, 40.0], [-6.0, 0.0, 120.0]]], dtype=torch.float64)      # on camera_front_left's axis (offset +6)
    coords = project(pts, rec, None).float()
    coords[0, 0, :, 0] = float(np.float32(cams[0].image_center[0]) / np.float32(cams[0].image_size[1]))
    coords[0, 0, :, 1] = float(np.float32(cams[0].image_center[1]) / np.float32(cams[0].image_size[0]))
    assert bool(torch.isfinite(coords).all())
    conf = torch.ones(1, 4, 2)
    got = hip.triangulate(coords.to(DEV), conf.to(DEV), rec.to(DEV), None, 1.0, 1.0, THR, MIN_DET)
    f64, f32 = statement(coords.double(), conf.double(), rec, None, 1.0, 1.0), statement(coords, conf, rec, None, 1.0, 1.0)
    assert bool(got[3].all()) and all(bool(torch.isfinite(t).all()) for t in got[:3])
    for i, name in enumerate(("pts", "cost", "resid")):
        err, allowed = yardstick(name, got[i], f32[i], f64[i])
        assert err <= allowed, (name, err, allowed)
    # (the guard replaces a ray at most 1e-4 pixels = 4e-7 rad off the axis: 5e-5 cm at 120 cm, far inside this)
    assert float((got[0].double().cpu() - pts).abs().max()) < 1e-2
    # and the gradient at the axis is finite (the ray is constant there)
    g_coords, g_conf = hip.triangulate_bwd(coords.to(DEV), conf.to(DEV), rec.to(DEV), None, torch.ones(1, 2, 3, device=DEV), None, 1.0, 1.0,
                                           THR, MIN_DET)
    assert bool(torch.isfinite(g_coords).all()) and bool(torch.isfinite(g_conf).all()) and float(g_coords[0, 0].abs().max()) == 0.0


def test_parallel_rays_are_not_ok():
    from egorear_amd import hip
    cams = rig()
    rec = records([cams[0], cams[0]])
    coords = torch.tensor([20.0, 30.0]).expand(2, 2, 3, 2).contiguous()
    pts, cost, resid, ok = hip.triangulate(coords.to(DEV), torch.ones(2, 2, 3, device=DEV), rec.to(DEV), None, 1.0 / HM, 1.0 / HM, THR, MIN_DET)
    assert int(ok.sum()) == 0 and float(pts.abs().sum()) == 0.0 and float(cost.abs().sum()) == 0.0 and float(resid.abs().sum()) == 0.0
    g_coords, g_conf = hip.triangulate_bwd(coords.to(DEV), torch.ones(2, 2, 3, device=DEV), rec.to(DEV), None, torch.ones(2, 3, 3, device=DEV),
                                           torch.ones(2, 3, device=DEV), 1.0 / HM, 1.0 / HM, THR, MIN_DET)
    assert float(g_coords.abs().sum()) == 0.0 and float(g_conf.abs().sum()) == 0.0


# --------------------------------------------------------------------------- backward

@pytest.mark.parametrize("shape", SHAPES)
def test_backward_against_float64_autograd(shape):
    from egorear_amd import decode
    d = shape_data(shape)
    bad = []
    for case in CASES:
        coords, conf, thr, ref = d["cases"][case]
        c, w = coords.to(DEV).requires_grad_(), conf.to(DEV).requires_grad_()
        ctm = None if d["ctm"] is None else d["ctm"].to(DEV)
        pts, cost, resid, ok = decode.triangulate_op(c, w, d["rec"].to(DEV), ctm, 1.0 / HM, 1.0 / HM, thr, MIN_DET)
        assert pts.requires_grad and cost.requires_grad and not resid.requires_grad and not ok.requires_grad
        g_coords, g_conf = torch.autograd.grad([pts, cost], [c, w], [d["g_pts"].to(DEV), d["g_cost"].to(DEV)])
        torch.cuda.synchronize()
        print(f"{shape} {case}:")
        for name, got in (("g_coords", g_coords), ("g_conf", g_conf)):
            err, allowed = yardstick(name, got, ref["f32"][name], ref["f64"][name])
            if not err <= allowed:
                bad.append((shape, case, name, err, allowed))
        excluded = ~((conf >= thr) & torch.isfinite(coords).all(-1)) | ~ok.cpu().bool().unsqueeze(1)
        assert float(g_conf.cpu()[excluded].abs().sum()) == 0.0 and float(g_coords.cpu()[excluded].abs().sum()) == 0.0
        assert bool(torch.isfinite(g_coords).all()) and bool(torch.isfinite(g_conf).all())
    assert not bad, bad


# --------------------------------------------------------------------------- determinism and replay

def test_two_runs_and_a_graph_replay_give_the_same_bits():
    from egorear_amd import hip
    d = shape_data(SHAPES[0])
    coords, conf, _, _ = d["cases"]["dropped"]
    c, w, rec = coords.to(DEV), conf.to(DEV), d["rec"].to(DEV)
    gp, gc = d["g_pts"].to(DEV), d["g_cost"].to(DEV)
    eager = hip.triangulate(c, w, rec, None, 1.0 / HM, 1.0 / HM, THR, MIN_DET)
    g_eager = hip.triangulate_bwd(c, w, rec, None, gp, gc, 1.0 / HM, 1.0 / HM, THR, MIN_DET)
    again = hip.triangulate(c, w, rec, None, 1.0 / HM, 1.0 / HM, THR, MIN_DET)
    g_again = hip.triangulate_bwd(c, w, rec, None, gp, gc, 1.0 / HM, 1.0 / HM, THR, MIN_DET)
    for a, b in zip(eager + g_eager, again + g_again):
        assert torch.equal(a, b)
    one = hip.triangulate(c[2:3].contiguous(), w[2:3].contiguous(), rec, None, 1.0 / HM, 1.0 / HM, THR, MIN_DET)
    for a, b in zip(eager, one):                                      # a frame's bits do not depend on the batch around it
        assert torch.equal(a[2:3], b)
    torch.cuda.synchronize()
    static = c.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                    # one stream, no parallel branches
        out = hip.triangulate(static, w, rec, None, 1.0 / HM, 1.0 / HM, THR, MIN_DET)
        g = hip.triangulate_bwd(static, w, rec, None, gp, gc, 1.0 / HM, 1.0 / HM, THR, MIN_DET)
    static.copy_(torch.zeros_like(c))
    graph.replay()
    static.copy_(c)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager + g_eager, out + g):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------- heat maps to 3-D

@pytest.fixture(scope="module")
def bump_maps():
    """Gaussian bumps (sigma 1, 64 x 64) at the projections of known points, B = 2, V = 4, J = 15, on the syn rig."""
    g = torch.Generator().manual_seed(77)
    cams = rig()
    rec = records(cams)
    pts = random_points(2, 15, g)
    return {"cams": cams, "rec": rec, "pts": pts, "hm": bumps(pts, rec, None, HM, HM).float().contiguous()}


def test_decode_joints_3d_on_rendered_bumps(bump_maps):
    from egorear_amd import decode
    hm, rec, pts = bump_maps["hm"], bump_maps["rec"], bump_maps["pts"]
    tri, j2 = decode.decode_joints_3d(hm.to(DEV), bump_maps["cams"], beta=100.0, threshold=0.5)
    torch.cuda.synchronize()
    assert tri.pose.shape == (2, 15, 3) and tri.cost.shape == (2, 15) and tri.residual.shape == (2, 4, 15)
    assert tri.valid.dtype == torch.bool and bool(tri.valid.all()) and j2.soft.shape == (2, 4, 15, 2)
    by_name, _ = decode.decode_joints_3d(hm.to(DEV), "ego4view_syn")                  # the packaged calibrations, by camera_model
    assert torch.equal(by_name.pose, tri.pose)
    # the bound: what the float64 statement makes of the float64 soft-argmax of the same maps, plus the yardstick
    c64, m64 = soft_argmax_statement(hm.double(), 100.0)
    c32, m32 = soft_argmax_statement(hm, 100.0)
    p64 = statement(c64, m64, rec, None, 1.0 / HM, 1.0 / HM)[0]
    p32 = statement(c32, m32, rec, None, 1.0 / HM, 1.0 / HM)[0]
    decode_err = float((p64 - pts).abs().max())
    err, allowed = yardstick("pose", tri.pose, p32, p64)
    total = float((tri.pose.double().cpu() - pts).abs().max())
    print(f"pose error against the rendered points: hip {total:.4e} cm, float64 decode {decode_err:.4e} cm")
    assert err <= allowed and total <= decode_err + allowed


def test_gradient_reaches_the_heat_maps_through_both_backwards(bump_maps):
    from egorear_amd import decode, hip
    g = torch.Generator().manual_seed(5)
    g_pts, g_cost = torch.randn(2, 15, 3, generator=g).to(DEV), torch.randn(2, 15, generator=g).to(DEV)
    hm = bump_maps["hm"].to(DEV).requires_grad_()
    tri, _ = decode.decode_joints_3d(hm, bump_maps["cams"])
    (g_hm,) = torch.autograd.grad([tri.pose, tri.cost], [hm], [g_pts, g_cost])
    coords, maxvals, index, _, stat, _ = hip.soft_argmax(hm.detach(), 100.0, 0, False, 0.5)
    g_coords, g_conf = hip.triangulate_bwd(coords.view(2, 4, 15, 2), maxvals.view(2, 4, 15), bump_maps["rec"].to(DEV), None, g_pts, g_cost,
                                           1.0 / HM, 1.0 / HM, 0.5, MIN_DET)
    want = hip.soft_argmax_bwd(hm.detach(), stat, coords, index, g_coords.view(-1, 2), g_conf.view(-1), 100.0, 0)
    torch.cuda.synchronize()
    assert float(g_hm.abs().max()) > 0.0 and torch.equal(g_hm, want.view_as(g_hm))


def test_bad_launches_are_refused():
    from egorear_amd import hip
    rec = records(rig()).to(DEV)
    coords, conf = torch.zeros(1, 4, 2, 2, device=DEV), torch.ones(1, 4, 2, device=DEV)
    pts, cost, resid, ok = (torch.empty(1, 2, 3, device=DEV), torch.empty(1, 2, device=DEV), torch.empty(1, 4, 2, device=DEV),
                            torch.empty(1, 2, dtype=torch.uint8, device=DEV))
    for V, sx, det in ((1, 1.0, 1e-6), (5, 1.0, 1e-6), (4, 0.0, 1e-6), (4, 1.0, -1.0), (4, 1.0, float("inf"))):      # the C entry itself
        rc = hip.lib.egr_triangulate_f32(coords.data_ptr(), conf.data_ptr(), rec.data_ptr(), None, 1, V, 2, sx, 1.0, 0.5, det, pts.data_ptr(),
                                         cost.data_ptr(), resid.data_ptr(), ok.data_ptr(), None)
        assert rc == hip.EINVAL, (V, sx, det, rc)

"""The ray-space clip smoother without a device: the float64 statement of tests/ray_track_statement.py against what it
must reduce to - the triangulation at T = 1, a straight line seen by one camera at a time, its own block-banded loop, Huber's
majorise-minimise property, the corners of the solvability rule - and the Python layers: operand checks, fake implementations, the
library's own refusals."""
import ctypes
import itertools

import pytest
import torch

import fisheye_statement as FS
import ray_track_statement as RS

META = lambda *shape, **kw: torch.empty(*shape, device="meta", **kw)
LAMBDAS = [(0.0, 10.0), (1.0, 0.0), (0.5, 100.0), (0.0, 1000.0)]          # (lambda_v, lambda_a): the trajectory tests' pairs


def fit(sc, **kw):
    return RS.fit(sc["coords"], sc["conf"], sc["rec"], sc["ctm"], sc["sx"], sc["sy"], **kw)


# --------------------------------------------------------------------------- what the statement reduces to

@pytest.mark.parametrize("rw", [False, True])
@pytest.mark.parametrize("V", [2, 3, 4])
def test_one_frame_is_the_triangulation(V, rw):
    sc = RS.scene(3, 1, V, 5, "dense", rw)
    tri, _, _, ok = FS.statement(sc["coords"][:, 0].double(), sc["conf"][:, 0].double(), sc["rec"], None if sc["ctm"] is None else sc["ctm"][:, 0].double(),
                                 sc["sx"], sc["sy"])
    for lv, la in ((1.0, 0.0), (0.5, 100.0)):                                          # (one frame: no row of either penalty)
        out = fit(sc, lv=lv, la=la)
        err = float((out["pose"][:, 0] - tri).abs().max())
        print(f"V {V} rw {rw} lambda {(lv, la)}: |track - triangulated point| {err:.3e} cm")
        assert bool(ok.all()) and bool(out["ok"].all()) and bool(out["valid"].all())
        assert err <= 1e-9


def line_scene(T, V, rw, J=3):
    """Joints on straight lines at 3.3 cm a frame (a limb at 1 m/s filmed at 30 frames a second), noise-free, float64 coordinates;
    frame t is seen by camera t mod V alone."""
    g = torch.Generator().manual_seed(100 * T + V + (7 if rw else 0))
    cams = FS.rig("ego4view_rw" if rw else "ego4view_syn")[:V]
    rec = FS.records(cams)
    vel = torch.randn(1, J, 3, generator=g, dtype=torch.float64)
    vel = 3.3 * vel / vel.norm(dim=-1, keepdim=True)
    t = torch.arange(T, dtype=torch.float64).view(1, T, 1, 1) - (T - 1) / 2
    truth = FS.random_points(1, J, g).unsqueeze(1) + vel.unsqueeze(1) * t
    ctm = FS.random_ctm(T, V, cams, g) if rw else None
    sx = sy = 1.0 / FS.HM
    coords = FS.project(truth.view(T, J, 3), rec, None if ctm is None else ctm.double(), sx, sy).view(1, T, V, J, 2)
    conf = torch.zeros(1, T, V, J, dtype=torch.float64)
    for tt in range(T):
        conf[0, tt, tt % V] = 0.9
    return {"coords": coords, "conf": conf, "rec": rec, "ctm": None if ctm is None else ctm.view(1, T, V, 4, 4), "sx": sx, "sy": sy, "truth": truth}


@pytest.mark.parametrize("rw", [False, True])
@pytest.mark.parametrize("V", [2, 4])
@pytest.mark.parametrize("T", [3, 4, 5, 33])
def test_a_line_seen_by_one_camera_at_a_time_comes_back(T, V, rw):
    """Every frame has one ray: nothing for the triangulation, and with the acceleration penalty alone exactly the line.  (T = 3 with
    two cameras is exactly determined - six ray equations for the six unknowns of a line - and at accel_weight 1000 cond(A) is 1e9 to
    4e9: solved about the device origin the float64 solve's own rounding, eps |A| |x| / lambda_min, is 0.4e-6 to 1.4e-6 cm there;
    the statement is therefore solved a second time about the first solution's mean, where |unknowns| is the track's extent.)"""
    sc = line_scene(T, V, rw)
    _, _, _, ok = FS.statement(sc["coords"].view(T, V, 3, 2), sc["conf"].view(T, V, 3), sc["rec"], None if sc["ctm"] is None else sc["ctm"].view(T, V, 4, 4).double(),
                               sc["sx"], sc["sy"])
    assert not bool(ok.any())                                                          # today's path returns nothing here
    for la in (1.0, 10.0, 1000.0):
        first = fit(sc, lv=0.0, la=la, max_gap=0)
        out = fit(sc, lv=0.0, la=la, max_gap=0, centre=first["pose"].mean(1))
        err, raw = float((out["pose"] - sc["truth"]).abs().max()), float((first["pose"] - sc["truth"]).abs().max())
        print(f"T {T} V {V} rw {rw} accel {la}: |track - line| {err:.3e} cm (about the origin {raw:.3e}), energy {float(out['energy'].max()):.3e}, "
              f"cond(A) {out['cond']:.3e}")
        assert bool(out["ok"].all()) and bool(out["valid"].all()) and bool((out["rays"] == 1).all())
        assert err <= 1e-6 and float(out["energy"].max()) <= 1e-9


@pytest.mark.parametrize("case", RS.CASES)
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 2, 3), (1, 3, 2), (2, 4, 15), (1, 5, 16), (3, 64, 15), (1, 65, 16)])
def test_the_banded_loop_agrees_with_the_dense_solve(shape, case):
    """Both are solved about the mean of a first dense solution: a float64 solve's rounding is eps cond(A) |unknowns|.  What 1e-6 cm
    can resolve is cond(A) up to about 1e8, not the 1e10 asserted: the `oneview` case therefore alternates single views with whole
    frames (cond(A) <= 4e6 here) - with single views drawn at random, three frames of the front pair reached cond(A) 2e9 at
    accel_weight 1000, where the two float64 solves differ by 2e-6 cm about any centre."""
    N, T, J = shape
    for i, lam in enumerate(LAMBDAS):
        V, rw = 2 + (i + T) % 3, bool((i + J) % 2)
        sc = RS.scene(N, T, V, J, case, rw)
        first = fit(sc, lv=lam[0], la=lam[1])
        centre = first["pose"].mean(1)                                                  # (both solves about the track's own place)
        out = fit(sc, lv=lam[0], la=lam[1], centre=centre)
        x, low, top = RS.banded_fit(sc["coords"], sc["conf"], sc["rec"], sc["ctm"], sc["sx"], sc["sy"], lv=lam[0], la=lam[1], centre=centre)
        ok = out["ok"]
        diff = (x - out["pose"]).abs().permute(0, 2, 1, 3)[ok]
        err = float(diff.max()) if diff.numel() else 0.0
        ratio = float((low / top)[ok].min()) if bool(ok.any()) else float("inf")
        print(f"{shape} V {V} rw {rw} {case} lambda {lam}: {int(ok.sum())} of {N * J} tracks solvable, |banded - dense| {err:.3e} cm, cond(A) "
              f"{out['cond']:.3e}, smallest pivot / largest diagonal entry {ratio:.3e}")
        assert out["cond"] <= 1e10 and err <= 1e-6
        if case == "gaps":                                                              # every fifth track has no ray at all
            assert not bool(ok.all()) or N * J < 5
            assert float(out["pose"].permute(0, 2, 1, 3)[~ok].abs().sum()) == 0.0 and not bool(out["valid"].permute(0, 2, 1)[~ok].any())


def test_hubers_energy_does_not_increase_and_the_bad_views_lose():
    """Single views off by 10 to 30 heat-map pixels in three frames a track: the energy with Huber's rho falls from round to round (a
    majorise-minimise step), and at those frames the reweighted track is nearer the truth than the plain one."""
    sc = RS.scene(2, 24, 4, 6, "glitch", noise=0.05, glitch_px=(10.0, 30.0))
    at = sorted({(n, t, j) for n, t, _, j in sc["glitches"]})
    pick = lambda x: torch.stack([x[n, t, j] for n, t, j in at])
    for lam in LAMBDAS:
        before, errs = None, []
        for K in range(9):
            out = fit(sc, lv=lam[0], la=lam[1], huber=1.0, reweights=K)
            E = out["energy"]
            errs.append(float((pick(out["pose"]) - pick(sc["truth"])).norm(dim=-1).mean()))
            print(f"lambda {lam} K {K}: energy {float(E.sum()):.6f}, mean error at the glitches {errs[-1]:.4f} cm")
            assert before is None or bool((E <= before * (1.0 + 1e-12)).all()), (lam, K)
            before = E
        assert errs[-1] < errs[0] and errs[4] < errs[0], (lam, errs)


def corner(T, used, lv, la, static=False):
    """One track of a joint on a line (or at rest); `used` lists the (frame, view) pairs that see it."""
    sc = line_scene(T, 4, False, J=1)
    if static:
        truth = sc["truth"][:, :1].expand(1, T, 1, 3).contiguous()
        sc["coords"] = FS.project(truth.view(T, 1, 3), sc["rec"], None, sc["sx"], sc["sy"]).view(1, T, 4, 1, 2)
    sc["conf"] = torch.zeros(1, T, 4, 1, dtype=torch.float64)
    for t, v in used:
        sc["conf"][0, t, v, 0] = 0.9
    use, w, d, R, tt = RS.clip_rays(sc["coords"], sc["conf"], sc["rec"], None, sc["sx"], sc["sy"])
    G, g = RS.blocks(w, d, R, tt, 1, T)
    _, low, top = RS.banded(G, g, lv, la)
    return bool(fit(sc, lv=lv, la=la)["ok"][0, 0]), bool(RS.enough_rays(use, 1, T, lv)[0, 0]), float(low[0, 0] / top[0, 0])


def test_the_corners_of_the_solvability_rule():
    """Each corner stands a factor of 1e3 or more away from min_pivot_ratio = 1e-10, on the side named."""
    T = 6
    every = [(t, 0) for t in range(T)]
    cases = [  # (what, used rays, lv, la, static, solvable, rule (a) holds)
        ("two rays, acceleration alone", [(2, 0), (2, 1)], 0.0, 10.0, False, False, False),
        ("two rays with a velocity penalty", [(2, 0), (2, 1)], 1.0, 10.0, False, True, True),
        ("one ray with a velocity penalty", [(2, 0)], 1.0, 10.0, False, False, False),
        ("four rays on one frame, acceleration alone", [(3, 0), (3, 1), (3, 2), (3, 3)], 0.0, 10.0, False, False, False),
        ("four rays on one frame with a velocity penalty", [(3, 0), (3, 1), (3, 2), (3, 3)], 0.5, 0.0, False, True, True),
        # (rule (a) is necessary, not sufficient: two rays fix the point of their frame, the third leaves the velocity along itself free)
        ("three rays on two frames, acceleration alone", [(1, 0), (1, 1), (4, 2)], 0.0, 10.0, False, False, True),
        ("two rays on each of two frames, acceleration alone", [(1, 0), (1, 1), (4, 2), (4, 3)], 0.0, 10.0, False, True, True),
        ("a point at rest seen through one camera centre, acceleration alone", every, 0.0, 10.0, True, False, True),
        ("the same with a velocity penalty", every, 1.0, 0.0, True, False, True),
        ("a point at rest seen by two cameras in turn, acceleration alone", [(t, t % 2) for t in range(T)], 0.0, 10.0, True, True, True),
    ]
    for what, used, lv, la, static, want, want_a in cases:
        ok, enough, ratio = corner(T, used, lv, la, static)
        print(f"{what}: solvable {ok}, rule (a) {enough}, smallest pivot / largest diagonal entry {ratio:.3e}")
        assert ok == want and enough == want_a, what
        assert ratio >= 1e-7 if want else (ratio <= 1e-13 or not enough), what
        if not want and enough:
            assert ratio <= 1e-13, what                                                 # rule (b) alone refuses it


# --------------------------------------------------------------------------- the Python layers without a device

def test_every_bad_parameter_and_shape_is_a_value_error_before_any_launch():
    from egorear_amd import decode, hip
    cams = FS.rig()
    rec = FS.records(cams)
    good = dict(sx=1 / 64, sy=1 / 64, threshold=0.5, vel_weight=0.0, accel_weight=10.0, huber=0.0, reweights=0, max_gap=8, min_pivot_ratio=1e-10)
    bad = ({"vel_weight": -1.0}, {"accel_weight": -1.0}, {"accel_weight": 0.0}, {"vel_weight": float("nan")}, {"accel_weight": float("inf")},
           {"huber": -0.5}, {"huber": float("nan")}, {"reweights": -1}, {"reweights": 17}, {"reweights": 2}, {"huber": 1.0},
           {"reweights": 1.0, "huber": 1.0}, {"reweights": True, "huber": 1.0}, {"max_gap": -1}, {"max_gap": 1.5}, {"sx": 0.0}, {"sy": float("inf")},
           {"threshold": float("nan")}, {"min_pivot_ratio": -1e-3}, {"min_pivot_ratio": 1.0}, {"min_pivot_ratio": float("nan")})
    for kw in bad:
        args = dict(good, **kw)
        for c, f, r in ((torch.zeros(2, 6, 4, 3, 2), torch.ones(2, 6, 4, 3), rec), (META(2, 6, 4, 3, 2), META(2, 6, 4, 3), rec.to("meta"))):
            with pytest.raises(ValueError):
                hip.ray_track(c, f, r, None, **args)
        if type(args["reweights"]) is int and type(args["max_gap"]) is int:           # (the operator's schema refuses other types itself)
            with pytest.raises(ValueError):
                decode.ray_track_op(META(2, 6, 4, 3, 2), META(2, 6, 4, 3), rec.to("meta"), None, *(args[k] for k in good))
        if not {"sx", "sy"} & set(kw):
            with pytest.raises(ValueError):
                decode.fit_ray_tracks(META(2, 6, 4, 3, 2), META(2, 6, 4, 3), cams, None, (64, 64), args["threshold"], args["accel_weight"],
                                      args["vel_weight"], args["huber"], args["reweights"], args["max_gap"], args["min_pivot_ratio"])
            with pytest.raises(ValueError):
                decode.decode_clip_3d_rays(META(1, 6, 4, 3, 16, 16), cams, threshold=args["threshold"], accel_weight=args["accel_weight"],
                                           vel_weight=args["vel_weight"], huber_cm=args["huber"], reweights=args["reweights"], max_gap=args["max_gap"],
                                           min_pivot_ratio=args["min_pivot_ratio"])
    mrec = rec.to("meta")
    shapes = ((META(2, 6, 4, 3), META(2, 6, 4, 3), mrec, None), (META(2, 6, 4, 3, 3), META(2, 6, 4, 3), mrec, None),
              (META(0, 6, 4, 3, 2), META(0, 6, 4, 3), mrec, None), (META(1, 4097, 4, 1, 2), META(1, 4097, 4, 1), mrec, None),
              (META(2, 6, 4, 3, 2, dtype=torch.float64), META(2, 6, 4, 3), mrec, None), (META(2, 6, 4, 3, 2), META(2, 6, 4, 4), mrec, None),
              (META(2, 6, 4, 3, 2), META(2, 6, 4, 3, dtype=torch.float64), mrec, None), (META(2, 6, 1, 3, 2), META(2, 6, 1, 3), mrec[:1], None),
              (META(2, 6, 5, 3, 2), META(2, 6, 5, 3), META(5, 30), None), (META(2, 6, 4, 3, 2), META(2, 6, 4, 3), mrec[:3], None),
              (META(2, 6, 4, 3, 2), META(2, 6, 4, 3), META(4, 17), None), (META(2, 6, 4, 3, 2), META(2, 6, 4, 3), mrec, META(12, 4, 4, 4)),
              (META(2, 6, 4, 3, 2), META(2, 6, 4, 3), mrec, META(2, 6, 4, 4, 4, dtype=torch.float64)),
              (META(1 << 10, 1 << 10, 4, 1 << 8, 2), META(1 << 10, 1 << 10, 4, 1 << 8), mrec, None))
    for c, f, r, m in shapes:
        with pytest.raises(ValueError):
            hip.ray_track(c, f, r, m, **good)
        with pytest.raises(ValueError):
            decode.ray_track_op(c, f, r, m, *(good[k] for k in good))
    with pytest.raises(ValueError):
        hip.ray_track(torch.zeros(2, 6, 4, 3, 2).transpose(0, 1), torch.ones(6, 2, 4, 3), rec, None, **good)       # not contiguous
    for hm in (META(6, 4, 3, 16), META(1, 6, 1, 3, 16, 16), META(1, 6, 5, 3, 16, 16), META(1, 6, 4, 3, 16, 16, dtype=torch.float64)):
        with pytest.raises(ValueError):
            decode.decode_clip_3d_rays(hm, cams)
    with pytest.raises(ValueError):
        decode.decode_clip_3d_rays(META(2, 6, 4, 3, 16, 16), cams, META(12, 4, 4, 4))
    with pytest.raises(ValueError):
        decode.fit_ray_tracks(META(2, 6, 4, 3, 2), META(2, 6, 4, 3), cams, heatmap_size=(0, 64))
    assert hip.RAY_TRACK_RAY_SLOTS == 4 and hip.RAY_TRACK_SOLVE_SLOTS == 18


def test_cpu_tensors_are_refused():
    from egorear_amd import decode, hip
    cams = FS.rig()
    c, f = torch.zeros(1, 6, 4, 3, 2), torch.ones(1, 6, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.ray_track(c, f, FS.records(cams))
    with pytest.raises(ValueError, match="no CPU path"):
        decode.fit_ray_tracks(c, f, cams)
    with pytest.raises(ValueError, match="no CPU path"):
        decode.decode_clip_3d_rays(torch.zeros(6, 4, 3, 16, 16), cams)
    with pytest.raises((NotImplementedError, RuntimeError)):                         # the operator itself: no CPU kernel, no fallback
        decode.ray_track_op(c, f, FS.records(cams), None, 1 / 64, 1 / 64, 0.5, 0.0, 10.0, 0.0, 0, 8, 1e-10)


def test_the_operators_fake_gives_the_documented_shapes_and_dtypes():
    from egorear_amd import decode
    assert hasattr(torch.ops.egorear_amd, "ray_track")
    rec = FS.records(FS.rig()).to("meta")
    for (N, T, V, J), with_ctm in itertools.product(((1, 1, 2, 1), (2, 2, 3, 3), (3, 64, 4, 15), (1, 4096, 2, 2)), (False, True)):
        coords, conf = META(N, T, V, J, 2).requires_grad_(), META(N, T, V, J).requires_grad_()
        ctm = META(N, T, V, 4, 4) if with_ctm else None
        for huber, K in ((0.0, 0), (1.0, 4)):
            pose, valid, residual, weight, rays, energy = decode.ray_track_op(coords, conf, rec[:V], ctm, 1 / 64, 1 / 64, 0.5, 0.5, 10.0, huber, K, 8, 1e-10)
            assert pose.shape == (N, T, J, 3) and valid.shape == rays.shape == (N, T, J) and residual.shape == weight.shape == (N, T, V, J)
            assert energy.shape == (N, J) and valid.dtype == rays.dtype == torch.uint8
            assert all(t.dtype == torch.float32 and not t.requires_grad for t in (pose, residual, weight, energy))
    cams = FS.rig()
    track = decode.fit_ray_tracks(META(2, 6, 4, 15, 2).requires_grad_(), META(2, 6, 4, 15), cams, huber_cm=2.0, reweights=3)
    assert isinstance(track, decode.RayTrack3D) and track._fields == ("pose", "valid", "residual", "weight", "rays", "energy")
    assert track.pose.shape == (2, 6, 15, 3) and track.valid.dtype == torch.bool and track.rays.dtype == torch.uint8 and not track.pose.requires_grad
    one = decode.fit_ray_tracks(META(6, 3, 5, 2), META(6, 3, 5), cams[:3], META(6, 3, 4, 4))      # (T, V, J, 2): one clip
    assert one.pose.shape == (6, 5, 3) and one.valid.shape == one.rays.shape == (6, 5) and one.residual.shape == one.weight.shape == (6, 3, 5)
    assert one.energy.shape == (5,)
    joints, track = decode.decode_clip_3d_rays(META(2, 6, 4, 15, 64, 64), cams, huber_cm=1.0, reweights=4)
    assert isinstance(joints, decode.Joints2D) and isinstance(track, decode.RayTrack3D)
    assert joints.soft.shape == joints.hard.shape == (2, 6, 4, 15, 2) and joints.maxvals.shape == joints.valid.shape == (2, 6, 4, 15)
    assert track.pose.shape == (2, 6, 15, 3) and track.residual.shape == (2, 6, 4, 15) and track.energy.shape == (2, 15)
    joints, track = decode.decode_clip_3d_rays(META(6, 2, 5, 32, 32), cams[:2], META(6, 2, 4, 4))
    assert joints.soft.shape == (6, 2, 5, 2) and track.pose.shape == (6, 5, 3) and track.energy.shape == (5,)


def test_decode_clip_3d_rays_traces_as_one_graph_of_two_operators():
    import torch._dynamo as dynamo
    from egorear_amd import decode
    cams = FS.rig()

    def serving_side(hm):
        joints, track = decode.decode_clip_3d_rays(hm, cams, max_gap=4)
        return track.pose, track.valid, joints.valid

    hm = META(2, 6, 4, 15, 64, 64)
    serving_side(hm)                                                                   # (warms the record cache: the upload is not traced)
    dynamo.reset()
    ex = dynamo.explain(serving_side)(hm)
    assert ex.graph_break_count == 0 and ex.graph_count == 1, ex
    targets = [str(nd.target) for g in ex.graphs for nd in g.graph.nodes if nd.op == "call_function"]
    for name in ("egorear_amd.soft_argmax", "egorear_amd.ray_track"):
        assert sum(name in t for t in targets) == 1, (name, targets)


def test_the_library_exports_both_entries_and_refuses_bad_arguments_itself():
    from egorear_amd import hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ("egr_ray_track_f32", "egr_ray_track_workspace_bytes"):
        assert name in hip.EXPORTS and hasattr(lib, name), name
    size = hip.lib.egr_ray_track_workspace_bytes
    assert size(3, 64, 4, 15) == (4 * 4 + 18) * 64 * 3 * 15 * 8 and size(1, 1, 2, 1) == (4 * 2 + 18) * 8
    for shape in ((0, 8, 4, 2), (1, 0, 4, 2), (1, 4097, 4, 2), (1, 8, 1, 2), (1, 8, 5, 2), (1, 8, 4, 0), (1 << 10, 1 << 10, 4, 1 << 8)):
        assert size(*shape) == 0, shape
    p = ctypes.c_void_p(64)                                                            # pointers that are never followed

    def call(N=1, T=8, V=4, J=2, sx=1 / 64, sy=1 / 64, thr=0.5, lv=0.0, la=10.0, huber=0.0, K=0, gap=8, ratio=1e-10, ws=p, nbytes=1 << 40, out=p,
             coords=p):
        return hip.lib.egr_ray_track_f32(coords, p, p, None, N, T, V, J, sx, sy, thr, lv, la, huber, K, gap, ratio, ws, nbytes, out, p, p, p, p, p, None)

    assert call(ws=None) == hip.ENULL and call(out=None) == hip.ENULL and call(coords=None) == hip.ENULL
    for kw in ({"N": 0}, {"T": 0}, {"T": 4097}, {"J": 0}, {"V": 1}, {"V": 5}, {"N": 1 << 10, "T": 1 << 10, "J": 1 << 8}, {"lv": -1.0}, {"la": 0.0},
               {"la": float("nan")}, {"lv": float("inf")}, {"huber": -1.0}, {"huber": float("nan")}, {"K": -1}, {"K": 17}, {"K": 1},
               {"huber": 1.0}, {"gap": -1}, {"sx": 0.0}, {"sy": float("inf")}, {"thr": float("nan")}, {"ratio": -1.0}, {"ratio": 1.0},
               {"ratio": float("nan")}):
        assert call(**kw) == hip.EINVAL, kw
    assert call(nbytes=size(1, 8, 4, 2) - 8) == hip.EWORKSPACE

"""CPU-side checks of the temporal trajectory smoother (egorear_amd/decode.py): the statements of
tests/trajectory_statement.py, which the GPU tests compare the kernel with, are held to known answers - a line comes back as the line,
a constant as the constant, the banded elimination agrees with the dense solve, Huber's energy does not increase over the reweighting
rounds, the validity rule on its corners - and the Python layers are checked as far as they go without a device: every parameter and
shape error is a ValueError before any launch, the operators' fake implementations give the documented shapes and dtypes, the library
exports the two entries and refuses bad arguments itself."""
import ctypes

import pytest
import torch

import fisheye_statement as FS
import trajectory_statement as TS

META = lambda *s, **k: torch.empty(*s, device="meta", **k)


# --------------------------------------------------------------------------- the statements on known answers

@pytest.mark.parametrize("T", [3, 4, 5, 33, 129])
def test_observations_on_a_line_return_the_line(T):
    g = torch.Generator().manual_seed(T)
    N, J = 2, 4
    t = torch.arange(T, dtype=torch.float64).view(1, T, 1, 1)
    line = FS.random_points(N, J, g).unsqueeze(1) + 0.3 * torch.randn(N, 1, J, 3, generator=g, dtype=torch.float64) * t
    weight = 0.5 + torch.rand(N, T, J, generator=g, dtype=torch.float64)
    weight[torch.rand(N, T, J, generator=g) < 0.5] = 0.0
    weight[:, 0], weight[:, T - 1] = 1.0, 0.7                                         # any gaps, two observations at the least
    planted = line.clone()
    planted[weight == 0] = float("nan")                                               # what stands in a gap is never read
    for la in (1.0, 10.0, 1000.0):
        out = TS.smooth(planted, weight, None, 0.0, la, max_gap=T)
        w, z = TS.base_weights(planted, weight, None)
        err, eb = float((out["pose"] - line).abs().max()), float((TS.banded(w, z, 0.0, la) - line).abs().max())
        print(f"T {T} lambda_a {la}: |dense - line| {err:.3e}, |banded - line| {eb:.3e}, energy {float(out['energy'].max()):.3e}")
        assert err <= 1e-9 and eb <= 1e-9 and float(out["energy"].abs().max()) <= 1e-9
        assert bool(out["valid"].all()) and float(out["residual"].max()) <= 1e-9


def test_a_constant_track_returns_the_constant():
    g = torch.Generator().manual_seed(5)
    N, T, J = 2, 40, 3
    const = FS.random_points(N, J, g).unsqueeze(1).expand(N, T, J, 3).contiguous()
    obs = (torch.rand(N, T, J, generator=g) < 0.4).to(torch.uint8)
    obs[:, 7] = 1
    for lv in (0.1, 1.0, 100.0):
        out = TS.smooth(const, None, obs, lv, 0.0)
        w, z = TS.base_weights(const, None, obs)
        assert float((out["pose"] - const).abs().max()) <= 1e-9 and float((TS.banded(w, z, lv, 0.0) - const).abs().max()) <= 1e-9
        assert float(out["energy"].abs().max()) <= 1e-9


def test_the_banded_loop_agrees_with_the_dense_solve():
    worst = 0.0
    for shape in ((1, 1, 1), (2, 2, 3), (1, 3, 2), (2, 4, 15), (1, 5, 16), (3, 64, 15), (1, 65, 16), (2, 257, 5)):
        for case in ("dense", "gaps", "mask", "glitch"):
            sc = TS.scene(*shape, case)
            for lv, la in ((0.0, 10.0), (1.0, 0.0), (0.5, 100.0), (0.0, 1000.0)):
                out = TS.smooth(sc["pose"], sc["weight"], sc["obs"], lv, la)
                w, z = TS.base_weights(sc["pose"].double(), None if sc["weight"] is None else sc["weight"].double(), sc["obs"])
                x = torch.where(out["ok"].view(shape[0], 1, shape[2], 1), TS.banded(w, z, lv, la), torch.zeros_like(out["pose"]))
                worst = max(worst, float((x - out["pose"]).abs().max()))
    print(f"well-observed clips up to T = 257: |banded - dense| {worst:.3e} cm")
    assert worst <= 1e-6
    # the worst conditioning tried: three adjacent observations in T = 129 at lambda_a = 1000
    g = torch.Generator().manual_seed(9)
    pose = (FS.random_points(1, 4, g).unsqueeze(1) + torch.randn(1, 129, 4, 3, generator=g, dtype=torch.float64)).float()
    weight = torch.zeros(1, 129, 4)
    weight[:, 60:63] = 1.0
    cond = TS.condition(pose, weight, None, 0.0, 1000.0)
    out = TS.smooth(pose, weight, None, 0.0, 1000.0)
    w, z = TS.base_weights(pose.double(), weight.double(), None)
    err = float((TS.banded(w, z, 0.0, 1000.0) - out["pose"]).abs().max())
    print(f"three adjacent observations in T = 129, lambda_a 1000: cond(A) {cond:.3e}, |banded - dense| {err:.3e} cm")
    assert err <= 1e-6 and cond <= 1e10


def test_hubers_energy_does_not_increase_over_the_reweighting_rounds():
    sc = TS.scene(3, 64, 15, "glitch")
    for lv, la in ((0.0, 10.0), (0.5, 100.0)):
        E = [float(TS.smooth(sc["pose"], sc["weight"], None, lv, la, 1.0, K)["energy"].sum()) for K in range(1, 9)]
        w, z = TS.base_weights(sc["pose"].double(), sc["weight"].double(), None)
        plain = TS.smooth(sc["pose"], sc["weight"], None, lv, la)["pose"]             # K = 0: the plain solution, in Huber's energy
        E = [float(TS.energy(plain, z, w, lv, la, 1.0).sum())] + E
        print(f"lambda ({lv}, {la}): Huber's energy over K = 0..8: {[round(e, 4) for e in E]}")
        assert all(b <= a + 1e-9 * abs(a) for a, b in zip(E, E[1:])), E
        assert E[-1] < 0.6 * E[0]                                                      # and the glitches were worth reweighting
    # the reweighted track is closer to the truth than the plain one where the glitches are
    plain = TS.smooth(sc["pose"], sc["weight"], None, 0.0, 10.0)["pose"]
    robust = TS.smooth(sc["pose"], sc["weight"], None, 0.0, 10.0, 1.0, 4)["pose"]
    e_plain, e_robust = float((plain - sc["truth"]).norm(dim=-1).mean()), float((robust - sc["truth"]).norm(dim=-1).mean())
    print(f"mean error: plain {e_plain:.4f} cm, Huber K = 4 {e_robust:.4f} cm")
    assert e_robust < e_plain


def test_the_validity_rule_and_its_corners():
    one = torch.ones(1, 1, 1, 3)
    # T = 1: observed -> solvable under either penalty; not observed -> never
    for lv, la in ((0.0, 10.0), (1.0, 0.0)):
        out = TS.smooth(one, None, None, lv, la)
        assert bool(out["ok"].all()) and bool(out["valid"].all()) and torch.equal(out["pose"], one.double())
        out = TS.smooth(one, torch.zeros(1, 1, 1), None, lv, la)
        assert not bool(out["ok"].any()) and not bool(out["valid"].any()) and float(out["pose"].abs().max()) == 0.0
    # T = 2: with lambda_v = 0 nothing couples the frames, so both must be observed; with lambda_v > 0 one is enough
    two = torch.tensor([1.0, 2.0, 3.0]).view(1, 1, 1, 3) * torch.tensor([1.0, 2.0]).view(1, 2, 1, 1)
    half = torch.tensor([1, 0], dtype=torch.uint8).view(1, 2, 1)
    assert bool(TS.smooth(two, None, None, 0.0, 10.0)["ok"].all())
    out = TS.smooth(two, None, half, 0.0, 10.0, max_gap=5)
    assert not bool(out["ok"].any()) and not bool(out["valid"].any()) and float(out["energy"].abs().max()) == 0.0
    out = TS.smooth(two, None, half, 1.0, 0.0, max_gap=0)
    assert bool(out["ok"].all()) and out["valid"].flatten().tolist() == [True, False]
    assert torch.allclose(out["pose"][0, 1, 0], two[0, 0, 0].double(), atol=1e-12)    # the gap takes its neighbour's place
    assert bool(TS.smooth(two, None, half, 1.0, 0.0, max_gap=1)["valid"].all())
    # T >= 3 with lambda_v = 0: two observations fix the line, one does not
    obs = torch.zeros(1, 9, 1, dtype=torch.uint8)
    obs[0, 2] = obs[0, 5] = 1
    pose = torch.randn(1, 9, 1, 3, generator=torch.Generator().manual_seed(1))
    out = TS.smooth(pose, None, obs, 0.0, 10.0, max_gap=2)
    assert bool(out["ok"].all()) and out["valid"].flatten().tolist() == [True] * 8 + [False]
    obs[0, 5] = 0
    assert not bool(TS.smooth(pose, None, obs, 0.0, 10.0)["ok"].any()) and bool(TS.smooth(pose, None, obs, 0.1, 10.0)["ok"].all())
    # a weight that is zero, negative or not finite, and a pose that is not finite, each make a gap
    weight = torch.ones(1, 9, 1)
    weight[0, 0], weight[0, 1], weight[0, 3] = 0.0, float("nan"), -1.0
    pose[0, 4, 0, 1] = float("inf")
    w, z = TS.base_weights(pose, weight, None)
    assert (w.flatten() > 0).tolist() == [False, False, True, False, False, True, True, True, True] and bool(torch.isfinite(z).all())


def test_the_statement_is_stationary_and_its_gradients_are_those_of_the_formula():
    sc = TS.scene(2, 17, 3, "gaps")
    lv, la = 0.5, 100.0
    p64, w64 = sc["pose"].double().requires_grad_(), sc["weight"].double().requires_grad_()
    out = TS.smooth(p64, w64, None, lv, la)
    g, allowed, ok = TS.stationarity(out["pose"].detach().float(), sc["weight"], None, sc["pose"], lv, la)
    ratio = float((g.abs().amax(-1) / allowed).max())
    print(f"float64 statement rounded to fp32: largest |g_i| / allowance {ratio:.3g}")
    assert bool(ok.all()) and ratio <= 0.5 + 1e-6                                      # rounding the minimiser costs half the sum
    gx = torch.randn(out["pose"].shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    (out["pose"] * gx).sum().backward()
    w, z = TS.base_weights(sc["pose"].double(), sc["weight"].double(), None)
    A = TS.matrices(w, ok, lv, la)
    u = TS.solve_tracks(A, gx.permute(0, 2, 1, 3)).permute(0, 2, 1, 3)
    assert float((p64.grad - w.unsqueeze(-1) * u).abs().max()) <= 1e-10
    want = torch.where(w > 0, (u * (z - out["pose"].detach())).sum(-1), torch.zeros_like(w))
    assert float((w64.grad - want).abs().max()) <= 1e-10


def test_every_case_of_the_generator_is_what_it_says():
    for shape in ((2, 4, 15), (3, 64, 15), (2, 257, 5)):
        N, T, J = shape
        for case in TS.CASES:
            sc = TS.scene(*shape, case)
            w, z = TS.base_weights(sc["pose"], sc["weight"], sc["obs"])
            seen = (w > 0).sum(1)
            assert sc["pose"].dtype == torch.float32 and tuple(sc["pose"].shape) == (N, T, J, 3)
            if case in ("dense", "glitch"):
                assert int(seen.min()) == T
            if case == "gaps" and T > 20:
                assert 0.4 * T < float(seen.float().mean()) < 0.8 * T
            if case == "ends":
                assert not bool((w[:, :T // 4] > 0).any()) and not bool((w[:, T - T // 4:] > 0).any()) and int(seen.min()) == T - 2 * (T // 4)
            if case == "sparse":
                assert sorted(set(seen.flatten().tolist())) == [0, 1, 2]
            if case == "mask":
                assert sc["weight"] is None and sc["obs"].dtype == torch.uint8 and int(seen.min()) < T
            if case == "nonfinite":
                bad = ~torch.isfinite(sc["pose"]).all(-1) | ~torch.isfinite(sc["weight"])
                assert int((bad & (sc["weight"] == 0)).sum()) > 0 and int((bad & (sc["weight"] != 0)).sum()) > 0
                tw, tz = TS.base_weights(sc["twin"]["pose"], sc["twin"]["weight"], None)
                assert torch.equal(tw, w) and torch.equal(tz, z) and bool(torch.isfinite(sc["twin"]["pose"]).all())
            if case == "glitch":
                jump = (sc["pose"].double() - sc["truth"]).norm(dim=-1)
                assert int((jump > 20.0).sum()) == 3 * N * J and float(jump.max()) < 55.0


# --------------------------------------------------------------------------- the Python layers without a device

def test_every_bad_parameter_and_shape_is_a_value_error_before_any_launch():
    from egorear_amd import decode, hip
    pose, weight, obs = torch.zeros(2, 6, 3, 3), torch.ones(2, 6, 3), torch.ones(2, 6, 3, dtype=torch.uint8)
    good = dict(vel_weight=0.0, accel_weight=10.0, huber=0.0, reweights=0, max_gap=8)
    bad = ({"vel_weight": -1.0}, {"accel_weight": -1.0}, {"accel_weight": 0.0}, {"vel_weight": float("nan")}, {"accel_weight": float("inf")},
           {"huber": -0.5}, {"huber": float("nan")}, {"reweights": -1}, {"reweights": 17}, {"reweights": 2}, {"huber": 1.0},
           {"reweights": 1.0, "huber": 1.0}, {"reweights": True, "huber": 1.0}, {"max_gap": -1}, {"max_gap": 1.5})
    for kw in bad:
        args = dict(good, **kw)
        for p, w, o in ((pose, weight, obs), (META(2, 6, 3, 3), META(2, 6, 3), None)):      # host tensors and meta tensors alike
            with pytest.raises(ValueError):
                hip.trajectory_smooth(p, w, o, **args)
        with pytest.raises(ValueError):
            decode.smooth_trajectory(META(2, 6, 3, 3), None, None, args["accel_weight"], args["vel_weight"], args["huber"], args["reweights"],
                                     args["max_gap"])
        with pytest.raises(ValueError):
            decode.decode_clip_3d(META(1, 6, 4, 3, 16, 16), FS.rig(), accel_weight=args["accel_weight"], vel_weight=args["vel_weight"],
                                  huber_cm=args["huber"], reweights=args["reweights"], max_gap=args["max_gap"])
    shapes = ((META(2, 6, 3), None, None), (META(2, 6, 3, 2), None, None), (META(0, 6, 3, 3), None, None), (META(1, 4097, 1, 3), None, None),
              (META(2, 6, 3, 3, dtype=torch.float64), None, None), (META(2, 6, 3, 3), META(2, 6, 4), None),
              (META(2, 6, 3, 3), META(2, 6, 3, dtype=torch.float64), None), (META(2, 6, 3, 3), None, META(2, 6, 3)),
              (META(2, 6, 3, 3), None, META(2, 5, 3, dtype=torch.uint8)), (META(1 << 16, 1 << 10, 1 << 5, 3), None, None))
    for p, w, o in shapes:
        with pytest.raises(ValueError):
            hip.trajectory_smooth(p, w, o, **good)
        with pytest.raises(ValueError):
            decode.trajectory_smooth_op(p, w, o, 0.0, 10.0, 0.0, 0, 8)
        if p.dim() == 4:
            with pytest.raises(ValueError):
                decode.smooth_trajectory(p, w, o)
    assert hip.TRAJECTORY_MAX_T == 4096
    for g in (META(2, 6, 3), META(2, 6, 3, 3, dtype=torch.float64), META(2, 5, 3, 3)):
        with pytest.raises(ValueError):
            hip.trajectory_smooth_bwd(META(2, 6, 3, 3), None, None, g, 0.0, 10.0)
    with pytest.raises(ValueError):
        hip.trajectory_smooth_bwd(META(2, 6, 3, 3), None, None, META(2, 6, 3, 3), 0.0, 0.0)
    for hm in (META(6, 4, 3, 16), META(1, 6, 1, 3, 16, 16), META(1, 6, 5, 3, 16, 16)):
        with pytest.raises(ValueError):
            decode.decode_clip_3d(hm, FS.rig()[:min(max(hm.shape[2] if hm.dim() == 6 else 4, 2), 4)])
    with pytest.raises(ValueError):
        decode.decode_clip_3d(META(2, 6, 4, 3, 16, 16), FS.rig(), META(12, 4, 4, 4))


def test_cpu_tensors_are_refused():
    from egorear_amd import decode, hip
    pose = torch.zeros(1, 6, 3, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.trajectory_smooth(pose)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.trajectory_smooth_bwd(pose, None, None, pose)
    with pytest.raises(ValueError, match="no CPU path"):
        decode.smooth_trajectory(pose)
    with pytest.raises(ValueError, match="no CPU path"):
        decode.decode_clip_3d(torch.zeros(6, 4, 3, 16, 16), FS.rig())
    with pytest.raises((NotImplementedError, RuntimeError)):                         # the operator itself: no CPU kernel, no fallback
        decode.trajectory_smooth_op(pose, None, None, 0.0, 10.0, 0.0, 0, 8)
    with pytest.raises((NotImplementedError, RuntimeError)):
        decode.trajectory_smooth_bwd_op(pose, None, None, pose, 0.0, 10.0)


def test_the_operators_fakes_give_the_documented_shapes_and_dtypes():
    from egorear_amd import decode
    for name in ("trajectory_smooth", "trajectory_smooth_bwd"):
        assert hasattr(torch.ops.egorear_amd, name), name
    for N, T, J in ((1, 1, 1), (2, 2, 3), (3, 64, 15), (1, 4096, 2)):
        for with_w, with_o in ((True, True), (False, False), (True, False)):
            pose = META(N, T, J, 3).requires_grad_()
            weight = META(N, T, J).requires_grad_() if with_w else None
            obs = META(N, T, J, dtype=torch.uint8) if with_o else None
            out, valid, residual, used, energy = decode.trajectory_smooth_op(pose, weight, obs, 0.5, 10.0, 0.0, 0, 8)
            assert out.shape == (N, T, J, 3) and valid.shape == residual.shape == used.shape == (N, T, J) and energy.shape == (N, J)
            assert valid.dtype == torch.uint8 and all(t.dtype == torch.float32 for t in (out, residual, used, energy))
            assert out.requires_grad and not residual.requires_grad and not used.requires_grad and not energy.requires_grad
            robust = decode.trajectory_smooth_op(pose, weight, obs, 0.5, 10.0, 1.0, 4, 8)
            assert robust[0].shape == (N, T, J, 3) and not any(t.requires_grad for t in robust)       # no gradient through the Huber form
            g_in, g_w = decode.trajectory_smooth_bwd_op(pose.detach(), None if weight is None else weight.detach(), obs, META(N, T, J, 3), 0.5, 10.0)
            assert g_in.shape == (N, T, J, 3) and g_w.shape == ((N, T, J) if with_w else (0,)) and g_in.dtype == g_w.dtype == torch.float32
            track = decode.smooth_trajectory(pose, weight, None if obs is None else obs.view(torch.bool), huber_cm=2.0, reweights=3)
            assert isinstance(track, decode.Track3D) and track._fields == ("pose", "valid", "residual", "weight", "energy")
            assert track.pose.shape == (N, T, J, 3) and track.valid.dtype == torch.bool and track.energy.shape == (N, J)
    clip = decode.smooth_trajectory(META(7, 5, 3))                                     # (T, J, 3): one clip
    assert clip.pose.shape == (7, 5, 3) and clip.valid.shape == clip.residual.shape == clip.weight.shape == (7, 5) and clip.energy.shape == (5,)
    cams = FS.rig()
    joints, track = decode.decode_clip_3d(META(2, 6, 4, 15, 64, 64), cams, huber_cm=1.0, reweights=4)
    assert isinstance(joints, decode.Joints3D) and isinstance(track, decode.Track3D)
    assert joints.pose.shape == track.pose.shape == (2, 6, 15, 3) and joints.residual.shape == (2, 6, 4, 15) and joints.valid.shape == (2, 6, 15)
    assert track.valid.shape == (2, 6, 15) and track.energy.shape == (2, 15)
    joints, track = decode.decode_clip_3d(META(6, 3, 5, 32, 32), cams[:3], META(6, 3, 4, 4))
    assert joints.pose.shape == track.pose.shape == (6, 5, 3) and joints.cost.shape == (6, 5) and track.energy.shape == (5,)


def test_decode_clip_3d_traces_as_one_graph_of_three_launches():
    import torch._dynamo as dynamo
    from egorear_amd import decode
    cams = FS.rig()

    def serving_side(hm):
        joints, track = decode.decode_clip_3d(hm, cams, max_gap=4)
        return track.pose, track.valid, joints.valid

    hm = META(2, 6, 4, 15, 64, 64)
    serving_side(hm)                                                                   # (warms the record cache: the upload is not traced)
    dynamo.reset()
    ex = dynamo.explain(serving_side)(hm)
    assert ex.graph_break_count == 0 and ex.graph_count == 1, ex
    targets = [str(nd.target) for g in ex.graphs for nd in g.graph.nodes if nd.op == "call_function"]
    for name in ("egorear_amd.soft_argmax", "egorear_amd.triangulate", "egorear_amd.trajectory_smooth"):
        assert sum(name in t for t in targets) == 1, (name, targets)


def test_the_library_exports_the_two_entries_and_refuses_bad_arguments_itself():
    from egorear_amd import hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ("egr_trajectory_smooth_f32", "egr_trajectory_smooth_bwd_f32"):
        assert name in hip.EXPORTS and hasattr(lib, name), name
    p = ctypes.c_void_p(64)                                                            # pointers that are never followed

    def fwd(N=1, T=8, J=2, lv=0.0, la=10.0, huber=0.0, K=0, gap=8, ws=p, out=p):
        return hip.lib.egr_trajectory_smooth_f32(p, None, None, N, T, J, lv, la, huber, K, gap, ws, out, p, p, p, p, None)

    assert fwd(ws=None) == hip.ENULL and fwd(out=None) == hip.ENULL
    for kw in ({"N": 0}, {"T": 0}, {"T": 4097}, {"J": 0}, {"N": 1 << 16, "T": 1 << 10, "J": 1 << 5}, {"lv": -1.0}, {"la": 0.0},
               {"la": float("nan")}, {"lv": float("inf")}, {"huber": -1.0}, {"huber": float("nan")}, {"K": -1}, {"K": 17}, {"K": 1},
               {"huber": 1.0}, {"gap": -1}):
        assert fwd(**kw) == hip.EINVAL, kw
    bwd = lambda **kw: hip.lib.egr_trajectory_smooth_bwd_f32(p, None, None, kw.get("g", p), 1, kw.get("T", 8), 2, kw.get("lv", 0.0),
                                                             kw.get("la", 10.0), p, p, None, None)
    assert bwd(g=None) == hip.ENULL
    for kw in ({"T": 0}, {"T": 4097}, {"la": 0.0}, {"lv": -1.0}):
        assert bwd(**kw) == hip.EINVAL, kw

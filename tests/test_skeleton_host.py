"""CPU-side checks of the bone-length-constrained skeleton fit (egorear_amd/decode.py): the three operators are registered
with fake implementations and no gradient, the public functions give the documented shapes on meta tensors, `decode_joints_3d_skeleton`
traces under Dynamo as one graph of three launches, bad tables, parameters and CPU tensors are refused before any launch, the library
exports the three entries - and the statements of tests/skeleton_statement.py, which the GPU tests compare the kernels with, are
themselves held to known answers here."""
import ctypes

import pytest
import torch

import fisheye_statement as FS
import skeleton_statement as SS

# (B, V, J, rw)
META_SHAPES = ((2, 4, 15, False), (1, 2, 5, False), (3, 3, 2, False), (2, 4, 16, True), (1, 4, 1, False))


def _meta(B, V, J, rw):
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)
    return {"coords": m(B, V, J, 2), "conf": m(B, V, J), "cams": m(V, 30), "ctm": m(B, V, 4, 4) if rw else None,
            "L": m(B, J) if rw else m(J), "init": m(B, J, 3), "ok": m(B, J, dtype=torch.uint8)}


def _fit_op(decode, a, parents, **kw):
    args = dict(sx=1 / 64, sy=1 / 64, threshold=0.5, min_det_ratio=1e-6, bone_weight=1.0, prior_weight=0.0, iterations=16)
    args.update(kw)
    return decode.skeleton_fit_op(a["coords"], a["conf"], a["cams"], a["ctm"], parents, a["L"], a["init"], a["ok"], args["sx"], args["sy"],
                                  args["threshold"], args["min_det_ratio"], args["bone_weight"], args["prior_weight"], args["iterations"])


def test_operators_are_registered_with_fake_implementations_and_no_gradient():
    from egorear_amd import decode
    for name in ("skeleton_fit", "bone_lengths", "skeleton_resize"):
        assert hasattr(torch.ops.egorear_amd, name), name
    for B, V, J, rw in META_SHAPES:
        a = _meta(B, V, J, rw)
        a["coords"].requires_grad_()
        a["init"].requires_grad_()
        parents = list(SS.default_parents(J))
        out = _fit_op(decode, a, parents)
        pose, ray_cost, bone, valid, energy0, energy, grad, steps = out
        assert pose.shape == (B, J, 3) and ray_cost.shape == bone.shape == valid.shape == (B, J)
        assert energy0.shape == energy.shape == grad.shape == steps.shape == (B,)
        assert valid.dtype == torch.uint8 and steps.dtype == torch.int32
        assert all(t.dtype == torch.float32 for t in (pose, ray_cost, bone, energy0, energy, grad))
        assert not any(t.requires_grad for t in out)
        length, spread, count = decode.bone_lengths_op(pose, valid, parents)
        assert length.shape == spread.shape == count.shape == (J,) and count.dtype == torch.int32 and length.dtype == torch.float32
        moved = decode.skeleton_resize_op(a["init"], valid, a["L"], parents)
        assert moved.shape == (B, J, 3) and moved.dtype == torch.float32 and not moved.requires_grad


def test_public_functions_give_the_documented_shapes_on_meta():
    from egorear_amd import decode
    cams = FS.rig()
    for B, V, J, rw in META_SHAPES:
        a = _meta(B, V, J, rw)
        parents = None if J in (15, 16) else SS.default_parents(J)
        fit = decode.fit_skeleton(a["coords"], a["conf"], cams[:V], a["L"], a["init"], a["ok"], parents, a["ctm"])
        assert isinstance(fit, decode.Skeleton3D)
        assert fit._fields == ("pose", "ray_cost", "bone", "valid", "energy0", "energy", "grad", "steps")
        assert fit.pose.shape == (B, J, 3) and fit.valid.shape == (B, J) and fit.valid.dtype == torch.bool and fit.steps.dtype == torch.int32
        no_flags = decode.fit_skeleton(a["coords"], a["conf"], cams[:V], a["L"], a["init"], None, parents, a["ctm"], prior_weight=1e-3,
                                       iterations=48)
        assert no_flags.energy.shape == (B,)
        stats = decode.estimate_bone_lengths(fit.pose, fit.valid, parents)
        assert isinstance(stats, decode.BoneStats) and stats._fields == ("length", "spread", "count") and stats.length.shape == (J,)
        assert decode.resize_skeleton(fit.pose, fit.valid, stats.length, parents).shape == (B, J, 3)
        hm = torch.empty(B, V, J, 64, 64, device="meta")
        sk, tri, j2 = decode.decode_joints_3d_skeleton(hm, cams[:V], a["L"], parents=parents, coord_trans_mat=a["ctm"])
        assert isinstance(sk, decode.Skeleton3D) and isinstance(tri, decode.Joints3D) and isinstance(j2, decode.Joints2D)
        assert sk.pose.shape == tri.pose.shape == (B, J, 3) and j2.soft.shape == (B, V, J, 2)
        sk2, _, _ = decode.decode_joints_3d_skeleton(hm, cams[:V], a["L"], a["init"], a["ok"].view(torch.bool), parents, a["ctm"])
        assert sk2.pose.shape == (B, J, 3)
    with pytest.raises(ValueError, match="explicit parent table"):
        decode.fit_skeleton(torch.empty(1, 4, 7, 2, device="meta"), torch.empty(1, 4, 7, device="meta"), cams, torch.empty(7, device="meta"),
                            torch.empty(1, 7, 3, device="meta"))


def test_decode_joints_3d_skeleton_traces_as_one_graph_of_three_launches():
    import torch._dynamo as dynamo
    from egorear_amd import decode
    lin = torch.nn.Conv2d(4, 15, 1, device="meta")
    cams = FS.rig()
    L = torch.empty(15, device="meta")

    def serving_side(feat, prev, prev_ok):
        hm = lin(feat).view(2, 4, 15, 64, 64)
        sk, tri, _ = decode.decode_joints_3d_skeleton(hm, cams, L, prev, prev_ok, iterations=48)
        return sk.pose, sk.valid, tri.valid

    feat, prev, prev_ok = torch.empty(8, 4, 64, 64, device="meta"), torch.empty(2, 15, 3, device="meta"), torch.empty(2, 15, dtype=torch.bool,
                                                                                                                      device="meta")
    pose, valid, _ = serving_side(feat, prev, prev_ok)            # (also warms the record cache: the upload is not part of a graph)
    assert pose.shape == (2, 15, 3) and not pose.requires_grad and valid.dtype == torch.bool
    dynamo.reset()
    ex = dynamo.explain(serving_side)(feat, prev, prev_ok)
    assert ex.graph_break_count == 0 and ex.graph_count == 1, ex
    targets = [str(nd.target) for g in ex.graphs for nd in g.graph.nodes if nd.op == "call_function"]
    for name in ("egorear_amd.soft_argmax", "egorear_amd.triangulate", "egorear_amd.skeleton_fit"):
        assert sum(name in t for t in targets) == 1, (name, targets)


def test_bad_tables_and_parameters_are_refused_before_any_launch():
    from egorear_amd import decode, hip
    cams = FS.rig()
    a = _meta(2, 4, 5, False)
    good = [0, 0, 1, 1, 3]
    _fit_op(decode, a, good)
    for parents in ([0, 1, 1, 1, 3], [0, 0, 2, 1, 3], [0, 0, 1, 1, 4], [1, 0, 1, 1, 3], [0, 0, 1, 1, 5], [0, 0, -1, 1, 3], [0, 0, 1, 1],
                    [0, 0, 1, 1, 3, 4], [0, 0, 1.5, 1, 3], "abcde"):
        with pytest.raises(ValueError):
            hip._parents("test", parents, 5)
        with pytest.raises(ValueError):
            decode.fit_skeleton(a["coords"], a["conf"], cams, a["L"], a["init"], a["ok"], parents)
        if not isinstance(parents, str) and all(isinstance(v, int) for v in parents):
            with pytest.raises(ValueError):
                _fit_op(decode, a, parents)
            with pytest.raises(ValueError):
                decode.estimate_bone_lengths(a["init"], a["ok"], parents)
            with pytest.raises(ValueError):
                decode.resize_skeleton(a["init"], a["ok"], a["L"], parents)
    with pytest.raises(ValueError):
        hip._parents("test", torch.tensor([0.0, 0.0]), 2)
    assert list(hip._parents("test", torch.tensor([0, 0, 1]), 3)) == [0, 0, 1]
    b = _meta(1, 4, 17, False)                                                       # J = 17: one more than a lane a joint allows
    with pytest.raises(ValueError):
        decode.fit_skeleton(b["coords"], b["conf"], cams, b["L"], b["init"], b["ok"], list(range(-1, 16)))
    with pytest.raises(ValueError):
        decode.fit_skeleton(b["coords"], b["conf"], cams, b["L"], b["init"], b["ok"], [0] + list(range(16)))
    with pytest.raises(ValueError):
        decode.estimate_bone_lengths(b["init"], b["ok"], [0] + list(range(16)))
    for kw in ({"bone_weight": -1.0}, {"bone_weight": float("nan")}, {"bone_weight": float("inf")}, {"prior_weight": -1e-3},
               {"prior_weight": float("nan")}, {"iterations": 0}, {"iterations": 257}, {"iterations": 16.0}, {"iterations": True},
               {"min_det_ratio": -1.0}, {"heatmap_size": (0, 64)}):
        with pytest.raises(ValueError):
            decode.fit_skeleton(a["coords"], a["conf"], cams, a["L"], a["init"], a["ok"], good, **kw)
        if "heatmap_size" not in kw:
            if type(kw.get("iterations", 1)) is int:                                 # (the operator's schema types its own arguments)
                with pytest.raises(ValueError):
                    _fit_op(decode, a, good, **kw)
            with pytest.raises(ValueError):
                decode.decode_joints_3d_skeleton(torch.empty(2, 4, 5, 16, 16, device="meta"), cams, a["L"], parents=good, **kw)
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)
    for bad in ({"L": m(4)}, {"L": m(3, 5)}, {"L": m(5, dtype=torch.float64)}, {"init": m(2, 5, 2)}, {"init": m(2, 4, 3)},
                {"init": m(2, 5, 3, dtype=torch.float64)}, {"ok": m(2, 5)}, {"ok": m(2, 4, dtype=torch.uint8)}, {"conf": m(2, 4, 4)},
                {"coords": m(2, 4, 5, 3)}, {"cams": m(4, 17)}, {"ctm": m(2, 3, 4, 4)}, {"coords": m(2, 4, 5, 2, dtype=torch.float64)}):
        with pytest.raises(ValueError):
            _fit_op(decode, dict(a, **bad), good)
    with pytest.raises(ValueError):
        decode.fit_skeleton(a["coords"][:, :1], a["conf"][:, :1], cams[:1], a["L"], a["init"], a["ok"], good)      # one view
    for pose, valid, L in ((m(2, 5, 2), a["ok"], a["L"]), (m(2, 5), a["ok"], a["L"]), (a["init"], m(2, 4, dtype=torch.uint8), a["L"]),
                           (a["init"], m(2, 5), a["L"]), (a["init"].double(), a["ok"], a["L"]), (a["init"], a["ok"], m(6)),
                           (m(0, 5, 3), m(0, 5, dtype=torch.uint8), a["L"])):
        with pytest.raises(ValueError):
            decode.resize_skeleton(pose, valid, L, good)
        with pytest.raises(ValueError):
            decode.skeleton_resize_op(pose, valid, L, good)
        if L is a["L"]:
            with pytest.raises(ValueError):
                decode.estimate_bone_lengths(pose, valid, good)
            with pytest.raises(ValueError):
                decode.bone_lengths_op(pose, valid, good)
    with pytest.raises(ValueError):
        decode.decode_joints_3d_skeleton(torch.empty(2, 4, 5, 16, 16, device="meta"), cams, a["L"], m(2, 4, 3), parents=good)


def test_cpu_tensors_are_refused():
    from egorear_amd import decode, hip
    cams = FS.rig()
    good = [0, 0, 1]
    coords, conf, L, init, ok = torch.zeros(1, 4, 3, 2), torch.ones(1, 4, 3), torch.ones(3), torch.zeros(1, 3, 3), torch.ones(1, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no CPU path"):
        decode.fit_skeleton(coords, conf, cams, L, init, ok, good)
    with pytest.raises(ValueError, match="no CPU path"):
        decode.estimate_bone_lengths(init, ok, good)
    with pytest.raises(ValueError, match="no CPU path"):
        decode.resize_skeleton(init, ok, L, good)
    with pytest.raises(ValueError, match="no CPU path"):
        decode.decode_joints_3d_skeleton(torch.zeros(1, 4, 3, 16, 16), cams, L, parents=good)
    with pytest.raises((NotImplementedError, RuntimeError)):                         # the operators themselves: no CPU kernel, no fallback
        decode.skeleton_fit_op(coords, conf, torch.zeros(4, 30), None, good, L, init, ok, 1 / 64, 1 / 64, 0.5, 1e-6, 1.0, 0.0, 16)
    with pytest.raises((NotImplementedError, RuntimeError)):
        decode.bone_lengths_op(init, ok, good)
    with pytest.raises((NotImplementedError, RuntimeError)):
        decode.skeleton_resize_op(init, ok, L, good)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.skeleton_fit(coords, conf, torch.zeros(4, 30), None, good, L, init, ok)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.bone_lengths(init, ok, good)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.skeleton_resize(init, ok, L, good)


def test_the_library_exports_the_three_entries_and_refuses_bad_arguments_itself():
    from egorear_amd import hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ("egr_skeleton_fit_f32", "egr_bone_lengths_f32", "egr_skeleton_resize_f32"):
        assert name in hip.EXPORTS and hasattr(lib, name), name
    # the entries validate before they launch: with pointers that are never followed, every refusal is a return code
    p = ctypes.c_void_p(64)
    table = lambda *v: (ctypes.c_int32 * len(v))(*v)

    def fit(parents, J=3, V=4, lam=1.0, rho=0.0, iterations=16):
        return hip.lib.egr_skeleton_fit_f32(p, p, p, None, parents, p, 0, p, p, 1, V, J, 1.0, 1.0, 0.5, 1e-6, lam, rho, iterations, p, p, p, p, p,
                                            p, p, p, None)

    assert fit(None) == hip.ENULL
    for kw in ({"parents": table(0, 1, 1)}, {"parents": table(1, 0, 1)}, {"parents": table(0, 0, 2)}, {"parents": table(0, 0, -1)},
               {"parents": table(*([0] * 17)), "J": 17}, {"parents": table(0, 0, 1), "V": 1}, {"parents": table(0, 0, 1), "lam": -1.0},
               {"parents": table(0, 0, 1), "lam": float("nan")}, {"parents": table(0, 0, 1), "rho": float("inf")},
               {"parents": table(0, 0, 1), "iterations": 0}, {"parents": table(0, 0, 1), "iterations": 257}):
        assert fit(**kw) == hip.EINVAL, kw
    assert hip.lib.egr_bone_lengths_f32(p, p, table(0, 1), 1, 2, p, p, p, None) == hip.EINVAL
    assert hip.lib.egr_bone_lengths_f32(p, p, table(0, 0), 0, 2, p, p, p, None) == hip.EINVAL
    assert hip.lib.egr_skeleton_resize_f32(p, p, table(0, 1), p, 0, 1, 2, ctypes.c_void_p(128), None) == hip.EINVAL
    assert hip.lib.egr_skeleton_resize_f32(p, p, table(0, 0), p, 0, 1, 2, p, None) == hip.EINVAL          # in place
    assert hip.lib.egr_skeleton_resize_f32(p, p, None, p, 0, 1, 2, ctypes.c_void_p(128), None) == hip.ENULL


def test_the_15_joint_table_is_the_16_joint_table_without_the_head():
    from egorear_amd import decode
    sixteen = decode.SKELETON_PARENTS_16
    assert tuple(sixteen) == SS.PARENTS_16 and len(sixteen) == 16
    # joint 0 (the head) hangs on nothing else; without it joint i becomes i - 1 and the neck, whose parent it was, the root
    assert all(p != 0 for p in sixteen[2:])
    fifteen = tuple(0 if j == 1 else sixteen[j] - 1 for j in range(1, 16))
    assert tuple(decode.HEATMAP_PARENTS_15) == fifteen == SS.parents_15()
    assert fifteen[0] == 0 and all(0 <= fifteen[j] < j for j in range(1, 15))


# --------------------------------------------------------------------------- the statements, on the CPU

def _problem(sc, lam, rho=0.0, conf=None, coords=None, dt=torch.float64):
    conf = sc["conf"] if conf is None else conf
    coords = sc["coords"] if coords is None else coords
    return SS.Problem(coords.to(dt), conf.to(dt), sc["rec"], sc["ctm"], sc["parents"], sc["lengths"].to(dt), sc["init"].to(dt), sc["init_ok"],
                      lam, rho)


@pytest.mark.parametrize("B,V,J,rw", [(3, 4, 15, False), (2, 4, 16, True), (2, 2, 5, False)])
def test_without_bones_and_prior_the_fit_is_the_triangulation(B, V, J, rw):
    sc = SS.scene(B, V, J, rw)
    conf = sc["conf"].clone()
    conf[0, 1:, J - 1] = 0.3                     # one joint is not triangulable: one view
    conf[B - 1, :, 1] = 0.3                      # another has no view
    pr = _problem(sc, 0.0, conf=conf)
    out, E0, grad, steps = SS.fit_statement(pr, 16)
    pts, cost, _, ok = FS.statement(sc["coords"].double(), conf.double(), sc["rec"], sc["ctm"], 1.0 / SS.HM, 1.0 / SS.HM)
    assert int((~ok).sum()) == 2
    # (the bone of the one-view joint is constrained and its parent active, so it takes part; lambda = 0 leaves it on its ray)
    assert bool(out["valid"][ok].all()) and not bool(out["valid"][B - 1, 1])
    err = float((out["pose"] - pts)[ok].abs().max())
    print(f"({B}, {V}, {J}): |fit - triangulation| {err:.3e} cm over {int(ok.sum())} joints, |cost| {float((out['ray_cost'] - cost)[ok].abs().max()):.3e}")
    assert err < 1e-9 and float((out["ray_cost"] - cost)[ok].abs().max()) < 1e-9
    assert bool((out["energy"] <= E0).all())


@pytest.mark.parametrize("B,V,J,rw,chain", [(2, 4, 15, False, False), (2, 4, 16, True, False), (2, 2, 5, False, True)])
def test_noise_free_projections_and_true_lengths_return_the_true_pose(B, V, J, rw, chain):
    sc = SS.scene(B, V, J, rw, chain, noise=0.0)
    exact = FS.project(sc["pts"], sc["rec"], sc["ctm"]) * SS.HM                       # float64: not rounded to fp32
    sc["lengths"] = (sc["pts"] - sc["pts"][:, list(sc["parents"])]).norm(dim=-1)[0]
    for lam, rho in ((1.0, 0.0), (10.0, 0.0), (1.0, 1e-3)):
        pr = _problem(sc, lam, rho, coords=exact)
        out, E0, grad, steps = SS.fit_statement(pr, 32)
        err = float((out["pose"] - sc["pts"]).norm(dim=-1).max())
        print(f"({B}, {V}, {J}) lambda {lam} rho {rho}: |fit - truth| {err:.3e} cm, energy {float(E0.max()):.3e} -> {float(out['energy'].max()):.3e}")
        assert bool(out["valid"].all())
        if rho == 0.0:
            assert err < 1e-7 and float(out["energy"].max()) < 1e-12
        else:                                    # the prior pulls every joint from the truth, where the rest vanishes, towards its init
            assert 1e-4 < err < 3.0 and bool((out["energy"] < E0).all())
    # one joint left a single view: the triangulation has nothing for it, the fit returns it.  (Its ray meets the sphere of its bone
    # twice, and both points have energy 0: from 3 cm off the fit lands on one of them, from 0.5 cm off on the true one.)
    leaf = SS.limb_joint(sc["parents"])
    conf = SS.keep_views(sc, leaf, 1)
    ok = FS.statement(exact, conf.double(), sc["rec"], sc["ctm"], 1.0 / SS.HM, 1.0 / SS.HM)[3]
    assert not bool(ok[:, leaf].any()) and int((~ok).sum()) == B
    out = SS.fit_statement(_problem(sc, 1.0, conf=conf, coords=exact), 48)[0]
    assert bool(out["valid"].all()) and float(out["energy"].max()) < 1e-12
    assert float((out["bone"][:, leaf] - sc["lengths"][leaf]).abs().max()) < 1e-7
    sc["init"] = (sc["pts"] + (sc["init"].double() - sc["pts"]) / 6.0).float()
    out = SS.fit_statement(_problem(sc, 1.0, conf=conf, coords=exact), 48)[0]
    err = float((out["pose"][:, leaf] - sc["pts"][:, leaf]).norm(dim=-1).max())
    print(f"({B}, {V}, {J}) one view: |fit - truth| of that joint {err:.3e} cm")
    assert bool(out["valid"].all()) and err < 1e-7


@pytest.mark.parametrize("B,V,J,rw,chain", [(2, 4, 16, True, False), (2, 2, 5, False, True), (1, 3, 2, False, False)])
def test_the_statement_and_the_newton_referee_agree(B, V, J, rw, chain):
    sc = SS.scene(B, V, J, rw, chain)
    for case, lam in (("full", 1.0), ("one_view", 10.0), ("unseen_prior", 1.0)):
        pr = SS.problem(sc, SS.case_operands(sc, case), lam, torch.float64)
        out = SS.fit_statement(pr, 128)[0]
        # (from the statement's result where the energy has two minima - one view, two-view rig - else from the init, like the fit)
        ref, gmax = SS.newton_referee(pr, out["pose"] if case == "one_view" and V == 2 else None)
        err = float((out["pose"] - ref)[pr.active].abs().max())
        print(f"({B}, {V}, {J}) {case} lambda {lam}: |statement - referee| {err:.3e} cm, referee |grad| {float(gmax.max()):.1e}")
        assert float(gmax.max()) < 1e-10 and err < 1e-6
        assert float((SS.energy(pr, ref)[0] - out["energy"]).abs().max()) < 1e-9


def test_statements_of_the_small_launches_on_known_answers():
    parents = (0, 0, 1, 1)
    pose = torch.tensor([[[0.0, 0, 0], [3, 4, 0], [3, 4, 12], [3, 10, 0]],
                         [[1.0, 1, 1], [1, 1, 3], [1, 4, 7], [1, 1, 3]]], dtype=torch.float64)
    valid = torch.tensor([[1, 1, 1, 0], [1, 1, 1, 1]], dtype=torch.uint8)
    length, spread, count = SS.bone_lengths_statement(pose, valid, parents)
    assert count.tolist() == [0, 2, 2, 1]
    assert length.tolist() == [0.0, 3.5, 8.5, 0.0] and spread.tolist() == [0.0, 1.5, 3.5, 0.0]       # bone 3 of frame 1 has length 0
    L = torch.tensor([0.0, 10.0, 6.0, 2.0], dtype=torch.float64)
    out = SS.resize_statement(pose, valid, L, parents)
    assert out[0].tolist() == [[0.0, 0, 0], [6, 8, 0], [6, 8, 6], [3, 10, 0]]          # the invalid joint keeps its place
    # frame 1: bone 3 has no direction and keeps its (zero) vector: the joint follows its moved parent
    assert torch.allclose(out[1], torch.tensor([[1.0, 1, 1], [1, 1, 11], [1, 4.6, 15.8], [1, 1, 11]], dtype=torch.float64), atol=1e-12)
    mid = torch.tensor([[1, 0, 1, 1]], dtype=torch.uint8)                             # an invalid joint mid-chain: its children stay too
    assert torch.equal(SS.resize_statement(pose[:1], mid, L, parents), pose[:1])
    free = SS.resize_statement(pose[:1], valid[:1], torch.tensor([0.0, 10.0, float("nan"), 2.0], dtype=torch.float64), parents)
    assert free[0].tolist() == [[0.0, 0, 0], [6, 8, 0], [6, 8, 12], [3, 10, 0]]        # a bone without a length keeps its vector

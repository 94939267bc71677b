"""CPU-side checks of the volumetric fusion (egorear_amd/decode.py): both operators are registered with fake implementations and an
autograd formula that reaches the heat maps only, both public functions give the documented shapes on meta tensors,
`decode_joints_3d_volumetric` traces under Dynamo as one graph, every limit of the kernels is refused before any launch, and CPU
tensors are refused."""
import pytest
import torch

from fisheye_statement import rig

def _meta(*shape, **kw):
    return torch.empty(*shape, device="meta", **kw)


def test_operators_are_registered_with_fake_implementations():
    from egorear_amd import decode, hip
    assert hasattr(torch.ops.egorear_amd, "volume_fuse") and hasattr(torch.ops.egorear_amd, "volume_fuse_bwd")
    assert "egr_volume_fuse_f32" in hip.EXPORTS and "egr_volume_fuse_bwd_f32" in hip.EXPORTS
    for B, V, J, H, W, G, rw, with_ok in ((2, 4, 15, 64, 64, 16, False, False), (3, 2, 5, 16, 12, 4, False, True), (1, 3, 16, 32, 32, 32, True, True)):
        hm = _meta(B, V, J, H, W, requires_grad=True)
        conf, centers = _meta(B, V, J, requires_grad=True), _meta(B, J, 3, requires_grad=True)
        ctm = _meta(B, V, 4, 4) if rw else None
        ok_in = _meta(B, J, dtype=torch.uint8) if with_ok else None
        pose, peak, index, spread, ok = decode.volume_fuse_op(hm, conf, centers, _meta(V, 30), ctm, ok_in, G, 40.0, 100.0, 0.5)
        assert pose.shape == (B, J, 3) and peak.shape == index.shape == spread.shape == ok.shape == (B, J)
        assert pose.dtype == peak.dtype == spread.dtype == torch.float32 and index.dtype == torch.int32 and ok.dtype == torch.uint8
        assert pose.requires_grad and peak.requires_grad
        assert not spread.requires_grad and not index.requires_grad and not ok.requires_grad
        # the registered autograd formula, on meta: from the pose, from the peak and from both - to the heat maps, and to nothing else
        for outs in ([pose], [peak], [pose, peak]):
            g_hm, g_conf, g_centers = torch.autograd.grad(outs, [hm, conf, centers], [torch.empty_like(o) for o in outs], retain_graph=True,
                                                          allow_unused=True)
            assert g_hm.shape == hm.shape and g_hm.dtype == torch.float32 and g_conf is None and g_centers is None
        g = decode.volume_fuse_bwd_op(hm.detach(), conf.detach(), centers.detach(), _meta(V, 30), ctm, ok_in, _meta(B, J, 3), None, G, 40.0,
                                      100.0, 0.5)
        assert g.shape == hm.shape and g.dtype == torch.float32
        g = decode.volume_fuse_bwd_op(hm.detach(), conf.detach(), centers.detach(), _meta(V, 30), ctm, ok_in, None, _meta(B, J), G, 40.0,
                                      100.0, 0.5)
        assert g.shape == hm.shape


def test_public_functions_give_the_documented_shapes_on_meta():
    from egorear_amd import decode
    cams = rig()
    hm = _meta(2, 4, 15, 64, 64)
    out = decode.fuse_joints_volumetric(hm, _meta(2, 15, 3), cams)
    assert isinstance(out, decode.Volume3D) and out._fields == ("pose", "peak", "index", "spread", "valid")
    assert out.pose.shape == (2, 15, 3) and out.peak.shape == out.index.shape == out.spread.shape == out.valid.shape == (2, 15)
    assert out.valid.dtype == torch.bool and out.index.dtype == torch.int32 and out.pose.dtype == torch.float32
    one = decode.fuse_joints_volumetric(hm, _meta(2, 3), cams, conf=_meta(2, 4, 15), grid=32, cube_cm=60.0, beta=50.0)     # (B, 3) centres
    assert one.pose.shape == (2, 15, 3)
    two = decode.fuse_joints_volumetric(_meta(3, 2, 5, 16, 12), _meta(3, 5, 3), cams[:2], grid=4)
    assert two.pose.shape == (3, 5, 3) and two.valid.shape == (3, 5)
    rw = decode.fuse_joints_volumetric(hm, _meta(2, 15, 3), "ego4view_rw", coord_trans_mat=_meta(2, 4, 4, 4))
    assert rw.pose.shape == (2, 15, 3)
    vol, tri, j2 = decode.decode_joints_3d_volumetric(hm, "ego4view_syn")
    assert isinstance(vol, decode.Volume3D) and isinstance(tri, decode.Joints3D) and isinstance(j2, decode.Joints2D)
    assert vol.pose.shape == tri.pose.shape == (2, 15, 3) and j2.soft.shape == (2, 4, 15, 2) and vol.valid.dtype == torch.bool
    vol, tri, _ = decode.decode_joints_3d_volumetric(_meta(2, 4, 15, 64, 48), cams, coord_trans_mat=_meta(2, 4, 4, 4), grid=8, volume_beta=20.0)
    assert vol.spread.shape == (2, 15) and tri.residual.shape == (2, 4, 15)


def test_decode_joints_3d_volumetric_traces_as_one_graph():
    import torch._dynamo as dynamo
    from egorear_amd import decode
    lin = torch.nn.Conv2d(4, 15, 1, device="meta")
    cams = rig()

    def serving_side(feat):
        hm = lin(feat).view(2, 4, 15, 64, 64)
        vol, tri, j2 = decode.decode_joints_3d_volumetric(hm, cams)
        named = decode.fuse_joints_volumetric(hm, tri.pose.detach(), "ego4view_syn", conf=j2.maxvals.detach(), grid=8)
        return vol.pose.sum() + vol.peak.mean() + named.pose.mean(), vol.valid, vol.index, tri.pose

    feat = _meta(8, 4, 64, 64)
    loss, valid, index, tri_pose = serving_side(feat)         # (also warms the record cache: the upload is not part of a graph)
    assert loss.requires_grad and valid.shape == (2, 15) and index.dtype == torch.int32 and tri_pose.shape == (2, 15, 3)
    dynamo.reset()
    ex = dynamo.explain(serving_side)(feat)
    assert ex.graph_break_count == 0 and ex.graph_count == 1, ex
    targets = [str(nd.target) for g in ex.graphs for nd in g.graph.nodes if nd.op == "call_function"]
    assert sum("egorear_amd.volume_fuse" in t for t in targets) == 2, targets
    assert sum("egorear_amd.triangulate" in t for t in targets) == 1 and sum("egorear_amd.soft_argmax" in t for t in targets) == 1, targets


def test_the_gradient_of_the_chain_reaches_the_heat_maps_on_meta():
    from egorear_amd import decode
    hm = _meta(2, 4, 15, 64, 64, requires_grad=True)
    vol, tri, _ = decode.decode_joints_3d_volumetric(hm, rig())
    assert vol.pose.requires_grad and vol.peak.requires_grad and not vol.spread.requires_grad
    (g,) = torch.autograd.grad([vol.pose, vol.peak], [hm], [torch.empty_like(vol.pose), torch.empty_like(vol.peak)])
    assert g.shape == hm.shape


def test_bad_operands_are_refused_before_any_launch():
    from egorear_amd import decode, hip
    cams = rig()
    rec = torch.zeros(4, 30)
    hm, conf, centers = torch.zeros(2, 4, 3, 64, 64), torch.ones(2, 4, 3), torch.zeros(2, 3, 3)

    def both(hm=hm, conf=conf, centers=centers, cams=cams, rec=rec, ctm=None, **kw):
        """the public function and the launcher refuse alike"""
        with pytest.raises(ValueError):
            decode.fuse_joints_volumetric(hm, centers, cams, conf=conf, coord_trans_mat=ctm, **kw)
        hip_kw = {{"cube_cm": "cube"}.get(k, k): v for k, v in kw.items()}
        with pytest.raises(ValueError):
            hip.volume_fuse(hm, conf, centers, rec, ctm, None, **hip_kw)
        with pytest.raises(ValueError):
            hip.volume_fuse_bwd(hm, conf, centers, rec, ctm, None, None, None, **hip_kw)

    for V in (1, 5):                                                                  # 2 <= V <= 4
        both(hm=torch.zeros(2, V, 3, 8, 8), conf=torch.ones(2, V, 3), cams=(cams + cams)[:V], rec=torch.zeros(V, 30))
    for G in (1, 0, -4, 33, 64):                                                      # 2 <= G <= 32
        both(grid=G)
    for G in (16.0, "16", None, True):
        both(grid=G)
    both(hm=torch.zeros(1, 4, 1, 64, 65), conf=torch.ones(1, 4, 1), centers=torch.zeros(1, 1, 3))         # V * H * W <= 16384
    both(hm=torch.zeros(1, 3, 1, 128, 64), conf=torch.ones(1, 3, 1), centers=torch.zeros(1, 1, 3), cams=cams[:3], rec=torch.zeros(3, 30))
    both(hm=torch.zeros(1, 2, 1, 8193, 1), conf=torch.ones(1, 2, 1), centers=torch.zeros(1, 1, 3), cams=cams[:2], rec=torch.zeros(2, 30))
    for bad in (0.0, -40.0, float("inf"), float("nan")):                              # cube and beta positive and finite
        both(cube_cm=bad)
        both(beta=bad)
    for h in (hm.double(), hm.half(), hm.long()):                                     # fp32 throughout
        both(hm=h)
    both(conf=conf.double())
    both(centers=centers.double())
    both(ctm=torch.zeros(2, 4, 4, 4).double())
    for h in (torch.zeros(2, 4, 3, 64), torch.zeros(2, 4, 3, 2, 64, 64), torch.zeros(0, 4, 3, 8, 8)):
        both(hm=h)
    for w in (torch.ones(2, 4, 2), torch.ones(2, 3, 3), torch.ones(2, 4, 3, 1)):
        both(conf=w)
    for c in (torch.zeros(2, 3, 2), torch.zeros(2, 4, 3), torch.zeros(1, 3, 3), torch.zeros(3)):
        both(centers=c)
    for m in (torch.zeros(2, 4, 4), torch.zeros(1, 4, 4, 4), torch.zeros(2, 3, 4, 4), torch.zeros(2, 4, 3, 4)):
        both(ctm=m)
    with pytest.raises(ValueError):
        decode.fuse_joints_volumetric(hm, centers, cams[:3])                         # four views, three cameras
    with pytest.raises(ValueError):
        hip.volume_fuse(hm, conf, centers, torch.zeros(4, 17))                      # the shipped 17-float record is not a ray record
    for ok_in in (torch.ones(2, 3), torch.ones(2, 4, dtype=torch.uint8), torch.ones(2, 3, dtype=torch.bool)):
        with pytest.raises(ValueError):
            hip.volume_fuse(hm, conf, centers, rec, None, ok_in)
    with pytest.raises(ValueError):
        hip.volume_fuse_bwd(hm, conf, centers, rec, None, None, torch.zeros(2, 3, 2), None)
    with pytest.raises(ValueError):
        hip.volume_fuse_bwd(hm, conf, centers, rec, None, None, None, torch.zeros(2, 4))
    with pytest.raises(ValueError):
        hip.volume_fuse_bwd(hm, conf, centers, rec, None, None, torch.zeros(2, 3, 3).double(), None)
    with pytest.raises(ValueError):
        hip.volume_fuse(hm.transpose(-1, -2), conf, centers, rec)                   # the launcher reads its operands as they lie
    # the operators (their fake implementations) refuse alike
    m = lambda t: t.to("meta")
    for kw in ({"grid": 1}, {"grid": 33}, {"cube": 0.0}, {"cube": float("nan")}, {"beta": -1.0}, {"beta": float("inf")}):
        args = {"grid": 16, "cube": 40.0, "beta": 100.0, **kw}
        with pytest.raises(ValueError):
            decode.volume_fuse_op(m(hm), m(conf), m(centers), m(rec), None, None, args["grid"], args["cube"], args["beta"], 0.5)
        with pytest.raises(ValueError):
            decode.volume_fuse_bwd_op(m(hm), m(conf), m(centers), m(rec), None, None, None, None, args["grid"], args["cube"], args["beta"], 0.5)
    with pytest.raises(ValueError):
        decode.volume_fuse_op(_meta(1, 4, 1, 64, 65), _meta(1, 4, 1), _meta(1, 1, 3), m(rec), None, None, 16, 40.0, 100.0, 0.5)
    with pytest.raises(ValueError):
        decode.volume_fuse_bwd_op(m(hm), m(conf), m(centers), m(rec), None, None, _meta(2, 3, 2), None, 16, 40.0, 100.0, 0.5)
    # the chain
    with pytest.raises(ValueError):
        decode.decode_joints_3d_volumetric(torch.zeros(2, 15, 8, 8), cams)                                # (B, V, J, H, W) only
    with pytest.raises(ValueError):
        decode.decode_joints_3d_volumetric(torch.zeros(2, 5, 15, 8, 8), cams + cams[:1])
    for kw in ({"grid": 33}, {"cube_cm": -1.0}, {"volume_beta": 0.0}, {"beta": 0.0}):
        with pytest.raises(ValueError):
            decode.decode_joints_3d_volumetric(_meta(2, 4, 15, 64, 64), cams, **kw)
    with pytest.raises(ValueError):
        decode.decode_joints_3d_volumetric(_meta(1, 4, 15, 128, 64), cams)                                # more than the LDS image holds


def test_cpu_tensors_are_refused():
    from egorear_amd import decode, hip
    cams = rig()
    hm, conf, centers, rec = torch.zeros(2, 4, 3, 16, 16), torch.ones(2, 4, 3), torch.zeros(2, 3, 3), torch.zeros(4, 30)
    with pytest.raises(RuntimeError, match="no CPU path"):
        decode.fuse_joints_volumetric(hm, centers, cams)
    with pytest.raises(RuntimeError, match="no CPU path"):
        decode.fuse_joints_volumetric(hm, centers[:, 0].contiguous(), "ego4view_rw", conf=conf, coord_trans_mat=torch.zeros(2, 4, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        decode.decode_joints_3d_volumetric(hm, cams)
    with pytest.raises((NotImplementedError, RuntimeError)):                          # the operator itself: no CPU kernel, no fallback
        decode.volume_fuse_op(hm, conf, centers, rec, None, None, 16, 40.0, 100.0, 0.5)
    with pytest.raises((NotImplementedError, RuntimeError)):
        decode.volume_fuse_bwd_op(hm, conf, centers, rec, None, None, torch.zeros(2, 3, 3), None, 16, 40.0, 100.0, 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.volume_fuse(hm, conf, centers, rec)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.volume_fuse_bwd(hm, conf, centers, rec, None, None, torch.zeros(2, 3, 3), torch.zeros(2, 3))

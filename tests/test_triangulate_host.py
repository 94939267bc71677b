"""CPU-side checks of the fisheye triangulation (egorear_amd/decode.py, egorear_amd/camera.py): both operators are registered with fake
implementations and an autograd formula, `decode_joints_3d` traces under Dynamo as one graph on meta tensors, shape / dtype / parameter
errors are raised before any launch, CPU tensors are refused, the shipped camera record is unchanged and the new one carries the C2W
polynomial, and the Newton inverse of the W2C polynomial converges as DESIGN.md 5n says."""
import json
import os

import numpy as np
import pytest
import torch

from fisheye_statement import calib_dir, rig

def _meta_cams(V=4):
    return torch.empty(V, 30, device="meta")


def test_operators_are_registered_with_fake_implementations():
    from egorear_amd import decode
    assert hasattr(torch.ops.egorear_amd, "triangulate") and hasattr(torch.ops.egorear_amd, "triangulate_bwd")
    for B, V, J, rw in ((2, 4, 15, False), (3, 2, 5, False), (1, 3, 16, True)):
        coords = torch.empty(B, V, J, 2, device="meta", requires_grad=True)
        conf = torch.empty(B, V, J, device="meta", requires_grad=True)
        ctm = torch.empty(B, V, 4, 4, device="meta") if rw else None
        pts, cost, resid, ok = decode.triangulate_op(coords, conf, _meta_cams(V), ctm, 1 / 64, 1 / 64, 0.5, 1e-6)
        assert pts.shape == (B, J, 3) and cost.shape == (B, J) and resid.shape == (B, V, J) and ok.shape == (B, J)
        assert pts.dtype == cost.dtype == resid.dtype == torch.float32 and ok.dtype == torch.uint8
        assert pts.requires_grad and cost.requires_grad and not resid.requires_grad and not ok.requires_grad
        # the registered autograd formula, on meta: from the points and from the cost, together and one at a time
        g_coords, g_conf = torch.autograd.grad([pts, cost], [coords, conf], [torch.empty_like(pts), torch.empty_like(cost)], retain_graph=True)
        assert g_coords.shape == coords.shape and g_conf.shape == conf.shape and g_coords.dtype == g_conf.dtype == torch.float32
        g_coords, g_conf = torch.autograd.grad([cost], [coords, conf], [torch.empty_like(cost)])
        assert g_coords.shape == coords.shape and g_conf.shape == conf.shape
        g2 = decode.triangulate_bwd_op(coords.detach(), conf.detach(), _meta_cams(V), ctm, torch.empty(B, J, 3, device="meta"), None,
                                       1 / 64, 1 / 64, 0.5, 1e-6)
        assert g2[0].shape == coords.shape and g2[1].shape == conf.shape


def test_public_functions_give_the_documented_shapes_on_meta():
    from egorear_amd import decode
    cams = rig()
    coords, conf = torch.empty(2, 4, 15, 2, device="meta"), torch.empty(2, 4, 15, device="meta")
    out = decode.triangulate_joints(coords, conf, cams)
    assert isinstance(out, decode.Joints3D) and out._fields == ("pose", "cost", "residual", "valid")
    assert out.pose.shape == (2, 15, 3) and out.cost.shape == (2, 15) and out.residual.shape == (2, 4, 15) and out.valid.shape == (2, 15)
    assert out.valid.dtype == torch.bool
    two = decode.triangulate_joints(coords[:, :2].contiguous(), conf[:, :2].contiguous(), cams[:2], heatmap_size=(1, 1))
    assert two.pose.shape == (2, 15, 3) and two.residual.shape == (2, 2, 15)
    rw = decode.triangulate_joints(coords, conf, "ego4view_rw", coord_trans_mat=torch.empty(2, 4, 4, 4, device="meta"))
    assert rw.pose.shape == (2, 15, 3)
    tri, j2 = decode.decode_joints_3d(torch.empty(2, 4, 15, 64, 48, device="meta"), "ego4view_syn")
    assert tri.pose.shape == (2, 15, 3) and isinstance(j2, decode.Joints2D) and j2.soft.shape == (2, 4, 15, 2)
    # the records are uploaded once per (cameras, device)
    assert decode._ray_records(cams, None, torch.device("meta")) is decode._ray_records(cams, None, torch.device("meta"))
    assert decode._ray_records("ego4view_syn", None, torch.device("meta")) is decode._ray_records("ego4view_syn", None, torch.device("meta"))


def test_decode_joints_3d_traces_as_one_graph():
    import torch._dynamo as dynamo
    from egorear_amd import decode
    lin = torch.nn.Conv2d(4, 15, 1, device="meta")
    cams = rig()

    def serving_side(feat):
        hm = lin(feat).view(2, 4, 15, 64, 64)
        tri, j2 = decode.decode_joints_3d(hm, cams)
        named, _ = decode.decode_joints_3d(hm, "ego4view_syn")
        return tri.pose.sum() + tri.cost.mean() + named.cost.mean(), tri.valid, j2.soft

    feat = torch.empty(8, 4, 64, 64, device="meta")
    loss, valid, soft = serving_side(feat)                    # (also warms the record cache: the upload is not part of a graph)
    assert loss.requires_grad and valid.shape == (2, 15) and soft.shape == (2, 4, 15, 2)
    dynamo.reset()
    ex = dynamo.explain(serving_side)(feat)
    assert ex.graph_break_count == 0 and ex.graph_count == 1, ex
    targets = [str(nd.target) for g in ex.graphs for nd in g.graph.nodes if nd.op == "call_function"]
    assert sum("egorear_amd.triangulate" in t for t in targets) == 2 and sum("egorear_amd.soft_argmax" in t for t in targets) == 2, targets


def test_bad_operands_are_refused_before_any_launch():
    from egorear_amd import decode, hip
    cams = rig()
    ok_c, ok_w = torch.zeros(2, 4, 15, 2), torch.ones(2, 4, 15)
    for V in (1, 5):                                                                 # 2 to 4 views
        with pytest.raises(ValueError):
            decode.triangulate_joints(torch.zeros(2, V, 15, 2), torch.ones(2, V, 15), (cams + cams)[:V])
        with pytest.raises(ValueError):
            hip.triangulate(torch.zeros(2, V, 15, 2), torch.ones(2, V, 15), torch.zeros(V, 30))
    with pytest.raises(ValueError):
        decode.triangulate_joints(ok_c, ok_w, cams[:3])                              # four views, three cameras
    with pytest.raises(ValueError):
        decode.triangulate_joints(ok_c, ok_w, cams[:1])
    for bad_w in (torch.ones(2, 4, 14), torch.ones(2, 3, 15), torch.ones(2, 4, 15, 1)):
        with pytest.raises(ValueError):
            decode.triangulate_joints(ok_c, bad_w, cams)
        with pytest.raises(ValueError):
            hip.triangulate(ok_c, bad_w, torch.zeros(4, 30))
    for bad_c in (torch.zeros(2, 4, 15, 3), torch.zeros(2, 4, 15), torch.zeros(0, 4, 15, 2)):
        with pytest.raises(ValueError):
            decode.triangulate_joints(bad_c, ok_w, cams)
    for bad_m in (torch.zeros(2, 4, 4), torch.zeros(1, 4, 4, 4), torch.zeros(2, 3, 4, 4), torch.zeros(2, 4, 3, 4)):
        with pytest.raises(ValueError):
            decode.triangulate_joints(ok_c, ok_w, cams, coord_trans_mat=bad_m)
        with pytest.raises(ValueError):
            hip.triangulate(ok_c, ok_w, torch.zeros(4, 30), bad_m)
    for c, w, m in ((ok_c.double(), ok_w, None), (ok_c, ok_w.half(), None), (ok_c.long(), ok_w, None), (ok_c, ok_w, torch.zeros(2, 4, 4, 4).double())):
        with pytest.raises(ValueError):
            decode.triangulate_joints(c, w, cams, coord_trans_mat=m)
        with pytest.raises(ValueError):
            hip.triangulate(c, w, torch.zeros(4, 30), m)
    for size in ((0, 64), (64, 0), (-64, 64), (64,), (float("nan"), 64), (float("inf"), 64), None):
        with pytest.raises(ValueError):
            decode.triangulate_joints(ok_c, ok_w, cams, heatmap_size=size)
    for ratio in (-1e-6, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            decode.triangulate_joints(ok_c, ok_w, cams, min_det_ratio=ratio)
        with pytest.raises(ValueError):
            hip.triangulate(ok_c, ok_w, torch.zeros(4, 30), min_det_ratio=ratio)
        with pytest.raises(ValueError):
            decode.triangulate_op(ok_c.to("meta"), ok_w.to("meta"), _meta_cams(), None, 1 / 64, 1 / 64, 0.5, ratio)
    with pytest.raises(ValueError):
        hip.triangulate(ok_c, ok_w, torch.zeros(4, 17))                              # the shipped 17-float record is not a ray record
    with pytest.raises(ValueError):
        hip.triangulate_bwd(ok_c, ok_w, torch.zeros(4, 30), None, torch.zeros(2, 15, 2), None)
    with pytest.raises(ValueError):
        hip.triangulate_bwd(ok_c, ok_w, torch.zeros(4, 30), None, None, torch.zeros(2, 14))
    with pytest.raises(ValueError):
        decode.triangulate_bwd_op(ok_c.to("meta"), ok_w.to("meta"), _meta_cams(), None, torch.zeros(2, 15, 2, device="meta"), None,
                                  1 / 64, 1 / 64, 0.5, 1e-6)
    with pytest.raises(ValueError):
        decode.decode_joints_3d(torch.zeros(2, 15, 8, 8), cams)                       # (B, V, J, H, W) only
    with pytest.raises(ValueError):
        decode.decode_joints_3d(torch.zeros(2, 5, 15, 8, 8), cams + cams[:1])


def test_cpu_tensors_are_refused():
    from egorear_amd import decode, hip
    cams = rig()
    coords, conf = torch.zeros(2, 4, 15, 2), torch.ones(2, 4, 15)
    with pytest.raises(RuntimeError, match="no CPU path"):
        decode.triangulate_joints(coords, conf, cams)
    with pytest.raises(RuntimeError, match="no CPU path"):
        decode.triangulate_joints(coords, conf, "ego4view_rw", coord_trans_mat=torch.zeros(2, 4, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        decode.decode_joints_3d(torch.zeros(2, 4, 15, 8, 8), cams)
    with pytest.raises((NotImplementedError, RuntimeError)):                          # the operator itself: no CPU kernel, no fallback
        decode.triangulate_op(coords, conf, torch.zeros(4, 30), None, 1 / 64, 1 / 64, 0.5, 1e-6)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.triangulate(coords, conf, torch.zeros(4, 30))
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.triangulate_bwd(coords, conf, torch.zeros(4, 30), None, torch.zeros(2, 15, 3), torch.zeros(2, 15))


def test_shipped_camera_record_is_unchanged_and_the_ray_record_extends_it():
    from egorear_amd import camera, hip
    assert camera.MAX_POLY == 12 and camera.RAY_REC == hip.RAY_REC == 30
    offsets = {"camera_front_left": (6.0, 0.0, 0.0), "camera_front_right": (-6.0, 0.0, 0.0), "camera_back_left": (-6.0, 37.0, 0.0),
               "camera_back_right": (6.0, 37.0, 0.0)}
    for cam in rig():
        with open(os.path.join(calib_dir(), cam.camera_name + ".json")) as f:
            d = json.load(f)
        # packed(): the 17 floats the shipped kernels read, field for field
        rec = cam.packed()
        assert rec.shape == (17,) and rec.dtype == np.float32
        want = np.zeros(17, dtype=np.float32)
        want[0] = len(d["polynomialW2C"])
        want[1:3] = d["image_center"]
        want[3], want[4] = d["size"][1], d["size"][0]
        want[5:5 + len(d["polynomialW2C"])] = d["polynomialW2C"]
        assert np.array_equal(rec, want)
        # packed_rays(): those, then the C2W polynomial of the JSON, the flip flag and the offset
        ray = cam.packed_rays()
        assert ray.shape == (30,) and ray.dtype == np.float32 and np.array_equal(ray[:17], rec)
        n = len(d["polynomialC2W"])
        assert ray[17] == n and np.array_equal(ray[18:18 + n], np.asarray(d["polynomialC2W"], dtype=np.float32)) and not ray[18 + n:26].any()
        assert cam.fisheye_polynomial == [float(np.float32(v)) for v in d["polynomialC2W"]]
        assert ray[26] == (1.0 if "back" in cam.camera_name else 0.0) and tuple(ray[27:30]) == offsets[cam.camera_name]


def test_newton_on_w2c_from_the_c2w_seed_inverts_the_projection():
    """float64: for each packaged calibration, rho = W2C(theta) over theta in [-pi/2 + 1e-3, -0.2]; the C2W seed and the kernel's two
    Newton steps return theta to 1e-12, and a third step changes nothing an fp32 result could show."""
    for cam in rig():
        w2c = np.asarray(cam.fisheye_inv_polynomial, dtype=np.float64)[::-1]
        c2w = np.asarray(cam.fisheye_polynomial, dtype=np.float64)[::-1]
        dw2c = np.polyder(w2c)
        theta = np.linspace(-np.pi / 2 + 1e-3, -0.2, 20001)
        rho = np.polyval(w2c, theta)
        assert rho.min() > 0 and np.all(np.diff(rho) > 0)
        wide = np.linspace(-np.pi / 2, 0.3, 20001)
        assert np.polyval(dw2c, wide).min() >= 275.0                                 # the iteration cannot stall on the image circle
        t = np.arctan(np.polyval(c2w, rho) / rho)
        seed = np.abs(t - theta).max()
        errs = []
        for _ in range(3):
            t = t - (np.polyval(w2c, t) - rho) / np.polyval(dw2c, t)
            errs.append(np.abs(t - theta).max())
        print(f"{cam.camera_name}: seed {seed:.3e} rad, after 1 / 2 / 3 Newton steps {errs[0]:.3e} / {errs[1]:.3e} / {errs[2]:.3e}")
        assert seed < 1e-4 and errs[1] <= 1e-12
        assert errs[0] < 2.0 ** -27 and abs(errs[2] - errs[1]) < 1e-14       # one step: below half an fp32 ulp of the smallest |theta| here

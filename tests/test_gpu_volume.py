"""Volumetric fusion on the GPU (egr_volume_fuse_f32 / egr_volume_fuse_bwd_f32, egorear_amd/decode.py) against the float64 statement of
its math in tests/volume_statement.py.  torch.autograd differentiates the statement.

The yardstick (fisheye_statement.yardstick, with `shape_own`) is that of test_gpu_soft_argmax.py: a HIP output or gradient may deviate
from the float64 statement (evaluated on the same fp32 inputs) by at most 8 x the deviation of torch's fp32 CPU evaluation of that
statement - taken per output kind as the maximum over the cases of one shape, so that one lucky case cannot shrink the allowance -
with a floor of 4 ulp (fp32) of the output's largest magnitude.  Both figures are printed per case.  `index` is compared exactly on the
pairs whose float64 best and second-best score differ by more than 8 x the fp32 statement's largest score deviation in that case; at
most one pair in ten of a case may be left out this way, which is checked here on the CPU."""
import math

import pytest
import torch

from fisheye_statement import MARGIN, THR, bumps, heatmap_coords, random_ctm, random_points, records, rig, ulp32, yardstick
from volume_statement import offsets, statement

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CUBE = 40.0
# (B, V, J, H, W, G, rw): the product's maps; the smallest, non-square, the two front cameras; an odd grid with lanes that own no voxel;
# rw with a per-sample coord_trans_mat (rotations up to 0.05 rad); the largest grid
SHAPES = [(2, 4, 3, 64, 64, 8, False), (1, 2, 1, 16, 12, 4, False), (3, 3, 2, 32, 32, 5, False), (2, 4, 2, 64, 64, 16, True),
          (1, 4, 1, 64, 64, 32, False)]
CASES = ("bumps", "noise", "dropped", "nan", "border")


def evaluate(hm, conf, centers, rec, ctm, G, cube, beta, thr, g_pose, g_peak, center_ok=None):
    """The statement and its autograd in float64 and in float32 on the same fp32 inputs, and which pairs' index is decided."""
    out = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        h = hm.clone().to(dt).requires_grad_()
        r = statement(h, conf.to(dt), centers.to(dt), rec, None if ctm is None else ctm, G, cube, beta, thr, center_ok)
        (g,) = torch.autograd.grad([r["pose"], r["peak"]], [h], [g_pose.to(dt), g_peak.to(dt)])
        out[name] = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in r.items()}
        out[name]["g_hm"] = g
    s_dev = float((out["f32"]["S"].double() - out["f64"]["S"]).abs().max())
    top2 = out["f64"]["S"].topk(2, -1)[0]
    out["decided"] = ((top2[..., 0] - top2[..., 1]) > MARGIN * s_dev) | ~out["f64"]["valid"]
    out["s_dev"] = s_dev
    return out


# --------------------------------------------------------------------------- data, computed once and shared (never modified)

_CACHE = {}


def shape_data(shape):
    if shape in _CACHE:
        return _CACHE[shape]
    B, V, J, H, W, G, rw = shape
    g = torch.Generator().manual_seed(1000 * B + 100 * V + 10 * J + G)
    cams = rig("ego4view_rw" if rw else "ego4view_syn")[:V]
    rec = records(cams)
    ctm = random_ctm(B, V, cams, g) if rw else None
    pts = random_points(B, J, g)
    clean = bumps(pts, rec, ctm, H, W).float().contiguous()
    g_pose, g_peak = torch.randn(B, J, 3, generator=g), torch.randn(B, J, generator=g)
    cases = {}
    for case in CASES:
        hm, conf, thr, beta = clean, torch.rand(B, V, J, generator=g) * 0.4 + 0.6, THR, 100.0
        centers = (pts + (torch.rand(B, J, 3, generator=g, dtype=torch.float64) - 0.5) * 6.0).float()      # a few cm off the point
        if case == "noise":              # every pixel and every voxel carries weight; every view counts, with its own weight
            hm, beta, thr = torch.rand(B, V, J, H, W, generator=g), 5.0, 0.05
            conf = torch.rand(B, V, J, generator=g) * 0.9 + 0.1
        elif case == "dropped":          # pair k loses (k + 1) % (V + 1) of its views: V, ..., one, zero views are left
            for k in range(B * J):
                for i in range((k + 1) % (V + 1)):
                    conf[k // J, (k + i) % V, k % J] = 0.3
        elif case == "nan":              # pair k: a NaN conf, a NaN centre, an inf conf in turn (one view, one coordinate)
            for k in range(B * J):
                if k % 3 == 1:
                    centers[k // J, k % J, k % 3] = float("nan")
                else:
                    conf[k // J, k % V, k % J] = float("nan") if k % 3 == 0 else float("inf")
        elif case == "border":           # low and far to the side: part of the cube projects outside the images (the zero padding)
            hm, beta = torch.rand(B, V, J, H, W, generator=g), 5.0
            side = torch.where(torch.rand(B, J, generator=g) < 0.5, -1.0, 1.0)
            centers = torch.stack((side * 75.0, torch.rand(B, J, generator=g) * 30.0, torch.rand(B, J, generator=g) * 4.0 + 14.0), -1)
        hm, conf, centers = hm.contiguous(), conf.contiguous(), centers.contiguous()
        cases[case] = (hm, conf, centers, thr, beta, evaluate(hm, conf, centers, rec, ctm, G, CUBE, beta, thr, g_pose, g_peak))
    _CACHE[shape] = {"cams": cams, "rec": rec, "ctm": ctm, "pts": pts, "g_pose": g_pose, "g_peak": g_peak, "cases": cases}
    return _CACHE[shape]


def own_deviation(d, name):
    """The fp32 statement's deviation from the float64 statement for one output kind: the maximum over the cases of the shape."""
    return max(float((ref["f32"][name].double() - ref["f64"][name]).abs().max()) for *_, ref in d["cases"].values())


def launch(d, hm, conf, centers, G, beta, thr, cube=CUBE, center_ok=None):
    from egorear_amd import hip
    ctm = None if d["ctm"] is None else d["ctm"].to(DEV)
    return hip.volume_fuse(hm.to(DEV), conf.to(DEV), centers.to(DEV), d["rec"].to(DEV), ctm, center_ok, G, cube, beta, thr)


# --------------------------------------------------------------------------- the cases themselves, on the CPU

@pytest.mark.parametrize("shape", SHAPES)
def test_the_cases_cover_what_they_are_meant_to(shape):
    d = shape_data(shape)
    B, V, J, H, W, G, _ = shape
    for case in CASES:
        hm, conf, centers, thr, beta, ref = d["cases"][case]
        left_out = int((~ref["decided"]).sum())
        print(f"{shape} {case}: fp32 score deviation {ref['s_dev']:.3e}, pairs whose index is not decided {left_out} of {B * J}, "
              f"voxel-view samples inside {ref['f64']['sampled']:.3f}, across the border {ref['f64']['partial']:.3f}")
        assert 10 * left_out <= B * J, (shape, case, left_out)                    # at most one pair in ten
        assert torch.equal(ref["f32"]["valid"], ref["f64"]["valid"])
        used = ((conf >= thr) & torch.isfinite(conf)).sum(1)
        if case in ("bumps", "noise", "border"):
            assert bool(ref["f64"]["valid"].all())
        if case == "dropped" and B * J >= V + 1:
            assert sorted(set(used.view(-1).tolist())) == list(range(V + 1))       # V, ..., two, one and zero views all occur
        if case == "nan":
            assert int((~torch.isfinite(conf)).sum()) >= 1 and (B * J < 2 or int((~torch.isfinite(centers)).sum()) >= 1)
            assert torch.equal(ref["f64"]["valid"], (used >= 2) & torch.isfinite(centers).all(-1))
        if case == "border":             # some samples straddle the border, some fall outside altogether, some are whole
            assert ref["f64"]["partial"] > 0.0 and 0.05 < ref["f64"]["sampled"] < 0.95
        if case in ("bumps", "noise"):
            assert ref["f64"]["sampled"] > 0.5


# --------------------------------------------------------------------------- forward

@pytest.mark.parametrize("shape", SHAPES)
def test_forward_against_the_float64_statement(shape):
    d = shape_data(shape)
    B, V, J, H, W, G, _ = shape
    own = {name: own_deviation(d, name) for name in ("pose", "peak", "spread")}
    bad = []
    for case in CASES:
        hm, conf, centers, thr, beta, ref = d["cases"][case]
        pose, peak, index, spread, ok = launch(d, hm, conf, centers, G, beta, thr)
        torch.cuda.synchronize()
        print(f"{shape} {case}:")
        assert index.dtype == torch.int32 and ok.dtype == torch.uint8
        assert torch.equal(ok.cpu().bool(), ref["f64"]["valid"]), (shape, case)
        for name, got in (("pose", pose), ("peak", peak), ("spread", spread)):
            err, allowed = yardstick(name, got, ref["f32"][name], ref["f64"][name], own[name])
            if not err <= allowed:
                bad.append((shape, case, name, err, allowed))
        keep = ref["decided"]
        print(f"    index: compared on {int(keep.sum())} of {B * J} pairs, {int((index.cpu().long() != ref['f64']['index'])[keep].sum())} differ")
        assert torch.equal(index.cpu().long()[keep], ref["f64"]["index"][keep]), (shape, case)
        dead = ~ok.cpu().bool()
        assert float(pose.cpu()[dead].abs().sum()) == 0.0 and float(peak.cpu()[dead].abs().sum()) == 0.0
        assert float(spread.cpu()[dead].abs().sum()) == 0.0 and bool((index.cpu()[dead] == -1).all())
        assert bool((index.cpu()[~dead] >= 0).all()) and bool((index.cpu() < G ** 3).all())
        assert bool(torch.isfinite(pose).all()) and bool(torch.isfinite(peak).all()) and bool(torch.isfinite(spread).all())
    assert not bad, bad


# --------------------------------------------------------------------------- backward

@pytest.mark.parametrize("shape", SHAPES)
def test_backward_against_float64_autograd(shape):
    from egorear_amd import decode
    d = shape_data(shape)
    B, V, J, H, W, G, _ = shape
    own = own_deviation(d, "g_hm")
    bad = []
    for case in CASES:
        hm, conf, centers, thr, beta, ref = d["cases"][case]
        h = hm.to(DEV).requires_grad_()
        w, c = conf.to(DEV).requires_grad_(), centers.to(DEV).requires_grad_()
        ctm = None if d["ctm"] is None else d["ctm"].to(DEV)
        pose, peak, index, spread, ok = decode.volume_fuse_op(h, w, c, d["rec"].to(DEV), ctm, None, G, CUBE, beta, thr)
        assert pose.requires_grad and peak.requires_grad and not spread.requires_grad and not index.requires_grad and not ok.requires_grad
        g_hm, g_w, g_c = torch.autograd.grad([pose, peak], [h, w, c], [d["g_pose"].to(DEV), d["g_peak"].to(DEV)], allow_unused=True)
        torch.cuda.synchronize()
        assert g_w is None and g_c is None                                        # the cube is placed, not learned
        print(f"{shape} {case}:")
        err, allowed = yardstick("g_hm", g_hm, ref["f32"]["g_hm"], ref["f64"]["g_hm"], own)
        if not err <= allowed:
            bad.append((shape, case, err, allowed))
        excluded = ~((conf >= thr) & torch.isfinite(conf)) | ~ok.cpu().bool().unsqueeze(1)
        assert float(g_hm.cpu()[excluded].abs().sum()) == 0.0                     # excluded views and invalid pairs: exactly zero
        assert bool(torch.isfinite(g_hm).all())
        if bool(ok.any()):
            assert float(g_hm.abs().max()) > 0.0
    assert not bad, bad


def test_the_backward_writes_every_element():
    """The output buffer is not zeroed first: a poisoned buffer comes back without a trace of the poison."""
    from egorear_amd import hip
    d = shape_data(SHAPES[2])
    hm, conf, centers, thr, beta, ref = d["cases"]["dropped"]
    B, V, J, H, W, G, _ = SHAPES[2]
    h, w, c, rec = hm.to(DEV), conf.to(DEV), centers.to(DEV), d["rec"].to(DEV)
    gp, gk = d["g_pose"].to(DEV), d["g_peak"].to(DEV)
    g_hm = torch.full((B, V, J, H, W), float("nan"), device=DEV)
    rc = hip.lib.egr_volume_fuse_bwd_f32(h.data_ptr(), w.data_ptr(), c.data_ptr(), rec.data_ptr(), None, None, B, V, J, H, W, G, CUBE, beta,
                                         thr, gp.data_ptr(), gk.data_ptr(), g_hm.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isfinite(g_hm).all())
    err, allowed = yardstick("g_hm", g_hm, ref["f32"]["g_hm"], ref["f64"]["g_hm"], own_deviation(d, "g_hm"))
    assert err <= allowed


# --------------------------------------------------------------------------- a voxel on an optical axis

def test_a_voxel_on_the_optical_axis():
    """syn rig, G = 8, cube 32 (4 cm voxels, exact in fp32): column (ix, iy) = (3, 3) of the cube around (-4, 2, 2) is x = -6, y = 0 -
    camera_front_left's optical axis (its offset is +6) - at z = -12 ... 16: in front of the camera (the image centre), at its centre
    and behind it (no sample).  Noise maps at beta 5, so those voxels weigh like any other."""
    from egorear_amd import hip
    cams = rig()
    rec = records(cams)
    G, cube, beta = 8, 32.0, 5.0
    g = torch.Generator().manual_seed(11)
    hm = torch.rand(1, 4, 2, 64, 64, generator=g)
    conf = torch.ones(1, 4, 2)
    centers = torch.tensor([[[-4.0, 2.0, 2.0], [-4.0, 2.0, 30.0]]])
    o = offsets(G, cube, torch.float64)
    on_axis = ((centers[0, 0].double() + o)[:, :2] == torch.tensor([-6.0, 0.0], dtype=torch.float64)).all(-1)
    assert int(on_axis.sum()) == G                                                 # the whole column, exactly
    x, y, take = heatmap_coords(centers.double().view(1, 1, 2, 1, 3) + o, rec, None, 64, 64)
    # z = -12, -8, -4, 0 of view 0 give no sample; column (6, 3) is camera_front_right's axis (x = 6) and does the same in view 1
    assert int((~take[0, 0, 0]).sum()) == 4 and int((~take[0, 1, 0]).sum()) == 4 and not bool((~take[0, 2:]).any())
    assert int((~take[0, :, 1]).sum()) == 0                                        # the second cube is wholly in front
    g_pose, g_peak = torch.randn(1, 2, 3, generator=g), torch.randn(1, 2, generator=g)
    ref = evaluate(hm, conf, centers, rec, None, G, cube, beta, THR, g_pose, g_peak)
    assert bool(torch.isfinite(ref["f64"]["g_hm"]).all()) and bool(ref["decided"].all())
    got = hip.volume_fuse(hm.to(DEV), conf.to(DEV), centers.to(DEV), rec.to(DEV), None, None, G, cube, beta, THR)
    g_hm = hip.volume_fuse_bwd(hm.to(DEV), conf.to(DEV), centers.to(DEV), rec.to(DEV), None, None, g_pose.to(DEV), g_peak.to(DEV), G, cube,
                               beta, THR)
    torch.cuda.synchronize()
    assert bool(got[4].all()) and torch.equal(got[2].cpu().long(), ref["f64"]["index"])
    for i, name in ((0, "pose"), (1, "peak"), (3, "spread")):
        err, allowed = yardstick(name, got[i], ref["f32"][name], ref["f64"][name], float((ref["f32"][name].double() - ref["f64"][name]).abs().max()))
        assert err <= allowed, (name, err, allowed)
    err, allowed = yardstick("g_hm", g_hm, ref["f32"]["g_hm"], ref["f64"]["g_hm"],
                             float((ref["f32"]["g_hm"].double() - ref["f64"]["g_hm"]).abs().max()))
    assert err <= allowed and bool(torch.isfinite(g_hm).all())


# --------------------------------------------------------------------------- known answers

def test_all_ones_maps_give_the_centre_and_the_uniform_spread():
    """All-ones maps and a cube wholly inside every image: every score is exactly 1, so the distribution is uniform over the voxels."""
    from egorear_amd import hip
    rec = records(rig())
    for V, H, W, G, cube in ((4, 64, 64, 8, 40.0), (3, 32, 32, 5, 40.0), (2, 16, 12, 4, 20.0), (4, 64, 64, 32, 40.0)):
        hm, conf = torch.ones(1, V, 2, H, W), torch.ones(1, V, 2)
        centers = torch.tensor([[[3.0, 25.0, 80.0], [-10.0, 18.5, 65.25]]])
        want = cube * math.sqrt((G * G - 1) / (4.0 * G * G))
        ref = statement(hm.double(), conf.double(), centers.double(), rec[:V], None, G, cube, 100.0, THR)
        assert ref["sampled"] == 1.0 and float(ref["S"].min()) == 1.0 and float(ref["S"].max()) == 1.0
        assert float((ref["pose"] - centers.double()).abs().max()) < 1e-12 and float((ref["spread"] - want).abs().max()) < 1e-12
        assert bool((ref["index"] == 0).all()) and float((ref["peak"] - 1.0).abs().max()) == 0.0
        pose, peak, index, spread, ok = hip.volume_fuse(hm.to(DEV), conf.to(DEV), centers.to(DEV), rec[:V].to(DEV), None, None, G, cube, 100.0, THR)
        torch.cuda.synchronize()
        print(f"V {V} G {G}: |pose - centre| {float((pose.cpu() - centers).abs().max()):.3e}, spread {float(spread[0, 0]):.7f} against {want:.7f}")
        assert bool(ok.all()) and bool((index == 0).all()) and bool((peak == 1.0).all())
        assert float((pose.cpu() - centers).abs().max()) <= 4.0 * ulp32(float(centers.abs().max()))
        assert float((spread.cpu().double() - want).abs().max()) <= 4.0 * ulp32(want)


# five seeded points for which the float64 statement separates the two candidates with room (two of a hundred random draws do not)
DISAMBIGUATION_POINTS = [(-30.0, 53.0, 60.0), (26.0, 65.0, 44.0), (-13.0, 9.0, 74.0), (2.0, 62.0, 66.0), (-37.0, 54.0, 99.0)]


def test_the_fusion_picks_the_point_all_views_agree_on():
    """Four views hold a height-1 bump of P; view 0 also holds a height-1.2 bump of Q = P + (15, -10, 20) cm.  View 0's own arg-max
    goes to Q; the fused pose and the best voxel of an 80 cm cube around the midpoint stay with P."""
    from egorear_amd import hip
    rec = records(rig())
    G, cube = 16, 80.0
    P = torch.tensor(DISAMBIGUATION_POINTS, dtype=torch.float64).view(1, -1, 3)
    J = P.shape[1]
    Q = P + torch.tensor([15.0, -10.0, 20.0], dtype=torch.float64)
    maps = bumps(P, rec, None, 64, 64)
    maps[:, 0] += bumps(Q, rec, None, 64, 64, height=1.2)[:, 0]
    hm = maps.float().contiguous()
    conf = torch.ones(1, 4, J)
    centers = ((P + Q) / 2).float()
    xq, yq, _ = heatmap_coords(Q.view(1, 1, J, 1, 3), rec, None, 64, 64)
    xp, yp, _ = heatmap_coords(P.view(1, 1, J, 1, 3), rec, None, 64, 64)
    hard = hm[0, 0].view(J, -1).argmax(-1)
    hx, hy = (hard % 64).double(), (hard // 64).double()
    to_q = torch.hypot(hx - xq[0, 0, :, 0], hy - yq[0, 0, :, 0])
    to_p = torch.hypot(hx - xp[0, 0, :, 0], hy - yp[0, 0, :, 0])
    assert bool((to_q < to_p).all()) and bool((to_q < 1.0).all())                  # the view alone picks the distractor
    o = offsets(G, cube, torch.float64)

    def check(pose, index, who):
        pose, voxel = pose.double().cpu(), centers.double() + o[index.cpu().long()]
        for name, at in (("pose", pose), ("index voxel", voxel)):
            dp, dq = (at - P).norm(dim=-1), (at - Q).norm(dim=-1)
            print(f"    {who} {name}: distance to P {[round(v, 2) for v in dp.view(-1).tolist()]} cm, to Q {[round(v, 2) for v in dq.view(-1).tolist()]} cm")
            assert bool((2.0 * dp < dq).all()), (who, name)                         # with room: at least twice as near

    ref = statement(hm.double(), conf.double(), centers.double(), rec, None, G, cube, 100.0, THR)
    check(ref["pose"], ref["index"], "float64 statement")
    pose, peak, index, spread, ok = hip.volume_fuse(hm.to(DEV), conf.to(DEV), centers.to(DEV), rec.to(DEV), None, None, G, cube, 100.0, THR)
    torch.cuda.synchronize()
    assert bool(ok.all())
    check(pose, index, "kernel")


# --------------------------------------------------------------------------- determinism and replay

def test_the_forward_gives_the_same_bits_again_alone_and_replayed():
    from egorear_amd import hip
    shape = SHAPES[0]
    B, V, J, H, W, G, _ = shape
    d = shape_data(shape)
    hm, conf, centers, thr, beta, ref = d["cases"]["dropped"]
    h, w, c, rec = hm.to(DEV), conf.to(DEV), centers.to(DEV), d["rec"].to(DEV)
    gp, gk = d["g_pose"].to(DEV), d["g_peak"].to(DEV)
    eager = hip.volume_fuse(h, w, c, rec, None, None, G, CUBE, beta, thr)
    again = hip.volume_fuse(h, w, c, rec, None, None, G, CUBE, beta, thr)
    for a, b in zip(eager, again):
        assert torch.equal(a, b)
    for b_, j_ in ((1, 2), (0, 1)):                                    # a pair's bits do not depend on the batch around it
        one = hip.volume_fuse(h[b_:b_ + 1, :, j_:j_ + 1].contiguous(), w[b_:b_ + 1, :, j_:j_ + 1].contiguous(),
                              c[b_:b_ + 1, j_:j_ + 1].contiguous(), rec, None, None, G, CUBE, beta, thr)
        for a, b in zip(eager, one):
            assert torch.equal(a[b_:b_ + 1, j_:j_ + 1], b)
    noise = d["cases"]["noise"]
    big = hip.volume_fuse(noise[0].to(DEV), noise[1].to(DEV), noise[2].to(DEV), rec, None, None, G, CUBE, noise[4], noise[3])
    big2 = hip.volume_fuse(noise[0].to(DEV), noise[1].to(DEV), noise[2].to(DEV), rec, None, None, G, CUBE, noise[4], noise[3])
    for a, b in zip(big, big2):
        assert torch.equal(a, b)
    torch.cuda.synchronize()
    static = h.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                     # one stream, no parallel branches: forward and backward
        out = hip.volume_fuse(static, w, c, rec, None, None, G, CUBE, beta, thr)
        g = hip.volume_fuse_bwd(static, w, c, rec, None, None, gp, gk, G, CUBE, beta, thr)
    static.copy_(torch.zeros_like(h))
    graph.replay()
    static.copy_(h)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(a, b)
    err, allowed = yardstick("replayed g_hm", g, ref["f32"]["g_hm"], ref["f64"]["g_hm"], own_deviation(d, "g_hm"))
    assert err <= allowed                                             # (LDS float adds: the backward is held to the tolerance only)


# --------------------------------------------------------------------------- heat maps to 3-D through the three launches

def test_decode_joints_3d_volumetric_is_the_three_operators_chained():
    from egorear_amd import decode, hip
    g = torch.Generator().manual_seed(77)
    cams = rig()
    rec = records(cams)
    pts = random_points(2, 5, g)
    hm = bumps(pts, rec, None, 64, 64).float()
    hm[1, :3, 2] = 0.0                                                # joint (1, 2): one view left - its triangulation is not valid
    hm = hm.contiguous().to(DEV).requires_grad_()
    vol, tri, j2 = decode.decode_joints_3d_volumetric(hm, cams, grid=8, cube_cm=32.0, volume_beta=50.0)
    g_pose, g_peak = torch.randn(2, 5, 3, generator=g).to(DEV), torch.randn(2, 5, generator=g).to(DEV)
    (g_hm,) = torch.autograd.grad([vol.pose, vol.peak], [hm], [g_pose, g_peak])
    h = hm.detach()
    coords, maxvals, index, _, stat, _ = hip.soft_argmax(h, 100.0, 0, False, 0.5)
    p3, cost, resid, ok3 = hip.triangulate(coords.view(2, 4, 5, 2), maxvals.view(2, 4, 5), rec.to(DEV), None, 1 / 64, 1 / 64, 0.5, 1e-6)
    want = hip.volume_fuse(h, maxvals.view(2, 4, 5), p3, rec.to(DEV), None, ok3, 8, 32.0, 50.0, 0.5)
    want_g = hip.volume_fuse_bwd(h, maxvals.view(2, 4, 5), p3, rec.to(DEV), None, ok3, g_pose, g_peak, 8, 32.0, 50.0, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(tri.pose, p3) and torch.equal(tri.valid, ok3.bool()) and torch.equal(j2.maxvals, maxvals.view(2, 4, 5))
    for a, b in zip((vol.pose, vol.peak, vol.index, vol.spread), want[:4]):
        assert torch.equal(a, b)
    assert vol.valid.dtype == torch.bool and torch.equal(vol.valid, want[4].bool())
    assert not bool(tri.valid[1, 2]) and not bool(vol.valid[1, 2]) and int(vol.valid.sum()) == 9
    assert float(vol.pose.detach()[1, 2].abs().sum()) == 0.0 and int(vol.index[1, 2]) == -1 and float(g_hm[1, :, 2].abs().sum()) == 0.0
    assert float(g_hm.abs().max()) > 0.0 and bool(torch.isfinite(g_hm).all())
    scale = float(want_g.abs().max())
    assert float((g_hm - want_g).abs().max()) <= 1e-5 * scale         # the same launch twice, up to the order of its LDS adds
    err = (vol.pose.detach().double().cpu() - pts).norm(dim=-1)[vol.valid.cpu()]
    err3 = (tri.pose.detach().double().cpu() - pts).norm(dim=-1)[vol.valid.cpu()]
    print(f"error against the rendered points: volumetric mean {float(err.mean()):.3f} max {float(err.max()):.3f} cm, "
          f"triangulated mean {float(err3.mean()):.3f} max {float(err3.max()):.3f} cm")


def test_bad_launches_are_refused():
    from egorear_amd import hip
    rec = records(rig()).to(DEV)
    hm, conf, centers = torch.zeros(1, 4, 2, 8, 8, device=DEV), torch.ones(1, 4, 2, device=DEV), torch.zeros(1, 2, 3, device=DEV)
    pose, peak, index = torch.empty(1, 2, 3, device=DEV), torch.empty(1, 2, device=DEV), torch.empty(1, 2, dtype=torch.int32, device=DEV)
    spread, ok, g_hm = torch.empty(1, 2, device=DEV), torch.empty(1, 2, dtype=torch.uint8, device=DEV), torch.empty_like(hm)
    nan, inf = float("nan"), float("inf")
    for V, H, W, G, cube, beta in ((1, 8, 8, 8, 40.0, 100.0), (5, 8, 8, 8, 40.0, 100.0), (4, 8, 8, 1, 40.0, 100.0), (4, 8, 8, 33, 40.0, 100.0),
                                   (4, 64, 65, 8, 40.0, 100.0), (4, 8, 8, 8, 0.0, 100.0), (4, 8, 8, 8, inf, 100.0), (4, 8, 8, 8, nan, 100.0),
                                   (4, 8, 8, 8, 40.0, 0.0), (4, 8, 8, 8, 40.0, -1.0), (4, 8, 8, 8, 40.0, inf), (4, 0, 8, 8, 40.0, 100.0)):
        rc = hip.lib.egr_volume_fuse_f32(hm.data_ptr(), conf.data_ptr(), centers.data_ptr(), rec.data_ptr(), None, None, 1, V, 2, H, W, G,
                                         cube, beta, 0.5, pose.data_ptr(), peak.data_ptr(), index.data_ptr(), spread.data_ptr(), ok.data_ptr(),
                                         None)
        assert rc == hip.EINVAL, (V, H, W, G, cube, beta, rc)
        rc = hip.lib.egr_volume_fuse_bwd_f32(hm.data_ptr(), conf.data_ptr(), centers.data_ptr(), rec.data_ptr(), None, None, 1, V, 2, H, W, G,
                                             cube, beta, 0.5, None, None, g_hm.data_ptr(), None)
        assert rc == hip.EINVAL, (V, H, W, G, cube, beta, rc)

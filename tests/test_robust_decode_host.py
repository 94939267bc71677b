"""CPU-side checks of the multi-peak decoder and the consensus triangulation (egorear_amd/decode.py): both operators are
registered with fake implementations and no gradient, the public functions give the documented shapes on meta tensors,
`decode_joints_3d_robust` traces under Dynamo as one graph of three launches, bad parameters and CPU tensors are refused before any
launch, the library exports the two entries - and the float64 statements of both kernels (tests/robust_statement.py), which the GPU
tests compare the kernels with, are themselves held to known answers and to the distractor scene here."""
import ctypes

import pytest
import torch

import fisheye_statement as FS
import robust_statement as RS


def _meta_cams(V=4):
    return torch.empty(V, 30, device="meta")


def test_operators_are_registered_with_fake_implementations_and_no_gradient():
    from egorear_amd import decode
    assert hasattr(torch.ops.egorear_amd, "find_peaks") and hasattr(torch.ops.egorear_amd, "consensus")
    for B, V, J, K, rw in ((2, 4, 15, 3, False), (3, 2, 5, 1, False), (1, 3, 16, 4, True), (2, 4, 2, 4, True)):
        hm = torch.empty(B, V, J, 64, 48, device="meta", requires_grad=True)
        coords, score, index, count = decode.find_peaks_op(hm, K, 1, 2, 100.0, 0.5)
        assert coords.shape == (B, V, J, K, 2) and score.shape == (B, V, J, K) and index.shape == (B, V, J, K) and count.shape == (B, V, J)
        assert coords.dtype == score.dtype == torch.float32 and index.dtype == count.dtype == torch.int32
        assert not any(t.requires_grad for t in (coords, score, index, count))
        ctm = torch.empty(B, V, 4, 4, device="meta") if rw else None
        out = decode.consensus_op(coords, score, index, _meta_cams(V), ctm, 1 / 48, 1 / 64, 2.0, 2, 1e-6)
        choice, sel_coords, sel_conf, total, inliers, hyp = out
        assert choice.shape == (B, V, J) and sel_coords.shape == (B, V, J, 2) and sel_conf.shape == (B, V, J)
        assert total.shape == inliers.shape == hyp.shape == (B, J)
        assert choice.dtype == inliers.dtype == hyp.dtype == torch.int32 and sel_coords.dtype == sel_conf.dtype == total.dtype == torch.float32
        assert not any(t.requires_grad for t in out)


def test_public_functions_give_the_documented_shapes_on_meta():
    from egorear_amd import decode
    cams = FS.rig()
    for B, V, J, K, rw in ((2, 4, 15, 3, False), (1, 2, 3, 1, False), (3, 3, 2, 4, False), (2, 4, 5, 4, True), (1, 2, 1, 1, True)):
        hm = torch.empty(B, V, J, 64, 64, device="meta")
        ctm = torch.empty(B, V, 4, 4, device="meta") if rw else None
        peaks = decode.find_peaks_2d(hm, k=K)
        assert isinstance(peaks, decode.Peaks2D) and peaks._fields == ("coords", "score", "index", "count")
        assert peaks.coords.shape == (B, V, J, K, 2) and peaks.score.shape == peaks.index.shape == (B, V, J, K) and peaks.count.shape == (B, V, J)
        agreed = decode.select_consistent(peaks, cams[:V], ctm, heatmap_size=(64, 64))
        assert isinstance(agreed, decode.Consensus) and agreed._fields == ("coords", "conf", "choice", "score", "inliers", "hypothesis")
        assert agreed.coords.shape == (B, V, J, 2) and agreed.conf.shape == agreed.choice.shape == (B, V, J)
        assert agreed.score.shape == agreed.inliers.shape == agreed.hypothesis.shape == (B, J)
        assert agreed.choice.dtype == agreed.inliers.dtype == agreed.hypothesis.dtype == torch.int32
        tri, agreed2, peaks2 = decode.decode_joints_3d_robust(hm, cams[:V], ctm, k=K, max_reproj=2.0)
        assert isinstance(tri, decode.Joints3D) and isinstance(agreed2, decode.Consensus) and isinstance(peaks2, decode.Peaks2D)
        assert tri.pose.shape == (B, J, 3) and tri.residual.shape == (B, V, J) and tri.valid.dtype == torch.bool
        assert agreed2.coords.shape == (B, V, J, 2) and peaks2.coords.shape == (B, V, J, K, 2)
    named, _, _ = decode.decode_joints_3d_robust(torch.empty(2, 4, 15, 32, 48, device="meta"), "ego4view_syn")
    assert named.pose.shape == (2, 15, 3)


def test_decode_joints_3d_robust_traces_as_one_graph_of_three_launches():
    import torch._dynamo as dynamo
    from egorear_amd import decode
    lin = torch.nn.Conv2d(4, 15, 1, device="meta")
    cams = FS.rig()

    def serving_side(feat):
        hm = lin(feat).view(2, 4, 15, 64, 64)
        tri, agreed, peaks = decode.decode_joints_3d_robust(hm, cams, k=3, max_reproj=2.0)
        return tri.pose, tri.valid, agreed.choice, peaks.count

    feat = torch.empty(8, 4, 64, 64, device="meta")
    pose, valid, choice, count = serving_side(feat)               # (also warms the record cache: the upload is not part of a graph)
    assert pose.shape == (2, 15, 3) and not pose.requires_grad and valid.shape == (2, 15) and choice.shape == (2, 4, 15)
    dynamo.reset()
    ex = dynamo.explain(serving_side)(feat)
    assert ex.graph_break_count == 0 and ex.graph_count == 1, ex
    targets = [str(nd.target) for g in ex.graphs for nd in g.graph.nodes if nd.op == "call_function"]
    for name in ("egorear_amd.find_peaks", "egorear_amd.consensus", "egorear_amd.triangulate"):
        assert sum(name in t for t in targets) == 1, (name, targets)
    assert not any("soft_argmax" in t for t in targets), targets


def test_bad_parameters_are_refused_before_any_launch():
    from egorear_amd import decode, hip
    cams = FS.rig()
    hm = torch.zeros(1, 4, 2, 16, 16, device="meta")
    for kw in ({"k": 0}, {"k": 5}, {"k": 2.0}, {"nms_radius": 0}, {"nms_radius": 4}, {"refine_radius": -1}, {"refine_radius": 4},
               {"beta": 0.0}, {"beta": float("inf")}, {"threshold": float("nan")}):
        with pytest.raises(ValueError):
            decode.find_peaks_2d(hm, **kw)
        with pytest.raises(ValueError):
            decode.decode_joints_3d_robust(hm, cams, **kw)
        with pytest.raises(ValueError):
            hip.find_peaks(torch.zeros(2, 16, 16), **{("min_score" if k == "threshold" else k): v for k, v in kw.items()})
    for big in (torch.zeros(1, 4, 2, 64, 65, device="meta"), torch.zeros(1, 4, 2, 1, 4097, device="meta"), torch.zeros(1, 4, 2, 0, 8, device="meta")):
        with pytest.raises(ValueError):                                              # 1 <= H * W <= 4096
            decode.find_peaks_2d(big)
        with pytest.raises(ValueError):
            decode.find_peaks_op(big, 3, 1, 2, 100.0, 0.5)
    with pytest.raises(ValueError):
        decode.find_peaks_2d(torch.zeros(4, 2, 16, 16, device="meta"))               # (B, V, J, H, W) only
    with pytest.raises(ValueError):
        decode.find_peaks_2d(hm.double())
    peaks = decode.find_peaks_2d(hm)
    for kw in ({"max_reproj": 0.0}, {"max_reproj": -1.0}, {"max_reproj": float("nan")}, {"min_views": 1}, {"min_views": 5},
               {"min_views": 2.0}, {"min_det_ratio": -1.0}, {"heatmap_size": (0, 16)}):
        with pytest.raises(ValueError):
            decode.select_consistent(peaks, cams, **kw)
        if "heatmap_size" not in kw:
            with pytest.raises(ValueError):
                decode.decode_joints_3d_robust(hm, cams, **kw)
    three = decode.find_peaks_2d(hm[:, :3])
    with pytest.raises(ValueError):
        decode.select_consistent(three, cams[:3], min_views=4)                       # V + 1
    with pytest.raises(ValueError):
        decode.select_consistent(peaks, cams[:3])                                    # four views, three cameras
    with pytest.raises(ValueError):
        decode.consensus_op(peaks.coords, peaks.score, peaks.index, torch.empty(4, 17, device="meta"), None, 1 / 16, 1 / 16, 2.0, 2, 1e-6)
    with pytest.raises(ValueError):
        decode.consensus_op(peaks.coords, peaks.score, peaks.index.long(), _meta_cams(), None, 1 / 16, 1 / 16, 2.0, 2, 1e-6)
    with pytest.raises(ValueError):
        decode.consensus_op(peaks.coords, peaks.score[..., :2], peaks.index, _meta_cams(), None, 1 / 16, 1 / 16, 2.0, 2, 1e-6)
    with pytest.raises(ValueError):
        decode.select_consistent(peaks, cams, coord_trans_mat=torch.empty(1, 3, 4, 4, device="meta"))
    with pytest.raises(ValueError):
        decode.decode_joints_3d_robust(torch.zeros(1, 5, 2, 16, 16, device="meta"), cams + cams[:1])
    with pytest.raises(ValueError):
        decode.decode_joints_3d_robust(torch.zeros(1, 1, 2, 16, 16, device="meta"), cams[:1])


def test_cpu_tensors_are_refused():
    from egorear_amd import decode, hip
    cams = FS.rig()
    hm = torch.zeros(1, 4, 2, 16, 16)
    with pytest.raises(ValueError, match="no CPU path"):
        decode.find_peaks_2d(hm)
    with pytest.raises(ValueError, match="no CPU path"):
        decode.decode_joints_3d_robust(hm, cams)
    cpu_peaks = decode.Peaks2D(torch.zeros(1, 4, 2, 3, 2), torch.zeros(1, 4, 2, 3), torch.zeros(1, 4, 2, 3, dtype=torch.int32),
                               torch.zeros(1, 4, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="no CPU path"):
        decode.select_consistent(cpu_peaks, cams, heatmap_size=(16, 16))
    with pytest.raises((NotImplementedError, RuntimeError)):                         # the operators themselves: no CPU kernel, no fallback
        decode.find_peaks_op(hm, 3, 1, 2, 100.0, 0.5)
    with pytest.raises((NotImplementedError, RuntimeError)):
        decode.consensus_op(cpu_peaks.coords, cpu_peaks.score, cpu_peaks.index, torch.zeros(4, 30), None, 1 / 16, 1 / 16, 2.0, 2, 1e-6)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.find_peaks(hm)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.consensus(cpu_peaks.coords, cpu_peaks.score, cpu_peaks.index, torch.zeros(4, 30))


def test_the_library_exports_the_two_entries():
    from egorear_amd import hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ("egr_peaks_f32", "egr_consensus_f32"):
        assert name in hip.EXPORTS and hasattr(lib, name), name


# --------------------------------------------------------------------------- the float64 statements, on the CPU

def test_statement_known_answers_of_the_peaks():
    const = torch.full((1, 6, 5), 0.75, dtype=torch.float64)
    coords, score, index, count = RS.peaks_statement(const, 3, 1, 2, 100.0, 0.5)
    assert index.tolist() == [[0, -1, -1]] and count.tolist() == [1] and score.tolist() == [[0.75, 0.0, 0.0]]
    assert float(coords[0, 1:].abs().sum()) == 0.0
    # a constant window: the weights are equal and the mean is that of the clipped window, columns 0..2 and rows 0..2
    assert coords[0, 0].tolist() == [1.0, 1.0]
    low = torch.full((1, 6, 5), 0.25, dtype=torch.float64)
    assert RS.peaks_statement(low, 2, 1, 2, 100.0, 0.5)[3].tolist() == [0]
    plateau = torch.zeros(1, 5, 7, dtype=torch.float64)
    plateau[0, 2, 3:6] = 0.9                                                         # three equal pixels in a row
    plateau[0, 4, 0] = 0.6
    coords, score, index, count = RS.peaks_statement(plateau, 4, 1, 0, 100.0, 0.5)
    assert index.tolist() == [[2 * 7 + 3, 4 * 7 + 0, -1, -1]] and count.tolist() == [2]      # the plateau's first pixel, once
    assert coords[0, 0].tolist() == [3.0, 2.0] and coords[0, 1].tolist() == [0.0, 4.0]       # refine_radius 0: the pixel itself
    # at nms_radius 1 the plateau's last pixel has only its middle one for an earlier equal neighbour - still no peak; the
    # middle and last pixels two apart are both peaks at radius 1 when the middle one is lowered
    plateau[0, 2, 4] = 0.5
    assert RS.peaks_statement(plateau, 4, 1, 0, 100.0, 0.5)[2].tolist() == [[2 * 7 + 3, 2 * 7 + 5, 4 * 7 + 0, -1]]
    assert RS.peaks_statement(plateau, 4, 2, 0, 100.0, 0.5)[2].tolist() == [[2 * 7 + 3, 4 * 7 + 0, -1, -1]]
    odd = torch.zeros(1, 4, 4, dtype=torch.float64)
    odd[0, 1, 1], odd[0, 1, 2], odd[0, 3, 3], odd[0, 0, 3] = float("nan"), 0.8, float("inf"), float("-inf")
    coords, score, index, count = RS.peaks_statement(odd, 2, 1, 1, 100.0, 0.5)
    assert index.tolist() == [[1 * 4 + 2, -1]]                                        # NaN is -inf; +inf is no peak and hides (2, 2)'s ring only
    assert bool(torch.isfinite(coords).all())


def _projected_candidates(V, K, g, rw=False):
    """Exact projections of random points as candidate 0 of every view, a higher-scored distractor in view 1 (slot order: best first)."""
    B, J = 2, 5
    cams = FS.rig("ego4view_rw" if rw else "ego4view_syn")[:V]
    rec = FS.records(cams)
    ctm = FS.random_ctm(B, V, cams, g) if rw else None
    pts = FS.random_points(B, J, g)
    true = FS.project(pts, rec, ctm) * RS.HM
    cand = torch.zeros(B, V, J, K, 2, dtype=torch.float64)
    cscore = torch.zeros(B, V, J, K, dtype=torch.float64)
    cindex = torch.full((B, V, J, K), -1, dtype=torch.int64)
    cand[:, :, :, 0], cscore[:, :, :, 0], cindex[:, :, :, 0] = true, 0.9, 1
    if K > 1:
        cand[:, 1, :, 1], cscore[:, 1, :, 1], cindex[:, 1, :, 1] = true[:, 1], 0.9, 1      # the true one moves to slot 1 ...
        cand[:, 1, :, 0] = true[:, 1] + torch.tensor([13.0, -11.0], dtype=torch.float64)   # ... behind a distractor scored 1.2
        cscore[:, 1, :, 0] = 1.2
    return rec, ctm, pts, cand, cscore, cindex


@pytest.mark.parametrize("V,K,rw", [(4, 3, False), (3, 2, False), (4, 4, True), (2, 1, False)])
def test_statement_chooses_the_candidates_the_views_agree_on(V, K, rw):
    g = torch.Generator().manual_seed(11 * V + K)
    rec, ctm, pts, cand, cscore, cindex = _projected_candidates(V, K, g, rw)
    ref = RS.consensus_statement(cand, cscore, cindex, rec, ctm, 1.0 / RS.HM, 1.0 / RS.HM, 2.0, 2)
    want = torch.zeros(2, V, 5, dtype=torch.int32)
    if K > 1:
        want[:, 1] = 1
    assert torch.equal(ref["choice"], want) and bool((ref["inliers"] == V).all()) and bool((ref["hyp"] >= 0).all())
    assert torch.equal(ref["sel_coords"], RS.gather_choice(cand, cscore, want)[0]) and bool((ref["sel_conf"] == 0.9).all())
    assert float((ref["score"] - 0.9 * V).abs().max()) < 1e-9
    pose, _, _, ok = FS.statement(ref["sel_coords"], ref["sel_conf"], rec, ctm, 1.0 / RS.HM, 1.0 / RS.HM)
    err = float((pose - pts).norm(dim=-1).max())
    print(f"V {V} K {K} rw {rw}: pose error {err:.3e} cm, decided {int(RS.decided(ref).sum())} of {ref['hyp'].numel()}")
    assert bool(ok.all()) and err < 1e-3
    if V > 2:
        assert bool(RS.decided(ref).all())


def test_statement_reports_no_consensus_for_inconsistent_candidates():
    g = torch.Generator().manual_seed(3)
    rec, _, pts, cand, cscore, cindex = _projected_candidates(4, 2, g)
    # every view looks at a different point: no two rays meet within 2 px of a third view's candidate, and min_views = 3 asks for one
    for v in range(4):
        cand[:, v, :, 0] = (FS.project(FS.random_points(2, 5, g), rec, None) * RS.HM)[:, v]
    cindex[..., 1] = -1                                                               # and the second slots are empty
    ref = RS.consensus_statement(cand, cscore, cindex, rec, None, 1.0 / RS.HM, 1.0 / RS.HM, 2.0, 3)
    assert bool((ref["hyp"] == -1).all()) and bool((ref["choice"] == -1).all()) and bool((ref["inliers"] == 0).all())
    assert float(ref["score"].abs().sum()) == 0.0 and float(ref["sel_coords"].abs().sum()) == 0.0 and float(ref["sel_conf"].abs().sum()) == 0.0
    # candidates that do not exist give none either: NaN coordinates, non-positive or infinite scores, index -1
    rec, _, pts, cand, cscore, cindex = _projected_candidates(4, 2, g)
    cand[:, 0, :, :, 0], cscore[:, 1], cscore[:, 2], cindex[:, 3] = float("nan"), 0.0, float("inf"), -1
    ref = RS.consensus_statement(cand, cscore, cindex, rec, None, 1.0 / RS.HM, 1.0 / RS.HM, 2.0, 2)
    assert bool((ref["hyp"] == -1).all()) and bool((ref["choice"] == -1).all())


@pytest.fixture(scope="module")
def scene():
    return RS.distractor_scene(2)


def test_the_distractor_scene_on_the_statements(scene):
    """The scene of DESIGN.md 5p at B = 2: the robust chain is within 15 cm everywhere, the top-1 chain is beyond 15 cm for at least
    half the pairs (float64 prototype over 10 frames: robust maximum 11.04 cm, top-1 mean 91 cm)."""
    hm, rec, pts = scene["hm"].double(), scene["rec"], scene["pts"]
    robust, ok, con, _ = RS.robust_chain(hm, rec)
    top1, ok1 = RS.top1_chain(hm, rec)
    e_r, e_1 = (robust - pts).norm(dim=-1), (top1 - pts).norm(dim=-1)
    print(f"robust: mean {float(e_r.mean()):.3f} cm, max {float(e_r.max()):.3f} cm; top-1: mean {float(e_1.mean()):.2f} cm, "
          f"{int((e_1 > 15).sum())} of {e_1.numel()} pairs beyond 15 cm; inliers {sorted(set(con['inliers'].view(-1).tolist()))}")
    assert bool(ok.all()) and bool(ok1.all())
    assert float(e_r.max()) < 15.0
    assert int((e_1 > 15.0).sum()) * 2 >= e_1.numel()
    assert bool((con["inliers"] == 4).all()) and bool(RS.decided(con).all())

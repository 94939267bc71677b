"""Consensus over candidate peaks on the GPU (egr_consensus_f32, egorear_amd/decode.py) against the float64 statement of
tests/robust_statement.py, and the robust chain end to end.  The selection is discrete: `choice`, `inliers` and `hyp` must equal the
statement's for every pair that is decided - the statement's winning score leads the best hypothesis with a different choice by more
than 1e-6, relative - and at most 5 % of a case's pairs may be undecided, which the float64 statement alone is held to first.
`sel_coords` / `sel_conf` are copies: bit-equal to the gathered candidates.  `score` meets the yardstick of fisheye_statement.py."""
import pytest
import torch

import fisheye_statement as FS
import robust_statement as RS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HM, TAU = RS.HM, 2.0
# (B, V, J, K, rw): the product's four views; the two front cameras with every slot; three views; rw with rotations up to 0.05 rad
SHAPES = [(2, 4, 3, 3, False), (1, 2, 1, 4, False), (3, 3, 2, 2, False), (2, 4, 2, 3, True)]
CASES = ("projected", "random", "emptied", "nonfinite")


def make_case(case, shape, g, true):
    """cand (B, V, J, K, 2), cscore (B, V, J, K) float32, cindex (B, V, J, K) int32, min_views."""
    B, V, J, K, _ = shape
    cand = torch.rand(B, V, J, K, 2, generator=g) * (HM - 1)                        # distractors anywhere on the map
    cscore = 0.5 + 0.8 * torch.rand(B, V, J, K, generator=g)
    cindex = torch.randint(0, HM * HM, (B, V, J, K), generator=g, dtype=torch.int32)
    min_views = 2
    # "random" stops here: such candidates mostly agree on nothing, and where two rays do meet a few hypotheses compete
    if case != "random":               # the projections, 0.05 px of noise, in a random slot of every view
        slot = torch.randint(0, K, (B, V, J), generator=g)
        noisy = true + 0.05 * torch.randn(B, V, J, 2, generator=g)
        cand.scatter_(3, slot.view(B, V, J, 1, 1).expand(B, V, J, 1, 2), noisy.unsqueeze(3))
        if K > 1:                      # and one unfilled slot - index -1 - next to it in every other pair
            spare = (slot + 1) % K
            cindex.scatter_(3, spare.unsqueeze(-1), torch.where((torch.arange(B * V * J).view(B, V, J, 1) % 2) == 0, -1,
                                                                cindex.gather(3, spare.unsqueeze(-1))).to(torch.int32))
    if case == "emptied":              # pair n loses (n + 1) % (V + 1) of its views altogether: V, ..., two, one and no view is left
        for n in range(B * J):
            for i in range((n + 1) % (V + 1)):
                cindex[n // J, (n + i) % V, n % J, :] = -1
    if case == "nonfinite":            # NaN / inf coordinates and scores, non-positive scores: those candidates do not exist
        r = torch.rand(B, V, J, K, generator=g)
        cand[..., 0][r < 0.08] = float("nan")
        cand[..., 1][(r >= 0.08) & (r < 0.16)] = float("inf")
        cscore[(r >= 0.16) & (r < 0.24)] = float("nan")
        cscore[(r >= 0.24) & (r < 0.32)] = float("inf")
        cscore[(r >= 0.32) & (r < 0.40)] = 0.0
        cscore[(r >= 0.40) & (r < 0.45)] = -0.7
    return cand.contiguous(), cscore.contiguous(), cindex.contiguous(), min_views


_CACHE = {}


def shape_data(shape):
    """Per case the candidates and the statement in float64 and in float32, computed once (on the CPU)."""
    if shape in _CACHE:
        return _CACHE[shape]
    B, V, J, K, rw = shape
    g = torch.Generator().manual_seed(1000 * B + 100 * V + 10 * J + K)
    cams = FS.rig("ego4view_rw" if rw else "ego4view_syn")[:V]
    rec = FS.records(cams)
    ctm = FS.random_ctm(B, V, cams, g) if rw else None
    pts = FS.random_points(B, J, g)
    true = (FS.project(pts, rec, ctm) * HM).float()
    cases = {}
    for case in CASES:
        cand, cscore, cindex, mv = make_case(case, shape, g, true)
        f64 = RS.consensus_statement(cand.double(), cscore.double(), cindex, rec, ctm, 1.0 / HM, 1.0 / HM, TAU, mv)
        f32 = RS.consensus_statement(cand, cscore, cindex, rec, ctm, 1.0 / HM, 1.0 / HM, TAU, mv)
        cases[case] = (cand, cscore, cindex, mv, f64, f32)
    _CACHE[shape] = {"cams": cams, "rec": rec, "ctm": ctm, "pts": pts, "cases": cases}
    return _CACHE[shape]


def launch(d, cand, cscore, cindex, mv):
    from egorear_amd import hip
    ctm = None if d["ctm"] is None else d["ctm"].to(DEV)
    return hip.consensus(cand.to(DEV), cscore.to(DEV), cindex.to(DEV), d["rec"].to(DEV), ctm, 1.0 / HM, 1.0 / HM, TAU, mv, FS.MIN_DET)


@pytest.mark.parametrize("shape", SHAPES)
def test_consensus_against_the_float64_statement(shape):
    d = shape_data(shape)
    B, V, J, K, _ = shape
    bad = []
    for case in CASES:
        cand, cscore, cindex, mv, f64, f32 = d["cases"][case]
        sure = RS.decided(f64)
        found = f64["hyp"] >= 0
        print(f"{shape} {case}: min_views {mv}, {int(found.sum())} of {B * J} pairs with a consensus, {int((~sure).sum())} undecided, "
              f"inliers {sorted(set(f64['inliers'].view(-1).tolist()))}")
        assert int((~sure).sum()) * 20 <= B * J, (shape, case)                        # the condition, on the statement alone
        choice, sel_coords, sel_conf, score, inliers, hyp = (t.cpu() for t in launch(d, cand, cscore, cindex, mv))
        assert torch.equal(hyp[sure], f64["hyp"][sure]), (shape, case)
        assert torch.equal(inliers[sure], f64["inliers"][sure]), (shape, case)
        assert torch.equal(choice.permute(0, 2, 1)[sure], f64["choice"].permute(0, 2, 1)[sure]), (shape, case)
        want_coords, want_conf = RS.gather_choice(cand, cscore, choice)               # copies of the chosen candidates, bit for bit
        assert torch.equal(sel_coords.view(torch.int32), want_coords.view(torch.int32)), (shape, case)
        assert torch.equal(sel_conf.view(torch.int32), want_conf.view(torch.int32)), (shape, case)
        none = hyp < 0
        assert bool((choice.permute(0, 2, 1)[none] == -1).all()) and float(score[none].abs().sum()) == 0.0 and int(inliers[none].sum()) == 0
        assert torch.equal(inliers, (choice >= 0).sum(1).to(torch.int32)) and bool((inliers[~none] >= mv).all())
        assert bool(torch.isfinite(score).all()) and bool(torch.isfinite(sel_coords).all()) and bool(torch.isfinite(sel_conf).all())
        # the score: the fp32 evaluation's score of the hypothesis the float64 statement chose is the yardstick's other leg
        own = f32["all_score"].gather(2, f64["hyp"].long().clamp(min=0).unsqueeze(-1)).squeeze(-1)
        keep = sure & found
        if bool(keep.any()):
            err, allowed = FS.yardstick("score", score[keep], own[keep], f64["score"][keep])
            if not err <= allowed:
                bad.append((shape, case, err, allowed))
        # what the cases are for
        if case == "projected":
            assert bool(found.all()) and int(f64["inliers"].min()) == V
        if case == "random" and V > 2:
            assert 0 < int(found.sum()) < B * J
        if case == "emptied" and B * J >= V + 1:
            assert sorted(set(f64["inliers"].view(-1).tolist())) == [0] + list(range(2, V + 1))       # one view left: no consensus
    assert not bad, bad


def test_two_runs_agree_and_a_pair_alone_gives_its_bits_in_the_batch():
    for shape in (SHAPES[0], SHAPES[3]):
        d = shape_data(shape)
        B, V, J, K, _ = shape
        for case in ("projected", "nonfinite"):
            cand, cscore, cindex, mv = d["cases"][case][:4]
            first, again = launch(d, cand, cscore, cindex, mv), launch(d, cand, cscore, cindex, mv)
            for a, b in zip(first, again):
                assert torch.equal(a, b), (shape, case)
            b, j = B - 1, J - 1
            alone = dict(d, ctm=None if d["ctm"] is None else d["ctm"][b:b + 1].contiguous())
            one = launch(alone, cand[b:b + 1, :, j:j + 1].contiguous(), cscore[b:b + 1, :, j:j + 1].contiguous(),
                         cindex[b:b + 1, :, j:j + 1].contiguous(), mv)
            for a, o in zip(first[:3], one[:3]):                                       # (B, V, J, ...) outputs
                assert torch.equal(a[b:b + 1, :, j:j + 1], o), (shape, case)
            for a, o in zip(first[3:], one[3:]):                                       # (B, J) outputs
                assert torch.equal(a[b:b + 1, j:j + 1], o), (shape, case)
    torch.cuda.synchronize()


def test_the_entry_refuses_what_it_does_not_support():
    from egorear_amd import hip
    rec = FS.records(FS.rig()).to(DEV)
    cand, cscore = torch.zeros(1, 4, 2, 3, 2, device=DEV), torch.ones(1, 4, 2, 3, device=DEV)
    cindex = torch.zeros(1, 4, 2, 3, dtype=torch.int32, device=DEV)
    out = (torch.empty(1, 4, 2, dtype=torch.int32, device=DEV), torch.empty(1, 4, 2, 2, device=DEV), torch.empty(1, 4, 2, device=DEV),
           torch.empty(1, 2, device=DEV), torch.empty(1, 2, dtype=torch.int32, device=DEV), torch.empty(1, 2, dtype=torch.int32, device=DEV))
    ptrs = [t.data_ptr() for t in out]
    ok = dict(V=4, K=3, sx=1.0, tau=2.0, mv=2, det=1e-6)
    for change in ({"V": 1}, {"V": 5}, {"K": 0}, {"K": 5}, {"sx": 0.0}, {"tau": 0.0}, {"tau": -1.0}, {"tau": float("nan")}, {"mv": 1}, {"mv": 5},
                   {"det": -1.0}, {"det": float("inf")}):
        a = dict(ok, **change)
        rc = hip.lib.egr_consensus_f32(cand.data_ptr(), cscore.data_ptr(), cindex.data_ptr(), rec.data_ptr(), None, 1, a["V"], 2, a["K"],
                                       a["sx"], 1.0, a["tau"], a["mv"], a["det"], *ptrs, None)
        assert rc == hip.EINVAL, (change, rc)


# --------------------------------------------------------------------------- the consensus point is the triangulated point

def support(p, cand, cscore, cindex, rec, ctm):
    """RS.consensus_statement's support of the points p (B, J, 3), in p's dtype: (score (B, J), inliers (B, J) int32)."""
    exists = RS.candidates_exist(cand, cscore, cindex)
    zero = torch.zeros_like(cscore)
    xy = torch.where(exists.unsqueeze(-1), cand, torch.zeros_like(cand))
    proj = FS.project(p, rec, None if ctm is None else ctm.to(p.dtype), 1.0 / HM, 1.0 / HM)
    keep = 1.0 - ((proj.unsqueeze(3) - xy) ** 2).sum(-1) / (TAU * TAU)
    best = torch.where(exists & (keep > 0), torch.where(exists, cscore, zero) * keep, zero).max(-1)[0]      # (B, V, J): 0 = no support
    return best.sum(1), (best > 0).sum(1).to(torch.int32)


# (B, V, J, K, rw): one hypothesis a pair; 96 of them, two passes over the 64 lanes
SHARED = [(2, 2, 3, 1, False), (2, 2, 3, 1, True), (2, 4, 3, 4, False), (2, 4, 3, 4, True)]


@pytest.mark.parametrize("shape", SHARED)
def test_the_winning_hypothesis_scores_what_its_triangulated_point_scores(shape):
    """The consensus solves its two rays with the triangulation's code (egr_rays.h): egr_triangulate_f32 of the winning hypothesis's
    two candidates gives the point whose reprojections, in float64 on the host, support the candidates with the kernel's `score`
    (the yardstick of test_consensus_against_the_float64_statement) and in exactly the kernel's `inliers` views."""
    from egorear_amd import hip
    B, V, J, K, rw = shape
    g = torch.Generator().manual_seed(7000 + 100 * V + 10 * K + int(rw))
    cams = FS.rig("ego4view_rw" if rw else "ego4view_syn")[:V]
    rec = FS.records(cams)
    ctm = FS.random_ctm(B, V, cams, g) if rw else None
    true = (FS.project(FS.random_points(B, J, g), rec, ctm) * HM).float()
    cand, cscore, cindex, mv = make_case("projected", shape, g, true)
    assert float(cscore.min()) >= FS.THR                                               # every candidate's view counts in the triangulation
    f64 = RS.consensus_statement(cand.double(), cscore.double(), cindex, rec, ctm, 1.0 / HM, 1.0 / HM, TAU, mv)
    f32 = RS.consensus_statement(cand, cscore, cindex, rec, ctm, 1.0 / HM, 1.0 / HM, TAU, mv)
    sure = RS.decided(f64)
    assert int((~sure).sum()) * 20 <= B * J and bool((f64["hyp"] >= 0).all()), shape     # on the statement alone
    d = {"rec": rec, "ctm": ctm}
    _, _, _, score, inliers, hyp = (t.cpu() for t in launch(d, cand, cscore, cindex, mv))
    assert torch.equal(hyp[sure], f64["hyp"][sure]) and torch.equal(inliers[sure], f64["inliers"][sure]), shape
    assert bool((hyp >= 0).all())
    # the winning hypothesis's two candidates, every other view excluded by a confidence of 0
    coords, conf = torch.zeros(B, V, J, 2), torch.zeros(B, V, J)
    pairs = RS.view_pairs(V)
    for b in range(B):
        for j in range(J):
            h = int(hyp[b, j])
            (va, vb), ka, kb = pairs[h // (K * K)], (h // K) % K, h % K
            for v, k in ((va, ka), (vb, kb)):
                coords[b, v, j], conf[b, v, j] = cand[b, v, j, k], cscore[b, v, j, k]
    pts, _, _, ok = (t.cpu() for t in hip.triangulate(coords.to(DEV), conf.to(DEV), rec.to(DEV), None if ctm is None else ctm.to(DEV),
                                                        1.0 / HM, 1.0 / HM, FS.THR, FS.MIN_DET))
    assert bool(ok.all()), shape
    want, views = support(pts.double(), cand.double(), cscore.double(), cindex, rec, ctm)
    print(f"{shape}: hypotheses {sorted(set(hyp.view(-1).tolist()))}, inliers {sorted(set(inliers.view(-1).tolist()))}")
    assert torch.equal(inliers, views), shape
    own = f32["all_score"].gather(2, f64["hyp"].long().unsqueeze(-1)).squeeze(-1)
    err, allowed = FS.yardstick("score", score[sure], own[sure], want[sure])
    assert err <= allowed, (shape, err, allowed)


# --------------------------------------------------------------------------- heat maps to 3-D, robustly

@pytest.fixture(scope="module")
def scene():
    s = RS.distractor_scene(2)
    s["f64"] = RS.robust_chain(s["hm"].double(), s["rec"])
    s["f32"] = RS.robust_chain(s["hm"], s["rec"])
    return s


def test_robust_chain_on_the_distractor_scene(scene):
    """The bounds of test_robust_decode_host.py, on the kernels: every robust error < 15 cm, the top-1 error > 15 cm for at least half
    the pairs; and the robust pose is within the triangulation's yardstick of the statement chain's pose."""
    from egorear_amd import decode
    hm, pts = scene["hm"].to(DEV), scene["pts"]
    rob, con, peaks = decode.decode_joints_3d_robust(hm, scene["cams"], k=3, max_reproj=TAU)
    top1, _ = decode.decode_joints_3d(hm, scene["cams"])
    torch.cuda.synchronize()
    e_r, e_1 = (rob.pose.double().cpu() - pts).norm(dim=-1), (top1.pose.double().cpu() - pts).norm(dim=-1)
    print(f"robust: mean {float(e_r.mean()):.3f} cm, max {float(e_r.max()):.3f} cm; top-1: mean {float(e_1.mean()):.2f} cm, "
          f"{int((e_1 > 15).sum())} of {e_1.numel()} pairs beyond 15 cm")
    assert bool(rob.valid.all()) and float(e_r.max()) < 15.0
    assert int((e_1 > 15.0).sum()) * 2 >= e_1.numel()
    p64, ok64, con64, peaks64 = scene["f64"]
    assert bool(RS.decided(con64).all())
    assert torch.equal(con.choice.cpu(), con64["choice"]) and torch.equal(con.hypothesis.cpu(), con64["hyp"])
    assert torch.equal(con.inliers.cpu(), con64["inliers"]) and bool((con.inliers == 4).all())
    assert torch.equal(peaks.index.cpu(), peaks64[2]) and torch.equal(peaks.count.cpu(), peaks64[3])
    err, allowed = FS.yardstick("pose", rob.pose, scene["f32"][0], p64)
    assert err <= allowed, (err, allowed)
    # the residual reports the accepted views, which here are all four; the distractor view's own top-1 peak is not among them
    assert float(rob.residual.max()) < 15.0 and bool((con.conf > 0.5).all())
    by_name, _, _ = decode.decode_joints_3d_robust(hm, "ego4view_syn", k=3, max_reproj=TAU)
    assert torch.equal(by_name.pose, rob.pose)


def test_the_chain_replays_from_a_graph_bit_for_bit(scene):
    from egorear_amd import decode
    hm = scene["hm"].to(DEV)
    eager = decode.decode_joints_3d_robust(hm, scene["cams"], k=3, max_reproj=TAU)      # (also warms the record cache)
    torch.cuda.synchronize()
    static = hm.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                      # one stream, no parallel branches
        out = decode.decode_joints_3d_robust(static, scene["cams"], k=3, max_reproj=TAU)
    static.zero_()
    graph.replay()
    static.copy_(hm)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        for x, y in zip(a, b):
            assert torch.equal(x, y)

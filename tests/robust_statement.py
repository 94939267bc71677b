"""Float64 statements of the multi-peak decoder (egr_peaks_f32) and of the consensus over its candidates (egr_consensus_f32), DESIGN.md 5p,
written in elementwise torch operations, plus the distractor scene the robust chain is judged on.  Shared by test_robust_decode_host.py,
test_gpu_peaks.py, test_gpu_consensus.py and tools/robust_accuracy.py; every function computes in the dtype of its first operand, so
the same code gives the float64 statement and torch's fp32 evaluation of it (the yardstick of fisheye_statement.py).  The camera math -
the triangulation of a hypothesis and the Horner projection of its point - is fisheye_statement's."""
import torch

import fisheye_statement as FS

HM = FS.HM
NEG = float("-inf")


# --------------------------------------------------------------------------- peaks

def peaks_statement(hm, K, rn, r, beta, min_score):
    """hm (N, H, W) -> coords (N, K, 2), score (N, K), index (N, K) int32, count (N,) int32."""
    dt = hm.dtype
    N, H, W = hm.shape
    h = torch.where(torch.isnan(hm), torch.full_like(hm, NEG), hm)                      # NaN counts as -inf
    pad = torch.full((N, H + 2 * rn, W + 2 * rn), NEG, dtype=dt)                         # outside the map: -inf
    pad[:, rn:rn + H, rn:rn + W] = h
    peak = torch.isfinite(h) & (h > min_score)
    for dy in range(-rn, rn + 1):
        for dx in range(-rn, rn + 1):
            if dy == 0 and dx == 0:
                continue
            nb = pad[:, rn + dy:rn + dy + H, rn + dx:rn + dx + W]
            peak &= (h > nb) if (dy < 0 or (dy == 0 and dx < 0)) else (h >= nb)        # earlier flat index: strictly; later: or equal
    flat = torch.where(peak, h, torch.full_like(h, NEG)).view(N, H * W)
    order = torch.sort(flat, dim=1, descending=True, stable=True)[1]                     # equal values keep the smaller flat index first
    if H * W < K:
        order = torch.cat((order, torch.zeros(N, K - H * W, dtype=order.dtype)), 1)
        kept = torch.cat((peak.view(N, -1).gather(1, order[:, :H * W]), torch.zeros(N, K - H * W, dtype=torch.bool)), 1)
    else:
        order = order[:, :K]
        kept = peak.view(N, -1).gather(1, order)
    m = h.view(N, -1).gather(1, order)
    rm, cm = torch.div(order, W, rounding_mode="floor"), order % W
    s = torch.zeros(N, K, dtype=dt)
    sx, sy = torch.zeros(N, K, dtype=dt), torch.zeros(N, K, dtype=dt)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            y, x = rm + dy, cm + dx
            inside = (y >= 0) & (y < H) & (x >= 0) & (x < W)
            hp = h.view(N, -1).gather(1, (y.clamp(0, H - 1) * W + x.clamp(0, W - 1)))
            use = inside & torch.isfinite(hp) & kept
            e = torch.where(use, torch.exp(beta * (torch.where(use, hp, m) - m)), torch.zeros_like(m))
            s, sx, sy = s + e, sx + e * dx, sy + e * dy
    one = torch.ones_like(s)
    zero = torch.zeros_like(s)
    x = torch.where(kept, cm.to(dt) + sx / torch.where(kept, s, one), zero)
    y = torch.where(kept, rm.to(dt) + sy / torch.where(kept, s, one), zero)
    score = torch.where(kept, m, zero)
    index = torch.where(kept, order, torch.full_like(order, -1)).to(torch.int32)
    return torch.stack((x, y), -1), score, index, kept.sum(1).to(torch.int32)


# --------------------------------------------------------------------------- consensus

def view_pairs(V):
    return [(a, b) for a in range(V) for b in range(a + 1, V)]


def candidates_exist(cand, cscore, cindex):
    return (cindex >= 0) & torch.isfinite(cscore) & (cscore > 0) & torch.isfinite(cand).all(-1)


def consensus_statement(cand, cscore, cindex, rec, ctm, sx, sy, tau, min_views, min_det_ratio=FS.MIN_DET):
    """cand (B, V, J, K, 2), cscore (B, V, J, K) in their own dtype, cindex (B, V, J, K) -> dict: choice (B, V, J), sel_coords, sel_conf,
    score (B, J), inliers, hyp, and per hypothesis h: all_score (B, J, NH), all_ok (B, J, NH) = qualifies, all_choice (B, J, NH, V)."""
    dt = cand.dtype
    B, V, J, K, _ = cand.shape
    exists = candidates_exist(cand, cscore, cindex)
    zero = torch.zeros_like(cscore)
    w = torch.where(exists, cscore, zero)
    xy = torch.where(exists.unsqueeze(-1), cand, torch.zeros_like(cand))
    ctm_d = None if ctm is None else ctm.to(dt)
    scores, oks, choices = [], [], []
    for a, b in view_pairs(V):
        rec2 = rec[[a, b]]
        ctm2 = None if ctm is None else ctm[:, [a, b]]
        for ka in range(K):
            for kb in range(K):
                c2 = torch.stack((xy[:, a, :, ka], xy[:, b, :, kb]), 1)
                w2 = torch.stack((w[:, a, :, ka], w[:, b, :, kb]), 1)
                p, _, _, ok = FS.statement(c2, w2, rec2, ctm2, sx, sy, thr=0.0, min_det_ratio=min_det_ratio)
                proj = FS.project(p, rec, ctm_d, sx, sy)                                    # (B, V, J, 2)
                e2 = ((proj.unsqueeze(3) - xy) ** 2).sum(-1)                               # (B, V, J, K)
                keep = 1.0 - e2 / (tau * tau)
                term = torch.where(exists & (keep > 0), w * keep, zero)                    # (a NaN fails the comparison)
                best = torch.zeros(B, V, J, dtype=dt)
                bk = torch.full((B, V, J), -1, dtype=torch.int64)
                for k in range(K):                                                          # ties go to the smaller k
                    better = term[..., k] > best
                    best = torch.where(better, term[..., k], best)
                    bk = torch.where(better, torch.full_like(bk, k), bk)
                scores.append(best.sum(1))
                oks.append(ok & ((bk >= 0).sum(1) >= min_views))
                choices.append(bk.permute(0, 2, 1))
    all_score, all_ok, all_choice = torch.stack(scores, -1), torch.stack(oks, -1), torch.stack(choices, 2)
    NH = all_score.shape[-1]
    win = torch.full((B, J), -1.0, dtype=dt)
    hyp = torch.full((B, J), -1, dtype=torch.int64)
    for h in range(NH):                                                                     # ties go to the smaller h
        better = all_ok[..., h] & (all_score[..., h] > win)
        win = torch.where(better, all_score[..., h], win)
        hyp = torch.where(better, torch.full_like(hyp, h), hyp)
    none = hyp < 0
    choice = all_choice.gather(2, hyp.clamp(min=0).view(B, J, 1, 1).expand(B, J, 1, V)).squeeze(2)      # (B, J, V)
    choice = torch.where(none.unsqueeze(-1), torch.full_like(choice, -1), choice).permute(0, 2, 1).contiguous()
    sel_coords, sel_conf = gather_choice(cand, cscore, choice)
    return {"choice": choice.to(torch.int32), "sel_coords": sel_coords, "sel_conf": sel_conf,
            "score": torch.where(none, torch.zeros_like(win), win), "inliers": (choice >= 0).sum(1).to(torch.int32),
            "hyp": hyp.to(torch.int32), "all_score": all_score, "all_ok": all_ok, "all_choice": all_choice}


def gather_choice(cand, cscore, choice):
    """The chosen candidates, copied: (B, V, J, 2) and (B, V, J); 0 where choice is -1."""
    k = choice.long().clamp(min=0)
    picked = choice >= 0
    coords = cand.gather(3, k.view(k.shape + (1, 1)).expand(k.shape + (1, 2))).squeeze(3)
    conf = cscore.gather(3, k.unsqueeze(-1)).squeeze(3)
    return torch.where(picked.unsqueeze(-1), coords, torch.zeros_like(coords)), torch.where(picked, conf, torch.zeros_like(conf))


def decided(ref, rel=1e-6):
    """(B, J) bool: the winning score leads the best qualifying hypothesis with a different choice by more than `rel`, relative (a
    pair without any qualifying hypothesis has no rival and counts as decided)."""
    B, J, NH, V = ref["all_choice"].shape
    win_choice = ref["choice"].long().permute(0, 2, 1).unsqueeze(2)                         # (B, J, 1, V)
    differs = (ref["all_choice"] != win_choice).any(-1) & ref["all_ok"]
    rival = torch.where(differs, ref["all_score"], torch.full_like(ref["all_score"], NEG)).max(-1)[0]
    return (ref["hyp"] < 0) | (ref["score"] - rival > rel * ref["score"])


# --------------------------------------------------------------------------- the distractor scene

def distractor_scene(B, views=(0, 1, 2, 3), seed=77, J=15, distract=1, height=1.2):
    """Sigma-1 bumps on 64 x 64 maps at the syn rig's projections of random points (test_gpu_triangulate.py's bump_maps scene: seed 77,
    15 joints a frame), plus, in `distract` different views per joint, one extra bump of `height` at a random spot more than 10 px from
    the true one.  -> dict: cams, rec, pts (B, J, 3) float64, hm (B, V, J, 64, 64) float32, centre (B, V, J, 2), which (B, J, distract)."""
    g = torch.Generator().manual_seed(seed)
    cams = [FS.rig()[v] for v in views]
    rec = FS.records(cams)
    V = len(views)
    pts = FS.random_points(B, J, g)
    centre = FS.project(pts, rec, None) * HM
    assert bool(((centre > 0) & (centre < HM - 1)).all()), "a projection left the image"
    hm = FS.bumps(pts, rec, None, HM, HM)
    g2 = torch.Generator().manual_seed(seed + 1)
    which = torch.stack([torch.randperm(V, generator=g2)[:distract] for _ in range(B * J)]).view(B, J, distract)
    for b in range(B):
        for j in range(J):
            for v in which[b, j].tolist():
                while True:
                    spot = torch.rand(2, generator=g2, dtype=torch.float64) * (HM - 5) + 2
                    if float((spot - centre[b, v, j]).norm()) > 10.0:
                        break
                hm[b, v, j] += height * FS.render(spot[0], spot[1], HM, HM)
    return {"cams": cams, "rec": rec, "pts": pts, "hm": hm.float().contiguous(), "centre": centre, "which": which}


def robust_chain(hm, rec, ctm=None, K=3, rn=1, r=2, beta=100.0, thr=0.5, tau=2.0, min_views=2):
    """The statements chained as decode_joints_3d_robust chains the launches, in hm's dtype: (pose (B, J, 3), ok (B, J), consensus dict,
    peaks tuple)."""
    B, V, J, H, W = hm.shape
    coords, score, index, count = peaks_statement(hm.reshape(-1, H, W), K, rn, r, beta, thr)
    cand, cscore, cindex = coords.view(B, V, J, K, 2), score.view(B, V, J, K), index.view(B, V, J, K)
    con = consensus_statement(cand, cscore, cindex, rec, ctm, 1.0 / W, 1.0 / H, tau, min_views)
    pose, _, _, ok = FS.statement(con["sel_coords"], con["sel_conf"], rec, ctm, 1.0 / W, 1.0 / H, thr)
    return pose, ok, con, (cand, cscore, cindex, count.view(B, V, J))


def top1_chain(hm, rec, ctm=None, beta=100.0, thr=0.5):
    """What decode_joints_3d does, as statements: the whole-map soft-argmax, then the triangulation of every view."""
    H, W = hm.shape[-2:]
    c, m = FS.soft_argmax_statement(hm, beta)
    pose, _, _, ok = FS.statement(c, m, rec, ctm, 1.0 / W, 1.0 / H, thr)
    return pose, ok

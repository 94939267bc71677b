"""The float64 statements of the information-weighted clip smoother (egr_joint_info_f32 / egr_info_track_f32) and the
scenes it is tested on.  Not a test module: test_info_track_host.py, test_gpu_info_track.py and tools/info_track_bench.py import it.
It builds on fisheye_statement (the projection, the extrinsics, the triangulation), trajectory_statement (the penalty, the validity
rule, the moving skeleton) and ray_track_statement (the dense block matrix and the block-banded loop) as they stand.

  information     W = sum_v conf_v J_v^T J_v of a point under the views that see it: J_v by AUTOGRAD through FS.project (elementwise
                  torch, Horner) - independent of the kernel's analytic derivation - the inclusion rule, sigma and valid from the
                  closed-form 3 x 3 inverse FS.statement uses, in the dtype of the points.
  fit             the smoother: per track the DENSE 3T x 3T matrix blockdiag(s_t W_t) + penalty (x) I_3, torch.linalg.solve (one track
                  a call) for the displacement from the observations, the gaps about the mean of a first solution, the IRLS loop of the Huber form in pixels, the energy, the validity, in
                  the dtype it is asked for (float64: the statement; float32: the evaluation that sets the yardstick's allowance).  The
                  solvability flags are always decided in float64, by RS.banded.
  scene           the cases of CASES on a moving skeleton seen by the rig."""
import torch

import fisheye_statement as FS
import ray_track_statement as RS
import trajectory_statement as TS

CASES = ("dense", "gaps", "oneview", "glitch")
MIN_PIVOT = 1e-10
ORDER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))                     # the six entries of a symmetric matrix, as the kernels lay them out


# --------------------------------------------------------------------------- the information matrix

def jacobians(points, enter, rec, ctm, sx, sy):
    """points (B, J, 3) in their own dtype, enter (B, V, J) -> d FS.project / d point, (B, V, J, 2, 3), by autograd: one view at a time,
    one backward pass per coordinate - an output of joint (b, j) depends on that joint's point alone, so the gradient of the sum is the
    Jacobian's row.  Where a view does not enter the point is replaced by a harmless one before it is projected (the derivative of
    sqrt at an on-axis point would put a NaN into the joint's other views); those rows are selected away by the caller."""
    V = rec.shape[0]
    harmless = torch.tensor([1.0, 2.0, 100.0], dtype=points.dtype)
    views = []
    for v in range(V):
        p = torch.where(enter[:, v].unsqueeze(-1), points.detach(), harmless).requires_grad_()
        out = FS.project(p, rec[v:v + 1], None if ctm is None else ctm[:, v:v + 1].to(p.dtype), sx, sy)        # (B, 1, J, 2)
        views.append(torch.stack([torch.autograd.grad(out[:, 0, :, c].sum(), p, retain_graph=True)[0] for c in range(2)], -2))
    return torch.stack(views, 1)


def enters(points, conf, rec, ctm, thr=FS.THR):
    """(B, V, J) bool: the view's confidence passes FS.rays' rule, the point is finite and gives a pixel off the optical axis."""
    dt = points.dtype
    R, t = FS.extrinsics(rec, None if ctm is None else ctm.to(dt), dt)
    p = points.unsqueeze(1)
    q = [sum(R[r][k] * p[..., k] for k in range(3)) + t[r] for r in range(3)]
    n = torch.sqrt(q[0] * q[0] + q[1] * q[1])
    finite = torch.isfinite(points).all(-1).unsqueeze(1) & torch.isfinite(q[0]) & torch.isfinite(q[1]) & torch.isfinite(q[2])
    return (conf >= thr) & (conf > 0) & torch.isfinite(conf) & finite & (n > 0)


def six(M):
    """(..., 3, 3) -> (..., 6) in ORDER."""
    return torch.stack([M[..., k, l] for k, l in ORDER], -1)


def full(s):
    """(..., 6) -> (..., 3, 3) symmetric."""
    at = {kl: i for i, kl in enumerate(ORDER)}
    return torch.stack([torch.stack([s[..., at[min(k, l), max(k, l)]] for l in range(3)], -1) for k in range(3)], -2)


def information(points, conf, rec, ctm, sx, sy, thr=FS.THR, min_det_ratio=FS.MIN_DET):
    """points (B, J, 3) cm, conf (B, V, J) in the dtype of the points, rec (V, 30), ctm (B, V, 4, 4) | None -> dict(info (B, J, 6), views
    (B, J) uint8, sigma (B, J), valid (B, J) bool).  An excluded view is selected away, never multiplied."""
    dt = points.dtype
    conf = conf.to(dt)
    enter = enters(points, conf, rec, ctm, thr)
    Jv = jacobians(points, enter, rec, ctm, sx, sy)
    Jv = torch.where(enter[..., None, None], Jv, torch.zeros_like(Jv))
    w = torch.where(enter, conf, torch.zeros_like(conf))
    W = (w[..., None, None] * (Jv.transpose(-1, -2) @ Jv)).sum(1)                       # (B, J, 3, 3)
    a00, a01, a02, a11, a12, a22 = (W[..., k, l] for k, l in ORDER)
    c00, c11, c22 = a11 * a22 - a12 * a12, a00 * a22 - a02 * a02, a00 * a11 - a01 * a01
    c01, c02 = a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    det = a00 * c00 + a01 * c01 + a02 * c02
    tr3 = (a00 + a11 + a22) / 3
    ok = (enter.sum(1) >= 1) & (a00 > 0) & (c22 > 0) & (det > 0) & (det > min_det_ratio * tr3 * tr3 * tr3)
    ds = torch.where(ok, det, torch.ones_like(det))
    sigma = torch.where(ok, torch.sqrt((c00 + c11 + c22) / ds), torch.zeros_like(det))
    return {"info": six(W), "views": enter.sum(1).to(torch.uint8), "sigma": sigma, "valid": ok}


# --------------------------------------------------------------------------- the smoother

def used_frames(pose, info, obs):
    """(N, T, J) bool: observed, pose and the six entries finite, every diagonal entry >= 0, the trace > 0."""
    on = torch.isfinite(pose).all(-1) & torch.isfinite(info).all(-1)
    on = on & (info[..., 0] >= 0) & (info[..., 3] >= 0) & (info[..., 5] >= 0) & (info[..., 0] + info[..., 3] + info[..., 5] > 0)
    return on if obs is None else on & (obs != 0)


def operands(pose, info, obs, dt):
    """-> used (N, T, J) bool, z (N, J, T, 3) and W (N, J, T, 3, 3) in dtype dt, zeros where the frame is not used."""
    used = used_frames(pose, info, obs)
    z = torch.where(used.unsqueeze(-1), pose, torch.zeros_like(pose)).to(dt)
    W = full(torch.where(used.unsqueeze(-1), info, torch.zeros_like(info)).to(dt))
    return used, z.permute(0, 2, 1, 3), W.permute(0, 2, 1, 3, 4)


def enough_frames(used, lv):
    """Rule (a), (N, J) bool."""
    T = used.shape[1]
    seen = used.sum(1)
    if lv > 0:
        return seen >= 1
    return seen >= 2 if T >= 3 else seen == T


def solvable(used, W, z, lv, la, min_pivot_ratio=MIN_PIVOT):
    """(N, J) bool: rule (a) and rule (b) - every scalar pivot of RS.banded on the plain problem above min_pivot_ratio x the largest
    diagonal entry - decided in float64."""
    W, z = W.double(), z.double()
    _, low, top = RS.banded(W, (W @ z.unsqueeze(-1)).squeeze(-1), lv, la)
    return enough_frames(used, lv) & (low > min_pivot_ratio * top)


def displacement(W, x, z):
    """sqrt((x - z)^T W (x - z)), (N, J, T): the displacement in coordinate units; 0 where rounding leaves the form negative."""
    d = (x - z).unsqueeze(-1)
    r2 = (d.transpose(-1, -2) @ W @ d).squeeze(-1).squeeze(-1)
    return torch.sqrt(torch.clamp(r2, min=0.0))


def solve(W, z, on, ok, lv, la, fill):
    """x (N, J, T, 3) of (blockdiag(W_t) + P) x = (W_t z_t), P = penalty (x) I, solved for the displacement d = x - z~ from z~_t = z_t at
    a used frame (`on` (N, J, T)) and `fill` (N, J, 3) in a gap: (blockdiag(W) + P) d = -P z~, since W_t = 0 in a gap.  The unknowns
    are then the size of the noise, and a frame that no penalty couples to its neighbours comes back exactly."""
    N, J, T = W.shape[:3]
    zt = torch.where(on.unsqueeze(-1), z, fill.unsqueeze(2).expand_as(z))
    P = TS.penalty(T, lv, la, W.dtype)
    rhs = -(P @ zt)                                                                     # (T, T) @ (N, J, T, 3)
    A = RS.dense_matrix(W, ok, lv, la)
    return zt + TS.solve_tracks(A, rhs.reshape(N, J, 3 * T, 1)).view(N, J, T, 3)


def fit(pose, info, obs, lv=0.0, la=1.0, huber=0.0, reweights=0, max_gap=8, min_pivot_ratio=MIN_PIVOT, dt=torch.float64):
    """The statement in dtype `dt` on the given (fp32) operands -> dict(pose (N, T, J, 3), valid (N, T, J) bool, residual, weight
    (N, T, J), energy (N, J), ok (N, J) bool, cond: the largest condition number over the solvable tracks).  Every solve is made twice:
    with the gaps' unknowns about the device origin, then about the mean of that solution, where they are the track's extent and not
    its distance from the device (a solve's rounding error is eps |A| |unknowns| / lambda_min)."""
    used, z, W = operands(pose, info, obs, dt)
    N, J, T = W.shape[:3]
    ok = solvable(used, W, z, lv, la, min_pivot_ratio)
    live = ok.unsqueeze(-1)
    on = used.permute(0, 2, 1)                                                          # (N, J, T)
    s = on.to(dt)
    for k in range(reweights + 1):
        Ws = s[..., None, None] * W
        first = solve(Ws, z, on, ok, lv, la, torch.zeros(N, J, 3, dtype=dt))
        x = solve(Ws, z, on, ok, lv, la, first.mean(2))
        if k < reweights:
            r = displacement(W, x, z)
            s = torch.where(on, torch.where(r > huber, huber / torch.where(r > huber, r, torch.ones_like(r)), torch.ones_like(r)), torch.zeros_like(r))
    x = torch.where(live.unsqueeze(-1), x, torch.zeros_like(x))
    r = torch.where(on & live, displacement(W, x, z), torch.zeros_like(s))
    rho = r * r if huber <= 0 else torch.where(r > huber, 2.0 * huber * r - huber * huber, r * r)
    E = rho.sum(2)
    if T >= 2:
        E = E + lv * ((x[:, :, 1:] - x[:, :, :-1]) ** 2).sum((2, 3))
    if T >= 3:
        E = E + la * ((x[:, :, 2:] - 2.0 * x[:, :, 1:-1] + x[:, :, :-2]) ** 2).sum((2, 3))
    cond = 1.0
    if dt == torch.float64 and bool(ok.any()):
        cond = max(float(torch.linalg.cond(a)) for a in RS.dense_matrix(W, ok, lv, la)[ok])
    return {"pose": x.permute(0, 2, 1, 3), "valid": TS.validity(used.to(torch.float64), ok, max_gap), "residual": r.permute(0, 2, 1),
            "weight": torch.where(on & live, s, torch.zeros_like(s)).permute(0, 2, 1), "energy": torch.where(ok, E, torch.zeros_like(E)),
            "ok": ok, "cond": cond}


def try_fit(*args, **kw):
    """`fit`, or None where the evaluation does not factor or is not finite (float32 on an ill-conditioned clip)."""
    try:
        out = fit(*args, **kw)
    except RuntimeError:
        return None
    return out if all(bool(torch.isfinite(out[k]).all()) for k in ("pose", "residual", "weight", "energy")) else None


def banded_fit(pose, info, obs, lv, la):
    """The plain problem by RS.banded - the Python restatement of the kernels' block elimination - in float64, about the mean of the
    used observations -> x (N, T, J, 3), smallest pivot (N, J), largest diagonal entry (N, J)."""
    used, z, W = operands(pose, info, obs, torch.float64)
    on = used.permute(0, 2, 1).unsqueeze(-1).double()
    c = ((z * on).sum(2) / on.sum(2).clamp(min=1.0)).unsqueeze(2)
    x, low, top = RS.banded(W, (W @ (z - c).unsqueeze(-1)).squeeze(-1), lv, la)
    return x + c.permute(0, 2, 1, 3), low, top


# --------------------------------------------------------------------------- scenes

def scene(N, T, V, J, case, rw=False, seed=0, noise=0.1):
    """dict(pose (N, T, J, 3) fp32 cm: the per-frame triangulation of noisy projections (`noise` heat-map pixels) of a moving skeleton,
    info (N, T, J, 6) fp32: the information matrices at the truth under the views that see the frame, obs (N, T, J) uint8 | None,
    conf (N, T, V, J), rec, ctm (N, T, V, 4, 4) | None, sx, sy, truth float64) of one case:
      dense    every view, every frame;
      gaps     unobserved frames (a long run where T > 20, every fifth track unobserved throughout) with NaN, infinities and garbage
               planted in their poses and matrices, and frames that are observed but carry a NaN, a negative diagonal or a zero matrix;
      oneview  every other frame of a track keeps one view: a rank-2 matrix and a point somewhere on that view's ray, alternating with
               whole frames so that cond(A) stays where 1e-6 cm is resolvable (the note in test_ray_track_host.py);
      glitch   three single frames a track displaced by 25 to 50 cm, listed in `glitches` as (n, t, j)."""
    assert case in CASES, case
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + 13 * T + 31 * J + 101 * V + CASES.index(case) + (500 if rw else 0))
    cams = FS.rig("ego4view_rw" if rw else "ego4view_syn")[:V]
    rec = FS.records(cams)
    truth = TS.motion(N, T, J, g)
    ctm = FS.random_ctm(N * T, V, cams, g) if rw else None
    c64 = None if ctm is None else ctm.double()
    sx = sy = 1.0 / FS.HM
    flat = truth.view(N * T, J, 3)
    coords = FS.project(flat, rec, c64, sx, sy) + noise * torch.randn(N * T, V, J, 2, generator=g, dtype=torch.float64)
    conf = (0.6 + 0.4 * torch.rand(N, T, V, J, generator=g)).float()
    if case == "oneview":
        keep = torch.randint(0, V, (N, T, 1, J), generator=g) == torch.arange(V).view(1, 1, V, 1)
        n_, t_, j_ = torch.arange(N).view(N, 1, 1, 1), torch.arange(T).view(1, T, 1, 1), torch.arange(J).view(1, 1, 1, J)
        single = ((n_ + t_ + j_) % 2 == 1).expand(N, T, V, J)
        conf = torch.where(single & ~keep, torch.zeros_like(conf), conf)
    cf = conf.view(N * T, V, J)
    tri, _, _, ok = FS.statement(coords, cf.double(), rec, c64, sx, sy)
    wander = flat + 0.5 * torch.randn(N * T, J, 3, generator=g, dtype=torch.float64)     # where one view fixes no point: anywhere near
    pose = torch.where(ok.unsqueeze(-1), tri, wander).float().view(N, T, J, 3)
    info = information(flat, cf.double(), rec, c64, sx, sy)["info"].float().view(N, T, J, 6)
    obs, glitches = None, []
    if case == "oneview":
        obs = torch.ones(N, T, J, dtype=torch.uint8)
    elif case == "gaps":
        drop = torch.rand(N, T, J, generator=g) < 0.3
        if T > 20:
            start = int(torch.randint(2, T - 14, (1,), generator=g))
            drop[:, start:start + 12, ::2] = True
        for n in range(N):
            for j in range(J):
                if (n + j) % 5 == 4:
                    drop[n, :, j] = True
        obs = (~drop).to(torch.uint8)
        bad = torch.tensor([float("nan"), float("inf"), float("-inf"), 3.0e38, -1.0e30])
        pose[drop] = bad[torch.randint(0, 5, pose.shape, generator=g)][drop]
        info[drop] = bad[torch.randint(0, 5, info.shape, generator=g)][drop]
        spoil = (torch.rand(N, T, J, generator=g) < 0.1) & ~drop                        # observed, and still not a frame
        for n, t, j in spoil.nonzero().tolist():
            kind = (n + t + j) % 4
            if kind == 0:
                pose[n, t, j, (t + j) % 3] = float("nan")
            elif kind == 1:
                info[n, t, j, (0, 3, 5)[(t + j) % 3]] = -1.0
            elif kind == 2:
                info[n, t, j] = 0.0
            else:
                info[n, t, j, (t + j) % 6] = float("inf")
    elif case == "glitch":
        for n in range(N):
            for j in range(J):
                for t in torch.randperm(T, generator=g)[:3].tolist():
                    d = torch.randn(3, generator=g)
                    pose[n, t, j] += d / d.norm() * (25.0 + 25.0 * float(torch.rand(1, generator=g)))
                    glitches.append((n, t, j))
    return {"pose": pose.contiguous(), "info": info.contiguous(), "obs": obs, "conf": conf.contiguous(), "rec": rec,
            "ctm": None if ctm is None else ctm.view(N, T, V, 4, 4), "sx": sx, "sy": sy, "truth": truth, "cams": cams, "glitches": glitches}

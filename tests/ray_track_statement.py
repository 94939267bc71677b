"""The float64 statement of the ray-space clip smoother (egr_ray_track_f32) and the scenes it is tested on.  Not a test
module: test_ray_track_host.py, test_gpu_ray_track.py and tools/ray_track_bench.py import it.  It builds on fisheye_statement (the rays,
their normal equations and distances) and trajectory_statement (the penalty, the validity rule, the moving skeleton) as they stand.

A track is one joint j of one clip n: T frames, V rays a frame with weights w_tv = conf where the view is used (FS.rays' rule), else 0.
Its positions minimise
    E(x) = sum_t sum_v w_tv rho(dist_tv(x_t)) + lv sum |x_{t+1} - x_t|^2 + la sum |x_{t+1} - 2 x_t + x_{t-1}|^2.

  fit             the statement: per track the DENSE 3T x 3T matrix blockdiag(G_t) + penalty (x) I_3 from FS.normal_equations and
                  TS.penalty, torch.linalg.solve (one track a call), the IRLS loop of the Huber form, the energy, the validity, in the
                  dtype it is asked for (float64: the statement; float32: the evaluation that sets the yardstick's allowance).  The
                  solvability flags are always decided in float64, by `banded`.
  banded          the block LDL^T along t as a Python loop, every pivot by the 3 x 3 LDL^T of the triangulation: x, the smallest scalar
                  pivot and the largest diagonal entry of every track.  Rule (b) of the solvability is written here, once.
  scene           the cases of CASES on a moving skeleton seen by the rig."""
import torch

import fisheye_statement as FS
import trajectory_statement as TS

CASES = ("dense", "oneview", "gaps", "glitch")
MIN_PIVOT = 1e-10


# --------------------------------------------------------------------------- the rays of a clip

def clip_rays(coords, conf, rec, ctm, sx, sy, thr=FS.THR):
    """coords (N, T, V, J, 2), conf (N, T, V, J) in their own dtype, ctm (N, T, V, 4, 4) | None -> use (B, V, J) bool, w (B, V, J), d[3],
    R[3][3], t[3] of the B = N T frames, as FS.rays gives them."""
    N, T, V, J = conf.shape
    flat = None if ctm is None else ctm.reshape(N * T, V, 4, 4)
    return FS.rays(coords.reshape(N * T, V, J, 2), conf.reshape(N * T, V, J), rec, flat, sx, sy, thr)


def blocks(wr, d, R, t, N, T):
    """Per-ray weights wr (B, V, J) -> G (N, J, T, 3, 3) and g (N, J, T, 3): every frame's normal equations."""
    A, b = FS.normal_equations(wr, d, R, t)
    J = wr.shape[-1]
    G = torch.stack([torch.stack([A[min(k, l), max(k, l)] for l in range(3)], -1) for k in range(3)], -2)       # (B, J, 3, 3)
    return G.view(N, T, J, 3, 3).permute(0, 2, 1, 3, 4), torch.stack(b, -1).view(N, T, J, 3).permute(0, 2, 1, 3)


def distances(d, R, t, x):
    """x (N, T, J, 3) -> the ray distances (B, V, J)."""
    flat = x.reshape(-1, x.shape[2], 3)
    return torch.sqrt(FS.ray_dist2(d, R, t, lambda k: flat[..., k]))


def enough_rays(use, N, T, lv):
    """Rule (a), (N, J) bool, from the used rays (B, V, J)."""
    count = use.sum(1).view(N, T, -1)                                                  # (N, T, J)
    if lv > 0:
        return count.sum(1) >= 2
    if T >= 3:
        return (count.sum(1) >= 3) & ((count > 0).sum(1) >= 2)
    return (count >= 2).all(1)


# --------------------------------------------------------------------------- the block-banded elimination, as a loop

def ldl3(D):
    """D (..., 3, 3) symmetric -> (d1, d2, d3, l21, l31, l32) by the LDL^T of the triangulation (no pivoting)."""
    a00, a01, a02, a11, a12, a22 = D[..., 0, 0], D[..., 0, 1], D[..., 0, 2], D[..., 1, 1], D[..., 1, 2], D[..., 2, 2]
    d1 = a00
    l21, l31 = a01 / d1, a02 / d1
    d2 = a11 - l21 * a01
    l32 = (a12 - l31 * a01) / d2
    d3 = a22 - l31 * a02 - l32 * l32 * d2
    return d1, d2, d3, l21, l31, l32


def ldl3_solve(f, rhs):
    """rhs (..., 3, m) -> D^-1 rhs."""
    d1, d2, d3, l21, l31, l32 = (v.unsqueeze(-1) for v in f)
    y1 = rhs[..., 0, :]
    y2 = rhs[..., 1, :] - l21 * y1
    y3 = rhs[..., 2, :] - l31 * y1 - l32 * y2
    x3 = y3 / d3
    x2 = y2 / d2 - l32 * x3
    x1 = y1 / d1 - l21 * x2 - l31 * x3
    return torch.stack((x1, x2, x3), -2)


def banded(G, g, lv, la):
    """G (N, J, T, 3, 3), g (N, J, T, 3) float64 -> x (N, T, J, 3), the smallest scalar pivot (N, J) and the largest diagonal entry
    (N, J) of every track: D_t = G_t + a_t I - E_{t-1} D_{t-1} E_{t-1}^T - F_{t-2} D_{t-2} F_{t-2}^T, E_t = (b_t I - c_{t-1} E_{t-1}^T)
    D_t^-1, F_t = c_t D_t^-1, then the two substitutions.  Every track is eliminated (one that is not solvable may divide by zero:
    mask it afterwards)."""
    G, g = G.double(), g.double()
    N, J, T = G.shape[:3]
    a, b, c = TS.band(T, lv, la)
    eye = torch.eye(3, dtype=torch.float64).expand(N, J, 3, 3)
    D, Di, E, y = [], [], [], []
    low = torch.full((N, J), float("inf"), dtype=torch.float64)
    top = torch.zeros(N, J, dtype=torch.float64)
    nan = torch.zeros(N, J, dtype=torch.bool)
    for t in range(T):
        Dt = G[:, :, t] + a[t] * eye
        yt = g[:, :, t].unsqueeze(-1)
        Mt = b[t] * eye
        if t >= 1:
            Dt = Dt - E[t - 1] @ D[t - 1] @ E[t - 1].transpose(-1, -2)
            yt = yt - E[t - 1] @ y[t - 1]
            Mt = Mt - c[t - 1] * E[t - 1].transpose(-1, -2)
        if t >= 2:
            Dt = Dt - c[t - 2] * c[t - 2] * Di[t - 2]
            yt = yt - c[t - 2] * (Di[t - 2] @ y[t - 2])
        Dt = 0.5 * (Dt + Dt.transpose(-1, -2))
        f = ldl3(Dt)
        piv = torch.stack(f[:3], -1)
        nan = nan | torch.isnan(piv).any(-1)
        low = torch.minimum(low, torch.nan_to_num(piv, nan=float("inf")).amin(-1))
        top = torch.maximum(top, torch.diagonal(G[:, :, t], dim1=-2, dim2=-1).amax(-1) + a[t])
        inv = ldl3_solve(f, eye)
        D.append(Dt)
        Di.append(inv)
        E.append(Mt @ inv)
        y.append(yt)
    x = [None] * T
    for t in range(T - 1, -1, -1):
        xt = Di[t] @ y[t]
        if t + 1 < T:
            xt = xt - E[t].transpose(-1, -2) @ x[t + 1]
        if t + 2 < T:
            xt = xt - c[t] * (Di[t] @ x[t + 2])
        x[t] = xt
    low = torch.where(nan, torch.full_like(low, float("-inf")), low)
    return torch.stack(x, 2).squeeze(-1).permute(0, 2, 1, 3), low, top


def centred(R, t, centre, T):
    """The translations of the problem in u = x - centre, centre (N, J, 3) a point a track: R (c + u) + t = R u + (R c + t)."""
    c = centre.repeat_interleave(T, 0).unsqueeze(1)                                    # (B, 1, J, 3)
    return [t[r] + sum(R[r][k] * c[..., k] for k in range(3)) for r in range(3)]


def banded_fit(coords, conf, rec, ctm, sx, sy, thr=FS.THR, lv=0.0, la=10.0, centre=None):
    """`banded` on the plain problem of a clip's operands, in float64, solved about `centre` (N, J, 3) like `fit` where it is given
    -> x (N, T, J, 3), smallest pivot (N, J), largest diagonal entry (N, J)."""
    N, T, V, J = conf.shape
    _, w, d, R, t = clip_rays(coords.double(), conf.double(), rec, None if ctm is None else ctm.double(), sx, sy, thr)
    if centre is not None:
        t = centred(R, t, centre.double(), T)
    x, low, top = banded(*blocks(w, d, R, t, N, T), lv, la)
    return (x if centre is None else x + centre.double().unsqueeze(1)), low, top


def solvable(use, G, g, N, T, lv, la, min_pivot_ratio=MIN_PIVOT):
    """(N, J) bool: rule (a) and rule (b) - every scalar pivot of `banded` above min_pivot_ratio x the largest diagonal entry."""
    _, low, top = banded(G, g, lv, la)
    return enough_rays(use, N, T, lv) & (low > min_pivot_ratio * top)


# --------------------------------------------------------------------------- the dense statement

def dense_matrix(G, ok, lv, la):
    """(N, J, 3T, 3T): blockdiag(G_t) + penalty (x) I_3 in G's dtype, unknowns ordered (t, coordinate); the identity for a dead track."""
    N, J, T = G.shape[:3]
    P = torch.kron(TS.penalty(T, lv, la, G.dtype), torch.eye(3, dtype=G.dtype))
    A = P.expand(N, J, 3 * T, 3 * T).clone()
    for t in range(T):
        A[:, :, 3 * t:3 * t + 3, 3 * t:3 * t + 3] += G[:, :, t]
    return torch.where(ok[..., None, None], A, torch.eye(3 * T, dtype=G.dtype).expand_as(A))


def energy(x, w, r, N, T, lv, la, huber):
    """(N, J): E at x (N, T, J, 3) with the base weights w and the ray distances r (B, V, J)."""
    rho = r * r if huber <= 0 else torch.where(r > huber, 2.0 * huber * r - huber * huber, r * r)
    E = (w * rho).sum(1).view(N, T, -1).sum(1)
    if T >= 2:
        E = E + lv * ((x[:, 1:] - x[:, :-1]) ** 2).sum((1, 3))
    if T >= 3:
        E = E + la * ((x[:, 2:] - 2.0 * x[:, 1:-1] + x[:, :-2]) ** 2).sum((1, 3))
    return E


def fit(coords, conf, rec, ctm, sx, sy, thr=FS.THR, lv=0.0, la=10.0, huber=0.0, reweights=0, max_gap=8, min_pivot_ratio=MIN_PIVOT,
        dt=torch.float64, centre=None):
    """The statement in dtype `dt` on the given (fp32) operands -> dict(pose (N, T, J, 3), valid (N, T, J) bool, residual, weight
    (N, T, V, J), rays (N, T, J) uint8, energy (N, J), ok (N, J) bool, cond: the largest condition number over the solvable tracks).
    With `centre` (N, J, 3) the same problem is solved in u = x - centre: the same minimiser, but a solve's rounding error is
    eps |A| |unknowns| / lambda_min, and |u| is the track's extent, not its distance from the device (|x| ~ 100 cm)."""
    N, T, V, J = conf.shape
    use, w64, d64, R64, t64 = clip_rays(coords.double(), conf.double(), rec, None if ctm is None else ctm.double(), sx, sy, thr)
    if centre is not None:
        t64 = centred(R64, t64, centre.double(), T)
    G64, g64 = blocks(w64, d64, R64, t64, N, T)
    ok = solvable(use, G64, g64, N, T, lv, la, min_pivot_ratio)
    if dt == torch.float64:
        w, d, R, t = w64, d64, R64, t64
    else:
        _, w, d, R, t = clip_rays(coords.to(dt), conf.to(dt), rec, None if ctm is None else ctm.to(dt), sx, sy, thr)
        if centre is not None:
            t = centred(R, t, centre.to(dt), T)
    s = torch.ones_like(w)
    for k in range(reweights + 1):
        used = w * s
        G, g = blocks(used, d, R, t, N, T)
        A = dense_matrix(G, ok, lv, la)
        x = TS.solve_tracks(A, g.reshape(N, J, 3 * T, 1)).view(N, J, T, 3).permute(0, 2, 1, 3)
        if k < reweights:
            r = distances(d, R, t, x)
            s = torch.where(r > huber, huber / torch.where(r > huber, r, torch.ones_like(r)), torch.ones_like(r))
    seen = use.sum(1).view(N, T, J)
    live = ok.view(N, 1, 1, J).expand(N, T, V, J).reshape(N * T, V, J)
    zero = torch.zeros_like(w)
    r = torch.where(use & live, distances(d, R, t, x), zero)
    if centre is not None:
        x = x + centre.to(dt).unsqueeze(1)
    x = torch.where(ok.view(N, 1, J, 1), x, torch.zeros_like(x))
    cond = 1.0
    if dt == torch.float64 and bool(ok.any()):
        cond = max(float(torch.linalg.cond(a)) for a in dense_matrix(G64, ok, lv, la)[ok])
    return {"pose": x, "valid": TS.validity(seen.to(torch.float64), ok, max_gap), "residual": r.view(N, T, V, J),
            "weight": torch.where(live, used, zero).view(N, T, V, J),
            "rays": torch.where(ok.view(N, 1, J), seen, torch.zeros_like(seen)).to(torch.uint8),
            "energy": torch.where(ok, energy(x, w, r, N, T, lv, la, huber), torch.zeros_like(w[:N, 0])), "ok": ok, "cond": cond}


def try_fit(*args, **kw):
    """`fit`, or None where the evaluation does not factor or is not finite (float32 on an ill-conditioned clip)."""
    try:
        out = fit(*args, **kw)
    except RuntimeError:
        return None
    return out if all(bool(torch.isfinite(out[k]).all()) for k in ("pose", "residual", "weight", "energy")) else None


# --------------------------------------------------------------------------- scenes

def scene(N, T, V, J, case, rw=False, seed=0, noise=0.1, glitch_px=(5.0, 10.0)):
    """dict(coords (N, T, V, J, 2) fp32 in pixels of an FS.HM map, conf (N, T, V, J) fp32, rec (V, 30), ctm (N, T, V, 4, 4) fp32 | None,
    sx, sy, truth float64 (N, T, J, 3)) of one case: `dense` every view; `oneview` every other frame of a track keeps one view (which one is random);
    `gaps` frames nobody sees, one view here and there, and every fifth track without a ray; `glitch` three single views a track off
    by `glitch_px` (5 to 10) heat-map pixels, listed in `glitches` as (n, t, v, j)."""
    assert case in CASES, case
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + 13 * T + 31 * J + 101 * V + CASES.index(case) + (500 if rw else 0))
    cams = FS.rig("ego4view_rw" if rw else "ego4view_syn")[:V]
    rec = FS.records(cams)
    truth = TS.motion(N, T, J, g)
    ctm = FS.random_ctm(N * T, V, cams, g) if rw else None
    sx = sy = 1.0 / FS.HM
    coords = FS.project(truth.view(N * T, J, 3), rec, None if ctm is None else ctm.double(), sx, sy).view(N, T, V, J, 2)
    coords = coords + noise * torch.randn(N, T, V, J, 2, generator=g, dtype=torch.float64)
    conf = (0.6 + 0.4 * torch.rand(N, T, V, J, generator=g)).float()
    low = (0.3 * torch.rand(N, T, V, J, generator=g)).float()                         # below the threshold, some of them 0
    low[torch.rand(N, T, V, J, generator=g) < 0.5] = 0.0
    keep = torch.randint(0, V, (N, T, 1, J), generator=g) == torch.arange(V).view(1, 1, V, 1)
    if case == "oneview":
        n_, t_, j_ = torch.arange(N).view(N, 1, 1, 1), torch.arange(T).view(1, T, 1, 1), torch.arange(J).view(1, 1, 1, J)
        single = ((n_ + t_ + j_) % 2 == 1).expand(N, T, V, J)                        # every other frame of a track, its neighbours whole
        conf = torch.where(single & ~keep, low, conf)
    elif case == "gaps":
        drop = torch.rand(N, T, 1, J, generator=g) < 0.3
        if T > 20:
            start = int(torch.randint(2, T - 14, (1,), generator=g))
            drop[:, start:start + 12, :, ::2] = True
        single = (torch.rand(N, T, 1, J, generator=g) < 0.2).expand(N, T, V, J)
        conf = torch.where(single & ~keep, low, conf)
        conf = torch.where(drop.expand(N, T, V, J), low, conf)
        for n in range(N):
            for j in range(J):
                if (n + j) % 5 == 4:
                    conf[n, :, :, j] = low[n, :, :, j]
    glitches = []
    if case == "glitch":
        for n in range(N):
            for j in range(J):
                for t in torch.randperm(T, generator=g)[:3].tolist():
                    v = int(torch.randint(0, V, (1,), generator=g))
                    e = torch.randn(2, generator=g, dtype=torch.float64)
                    coords[n, t, v, j] += e / e.norm() * (glitch_px[0] + (glitch_px[1] - glitch_px[0]) * float(torch.rand(1, generator=g)))
                    glitches.append((n, t, v, j))
    return {"coords": coords.float().contiguous(), "conf": conf.contiguous(), "rec": rec, "ctm": None if ctm is None else ctm.view(N, T, V, 4, 4),
            "sx": sx, "sy": sy, "truth": truth, "cams": cams, "glitches": glitches}

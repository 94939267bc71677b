"""The float64 statement of the temporal trajectory smoother (egr_trajectory_smooth_f32 / egr_trajectory_smooth_bwd_f32)
and the scenes it is tested on.  Not a test module: test_trajectory_host.py, test_gpu_trajectory.py and tools/trajectory_bench.py
import it.

A track is one joint of one clip: observations z_t (cm) for t = 0..T-1 with base weights
    w_t = weight_t [obs_t != 0] [z_t and weight_t finite, weight_t > 0],
and its smoothed positions minimise
    E(x) = sum_t w_t rho(|x_t - z_t|) + lv sum |x_{t+1} - x_t|^2 + la sum |x_{t+1} - 2 x_t + x_{t-1}|^2.

  smooth          the statement: a DENSE A = W + lv D1^T D1 + la D2^T D2 built from the difference matrices, torch.linalg.solve
                  (one track a call), the IRLS loop of the Huber form, the energies and the validity rule, in the dtype it is asked for (float64: the statement;
                  float32: the evaluation that sets the yardstick's allowance).  Differentiable in its plain form by autograd.
  banded          a second statement of another kind: the pentadiagonal LDL^T elimination along t as a Python loop.
  stationarity    at a given fp32 pose, g = A x - W z in float64 and the allowance sum_k |A_ik| ulp32(max |x| of the track).
  scene           the cases of CASES on a moving skeleton."""
import torch

import fisheye_statement as FS

CASES = ("dense", "gaps", "ends", "sparse", "nonfinite", "mask", "glitch")


# --------------------------------------------------------------------------- the matrices

def differences(T, dt=torch.float64):
    """D1 (T-1, T) and D2 (T-2, T): first and second differences along t (no rows where T is too short)."""
    D1, D2 = torch.zeros(max(T - 1, 0), T, dtype=dt), torch.zeros(max(T - 2, 0), T, dtype=dt)
    for i in range(T - 1):
        D1[i, i], D1[i, i + 1] = -1.0, 1.0
    for i in range(T - 2):
        D2[i, i], D2[i, i + 1], D2[i, i + 2] = 1.0, -2.0, 1.0
    return D1, D2


def penalty(T, lv, la, dt=torch.float64):
    D1, D2 = differences(T, dt)
    return lv * (D1.t() @ D1) + la * (D2.t() @ D2)


def base_weights(pose, weight, obs):
    """pose (N, T, J, 3), weight (N, T, J) | None, obs (N, T, J) | None -> w (N, T, J) and z (N, T, J, 3) in pose's dtype: a frame
    that is not observed has w = 0 and z = 0 - what was planted there is selected away, never multiplied."""
    on = torch.isfinite(pose).all(-1)
    if weight is not None:
        on = on & torch.isfinite(weight) & (weight > 0)
    if obs is not None:
        on = on & (obs != 0)
    wt = torch.ones_like(pose[..., 0]) if weight is None else weight.to(pose.dtype)
    return torch.where(on, wt, torch.zeros_like(wt)), torch.where(on.unsqueeze(-1), pose, torch.zeros_like(pose))


def solvable(w, lv):
    """(N, J) bool: A is positive definite, decided from the base weights."""
    T = w.shape[1]
    seen = (w > 0).sum(1)
    if lv > 0:
        return seen >= 1
    return seen >= 2 if T >= 3 else seen == T


def validity(w, ok, max_gap):
    """(N, T, J) bool: a frame of a solvable track whose distance to the nearest observed frame is <= max_gap."""
    N, T, J = w.shape
    far = 1 << 30
    seen = w > 0
    dist = torch.full((N, T, J), far, dtype=torch.int64)
    run = torch.full((N, J), far, dtype=torch.int64)
    for t in range(T):
        run = torch.where(seen[:, t], torch.zeros_like(run), (run + 1).clamp(max=far))
        dist[:, t] = run
    run = torch.full((N, J), far, dtype=torch.int64)
    for t in range(T - 1, -1, -1):
        run = torch.where(seen[:, t], torch.zeros_like(run), (run + 1).clamp(max=far))
        dist[:, t] = torch.minimum(dist[:, t], run)
    return (dist <= max_gap) & ok.unsqueeze(1)


def matrices(w, ok, lv, la):
    """Per track the dense A (N, J, T, T) in w's dtype; the identity for a track that is not solvable."""
    T = w.shape[1]
    P = penalty(T, lv, la, w.dtype)
    A = torch.diag_embed(w.permute(0, 2, 1)) + P
    return torch.where(ok[..., None, None], A, torch.eye(T, dtype=w.dtype).expand_as(A))


def solve_tracks(A, rhs):
    """torch.linalg.solve of A (N, J, T, T) x = rhs (N, J, T, R), one track a call.  (The batched call is not used: after a
    torch.set_num_threads - which other test modules of the suite make - its LU of matrices of this size fails inside the LAPACK
    library with illegal pivots, or does not return.)"""
    N, J = A.shape[:2]
    return torch.stack([torch.stack([torch.linalg.solve(A[n, j], rhs[n, j]) for j in range(J)]) for n in range(N)])


def energy(x, z, w, lv, la, huber):
    """(N, J): E at x (N, T, J, 3), rho as configured."""
    r = torch.sqrt(((x - z) ** 2).sum(-1))
    rho = r * r if huber <= 0 else torch.where(r > huber, 2.0 * huber * r - huber * huber, r * r)
    E = (w * rho).sum(1)
    if x.shape[1] >= 2:
        E = E + lv * ((x[:, 1:] - x[:, :-1]) ** 2).sum((1, 3))
    if x.shape[1] >= 3:
        E = E + la * ((x[:, 2:] - 2.0 * x[:, 1:-1] + x[:, :-2]) ** 2).sum((1, 3))
    return E


def smooth(pose, weight, obs, lv, la, huber=0.0, reweights=0, max_gap=8, dt=torch.float64):
    """The statement in dtype `dt` on the given (fp32) operands -> dict(pose (N, T, J, 3), valid (N, T, J) bool, residual, weight
    (N, T, J), energy (N, J), ok (N, J) bool).  With requires_grad operands of dtype `dt` the plain form is differentiable.  Raises
    what torch.linalg.solve raises where a float32 evaluation does not factor."""
    pose = pose if pose.dtype == dt else pose.to(dt)
    weight = None if weight is None else (weight if weight.dtype == dt else weight.to(dt))
    w, z = base_weights(pose, weight, obs)
    ok = solvable(w.detach(), lv)
    s = torch.ones_like(w)
    for k in range(reweights + 1):
        used = w * s
        A = matrices(used, ok, lv, la)
        rhs = (used.unsqueeze(-1) * z).permute(0, 2, 1, 3)                            # (N, J, T, 3)
        x = solve_tracks(A, rhs).permute(0, 2, 1, 3)
        if k < reweights:
            r = torch.sqrt(((x - z) ** 2).sum(-1))
            s = torch.where(r > huber, huber / torch.where(r > huber, r, torch.ones_like(r)), torch.ones_like(r))
    live = ok.unsqueeze(1)
    zero = torch.zeros_like(w)
    x = torch.where(live.unsqueeze(-1), x, torch.zeros_like(x))
    r = torch.sqrt(torch.where(w > 0, ((x - z) ** 2).sum(-1), zero))
    return {"pose": x, "valid": validity(w.detach(), ok, max_gap), "residual": torch.where(live, r, zero),
            "weight": torch.where(live, used, zero), "energy": torch.where(ok, energy(x, z, w, lv, la, huber), torch.zeros_like(w[:, 0])),
            "ok": ok}


def try_smooth(*args, **kw):
    """`smooth`, or None where the evaluation does not factor or is not finite (float32 on an ill-conditioned clip)."""
    try:
        out = smooth(*args, **kw)
    except RuntimeError:
        return None
    return out if all(bool(torch.isfinite(out[k]).all()) for k in ("pose", "residual", "weight", "energy")) else None


# --------------------------------------------------------------------------- the banded elimination, as a loop

def band(T, lv, la):
    """Rows of lv D1^T D1 + la D2^T D2 written down directly: diagonal a (T), A[t][t+1] = b (T), A[t][t+2] = c (T), python floats."""
    a, b, c = [], [], []
    for t in range(T):
        mid, up, dn = int(1 <= t <= T - 2), int(t + 1 <= T - 2), int(t >= 2)
        a.append(lv * (int(t > 0) + int(t < T - 1)) + la * (up + 4 * mid + dn))
        b.append(-lv - la * 2 * (mid + up) if t < T - 1 else 0.0)
        c.append(la if up else 0.0)
    return a, b, c


def banded(w, z, lv, la):
    """x (N, T, J, 3) float64 of A x = W z by LDL^T along t without pivoting: d_t = a_t - e_{t-1}^2 d_{t-1} - f_{t-2}^2 d_{t-2},
    e_t = (b_t - f_{t-1} d_{t-1} e_{t-1}) / d_t, f_t = c_t / d_t, then the two substitutions.  Every track is eliminated (a track
    that is not solvable divides by zero: mask it afterwards)."""
    w, z = w.double(), z.double()
    N, T, J = w.shape
    a, b, c = band(T, lv, la)
    zero = torch.zeros(N, J, dtype=torch.float64)
    d, e, f, y = [], [], [], []
    for t in range(T):
        dt_ = a[t] + w[:, t]
        yt = w[:, t].unsqueeze(-1) * z[:, t]
        et = torch.full_like(zero, b[t])
        if t >= 1:
            dt_ = dt_ - e[t - 1] ** 2 * d[t - 1]
            yt = yt - e[t - 1].unsqueeze(-1) * y[t - 1]
            et = et - f[t - 1] * d[t - 1] * e[t - 1]
        if t >= 2:
            dt_ = dt_ - f[t - 2] ** 2 * d[t - 2]
            yt = yt - f[t - 2].unsqueeze(-1) * y[t - 2]
        d.append(dt_)
        e.append(et / dt_)
        f.append(c[t] / dt_)
        y.append(yt)
    x = [None] * T
    for t in range(T - 1, -1, -1):
        xt = y[t] / d[t].unsqueeze(-1)
        if t + 1 < T:
            xt = xt - e[t].unsqueeze(-1) * x[t + 1]
        if t + 2 < T:
            xt = xt - f[t].unsqueeze(-1) * x[t + 2]
        x[t] = xt
    return torch.stack(x, 1)


def stationarity(pose32, weight, obs, operand_pose, lv, la):
    """At the returned fp32 pose (N, T, J, 3): g = A x - W z in float64 (N, T, J, 3), the allowance sum_k |A_ik| ulp32(max |x| of
    the track) (N, T, J) and the solvable flags (N, J) - of the plain form on the operands' base weights."""
    w, z = base_weights(operand_pose.double(), None if weight is None else weight.double(), obs)
    ok = solvable(w, lv)
    A = matrices(w, ok, lv, la)
    x = pose32.double().permute(0, 2, 1, 3)
    g = (A @ x - (w.unsqueeze(-1) * z).permute(0, 2, 1, 3)).permute(0, 2, 1, 3)
    g = torch.where(ok.view(ok.shape[0], 1, ok.shape[1], 1), g, torch.zeros_like(g))  # (a track that is not solvable has no system)
    top = x.abs().amax((2, 3))
    ulp = torch.tensor([[FS.ulp32(float(v)) for v in row] for row in top], dtype=torch.float64)
    return g, (A.abs().sum(-1) * ulp.unsqueeze(-1)).permute(0, 2, 1), ok


def condition(pose, weight, obs, lv, la):
    """The largest 2-norm condition number of A over the solvable tracks of a scene (1 when there is none)."""
    w, _ = base_weights(pose.double(), None if weight is None else weight.double(), obs)
    ok = solvable(w, lv)
    if not bool(ok.any()):
        return 1.0
    return max(float(torch.linalg.cond(A)) for A in matrices(w, ok, lv, la)[ok])          # (one track a call, as solve_tracks)


# --------------------------------------------------------------------------- scenes

def motion(N, T, J, g):
    """A moving skeleton, float64 (N, T, J, 3) cm: every joint swings about its own place, a few cm per frame at the most."""
    t = torch.arange(T, dtype=torch.float64).view(1, T, 1, 1)
    place = FS.random_points(N, J, g).unsqueeze(1)
    amp = 4.0 + 8.0 * torch.rand(N, 1, J, 3, generator=g, dtype=torch.float64)
    freq = 0.02 + 0.06 * torch.rand(N, 1, J, 3, generator=g, dtype=torch.float64)
    phase = 6.283185307179586 * torch.rand(N, 1, J, 3, generator=g, dtype=torch.float64)
    drift = 0.05 * torch.randn(N, 1, J, 3, generator=g, dtype=torch.float64)
    return place + amp * torch.sin(freq * t + phase) + drift * t


def scene(N, T, J, case, seed=0, noise=0.5):
    """dict(pose (N, T, J, 3) fp32, weight (N, T, J) fp32 | None, obs (N, T, J) uint8 | None, truth float64) of one case;
    `nonfinite` also carries `twin`: the same scene with the planted values replaced by zeros at weight 0."""
    assert case in CASES, case
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + 13 * T + 31 * J + CASES.index(case))
    truth = motion(N, T, J, g)
    pose = (truth + noise * torch.randn(N, T, J, 3, generator=g, dtype=torch.float64)).float()
    weight = (0.5 + 0.5 * torch.rand(N, T, J, generator=g)).float()
    obs = None
    drop = torch.rand(N, T, J, generator=g) < 0.3
    if T > 20:
        start = int(torch.randint(2, T - 14, (1,), generator=g))
        drop[:, start:start + 12, ::2] = True
    out = {"truth": truth}
    if case == "gaps":
        weight[drop] = 0.0
    elif case == "ends":
        q = T // 4
        weight[:, :q] = 0.0
        weight[:, T - q:] = 0.0
    elif case == "sparse":
        keep = torch.zeros(N, T, J, dtype=torch.bool)
        for n in range(N):
            for j in range(J):
                count = min(2 - (n + j) % 3, T)                                       # exactly 2, 1 and 0 observations
                if count == 2:
                    first = int(torch.randint(0, max(T // 3, 1), (1,), generator=g))
                    second = T - 1 - int(torch.randint(0, max(T // 3, 1), (1,), generator=g))
                    keep[n, first, j] = keep[n, max(second, first + 1), j] = True
                elif count == 1:
                    keep[n, int(torch.randint(0, T, (1,), generator=g)), j] = True
        weight[~keep] = 0.0
    elif case == "nonfinite":
        weight[drop] = 0.0
        twin_pose, twin_weight = pose.clone(), weight.clone()
        planted = torch.rand(N, T, J, generator=g) < 0.15                              # at weight 0 and at w > 0 alike
        kind = torch.randint(0, 4, (N, T, J), generator=g)
        bad = torch.tensor([float("nan"), float("inf"), float("-inf")])
        for n, t, j in planted.nonzero().tolist():
            k = int(kind[n, t, j])
            if k == 3:
                weight[n, t, j] = bad[(n + t + j) % 3]                                 # a weight that is not finite
            else:
                pose[n, t, j, (t + j) % 3] = bad[k]
            twin_pose[n, t, j] = 0.0
            twin_weight[n, t, j] = 0.0
        unseen = weight == 0.0
        pose[unseen & (torch.rand(N, T, J, generator=g) < 0.5)] = float("nan")         # and at frames nobody observed
        twin_pose[unseen] = 0.0
        out["twin"] = {"pose": twin_pose, "weight": twin_weight, "obs": None}
    elif case == "mask":
        obs, weight = (~drop).to(torch.uint8), None
    elif case == "glitch":
        for n in range(N):
            for j in range(J):
                for t in torch.randperm(T, generator=g)[:3].tolist():
                    d = torch.randn(3, generator=g)
                    pose[n, t, j] += (d / d.norm() * (25.0 + 25.0 * float(torch.rand(1, generator=g)))).float()
    out.update(pose=pose.contiguous(), weight=weight, obs=obs)
    return out

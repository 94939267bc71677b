"""Statements of the bone-length-constrained skeleton fit (egr_skeleton_fit_f32) and of the two small launches that belong with it
(egr_bone_lengths_f32, egr_skeleton_resize_f32), DESIGN.md 5q, in torch, so that they run in float64 and in float32:

  energy          nothing but the three sums of the energy, on the rays of fisheye_statement.py (the triangulation's);
  fit_statement   the kernel's algorithm - Levenberg-Marquardt on the Gauss-Newton model with the header's damping schedule - with a
                  dense Cholesky solve in place of the elimination along the tree;
  newton_referee  a different algorithm: full Newton on the exact autograd Hessian with a backtracking line search, to |grad| < 1e-10;
  bone_lengths_statement, resize_statement  the small launches, as loops.

The scenes the CPU and the GPU tests share are made here too."""
import math

import torch

import fisheye_statement as FS

HM = FS.HM
MU0, MU_DOWN, MU_UP, MU_MIN, MU_MAX = 1e-3, 0.1, 10.0, 1e-12, 1e12     # the damping schedule of include/egorear_hip.h
MIN_BONE = 1e-9
PARENTS_16 = (0, 0, 1, 1, 2, 3, 4, 5, 2, 3, 8, 9, 10, 11, 12, 13)        # Skeleton.kinematic_parents of the reference


def parents_15():
    """The 16-joint table with joint 0 removed and the rest re-indexed: the neck becomes the root."""
    return tuple(max(p - 1, 0) for p in PARENTS_16[1:])


class Problem:
    """One launch's operands, the rays made of them, and what is decided once per frame: which joints and bones take part."""

    def __init__(self, coords, conf, rec, ctm, parents, bone_length, init, init_ok, lam, rho, sx=1.0 / HM, sy=1.0 / HM, thr=FS.THR,
                 min_det_ratio=FS.MIN_DET):
        dt = coords.dtype
        B, V, J = conf.shape
        self.B, self.V, self.J, self.dt, self.lam, self.rho = B, V, J, dt, float(lam), float(rho)
        self.parents = torch.tensor(list(parents), dtype=torch.int64)
        _, self.w, self.d, self.R, self.t = FS.rays(coords, conf, rec, ctm, sx, sy, thr)
        tri_ok = FS.statement(coords, conf, rec, ctm, sx, sy, thr, min_det_ratio)[3]
        used = (self.w > 0).sum(1)
        L = bone_length.to(dt).expand(B, J) if bone_length.dim() == 1 else bone_length.to(dt)
        constrained = (L > 0) & torch.isfinite(L)
        constrained[:, 0] = False
        init = init.to(dt)
        fine = init_ok.bool() & torch.isfinite(init).all(-1)
        active = torch.zeros(B, J, dtype=torch.bool)
        for j in range(J):                       # in index order: a parent is decided before its children
            par = int(self.parents[j])
            anchored = (used[:, j] >= 1) & constrained[:, j] & active[:, par] if j > 0 else torch.zeros(B, dtype=torch.bool)
            active[:, j] = fine[:, j] & (tri_ok[:, j] | anchored) if self.rho == 0.0 else fine[:, j]
        self.active = active
        self.bone_on = active & constrained & active[:, self.parents]
        self.L = torch.where(constrained, L, torch.zeros_like(L))
        self.init = torch.where(fine.unsqueeze(-1), init, torch.zeros_like(init))
        self.wsum = self.w.sum(1)
        A, b = FS.normal_equations(self.w, self.d, self.R, self.t)      # of every joint's rays: A p = b, (B, J, 3, 3) and (B, J, 3)
        self.A = torch.stack([torch.stack([A[min(k, l), max(k, l)] for l in range(3)], -1) for k in range(3)], -2)
        self.b = torch.stack(b, -1)

    def start(self):
        return torch.where(self.active.unsqueeze(-1), self.init, torch.zeros_like(self.init))


def bone_vectors(pr, p):
    """(d, len) of every joint's bone to its parent; where the bone is not used d is (1, 0, 0), so that the length differentiates."""
    d = p - p[:, pr.parents]
    safe = torch.zeros_like(d)
    safe[..., 0] = 1.0
    d = torch.where(pr.bone_on.unsqueeze(-1), d, safe)
    return d, torch.sqrt((d * d).sum(-1))


def energy(pr, p):
    """E (B) = sum_j sum_v w dist^2 + lambda sum_bones (len - L)^2 + rho sum_j |p - init|^2 over the active joints and used bones; and
    the joints' data sums (B, J)."""
    data = (pr.w * FS.ray_dist2(pr.d, pr.R, pr.t, lambda k: p[..., k])).sum(1)
    prior = pr.rho * ((p - pr.init) ** 2).sum(-1)
    _, length = bone_vectors(pr, p)
    zero = torch.zeros_like(data)
    per_joint = torch.where(pr.active, data + prior, zero) + torch.where(pr.bone_on, pr.lam * (length - pr.L) ** 2, zero)
    return per_joint.sum(1), data


def results(pr, p):
    """The kernel's per-joint outputs at p: pose, ray_cost, bone, valid."""
    E, data = energy(pr, p)
    zero = torch.zeros_like(data)
    cost = torch.where(pr.active & (pr.wsum > 0), data / torch.where(pr.wsum > 0, pr.wsum, torch.ones_like(pr.wsum)), zero)
    _, length = bone_vectors(pr, p)
    return {"pose": torch.where(pr.active.unsqueeze(-1), p, torch.zeros_like(p)), "ray_cost": cost,
            "bone": torch.where(pr.bone_on, length, zero), "valid": pr.active, "bone_on": pr.bone_on, "energy": E}


# --------------------------------------------------------------------------- the kernel's algorithm, dense

def gauss_newton_system(pr, p):
    """g = dE/dp / 2 (B, J, 3), the Gauss-Newton H / 2 (B, 3J, 3J) - rows of joints that take no part are the identity - and gq, the
    share of g that the quadratic terms (rays and prior) have."""
    B, J = pr.B, pr.J
    d, length = bone_vectors(pr, p)
    has_dir = pr.bone_on & (length >= MIN_BONE)
    u = torch.where(has_dir.unsqueeze(-1), d / torch.where(has_dir, length, torch.ones_like(length)).unsqueeze(-1), torch.zeros_like(d))
    lr = torch.where(pr.bone_on, pr.lam * (length - pr.L), torch.zeros_like(length)).unsqueeze(-1)
    gq = (pr.A @ p.unsqueeze(-1)).squeeze(-1) - pr.b + pr.rho * (p - pr.init)
    gq = torch.where(pr.active.unsqueeze(-1), gq, torch.zeros_like(gq))
    g = (gq + lr * u).index_add(1, pr.parents, -(lr * u))
    uu = pr.lam * u.unsqueeze(-1) * u.unsqueeze(-2)                                    # (B, J, 3, 3)
    eye = torch.eye(3, dtype=pr.dt).expand(B, J, 3, 3)
    Hd = torch.where(pr.active.view(B, J, 1, 1), pr.A + pr.rho * eye + uu, eye).index_add(1, pr.parents, uu)
    H = torch.zeros(B, J, 3, J, 3, dtype=pr.dt)
    for j in range(J):
        par = int(pr.parents[j])
        H[:, j, :, j, :] = Hd[:, j]
        if j > 0:
            H[:, j, :, par, :] = H[:, j, :, par, :] - uu[:, j]
            H[:, par, :, j, :] = H[:, par, :, j, :] - uu[:, j]
    return g, H.view(B, 3 * J, 3 * J), gq


def energy_change(pr, p, delta, gq):
    """E(p + delta) - E(p) (B), as a difference: exactly 2 gq . delta + delta^T (A + rho I) delta for the quadratic terms, and
    lambda (len' - len)(r + r') with len' - len = (dd . (d + d')) / (len + len') for a bone - so that steps far below the rounding
    of E itself are still decided by their sign (the kernel's rule)."""
    quad = ((2.0 * gq + (pr.A @ delta.unsqueeze(-1)).squeeze(-1) + pr.rho * delta) * delta).sum(-1)
    d, length = bone_vectors(pr, p)
    d2, length2 = bone_vectors(pr, p + delta)
    dd = delta - delta[:, pr.parents]
    total = length + length2
    dlen = torch.where(total > 0, (dd * (d + d2)).sum(-1) / torch.where(total > 0, total, torch.ones_like(total)), torch.zeros_like(total))
    zero = torch.zeros_like(quad)
    bone = pr.lam * dlen * ((length - pr.L) + (length2 - pr.L))
    return (torch.where(pr.active, quad, zero) + torch.where(pr.bone_on, bone, zero)).sum(1)


def fit_statement(pr, iterations):
    """-> (results at the fitted p, energy0 (B), grad (B), steps (B)), by the kernel's rule: `iterations` times solve
    (H + mu diag H) delta = -g, keep p + delta iff the system is positive definite and E does not increase; mu as in the header."""
    B, J = pr.B, pr.J
    p = pr.start()
    E0 = energy(pr, p)[0]
    mu = torch.full((B,), MU0, dtype=pr.dt)
    steps = torch.zeros(B, dtype=torch.int32)
    for _ in range(iterations):
        g, H, gq = gauss_newton_system(pr, p)
        damped = H + mu.view(B, 1, 1) * torch.diag_embed(torch.diagonal(H, dim1=1, dim2=2))
        chol, info = torch.linalg.cholesky_ex(damped)
        chol = torch.where((info == 0).view(B, 1, 1), chol, torch.eye(3 * J, dtype=pr.dt).expand(B, -1, -1))
        delta = torch.cholesky_solve(-g.reshape(B, 3 * J, 1), chol).view(B, J, 3)
        delta = torch.where(pr.active.unsqueeze(-1), delta, torch.zeros_like(delta))
        keep = (info == 0) & (energy_change(pr, p, delta, gq) <= 0)
        p = torch.where(keep.view(B, 1, 1), p + delta, p)
        steps += keep.to(torch.int32)
        mu = torch.where(keep, torch.clamp(mu * MU_DOWN, min=MU_MIN), torch.clamp(mu * MU_UP, max=MU_MAX))
    g = gauss_newton_system(pr, p)[0]
    out = results(pr, p)
    steps = torch.where(pr.active.any(1), steps, torch.zeros_like(steps))             # a frame without an active joint gives zeros
    return out, E0, 2.0 * g.abs().amax((1, 2)), steps


# --------------------------------------------------------------------------- the referee and the stationarity measure

def grad_hess(pr, pose):
    """dE/dp (B, 3J) and the exact Hessian (B, 3J, 3J) of `energy` at `pose`, by autograd."""
    B, J = pr.B, pr.J
    p = pose.clone().to(pr.dt).requires_grad_()
    E = energy(pr, p)[0].sum()
    (g,) = torch.autograd.grad(E, p, create_graph=True)
    flat = g.reshape(-1)
    rows = []
    for i in range(flat.numel()):
        (row,) = torch.autograd.grad(flat[i], p, retain_graph=True, allow_unused=True)
        rows.append(torch.zeros_like(p) if row is None else row)
    Hall = torch.stack(rows).view(B, 3 * J, B, 3 * J)
    H = torch.stack([Hall[b, :, b, :] for b in range(B)])
    return g.detach().reshape(B, 3 * J), H


def newton_referee(pr, start=None, tol=1e-10, max_iter=100):
    """-> (pose (B, J, 3), largest |dE/dp| component (B)): full Newton on the exact Hessian (shifted by tau I only while it is not
    positive definite), Armijo backtracking, every frame to |grad| < tol; from the init, or from `start` (a ray meets a bone's sphere
    twice: where the energy has two minima, `start` says which basin is meant)."""
    B, J = pr.B, pr.J
    p = (pr.start() if start is None else torch.where(pr.active.unsqueeze(-1), start.to(pr.dt), torch.zeros_like(pr.init))).clone()
    mask = pr.active.unsqueeze(-1).expand(B, J, 3).reshape(B, 3 * J)
    eye = torch.eye(3 * J, dtype=pr.dt)
    gmax = torch.zeros(B, dtype=pr.dt)
    for b in range(B):
        sub = _OneFrame(pr, b)
        x = p[b:b + 1]
        for _ in range(max_iter):
            g, H = grad_hess(sub, x)
            g, H = g[0], H[0]
            m = mask[b]
            gmax[b] = g[m].abs().max() if bool(m.any()) else 0.0
            if float(gmax[b]) < tol:
                break
            H = torch.where(m.unsqueeze(0) & m.unsqueeze(1), H, eye)
            tau = 0.0
            while True:
                chol, info = torch.linalg.cholesky_ex(H + tau * eye)
                if int(info) == 0:
                    break
                tau = max(10.0 * tau, 1e-6)
            step = torch.cholesky_solve(-torch.where(m, g, torch.zeros_like(g)).view(-1, 1), chol).view(1, J, 3)
            E, slope, s = float(energy(sub, x)[0]), float((g * step.view(-1)).sum()), 1.0
            # (the last term: E is a sum, and its own rounding must not refuse the steps that finish the convergence)
            while s > 1e-12 and not float(energy(sub, x + s * step)[0]) <= E + 1e-4 * s * slope + 1e-14 * abs(E):
                s *= 0.5
            x = x + s * step
        p[b:b + 1] = x
    return p, gmax


class _OneFrame:
    """Frame b of a Problem, as a Problem of one frame."""

    def __init__(self, pr, b):
        pick = lambda a: a[b:b + 1] if a.shape[0] == pr.B and pr.B > 1 else a
        self.B, self.V, self.J, self.dt, self.lam, self.rho, self.parents = 1, pr.V, pr.J, pr.dt, pr.lam, pr.rho, pr.parents
        self.w, self.d = pr.w[b:b + 1], [x[b:b + 1] for x in pr.d]
        self.R, self.t = [[pick(x) for x in row] for row in pr.R], [pick(x) for x in pr.t]
        for name in ("active", "bone_on", "L", "init", "wsum", "A", "b"):
            setattr(self, name, getattr(pr, name)[b:b + 1])

    start = Problem.start


# --------------------------------------------------------------------------- the two small launches

def bone_lengths_statement(pose, valid, parents):
    """-> length (J), spread (J), count (J): mean and population standard deviation over the frames where both ends are valid."""
    B, J, _ = pose.shape
    length, spread, count = torch.zeros(J, dtype=pose.dtype), torch.zeros(J, dtype=pose.dtype), torch.zeros(J, dtype=torch.int32)
    for j in range(1, J):
        both = valid[:, j].bool() & valid[:, parents[j]].bool()
        if int(both.sum()) == 0:
            continue
        lens = (pose[both, j] - pose[both, parents[j]]).norm(dim=-1)
        length[j], count[j] = lens.mean(), int(both.sum())
        spread[j] = torch.sqrt(((lens - lens.mean()) ** 2).mean())
    return length, spread, count


def resize_statement(pose, valid, bone_length, parents):
    """Skeleton._skeleton_resize in cm, with the validity rule: a joint that is not valid keeps its place, and so does a joint whose
    parent is not valid; a bone without a length (<= 0, not finite) or without a direction keeps its vector."""
    B, J, _ = pose.shape
    L = bone_length.expand(B, J) if bone_length.dim() == 1 else bone_length
    out = pose.clone()
    for b in range(B):
        for j in range(1, J):
            par = parents[j]
            if not (bool(valid[b, j]) and bool(valid[b, par])):
                continue
            d = pose[b, j] - pose[b, par]
            n = float(d.norm())
            if float(L[b, j]) > 0 and math.isfinite(float(L[b, j])) and n >= MIN_BONE:
                d = d * (L[b, j] / d.norm())
            out[b, j] = out[b, par] + d
    return out


# --------------------------------------------------------------------------- scenes

def chain_parents(J):
    return tuple(max(j - 1, 0) for j in range(J))


def default_parents(J, chain=False):
    if chain:
        return chain_parents(J)
    return PARENTS_16 if J == 16 else parents_15() if J == 15 else chain_parents(J)


def random_skeleton(B, J, parents, g):
    """Poses (B, J, 3) float64 of a skeleton whose bones (J, the same in every frame) are 10 to 35 cm, inside the box of FS.random_points."""
    lengths = torch.rand(J, generator=g, dtype=torch.float64) * 25 + 10
    lengths[0] = 0.0
    lo, hi = torch.tensor([-60.0, -40.0, 15.0], dtype=torch.float64), torch.tensor([60.0, 80.0, 150.0], dtype=torch.float64)
    pts = torch.zeros(B, J, 3, dtype=torch.float64)
    pts[:, 0] = FS.random_points(B, 1, g)[:, 0] * 0.5 + torch.tensor([0.0, 10.0, 40.0], dtype=torch.float64)
    for j in range(1, J):
        u = torch.randn(B, 3, generator=g, dtype=torch.float64)
        u = u / u.norm(dim=-1, keepdim=True)
        child = pts[:, parents[j]] + lengths[j] * u
        u = torch.where((child < lo) | (child > hi), -u, u)                            # a step out of the box is mirrored back in
        pts[:, j] = pts[:, parents[j]] + lengths[j] * u
    return pts, lengths


def scene(B, V, J, rw, chain=False, noise=0.1, off=3.0, seed=None):
    """A skeleton seen by the rig: poses, true bone lengths, noisy fp32 coords (pixels of a 64 x 64 map), confidences, an init `off` cm
    from the truth.  (The noise sets how fast Gauss-Newton converges: the curvature it drops is a bone's tension over its length,
    the tension is what the noise leaves at the optimum, and along the rays the data term is soft - DESIGN.md 5q has the table.)"""
    g = torch.Generator().manual_seed(1000 * B + 100 * V + J if seed is None else seed)
    parents = default_parents(J, chain)
    cams = FS.rig("ego4view_rw" if rw else "ego4view_syn")[:V]
    rec = FS.records(cams)
    ctm = FS.random_ctm(B, V, cams, g) if rw else None
    pts, lengths = random_skeleton(B, J, parents, g)
    coords = (FS.project(pts, rec, ctm) * HM + noise * torch.randn(B, V, J, 2, generator=g, dtype=torch.float64)).float()
    conf = (torch.rand(B, V, J, generator=g) * 0.4 + 0.6).float()
    u = torch.randn(B, J, 3, generator=g, dtype=torch.float64)
    init = (pts + off * u / u.norm(dim=-1, keepdim=True)).float()
    return {"B": B, "V": V, "J": J, "parents": parents, "cams": cams, "rec": rec, "ctm": ctm, "pts": pts, "lengths": lengths.float(),
            "coords": coords.contiguous(), "conf": conf.contiguous(), "init": init.contiguous(),
            "init_ok": torch.ones(B, J, dtype=torch.uint8)}


def limb_joint(parents):
    """The last joint of the table: a leaf at the end of a limb (the only child of the root when there is one bone)."""
    return len(parents) - 1


def keep_views(sc, joint, views, frame=None):
    """A copy of the scene's conf in which `joint` keeps the first `views` of its views (the rest fall below the threshold)."""
    conf = sc["conf"].clone()
    frames = range(sc["B"]) if frame is None else [frame]
    for b in frames:
        conf[b, views:, joint] = 0.3
    return conf


CASES = ("full", "one_view", "unseen_prior", "unseen", "no_init", "nonfinite", "free_bones")
LAMBDAS = (0.0, 1.0, 10.0)
NAN, INF = float("nan"), float("inf")


def case_operands(sc, case):
    """The scene's operands bent into one of the cases: coords, conf, init, init_ok, bone_length, rho (the scene is not modified)."""
    B, J = sc["B"], sc["J"]
    coords, conf, init, init_ok, L = (sc[k].clone() for k in ("coords", "conf", "init", "init_ok", "lengths"))
    leaf, mid, rho = limb_joint(sc["parents"]), J // 2, 0.0
    if case == "one_view":                   # the limb's last joint keeps view 0 alone
        conf[:, 1:, leaf] = 0.3
    elif case in ("unseen_prior", "unseen"):  # ... or no view at all: only a prior can hold it
        conf[:, :, leaf] = 0.3
        rho = 1e-3 if case == "unseen_prior" else 0.0
    elif case == "no_init":                  # a leaf without an init in the first frame, a mid-chain joint in the last
        init_ok[0, leaf] = 0
        init_ok[B - 1, mid] = 0
    elif case == "nonfinite":
        coords[0, 0, leaf, 0] = NAN          # that view alone is excluded
        coords[B - 1, 1, 0, 1] = INF
        conf[0, 1, mid] = INF
        conf[B - 1, 0, leaf] = NAN
        init[0, mid, 1] = NAN                # that joint has no init
        init[B - 1, 0, 2] = -INF
    elif case == "free_bones":               # lengths that leave their bones unconstrained
        L[leaf] = 0.0
        if J > 2:
            L[1] = -5.0
        if J > 3:
            L[2] = NAN
    elif case != "full":
        raise ValueError(case)
    if sc["ctm"] is not None:                # the rw scene carries its lengths per frame
        L = L.expand(B, J).contiguous()
    return {"coords": coords, "conf": conf, "init": init, "init_ok": init_ok, "bone_length": L, "rho": rho}


def problem(sc, ops, lam, dt):
    cast = lambda t: t.to(dt)
    return Problem(cast(ops["coords"]), cast(ops["conf"]), sc["rec"], sc["ctm"], sc["parents"], cast(ops["bone_length"]), cast(ops["init"]),
                   ops["init_ok"], lam, ops["rho"])


def stationarity(pr, pose, margin=FS.MARGIN):
    """-> (the largest |g_i| / allowed_i over the active components, g (B, 3J), the active components (B, 3J), allowed (B, 3J)) at
    `pose`, with g and the exact H of `energy` in float64 and allowed_i = margin * sum_k |H_ik| * ulp32(max |pose|): rounding the
    minimiser to fp32 costs up to 1 / (2 margin) of that."""
    g, H = grad_hess(pr, pose.double())
    allowed = margin * H.abs().sum(-1) * FS.ulp32(float(pose.abs().max()))
    m = pr.active.unsqueeze(-1).expand(pr.B, pr.J, 3).reshape(pr.B, 3 * pr.J)
    if not bool(m.any()):
        return 0.0, g, m, allowed
    return float((g.abs()[m] / allowed[m]).max()), g, m, allowed

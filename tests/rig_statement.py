"""The float64 statement of the rig self-calibration (egr_rig_refine_f32, egorear_amd/decode.py refine_rig), in elementwise
torch operations on top of fisheye_statement's rays, normal equations and ray distances: the reduced objective as a function of the
cameras' rotation vectors, the Levenberg-Marquardt iteration of the kernel with its mask rule and damping schedule, the solver-independent
stationarity check, the scenes and the cases.  Every function computes in the dtype of its operands, so the same code gives the float64
statement and torch's fp32 evaluation of it, which sets the allowance of the GPU test.  Not a test module: test_rig_host.py,
test_gpu_rig.py and tools/rig_accuracy.py import it.

  E(dR_0..dR_{V-1}) = sum_pairs min_p sum_v w_v |P(d_v) dR_v (R_v p + t_v)|^2 + prior_weight * sum_v |dR_v - I|_F^2,   P(d) = I - d d^T

(the rotation of the ray by dR^T is written as the rotation of the camera-frame point by dR: the same distance).  A pair (frame, joint)
counts when, at dR = I, two views or more carry weight and its normal equations pass rays::factor's test with min_det_ratio; later
iterates solve the same pairs with the positivity test alone, and a candidate at which one of them fails is refused.

The damping schedule (stated once in DESIGN.md 5t): mu starts at MU0 = 1e-4; every iteration solves (H + mu diag H) delta = -g on the
free cameras at the accepted rotations, H the Gauss-Newton matrix of the data term with the point eliminated plus the prior's exact
Hessian, and tries dR <- exp([delta]x) dR; the candidate is accepted iff every counted pair factors and E falls strictly, after which mu
is multiplied by 0.1 (not below 1e-12); a refused one multiplies it by 10 (not above 1e12) and the next iteration solves again from
the stored system."""
import math

import torch

import fisheye_statement as FS

MARGIN = FS.MARGIN
HM = FS.HM
MU0, MU_DOWN, MU_UP, MU_MIN, MU_MAX = 1e-4, 0.1, 10.0, 1e-12, 1e12
PIVOT_TOL = 1e-10         # a pivot of the undamped first system at or below this fraction of its diagonal entry: not factorable
CASES = ("calibrated", "rotated", "noisy", "emptied", "prior", "all_fixed", "nothing")
PRIOR = 1.0e3


# --------------------------------------------------------------------------- small dense algebra, elementwise

def mm(a, b):
    """(..., n, k) @ (..., k, m) as products and one sum."""
    return (a.unsqueeze(-1) * b.unsqueeze(-3)).sum(-2)


def tr(a):
    return a.transpose(-1, -2)


def skew(r):
    """[r]x of r (..., 3)."""
    z = torch.zeros_like(r[..., 0])
    return torch.stack((torch.stack((z, -r[..., 2], r[..., 1]), -1), torch.stack((r[..., 2], z, -r[..., 0]), -1),
                        torch.stack((-r[..., 1], r[..., 0], z), -1)), -2)


def expm(r):
    """Rodrigues: rotation vectors (..., 3) -> matrices (..., 3, 3); below 1e-4 rad the two series, smooth through 0."""
    th2 = (r * r).sum(-1)
    small = th2 < 1e-8
    ths = torch.sqrt(torch.where(small, torch.ones_like(th2), th2))
    a = torch.where(small, 1.0 - th2 / 6.0, torch.sin(ths) / ths)
    b = torch.where(small, 0.5 - th2 / 24.0, (1.0 - torch.cos(ths)) / (ths * ths))
    K = skew(r)
    return torch.eye(3, dtype=r.dtype) + a[..., None, None] * K + b[..., None, None] * mm(K, K)


def logm(M):
    """The rotation vector (..., 3) of matrices (..., 3, 3) whose angle stays away from pi."""
    a = 0.5 * torch.stack((M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0], M[..., 1, 0] - M[..., 0, 1]), -1)
    s2 = (a * a).sum(-1)
    s = torch.sqrt(s2)
    c = 0.5 * (M[..., 0, 0] + M[..., 1, 1] + M[..., 2, 2] - 1.0)
    small = s < 1e-6
    k = torch.where(small, 1.0 + s2 / 6.0, torch.atan2(s, c) / torch.where(small, torch.ones_like(s), s))
    return a * k.unsqueeze(-1)


def inverse3(A):
    """A^-1 and det of symmetric A given as the dictionary of FS.normal_equations, by cofactors: (B, J, 3, 3), (B, J)."""
    a00, a01, a02, a11, a12, a22 = A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]
    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    det = a00 * c00 + a01 * c01 + a02 * c02
    adj = torch.stack((torch.stack((c00, c01, c02), -1), torch.stack((c01, c11, c12), -1), torch.stack((c02, c12, c22), -1)), -2)
    return adj, det


def positive(A):
    """rays::factor's positivity: the three pivots of the LDL^T of A."""
    d1 = A[0, 0]
    l21, l31 = A[0, 1] / d1, A[0, 2] / d1
    d2 = A[1, 1] - l21 * A[0, 1]
    l32 = (A[1, 2] - l31 * A[0, 1]) / d2
    d3 = A[2, 2] - l31 * A[0, 2] - l32 * l32 * d2
    return (d1 > 0) & (d2 > 0) & (d3 > 0), d1 * d2 * d3


def ldl_solve(H, rhs, tol=0.0):
    """x of H x = rhs for a small symmetric H (n, n) by LDL^T, a scalar at a time; None when a pivot is not above tol * its diagonal."""
    n = H.shape[0]
    L = [[None] * n for _ in range(n)]
    d = [None] * n
    for j in range(n):
        dj = H[j, j]
        for k in range(j):
            dj = dj - L[j][k] * L[j][k] * d[k]
        if not bool(dj > tol * H[j, j]):
            return None
        d[j] = dj
        for i in range(j + 1, n):
            s = H[i, j]
            for k in range(j):
                s = s - L[i][k] * L[j][k] * d[k]
            L[i][j] = s / dj
    y = [None] * n
    for i in range(n):
        s = rhs[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s
    x = [None] * n
    for i in range(n - 1, -1, -1):
        s = y[i] / d[i]
        for k in range(i + 1, n):
            s = s - L[k][i] * x[k]
        x[i] = s
    return torch.stack(x)


# --------------------------------------------------------------------------- the problem

class Problem:
    """The rays of a clip, fixed once (they do not depend on dR), and the pairs that count."""

    def __init__(self, coords, conf, rec, ctm, fixed=None, prior_weight=0.0, thr=FS.THR, min_det_ratio=FS.MIN_DET, sx=1.0 / HM, sy=1.0 / HM):
        dt = coords.dtype
        self.dt, (self.B, self.V, self.J) = dt, coords.shape[:3]
        self.use, self.w, d, R, t = FS.rays(coords, conf, rec, ctm, sx, sy, thr)
        self.d = torch.stack(d, -1)                                                               # (B, V, J, 3)
        shape = (-1, self.V, 1)
        self.R = torch.stack([torch.stack([R[r][c].expand(shape) for c in range(3)], -1) for r in range(3)], -2)   # (B | 1, V, 1, 3, 3)
        self.t = torch.stack([t[r].expand(shape) for r in range(3)], -1)                          # (B | 1, V, 1, 3)
        self.fixed = torch.tensor([v == 0 for v in range(self.V)] if fixed is None else [bool(f) for f in fixed])
        self.pw = float(prior_weight)
        self.ctm, self.rec = ctm, rec
        A, _, _ = self.normal(torch.eye(3, dtype=dt).expand(self.V, 3, 3))
        pos, det = positive(A)
        tr3 = (A[0, 0] + A[1, 1] + A[2, 2]) / 3
        self.mask = ((self.w > 0).sum(1) >= 2) & pos & (det > min_det_ratio * tr3 * tr3 * tr3)    # (B, J)
        self.pairs = int(self.mask.sum())
        self.free = (~self.fixed).repeat_interleave(3)

    def normal(self, dR):
        """The normal equations of every pair at the rotations dR (V, 3, 3): A, b of FS.normal_equations and the rotated (R', t')."""
        Rp, tp = mm(dR[None, :, None], self.R), mm(dR[None, :, None], self.t.unsqueeze(-1)).squeeze(-1)
        Rl = [[Rp[..., r, c] for c in range(3)] for r in range(3)]
        tl = [tp[..., r] for r in range(3)]
        A, b = FS.normal_equations(self.w, [self.d[..., k] for k in range(3)], Rl, tl)
        return A, b, (Rp, tp, Rl, tl)

    def solve(self, dR):
        """The point of every pair (B, J, 3) (0 where the pair does not count), the views' squared distances (B, V, J), `failed`: a
        counted pair whose normal equations are not positive definite at dR, and the rotated extrinsics."""
        A, b, ext = self.normal(dR)
        adj, det = inverse3(A)
        pos, _ = positive(A)
        failed = bool((self.mask & ~pos).any())
        ok = self.mask & pos
        ds = torch.where(ok, det, torch.ones_like(det))
        Ainv = torch.where(ok[..., None, None], adj / ds[..., None, None], torch.zeros_like(adj))
        p = mm(Ainv, torch.stack(b, -1).unsqueeze(-1)).squeeze(-1)
        rr = FS.ray_dist2([self.d[..., k] for k in range(3)], ext[2], ext[3], lambda k: p[..., k])
        return p, rr, failed, Ainv, ext

    def prior(self, dR):
        eye = torch.eye(3, dtype=dR.dtype)
        return self.pw * ((dR - eye) ** 2).sum()

    def data(self, dR):
        """(sum over the counted pairs of w dist^2, the sum of their weights, failed)."""
        _, rr, failed, _, _ = self.solve(dR)
        wm = torch.where(self.mask.unsqueeze(1), self.w, torch.zeros_like(self.w))
        return (wm * rr).sum(), wm.sum(), failed

    def objective(self, rotvec, base=None):
        """E at dR_v = exp([rotvec_v]x) base_v (base: the identity), fixed cameras at base_v; differentiable in rotvec (V, 3)."""
        dR = expm(torch.where(self.fixed.unsqueeze(-1), torch.zeros_like(rotvec), rotvec))
        if base is not None:
            dR = mm(dR, base)
        return self.data(dR)[0] + self.prior(dR)

    def system(self, dR):
        """(E_data, wsum, failed, g (3V), H (3V, 3V)) at dR: gradient and Gauss-Newton matrix of E with the points eliminated by their
        3 x 3 Schur complements, the prior's gradient and exact Hessian added; the unknown is delta of dR <- exp([delta]x) dR."""
        V, dt = self.V, self.dt
        p, rr, failed, Ainv, (Rp, tp, _, _) = self.solve(dR)
        m = self.mask.unsqueeze(1)
        w = torch.where(m, self.w, torch.zeros_like(self.w))                                      # (B, V, J)
        q = mm(Rp, p.unsqueeze(1).unsqueeze(-1)).squeeze(-1) + tp                                 # (B, V, J, 3)
        d = self.d
        r = q - d * (d * q).sum(-1, keepdim=True)
        g = (2.0 * w.unsqueeze(-1) * torch.linalg.cross(q, r)).sum((0, 2)).reshape(3 * V)
        Q = skew(q)
        Bm = Q - d.unsqueeze(-1) * mm(d.unsqueeze(-2), Q)                                         # P [q]x
        Cm = mm(tr(Rp).expand(Bm.shape), Bm)                                                      # R'^T P [q]x
        Y = mm(Ainv.unsqueeze(1), Cm)
        H = torch.zeros(3 * V, 3 * V, dtype=dt)
        for v in range(V):
            for u in range(V):
                blk = -(w[:, v] * w[:, u])[..., None, None] * mm(tr(Cm[:, v]), Y[:, u])
                if u == v:
                    blk = blk + w[:, v][..., None, None] * mm(tr(Bm[:, v]), Bm[:, v])
                H[3 * v:3 * v + 3, 3 * u:3 * u + 3] = 2.0 * blk.sum((0, 1))
        # the prior: d/d delta |exp([delta]x) dR - I|_F^2 = 2 (dR_32 - dR_23, dR_13 - dR_31, dR_21 - dR_12); its Hessian 2 (tr dR I - sym dR)
        if self.pw > 0.0:
            vee = torch.stack((dR[:, 2, 1] - dR[:, 1, 2], dR[:, 0, 2] - dR[:, 2, 0], dR[:, 1, 0] - dR[:, 0, 1]), -1)
            g = g + 2.0 * self.pw * vee.reshape(3 * V)
            eye = torch.eye(3, dtype=dt)
            for v in range(V):
                H[3 * v:3 * v + 3, 3 * v:3 * v + 3] += 2.0 * self.pw * ((dR[v, 0, 0] + dR[v, 1, 1] + dR[v, 2, 2]) * eye - 0.5 * (dR[v] + dR[v].T))
        wm = torch.where(self.mask.unsqueeze(1), self.w, torch.zeros_like(self.w))
        return (wm * rr).sum(), wm.sum(), failed, g, H

    def grad_hess(self, base):
        """Float64 gradient and exact Hessian (autograd, the point eliminated in closed form) of delta -> E(exp([delta]x) base) at 0."""
        z = torch.zeros(self.V, 3, dtype=self.dt, requires_grad=True)
        f = lambda x: self.objective(x, base)
        g = torch.autograd.grad(f(z), z)[0].reshape(-1)
        H = torch.autograd.functional.hessian(f, z.detach()).reshape(3 * self.V, 3 * self.V)
        return g, H


def apply_correction(matrix, rec, ctm, B):
    """[dR 0; 0 1] M_v in the decoders' convention, fp32 (B, V, 4, 4), of fp32 matrices dR (V, 3, 3): M the given coord_trans_mat
    ((B | 1, V, 4, 4)), or for the syn rig the record's flip and offset as FS.random_ctm writes them, fp32; the product in float64,
    rounded once."""
    return apply_correction_f64(matrix.float().double(), rec, ctm, True).expand(B, matrix.shape[0], 4, 4).float().contiguous()


def refine_statement(pr, iterations):
    """The kernel's iteration -> dict(rotation (V, 3), matrix (V, 3, 3) fp32, cost0, cost, pairs, steps, grad, valid, costs: the mean
    squared ray distance after every iteration, accepted or not).  Invalid (no pair, or the first system does not factor): identities
    and zeros."""
    V, dt = pr.V, pr.dt
    eye = torch.eye(3, dtype=dt).expand(V, 3, 3).contiguous()
    zero = torch.zeros((), dtype=dt)
    out = dict(rotation=torch.zeros(V, 3, dtype=dt), matrix=eye.float(), cost0=zero, cost=zero, pairs=0, steps=0, grad=zero, valid=False, costs=[],
               dR=eye)
    if pr.pairs == 0:
        return out
    free = pr.free
    idx = torch.nonzero(free).flatten()
    Ed, wsum, failed, g, H = pr.system(eye)
    if failed or not bool(torch.isfinite(Ed)):
        return out
    if len(idx) and ldl_solve(H[idx][:, idx], -g[idx], PIVOT_TOL) is None:
        return out
    dR, E = eye, Ed + pr.prior(eye)
    cost0, mu, steps = Ed / wsum, MU0, 0
    costs = [float(Ed / wsum)]
    for _ in range(iterations):
        delta = torch.zeros(3 * V, dtype=dt)
        if len(idx):
            Hf = H[idx][:, idx]
            x = ldl_solve(Hf + mu * torch.diag(torch.diagonal(Hf)), -g[idx])
            if x is not None and bool(torch.isfinite(x).all()):
                delta[idx] = x
        cand = mm(expm(delta.view(V, 3)), dR)
        Ed_c, _, failed, g_c, H_c = pr.system(cand)
        E_c = Ed_c + pr.prior(cand)
        if not failed and bool(E_c < E):
            dR, E, Ed, g, H, steps = cand, E_c, Ed_c, g_c, H_c, steps + 1
            mu = max(mu * MU_DOWN, MU_MIN)
        else:
            mu = min(mu * MU_UP, MU_MAX)
        costs.append(float(Ed / wsum))
    out.update(rotation=logm(dR), matrix=dR.float(), cost0=cost0, cost=Ed / wsum, pairs=pr.pairs, steps=steps,
               grad=g[idx].abs().max() if len(idx) else zero, valid=True, costs=costs, dR=dR)
    return out


def stationarity(pr, matrix):
    """The solver-independent check, at the rotation the returned fp32 matrices encode (`pr` in float64): -> (the largest |g_i| /
    allowed_i over the free components, g, allowed, free) with allowed_i = MARGIN * sum_k |H_ik| * ulp32(1.0), k over the free
    components: the matrices are rounded at the scale of 1, which moves the rotation by up to an ulp a component."""
    g, H = pr.grad_hess(matrix.double())
    free = pr.free
    allowed = MARGIN * (H.abs() * free.unsqueeze(0)).sum(1) * FS.ulp32(1.0)
    if not bool(free.any()):
        return 0.0, g, allowed, free
    ratio = float((g.abs()[free] / allowed[free]).max())
    return ratio, g, allowed, free


# --------------------------------------------------------------------------- scenes and cases

def _clip(cams, rec, rw, tilt, B, J, noise, g):
    V = len(cams)
    ctm = FS.random_ctm(B, V, cams, g) if rw else None
    pts = FS.random_points(B, J, g)
    true = apply_correction_f64(tilt, rec, ctm)
    coords = FS.project(pts, rec, true, 1.0 / HM, 1.0 / HM) + noise * torch.randn(B, V, J, 2, generator=g, dtype=torch.float64)
    conf = 0.6 + 0.4 * torch.rand(B, V, J, generator=g, dtype=torch.float64)
    return {"B": B, "V": V, "J": J, "rw": rw, "cams": cams, "rec": rec, "ctm": ctm, "pts": pts, "tilt": tilt, "true": true,
            "coords": coords.float(), "conf": conf.float()}


def scene(B, V, J, rw, ang, noise, seed):
    """A clip seen by a rig whose cameras 1..V-1 are tilted by a random vector with entries in +-ang (rad) against the nominal
    extrinsics: the nominal `ctm` (fp32 (B, V, 4, 4) per frame for rw, None for syn), the true tilts `tilt` (V, 3, 3) float64 and their
    vectors `vec`, the points and their projections through the TRUE cameras (`true`, float64 matrices) with `noise` (heat-map pixels)
    added, as fp32 coords / conf."""
    g = torch.Generator().manual_seed(seed)
    cams = FS.rig()[:V]
    rec = FS.records(cams)
    vec = (torch.rand(V, 3, generator=g, dtype=torch.float64) * 2 - 1) * ang
    vec[0] = 0.0
    sc = _clip(cams, rec, rw, expm(vec), B, J, noise, g)
    sc["vec"] = vec
    return sc


def more_frames(sc, B, seed):
    """Another clip of B frames seen by the same (tilted) rig, noise-free."""
    out = _clip(sc["cams"], sc["rec"], sc["rw"], sc["tilt"], B, sc["J"], 0.0, torch.Generator().manual_seed(seed))
    out["vec"] = sc["vec"]
    return out


def apply_correction_f64(tilt, rec, ctm, nominal_fp32=False):
    """apply_correction without the rounding, of float64 dR: (B | 1, V, 4, 4) float64."""
    V = tilt.shape[0]
    if ctm is None:
        r = rec.double()
        f = torch.where(r[:, 26] != 0, -torch.ones(V, dtype=torch.float64), torch.ones(V, dtype=torch.float64))
        m = torch.zeros(1, V, 4, 4, dtype=torch.float64)
        m[0, :, 0, 0], m[0, :, 1, 1], m[0, :, 2, 2], m[0, :, 3, 3] = f, f, 1.0, 1.0
        m[0, :, :3, 3] = r[:, 27:30] * 0.01
        m = m.float().double() if nominal_fp32 else m
    else:
        m = ctm.double()
    left = torch.zeros(V, 4, 4, dtype=torch.float64)
    left[:, :3, :3], left[:, 3, 3] = tilt, 1.0
    return mm(left.unsqueeze(0), m)


# (B, V, J, rw) of the GPU test
SHAPES = [(6, 4, 15, False), (40, 4, 3, True), (5, 2, 4, False), (3, 3, 2, False), (1, 4, 15, False), (700, 4, 3, False)]
_SCENE_OF = {"calibrated": (0.0, 0.0), "rotated": (0.03, 0.0), "noisy": (0.1, 0.1), "emptied": (0.03, 0.0), "prior": (0.03, 0.0),
             "all_fixed": (0.03, 0.0), "nothing": (0.03, 0.0)}


def case(shape, name, seed=0):
    """(scene, operands) of a case: operands = dict(coords, conf, fixed, prior_weight) - fp32 tensors, never modified afterwards."""
    B, V, J, rw = shape
    ang, noise = _SCENE_OF[name]
    sc = scene(B, V, J, rw, ang, noise, 1000 * seed + 17 * B + 5 * V + J)
    coords, conf = sc["coords"].clone(), sc["conf"].clone()
    fixed, pw = None, 0.0
    if name == "emptied":
        g = torch.Generator().manual_seed(99 + B)
        low = torch.rand(B, V, J, generator=g) < (0.2 if B * J >= 12 else 0.0)    # some views below the threshold
        low[B // 2, V - 1, 0] = True
        low[0, 1:, 0] = True                                              # one pair left with one view
        if B * J > 2:
            low[-1, :, -1] = True                                         # one with none
        conf[low] = 0.3 * conf[low]
        flat = coords.view(-1, 2)
        off, on = torch.nonzero(low.flatten()).flatten(), torch.nonzero(~low.flatten()).flatten()
        flat[off[0], 0], flat[off[-1], 1] = float("nan"), float("inf")    # planted where the view is excluded anyway ...
        flat[on[len(on) // 2], 0] = float("nan")                          # ... and where its confidence says it counts
        if len(on) > 7:
            flat[on[len(on) // 3], 1] = float("-inf")
            conf.view(-1)[on[len(on) // 5]] = float("nan")
    elif name == "prior":
        pw = PRIOR
    elif name == "all_fixed":
        fixed = [True] * V
    elif name == "nothing":
        conf = 0.4 * conf
    return sc, {"coords": coords, "conf": conf, "fixed": fixed, "prior_weight": pw}


def problem(sc, ops, dt):
    ctm = None if sc["ctm"] is None else sc["ctm"].to(dt)
    return Problem(ops["coords"].to(dt), ops["conf"].to(dt), sc["rec"], ctm, ops["fixed"], ops["prior_weight"])


def rms_cm(cost):
    return math.sqrt(max(float(cost), 0.0))

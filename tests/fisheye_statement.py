"""The float64 statements of the fisheye camera math that the 3-D decode kernels are held to, each written once, in
elementwise torch operations: the rig and its ray records, the two polynomial evaluators, the extrinsics, the rays with their normal
equations and distances, the triangulation built from them, one projection in the shape of egr_fisheye.h's `fisheye_pixel`, the bump
renderer and the yardstick.  Every function computes in the dtype of its first operand, so the same code gives the float64 statement and
torch's fp32 evaluation of it.  Not a test module: test_gpu_triangulate.py, test_gpu_volume.py, robust_statement.py,
skeleton_statement.py, the host tests and tools/*_accuracy.py import it.

Which statement passes which polynomial evaluator to `fisheye_pixel`, and why.  The fp32 evaluation of a statement sets its test's
allowance (MARGIN x its own deviation from float64, 4 ulp floor), so the order of a statement's arithmetic is part of the bar:

  power_sum   the kernel's order (egrf::w2c_rho), in `heatmap_coords`: the volume statement (volume_statement.py) and `bumps`, which
              renders every scene's heat maps;
  horner      in `project`: the consensus statement (robust_statement.py) and the scenes' coordinates.

Measured on the CPU when the copies of this code were merged here (the scenes' `project` took atan(-z / norm), without the on-axis
case): over every cached tensor of the five GPU test files - 10 657 leaves - atan2 and the on-axis case change no fp32 bit of a scene
and no bit of a statement, float64 or float32; the only float64 scene tensor that is kept, distractor_scene's `centre`, moves by
1.1e-14 px at the most.  Moving the consensus statement to power_sum, however, moves the fp32 allowance of `score` both ways -
7.64e-6 -> 1.21e-5 for (2, 4, 3, 3, syn) "random", 8.81e-7 -> 4.77e-7 for (1, 2, 1, 4, syn) "projected", 7.34e-6 -> 9.25e-6 for
(2, 4, 2, 3, rw) "emptied" - while its discrete outputs stay and its float64 score moves by 5.1e-15 at the most.  Hence the evaluator
is a parameter and each statement keeps the one it had."""
import math
import os

import numpy as np
import torch

MARGIN = 8.0
THR = 0.5
MIN_DET = 1e-6
HM = 64                                       # heat-map side: coords are pixels of a 64 x 64 map
NAMES = ("camera_front_left", "camera_front_right", "camera_back_left", "camera_back_right")


# --------------------------------------------------------------------------- camera data

def calib_dir():
    import egorear_amd
    return os.path.join(os.path.dirname(os.path.abspath(egorear_amd.__file__)), "calib", "ego4view")


def rig(model="ego4view_syn"):
    from egorear_amd.camera import FishEyeCameraCalibratedModel
    return [FishEyeCameraCalibratedModel(model, calib_dir(), n) for n in NAMES]


def records(cams):
    return torch.from_numpy(np.stack([c.packed_rays() for c in cams]))


def random_points(B, J, g):
    r = torch.rand(B, J, 3, generator=g, dtype=torch.float64)
    return torch.stack((r[..., 0] * 120 - 60, r[..., 1] * 120 - 40, r[..., 2] * 135 + 15), -1)


def random_ctm(B, V, cams, g):
    """Per sample a rotation of at most 0.05 rad about a random axis, composed with each camera's nominal pose; translations in m."""
    ax = torch.randn(B, 3, generator=g, dtype=torch.float64)
    ax = ax / ax.norm(dim=1, keepdim=True)
    ang = (torch.rand(B, generator=g, dtype=torch.float64) - 0.5) * 0.1
    K = torch.zeros(B, 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    rot = torch.eye(3, dtype=torch.float64) + torch.sin(ang).view(B, 1, 1) * K + (1 - torch.cos(ang)).view(B, 1, 1) * (K @ K)
    m = torch.zeros(B, V, 4, 4, dtype=torch.float64)
    for v, cam in enumerate(cams):
        f = -1.0 if cam.flip_xy else 1.0
        m[:, v, :3, :3] = torch.diag(torch.tensor([f, f, 1.0], dtype=torch.float64)) @ rot
        m[:, v, :3, 3] = torch.tensor(cam.offset, dtype=torch.float64) * 0.01
        m[:, v, 3, 3] = 1.0
    return m.float().contiguous()


def per_view(col, like):
    """A per-camera column (V,) shaped to broadcast against `like` (B, V, J, ...)."""
    return col.view((1, -1) + (1,) * (like.dim() - 2))


# --------------------------------------------------------------------------- polynomials: coef (V, n) against x (B, V, J, ...)

def horner(coef, x, n):
    """sum_i coef[..., i] x^i by Horner."""
    acc = torch.zeros_like(x)
    for i in range(n - 1, -1, -1):
        acc = acc * x + per_view(coef[:, i], x)
    return acc


def dhorner(coef, x, n):
    """Its derivative, by Horner."""
    acc = torch.zeros_like(x)
    for i in range(n - 1, 0, -1):
        acc = acc * x + i * per_view(coef[:, i], x)
    return acc


def power_sum(coef, x, n):
    """sum_i coef[..., i] x^i left to right from 0, as egrf::w2c_rho adds it (slots past the degree hold 0)."""
    acc, pw = torch.zeros_like(x), torch.ones_like(x)
    for i in range(n):
        acc = acc + per_view(coef[:, i], x) * pw
        pw = pw * x
    return acc


# --------------------------------------------------------------------------- extrinsics, rays, triangulation

def extrinsics(rec, ctm, dt, trailing=1):
    """R[r][c], t[r] broadcastable to (B, V) + `trailing` more dimensions: p_cam = R p + t in cm.  syn (ctm None): each camera on its
    own, R = diag(f, f, 1)."""
    V = rec.shape[0]
    one = (1,) * trailing
    if ctm is not None:
        m = ctm.to(dt)
        return ([[m[:, :, r, c].view((-1, V) + one) for c in range(3)] for r in range(3)],
                [100.0 * m[:, :, r, 3].view((-1, V) + one) for r in range(3)])
    rec = rec.to(dt)
    f = torch.where(rec[:, 26] != 0, -torch.ones_like(rec[:, 26]), torch.ones_like(rec[:, 26])).view((1, V) + one)
    z, o = torch.zeros_like(f), torch.ones_like(f)
    return [[f, z, z], [z, f, z], [z, z, o]], [rec[:, 27 + r].view((1, V) + one) for r in range(3)]


def rays(coords, conf, rec, ctm, sx, sy, thr, newton=6):
    """coords (B, V, J, 2), conf (B, V, J) in their own dtype; rec (V, 30) = camera.packed_rays(); ctm (B, V, 4, 4) or None -> use
    (B, V, J) bool, w (B, V, J), the directions d[3] in the camera frame by Newton on the W2C polynomial, and the extrinsics R[3][3],
    t[3] (broadcastable to (B, V, J))."""
    dt = coords.dtype
    c = rec.to(dt)
    x, y = coords[..., 0], coords[..., 1]
    use = (conf >= thr) & (conf > 0) & torch.isfinite(conf) & torch.isfinite(x) & torch.isfinite(y)
    zero = torch.zeros_like(conf)
    # (an excluded view weighs 0; its coordinates are replaced by the middle of the image so that 0 * its ray stays finite)
    w, x, y = torch.where(use, conf, zero), torch.where(use, x, zero + 0.5 / sx), torch.where(use, y, zero + 0.5 / sy)
    col = lambda i: per_view(c[:, i], conf)
    dx, dy = x * sx * col(3) - col(1), y * sy * col(4) - col(2)
    rho = torch.sqrt(dx * dx + dy * dy)
    axis = ~(rho >= 1e-4)
    rs = torch.where(axis, torch.ones_like(rho), rho)
    ux, uy = torch.where(axis, zero, dx / rs), torch.where(axis, zero, dy / rs)
    theta = torch.atan(horner(c[:, 18:26], rs, 8) / rs)
    for _ in range(newton):
        theta = theta - (horner(c[:, 5:17], theta, 12) - rs) / dhorner(c[:, 5:17], theta, 12)
    st, ct = torch.where(axis, -torch.ones_like(rho), torch.sin(theta)), torch.where(axis, zero, torch.cos(theta))
    R, t = extrinsics(rec, ctm, dt)
    return use, w, [ux * ct, uy * ct, -st], R, t


def normal_equations(w, d, R, t):
    """A p = b of every joint's weighted rays: A[k, l] (B, J) for l >= k (it is symmetric, bit for bit) and b[k] (B, J)."""
    e = [sum(R[r][k] * d[r] for r in range(3)) for k in range(3)]
    rt = [sum(R[r][k] * t[r] for r in range(3)) for k in range(3)]
    d_t = sum(d[r] * t[r] for r in range(3))
    A = {(k, l): (w * (sum(R[r][k] * R[r][l] for r in range(3)) - e[k] * e[l])).sum(1) for k in range(3) for l in range(k, 3)}
    return A, [-(w * (rt[k] - e[k] * d_t)).sum(1) for k in range(3)]


def ray_dist2(d, R, t, coord):
    """Squared distance of the points whose k-th coordinate (B, J) is coord(k) from every view's ray, (B, V, J).  (coord is called at
    every use: an indexing caller - lambda k: p[..., k] - then gives autograd one node per use, and the order in which p's gradient is
    summed, hence its last bits, rests on that.)"""
    q = [sum(R[r][k] * coord(k).unsqueeze(1) for k in range(3)) + t[r] for r in range(3)]
    dq = sum(d[r] * q[r] for r in range(3))
    return sum((q[r] - d[r] * dq) ** 2 for r in range(3))


def statement(coords, conf, rec, ctm, sx, sy, thr=THR, min_det_ratio=MIN_DET, newton=6):
    """The triangulation: operands as `rays` -> pts (B, J, 3), cost (B, J), resid (B, V, J), ok (B, J) bool; a closed-form symmetric
    solve of the normal equations, no LAPACK call."""
    use, w, d, R, t = rays(coords, conf, rec, ctm, sx, sy, thr, newton)
    A, b = normal_equations(w, d, R, t)
    a00, a01, a02, a11, a12, a22 = A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]
    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    det = a00 * c00 + a01 * c01 + a02 * c02
    tr3 = (a00 + a11 + a22) / 3
    ok = ((w > 0).sum(1) >= 2) & (det > min_det_ratio * tr3 * tr3 * tr3)
    ds = torch.where(ok, det, torch.ones_like(det))
    zj = torch.zeros_like(det)
    p = [torch.where(ok, (c00 * b[0] + c01 * b[1] + c02 * b[2]) / ds, zj), torch.where(ok, (c01 * b[0] + c11 * b[1] + c12 * b[2]) / ds, zj),
         torch.where(ok, (c02 * b[0] + c12 * b[1] + c22 * b[2]) / ds, zj)]
    rr = ray_dist2(d, R, t, lambda k: p[k])
    keep = use & ok.unsqueeze(1)
    wsum = torch.where(ok, w.sum(1), torch.ones_like(det))
    cost = torch.where(ok, (w * rr).sum(1) / wsum, zj)
    resid = torch.sqrt(torch.where(keep, rr, torch.zeros_like(rr)))
    return torch.stack(p, -1), cost, resid, ok


# --------------------------------------------------------------------------- the projection

def fisheye_pixel(p, rec, ctm, poly):
    """egr_fisheye.h's fisheye_pixel behind the extrinsics, un-chained and unclamped: device-frame points p (B, 1 | V, J, ..., 3), cm, in
    their own dtype -> image pixels x, y (B, V, J, ...) and `take`, false where the view gives no pixel (the camera centre and the
    optical axis behind it).  On the axis the direction counts as (0, 0).  `poly` evaluates the W2C polynomial: horner or power_sum."""
    dt = p.dtype
    c = rec.to(dt)
    R, t = extrinsics(rec, ctm, dt, p.dim() - 3)
    q = [sum(R[r][k] * p[..., k] for k in range(3)) + t[r] for r in range(3)]
    n = torch.sqrt(q[0] * q[0] + q[1] * q[1])
    rho = poly(c[:, 5:17], torch.atan2(-q[2], n), 12)
    on_axis = n == 0
    ns = torch.where(on_axis, torch.ones_like(n), n)
    ex, ey = torch.where(on_axis, torch.zeros_like(n), q[0] / ns), torch.where(on_axis, torch.zeros_like(n), q[1] / ns)
    return ex * rho + per_view(c[:, 1], n), ey * rho + per_view(c[:, 2], n), ~(on_axis & (q[2] <= 0))


def project(pts, rec, ctm, sx=1.0, sy=1.0):
    """world2camera_pytorch for one camera at a time, by Horner: pts (B, J, 3) cm in their own dtype -> (B, V, J, 2) in coords units,
    image pixels / (sx W_img): the normalised image points as it stands, pixels of an (H, W) map with sx, sy = 1 / W, 1 / H."""
    x, y, _ = fisheye_pixel(pts.unsqueeze(1), rec, ctm, horner)
    c = rec.to(pts.dtype)
    return torch.stack((x / (sx * per_view(c[:, 3], x)), y / (sy * per_view(c[:, 4], x))), -1)


def heatmap_coords(p, rec, ctm, H, W):
    """The kernels' order (power_sum): p (B, 1 | V, J, N, 3) -> heat-map coordinates x, y (B, V, J, N) of an (H, W) map and `take`."""
    x, y, take = fisheye_pixel(p, rec, ctm, power_sum)
    c = rec.to(p.dtype)
    return x * W / per_view(c[:, 3], x), y * H / per_view(c[:, 4], x), take


# --------------------------------------------------------------------------- scenes and the yardstick

def render(x, y, H, W):
    """Gaussian bumps (sigma 1 heat-map pixel) centred at x, y (any shape, float64) -> that shape + (H, W)."""
    xs, ys = torch.arange(W, dtype=torch.float64), torch.arange(H, dtype=torch.float64).view(H, 1)
    return torch.exp(-((xs - x[..., None, None]) ** 2 + (ys - y[..., None, None]) ** 2) / 2.0)


def bumps(pts, rec, ctm, H, W, height=1.0):
    """Bumps of `height` at the projections of pts (B, J, 3), float64 (B, V, J, H, W)."""
    x, y, _ = heatmap_coords(pts.double().unsqueeze(1).unsqueeze(3), rec, None if ctm is None else ctm.double(), H, W)
    return height * render(x.squeeze(-1), y.squeeze(-1), H, W)


def soft_argmax_statement(hm, beta):
    """softmax(beta h)-weighted mean (x, y) and the maximum of maps (..., H, W), in hm's dtype."""
    H, W = hm.shape[-2:]
    p = torch.softmax((hm * beta).reshape(hm.shape[:-2] + (H * W,)), dim=-1).reshape(hm.shape)
    x = (p.sum(-2) * torch.arange(W, dtype=hm.dtype)).sum(-1)
    y = (p.sum(-1) * torch.arange(H, dtype=hm.dtype)).sum(-1)
    return torch.stack((x, y), -1), hm.reshape(hm.shape[:-2] + (H * W,)).max(-1)[0]


def ulp32(m):
    return 0.0 if m == 0.0 else 2.0 ** (math.floor(math.log2(m)) - 23)


def yardstick(what, got, f32, f64, shape_own=None):
    """(HIP deviation, allowed deviation) of one output against the float64 statement: at most MARGIN x the deviation of torch's fp32
    evaluation of that statement - of this case, or `shape_own`, the largest over the cases of one shape - with a floor of 4 ulp (fp32)
    of the output's largest magnitude.  Prints the figures of this case."""
    f64 = f64.double()
    err, own = float((got.double().cpu() - f64).abs().max()), float((f32.double() - f64).abs().max())
    floor = 4.0 * ulp32(float(f64.abs().max()))
    of_shape = "" if shape_own is None else f" (largest of the shape's cases {shape_own:.3e})"
    print(f"    {what}: |hip - f64| {err:.3e}, |torch fp32 - f64| {own:.3e}{of_shape}, ratio {err / own if own else float('inf'):.3g}, "
          f"4 ulp floor {floor:.3e}, largest entry {float(f64.abs().max()):.4g}")
    return err, max(MARGIN * (own if shape_own is None else shape_own), floor)

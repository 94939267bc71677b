"""Float64 statement of the volumetric fusion (egr_volume_fuse_f32), DESIGN.md 5o, in elementwise torch operations with a gather for the
bilinear corners: voxel centres, the un-chained fisheye projection in the kernel's order (fisheye_statement.heatmap_coords), zero-padded
bilinear samples, the weighted fusion of the views and one 3-D soft-argmax.  It computes in the dtype of `hm`, so the same code gives
the float64 statement and torch's fp32 evaluation of it.  Shared by test_gpu_volume.py and tools/volume_accuracy.py."""
import torch

from fisheye_statement import heatmap_coords


def offsets(G, cube, dt):
    """o_i (N, 3) of voxel i = (iz * G + iy) * G + ix."""
    k = ((torch.arange(G, dtype=dt) + 0.5) / G - 0.5) * cube
    return torch.stack((k.repeat(G * G), k.repeat_interleave(G).repeat(G), k.repeat_interleave(G * G)), -1)


def statement(hm, conf, centers, rec, ctm, G, cube, beta, thr, center_ok=None):
    """hm (B, V, J, H, W), conf (B, V, J), centers (B, J, 3) in hm's dtype (float64 or float32); rec (V, 30) = camera.packed_rays(); ctm
    (B, V, 4, 4) or None -> dict(pose (B, J, 3), peak, index, spread, valid (B, J), S (B, J, N), partial = share of the voxel-view
    samples that miss at least one corner)."""
    dt = hm.dtype
    B, V, J, H, W = hm.shape
    zero = torch.zeros_like(conf)
    use = (conf >= thr) & (conf > 0) & torch.isfinite(conf)
    w = torch.where(use, conf, zero)
    valid = (use.sum(1) >= 2) & torch.isfinite(centers).all(-1)
    if center_ok is not None:
        valid = valid & center_ok.bool()
    c = torch.where(valid.unsqueeze(-1), centers, torch.zeros_like(centers))
    o = offsets(G, cube, dt)
    p = c.view(B, 1, J, 1, 3) + o
    x, y, take = heatmap_coords(p, rec, ctm, H, W)
    inside = take & (x > -1) & (x < W) & (y > -1) & (y < H)                    # (a NaN fails every comparison)
    xs, ys = torch.where(inside, x, torch.zeros_like(x)), torch.where(inside, y, torch.zeros_like(y))
    xf, yf = torch.floor(xs), torch.floor(ys)
    fx, fy = xs - xf, ys - yf
    x0, y0 = xf.long(), yf.long()
    flat = hm.reshape(B, V, J, H * W)
    corner, whole = {}, inside.clone()
    for dx in (0, 1):
        for dy in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            there = inside & (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)
            whole = whole & there
            got = torch.gather(flat, -1, yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1))
            corner[dx, dy] = torch.where(there, got, torch.zeros_like(got))       # a corner outside the map counts 0
    top = corner[0, 0] + fx * (corner[1, 0] - corner[0, 0])
    bot = corner[0, 1] + fx * (corner[1, 1] - corner[0, 1])
    s = top + fy * (bot - top)                                                     # (B, V, J, N)
    wsum = torch.where(valid, w.sum(1), torch.ones_like(w.sum(1)))
    S = (w.unsqueeze(-1) * s).sum(1) / wsum.unsqueeze(-1)                          # (B, J, N)
    peak, index = S.max(-1)                                                        # (the first of equal maxima)
    P = torch.softmax(beta * S, -1)
    off = (P.unsqueeze(-1) * o).sum(-2)
    spread = torch.sqrt((P * ((o - off.unsqueeze(-2)) ** 2).sum(-1)).sum(-1))
    zj = torch.zeros_like(peak)
    return {"pose": torch.where(valid.unsqueeze(-1), c + off, torch.zeros_like(off)), "peak": torch.where(valid, peak, zj),
            "index": torch.where(valid, index, torch.full_like(index, -1)), "spread": torch.where(valid, spread, zj), "valid": valid,
            "S": S.detach(), "partial": float((inside & ~whole)[use].float().mean()) if bool(use.any()) else 0.0,
            "sampled": float(whole[use].float().mean()) if bool(use.any()) else 0.0}

"""Evaluation metrics on the device.

Pose: mirrors the reference's `evaluate_pose` (pl_wrappers/egoposeformer/pose_3d_mvf_ex.py:317-333) and the helpers it
calls (utils/loss.py:9-48, models/utils/pose_metric.py:104-167) — same names, same units — but as ONE HIP kernel
on the device tensors, instead of a device-to-host copy and a Python loop of numpy SVDs.

Heat maps: `heatmap_metrics` / `evaluate_heatmap` mirror the `evaluate` of the two heat-map wrappers
(pl_wrappers/egoposeformer/heatmap.py:220-254, heatmap_mvf_ex.py:263-316) and `evaluate_heatmap` of pose_3d_mvf_ex.py:335-361 —
per-sample L1 error, L1 error where the ground truth is positive, MSE of the maps, MSE of the arg-max points under the ground
truth's validity mask — as one pass over the maps (`egr_heatmap_metrics_f32`: every predicted set and view group in one call,
fp64 sums in a fixed order), instead of a per-sample loop with boolean indexing and one device-to-host copy per sample.
`egorear_amd.evaluate` builds the wrappers' validation / test steps on top of both."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Optional, Sequence, Union

import torch

from . import hip

CM2MM = 10.0


def pose_metrics(pred_pose: torch.Tensor, gt_pose: torch.Tensor, pck_threshold_mm: float = 150.0, n_auc: int = 31,
                 return_aligned: bool = False):
    """pred_pose, gt_pose (B, J, 3) in cm on the device -> (B, 4) fp32 [mpjpe_mm, pa_mpjpe_mm, pck_3d %, auc_3d %]."""
    if not pred_pose.is_cuda:
        raise RuntimeError("egorear_amd.metrics: device tensors expected (no CPU path)")
    pred = pred_pose.detach().to(torch.float32).contiguous()
    gt = gt_pose.detach().to(device=pred.device, dtype=torch.float32).contiguous()   # the dataset yields float64 gt
    if pred.shape != gt.shape or pred.dim() != 3 or pred.shape[-1] != 3:
        raise RuntimeError("egorear_amd.metrics: pred / gt must both be (B, J, 3)")
    B, J = pred.shape[:2]
    out = torch.empty((B, 4), device=pred.device, dtype=torch.float32)
    aligned = torch.empty_like(pred) if return_aligned else None
    hip._launch("egr_pose_metrics_f32", hip.lib.egr_pose_metrics_f32, hip._p(pred), hip._p(gt), B, J, float(pck_threshold_mm), n_auc,
                hip._p(out), hip._p(aligned), hip._stream())
    return (out, aligned) if return_aligned else out


def compute_mpjpe_batch(pred_keypoints: torch.Tensor, gt_keypoints: torch.Tensor) -> torch.Tensor:
    """utils/loss.py:9-12 (result in the inputs' unit: cm)."""
    return pose_metrics(pred_keypoints, gt_keypoints)[:, 0] / CM2MM


def evaluate_pose(pred_pose: torch.Tensor, gt_pose: torch.Tensor, prefix: str) -> "OrderedDict[str, torch.Tensor]":
    """Same keys and units as the reference's evaluate_pose; values stay on the device."""
    m = pose_metrics(pred_pose, gt_pose)
    out = OrderedDict()
    out[prefix + "_mpjpe"] = m[:, 0]
    out[prefix + "_pa_mpjpe"] = m[:, 1]
    out[prefix + "_pck_3d"] = m[:, 2]
    out[prefix + "_auc_3d"] = m[:, 3]
    return out


# --------------------------------------------------------------------------- heat-map metrics

MAX_SETS, MAX_GROUPS = 4, 8      # EGR_HM_MAX_SETS / EGR_HM_MAX_GROUPS of include/egorear_hip.h


def heatmap_metrics(pred_sets: Union[torch.Tensor, Sequence[torch.Tensor]], gt: torch.Tensor,
                    view_groups: Optional[Sequence[Sequence[int]]] = None, threshold: float = 1.0) -> dict:
    """One launch for S predicted sets (a tensor or a list of up to 4), each (B, V, J, H, W) fp32 contiguous on the device, one
    ground truth of the same shape (float64 is cast) and G view groups [v0, v1) (None: one group of all views).  Raw device tensors:
        l1, pos_l1 (S, G, B) fp32; mse, mse_pts2d (S, G) fp32                       - the reference's four quantities
        argmax (S + 1, B, V, J) int32, maxval (S + 1, B, V, J) fp32: first maximum per map, the last row is the ground truth's;
        valid (B, V, J) uint8 = [max(gt) >= threshold]; partials (S, B*V*J, 3) fp64 - the per-map sums behind the above.
    Nothing synchronises: the call can be captured into a hipGraph."""
    sets = [pred_sets] if isinstance(pred_sets, torch.Tensor) else list(pred_sets)
    if not sets or not all(isinstance(t, torch.Tensor) for t in sets):
        raise RuntimeError("egorear_amd.metrics.heatmap_metrics: a tensor or a non-empty list of tensors expected")
    if not all(t.is_cuda for t in sets) or not gt.is_cuda:
        raise RuntimeError("egorear_amd.metrics: device tensors expected (no CPU path)")
    p0 = sets[0]
    if p0.dim() != 5 or any(t.shape != p0.shape for t in sets) or gt.shape != p0.shape:
        raise RuntimeError("egorear_amd.metrics.heatmap_metrics: every predicted set and gt must share one (B, V, J, H, W) shape")
    B, V, J, H, W = (int(d) for d in p0.shape)
    S = len(sets)
    groups = [(0, V)] if view_groups is None else [(int(a), int(b)) for a, b in view_groups]
    if S > MAX_SETS or not 1 <= len(groups) <= MAX_GROUPS or any(not 0 <= a < b <= V for a, b in groups):
        raise RuntimeError(f"egorear_amd.metrics.heatmap_metrics: at most {MAX_SETS} sets and {MAX_GROUPS} non-empty view groups inside [0, {V})")
    sets = [hip._cont(t.detach(), "a predicted heat-map set") for t in sets]
    g = gt.detach()
    if g.dtype == torch.float64:         # the dataset yields float64 ground truth
        g = g.to(torch.float32)
    g = hip._cont(g, "the ground-truth heat maps")
    dev, G, maps = p0.device, len(groups), B * V * J
    out = {"l1": torch.empty((S, G, B), device=dev, dtype=torch.float32), "pos_l1": torch.empty((S, G, B), device=dev, dtype=torch.float32),
           "mse": torch.empty((S, G), device=dev, dtype=torch.float32), "mse_pts2d": torch.empty((S, G), device=dev, dtype=torch.float32),
           "argmax": torch.empty((S + 1, B, V, J), device=dev, dtype=torch.int32), "maxval": torch.empty((S + 1, B, V, J), device=dev, dtype=torch.float32),
           "valid": torch.empty((B, V, J), device=dev, dtype=torch.uint8), "partials": torch.empty((S, maps, 3), device=dev, dtype=torch.float64)}
    ptrs = (C.c_void_p * S)(*[hip._p(t) for t in sets])
    vg = (C.c_int32 * (2 * G))(*[x for ab in groups for x in ab])
    hip._launch("egr_heatmap_metrics_f32", hip.lib.egr_heatmap_metrics_f32, ptrs, S, hip._p(g), B, V, J, H, W, vg, G, float(threshold),
                hip._p(out["partials"], torch.float64), hip._p(out["argmax"], torch.int32), hip._p(out["maxval"]),
                hip._p(out["valid"], torch.uint8), hip._p(out["l1"]), hip._p(out["pos_l1"]), hip._p(out["mse"]), hip._p(out["mse_pts2d"]),
                hip._stream(), nbytes=4.0 * (S + 1) * maps * H * W)
    return out


def heatmap_dict(raw: dict, s: int, g: int, prefix: str, full: bool = True) -> "OrderedDict[str, torch.Tensor]":
    """Set `s`, view group `g` of a `heatmap_metrics` result under the reference's key names, in its order."""
    out = OrderedDict()
    out[prefix + "_l1_error_heatmap"] = raw["l1"][s, g]
    out[prefix + "_pos_l1_error_heatmap"] = raw["pos_l1"][s, g]
    if full:
        out[prefix + "_mse_heatmap"] = raw["mse"][s, g]
        out[prefix + "_mse_pts2d"] = raw["mse_pts2d"][s, g]
    return out


def evaluate_heatmap(pred_heatmap: torch.Tensor, gt_heatmap: torch.Tensor, prefix: str, full: bool = True) -> "OrderedDict[str, torch.Tensor]":
    """Same keys, order and shapes as the wrappers' `evaluate` (heatmap.py:220-254, heatmap_mvf_ex.py:263-316); full=False: the
    two-key `evaluate_heatmap` of pose_3d_mvf_ex.py:335-361.  Values stay on the device: (B,), (B,), (), ().  View slices as the
    wrappers pass them (`pred[:, 0:2]`) are accepted (copied dense); `heatmap_metrics(..., view_groups=...)` evaluates several
    slices and sets in one launch without those copies."""
    if not pred_heatmap.is_cuda or not gt_heatmap.is_cuda:
        raise RuntimeError("egorear_amd.metrics: device tensors expected (no CPU path)")
    return heatmap_dict(heatmap_metrics(pred_heatmap.detach().contiguous(), gt_heatmap.detach().contiguous()), 0, 0, prefix, full)


# --------------------------------------------------------------------------- GT heat maps

def _gauss_table(sigma: float):
    """The reference's window, computed as it computes it (generate_heatmap.py:33-37): float32 numpy."""
    import numpy as np
    tmp_size = sigma * 3
    size = 2 * tmp_size + 1
    x = np.arange(0, size, 1, np.float32)
    y = x[:, np.newaxis]
    x0 = y0 = size // 2
    g = np.exp(-((x - x0) ** 2 + (y - y0) ** 2) / (2 * sigma ** 2))
    return int(tmp_size), np.ascontiguousarray(g.astype(np.float32))


def generate_target(joints: torch.Tensor, image_size: int = 872, heatmap_size: int = 64, sigma: float = 1.0) -> torch.Tensor:
    """generate_heatmap.py:10-48 on the device: joints (..., J, 2) pixel coordinates (any float dtype, device tensor)
    -> (..., J, heatmap_size, heatmap_size) fp32."""
    if not joints.is_cuda:
        raise RuntimeError("egorear_amd.metrics.generate_target: device tensor expected (no CPU path)")
    j64 = joints.detach().to(torch.float64).contiguous()
    lead = tuple(j64.shape[:-1])
    maps = j64.numel() // 2
    tmp, g = _gauss_table(sigma)
    gt = torch.from_numpy(g).to(joints.device)
    out = torch.empty(lead + (heatmap_size, heatmap_size), device=joints.device, dtype=torch.float32)
    hip._launch("egr_gt_heatmap_f32", hip.lib.egr_gt_heatmap_f32, hip._p(j64, torch.float64), maps, float(image_size), heatmap_size, tmp,
                hip._p(gt), hip._p(out), hip._stream())
    return out

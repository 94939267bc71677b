"""Soft-argmax decoding of heat maps on MI355X: sub-pixel 2-D joints with a confidence, differentiable.

The reference ships this only as library functions - `get_max_preds_soft_pytorch` (pose_estimation/utils/loss.py:145-177, which calls
`torch.cuda.comm.broadcast` with `torch.cuda.FloatTensor` and so cannot run on this stack as written) and `integrate_tensor_2d`
(pose_estimation/utils/util.py:80-109).  This module offers both under their names, signatures and return shapes on top of
`egr_soft_argmax_f32` / `egr_soft_argmax_bwd_f32` (include/egorear_hip.h), plus `decode_joints_2d`, the serving-side call
that returns the soft and the hard decode of (B, V, J, H, W) maps from ONE launch.

The kernels are wrapped as `torch.library` operators (`egorear_amd::soft_argmax`, `egorear_amd::soft_argmax_bwd`) with fake
implementations and a registered autograd formula, like `egorear_amd::msda_fwd`: gradient flows to the heat maps from the coordinates
and from `maxvals`; `index`, `valid` and the probabilities are not differentiable.  There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import torch

from . import hip

MODE_SOFTMAX, MODE_RELU = 0, 1


def _aligned(t: torch.Tensor) -> torch.Tensor:
    # (the register path needs 16-byte aligned maps; which path runs then depends on the shape alone, and so do the result's last bits)
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _check(hm: torch.Tensor, beta: float, mode: int, dims: Optional[int] = None, what: str = "soft_argmax"):
    """Shape / dtype / parameter errors, raised before anything is launched (and by the fake implementations)."""
    if dims is not None and hm.dim() != dims:
        raise ValueError(f"egorear_amd.decode.{what}: heat maps must be {dims}-dimensional, got {tuple(hm.shape)}")
    if hm.dim() < 2:
        raise ValueError(f"egorear_amd.decode.{what}: heat maps must be (..., H, W), got {tuple(hm.shape)}")
    if hm.dtype != torch.float32:
        raise ValueError(f"egorear_amd.decode.{what}: float32 heat maps expected, got {hm.dtype}")
    H, W = int(hm.shape[-2]), int(hm.shape[-1])
    if hm.numel() == 0 or H * W >= 1 << 24:
        raise ValueError(f"egorear_amd.decode.{what}: maps must hold between 1 and 2^24 - 1 elements, got {tuple(hm.shape)}")
    if mode not in (MODE_SOFTMAX, MODE_RELU):
        raise ValueError(f"egorear_amd.decode.{what}: mode must be 0 (softmax) or 1 (relu mass), got {mode!r}")
    if not (beta > 0.0 and math.isfinite(beta)):
        raise ValueError(f"egorear_amd.decode.{what}: beta must be a positive finite number, got {beta!r}")
    return tuple(hm.shape[:-2]), H, W


def _on_device(t: torch.Tensor, what: str):
    if not t.is_cuda and t.device.type != "meta":
        raise RuntimeError(f"egorear_amd.decode.{what}: no CPU path - tensors must live on the HIP device")


# ---- the operators ----------------------------------------------------------------------------------------------------------------

@torch.library.custom_op("egorear_amd::soft_argmax", mutates_args=(), device_types="cuda")
def soft_argmax_op(hm: torch.Tensor, beta: float, mode: int, normalize: bool, threshold: float, want_probs: bool
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(coords (..., 2), maxvals (...), index (...) int32, valid (...) uint8, stat (..., 2), probs (..., H, W) - or (0,) when not wanted)."""
    lead, H, W = _check(hm, beta, mode)
    coords, maxvals, index, valid, stat, probs = hip.soft_argmax(_aligned(hm), beta, mode, normalize, threshold, want_probs)
    return (coords.view(lead + (2,)), maxvals.view(lead), index.view(lead), valid.view(lead), stat.view(lead + (2,)),
            probs.view(hm.shape) if want_probs else hm.new_empty((0,)))


@soft_argmax_op.register_fake
def _soft_argmax_fake(hm, beta, mode, normalize, threshold, want_probs):
    lead, H, W = _check(hm, beta, mode)
    return (hm.new_empty(lead + (2,)), hm.new_empty(lead), hm.new_empty(lead, dtype=torch.int32), hm.new_empty(lead, dtype=torch.uint8),
            hm.new_empty(lead + (2,)), hm.new_empty(hm.shape if want_probs else (0,)))


@torch.library.custom_op("egorear_amd::soft_argmax_bwd", mutates_args=(), device_types="cuda")
def soft_argmax_bwd_op(hm: torch.Tensor, stat: torch.Tensor, coords: torch.Tensor, index: torch.Tensor, g_coords: torch.Tensor,
                       g_maxvals: Optional[torch.Tensor], beta: float, mode: int, normalize: bool) -> torch.Tensor:
    _check(hm, beta, mode, what="soft_argmax_bwd")
    gm = None if g_maxvals is None else g_maxvals.to(torch.float32).contiguous()
    return hip.soft_argmax_bwd(_aligned(hm), stat.contiguous(), coords.contiguous(), index.contiguous(),
                               g_coords.to(torch.float32).contiguous(), gm, beta, mode, normalize)


@soft_argmax_bwd_op.register_fake
def _soft_argmax_bwd_fake(hm, stat, coords, index, g_coords, g_maxvals, beta, mode, normalize):
    lead, H, W = _check(hm, beta, mode, what="soft_argmax_bwd")
    if tuple(g_coords.shape) != lead + (2,) or (g_maxvals is not None and tuple(g_maxvals.shape) != lead):
        raise ValueError(f"egorear_amd.decode.soft_argmax_bwd: g_coords must be {lead + (2,)} and g_maxvals {lead}")
    return hm.new_empty(hm.shape)


def _setup_context(ctx, inputs, output):
    hm, beta, mode, normalize, _, _ = inputs
    coords, _, index, _, stat, _ = output
    ctx.save_for_backward(hm, stat, coords, index)
    ctx.args = (beta, mode, normalize)


def _autograd(ctx, g_coords, g_maxvals, g_index, g_valid, g_stat, g_probs):
    hm, stat, coords, index = ctx.saved_tensors
    if g_coords is None:
        g_coords = torch.zeros_like(coords)
    beta, mode, normalize = ctx.args
    return soft_argmax_bwd_op(hm, stat, coords, index, g_coords, g_maxvals, beta, mode, normalize), None, None, None, None, None


soft_argmax_op.register_autograd(_autograd, setup_context=_setup_context)


# ---- the reference's functions ----------------------------------------------------------------------------------------------------

def get_max_preds_soft(batch_heatmaps: torch.Tensor, normalize: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """`get_max_preds_soft_pytorch` (utils/loss.py:145-177): batch_heatmaps (B, J, H, W) -> preds (B, J, 2) = softmax-weighted mean
    (x, y) of each map (beta 1; divided by (W, H) with `normalize`), maxvals (B, J, 1) = the maps' maxima.  Both differentiable."""
    _check(batch_heatmaps, 1.0, MODE_SOFTMAX, dims=4, what="get_max_preds_soft")
    _on_device(batch_heatmaps, "get_max_preds_soft")
    coords, maxvals, _, _, _, _ = soft_argmax_op(batch_heatmaps, 1.0, MODE_SOFTMAX, bool(normalize), 0.0, False)
    return coords, maxvals.unsqueeze(-1)


def integrate_tensor_2d(heatmaps: torch.Tensor, softmax: bool = True, multiplier: float = 100.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """`integrate_tensor_2d` (utils/util.py:80-109): heatmaps (B, J, H, W) -> coordinates (B, J, 2) in heat-map pixels, (x, y), and
    the weights they were taken with, (B, J, H, W): softmax(multiplier * h) over a map, or relu(multiplier * h) with `softmax=False`
    (where the coordinates divide by the map's mass; a map without positive mass gives NaN, as there - its gradient is zero here,
    NaN there).  The second value is returned detached: gradient flows through the coordinates only."""
    mode = MODE_SOFTMAX if softmax else MODE_RELU
    _check(heatmaps, float(multiplier), mode, dims=4, what="integrate_tensor_2d")
    _on_device(heatmaps, "integrate_tensor_2d")
    coords, _, _, _, _, probs = soft_argmax_op(heatmaps, float(multiplier), mode, False, 0.0, True)
    return coords, probs.detach()


class Joints2D(NamedTuple):
    soft: torch.Tensor      # (B, V, J, 2) soft-argmax (x, y), heat-map pixels
    hard: torch.Tensor      # (B, V, J, 2) first-maximum (x, y), heat-map pixels
    maxvals: torch.Tensor   # (B, V, J) the maps' maxima: the confidence
    valid: torch.Tensor     # (B, V, J) bool, maxvals >= threshold


def decode_joints_2d(heatmaps: torch.Tensor, beta: float = 100.0, threshold: float = 0.5) -> Joints2D:
    """heatmaps (B, V, J, H, W) -> Joints2D(soft, hard, maxvals, valid): sub-pixel joints (softmax at `beta`) next to the hard arg-max
    the anchors use, from one read of the maps (one launch; the hard (x, y) are two integer ops on its `index` output)."""
    _check(heatmaps, float(beta), MODE_SOFTMAX, dims=5, what="decode_joints_2d")
    _on_device(heatmaps, "decode_joints_2d")
    W = int(heatmaps.shape[-1])
    soft, maxvals, index, valid, _, _ = soft_argmax_op(heatmaps, float(beta), MODE_SOFTMAX, False, float(threshold), False)
    hard = torch.stack((index % W, torch.div(index, W, rounding_mode="floor")), -1).to(torch.float32)
    return Joints2D(soft, hard, maxvals, valid.view(torch.bool))     # (0 / 1 bytes: a reinterpretation, not a copy)

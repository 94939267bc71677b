"""Soft-argmax decoding of heat maps on MI355X: sub-pixel 2-D joints with a confidence, differentiable.

The reference ships this only as library functions - `get_max_preds_soft_pytorch` (pose_estimation/utils/loss.py:145-177, which calls
`torch.cuda.comm.broadcast` with `torch.cuda.FloatTensor` and so cannot run on this stack as written) and `integrate_tensor_2d`
(pose_estimation/utils/util.py:80-109).  This module offers both under their names, signatures and return shapes on top of
`egr_soft_argmax_f32` / `egr_soft_argmax_bwd_f32` (include/egorear_hip.h), plus `decode_joints_2d`, the serving-side call
that returns the soft and the hard decode of (B, V, J, H, W) maps from ONE launch.

The kernels are wrapped as `torch.library` operators (`egorear_amd::soft_argmax`, `egorear_amd::soft_argmax_bwd`) with fake
implementations and a registered autograd formula, like `egorear_amd::msda_fwd`: gradient flows to the heat maps from the coordinates
and from `maxvals`; `index`, `valid` and the probabilities are not differentiable.  There is no CPU path: CPU tensors raise.

`triangulate_joints` takes the decoded joints of 2 to 4 calibrated fisheye views to one 3-D point per joint (cm, device frame) on
`egr_triangulate_f32` / `egr_triangulate_bwd_f32` - operators `egorear_amd::triangulate`, `egorear_amd::triangulate_bwd`,
differentiable in the point and the cost with respect to the coordinates and the confidences - and `decode_joints_3d` chains the two
launches: heat maps -> Joints2D -> Joints3D, with no torch arithmetic in between.

`fuse_joints_volumetric` lets the views meet before the arg-max: a voxel cube around a coarse centre per joint, every voxel centre
projected into every camera, the heat maps sampled there, the samples fused with the views' weights and one 3-D soft-argmax taken, on
`egr_volume_fuse_f32` / `egr_volume_fuse_bwd_f32` - operators `egorear_amd::volume_fuse`, `egorear_amd::volume_fuse_bwd`,
differentiable in the pose and the peak score with respect to the heat maps of all views jointly (the centres and the confidences are
constants) - and `decode_joints_3d_volumetric` chains three launches: heat maps -> Joints2D -> Joints3D -> Volume3D around its pose.

`find_peaks_2d` keeps the K best local maxima of every map instead of its global one, `select_consistent` picks per joint the
candidates the views agree on - every two-view pair of candidates is triangulated and scored by how well the views' candidates
support its reprojections - on `egr_peaks_f32` / `egr_consensus_f32`, operators `egorear_amd::find_peaks`,
`egorear_amd::consensus`, neither differentiable - and `decode_joints_3d_robust` chains three launches: heat maps -> Peaks2D ->
Consensus -> Joints3D of the accepted views, so that one view firing on a second mode is out-voted instead of bending the pose.

`fit_skeleton` treats the joints of a frame as a skeleton: the rays' distances plus a bone-length term along the kinematic tree plus
an optional prior, minimised by Levenberg-Marquardt on `egr_skeleton_fit_f32`, operator `egorear_amd::skeleton_fit` - a
joint only one camera sees is placed by its ray and its bone.  `estimate_bone_lengths` (`egorear_amd::bone_lengths`) measures the bones
of a clip, `resize_skeleton` (`egorear_amd::skeleton_resize`) is the reference's rescale along the chain, and
`decode_joints_3d_skeleton` chains heat maps -> Joints2D -> Joints3D -> Skeleton3D.  None of them is differentiable.

`smooth_trajectory` is the time axis: per joint of a clip a penalised least-squares track over the frames - the observations, a
velocity and an acceleration penalty - on `egr_trajectory_smooth_f32` / `egr_trajectory_smooth_bwd_f32`, operators
`egorear_amd::trajectory_smooth`, `egorear_amd::trajectory_smooth_bwd`: it fills the frames the triangulation gave up, optionally
down-weights single-frame glitches by Huber reweighting, and is differentiable in its plain form with respect to the poses and their
weights.  `decode_clip_3d` chains heat maps of a clip -> Joints3D per frame -> Track3D, three launches.

`refine_rig` calibrates the rig itself: from the decoded joints of a clip, per camera the rotation about its own centre that makes the
views' rays meet best, by Levenberg-Marquardt on `egr_rig_refine_f32`, operator `egorear_amd::rig_refine`, not
differentiable.  Its `coord_trans_mat` goes to every function above in place of the given one; `apply_rig_correction` composes a fitted
correction with another clip's matrices, and `calibrate_rig` chains heat maps -> Joints2D -> RigFit.

`fit_ray_tracks` is the triangulation and the smoother as one problem: per joint of a clip the track closest to the views' rays over
the frames under the same penalties, on `egr_ray_track_f32`, operator `egorear_amd::ray_track`, not differentiable - a
frame one camera sees contributes its ray instead of being a gap, and the Huber form down-weights one bad view of a frame, not the
frame.  `decode_clip_3d_rays` chains heat maps of a clip -> Joints2D -> RayTrack3D.

`joint_information` is how well the views fix a point: the 3 x 3 information matrix of the pixel reprojection at a 3-D point, on
`egr_joint_info_f32`, operator `egorear_amd::joint_info`; `smooth_trajectory_info` is `smooth_trajectory` with that matrix in place of
the scalar weight, on `egr_info_track_f32`, operator `egorear_amd::info_track` - the range, which a near-parallel pair
measures badly, is smoothed hard and the directions across it barely.  Neither is differentiable.  `decode_clip_3d_info` chains heat
maps of a clip -> Joints3D -> Track3D (the linearisation track) -> Information3D at that track -> InfoTrack3D, five launches.

`filter_trajectory` is `smooth_trajectory` for a live stream: a causal filter with a fixed lag on `egr_trajectory_filter_f32` /
`egr_trajectory_filter_tail_f32`, operators `egorear_amd::trajectory_filter` (it mutates its state) and
`egorear_amd::trajectory_filter_tail` - every arriving frame gives frame t - lag of the plain track over the frames seen so far, at a
cost that does not grow with the stream; a gate down-weights an observation far from what the earlier frames predict.
`new_track_filter` makes the state, `filter_tail` reads the frames no step has described yet, `decode_stream_3d` chains heat maps ->
Joints3D -> TrackStep, three launches that one captured graph replays per frame.  Not differentiable.
"""
from __future__ import annotations

import math
import os
from typing import NamedTuple, Optional, Sequence, Tuple, Union

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


def _c(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else t.contiguous()


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
    hip._on_device("decode.get_max_preds_soft", batch_heatmaps)
    coords, maxvals, _, _, _, _ = soft_argmax_op(batch_heatmaps, 1.0, MODE_SOFTMAX, bool(normalize), 0.0, False)
    return coords, maxvals.unsqueeze(-1)


def integrate_tensor_2d(heatmaps: torch.Tensor, softmax: bool = True, multiplier: float = 100.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """`integrate_tensor_2d` (utils/util.py:80-109): heatmaps (B, J, H, W) -> coordinates (B, J, 2) in heat-map pixels, (x, y), and
    the weights they were taken with, (B, J, H, W): softmax(multiplier * h) over a map, or relu(multiplier * h) with `softmax=False`
    (where the coordinates divide by the map's mass; a map without positive mass gives NaN, as there - its gradient is zero here,
    NaN there).  The second value is returned detached: gradient flows through the coordinates only."""
    mode = MODE_SOFTMAX if softmax else MODE_RELU
    _check(heatmaps, float(multiplier), mode, dims=4, what="integrate_tensor_2d")
    hip._on_device("decode.integrate_tensor_2d", heatmaps)
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
    hip._on_device("decode.decode_joints_2d", heatmaps)
    W = int(heatmaps.shape[-1])
    soft, maxvals, index, valid, _, _ = soft_argmax_op(heatmaps, float(beta), MODE_SOFTMAX, False, float(threshold), False)
    hard = torch.stack((index % W, torch.div(index, W, rounding_mode="floor")), -1).to(torch.float32)
    return Joints2D(soft, hard, maxvals, valid.view(torch.bool))     # (0 / 1 bytes: a reinterpretation, not a copy)


# ---- triangulation ----------------------------------------------------------------------------------------------------------------

_CAMERA_NAMES = ("camera_front_left", "camera_front_right", "camera_back_left", "camera_back_right")
_PKG_CALIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "calib", "ego4view")
_RAY_RECORDS = {}    # (camera_model, calibration directory | the cameras' ids, device) -> (cameras, (V, 30) device tensor)


@torch.library.custom_op("egorear_amd::triangulate", mutates_args=(), device_types="cuda")
def triangulate_op(coords: torch.Tensor, conf: torch.Tensor, cams: torch.Tensor, ctm: Optional[torch.Tensor], sx: float, sy: float,
                   threshold: float, min_det_ratio: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(pts (B, J, 3) cm, cost (B, J) cm^2, resid (B, V, J) cm, ok (B, J) uint8) of coords (B, V, J, 2) * (sx, sy) = normalised image
    points, conf (B, V, J), cams (V, 30) = camera.packed_rays(), ctm (B, V, 4, 4) or None (the syn rig)."""
    hip._tri_operands(coords, conf, cams, ctm, sx, sy, min_det_ratio, "decode.triangulate", dense=False)
    return hip.triangulate(_c(coords), _c(conf), _c(cams), _c(ctm), sx, sy, threshold, min_det_ratio)


@triangulate_op.register_fake
def _triangulate_fake(coords, conf, cams, ctm, sx, sy, threshold, min_det_ratio):
    B, V, J = hip._tri_operands(coords, conf, cams, ctm, sx, sy, min_det_ratio, "decode.triangulate", dense=False)
    return (coords.new_empty((B, J, 3)), coords.new_empty((B, J)), coords.new_empty((B, V, J)), coords.new_empty((B, J), dtype=torch.uint8))


@torch.library.custom_op("egorear_amd::triangulate_bwd", mutates_args=(), device_types="cuda")
def triangulate_bwd_op(coords: torch.Tensor, conf: torch.Tensor, cams: torch.Tensor, ctm: Optional[torch.Tensor],
                       g_pts: Optional[torch.Tensor], g_cost: Optional[torch.Tensor], sx: float, sy: float, threshold: float,
                       min_det_ratio: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(g_coords (B, V, J, 2), g_conf (B, V, J)) from g_pts (B, J, 3) and g_cost (B, J), each None for zeros."""
    gp = None if g_pts is None else g_pts.to(torch.float32)
    gc = None if g_cost is None else g_cost.to(torch.float32)
    hip._tri_operands(coords, conf, cams, ctm, sx, sy, min_det_ratio, "decode.triangulate_bwd", gp, gc, dense=False)
    return hip.triangulate_bwd(_c(coords), _c(conf), _c(cams), _c(ctm), _c(gp), _c(gc), sx, sy, threshold, min_det_ratio)


@triangulate_bwd_op.register_fake
def _triangulate_bwd_fake(coords, conf, cams, ctm, g_pts, g_cost, sx, sy, threshold, min_det_ratio):
    B, V, J = hip._tri_operands(coords, conf, cams, ctm, sx, sy, min_det_ratio, "decode.triangulate_bwd", g_pts, g_cost, dense=False)
    return coords.new_empty((B, V, J, 2)), coords.new_empty((B, V, J))


def _tri_setup_context(ctx, inputs, output):
    coords, conf, cams, ctm, sx, sy, threshold, min_det_ratio = inputs
    ctx.has_ctm = ctm is not None
    ctx.save_for_backward(*((coords, conf, cams) + ((ctm,) if ctx.has_ctm else ())))
    ctx.args = (sx, sy, threshold, min_det_ratio)
    ctx.mark_non_differentiable(output[2])       # resid (ok is not a floating-point tensor)


def _tri_autograd(ctx, g_pts, g_cost, g_resid, g_ok):
    coords, conf, cams = ctx.saved_tensors[:3]
    ctm = ctx.saved_tensors[3] if ctx.has_ctm else None
    g_coords, g_conf = triangulate_bwd_op(coords, conf, cams, ctm, g_pts, g_cost, *ctx.args)
    return g_coords, g_conf, None, None, None, None, None, None


triangulate_op.register_autograd(_tri_autograd, setup_context=_tri_setup_context)


class Joints3D(NamedTuple):
    pose: torch.Tensor       # (B, J, 3) cm, device frame; 0 where not valid
    cost: torch.Tensor       # (B, J) weighted mean squared ray distance, cm^2
    residual: torch.Tensor   # (B, V, J) distance of the point from each view's ray, cm; 0 for excluded views
    valid: torch.Tensor      # (B, J) bool: at least two views carried weight and the rays were not parallel


def _ray_records(cameras: Union[str, Sequence], calib_dir: Optional[str], device: torch.device) -> torch.Tensor:
    """(V, 30) fp32 records of the cameras on `device`, uploaded once per (cameras, device).  A warm cache is a dictionary lookup,
    which traces; the upload itself is kept out of a traced graph."""
    if isinstance(cameras, str):
        key = (cameras, calib_dir or _PKG_CALIB, str(device))
    else:
        cameras = tuple(cameras)
        key = tuple(id(c) for c in cameras) + (str(device),)
    hit = _RAY_RECORDS.get(key)
    return hit[1] if hit is not None else _upload_ray_records(cameras, key, device)


@torch._dynamo.disable
def _upload_ray_records(cameras, key, device) -> torch.Tensor:
    import numpy as np
    if isinstance(cameras, str):
        from .camera import FishEyeCameraCalibratedModel
        cameras = tuple(FishEyeCameraCalibratedModel(cameras, key[1], n) for n in _CAMERA_NAMES)
    if not 2 <= len(cameras) <= 4:
        raise ValueError(f"egorear_amd.decode.triangulate_joints: 2 to 4 cameras are supported, got {len(cameras)}")
    rec = torch.from_numpy(np.stack([c.packed_rays() for c in cameras])).to(device)
    _RAY_RECORDS[key] = (cameras, rec)       # (the cameras are kept: their ids are the key)
    return rec


def _scales(heatmap_size) -> Tuple[float, float]:
    try:
        H, W = (float(v) for v in heatmap_size)
    except (TypeError, ValueError):
        raise ValueError(f"egorear_amd.decode.triangulate_joints: heatmap_size must be (H, W), got {heatmap_size!r}") from None
    if not (H > 0.0 and W > 0.0 and math.isfinite(H) and math.isfinite(W)):
        raise ValueError(f"egorear_amd.decode.triangulate_joints: heatmap_size must be positive, got {heatmap_size!r}")
    return 1.0 / W, 1.0 / H


def triangulate_joints(coords: torch.Tensor, conf: torch.Tensor, cameras: Union[str, Sequence], coord_trans_mat: Optional[torch.Tensor] = None,
                       heatmap_size: Tuple[float, float] = (64, 64), threshold: float = 0.5, min_det_ratio: float = 1e-6,
                       camera_calib_file_dir_path: Optional[str] = None) -> Joints3D:
    """coords (B, V, J, 2) = (x, y) in pixels of a `heatmap_size` = (H, W) map (anchors in [0, 1]: heatmap_size (1, 1)), conf (B, V, J)
    -> Joints3D(pose, cost, residual, valid): per joint the point closest, in the conf-weighted least-squares sense, to the V fisheye
    rays; a view counts when its conf >= threshold and its coordinates are finite.  `cameras`: 2 to 4 FishEyeCameraCalibratedModel in
    view order, or a camera_model string ("ego4view_syn" / "ego4view_rw": the four packaged calibrations, or those of
    `camera_calib_file_dir_path`).  Without `coord_trans_mat` the ego4view_syn rig places the cameras (each on its own: the offsets do
    not chain); with it (B, V, 4, 4), device frame (m) -> camera frame as in the rw models.  One launch; pose and cost are
    differentiable with respect to coords and conf."""
    sx, sy = _scales(heatmap_size)
    cams = _ray_records(cameras, camera_calib_file_dir_path, coords.device)
    hip._tri_operands(coords, conf, cams, coord_trans_mat, sx, sy, float(min_det_ratio), "decode.triangulate_joints", dense=False)
    hip._on_device("decode.triangulate_joints", coords, conf, coord_trans_mat)
    pts, cost, resid, ok = triangulate_op(coords, conf, cams, coord_trans_mat, sx, sy, float(threshold), float(min_det_ratio))
    return Joints3D(pts, cost, resid, ok.view(torch.bool))


def decode_joints_3d(heatmaps: torch.Tensor, cameras: Union[str, Sequence], coord_trans_mat: Optional[torch.Tensor] = None, beta: float = 100.0,
                     threshold: float = 0.5, min_det_ratio: float = 1e-6, camera_calib_file_dir_path: Optional[str] = None
                     ) -> Tuple[Joints3D, Joints2D]:
    """heatmaps (B, V, J, H, W) -> (Joints3D, Joints2D): soft-argmax, then the triangulation of its sub-pixel joints weighted by the
    maps' maxima - two launches with nothing between them (the pixel scale and the threshold are kernel arguments).  Gradients of
    pose and cost reach the heat maps through both backward operators."""
    _check(heatmaps, float(beta), MODE_SOFTMAX, dims=5, what="decode_joints_3d")
    if not 2 <= heatmaps.shape[1] <= 4:      # (the soft-argmax takes any V: without this it would run before the triangulation refuses)
        raise ValueError(f"egorear_amd.decode.decode_joints_3d: 2 to 4 views are supported, got {tuple(heatmaps.shape)}")
    joints2d = decode_joints_2d(heatmaps, beta=beta, threshold=threshold)
    H, W = int(heatmaps.shape[-2]), int(heatmaps.shape[-1])
    joints3d = triangulate_joints(joints2d.soft, joints2d.maxvals, cameras, coord_trans_mat, (H, W), threshold, min_det_ratio,
                                  camera_calib_file_dir_path)
    return joints3d, joints2d


# ---- volumetric fusion --------------------------------------------------------------------------------------------------------------

def _check_vol(hm, conf, centers, cams, ctm, center_ok, grid, cube, beta, what: str = "volume_fuse", g_pose=None, g_peak=None):
    # (the operators make their operands contiguous before the launch, which checks that too)
    return hip._volume_operands(hm, conf, centers, cams, ctm, center_ok, grid, cube, beta, "decode." + what, g_pose, g_peak, dense=False)


@torch.library.custom_op("egorear_amd::volume_fuse", mutates_args=(), device_types="cuda")
def volume_fuse_op(hm: torch.Tensor, conf: torch.Tensor, centers: torch.Tensor, cams: torch.Tensor, ctm: Optional[torch.Tensor],
                   center_ok: Optional[torch.Tensor], grid: int, cube: float, beta: float, threshold: float
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(pose (B, J, 3) cm, peak (B, J), index (B, J) int32, spread (B, J) cm, ok (B, J) uint8) of hm (B, V, J, H, W), conf (B, V, J),
    centers (B, J, 3) cm, cams (V, 30) = camera.packed_rays(), ctm (B, V, 4, 4) or None (the syn rig), center_ok (B, J) uint8 or None."""
    hm, conf, centers, cams, ctm, center_ok = _aligned(hm), _c(conf), _c(centers), _c(cams), _c(ctm), _c(center_ok)
    _check_vol(hm, conf, centers, cams, ctm, center_ok, grid, cube, beta)
    return hip.volume_fuse(hm, conf, centers, cams, ctm, center_ok, grid, cube, beta, threshold)


@volume_fuse_op.register_fake
def _volume_fuse_fake(hm, conf, centers, cams, ctm, center_ok, grid, cube, beta, threshold):
    B, V, J, H, W = _check_vol(hm, conf, centers, cams, ctm, center_ok, grid, cube, beta)
    return (hm.new_empty((B, J, 3)), hm.new_empty((B, J)), hm.new_empty((B, J), dtype=torch.int32), hm.new_empty((B, J)),
            hm.new_empty((B, J), dtype=torch.uint8))


@torch.library.custom_op("egorear_amd::volume_fuse_bwd", mutates_args=(), device_types="cuda")
def volume_fuse_bwd_op(hm: torch.Tensor, conf: torch.Tensor, centers: torch.Tensor, cams: torch.Tensor, ctm: Optional[torch.Tensor],
                       center_ok: Optional[torch.Tensor], g_pose: Optional[torch.Tensor], g_peak: Optional[torch.Tensor], grid: int,
                       cube: float, beta: float, threshold: float) -> torch.Tensor:
    """g_hm (B, V, J, H, W) from g_pose (B, J, 3) and g_peak (B, J), each None for zeros."""
    hm, conf, centers, cams, ctm, center_ok = _aligned(hm), _c(conf), _c(centers), _c(cams), _c(ctm), _c(center_ok)
    gp = None if g_pose is None else g_pose.to(torch.float32).contiguous()
    gk = None if g_peak is None else g_peak.to(torch.float32).contiguous()
    _check_vol(hm, conf, centers, cams, ctm, center_ok, grid, cube, beta, "volume_fuse_bwd", gp, gk)
    return hip.volume_fuse_bwd(hm, conf, centers, cams, ctm, center_ok, gp, gk, grid, cube, beta, threshold)


@volume_fuse_bwd_op.register_fake
def _volume_fuse_bwd_fake(hm, conf, centers, cams, ctm, center_ok, g_pose, g_peak, grid, cube, beta, threshold):
    _check_vol(hm, conf, centers, cams, ctm, center_ok, grid, cube, beta, "volume_fuse_bwd", g_pose, g_peak)
    return hm.new_empty(hm.shape)


def _vol_setup_context(ctx, inputs, output):
    hm, conf, centers, cams, ctm, center_ok, grid, cube, beta, threshold = inputs
    ctx.has_ctm, ctx.has_ok = ctm is not None, center_ok is not None
    ctx.save_for_backward(*((hm, conf, centers, cams) + ((ctm,) if ctx.has_ctm else ()) + ((center_ok,) if ctx.has_ok else ())))
    ctx.args = (grid, cube, beta, threshold)
    ctx.mark_non_differentiable(output[3])       # spread (index and ok are not floating-point tensors)


def _vol_autograd(ctx, g_pose, g_peak, g_index, g_spread, g_ok):
    hm, conf, centers, cams = ctx.saved_tensors[:4]
    rest = list(ctx.saved_tensors[4:])
    ctm = rest.pop(0) if ctx.has_ctm else None
    center_ok = rest.pop(0) if ctx.has_ok else None
    g_hm = volume_fuse_bwd_op(hm, conf, centers, cams, ctm, center_ok, g_pose, g_peak, *ctx.args)
    return g_hm, None, None, None, None, None, None, None, None, None      # conf and centers are constants: the cube is placed


volume_fuse_op.register_autograd(_vol_autograd, setup_context=_vol_setup_context)


class Volume3D(NamedTuple):
    pose: torch.Tensor       # (B, J, 3) cm, device frame: the centre + the softmax-weighted mean voxel offset; 0 where not valid
    peak: torch.Tensor       # (B, J) the largest fused score of the cube
    index: torch.Tensor      # (B, J) int32: the first voxel attaining it, (iz * G + iy) * G + ix; -1 where not valid
    spread: torch.Tensor     # (B, J) cm: rms radius of the softmax distribution about `pose` - a cheap uncertainty
    valid: torch.Tensor      # (B, J) bool: at least two views carried weight and the centre was usable


def _fuse(heatmaps, centers, cams, conf, coord_trans_mat, center_ok, grid, cube_cm, beta, threshold, what) -> Volume3D:
    if heatmaps.dim() != 5:
        raise ValueError(f"egorear_amd.decode.{what}: heat maps must be (B, V, J, H, W), got {tuple(heatmaps.shape)}")
    B, V, J = (int(v) for v in heatmaps.shape[:3])
    if centers.dim() == 2 and tuple(centers.shape) == (B, 3):
        centers = centers.unsqueeze(1).expand(B, J, 3)
    if conf is None:
        conf = heatmaps.new_ones((B, V, J))
    if isinstance(grid, bool) or not isinstance(grid, int):
        raise ValueError(f"egorear_amd.decode.{what}: grid must be an integer, got {grid!r}")
    _check_vol(heatmaps, conf, centers, cams, coord_trans_mat, center_ok, grid, float(cube_cm), float(beta), what)
    hip._on_device("decode." + what, heatmaps, conf, centers, coord_trans_mat, center_ok)
    pose, peak, index, spread, ok = volume_fuse_op(heatmaps, conf, centers, cams, coord_trans_mat, center_ok, grid, float(cube_cm),
                                                   float(beta), float(threshold))
    return Volume3D(pose, peak, index, spread, ok.view(torch.bool))


def fuse_joints_volumetric(heatmaps: torch.Tensor, centers: torch.Tensor, cameras: Union[str, Sequence], conf: Optional[torch.Tensor] = None,
                           coord_trans_mat: Optional[torch.Tensor] = None, grid: int = 16, cube_cm: float = 40.0, beta: float = 100.0,
                           threshold: float = 0.5, camera_calib_file_dir_path: Optional[str] = None) -> Volume3D:
    """heatmaps (B, V, J, H, W), centers (B, J, 3) - or (B, 3) for every joint of a frame - in cm, device frame -> Volume3D(pose, peak,
    index, spread, valid): a `grid`^3 voxel cube of side `cube_cm` is put around each centre, every voxel centre is projected into the V
    fisheye cameras, the heat maps are sampled there (bilinear, zero outside), the views' samples are averaged with the weights `conf`
    (B, V, J; None: every view weighs 1; a view counts when its conf >= threshold) and the joint is the softmax(beta * score)-weighted
    mean voxel.  `cameras` and `coord_trans_mat` as in `triangulate_joints`.  The centres come from `decode_joints_3d` or from a
    lifting head's pose; they and `conf` are constants - pose and peak are differentiable with respect to the heat maps, of all views
    jointly.  One launch (V * H * W <= 16384, 2 <= grid <= 32)."""
    cams = _ray_records(cameras, camera_calib_file_dir_path, heatmaps.device)
    return _fuse(heatmaps, centers, cams, conf, coord_trans_mat, None, grid, cube_cm, beta, threshold, "fuse_joints_volumetric")


def decode_joints_3d_volumetric(heatmaps: torch.Tensor, cameras: Union[str, Sequence], coord_trans_mat: Optional[torch.Tensor] = None,
                                grid: int = 16, cube_cm: float = 40.0, beta: float = 100.0, volume_beta: float = 100.0, threshold: float = 0.5,
                                min_det_ratio: float = 1e-6, camera_calib_file_dir_path: Optional[str] = None
                                ) -> Tuple[Volume3D, Joints3D, Joints2D]:
    """heatmaps (B, V, J, H, W) -> (Volume3D, Joints3D, Joints2D): `decode_joints_3d` (soft-argmax at `beta`, triangulation), then the
    volumetric fusion (softmax at `volume_beta`) in a cube around the detached triangulated pose, weighted by the maps' maxima - three
    launches with no torch arithmetic between them.  A joint whose triangulation is not valid is not valid here.  The gradient of the
    fused pose and peak reaches the heat maps through the fusion alone (the cube is placed, not learned); the triangulated pose and
    cost keep their own gradients."""
    joints3d, joints2d = decode_joints_3d(heatmaps, cameras, coord_trans_mat, beta, threshold, min_det_ratio, camera_calib_file_dir_path)
    cams = _ray_records(cameras, camera_calib_file_dir_path, heatmaps.device)
    # (bool -> uint8 and detach are reinterpretations: nothing is launched for them)
    volume = _fuse(heatmaps, joints3d.pose.detach(), cams, joints2d.maxvals.detach(), coord_trans_mat, joints3d.valid.view(torch.uint8),
                   grid, cube_cm, volume_beta, threshold, "decode_joints_3d_volumetric")
    return volume, joints3d, joints2d


# ---- multi-peak decoding and consensus triangulation --------------------------------------------------------------------------------

@torch.library.custom_op("egorear_amd::find_peaks", mutates_args=(), device_types="cuda")
def find_peaks_op(hm: torch.Tensor, k: int, nms_radius: int, refine_radius: int, beta: float, threshold: float
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(coords (..., k, 2) heat-map pixels, score (..., k), index (..., k) int32, count (...) int32) of hm (..., H, W), H * W <= 4096:
    egr_peaks_f32.  No output is differentiable: there is no gradient through the selection or the window refinement."""
    lead, _, _, _ = hip._peaks_operands(hm, k, nms_radius, refine_radius, beta, threshold, "decode.find_peaks", dense=False)
    coords, score, index, count = hip.find_peaks(_aligned(hm), k, nms_radius, refine_radius, beta, threshold)
    return coords.view(lead + (k, 2)), score.view(lead + (k,)), index.view(lead + (k,)), count.view(lead)


@find_peaks_op.register_fake
def _find_peaks_fake(hm, k, nms_radius, refine_radius, beta, threshold):
    lead, _, _, _ = hip._peaks_operands(hm, k, nms_radius, refine_radius, beta, threshold, "decode.find_peaks", dense=False)
    return (hm.new_empty(lead + (k, 2)), hm.new_empty(lead + (k,)), hm.new_empty(lead + (k,), dtype=torch.int32),
            hm.new_empty(lead, dtype=torch.int32))


@torch.library.custom_op("egorear_amd::consensus", mutates_args=(), device_types="cuda")
def consensus_op(cand: torch.Tensor, cscore: torch.Tensor, cindex: torch.Tensor, cams: torch.Tensor, ctm: Optional[torch.Tensor], sx: float,
                 sy: float, max_reproj: float, min_views: int, min_det_ratio: float
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(choice (B, V, J) int32, sel_coords (B, V, J, 2), sel_conf (B, V, J), score (B, J), inliers (B, J) int32, hyp (B, J) int32) of the
    candidates cand (B, V, J, K, 2), cscore (B, V, J, K), cindex (B, V, J, K) int32, cams (V, 30), ctm (B, V, 4, 4) or None:
    egr_consensus_f32.  No output is differentiable: the selection is a discrete choice, its coordinates are copies."""
    hip._consensus_operands(cand, cscore, cindex, cams, ctm, sx, sy, max_reproj, min_views, min_det_ratio, "decode.consensus", dense=False)
    return hip.consensus(_c(cand), _c(cscore), _c(cindex), _c(cams), _c(ctm), sx, sy, max_reproj, min_views, min_det_ratio)


@consensus_op.register_fake
def _consensus_fake(cand, cscore, cindex, cams, ctm, sx, sy, max_reproj, min_views, min_det_ratio):
    B, V, J, K = hip._consensus_operands(cand, cscore, cindex, cams, ctm, sx, sy, max_reproj, min_views, min_det_ratio, "decode.consensus",
                                         dense=False)
    return (cand.new_empty((B, V, J), dtype=torch.int32), cand.new_empty((B, V, J, 2)), cand.new_empty((B, V, J)), cand.new_empty((B, J)),
            cand.new_empty((B, J), dtype=torch.int32), cand.new_empty((B, J), dtype=torch.int32))


def _nograd_setup_context(ctx, inputs, output):
    ctx.n_inputs = len(inputs)
    ctx.mark_non_differentiable(*(t for t in output if t.is_floating_point()))


def _nograd_autograd(ctx, *grads):
    return (None,) * ctx.n_inputs


find_peaks_op.register_autograd(_nograd_autograd, setup_context=_nograd_setup_context)
consensus_op.register_autograd(_nograd_autograd, setup_context=_nograd_setup_context)


class Peaks2D(NamedTuple):
    coords: torch.Tensor     # (B, V, J, K, 2) refined (x, y), heat-map pixels, best peak first; 0 in unfilled slots
    score: torch.Tensor      # (B, V, J, K) the peaks' own values; 0 in unfilled slots
    index: torch.Tensor      # (B, V, J, K) int32 flat index of the peak pixel; -1 in unfilled slots
    count: torch.Tensor      # (B, V, J) int32 peaks kept, 0..K


class Consensus(NamedTuple):
    coords: torch.Tensor      # (B, V, J, 2) the chosen candidate of every view, copied; 0 where the view has no choice
    conf: torch.Tensor        # (B, V, J) its score; 0 where the view has no choice
    choice: torch.Tensor      # (B, V, J) int32 its slot k, or -1
    score: torch.Tensor       # (B, J) the winning hypothesis's support, summed over the views
    inliers: torch.Tensor     # (B, J) int32 views with a choice
    hypothesis: torch.Tensor  # (B, J) int32 (pair(a, b) * K + ka) * K + kb of the winner, or -1 when nothing qualifies


def find_peaks_2d(heatmaps: torch.Tensor, k: int = 3, nms_radius: int = 1, refine_radius: int = 2, beta: float = 100.0,
                  threshold: float = 0.5) -> Peaks2D:
    """heatmaps (B, V, J, H, W), H * W <= 4096 -> Peaks2D(coords, score, index, count): per map the `k` (1..4) best local maxima above
    `threshold` - a pixel that beats its (2 nms_radius + 1)^2 neighbourhood, a plateau counting once at its first pixel - ordered by value,
    each refined to sub-pixel by the softmax(beta h)-weighted mean over its (2 refine_radius + 1)^2 window.  One launch, one read of the
    maps.  Nothing here is differentiable."""
    if heatmaps.dim() != 5:
        raise ValueError(f"egorear_amd.decode.find_peaks_2d: heat maps must be (B, V, J, H, W), got {tuple(heatmaps.shape)}")
    hip._peaks_operands(heatmaps, k, nms_radius, refine_radius, float(beta), float(threshold), "decode.find_peaks_2d", dense=False)
    hip._on_device("decode.find_peaks_2d", heatmaps, exc=ValueError)
    return Peaks2D(*find_peaks_op(heatmaps, k, nms_radius, refine_radius, float(beta), float(threshold)))


def select_consistent(peaks: Peaks2D, cameras: Union[str, Sequence], coord_trans_mat: Optional[torch.Tensor] = None,
                      heatmap_size: Tuple[float, float] = (64, 64), max_reproj: float = 2.0, min_views: int = 2, min_det_ratio: float = 1e-6,
                      camera_calib_file_dir_path: Optional[str] = None) -> Consensus:
    """peaks = find_peaks_2d's result over maps of `heatmap_size` = (H, W) -> Consensus(coords, conf, choice, score, inliers,
    hypothesis): per (frame, joint) every pair of candidates from two views is triangulated, the point is projected back into all views
    and each view supports it with its best  score * max(0, 1 - e^2 / max_reproj^2)  (e: heat-map pixels); the best-supported point
    that at least `min_views` views support picks one candidate - or none - per view.  `coords` / `conf` are the operands
    `triangulate_joints` takes.  `cameras` and `coord_trans_mat` as there.  One launch.  Nothing here is differentiable."""
    sx, sy = _scales(heatmap_size)
    cand, cscore, cindex = peaks[0], peaks[1], peaks[2]
    cams = _ray_records(cameras, camera_calib_file_dir_path, cand.device)
    hip._consensus_operands(cand, cscore, cindex, cams, coord_trans_mat, sx, sy, float(max_reproj), min_views, float(min_det_ratio),
                            "decode.select_consistent", dense=False)
    hip._on_device("decode.select_consistent", cand, cscore, cindex, coord_trans_mat, exc=ValueError)
    choice, sel_coords, sel_conf, score, inliers, hyp = consensus_op(cand, cscore, cindex, cams, coord_trans_mat, sx, sy, float(max_reproj),
                                                                     min_views, float(min_det_ratio))
    return Consensus(sel_coords, sel_conf, choice, score, inliers, hyp)


def decode_joints_3d_robust(heatmaps: torch.Tensor, cameras: Union[str, Sequence], coord_trans_mat: Optional[torch.Tensor] = None, k: int = 3,
                            nms_radius: int = 1, refine_radius: int = 2, beta: float = 100.0, threshold: float = 0.5,
                            max_reproj: float = 2.0, min_views: int = 2, min_det_ratio: float = 1e-6,
                            camera_calib_file_dir_path: Optional[str] = None) -> Tuple[Joints3D, Consensus, Peaks2D]:
    """heatmaps (B, V, J, H, W) -> (Joints3D, Consensus, Peaks2D): the `k` best peaks of every map, the candidates the views agree on,
    then `triangulate_joints` of those - three launches with no torch operation between them (the consensus writes the
    triangulation's operands).  A view whose map fired on a second mode is out-voted by the others instead of bending the pose;
    `Joints3D.residual` reports the accepted views only, and a joint without a consensus is not valid.  With two views there is no
    third to out-vote a distractor: the consensus then only rejects pairs that do not meet.  Nothing here is differentiable."""
    # (the peaks take any V: without this guard they would run before the consensus refuses)
    if heatmaps.dim() != 5 or not 2 <= heatmaps.shape[1] <= 4:
        raise ValueError(f"egorear_amd.decode.decode_joints_3d_robust: heat maps must be (B, V, J, H, W) with 2 to 4 views, got "
                         f"{tuple(heatmaps.shape)}")
    peaks = find_peaks_2d(heatmaps, k, nms_radius, refine_radius, beta, threshold)
    H, W = int(heatmaps.shape[-2]), int(heatmaps.shape[-1])
    agreed = select_consistent(peaks, cameras, coord_trans_mat, (H, W), max_reproj, min_views, min_det_ratio, camera_calib_file_dir_path)
    # (a rejected view carries conf 0 and is excluded whatever the threshold; an accepted one scored above `threshold` already)
    joints3d = triangulate_joints(agreed.coords, agreed.conf, cameras, coord_trans_mat, (H, W), threshold, min_det_ratio,
                                  camera_calib_file_dir_path)
    return joints3d, agreed, peaks


# ---- bone-length-constrained skeleton fit -------------------------------------------------------------------------------------------

# Skeleton.kinematic_parents (pose_estimation/utils/skeleton.py:33-34) over the 16 joints of its heatmap_sequence: head, neck, then the
# arms and the legs down to the balls of the feet
SKELETON_PARENTS_16 = (0, 0, 1, 1, 2, 3, 4, 5, 2, 3, 8, 9, 10, 11, 12, 13)
# the 15 heat-map joints: the same tree without the head, re-indexed - the neck is the root
HEATMAP_PARENTS_15 = (0, 0, 0, 1, 2, 3, 4, 1, 2, 7, 8, 9, 10, 11, 12)


def _parents_for(parents, J: int, what: str):
    """The caller's table as it is (hip's validators judge it), or the 16- / 15-joint table by J."""
    if parents is not None:
        return parents
    if J == 16:
        return list(SKELETON_PARENTS_16)
    if J == 15:
        return list(HEATMAP_PARENTS_15)
    raise ValueError(f"egorear_amd.decode.{what}: {J} joints need an explicit parent table (15 and 16 have one)")


@torch.library.custom_op("egorear_amd::skeleton_fit", mutates_args=(), device_types="cuda")
def skeleton_fit_op(coords: torch.Tensor, conf: torch.Tensor, cams: torch.Tensor, ctm: Optional[torch.Tensor], parents: Sequence[int],
                    bone_length: torch.Tensor, init: torch.Tensor, init_ok: torch.Tensor, sx: float, sy: float, threshold: float,
                    min_det_ratio: float, bone_weight: float, prior_weight: float, iterations: int
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(pose (B, J, 3) cm, ray_cost (B, J), bone (B, J), valid (B, J) uint8, energy0 (B), energy (B), grad (B), steps (B) int32) of the
    triangulation's operands, a parent table, bone_length (J) or (B, J), init (B, J, 3) and init_ok (B, J) uint8: egr_skeleton_fit_f32
    (DESIGN.md 5q).  No output is differentiable: the implicit-function backward is not part of this operator."""
    hip._skeleton_operands(coords, conf, cams, ctm, parents, bone_length, init, init_ok, sx, sy, min_det_ratio, bone_weight, prior_weight,
                           iterations, "decode.skeleton_fit", dense=False)
    return hip.skeleton_fit(_c(coords), _c(conf), _c(cams), _c(ctm), parents, _c(bone_length), _c(init), _c(init_ok), sx, sy, threshold,
                            min_det_ratio, bone_weight, prior_weight, iterations)


@skeleton_fit_op.register_fake
def _skeleton_fit_fake(coords, conf, cams, ctm, parents, bone_length, init, init_ok, sx, sy, threshold, min_det_ratio, bone_weight,
                       prior_weight, iterations):
    B, V, J, _, _ = hip._skeleton_operands(coords, conf, cams, ctm, parents, bone_length, init, init_ok, sx, sy, min_det_ratio, bone_weight,
                                           prior_weight, iterations, "decode.skeleton_fit", dense=False)
    new = coords.new_empty
    return (new((B, J, 3)), new((B, J)), new((B, J)), new((B, J), dtype=torch.uint8), new((B,)), new((B,)), new((B,)),
            new((B,), dtype=torch.int32))


@torch.library.custom_op("egorear_amd::bone_lengths", mutates_args=(), device_types="cuda")
def bone_lengths_op(pose: torch.Tensor, valid: torch.Tensor, parents: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(length (J), spread (J), count (J) int32) of pose (B, J, 3), valid (B, J) uint8: egr_bone_lengths_f32.  Not differentiable."""
    hip._pose_operands(pose, valid, parents, "decode.bone_lengths", dense=False)
    return hip.bone_lengths(_c(pose), _c(valid), parents)


@bone_lengths_op.register_fake
def _bone_lengths_fake(pose, valid, parents):
    _, J, _ = hip._pose_operands(pose, valid, parents, "decode.bone_lengths", dense=False)
    return pose.new_empty((J,)), pose.new_empty((J,)), pose.new_empty((J,), dtype=torch.int32)


@torch.library.custom_op("egorear_amd::skeleton_resize", mutates_args=(), device_types="cuda")
def skeleton_resize_op(pose: torch.Tensor, valid: torch.Tensor, bone_length: torch.Tensor, parents: Sequence[int]) -> torch.Tensor:
    """pose (B, J, 3) with its bones set to bone_length (J) or (B, J) along the chain: egr_skeleton_resize_f32.  Not differentiable."""
    hip._resize_operands(pose, valid, bone_length, parents, "decode.skeleton_resize", dense=False)
    return hip.skeleton_resize(_c(pose), _c(valid), _c(bone_length), parents)


@skeleton_resize_op.register_fake
def _skeleton_resize_fake(pose, valid, bone_length, parents):
    hip._resize_operands(pose, valid, bone_length, parents, "decode.skeleton_resize", dense=False)
    return pose.new_empty(pose.shape)


def _nograd_setup_context_one(ctx, inputs, output):
    _nograd_setup_context(ctx, inputs, (output,))


skeleton_fit_op.register_autograd(_nograd_autograd, setup_context=_nograd_setup_context)
bone_lengths_op.register_autograd(_nograd_autograd, setup_context=_nograd_setup_context)
skeleton_resize_op.register_autograd(_nograd_autograd, setup_context=_nograd_setup_context_one)


class Skeleton3D(NamedTuple):
    pose: torch.Tensor       # (B, J, 3) cm, device frame; 0 where not valid
    ray_cost: torch.Tensor   # (B, J) weighted mean squared ray distance at the fitted point, cm^2 (Joints3D.cost's definition)
    bone: torch.Tensor       # (B, J) fitted bone length to the parent, cm; 0 for the root and for a bone that is not used
    valid: torch.Tensor      # (B, J) bool: the joint took part in the fit
    energy0: torch.Tensor    # (B) the energy at the init
    energy: torch.Tensor     # (B) the energy at the result, <= energy0
    grad: torch.Tensor       # (B) largest |dE/dp| component at the result: how converged the fit is
    steps: torch.Tensor      # (B) int32 steps kept


class BoneStats(NamedTuple):
    length: torch.Tensor     # (J) mean bone length over the frames where both ends are valid, cm; 0 for the root and when count is 0
    spread: torch.Tensor     # (J) its standard deviation, cm
    count: torch.Tensor      # (J) int32 those frames


def _as_flags(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.uint8) if t.dtype == torch.bool else t       # (a reinterpretation, not a copy)


def fit_skeleton(coords: torch.Tensor, conf: torch.Tensor, cameras: Union[str, Sequence], bone_length: torch.Tensor, init: torch.Tensor,
                 init_ok: Optional[torch.Tensor] = None, parents: Optional[Sequence[int]] = None,
                 coord_trans_mat: Optional[torch.Tensor] = None, heatmap_size: Tuple[float, float] = (64, 64), threshold: float = 0.5,
                 bone_weight: float = 1.0, prior_weight: float = 0.0, iterations: int = 16, min_det_ratio: float = 1e-6,
                 camera_calib_file_dir_path: Optional[str] = None) -> Skeleton3D:
    """coords (B, V, J, 2), conf (B, V, J), `cameras`, `coord_trans_mat`, `heatmap_size`, `threshold` as for `triangulate_joints`;
    bone_length (J) or (B, J) cm (`estimate_bone_lengths`, or the wearer's measurements; an entry <= 0 frees that bone); init (B, J, 3)
    cm - a triangulation, a lifting head's pose, the previous frame's fit - and init_ok (B, J) bool / uint8 (None: every joint)
    -> Skeleton3D: the joints that minimise  sum conf * dist^2(joint, its rays) + bone_weight * sum (bone - length)^2 + prior_weight *
    sum |joint - init|^2  along the tree `parents` (None: the 16- or 15-joint table by J).  With prior_weight 0 a joint takes part
    when its init is ok and its own rays fix it, or one ray and a bone to a parent that takes part do - so a joint that only one
    camera sees is placed, which the triangulation cannot do; with prior_weight > 0 every joint with an init takes part.
    `iterations` (1..256) Levenberg-Marquardt iterations on the Gauss-Newton model run, always.  Convergence is linear and depends on
    the scene: 16 regularise a triangulation; from 3 cm off at 0.1 px of noise most scenes reach fp32 stationarity in 16 to 32 and
    some need up to 176; at 0.3 px a few did not reach it within the 256 allowed - `grad` reports how stationary the
    result is, and the previous frame's fit as `init` is the cheap way to be close.  One launch; nothing here is differentiable."""
    sx, sy = _scales(heatmap_size)
    cams = _ray_records(cameras, camera_calib_file_dir_path, coords.device)
    if coords.dim() != 4:
        raise ValueError(f"egorear_amd.decode.fit_skeleton: coords must be (B, V, J, 2), got {tuple(coords.shape)}")
    table = _parents_for(parents, int(coords.shape[2]), "fit_skeleton")
    if init_ok is None:
        init_ok = torch.ones(coords.shape[0], coords.shape[2], dtype=torch.uint8, device=coords.device)
    init_ok = _as_flags(init_ok)
    table = hip._skeleton_operands(coords, conf, cams, coord_trans_mat, table, bone_length, init, init_ok, sx, sy, float(min_det_ratio),
                                   float(bone_weight), float(prior_weight), iterations, "decode.fit_skeleton", dense=False)[3]
    hip._on_device("decode.fit_skeleton", coords, conf, coord_trans_mat, bone_length, init, init_ok, exc=ValueError)
    pose, ray_cost, bone, valid, energy0, energy, grad, steps = skeleton_fit_op(
        coords, conf, cams, coord_trans_mat, table, bone_length, init, init_ok, sx, sy, float(threshold), float(min_det_ratio),
        float(bone_weight), float(prior_weight), iterations)
    return Skeleton3D(pose, ray_cost, bone, valid.view(torch.bool), energy0, energy, grad, steps)


def estimate_bone_lengths(pose: torch.Tensor, valid: torch.Tensor, parents: Optional[Sequence[int]] = None) -> BoneStats:
    """pose (B, J, 3) cm and valid (B, J) of a clip -> BoneStats(length, spread, count): every bone's mean length and standard
    deviation over the frames in which both of its ends are valid - where `bone_length` comes from when nobody measured the wearer.
    One launch, bit-reproducible; not differentiable."""
    if pose.dim() != 3:
        raise ValueError(f"egorear_amd.decode.estimate_bone_lengths: pose must be (B, J, 3), got {tuple(pose.shape)}")
    table = _parents_for(parents, int(pose.shape[1]), "estimate_bone_lengths")
    valid = _as_flags(valid)
    table = hip._pose_operands(pose, valid, table, "decode.estimate_bone_lengths", dense=False)[2]
    hip._on_device("decode.estimate_bone_lengths", pose, valid, exc=ValueError)
    return BoneStats(*bone_lengths_op(pose, valid, table))


def resize_skeleton(pose: torch.Tensor, valid: torch.Tensor, bone_length: torch.Tensor, parents: Optional[Sequence[int]] = None) -> torch.Tensor:
    """`Skeleton._skeleton_resize` (utils/skeleton.py:163-174) in cm: pose (B, J, 3), valid (B, J), bone_length (J) or (B, J) -> the
    pose with every bone between two valid joints rescaled to its length, walking the tree from the root - each error moves everything
    below it, and the cameras are not asked: the baseline `fit_skeleton` is compared with.  A joint that is not valid keeps its place
    and its children start chains of their own.  One launch; not differentiable."""
    if pose.dim() != 3:
        raise ValueError(f"egorear_amd.decode.resize_skeleton: pose must be (B, J, 3), got {tuple(pose.shape)}")
    table = _parents_for(parents, int(pose.shape[1]), "resize_skeleton")
    valid = _as_flags(valid)
    table = hip._resize_operands(pose, valid, bone_length, table, "decode.resize_skeleton", dense=False)[2]
    hip._on_device("decode.resize_skeleton", pose, valid, bone_length, exc=ValueError)
    return skeleton_resize_op(pose, valid, bone_length, table)


def decode_joints_3d_skeleton(heatmaps: torch.Tensor, cameras: Union[str, Sequence], bone_length: torch.Tensor,
                              init: Optional[torch.Tensor] = None, init_ok: Optional[torch.Tensor] = None,
                              parents: Optional[Sequence[int]] = None, coord_trans_mat: Optional[torch.Tensor] = None, beta: float = 100.0,
                              threshold: float = 0.5, bone_weight: float = 1.0, prior_weight: float = 0.0, iterations: int = 16,
                              min_det_ratio: float = 1e-6, camera_calib_file_dir_path: Optional[str] = None
                              ) -> Tuple[Skeleton3D, Joints3D, Joints2D]:
    """heatmaps (B, V, J, H, W) -> (Skeleton3D, Joints3D, Joints2D): `decode_joints_3d` (soft-argmax at `beta`, triangulation), then
    `fit_skeleton` on the same 2-D joints - three launches.  Without `init` the fit starts from the triangulated pose and takes its
    `valid` as init_ok: it only regularises what the triangulation found.  With the caller's init (B, J, 3) - the lifting head's pose,
    the previous frame's fit - and init_ok (B, J; None: every joint) it also places joints that fewer than two cameras see; a joint the
    caller's init_ok leaves out starts from the triangulated point where that is valid (one torch.where between the launches).
    Nothing in the fit is differentiable; the triangulated pose and cost keep their gradients."""
    what = "decode.decode_joints_3d_skeleton"
    # (what the fit would refuse is refused before the soft-argmax runs)
    if heatmaps.dim() != 5 or not 2 <= heatmaps.shape[1] <= 4:
        raise ValueError(f"egorear_amd.{what}: heat maps must be (B, V, J, H, W) with 2 to 4 views, got {tuple(heatmaps.shape)}")
    B, J = int(heatmaps.shape[0]), int(heatmaps.shape[2])
    parents, _ = hip._skeleton_parameters(B, J, _parents_for(parents, J, "decode_joints_3d_skeleton"), bone_length, init,
                                          None if init_ok is None else _as_flags(init_ok), float(bone_weight), float(prior_weight),
                                          iterations, what, dense=False)
    hip._on_device(what, heatmaps, coord_trans_mat, bone_length, init, init_ok, exc=ValueError)
    joints3d, joints2d = decode_joints_3d(heatmaps, cameras, coord_trans_mat, beta, threshold, min_det_ratio, camera_calib_file_dir_path)
    H, W = int(heatmaps.shape[-2]), int(heatmaps.shape[-1])
    tri, tri_ok = joints3d.pose.detach(), joints3d.valid
    if init is None:
        start, start_ok = tri, tri_ok
    else:
        if init_ok is None:
            start, start_ok = init, torch.ones_like(tri_ok)
        else:
            mine = init_ok.view(torch.bool) if init_ok.dtype == torch.uint8 else init_ok
            start, start_ok = torch.where(mine.unsqueeze(-1), init, tri), mine | tri_ok
    fit = fit_skeleton(joints2d.soft.detach(), joints2d.maxvals.detach(), cameras, bone_length, start, start_ok, parents, coord_trans_mat,
                       (H, W), threshold, bone_weight, prior_weight, iterations, min_det_ratio, camera_calib_file_dir_path)
    return fit, joints3d, joints2d


# ---- temporal trajectory smoothing ---------------------------------------------------------------------------------------------------

@torch.library.custom_op("egorear_amd::trajectory_smooth", mutates_args=(), device_types="cuda")
def trajectory_smooth_op(pose: torch.Tensor, weight: Optional[torch.Tensor], obs: Optional[torch.Tensor], vel_weight: float,
                         accel_weight: float, huber: float, reweights: int, max_gap: int
                         ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(pose_out (N, T, J, 3) cm, valid (N, T, J) uint8, residual (N, T, J) cm, weight_out (N, T, J), energy (N, J)) of pose (N, T, J, 3),
    weight (N, T, J) or None, obs (N, T, J) uint8 or None: egr_trajectory_smooth_f32.  pose_out is differentiable with
    respect to pose and weight in the plain form (huber 0); with huber > 0 no output is."""
    hip._trajectory_operands(pose, weight, obs, vel_weight, accel_weight, huber, reweights, max_gap, "decode.trajectory_smooth", dense=False)
    return hip.trajectory_smooth(_c(pose), _c(weight), _c(obs), vel_weight, accel_weight, huber, reweights, max_gap)


@trajectory_smooth_op.register_fake
def _trajectory_smooth_fake(pose, weight, obs, vel_weight, accel_weight, huber, reweights, max_gap):
    N, T, J = hip._trajectory_operands(pose, weight, obs, vel_weight, accel_weight, huber, reweights, max_gap, "decode.trajectory_smooth",
                                       dense=False)
    new = pose.new_empty
    return new((N, T, J, 3)), new((N, T, J), dtype=torch.uint8), new((N, T, J)), new((N, T, J)), new((N, J))


@torch.library.custom_op("egorear_amd::trajectory_smooth_bwd", mutates_args=(), device_types="cuda")
def trajectory_smooth_bwd_op(pose: torch.Tensor, weight: Optional[torch.Tensor], obs: Optional[torch.Tensor], g_pose: torch.Tensor,
                             vel_weight: float, accel_weight: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(g_pose_in (N, T, J, 3), g_weight (N, T, J) - or (0,) without a weight) from the cotangent of pose_out: the plain form only."""
    gp = g_pose.to(torch.float32)
    hip._trajectory_operands(pose, weight, obs, vel_weight, accel_weight, 0.0, 0, 0, "decode.trajectory_smooth_bwd", gp, dense=False)
    g_in, g_weight = hip.trajectory_smooth_bwd(_c(pose), _c(weight), _c(obs), _c(gp), vel_weight, accel_weight)
    return g_in, pose.new_empty((0,)) if g_weight is None else g_weight


@trajectory_smooth_bwd_op.register_fake
def _trajectory_smooth_bwd_fake(pose, weight, obs, g_pose, vel_weight, accel_weight):
    N, T, J = hip._trajectory_operands(pose, weight, obs, vel_weight, accel_weight, 0.0, 0, 0, "decode.trajectory_smooth_bwd", g_pose,
                                       dense=False)
    return pose.new_empty((N, T, J, 3)), pose.new_empty((0,) if weight is None else (N, T, J))


def _trj_setup_context(ctx, inputs, output):
    pose, weight, obs, vel_weight, accel_weight, huber, _, _ = inputs
    ctx.has_weight, ctx.has_obs = weight is not None, obs is not None
    ctx.save_for_backward(*((pose,) + ((weight,) if ctx.has_weight else ()) + ((obs,) if ctx.has_obs else ())))
    ctx.args = (vel_weight, accel_weight)
    # (valid is not a floating-point tensor; with huber > 0 nothing is differentiable, as for the operators without a gradient)
    ctx.mark_non_differentiable(*(output[2:] if huber == 0.0 else (output[0],) + tuple(output[2:])))


def _trj_autograd(ctx, g_pose, g_valid, g_residual, g_weight_out, g_energy):
    rest = list(ctx.saved_tensors)
    pose = rest.pop(0)
    weight = rest.pop(0) if ctx.has_weight else None
    obs = rest.pop(0) if ctx.has_obs else None
    if g_pose is None:
        g_pose = torch.zeros_like(pose)
    g_in, g_weight = trajectory_smooth_bwd_op(pose, weight, obs, g_pose, *ctx.args)
    return g_in, (g_weight if ctx.has_weight else None), None, None, None, None, None, None


trajectory_smooth_op.register_autograd(_trj_autograd, setup_context=_trj_setup_context)


class Track3D(NamedTuple):
    pose: torch.Tensor       # (N, T, J, 3) cm: the smoothed track, written for every frame of a solvable track; 0 for the others
    valid: torch.Tensor      # (N, T, J) bool: the track is solvable and an observed frame is at most max_gap frames away
    residual: torch.Tensor   # (N, T, J) cm: |pose - observation| at observed frames, 0 elsewhere
    weight: torch.Tensor     # (N, T, J) the weights of the last solve: the base weight times the Huber factor
    energy: torch.Tensor     # (N, J) the energy at the result


def _trj_parameters(accel_weight, vel_weight, huber_cm, reweights, max_gap):
    try:
        return float(vel_weight), float(accel_weight), float(huber_cm), reweights, max_gap
    except (TypeError, ValueError):
        raise ValueError(f"egorear_amd.decode.smooth_trajectory: accel_weight, vel_weight and huber_cm must be numbers, got "
                         f"{accel_weight!r}, {vel_weight!r}, {huber_cm!r}") from None


def smooth_trajectory(pose: torch.Tensor, weight: Optional[torch.Tensor] = None, observed: Optional[torch.Tensor] = None,
                      accel_weight: float = 10.0, vel_weight: float = 0.0, huber_cm: float = 0.0, reweights: int = 0, max_gap: int = 8
                      ) -> Track3D:
    """pose (N, T, J, 3) cm - or (T, J, 3), one clip - with weight (N, T, J) (None: 1) and observed (N, T, J) bool / uint8 (None: every
    frame; `Joints3D.valid` plugs in) -> Track3D(pose, valid, residual, weight, energy): per joint of every clip the track that minimises
      sum_t w_t rho(|x_t - z_t|) + vel_weight sum |x_{t+1} - x_t|^2 + accel_weight sum |x_{t+1} - 2 x_t + x_{t-1}|^2
    over the frames, w_t = weight_t where the frame is observed and pose and weight are finite (weight > 0), else 0: such a frame is a
    gap, filled from its neighbours, and what stands in it is never read.  rho is the square, or with huber_cm > 0 Huber's function
    at that radius, minimised by `reweights` (1..16) rounds of iteratively reweighted least squares after the plain solve - a
    single-frame glitch is down-weighted instead of bending the track.  With vel_weight 0 a track needs two observed frames (every
    frame where T <= 2), else one; a track without them gives zeros and valid False.  A frame is valid when an observed frame is at
    most `max_gap` frames away; the pose is written for every frame regardless.  One launch.  In the plain form (huber_cm 0) the pose
    is differentiable with respect to pose and weight; with huber_cm > 0 nothing is."""
    vel_weight, accel_weight, huber_cm, reweights, max_gap = _trj_parameters(accel_weight, vel_weight, huber_cm, reweights, max_gap)
    one = pose.dim() == 3
    if one:
        pose = pose.unsqueeze(0)
        weight = None if weight is None else weight.unsqueeze(0)
        observed = None if observed is None else observed.unsqueeze(0)
    if observed is not None:
        observed = _as_flags(observed)
    hip._trajectory_operands(pose, weight, observed, vel_weight, accel_weight, huber_cm, reweights, max_gap, "decode.smooth_trajectory",
                             dense=False)
    hip._on_device("decode.smooth_trajectory", pose, weight, observed, exc=ValueError)
    out, valid, residual, used, energy = trajectory_smooth_op(pose, weight, observed, vel_weight, accel_weight, huber_cm, reweights, max_gap)
    track = Track3D(out, valid.view(torch.bool), residual, used, energy)
    return Track3D(*(t.squeeze(0) for t in track)) if one else track


def decode_clip_3d(heatmaps: torch.Tensor, cameras: Union[str, Sequence], coord_trans_mat: Optional[torch.Tensor] = None, beta: float = 100.0,
                   threshold: float = 0.5, min_det_ratio: float = 1e-6, camera_calib_file_dir_path: Optional[str] = None,
                   accel_weight: float = 10.0, vel_weight: float = 0.0, huber_cm: float = 0.0, reweights: int = 0, max_gap: int = 8
                   ) -> Tuple[Joints3D, Track3D]:
    """heatmaps (N, T, V, J, H, W) - or (T, V, J, H, W), one clip - -> (Joints3D, Track3D): `decode_joints_3d` on the N * T frames
    (soft-argmax, triangulation), then `smooth_trajectory` of its pose with observed = its valid flags - three launches with nothing
    between them, bit-identical to calling the pieces.  `coord_trans_mat` is (N, T, V, 4, 4) ((T, V, 4, 4) for one clip) or None.  A
    joint that fewer than two cameras see for some frames is a gap that the neighbouring frames fill (Track3D.valid says how far they
    are).  Both results come in the clip's shape: Joints3D fields (N, T, J, ...), Track3D as `smooth_trajectory` gives it.  In the plain
    form the gradient of Track3D.pose reaches the heat maps through the three backward operators."""
    what = "decode.decode_clip_3d"
    one = heatmaps.dim() == 5
    if one:
        heatmaps = heatmaps.unsqueeze(0)
        coord_trans_mat = None if coord_trans_mat is None else coord_trans_mat.unsqueeze(0)
    if heatmaps.dim() != 6 or not 2 <= heatmaps.shape[2] <= 4:
        raise ValueError(f"egorear_amd.{what}: heat maps must be (N, T, V, J, H, W) or (T, V, J, H, W) with 2 to 4 views, got "
                         f"{tuple(heatmaps.shape)}")
    N, T, V, J = (int(v) for v in heatmaps.shape[:4])
    if coord_trans_mat is not None and tuple(coord_trans_mat.shape) != (N, T, V, 4, 4):
        raise ValueError(f"egorear_amd.{what}: coord_trans_mat must be {(N, T, V, 4, 4)}, got {tuple(coord_trans_mat.shape)}")
    # (what the smoother would refuse is refused before the soft-argmax runs)
    vel_weight, accel_weight, huber_cm, reweights, max_gap = _trj_parameters(accel_weight, vel_weight, huber_cm, reweights, max_gap)
    hip._trajectory_operands(heatmaps.new_empty((N, T, J, 3), device="meta"), None, None, vel_weight, accel_weight, huber_cm, reweights,
                             max_gap, what, dense=False)
    hip._on_device(what, heatmaps, coord_trans_mat, exc=ValueError)
    frames = heatmaps.reshape((N * T,) + tuple(heatmaps.shape[2:]))
    ctm = None if coord_trans_mat is None else coord_trans_mat.reshape(N * T, V, 4, 4)
    joints3d, _ = decode_joints_3d(frames, cameras, ctm, beta, threshold, min_det_ratio, camera_calib_file_dir_path)
    track = smooth_trajectory(joints3d.pose.view(N, T, J, 3), None, joints3d.valid.view(N, T, J), accel_weight, vel_weight, huber_cm,
                              reweights, max_gap)
    clip = Joints3D(joints3d.pose.view(N, T, J, 3), joints3d.cost.view(N, T, J), joints3d.residual.view(N, T, V, J), joints3d.valid.view(N, T, J))
    if one:
        clip, track = Joints3D(*(t.squeeze(0) for t in clip)), Track3D(*(t.squeeze(0) for t in track))
    return clip, track


# ---- causal fixed-lag filtering of a stream ------------------------------------------------------------------------------------------

@torch.library.custom_op("egorear_amd::trajectory_filter", mutates_args=("state",), device_types="cuda")
def trajectory_filter_op(state: torch.Tensor, pose: torch.Tensor, weight: Optional[torch.Tensor], obs: Optional[torch.Tensor],
                         reset: Optional[torch.Tensor], lag: int, vel_weight: float, accel_weight: float, gate: float, max_gap: int
                         ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(pose_out (N, C, J, 3) cm, valid (N, C, J) uint8, residual (N, C, J) cm, weight_out (N, C, J), frame (N, C) int64) of the next C
    frames pose (N, C, J, 3) of N streams, weight / obs (N, C, J) or None, reset (N,) uint8 or None; `state` (slots, N * J) float64 is
    updated in place: egr_trajectory_filter_f32.  No output is differentiable."""
    hip._filter_operands(state, pose, weight, obs, reset, lag, vel_weight, accel_weight, gate, max_gap, "decode.trajectory_filter", dense=False)
    return hip.trajectory_filter(state, _c(pose), _c(weight), _c(obs), _c(reset), lag, vel_weight, accel_weight, gate, max_gap)


def _filter_fake_outputs(like, N, R, J):
    new = like.new_empty
    return (new((N, R, J, 3), dtype=torch.float32), new((N, R, J), dtype=torch.uint8), new((N, R, J), dtype=torch.float32),
            new((N, R, J), dtype=torch.float32), new((N, R), dtype=torch.int64))


@trajectory_filter_op.register_fake
def _trajectory_filter_fake(state, pose, weight, obs, reset, lag, vel_weight, accel_weight, gate, max_gap):
    N, C, J = hip._filter_operands(state, pose, weight, obs, reset, lag, vel_weight, accel_weight, gate, max_gap, "decode.trajectory_filter",
                                   dense=False)
    return _filter_fake_outputs(pose, N, C, J)


@torch.library.custom_op("egorear_amd::trajectory_filter_tail", mutates_args=(), device_types="cuda")
def trajectory_filter_tail_op(state: torch.Tensor, N: int, J: int, lag: int, vel_weight: float, accel_weight: float, max_gap: int
                              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The five outputs of trajectory_filter for the last `lag` frames of the streams so far, (N, lag, J, ...): egr_trajectory_filter_tail_f32.
    The state is read only."""
    return hip.trajectory_filter_tail(state, N, J, lag, vel_weight, accel_weight, max_gap)


@trajectory_filter_tail_op.register_fake
def _trajectory_filter_tail_fake(state, N, J, lag, vel_weight, accel_weight, max_gap):
    slots = hip._filter_parameters("decode.trajectory_filter_tail", N, J, lag, vel_weight, accel_weight, 0.0, max_gap)
    hip._filter_state("decode.trajectory_filter_tail", state, N, J, slots)
    return _filter_fake_outputs(state, N, lag, J)


# Not differentiable, as consensus_op: the tail by the same registration; the step mutates its state, and an operator that is not
# functional takes no autograd formula - `filter_trajectory` hands it detached operands instead.  (A direct call of the operator with
# operands that require a gradient is not refused at the call: it fails at backward.)
trajectory_filter_tail_op.register_autograd(_nograd_autograd, setup_context=_nograd_setup_context)


class TrackFilterState(NamedTuple):
    tensor: torch.Tensor     # (slots, N * J) float64 on the device, updated in place by every step (include/egorear_hip.h has the layout)
    N: int                   # streams
    J: int                   # joints of a stream
    lag: int                 # frames an output lies behind the arriving frame
    accel_weight: float
    vel_weight: float
    gate_cm: float           # 0: no gate
    max_gap: int


class TrackStep(NamedTuple):
    pose: torch.Tensor       # (N, C, J, 3) cm: stream frame `frame` of the track over the frames seen so far; 0 where that is not solvable
    valid: torch.Tensor      # (N, C, J) bool: solvable and an observed frame among those seen is at most max_gap frames away
    residual: torch.Tensor   # (N, C, J) cm: |pose - observation| if that frame was observed, else 0
    weight: torch.Tensor     # (N, C, J) the weight that frame's observation was given: the base weight times the gate's factor
    frame: torch.Tensor      # (N, C) int64: the stream frame a row describes; -1 (and zeros) where there is none yet


def _filter_parameters(what, accel_weight, vel_weight, gate_cm, max_gap):
    try:
        return float(vel_weight), float(accel_weight), float(gate_cm), max_gap
    except (TypeError, ValueError):
        raise ValueError(f"egorear_amd.{what}: accel_weight, vel_weight and gate_cm must be numbers, got {accel_weight!r}, {vel_weight!r}, "
                         f"{gate_cm!r}") from None


def new_track_filter(N: int, J: int, lag: int, device, accel_weight: float = 10.0, vel_weight: float = 0.0, gate_cm: float = 0.0,
                     max_gap: int = 8) -> TrackFilterState:
    """The empty state of N streams of J joints for `filter_trajectory` / `decode_stream_3d`: outputs lie `lag` (0..64) frames behind
    the arriving frame; the penalties and `max_gap` are `smooth_trajectory`'s; with gate_cm > 0 an arriving observation farther than
    that from what the earlier frames predict for it is down-weighted by Huber's factor."""
    what = "decode.new_track_filter"
    vel_weight, accel_weight, gate_cm, max_gap = _filter_parameters(what, accel_weight, vel_weight, gate_cm, max_gap)
    hip._filter_parameters(what, N, J, lag, vel_weight, accel_weight, gate_cm, max_gap)
    if torch.device(device).type not in ("cuda", "meta"):
        raise ValueError(f"egorear_amd.{what}: no CPU path - the state must live on the HIP device")
    return TrackFilterState(hip.trajectory_filter_state(N, J, lag, device), N, J, lag, accel_weight, vel_weight, gate_cm, max_gap)


def _filter_state(what: str, state) -> Tuple[float, float, float, int]:
    if not isinstance(state, TrackFilterState) or not isinstance(state.tensor, torch.Tensor):
        raise ValueError(f"egorear_amd.{what}: state must be a TrackFilterState (new_track_filter), got {type(state).__name__}")
    vel_weight, accel_weight, gate_cm, max_gap = _filter_parameters(what, state.accel_weight, state.vel_weight, state.gate_cm, state.max_gap)
    slots = hip._filter_parameters(what, state.N, state.J, state.lag, vel_weight, accel_weight, gate_cm, max_gap)
    hip._filter_state(what, state.tensor, state.N, state.J, slots)
    return vel_weight, accel_weight, gate_cm, max_gap


def filter_trajectory(state: TrackFilterState, pose: torch.Tensor, weight: Optional[torch.Tensor] = None,
                      observed: Optional[torch.Tensor] = None, reset: Optional[torch.Tensor] = None) -> TrackStep:
    """The next frames of the streams of `state`: pose (N, C, J, 3) cm - or (N, J, 3), one frame - with weight (N, C, J) (None: 1),
    observed (N, C, J) bool / uint8 (None: every frame; `Joints3D.valid` plugs in) and reset (N,) bool / uint8 (a stream so marked
    starts anew with this call's first frame) -> TrackStep(pose, valid, residual, weight, frame).  The causal, fixed-lag form of
    `smooth_trajectory`: row c is frame t - lag of the track that `smooth_trajectory`'s plain form gives over the frames 0..t seen so
    far, t the frame arriving in row c - every frame costs the same, however long the stream.  With the state's gate_cm > 0 an
    observation's weight is first multiplied by min(1, gate_cm / its distance from the prediction of the earlier frames).  The state is
    updated in place; the result does not depend on how a stream is cut into calls.  One launch; nothing is differentiable."""
    what = "decode.filter_trajectory"
    vel_weight, accel_weight, gate_cm, max_gap = _filter_state(what, state)
    one = pose.dim() == 3
    if one:
        pose = pose.unsqueeze(1)
        weight = None if weight is None else weight.unsqueeze(1)
        observed = None if observed is None else observed.unsqueeze(1)
    if observed is not None:
        observed = _as_flags(observed)
    if reset is not None:
        reset = _as_flags(reset)
    N, _, J = hip._filter_operands(state.tensor, pose, weight, observed, reset, state.lag, vel_weight, accel_weight, gate_cm, max_gap, what,
                                   dense=False)
    if (N, J) != (state.N, state.J):
        raise ValueError(f"egorear_amd.{what}: the state was made for {state.N} streams of {state.J} joints, got pose {tuple(pose.shape)}")
    hip._on_device(what, state.tensor, pose, weight, observed, reset, exc=ValueError)
    out, valid, residual, used, frame = trajectory_filter_op(state.tensor, pose.detach(), None if weight is None else weight.detach(), observed,
                                                             reset, state.lag, vel_weight, accel_weight, gate_cm, max_gap)
    step = TrackStep(out, valid.view(torch.bool), residual, used, frame)
    return TrackStep(*(t.squeeze(1) for t in step)) if one else step


def filter_tail(state: TrackFilterState) -> TrackStep:
    """The last `lag` frames of the streams so far, which no step has described yet, as TrackStep with rows (N, lag, J, ...): the frames
    T - lag .. T - 1 of the track over all T frames seen (a row before the stream's start: frame -1 and zeros).  At the end of a stream
    it completes the output; at any time its last row is the causal estimate of the present.  The state is not modified.  One launch."""
    what = "decode.filter_tail"
    vel_weight, accel_weight, _, max_gap = _filter_state(what, state)
    hip._on_device(what, state.tensor, exc=ValueError)
    out, valid, residual, used, frame = trajectory_filter_tail_op(state.tensor, state.N, state.J, state.lag, vel_weight, accel_weight, max_gap)
    return TrackStep(out, valid.view(torch.bool), residual, used, frame)


def decode_stream_3d(state: TrackFilterState, heatmaps: torch.Tensor, cameras: Union[str, Sequence],
                     coord_trans_mat: Optional[torch.Tensor] = None, beta: float = 100.0, threshold: float = 0.5, min_det_ratio: float = 1e-6,
                     camera_calib_file_dir_path: Optional[str] = None) -> Tuple[Joints3D, TrackStep]:
    """heatmaps (N, C, V, J, H, W) - or (N, V, J, H, W), one frame - -> (Joints3D, TrackStep): `decode_joints_3d` on the N * C frames, then
    `filter_trajectory` of its pose with observed = its valid flags - three launches with nothing between them, bit-identical to calling
    the pieces, and no host value takes part: the call can be captured into one graph and replayed for every frame.  `coord_trans_mat`
    is (N, C, V, 4, 4) ((N, V, 4, 4) for one frame) or None.  Joints3D comes in the call's shape, (N, C, J, ...) or (N, J, ...)."""
    what = "decode.decode_stream_3d"
    _filter_state(what, state)
    one = heatmaps.dim() == 5
    if one:
        heatmaps = heatmaps.unsqueeze(1)
        coord_trans_mat = None if coord_trans_mat is None else coord_trans_mat.unsqueeze(1)
    if heatmaps.dim() != 6 or not 2 <= heatmaps.shape[2] <= 4:
        raise ValueError(f"egorear_amd.{what}: heat maps must be (N, C, V, J, H, W) or (N, V, J, H, W) with 2 to 4 views, got "
                         f"{tuple(heatmaps.shape)}")
    N, C, V, J = (int(v) for v in heatmaps.shape[:4])
    if (N, J) != (state.N, state.J):
        raise ValueError(f"egorear_amd.{what}: the state was made for {state.N} streams of {state.J} joints, got heat maps "
                         f"{tuple(heatmaps.shape)}")
    if coord_trans_mat is not None and tuple(coord_trans_mat.shape) != (N, C, V, 4, 4):
        raise ValueError(f"egorear_amd.{what}: coord_trans_mat must be {(N, C, V, 4, 4)}, got {tuple(coord_trans_mat.shape)}")
    hip._on_device(what, state.tensor, heatmaps, coord_trans_mat, exc=ValueError)
    frames = heatmaps.reshape((N * C,) + tuple(heatmaps.shape[2:]))
    ctm = None if coord_trans_mat is None else coord_trans_mat.reshape(N * C, V, 4, 4)
    joints3d, _ = decode_joints_3d(frames, cameras, ctm, beta, threshold, min_det_ratio, camera_calib_file_dir_path)
    step = filter_trajectory(state, joints3d.pose.view(N, C, J, 3), None, joints3d.valid.view(N, C, J))
    seen = Joints3D(joints3d.pose.view(N, C, J, 3), joints3d.cost.view(N, C, J), joints3d.residual.view(N, C, V, J), joints3d.valid.view(N, C, J))
    if one:
        seen, step = Joints3D(*(t.squeeze(1) for t in seen)), TrackStep(*(t.squeeze(1) for t in step))
    return seen, step


# ---- rig self-calibration ------------------------------------------------------------------------------------------------------------

@torch.library.custom_op("egorear_amd::rig_refine", mutates_args=(), device_types="cuda")
def rig_refine_op(coords: torch.Tensor, conf: torch.Tensor, cams: torch.Tensor, ctm: Optional[torch.Tensor], fixed: Sequence[int], sx: float,
                  sy: float, threshold: float, min_det_ratio: float, prior_weight: float, iterations: int
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
                             torch.Tensor]:
    """(rotation (V, 3) rad, matrix (V, 3, 3), coord_trans_mat (B, V, 4, 4), cost0 (1), cost (1), pairs (1) int32, steps (1) int32,
    grad (1), valid (1) uint8) of the triangulation's operands - ctm (B, V, 4, 4), (1, V, 4, 4) or None - and V flags, the held cameras:
    egr_rig_refine_f32.  No output is differentiable."""
    hip._rig_operands(coords, conf, cams, ctm, fixed, sx, sy, min_det_ratio, prior_weight, iterations, "decode.rig_refine", dense=False)
    return hip.rig_refine(_c(coords), _c(conf), _c(cams), _c(ctm), fixed, sx, sy, threshold, min_det_ratio, prior_weight, iterations)


@rig_refine_op.register_fake
def _rig_refine_fake(coords, conf, cams, ctm, fixed, sx, sy, threshold, min_det_ratio, prior_weight, iterations):
    B, V, J, _, _ = hip._rig_operands(coords, conf, cams, ctm, fixed, sx, sy, min_det_ratio, prior_weight, iterations, "decode.rig_refine",
                                      dense=False)
    new = coords.new_empty
    return (new((V, 3)), new((V, 3, 3)), new((B, V, 4, 4)), new((1,)), new((1,)), new((1,), dtype=torch.int32), new((1,), dtype=torch.int32),
            new((1,)), new((1,), dtype=torch.uint8))


rig_refine_op.register_autograd(_nograd_autograd, setup_context=_nograd_setup_context)


class RigFit(NamedTuple):
    rotation: torch.Tensor          # (V, 3) rotation vector of every camera's correction, rad; 0 for a held camera
    matrix: torch.Tensor            # (V, 3, 3) the same as matrices dR: p_cam' = dR (R p + t)
    coord_trans_mat: torch.Tensor   # (B, V, 4, 4) [dR 0; 0 1] M: what every decode function takes with the same `cameras`
    cost0: torch.Tensor             # () weighted mean squared ray distance over the counted pairs at the given rig, cm^2
    cost: torch.Tensor              # () the same at the result, <= cost0
    pairs: torch.Tensor             # () int32 (frame, joint) pairs that counted
    steps: torch.Tensor             # () int32 iterations whose step was kept
    grad: torch.Tensor              # () largest |dE/d rotation| component over the free cameras at the result
    valid: torch.Tensor             # () bool: false when no pair counts or the clip does not fix the rotations (then: the identity)


def refine_rig(coords: torch.Tensor, conf: torch.Tensor, cameras: Union[str, Sequence], coord_trans_mat: Optional[torch.Tensor] = None,
               heatmap_size: Tuple[float, float] = (64, 64), threshold: float = 0.5, min_det_ratio: float = 1e-6, fixed=None,
               prior_weight: float = 0.0, iterations: int = 8, camera_calib_file_dir_path: Optional[str] = None) -> RigFit:
    """coords (B, V, J, 2), conf (B, V, J) of a clip, `cameras`, `heatmap_size`, `threshold`, `min_det_ratio` as for
    `triangulate_joints`; `coord_trans_mat` None (the ego4view_syn rig), (B, V, 4, 4) per frame or (1, V, 4, 4) for the clip
    -> RigFit: per camera the rotation about its own centre that makes the views' rays meet best over the whole clip,
      sum over (frame, joint) of min_p sum_v conf_v dist^2(p, ray_v rotated) + prior_weight * sum_v |dR_v - I|_F^2,
    minimised over the cameras that are not `fixed` (V flags or a (V,) bool tensor in host memory; None holds view 0 alone, which
    removes the rig's common rotation; all held is legal and returns the identity).  Rotations are what drifts on a head-mounted rig
    and what this cost can see: translations are not refined - scaling the camera centres and the points together shrinks every ray
    distance, so free translations would collapse the rig.  A pair counts when the triangulation at the given rig is valid for it.
    `iterations` (1..256) Levenberg-Marquardt steps are tried, always; convergence is quadratic where the rays can meet (4 to 6 reach
    fp32 stationarity from 0.03 rad) and `grad` reports how stationary the result is.  `RigFit.coord_trans_mat` goes to every decode
    function in place of the given one.  Coordinate noise biases the fit - rays that meet closer to the cameras miss by less - by
    about 0.8 rad per squared heat-map pixel however long the clip: the joints should be better than 0.15 px for a
    0.03 rad drift, or `prior_weight` should hold the fit near the given rig.  Outliers are the caller's business: `select_consistent` yields coords / conf with out-voted
    views at zero confidence, which this function excludes like any view below `threshold`; there is no second robust scheme here.
    1 + 2 (iterations + 1) launches, no host synchronisation, bit-reproducible; nothing here is differentiable."""
    sx, sy = _scales(heatmap_size)
    cams = _ray_records(cameras, camera_calib_file_dir_path, coords.device)
    if coords.dim() != 4:
        raise ValueError(f"egorear_amd.decode.refine_rig: coords must be (B, V, J, 2), got {tuple(coords.shape)}")
    flags = [int(f) for f in hip._rig_operands(coords, conf, cams, coord_trans_mat, fixed, sx, sy, float(min_det_ratio), float(prior_weight),
                                               iterations, "decode.refine_rig", dense=False)[3]]
    hip._on_device("decode.refine_rig", coords, conf, coord_trans_mat, exc=ValueError)
    rotation, matrix, ctm, cost0, cost, pairs, steps, grad, valid = rig_refine_op(
        coords, conf, cams, coord_trans_mat, flags, sx, sy, float(threshold), float(min_det_ratio), float(prior_weight), iterations)
    return RigFit(rotation, matrix, ctm, cost0.view(()), cost.view(()), pairs.view(()), steps.view(()), grad.view(()),
                  valid.view(torch.bool).view(()))


def apply_rig_correction(matrix: torch.Tensor, cameras: Union[str, Sequence], coord_trans_mat: Optional[torch.Tensor], B: int,
                         camera_calib_file_dir_path: Optional[str] = None) -> torch.Tensor:
    """`RigFit.matrix` (V, 3, 3) of one clip applied to the rig of another: [dR 0; 0 1] M_v as fp32 (B, V, 4, 4), M the given
    `coord_trans_mat` ((B, V, 4, 4) or (1, V, 4, 4)) or, for None, the ego4view_syn rig written as matrices (the flip on the diagonal,
    the offsets in m, fp32) - the composition `refine_rig` returns, bit for bit, alone: float64 torch operations rounded once.  Not
    differentiable."""
    what = "decode.apply_rig_correction"
    if matrix.dim() != 3 or tuple(matrix.shape[1:]) != (3, 3) or not 2 <= matrix.shape[0] <= 4 or matrix.dtype != torch.float32:
        raise ValueError(f"egorear_amd.{what}: matrix must be a float32 (V, 3, 3) with 2 to 4 views, got {matrix.dtype} {tuple(matrix.shape)}")
    V = int(matrix.shape[0])
    if isinstance(B, bool) or not isinstance(B, int) or B < 1:
        raise ValueError(f"egorear_amd.{what}: B must be a positive integer, got {B!r}")
    if coord_trans_mat is not None and (tuple(coord_trans_mat.shape) not in ((B, V, 4, 4), (1, V, 4, 4)) or coord_trans_mat.dtype != torch.float32):
        raise ValueError(f"egorear_amd.{what}: coord_trans_mat must be a float32 {(B, V, 4, 4)} or {(1, V, 4, 4)}, got "
                         f"{coord_trans_mat.dtype} {tuple(coord_trans_mat.shape)}")
    hip._on_device(what, matrix, coord_trans_mat, exc=ValueError)
    with torch.no_grad():
        if coord_trans_mat is None:
            rec = _ray_records(cameras, camera_calib_file_dir_path, matrix.device).double()
            if tuple(rec.shape) != (V, hip.RAY_REC):
                raise ValueError(f"egorear_amd.{what}: {V} matrices for {rec.shape[0]} cameras")
            f = 1.0 - 2.0 * (rec[:, 26] != 0).double()
            m = torch.diag_embed(torch.stack((f, f, torch.ones_like(f), torch.ones_like(f)), -1))
            m[:, :3, 3] = (rec[:, 27:30] * 0.01).float().double()        # (fp32, as a caller would pass the rig)
            m = m.unsqueeze(0)
        else:
            m = coord_trans_mat.double()
        left = torch.zeros((V, 4, 4), dtype=torch.float64, device=matrix.device)
        left[:, :3, :3] = matrix.double()
        left[:, 3, 3] = 1.0
        out = (left.unsqueeze(0).unsqueeze(-1) * m.unsqueeze(-3)).sum(-2)
        return out.expand(B, V, 4, 4).float().contiguous()


def calibrate_rig(heatmaps: torch.Tensor, cameras: Union[str, Sequence], coord_trans_mat: Optional[torch.Tensor] = None, beta: float = 100.0,
                  threshold: float = 0.5, min_det_ratio: float = 1e-6, fixed=None, prior_weight: float = 0.0, iterations: int = 8,
                  camera_calib_file_dir_path: Optional[str] = None) -> Tuple[RigFit, Joints2D]:
    """heatmaps (B, V, J, H, W) of a clip -> (RigFit, Joints2D): `decode_joints_2d` (soft-argmax at `beta`), then `refine_rig` on its
    sub-pixel joints weighted by the maps' maxima, with nothing on the host in between - bit-identical to calling the two."""
    what = "decode.calibrate_rig"
    # (the soft-argmax takes any V: what the fit would refuse is refused before it runs)
    if heatmaps.dim() != 5 or not 2 <= heatmaps.shape[1] <= 4:
        raise ValueError(f"egorear_amd.{what}: heat maps must be (B, V, J, H, W) with 2 to 4 views, got {tuple(heatmaps.shape)}")
    _check(heatmaps, float(beta), MODE_SOFTMAX, dims=5, what="calibrate_rig")
    B, V, J, H, W = (int(v) for v in heatmaps.shape)
    cams = _ray_records(cameras, camera_calib_file_dir_path, heatmaps.device)
    hip._rig_operands(heatmaps.new_empty((B, V, J, 2), device="meta"), heatmaps.new_empty((B, V, J), device="meta"), cams, coord_trans_mat, fixed,
                      1.0 / W, 1.0 / H, float(min_det_ratio), float(prior_weight), iterations, what, dense=False)
    hip._on_device(what, heatmaps, coord_trans_mat, exc=ValueError)
    joints2d = decode_joints_2d(heatmaps, beta=beta, threshold=threshold)
    fit = refine_rig(joints2d.soft.detach(), joints2d.maxvals.detach(), cameras, coord_trans_mat, (H, W), threshold, min_det_ratio, fixed,
                     prior_weight, iterations, camera_calib_file_dir_path)
    return fit, joints2d


# ---- ray-space clip smoothing --------------------------------------------------------------------------------------------------------

@torch.library.custom_op("egorear_amd::ray_track", mutates_args=(), device_types="cuda")
def ray_track_op(coords: torch.Tensor, conf: torch.Tensor, cams: torch.Tensor, ctm: Optional[torch.Tensor], sx: float, sy: float,
                 threshold: float, vel_weight: float, accel_weight: float, huber: float, reweights: int, max_gap: int, min_pivot_ratio: float
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(pose (N, T, J, 3) cm, valid (N, T, J) uint8, residual (N, T, V, J) cm, weight (N, T, V, J), rays (N, T, J) uint8, energy (N, J)) of
    coords (N, T, V, J, 2) * (sx, sy) = normalised image points, conf (N, T, V, J), cams (V, 30), ctm (N, T, V, 4, 4) or None:
    egr_ray_track_f32.  No output is differentiable."""
    hip._ray_track_operands(coords, conf, cams, ctm, sx, sy, threshold, vel_weight, accel_weight, huber, reweights, max_gap, min_pivot_ratio,
                            "decode.ray_track", dense=False)
    return hip.ray_track(_c(coords), _c(conf), _c(cams), _c(ctm), sx, sy, threshold, vel_weight, accel_weight, huber, reweights, max_gap,
                         min_pivot_ratio)


@ray_track_op.register_fake
def _ray_track_fake(coords, conf, cams, ctm, sx, sy, threshold, vel_weight, accel_weight, huber, reweights, max_gap, min_pivot_ratio):
    N, T, V, J = hip._ray_track_operands(coords, conf, cams, ctm, sx, sy, threshold, vel_weight, accel_weight, huber, reweights, max_gap,
                                         min_pivot_ratio, "decode.ray_track", dense=False)
    new = coords.new_empty
    return (new((N, T, J, 3)), new((N, T, J), dtype=torch.uint8), new((N, T, V, J)), new((N, T, V, J)), new((N, T, J), dtype=torch.uint8),
            new((N, J)))


ray_track_op.register_autograd(_nograd_autograd, setup_context=_nograd_setup_context)


class RayTrack3D(NamedTuple):
    pose: torch.Tensor       # (N, T, J, 3) cm: the fitted track, written for every frame of a solvable track; 0 for the others
    valid: torch.Tensor      # (N, T, J) bool: the track is solvable and a frame with a used ray is at most max_gap frames away
    residual: torch.Tensor   # (N, T, V, J) cm: the distance of the pose from each used ray, 0 elsewhere
    weight: torch.Tensor     # (N, T, V, J) the ray weights of the last solve: conf times the Huber factor, 0 for a ray that is not used
    rays: torch.Tensor       # (N, T, J) uint8 the number of used rays of the frame
    energy: torch.Tensor     # (N, J) the energy at the result


def fit_ray_tracks(coords: torch.Tensor, conf: torch.Tensor, cameras: Union[str, Sequence], coord_trans_mat: Optional[torch.Tensor] = None,
                   heatmap_size: Tuple[float, float] = (64, 64), threshold: float = 0.5, accel_weight: float = 10.0, vel_weight: float = 0.0,
                   huber_cm: float = 0.0, reweights: int = 0, max_gap: int = 8, min_pivot_ratio: float = 1e-10,
                   camera_calib_file_dir_path: Optional[str] = None) -> RayTrack3D:
    """coords (N, T, V, J, 2) - or (T, V, J, 2), one clip - and conf (N, T, V, J) of a clip, `cameras`, `heatmap_size`, `threshold` as for
    `triangulate_joints`, `coord_trans_mat` (N, T, V, 4, 4) ((T, V, 4, 4) for one clip) or None -> RayTrack3D(pose, valid, residual,
    weight, rays, energy): per joint of every clip the track that minimises
      sum_t sum_v w_tv rho(dist(x_t, ray_tv)) + vel_weight sum |x_{t+1} - x_t|^2 + accel_weight sum |x_{t+1} - 2 x_t + x_{t-1}|^2,
    w_tv = conf where the view is used, else 0 - the triangulation and the smoother in one problem, so that a frame one camera sees
    contributes its ray (two of the point's three degrees of freedom) instead of being a gap, a near-parallel pair keeps what it
    measures well while the penalty fixes the depth, and with huber_cm > 0 (`reweights` 1..16 rounds of IRLS after the plain solve) a
    single bad view is down-weighted while the frame's other rays stay.  A frame without a used ray is filled from its neighbours.  A
    track is solvable when it has enough rays for the penalty's null space (2 with vel_weight > 0; else 3 on 2 frames, or 2 in every
    frame where T <= 2) and no pivot of its elimination falls to `min_pivot_ratio` of its largest diagonal entry; one that is not
    gives zeros and valid False.  A frame is valid when a frame with a used ray is at most `max_gap` frames away.  Two launches;
    nothing here is differentiable."""
    what = "decode.fit_ray_tracks"
    sx, sy = _scales(heatmap_size)
    vel_weight, accel_weight, huber_cm, reweights, max_gap = _trj_parameters(accel_weight, vel_weight, huber_cm, reweights, max_gap)
    one = coords.dim() == 4
    if one:
        coords, conf = coords.unsqueeze(0), conf.unsqueeze(0) if conf.dim() == 3 else conf
        coord_trans_mat = None if coord_trans_mat is None else coord_trans_mat.unsqueeze(0)
    cams = _ray_records(cameras, camera_calib_file_dir_path, coords.device)
    hip._ray_track_operands(coords, conf, cams, coord_trans_mat, sx, sy, threshold, vel_weight, accel_weight, huber_cm, reweights, max_gap,
                            min_pivot_ratio, what, dense=False)
    hip._on_device(what, coords, conf, coord_trans_mat, exc=ValueError)
    pose, valid, residual, weight, rays, energy = ray_track_op(coords, conf, cams, coord_trans_mat, sx, sy, float(threshold), vel_weight,
                                                               accel_weight, huber_cm, reweights, max_gap, float(min_pivot_ratio))
    track = RayTrack3D(pose, valid.view(torch.bool), residual, weight, rays, energy)
    return RayTrack3D(*(t.squeeze(0) for t in track)) if one else track


def decode_clip_3d_rays(heatmaps: torch.Tensor, cameras: Union[str, Sequence], coord_trans_mat: Optional[torch.Tensor] = None,
                        beta: float = 100.0, threshold: float = 0.5, accel_weight: float = 10.0, vel_weight: float = 0.0, huber_cm: float = 0.0,
                        reweights: int = 0, max_gap: int = 8, min_pivot_ratio: float = 1e-10,
                        camera_calib_file_dir_path: Optional[str] = None) -> Tuple[Joints2D, RayTrack3D]:
    """heatmaps (N, T, V, J, H, W) - or (T, V, J, H, W), one clip - -> (Joints2D, RayTrack3D): `decode_joints_2d` on the N * T frames
    (soft-argmax), then `fit_ray_tracks` of its sub-pixel joints weighted by the maps' maxima - the soft-argmax launch and the two of
    the fit with nothing between them, bit-identical to calling the pieces.  No per-frame triangulation happens: a joint one camera
    sees is a ray, not a gap.  Both results come in the clip's shape: Joints2D fields (N, T, V, J, ...).  Not differentiable."""
    what = "decode.decode_clip_3d_rays"
    one = heatmaps.dim() == 5
    if one:
        heatmaps = heatmaps.unsqueeze(0)
        coord_trans_mat = None if coord_trans_mat is None else coord_trans_mat.unsqueeze(0)
    if heatmaps.dim() != 6 or not 2 <= heatmaps.shape[2] <= 4:
        raise ValueError(f"egorear_amd.{what}: heat maps must be (N, T, V, J, H, W) or (T, V, J, H, W) with 2 to 4 views, got "
                         f"{tuple(heatmaps.shape)}")
    _check(heatmaps, float(beta), MODE_SOFTMAX, dims=6, what="decode_clip_3d_rays")
    N, T, V, J, H, W = (int(v) for v in heatmaps.shape)
    # (what the fit would refuse is refused before the soft-argmax runs)
    vel_weight, accel_weight, huber_cm, reweights, max_gap = _trj_parameters(accel_weight, vel_weight, huber_cm, reweights, max_gap)
    cams = _ray_records(cameras, camera_calib_file_dir_path, heatmaps.device)
    hip._ray_track_operands(heatmaps.new_empty((N, T, V, J, 2), device="meta"), heatmaps.new_empty((N, T, V, J), device="meta"), cams,
                            coord_trans_mat, 1.0 / W, 1.0 / H, threshold, vel_weight, accel_weight, huber_cm, reweights, max_gap, min_pivot_ratio,
                            what, dense=False)
    hip._on_device(what, heatmaps, coord_trans_mat, exc=ValueError)
    flat = decode_joints_2d(heatmaps.reshape((N * T, V, J, H, W)), beta=beta, threshold=threshold)
    joints2d = Joints2D(flat.soft.view(N, T, V, J, 2), flat.hard.view(N, T, V, J, 2), flat.maxvals.view(N, T, V, J), flat.valid.view(N, T, V, J))
    track = fit_ray_tracks(joints2d.soft.detach(), joints2d.maxvals.detach(), cameras, coord_trans_mat, (H, W), threshold, accel_weight,
                           vel_weight, huber_cm, reweights, max_gap, min_pivot_ratio, camera_calib_file_dir_path)
    if one:
        joints2d, track = Joints2D(*(t.squeeze(0) for t in joints2d)), RayTrack3D(*(t.squeeze(0) for t in track))
    return joints2d, track


# ---- information-weighted clip smoothing ---------------------------------------------------------------------------------------------

@torch.library.custom_op("egorear_amd::joint_info", mutates_args=(), device_types="cuda")
def joint_info_op(points: torch.Tensor, conf: torch.Tensor, cams: torch.Tensor, ctm: Optional[torch.Tensor], sx: float, sy: float,
                  threshold: float, min_det_ratio: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(info (B, J, 6), views (B, J) uint8, sigma (B, J), valid (B, J) uint8) of points (B, J, 3) cm, conf (B, V, J), cams (V, 30), ctm
    (B, V, 4, 4) or None: egr_joint_info_f32.  No output is differentiable."""
    hip._joint_info_operands(points, conf, cams, ctm, sx, sy, threshold, min_det_ratio, "decode.joint_info", dense=False)
    return hip.joint_info(_c(points), _c(conf), _c(cams), _c(ctm), sx, sy, threshold, min_det_ratio)


@joint_info_op.register_fake
def _joint_info_fake(points, conf, cams, ctm, sx, sy, threshold, min_det_ratio):
    B, _, J = hip._joint_info_operands(points, conf, cams, ctm, sx, sy, threshold, min_det_ratio, "decode.joint_info", dense=False)
    new = points.new_empty
    return new((B, J, 6)), new((B, J), dtype=torch.uint8), new((B, J)), new((B, J), dtype=torch.uint8)


@torch.library.custom_op("egorear_amd::info_track", mutates_args=(), device_types="cuda")
def info_track_op(pose: torch.Tensor, info: torch.Tensor, obs: Optional[torch.Tensor], vel_weight: float, accel_weight: float, huber: float,
                  reweights: int, max_gap: int, min_pivot_ratio: float
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(pose_out (N, T, J, 3) cm, valid (N, T, J) uint8, residual (N, T, J) in coordinate units, weight (N, T, J), energy (N, J)) of pose
    (N, T, J, 3), info (N, T, J, 6), obs (N, T, J) uint8 or None: egr_info_track_f32.  No output is differentiable."""
    hip._info_track_operands(pose, info, obs, vel_weight, accel_weight, huber, reweights, max_gap, min_pivot_ratio, "decode.info_track",
                             dense=False)
    return hip.info_track(_c(pose), _c(info), _c(obs), vel_weight, accel_weight, huber, reweights, max_gap, min_pivot_ratio)


@info_track_op.register_fake
def _info_track_fake(pose, info, obs, vel_weight, accel_weight, huber, reweights, max_gap, min_pivot_ratio):
    N, T, J = hip._info_track_operands(pose, info, obs, vel_weight, accel_weight, huber, reweights, max_gap, min_pivot_ratio,
                                       "decode.info_track", dense=False)
    new = pose.new_empty
    return new((N, T, J, 3)), new((N, T, J), dtype=torch.uint8), new((N, T, J)), new((N, T, J)), new((N, J))


joint_info_op.register_autograd(_nograd_autograd, setup_context=_nograd_setup_context)
info_track_op.register_autograd(_nograd_autograd, setup_context=_nograd_setup_context)


class Information3D(NamedTuple):
    info: torch.Tensor       # (B, J, 6) the information matrix sum_v conf_v J_v^T J_v in the order (00, 01, 02, 11, 12, 22), coordinate units^2 / cm^2
    views: torch.Tensor      # (B, J) uint8 the views that entered
    sigma: torch.Tensor      # (B, J) sqrt(trace(info^-1)): cm of positional standard deviation per unit of coordinate noise; 0 where not valid
    valid: torch.Tensor      # (B, J) bool: the matrix is positive definite and not too flat for its size (min_det_ratio)


class InfoTrack3D(NamedTuple):
    pose: torch.Tensor       # (N, T, J, 3) cm: the smoothed track, written for every frame of a solvable track; 0 for the others
    valid: torch.Tensor      # (N, T, J) bool: the track is solvable and a used frame is at most max_gap frames away
    residual: torch.Tensor   # (N, T, J) sqrt((pose - z)^T W (pose - z)) at used frames, in coordinate units (pixels); 0 elsewhere
    weight: torch.Tensor     # (N, T, J) the Huber factors of the last solve (1 in the plain form), 0 for a gap
    energy: torch.Tensor     # (N, J) the energy at the result


INFO_ACCEL_WEIGHT = 1.0      # the default accel_weight of the matrix-weighted smoother: the rendered clip's sweep set it


def joint_information(points: torch.Tensor, conf: torch.Tensor, cameras: Union[str, Sequence], coord_trans_mat: Optional[torch.Tensor] = None,
                      heatmap_size: Tuple[float, float] = (64, 64), threshold: float = 0.5, min_det_ratio: float = 1e-6,
                      camera_calib_file_dir_path: Optional[str] = None) -> Information3D:
    """points (B, J, 3) cm in the device frame, conf (B, V, J), `cameras`, `coord_trans_mat`, `heatmap_size`, `threshold` as for
    `triangulate_joints` -> Information3D(info, views, sigma, valid): per point W = sum_v conf_v J_v^T J_v, J_v the 2 x 3 Jacobian of
    view v's fisheye projection in pixels of a `heatmap_size` map - how well the views that see the point (conf >= threshold, and the
    point projects off the optical axis) fix it in each direction.  With unit pixel noise W^-1 is the covariance of the triangulated
    point: `sigma` = sqrt(trace(W^-1)) cm per pixel, several times larger along the range than across for the front pair.  It takes no
    coordinates: the matrix depends on where the point is, not on where it was observed.  One launch; not differentiable."""
    what = "decode.joint_information"
    sx, sy = _scales(heatmap_size)
    cams = _ray_records(cameras, camera_calib_file_dir_path, points.device)
    hip._joint_info_operands(points, conf, cams, coord_trans_mat, sx, sy, threshold, float(min_det_ratio), what, dense=False)
    hip._on_device(what, points, conf, coord_trans_mat, exc=ValueError)
    info, views, sigma, valid = joint_info_op(points, conf, cams, coord_trans_mat, sx, sy, float(threshold), float(min_det_ratio))
    return Information3D(info, views, sigma, valid.view(torch.bool))


def _info_parameters(accel_weight, vel_weight, huber_px, reweights, max_gap):
    try:
        return float(vel_weight), float(accel_weight), float(huber_px), reweights, max_gap
    except (TypeError, ValueError):
        raise ValueError(f"egorear_amd.decode.smooth_trajectory_info: accel_weight, vel_weight and huber_px must be numbers, got "
                         f"{accel_weight!r}, {vel_weight!r}, {huber_px!r}") from None


def smooth_trajectory_info(pose: torch.Tensor, info: torch.Tensor, observed: Optional[torch.Tensor] = None,
                           accel_weight: float = INFO_ACCEL_WEIGHT, vel_weight: float = 0.0, huber_px: float = 0.0, reweights: int = 0,
                           max_gap: int = 8, min_pivot_ratio: float = 1e-10) -> InfoTrack3D:
    """pose (N, T, J, 3) cm - or (T, J, 3), one clip - with info (N, T, J, 6) (`Information3D.info`) and observed (N, T, J) bool / uint8
    (None: every frame; `Joints3D.valid` plugs in) -> InfoTrack3D(pose, valid, residual, weight, energy): per joint of every clip the
    track that minimises
      sum_t rho(r_t) + vel_weight sum |x_{t+1} - x_t|^2 + accel_weight sum |x_{t+1} - 2 x_t + x_{t-1}|^2,   r_t^2 = (x_t - z_t)^T W_t (x_t - z_t)
    - `smooth_trajectory` with a 3 x 3 matrix in place of the scalar weight, so that a direction the cameras measure badly (the range,
    for the front pair) is smoothed hard and a direction they measure well barely.  A frame is used when it is observed, its pose and
    matrix are finite, the matrix's diagonal is >= 0 and its trace > 0; any other frame is a gap, filled from its neighbours, and what
    stands in it is never read.  A rank-2 matrix (one view) is a legitimate frame.  r_t is the displacement in pixels, so `huber_px` is
    a radius in pixels: with huber_px > 0, `reweights` (1..16) rounds of iteratively reweighted least squares follow the plain solve.
    A track without enough used frames (one with vel_weight > 0, else two, every frame where T <= 2), or whose elimination meets a
    pivot at or below `min_pivot_ratio` of its largest diagonal entry, gives zeros and valid False.  A frame is valid when a used
    frame is at most `max_gap` frames away.  The penalties are in pixel^2 / cm^2: accel_weight here is not `smooth_trajectory`'s.  One
    launch; nothing here is differentiable."""
    what = "decode.smooth_trajectory_info"
    vel_weight, accel_weight, huber_px, reweights, max_gap = _info_parameters(accel_weight, vel_weight, huber_px, reweights, max_gap)
    one = pose.dim() == 3
    if one:
        pose, info = pose.unsqueeze(0), info.unsqueeze(0) if info.dim() == 3 else info
        observed = None if observed is None else observed.unsqueeze(0)
    if observed is not None:
        observed = _as_flags(observed)
    hip._info_track_operands(pose, info, observed, vel_weight, accel_weight, huber_px, reweights, max_gap, min_pivot_ratio, what, dense=False)
    hip._on_device(what, pose, info, observed, exc=ValueError)
    out, valid, residual, weight, energy = info_track_op(pose, info, observed, vel_weight, accel_weight, huber_px, reweights, max_gap,
                                                         float(min_pivot_ratio))
    track = InfoTrack3D(out, valid.view(torch.bool), residual, weight, energy)
    return InfoTrack3D(*(t.squeeze(0) for t in track)) if one else track


def decode_clip_3d_info(heatmaps: torch.Tensor, cameras: Union[str, Sequence], coord_trans_mat: Optional[torch.Tensor] = None,
                        beta: float = 100.0, threshold: float = 0.5, min_det_ratio: float = 1e-6, linearise_accel_weight: float = 10.0,
                        accel_weight: float = INFO_ACCEL_WEIGHT, vel_weight: float = 0.0, huber_px: float = 0.0, reweights: int = 0,
                        max_gap: int = 8, min_pivot_ratio: float = 1e-10, camera_calib_file_dir_path: Optional[str] = None
                        ) -> Tuple[Joints3D, Track3D, InfoTrack3D]:
    """heatmaps (N, T, V, J, H, W) - or (T, V, J, H, W), one clip - -> (Joints3D, Track3D, InfoTrack3D): soft-argmax, triangulation,
    `smooth_trajectory` in its plain form at `linearise_accel_weight` (the first two results are `decode_clip_3d`'s, bit for bit), then
    `joint_information` AT THAT SMOOTHED TRACK with the soft-argmax confidences, then `smooth_trajectory_info` of the TRIANGULATED poses
    with observed = Joints3D.valid - five launches with nothing between them, bit-identical to calling the pieces.
    Why the matrices are taken at the smoothed track and not at the triangulated points: a matrix evaluated at a frame's own noisy
    point correlates with that frame's error - a point triangulated too near the rig projects with larger Jacobians and so gets more
    weight, and the weighted track is pulled towards the rig (`fit_ray_tracks` fails the same way: a ray distance in cm favours nearer
    points).  The scalar-smoothed track averages the noise of many frames, so matrices taken there are nearly independent of the
    frame's own error and the weighting is unbiased (DESIGN.md 5v has the argument and the measurements).  Not differentiable past the
    first two results."""
    what = "decode.decode_clip_3d_info"
    one = heatmaps.dim() == 5
    if one:
        heatmaps = heatmaps.unsqueeze(0)
        coord_trans_mat = None if coord_trans_mat is None else coord_trans_mat.unsqueeze(0)
    if heatmaps.dim() != 6 or not 2 <= heatmaps.shape[2] <= 4:
        raise ValueError(f"egorear_amd.{what}: heat maps must be (N, T, V, J, H, W) or (T, V, J, H, W) with 2 to 4 views, got "
                         f"{tuple(heatmaps.shape)}")
    N, T, V, J, H, W = (int(v) for v in heatmaps.shape)
    if coord_trans_mat is not None and tuple(coord_trans_mat.shape) != (N, T, V, 4, 4):
        raise ValueError(f"egorear_amd.{what}: coord_trans_mat must be {(N, T, V, 4, 4)}, got {tuple(coord_trans_mat.shape)}")
    # (what the two smoothers would refuse is refused before the soft-argmax runs)
    vel_weight, accel_weight, huber_px, reweights, max_gap = _info_parameters(accel_weight, vel_weight, huber_px, reweights, max_gap)
    _, lin_weight, _, _, _ = _trj_parameters(linearise_accel_weight, 0.0, 0.0, 0, max_gap)
    meta = lambda *shape: heatmaps.new_empty(shape, device="meta")
    hip._trajectory_operands(meta(N, T, J, 3), None, None, 0.0, lin_weight, 0.0, 0, max_gap, what, dense=False)
    hip._info_track_operands(meta(N, T, J, 3), meta(N, T, J, 6), None, vel_weight, accel_weight, huber_px, reweights, max_gap, min_pivot_ratio,
                             what, dense=False)
    hip._on_device(what, heatmaps, coord_trans_mat, exc=ValueError)
    frames = heatmaps.reshape((N * T, V, J, H, W))
    ctm = None if coord_trans_mat is None else coord_trans_mat.reshape(N * T, V, 4, 4)
    joints3d, joints2d = decode_joints_3d(frames, cameras, ctm, beta, threshold, min_det_ratio, camera_calib_file_dir_path)
    track = smooth_trajectory(joints3d.pose.view(N, T, J, 3), None, joints3d.valid.view(N, T, J), lin_weight, 0.0, 0.0, 0, max_gap)
    information = joint_information(track.pose.detach().reshape(N * T, J, 3), joints2d.maxvals.detach(), cameras, ctm, (H, W), threshold,
                                    min_det_ratio, camera_calib_file_dir_path)
    fine = smooth_trajectory_info(joints3d.pose.detach().view(N, T, J, 3), information.info.view(N, T, J, 6), joints3d.valid.view(N, T, J),
                                  accel_weight, vel_weight, huber_px, reweights, max_gap, min_pivot_ratio)
    clip = Joints3D(joints3d.pose.view(N, T, J, 3), joints3d.cost.view(N, T, J), joints3d.residual.view(N, T, V, J), joints3d.valid.view(N, T, J))
    if one:
        clip, track, fine = (Joints3D(*(t.squeeze(0) for t in clip)), Track3D(*(t.squeeze(0) for t in track)),
                             InfoTrack3D(*(t.squeeze(0) for t in fine)))
    return clip, track, fine

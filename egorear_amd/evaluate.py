"""Validation / test steps of the three Lightning wrappers on the device.

The wrappers' `eval_step` (pl_wrappers/egoposeformer/heatmap.py:125-142, heatmap_mvf_ex.py:144-185, pose_3d_mvf_ex.py:165-210)
runs the eval-mode forward, computes its metrics on the host (a device-to-host copy per sample) and hands `v.mean()` of each to
`self.log(..., sync_dist=True)`, which Lightning averages over the batches of the epoch (weighted by batch size) and over the ranks.
Here one step is ONE captured hipGraph per input signature - eval-mode forward, the metric launches (egorear_amd.metrics), the
means, and the addition into an on-device accumulator {sum of value * frames, frames} - replayed through runner.GraphedForward
(static input buffers, a new capture whenever the packed weights change).  `step` copies nothing to the host; `summary` is the
epoch's one device-to-host copy.

    ev = HeatmapMVFEXEval(net)                      # or trainer.evaluator()
    for batch in val_loader:
        logged = ev.step(batch["img"], batch["gt_heatmap"], "val")     # "val/proposal_stereo_front_l1_error_heatmap" -> 0-d tensor
    epoch = ev.summary(); ev.reset()

The values `step` returns are views of the graph's static output: they are overwritten by the next call (clone what must be kept).
`predict` mode (file output on the host) has no counterpart here."""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional

import torch

from . import metrics
from .runner import GraphedForward

MODES = ("val", "test")


class _EvalStep:
    """What the three classes share: the captured body, the accumulators and the epoch summary."""

    def __init__(self, net: torch.nn.Module, process_group=None, warmup: int = 1):
        self.net = net
        self.pg = process_group
        self._graph = GraphedForward(self._body, warmup=warmup)
        self._acc: Dict[str, torch.Tensor] = {}       # mode -> float64 (K + 1,): sum of value * frames per key, then the frames

    # -- what a subclass defines
    def keys(self, mode: str) -> List[str]:
        raise NotImplementedError

    def _metrics(self, mode: str, *inputs) -> "OrderedDict[str, torch.Tensor]":
        raise NotImplementedError

    # -- the captured body: runs eagerly as the warm-up, then once under capture
    def _body(self, mode, *inputs):
        net = self.net
        was_training = net.training
        net.eval()          # flags only: the eval-mode forward reads the BatchNorm running statistics and never writes them
        try:
            with torch.no_grad():
                d = self._metrics(mode, *inputs)
        finally:
            net.train(was_training)
        if list(d) != self.keys(mode):
            raise RuntimeError("egorear_amd.evaluate: metric keys differ from the declared list")
        vals = torch.stack([v.mean() for v in d.values()])      # what the wrapper passes to self.log
        if torch.cuda.is_current_stream_capturing():            # (the warm-up runs must not count)
            acc, frames = self._acc[mode], float(inputs[0].shape[0])
            acc[:-1].add_(vals.double() * frames)
            acc[-1:].add_(frames)
        return vals

    def _step(self, mode: str, *inputs) -> "OrderedDict[str, torch.Tensor]":
        if mode not in MODES:
            raise ValueError(f"egorear_amd.evaluate: mode must be one of {MODES} ('predict' writes files on the host and is not built)")
        if not all(t.is_cuda for t in inputs if isinstance(t, torch.Tensor)):
            raise RuntimeError("egorear_amd.evaluate: device tensors expected (no CPU path)")
        keys = self.keys(mode)
        if mode not in self._acc:       # allocated outside any capture: the graphs of every input signature add into it
            self._acc[mode] = torch.zeros(len(keys) + 1, device=inputs[0].device, dtype=torch.float64)
        vals = self._graph(mode, *inputs)       # a capture that fails raises: there is no eager fallback
        return OrderedDict((f"{mode}/{k}", vals[i]) for i, k in enumerate(keys))

    def captures(self) -> int:
        """Graphs held at the moment (one per mode and input signature since the weights last changed)."""
        return len(self._graph._graphs)

    def reset(self) -> None:
        for acc in self._acc.values():
            acc.zero_()

    def summary(self) -> Dict[str, float]:
        """Frame-weighted mean of every logged value over the steps since the last reset(), averaged over the ranks of the process
        group (Lightning's sync_dist=True) - one device-to-host copy."""
        from .dist import allreduce_mean_
        modes = [m for m in MODES if m in self._acc]
        if not modes:
            return {}
        parts = []
        for m in modes:
            acc = self._acc[m]
            parts += [acc[:-1] / acc[-1:].clamp_min(1.0), acc[-1:]]
        host = allreduce_mean_(torch.cat(parts), self.pg).cpu().tolist()
        out, at = {}, 0
        for m in modes:
            keys = self.keys(m)
            means, frames = host[at:at + len(keys)], host[at + len(keys)]
            at += len(keys) + 1
            if frames > 0:
                out.update((f"{m}/{k}", v) for k, v in zip(keys, means))
        return out


_HM_KEYS = ("_l1_error_heatmap", "_pos_l1_error_heatmap", "_mse_heatmap", "_mse_pts2d")


class HeatmapEval(_EvalStep):
    """PoseHeatmapLightningModel.eval_step (heatmap.py:125-142): `proposal_*` (4 keys).  A ground truth with more views than the
    stereo pair's estimator sees is cut to its first views, as train.HeatmapTrainer does."""

    def keys(self, mode):
        return ["proposal" + k for k in _HM_KEYS]

    def _metrics(self, mode, img, gt_heatmap):
        pred = self.net(img)
        gt = gt_heatmap if gt_heatmap.shape[1] == pred.shape[1] else gt_heatmap[:, :pred.shape[1]].contiguous()
        return metrics.heatmap_dict(metrics.heatmap_metrics(pred, gt), 0, 0, "proposal")

    def step(self, img, gt_heatmap, mode: str = "val"):
        return self._step(mode, img, gt_heatmap)


class HeatmapMVFEXEval(_EvalStep):
    """PoseHeatmapMVFEXLightningModel.eval_step (heatmap_mvf_ex.py:144-185): proposal_stereo_front, final_stereo_front,
    proposal_stereo_back, final_stereo_back (16 keys) from ONE metric launch - two sets, two view groups, the ground truth read
    once.  The `mid_{i}_*` entries of test mode cover the refiner layers between the first and the last; the estimator has one
    refiner layer (estimator.HeatmapMVF refuses more), so that list is empty in the reference too and nothing is built for it."""

    _ORDER = (("proposal_stereo_front", 0, 0), ("final_stereo_front", 1, 0), ("proposal_stereo_back", 0, 1), ("final_stereo_back", 1, 1))

    def keys(self, mode):
        return [p + k for p, _, _ in self._ORDER for k in _HM_KEYS]

    def _metrics(self, mode, img, gt_heatmap):
        hms, _ = self.net(img)
        V = hms[0].shape[1]
        raw = metrics.heatmap_metrics([hms[0], hms[-1]], gt_heatmap, view_groups=[(0, 2), (2, V)])
        out = OrderedDict()
        for prefix, s, g in self._ORDER:
            out.update(metrics.heatmap_dict(raw, s, g, prefix))
        return out

    def step(self, img, gt_heatmap, mode: str = "val"):
        return self._step(mode, img, gt_heatmap)


class Pose3DEval(_EvalStep):
    """Pose3DMVFEXLightningModel.eval_step (pose_3d_mvf_ex.py:165-210): the means of the two predicted poses the reference logs,
    `evaluate_pose` of the final and the proposal pose; "val" keeps the keys containing "mpjpe" (:206-207)."""

    _ALL = ["pred_pose_final", "pred_pose_proposal"] + [p + k for p in ("final", "proposal") for k in ("_mpjpe", "_pa_mpjpe", "_pck_3d", "_auc_3d")]

    def keys(self, mode):
        return [k for k in self._ALL if mode != "val" or "mpjpe" in k]

    def _metrics(self, mode, img, gt_pose, coord_trans_mat):
        preds, _ = self.net(img, coord_trans_mat)
        out = OrderedDict(pred_pose_final=preds[-1], pred_pose_proposal=preds[0])
        out.update(metrics.evaluate_pose(preds[-1], gt_pose, "final"))
        out.update(metrics.evaluate_pose(preds[0], gt_pose, "proposal"))
        return OrderedDict((k, v) for k, v in out.items() if mode != "val" or "mpjpe" in k)

    def step(self, img, gt_pose, mode: str = "val", coord_trans_mat: Optional[torch.Tensor] = None):
        return self._step(mode, img, gt_pose, coord_trans_mat)


def evaluator_for(net: torch.nn.Module, process_group=None) -> _EvalStep:
    """The eval step that belongs to an estimator class."""
    from .estimator import EgoPoseFormerHeatmap, EgoPoseFormerHeatmapMVFEX, EgoPoseFormerMVFEX
    for cls, ev in ((EgoPoseFormerHeatmapMVFEX, HeatmapMVFEXEval), (EgoPoseFormerHeatmap, HeatmapEval), (EgoPoseFormerMVFEX, Pose3DEval)):
        if isinstance(net, cls):
            return ev(net, process_group)
    raise RuntimeError("egorear_amd.evaluate: EgoPoseFormerHeatmap, EgoPoseFormerHeatmapMVFEX or EgoPoseFormerMVFEX expected")

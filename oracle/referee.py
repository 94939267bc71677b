"""Float64 referee of the whole inference path: the CPU oracle evaluated in float64 as the exact-ish result, and the distances of the
HIP path and of the float32 oracle from it, stage by stage.

TEST INFRASTRUCTURE (oracle/ header rule): imported by tests/ and tools/census_run.py only, as the checker.

The kernel tests hold every implicit-GEMM launch to "no further from fp64 than the fp32 launch"; this carries the same question to
the whole network.  Weights, cameras and inputs are float32 numbers; the float64 evaluation casts them and does every operation behind
them in double (the oracle keeps the dtype it is given: msda_core, the fish-eye projection and the anchors included).

Stages, all FRAME-FIRST (the frame is dim 0, so that frames can be selected and excluded):
  feat_init (B, V, C, H, W), hm_init (B, V, J, H, W), query / post_norm (B, G, J, C) and head_sum (B, G, C, h, w) of the four
  refiners (G = V), feat_refined, hm_refined, pose_0 .. pose_3 (B, J, 3).
Discrete decisions: argmax_init / argmax_refined (B, V, J) flat indices of both heat-map sets, valid_h (B, V, J) the refiners'
anchor mask (init maxima >= 0.5), valid_p the lifting head's reprojected-anchor mask.  A stage is compared only over the frames whose
decisions upstream of it (DEPENDS) agree in all three evaluations.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch

from . import egorear_oracle as O
from .census import ROUNDING_GAP

STAGES = ("feat_init", "hm_init", "query", "post_norm", "head_sum", "feat_refined", "hm_refined", "pose_0", "pose_1", "pose_2", "pose_3")
DECISIONS = ("argmax_init", "valid_h", "valid_p", "argmax_refined")
# the decisions a stage's value depends on: the init arg-maxes / masks place the refiners' anchors (everything behind their transformer
# layer), the lifting head's mask gates its three decoder layers; the refined arg-maxes feed nothing
_H = ("argmax_init", "valid_h")
DEPENDS = {"feat_init": (), "hm_init": (), "query": (), "post_norm": _H, "head_sum": _H, "feat_refined": _H, "hm_refined": _H,
           "pose_0": _H, "pose_1": _H + ("valid_p",), "pose_2": _H + ("valid_p",), "pose_3": _H + ("valid_p",)}


def cameras_as(cams: Sequence[O.FishEye], dtype) -> List[O.FishEye]:
    """Copies of the oracle's cameras with their float parameters (polynomial, centre, offset) in `dtype` - the same float32 numbers."""
    out = []
    for c in cams:
        d = O.FishEye.__new__(O.FishEye)
        d.__dict__.update(c.__dict__)
        d.poly, d.image_center, d.offset = c.poly.to(dtype), c.image_center.to(dtype), c.offset.to(dtype)
        out.append(d)
    return out


def reference_outputs(sd, cams, img: torch.Tensor, ctm: Optional[torch.Tensor] = None, dtype=torch.float32) -> Dict[str, object]:
    """The oracle's EgoPoseFormerMVFEX forward (O.mvfex_forward, step for step) in `dtype`, with the refiners' intermediates.
    -> {"stages": {name: tensor}, "decisions": {name: tensor}, "hms": [hm_init, hm_refined], "maxvals": (B, V, J)}."""
    sdd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    camd = cameras_as(cams, dtype)
    x = img.to(dtype)
    m = ctm.to(dtype) if ctm is not None else None
    with torch.no_grad():
        hms, feats, aux_h = O.heatmap_mvfex_forward(sdd, "heatmap_estimator", x, 0.5, capture=True)
        preds, aux_p = O.pose3d_forward(sdd, "pose3d_estimator", camd, feats[0], feats[-1], m, 3, True)
    mid = aux_h["mid"]
    st = {"feat_init": feats[0], "hm_init": hms[0],
          "query": torch.stack([mid[r]["query"] for r in O.REFINERS], 1),
          "post_norm": torch.stack([mid[r]["post_norm"] for r in O.REFINERS], 1),
          "head_sum": torch.stack([mid[r]["head_sum"] for r in O.REFINERS], 1),
          "feat_refined": feats[1], "hm_refined": hms[1]}
    st.update({f"pose_{i}": p for i, p in enumerate(preds)})
    dec = {"argmax_init": aux_h["argmax_idx"], "valid_h": aux_h["anchors_valid"], "valid_p": aux_p["anchors_valid"],
           "argmax_refined": hms[1].flatten(-2).argmax(-1)}
    return {"stages": st, "decisions": dec, "hms": list(hms), "maxvals": aux_h["maxvals"]}


def hip_outputs(net, img_dev: torch.Tensor, ctm_dev: Optional[torch.Tensor] = None, frames=None) -> Dict[str, object]:
    """One forward of the drop-in EgoPoseFormerMVFEX on the device, captured (engine.CAPTURE) in reference_outputs' format, on the CPU;
    `frames`: only these frames of the batch are kept."""
    from egorear_amd import engine
    engine.CAPTURE = cap = {}
    try:
        with torch.no_grad():
            preds, hms = net(img_dev) if ctm_dev is None else net(img_dev, ctm_dev)
    finally:
        engine.CAPTURE = None
    aux = net.__dict__["_egr_last_aux"]
    B, V = img_dev.shape[:2]
    G = cap["query"].shape[0]
    hs = cap["head_sum"]                                   # (G*B, h, w, C) NHWC -> (B, G, C, h, w)
    st = {"feat_init": cap["feat_init"], "hm_init": hms[0], "query": cap["query"].transpose(0, 1), "post_norm": cap["post_norm"].transpose(0, 1),
          "head_sum": hs.view(G, B, *hs.shape[1:]).permute(1, 0, 4, 2, 3), "feat_refined": cap["feat_refined"], "hm_refined": hms[1]}
    st.update({f"pose_{i}": p for i, p in enumerate(preds)})
    dec = {"argmax_init": aux["heatmap"]["argmax_idx"], "valid_h": aux["heatmap"]["anchors_valid"].bool(),
           "valid_p": aux["pose3d"]["anchors_valid"].bool(), "argmax_refined": hms[1].flatten(-2).argmax(-1)}
    sel = torch.arange(B, device=img_dev.device) if frames is None else torch.as_tensor(frames, dtype=torch.long, device=img_dev.device)
    cpu = lambda t: t.detach()[sel].contiguous().cpu()
    return {"stages": {k: cpu(v) for k, v in st.items()}, "decisions": {k: cpu(v) for k, v in dec.items()},
            "hms": [cpu(h) for h in hms], "maxvals": cpu(aux["heatmap"]["maxvals"])}


def select(out: Dict[str, object], idx) -> Dict[str, object]:
    """The frames `idx` (list / index tensor) of an output dict."""
    idx = torch.as_tensor(idx, dtype=torch.long)
    return {"stages": {k: v[idx] for k, v in out["stages"].items()}, "decisions": {k: v[idx] for k, v in out["decisions"].items()},
            "hms": [h[idx] for h in out["hms"]], "maxvals": out["maxvals"][idx]}


def concat(outs: Sequence[Dict[str, object]]) -> Dict[str, object]:
    """Output dicts of several batches as one, frames back to back."""
    return {"stages": {k: torch.cat([o["stages"][k] for o in outs]) for k in outs[0]["stages"]},
            "decisions": {k: torch.cat([o["decisions"][k] for o in outs]) for k in outs[0]["decisions"]},
            "hms": [torch.cat([o["hms"][i] for o in outs]) for i in range(len(outs[0]["hms"]))],
            "maxvals": torch.cat([o["maxvals"] for o in outs])}


def _ratio(a: float, b: float) -> float:
    return a / b if b > 0 else (0.0 if a == 0 else math.inf)


def stage_distances(hip, f32, f64) -> Dict[str, Dict[str, object]]:
    """Per stage: rms and max of (hip - f64) and (f32 - f64), relative to rms(f64) / max|f64|, their ratios hip / f32, and how many
    frames entered (those whose upstream decisions agree in all three evaluations) or were excluded, by decision."""
    n = next(iter(f64["stages"].values())).shape[0]
    # frames on which a decision differs between HIP and float64 or between float32 and float64
    differs = {}
    for d in DECISIONS:
        ref = f64["decisions"][d].reshape(n, -1)
        bad = torch.zeros(n, dtype=torch.bool)
        for other in (hip, f32):
            bad |= (other["decisions"][d].reshape(n, -1).to(ref.dtype) != ref).any(1)
        differs[d] = bad
    out = {}
    for s in STAGES:
        keep = torch.ones(n, dtype=torch.bool)
        reasons = {}
        for d in DEPENDS[s]:
            reasons[d] = int((differs[d] & keep).sum())      # (each excluded frame counted once, under the first decision it fails)
            keep &= ~differs[d]
        r = {"frames": int(keep.sum()), "excluded": n - int(keep.sum()), "reasons": {k: v for k, v in reasons.items() if v}}
        if r["frames"]:
            e = f64["stages"][s][keep].double()
            rms_e, max_e = float(e.pow(2).mean().sqrt()), float(e.abs().max())
            for tag, src in (("hip", hip), ("f32", f32)):
                dlt = src["stages"][s][keep].double() - e
                r["rms_" + tag] = _ratio(float(dlt.pow(2).mean().sqrt()), rms_e)
                r["max_" + tag] = _ratio(float(dlt.abs().max()), max_e)
            r["ratio_rms"], r["ratio_max"] = _ratio(r["rms_hip"], r["rms_f32"]), _ratio(r["max_hip"], r["max_f32"])
        out[s] = r
    return out


def _top2(flat: torch.Tensor):
    t = flat.topk(2, dim=-1).values
    return t[..., 0] - t[..., 1]


def argmax_vs_referee(hip_hms: Sequence[torch.Tensor], f64_hms: Sequence[torch.Tensor], f32_hms: Optional[Sequence[torch.Tensor]] = None,
                      threshold: float = 0.5) -> List[Dict[str, object]]:
    """Per heat-map set (B, V, J, H, W): the arg-max disagreements of HIP (and of float32) with float64, each with float64's own top-2
    gap and the float64 distance between its choice and HIP's; the flips of the `valid` decision (maximum >= threshold) with the
    float64 maximum's distance from the threshold.  `outside_rounding` / `flips_outside` count what no rounding-level difference
    explains (float64 gap to HIP's choice >= census.ROUNDING_GAP; |max_f64 - threshold| >= 1e-6)."""
    res = []
    for si, (h, e) in enumerate(zip(hip_hms, f64_hms)):
        hf, ef = h.flatten(-2).double(), e.flatten(-2).double()
        emax, ei = ef.max(-1)
        hi = hf.argmax(-1)
        gap2 = _top2(ef)
        r = {"set": si, "maps": int(ei.numel()), "hip_disagreements": int((hi != ei).sum()), "disagreements": []}
        for b, v, j in (hi != ei).nonzero().tolist():
            to_hip = float(ef[b, v, j, ei[b, v, j]] - ef[b, v, j, hi[b, v, j]])
            r["disagreements"].append({"frame": b, "view": v, "joint": j, "idx_f64": int(ei[b, v, j]), "idx_hip": int(hi[b, v, j]),
                                       "f64_top2_gap": float(gap2[b, v, j]), "f64_gap_to_hip": to_hip})
        r["outside_rounding"] = sum(d["f64_gap_to_hip"] >= ROUNDING_GAP for d in r["disagreements"])
        if f32_hms is not None:
            r["f32_disagreements"] = int((f32_hms[si].flatten(-2).argmax(-1) != ei).sum())
        ve, vh = emax >= threshold, hf.max(-1).values >= threshold
        r["valid_flips"] = [{"frame": b, "view": v, "joint": j, "max_f64": float(emax[b, v, j]), "f64_to_threshold": float(abs(emax[b, v, j] - threshold))}
                            for b, v, j in (ve != vh).nonzero().tolist()]
        r["flips_outside"] = sum(f["f64_to_threshold"] >= 1e-6 for f in r["valid_flips"])
        if f32_hms is not None:
            r["f32_valid_flips"] = int(((f32_hms[si].flatten(-2).max(-1).values >= threshold) != ve).sum())
        res.append(r)
    return res

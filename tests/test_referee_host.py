"""The float64 referee (oracle/referee.py) on the CPU: the float64 oracle really is float64 at every stage, its float32 twin is the
census oracle bit for bit, and the distance / arg-max bookkeeping the GPU test (test_gpu_float64_referee.py) relies on flags what it
must - an injected error at its own stage only, a flipped decision as an excluded frame, a near-tie as a rounding-level disagreement."""
import copy

import pytest
import torch

from egorear_amd import configs, synth
from egorear_amd.estimator import EgoPoseFormerMVFEX
from oracle import census
from oracle import egorear_oracle as O
from oracle import referee as R


def _sd(camera):
    return synth.synth_state_dict(synth.spec_of(EgoPoseFormerMVFEX(**copy.deepcopy(configs.pose3d_cfg(camera)))), 42)


@pytest.fixture(scope="module")
def syn(calib_dir):
    """Two frames at image scale 0.35 (maxima on both sides of the 0.5 threshold) through the float32 and the float64 oracle; while the
    float64 one runs, every deformable-attention core and fish-eye projection records the dtypes it saw."""
    torch.manual_seed(0)
    sd = _sd("ego4view_syn")
    cams = O.make_cameras("ego4view_syn", calib_dir)
    img = synth.synth_images(2, 4, seed=3, scale=0.35)
    f32 = R.reference_outputs(sd, cams, img, dtype=torch.float32)
    seen = []
    msda, w2c = O.msda_core, O.FishEye.world2camera

    def msda_spy(value, H, W, loc, attn):
        out = msda(value, H, W, loc, attn)
        seen.append(("msda_core", value.dtype, loc.dtype, attn.dtype, out.dtype))
        return out

    def w2c_spy(self, pts, m=None):
        pt, ok = w2c(self, pts, m)
        seen.append(("world2camera", pts.dtype, self.poly.dtype, self.image_center.dtype, pt.dtype))
        return pt, ok
    O.msda_core, O.FishEye.world2camera = msda_spy, w2c_spy
    try:
        f64 = R.reference_outputs(sd, cams, img, dtype=torch.float64)
    finally:
        O.msda_core, O.FishEye.world2camera = msda, w2c
    return {"sd": sd, "cams": cams, "img": img, "f32": f32, "f64": f64, "seen": seen}


def test_stage_table_covers_every_stage():
    assert set(R.DEPENDS) == set(R.STAGES)
    assert all(set(d) <= set(R.DECISIONS) for d in R.DEPENDS.values())


def test_float64_run_is_float64_at_every_stage(syn):
    f32, f64 = syn["f32"], syn["f64"]
    assert set(f64["stages"]) == set(R.STAGES)
    for k, v in f64["stages"].items():
        assert v.dtype == torch.float64, k
        assert f32["stages"][k].dtype == torch.float32 and f32["stages"][k].shape == v.shape, k
        # a genuine float64 evaluation: not the float32 numbers cast up, and not far from them either
        d = float((f32["stages"][k].double() - v).abs().max())
        assert 0 < d < 1e-5 * max(1.0, float(v.abs().max())), (k, d)
    assert all(h.dtype == torch.float64 for h in f64["hms"]) and f64["maxvals"].dtype == torch.float64
    kinds = {s[0] for s in syn["seen"]}
    assert kinds == {"msda_core", "world2camera"}
    for s in syn["seen"]:
        assert all(t == torch.float64 for t in s[1:]), s
    for k in R.DECISIONS:
        assert torch.equal(f32["decisions"][k], f64["decisions"][k]), k


def test_float64_run_with_per_frame_transforms(calib_dir):
    """ego4view_rw: the coord_trans_mat path of the projection stays float64 too."""
    sd = _sd("ego4view_rw")
    cams = O.make_cameras("ego4view_rw", calib_dir)
    out = R.reference_outputs(sd, cams, synth.synth_images(1, 4, seed=4), synth.synth_coord_trans_mat(1, seed=5), dtype=torch.float64)
    assert all(v.dtype == torch.float64 for v in out["stages"].values())
    assert out["decisions"]["valid_p"].shape == (1, 4, 16)


def test_float32_run_is_the_census_oracle_bit_for_bit(syn):
    ref = census.oracle_outputs(syn["sd"], syn["cams"], syn["img"], O)
    f32 = syn["f32"]
    for i in range(4):
        assert torch.equal(ref["preds"][i], f32["stages"][f"pose_{i}"])
    assert torch.equal(ref["hms"][0], f32["stages"]["hm_init"]) and torch.equal(ref["hms"][1], f32["stages"]["hm_refined"])
    assert torch.equal(ref["argmax_idx"], f32["decisions"]["argmax_init"])
    assert torch.equal(ref["valid_h"], f32["decisions"]["valid_h"]) and torch.equal(ref["valid_p"], f32["decisions"]["valid_p"])
    assert torch.equal(ref["maxvals"], f32["maxvals"])


def _copy(out):
    return {"stages": dict(out["stages"]), "decisions": dict(out["decisions"]), "hms": list(out["hms"]), "maxvals": out["maxvals"]}


@pytest.mark.parametrize("stage", ["feat_init", "post_norm", "hm_refined", "pose_2"])
def test_injected_error_is_flagged_at_its_stage_only(syn, stage):
    f32, f64 = syn["f32"], syn["f64"]
    hip = _copy(f32)
    hip["stages"][stage] = f64["stages"][stage] + 3 * (f32["stages"][stage].double() - f64["stages"][stage])
    t = R.stage_distances(hip, f32, f64)
    for s in R.STAGES:
        r = t[s]
        assert r["frames"] == 2 and r["excluded"] == 0 and r["rms_f32"] > 0
        want = 3.0 if s == stage else 1.0
        assert r["ratio_rms"] == pytest.approx(want, rel=1e-9) and r["ratio_max"] == pytest.approx(want, rel=1e-9), (s, r)


def test_flipped_decision_excludes_the_frame_downstream(syn):
    f32, f64 = syn["f32"], syn["f64"]
    hip = _copy(f32)
    a = hip["decisions"]["argmax_init"].clone()
    a[1, 2, 7] += 1                                          # frame 1: one initial arg-max elsewhere
    hip["decisions"]["argmax_init"] = a
    t = R.stage_distances(hip, f32, f64)
    for s in R.STAGES:
        if "argmax_init" in R.DEPENDS[s]:
            assert (t[s]["frames"], t[s]["excluded"], t[s]["reasons"]) == (1, 1, {"argmax_init": 1}), s
        else:
            assert (t[s]["frames"], t[s]["excluded"]) == (2, 0), s
    # a lifting-head mask flip in frame 0 (float32 side) takes that frame out of the three decoder layers as well
    f32b = _copy(f32)
    v = f32b["decisions"]["valid_p"].clone()
    v[0, 1, 3] = ~v[0, 1, 3]
    f32b["decisions"]["valid_p"] = v
    t = R.stage_distances(hip, f32b, f64)
    assert t["pose_0"]["frames"] == 1 and t["pose_1"]["frames"] == 0
    assert t["pose_3"]["reasons"] == {"argmax_init": 1, "valid_p": 1} and "rms_hip" not in t["pose_3"]
    assert t["query"]["frames"] == 2


def test_argmax_vs_referee_classifies_near_ties():
    f64 = torch.zeros(2, 1, 3, 4, 4, dtype=torch.float64)
    f64[0, 0, 0, 1, 1], f64[0, 0, 0, 1, 2] = 0.8, 0.8 - 2e-7     # a near-tie: HIP picking the runner-up is rounding
    f64[0, 0, 1, 0, 3], f64[0, 0, 1, 1, 3] = 0.9, 0.7            # a clear maximum: HIP picking the other one is an error
    f64[1, 0, 0, 2, 2] = 0.5 + 5e-7                              # a maximum on the threshold: a flip there is rounding
    f64[1, 0, 1, 3, 0] = 0.6                                     # ... well above it: a flip is an error
    f64[1, 0, 2, 0, 0] = 0.3
    hip = f64.clone().float()
    hip[0, 0, 0, 1, 2] = 0.8 + 1e-7
    hip[0, 0, 1, 1, 3] = 0.95
    hip[1, 0, 0, 2, 2] = 0.5 - 1e-7
    hip[1, 0, 1, 3, 0] = 0.45
    hms = [f64, f64.clone()]
    res = R.argmax_vs_referee([hip, f64.float()], hms, f32_hms=[f64.float(), f64.float()])
    r = res[0]
    assert r["maps"] == 6 and r["hip_disagreements"] == 2 and r["outside_rounding"] == 1 and r["f32_disagreements"] == 0
    near = [d for d in r["disagreements"] if d["joint"] == 0][0]
    far = [d for d in r["disagreements"] if d["joint"] == 1][0]
    assert near["idx_f64"] == 5 and near["idx_hip"] == 6 and near["f64_top2_gap"] == pytest.approx(2e-7, rel=1e-6)
    assert far["f64_gap_to_hip"] == pytest.approx(0.2) and far["f64_top2_gap"] == pytest.approx(0.2)
    assert sorted((f["frame"], f["joint"]) for f in r["valid_flips"]) == [(1, 0), (1, 1)] and r["flips_outside"] == 1
    assert r["f32_valid_flips"] == 0
    assert res[1]["hip_disagreements"] == 0 and res[1]["valid_flips"] == []

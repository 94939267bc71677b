"""Heat-map validation metrics (`evaluate` of pl_wrappers/egoposeformer/heatmap.py:220-254, heatmap_mvf_ex.py:263-316): the
fixture tests/golden/heatmap_eval.npz holds the REAL reference's outputs (tools/make_golden_heatmap_eval.py) beside the same
formulas in float64 with exactly rounded sums and the reference's own distance from them (`ref_err`); the inputs come from seeds.
CPU: the fixture against a numpy restatement, the C ABI.  GPU: `egr_heatmap_metrics_f32` against the fixture.

Bounds of the GPU comparison.  The kernel sums in fp64 and rounds once to fp32, so against the float64 column it may be off by
one fp32 ulp; the reference sums in fp32 in torch's order and is `ref_err` away from the float64 column, which the fixture
measured - against the reference the kernel gets 2 * ref_err + 1 ulp.  `_mse_pts2d` is a quotient of exact integers: one fp32
rounding, rtol 1e-6.  Arg-max points and validity are integers and must be equal."""
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

DEV = "cuda:0"
SUMS = ("l1", "pos_l1", "mse")


def _gen():
    spec = importlib.util.spec_from_file_location("make_golden_heatmap_eval", os.path.join(REPO, "tools", "make_golden_heatmap_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gen():
    return _gen()


@pytest.fixture(scope="module")
def data(gen):
    pred, gt = gen.cases()
    return pred, gt, np.load(os.path.join(GOLDEN, "heatmap_eval.npz"))


def _restate(pred, gt, thr=1.0):
    """The four formulas in plain numpy float64 (sums exactly rounded: independent of any order); pred, gt (B, Vg, J, H, W) fp32."""
    nb, w = pred.shape[0], pred.shape[-1]
    p, g = pred.astype(np.float64).reshape(nb, -1), gt.astype(np.float64).reshape(nb, -1)
    l1 = np.array([math.fsum(np.abs(p[b] - g[b])) for b in range(nb)])
    pos = np.array([math.fsum(np.abs(p[b] - g[b])[g[b] > 0]) for b in range(nb)])
    mse = math.fsum(((p - g) ** 2).reshape(-1)) / p.size
    pm, gm = pred.reshape(*pred.shape[:3], -1), gt.reshape(*gt.shape[:3], -1)
    pi, gi = pm.argmax(-1), gm.argmax(-1)
    valid = gm.max(-1) >= np.float32(thr)
    sq = ((pi % w - gi % w) * valid) ** 2 + ((pi // w - gi // w) * valid) ** 2
    return {"l1": l1, "pos_l1": pos, "mse": mse, "mse_pts2d": int(sq.sum()) / (2 * valid.size)}, pi, gi, valid


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def test_fixture_is_consistent_and_the_known_answers_hold(gen, data):
    pred, gt, fx = data
    assert gt.shape == (6, 4, 15, 64, 64) and gen.GROUPS == ((0, 2), (2, 4), (0, 4))
    for s in gen.SETS:
        for gi_, (v0, v1) in enumerate(gen.GROUPS):
            mine, pi, gidx, valid = _restate(pred[s][:, v0:v1].numpy(), gt[:, v0:v1].numpy())
            for name in SUMS + ("mse_pts2d",):
                f64, ref, err = fx[f"{s}{gi_}_{name}_f64"], fx[f"{s}{gi_}_{name}_ref"], fx[f"{s}{gi_}_{name}_ref_err"]
                assert ref.dtype == np.float32 and f64.dtype == np.float64
                assert np.array_equal(np.asarray(mine[name], dtype=np.float64), f64), (s, gi_, name)
                assert np.all(np.abs(ref.astype(np.float64) - np.asarray(mine[name])) <= err), (s, gi_, name)
            assert fx[f"{s}{gi_}_l1_ref"].shape == (6,) and fx[f"{s}{gi_}_pos_l1_ref"].shape == (6,)
            assert fx[f"{s}{gi_}_mse_ref"].shape == () and fx[f"{s}{gi_}_mse_pts2d_ref"].shape == ()
            if (v0, v1) == (0, 4):
                assert np.array_equal(pi, fx[f"{s}_argmax"]) and np.array_equal(gidx, fx["gt_argmax"]) and np.array_equal(valid, fx["gt_valid"])
            # the perfect sample: both per-sample errors are exactly 0; the points differ elsewhere, so the point error pins something
            assert fx[f"{s}{gi_}_l1_ref"][3] == 0.0 and fx[f"{s}{gi_}_pos_l1_ref"][3] == 0.0
            assert fx[f"{s}{gi_}_mse_pts2d_ref"] > 1.0
            # negative predictions where gt > 0: the positive-position error of that sample exceeds the ground truth's own mass there
            assert fx[f"{s}{gi_}_pos_l1_ref"][2] > float(gt[2, v0:v1].sum())
    valid, gidx = fx["gt_valid"], fx["gt_argmax"]
    assert not valid[0, 0, 2] and not valid[0, 1, 3] and gt[0, 0, 2].abs().sum() == 0      # joint outside: empty map, invalid
    assert valid[0, 0, 0] and gidx[0, 0, 0] == 0 and gidx[0, 0, 1] == 64 * 64 - 1           # peaks in the corners (clipped window)
    assert 0 < int((~valid).sum()) < valid.size
    b, v, j, i0, i1 = gen.TIE
    m = pred["a"][b, v, j].reshape(-1)
    assert m[i0] == m[i1] == m.max() and i0 < i1 and fx["a_argmax"][b, v, j] == i0        # the tie goes to the first index
    assert valid[b, v, j]
    assert (np.abs(fx["a_argmax"].astype(int) % 64 - gidx.astype(int) % 64)[valid] >= 3).sum() > 20      # arg-maxes pixels apart


def test_header_declares_and_library_exports_the_entry_point():
    from egorear_amd import hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "egorear_hip.h")).read(), flags=re.S)
    assert re.search(r"\begr_heatmap_metrics_f32\s*\(", text)
    assert hasattr(ctypes.CDLL(hip.LIB_PATH), "egr_heatmap_metrics_f32") and "egr_heatmap_metrics_f32" in hip.EXPORTS


def test_no_cpu_path():
    from egorear_amd import metrics
    t = torch.zeros(1, 2, 3, 8, 8)
    with pytest.raises(RuntimeError):
        metrics.heatmap_metrics(t, t)
    with pytest.raises(RuntimeError):
        metrics.evaluate_heatmap(t, t, "x")


def _check_against_fixture(raw, s_idx, s, gen, fx, report):
    for gi_ in range(len(gen.GROUPS)):
        for name in SUMS:
            got = raw[name][s_idx, gi_].cpu().numpy().astype(np.float64)
            ref, f64, err = fx[f"{s}{gi_}_{name}_ref"].astype(np.float64), fx[f"{s}{gi_}_{name}_f64"], fx[f"{s}{gi_}_{name}_ref_err"]
            d_ref, d_64 = np.abs(got - ref), np.abs(got - f64)
            report.append(f"{s}{gi_} {name}: |hip-ref| max {d_ref.max():.3e} (bound min {np.min(2 * err + _ulp32(got)):.3e})  |hip-f64| max {d_64.max():.3e} ulps {np.max(d_64 / _ulp32(f64)):.2f}")
            print(report[-1])
            assert np.all(d_ref <= 2 * err + _ulp32(got)), report[-1]
            assert np.all(d_64 <= _ulp32(f64)), report[-1]
        got = float(raw["mse_pts2d"][s_idx, gi_])
        print(f"{s}{gi_} mse_pts2d: hip {got!r} ref {float(fx[f'{s}{gi_}_mse_pts2d_ref'])!r}")
        np.testing.assert_allclose(got, fx[f"{s}{gi_}_mse_pts2d_ref"], rtol=1e-6, atol=0)


@pytest.mark.gpu
def test_hip_heatmap_metrics_match_the_reference(gen, data):
    from egorear_amd import metrics
    pred, gt, fx = data
    pa, pb, g = pred["a"].to(DEV), pred["b"].to(DEV), gt.to(DEV)
    report = []
    two = metrics.heatmap_metrics([pa, pb], g.double(), view_groups=gen.GROUPS)          # float64 gt like the dataset
    one = metrics.heatmap_metrics(pa, g, view_groups=gen.GROUPS)
    assert two["l1"].shape == (2, 3, 6) and two["mse"].shape == (2, 3) and two["argmax"].shape == (3, 6, 4, 15) and one["l1"].shape == (1, 3, 6)
    for raw, sets in ((two, ("a", "b")), (one, ("a",))):
        for i, s in enumerate(sets):
            assert np.array_equal(raw["argmax"][i].cpu().numpy(), fx[f"{s}_argmax"].astype(np.int32))
            _check_against_fixture(raw, i, s, gen, fx, report)
        assert np.array_equal(raw["argmax"][-1].cpu().numpy(), fx["gt_argmax"].astype(np.int32))
        assert np.array_equal(raw["valid"].cpu().numpy().astype(bool), fx["gt_valid"])
        assert torch.equal(raw["maxval"][-1], g.reshape(6, 4, 15, -1).max(-1).values)
    # the wrappers' call: a view slice, the reference's keys in its order, shapes (B,), (B,), (), ()
    ev = metrics.evaluate_heatmap(pa[:, 2:], g[:, 2:], "final_stereo_back")
    assert list(ev) == ["final_stereo_back" + k for k in ("_l1_error_heatmap", "_pos_l1_error_heatmap", "_mse_heatmap", "_mse_pts2d")]
    assert [tuple(v.shape) for v in ev.values()] == [(6,), (6,), (), ()] and all(v.is_cuda for v in ev.values())
    for k, name in zip(ev, ("l1", "pos_l1", "mse", "mse_pts2d")):
        assert torch.equal(ev[k], one[name][0, 1]), k          # group (2, 4) of the full launch, bit for bit
    assert list(metrics.evaluate_heatmap(pa, g, "x", full=False)) == ["x_l1_error_heatmap", "x_pos_l1_error_heatmap"]


@pytest.mark.gpu
def test_hip_heatmap_metrics_are_deterministic_and_sets_are_independent(gen, data):
    from egorear_amd import metrics
    pred, gt, _ = data
    pa, pb, g = pred["a"].to(DEV), pred["b"].to(DEV), gt.to(DEV)
    r1 = metrics.heatmap_metrics([pa, pb], g, view_groups=gen.GROUPS)
    r2 = metrics.heatmap_metrics([pa, pb], g, view_groups=gen.GROUPS)
    for k in r1:
        assert torch.equal(r1[k], r2[k]), k
    for i, p in enumerate((pa, pb)):
        single = metrics.heatmap_metrics(p, g, view_groups=gen.GROUPS)
        for k in ("l1", "pos_l1", "mse", "mse_pts2d", "partials", "argmax", "maxval"):
            assert torch.equal(single[k][0], r1[k][i]), (i, k)
    four = metrics.heatmap_metrics([pa, pb, pb, pa], g)
    assert torch.equal(four["l1"][0], four["l1"][3]) and torch.equal(four["mse"][1], four["mse"][2])


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 64])
def test_hip_heatmap_metrics_other_batch_sizes(batch):
    from egorear_amd import metrics
    g = torch.Generator().manual_seed(batch)
    gt = torch.rand(batch, 4, 15, 64, 64, generator=g) * 1.2
    gt[gt < 0.9] = 0.0
    pred = gt + 0.1 * torch.randn(batch, 4, 15, 64, 64, generator=g)
    raw = metrics.heatmap_metrics(pred.to(DEV), gt.to(DEV), view_groups=[(0, 2), (2, 4)])
    d = (pred.double() - gt.double()).abs()
    for gi_, (v0, v1) in enumerate(((0, 2), (2, 4))):
        l1 = d[:, v0:v1].reshape(batch, -1).sum(1)
        pos = (d * (gt > 0))[:, v0:v1].reshape(batch, -1).sum(1)
        mse = (d[:, v0:v1] ** 2).mean()
        np.testing.assert_allclose(raw["l1"][0, gi_].cpu().numpy(), l1.numpy(), rtol=2e-7)
        np.testing.assert_allclose(raw["pos_l1"][0, gi_].cpu().numpy(), pos.numpy(), rtol=2e-7)
        np.testing.assert_allclose(float(raw["mse"][0, gi_]), float(mse), rtol=2e-7)
    assert torch.equal(raw["argmax"][0].cpu().long(), pred.reshape(batch, 4, 15, -1).argmax(-1))


@pytest.mark.gpu
def test_hip_heatmap_metrics_refuse_what_they_do_not_handle():
    from egorear_amd import hip, metrics
    ok = torch.zeros(2, 4, 15, 8, 8, device=DEV)
    metrics.heatmap_metrics(ok, ok)
    with pytest.raises(hip.LaunchError) as e:                        # H * W not a multiple of the vector width
        metrics.heatmap_metrics(torch.zeros(2, 4, 15, 3, 3, device=DEV), torch.zeros(2, 4, 15, 3, 3, device=DEV))
    assert e.value.code == hip.EINVAL
    with pytest.raises(hip.LaunchError) as e:                        # J > 32
        metrics.heatmap_metrics(torch.zeros(1, 2, 33, 8, 8, device=DEV), torch.zeros(1, 2, 33, 8, 8, device=DEV))
    assert e.value.code == hip.EINVAL
    with pytest.raises(RuntimeError):                                # non-contiguous
        metrics.heatmap_metrics(ok[:, 0:2], ok[:, 0:2])
    with pytest.raises(RuntimeError):                                # not fp32
        metrics.heatmap_metrics(ok.half(), ok)
    for groups in ([(1, 1)], [(0, 5)], [(2, 1)], []):                # empty / out-of-range view group
        with pytest.raises(RuntimeError):
            metrics.heatmap_metrics(ok, ok, view_groups=groups)
    with pytest.raises(RuntimeError):                                # S <= 4
        metrics.heatmap_metrics([ok] * 5, ok)
    with pytest.raises(RuntimeError):                                # shapes differ
        metrics.heatmap_metrics(ok, ok[:1].contiguous())
    vg = (ctypes.c_int32 * 2)(1, 1)                                  # the C entry itself refuses an empty group
    ptrs = (ctypes.c_void_p * 1)(ok.data_ptr())
    z = ctypes.c_void_p(ok.data_ptr())
    assert hip.lib.egr_heatmap_metrics_f32(ptrs, 1, z, 2, 4, 15, 8, 8, vg, 1, 1.0, z, z, z, z, z, z, z, z, None) == hip.EINVAL
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_hip_heatmap_metrics_are_capturable(gen, data):
    """No synchronisation and no allocation outside torch's pool: the launch records into a hipGraph and replays with the same bits."""
    from egorear_amd import metrics
    pred, gt, _ = data
    pa, g = pred["a"].to(DEV), gt.to(DEV)
    eager = metrics.heatmap_metrics(pa, g, view_groups=gen.GROUPS)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rec = metrics.heatmap_metrics(pa, g, view_groups=gen.GROUPS)
    graph.replay()
    torch.cuda.synchronize()
    for k in ("l1", "pos_l1", "mse", "mse_pts2d", "argmax"):
        assert torch.equal(rec[k], eager[k]), k

"""CPU-side checks of the soft-argmax decode (egorear_amd/decode.py): the two operators are registered with fake implementations,
the reference-named functions trace under Dynamo as one graph on meta tensors, shape / dtype / parameter errors are raised before any
launch, CPU tensors are refused, and the trainer's new options default to "off"."""
import inspect

import pytest
import torch


def test_operators_are_registered_with_fake_implementations():
    from egorear_amd import decode
    assert hasattr(torch.ops.egorear_amd, "soft_argmax") and hasattr(torch.ops.egorear_amd, "soft_argmax_bwd")
    hm = torch.empty(2, 3, 8, 12, device="meta", requires_grad=True)
    coords, maxvals, index, valid, stat, probs = decode.soft_argmax_op(hm, 100.0, 0, False, 0.5, True)
    assert coords.shape == (2, 3, 2) and maxvals.shape == (2, 3) and stat.shape == (2, 3, 2) and probs.shape == hm.shape
    assert index.dtype == torch.int32 and valid.dtype == torch.uint8 and coords.dtype == maxvals.dtype == probs.dtype == torch.float32
    assert coords.requires_grad and maxvals.requires_grad and not index.requires_grad and not valid.requires_grad
    assert decode.soft_argmax_op(hm, 1.0, 1, True, 0.0, False)[5].shape == (0,)
    # the registered autograd formula, on meta: from the coordinates and from maxvals
    (g,) = torch.autograd.grad([coords, maxvals], [hm], [torch.empty_like(coords), torch.empty_like(maxvals)])
    assert g.shape == hm.shape and g.dtype == torch.float32
    g2 = decode.soft_argmax_bwd_op(hm.detach(), stat.detach(), coords.detach(), index, torch.empty(2, 3, 2, device="meta"), None, 100.0, 0, False)
    assert g2.shape == hm.shape


def test_reference_named_functions_trace_as_one_graph():
    import torch._dynamo as dynamo
    from egorear_amd import decode
    lin = torch.nn.Conv2d(4, 15, 1, device="meta")

    def lightning_side(feat, target):
        hm = lin(feat)
        coords, probs = decode.integrate_tensor_2d(hm)
        preds, maxvals = decode.get_max_preds_soft(hm, normalize=True)
        return (coords - target).abs().mean() + preds.sum() + maxvals.sum(), probs

    feat, target = torch.empty(2, 4, 64, 64, device="meta"), torch.empty(2, 15, 2, device="meta")
    loss, probs = lightning_side(feat, target)
    assert loss.requires_grad and not probs.requires_grad and probs.shape == (2, 15, 64, 64)
    coords, hm_w = decode.integrate_tensor_2d(torch.empty(2, 15, 64, 48, device="meta"), softmax=False, multiplier=10.0)
    assert coords.shape == (2, 15, 2) and hm_w.shape == (2, 15, 64, 48)
    preds, maxvals = decode.get_max_preds_soft(torch.empty(3, 15, 64, 64, device="meta"))
    assert preds.shape == (3, 15, 2) and maxvals.shape == (3, 15, 1)
    out = decode.decode_joints_2d(torch.empty(2, 4, 15, 64, 64, device="meta"))
    assert out.soft.shape == out.hard.shape == (2, 4, 15, 2) and out.maxvals.shape == out.valid.shape == (2, 4, 15)
    assert out.valid.dtype == torch.bool and out.hard.dtype == torch.float32
    dynamo.reset()
    ex = dynamo.explain(lightning_side)(feat, target)
    assert ex.graph_break_count == 0 and ex.graph_count == 1, ex
    targets = [str(nd.target) for g in ex.graphs for nd in g.graph.nodes if nd.op == "call_function"]
    assert sum("egorear_amd.soft_argmax" in t for t in targets) == 2, targets


def test_bad_operands_are_refused_before_any_launch():
    from egorear_amd import decode, hip
    hm = torch.zeros(2, 15, 8, 8)
    for bad in (hm[0], hm[None]):                                                     # (B, J, H, W) only
        with pytest.raises(ValueError):
            decode.integrate_tensor_2d(bad)
        with pytest.raises(ValueError):
            decode.get_max_preds_soft(bad)
    with pytest.raises(ValueError):
        decode.decode_joints_2d(hm)                                                   # (B, V, J, H, W) only
    for bad in (hm.double(), hm.half(), hm.long()):
        with pytest.raises(ValueError):
            decode.integrate_tensor_2d(bad)
    for mult in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            decode.integrate_tensor_2d(hm, multiplier=mult)
    with pytest.raises(ValueError):
        decode.soft_argmax_op(torch.zeros(2, 8, 8, device="meta"), 1.0, 2, False, 0.0, False)           # mode outside 0..1
    with pytest.raises(ValueError):
        decode.integrate_tensor_2d(torch.zeros(0, 15, 8, 8))
    with pytest.raises(ValueError):
        decode.soft_argmax_bwd_op(torch.zeros(2, 8, 8, device="meta"), torch.zeros(2, 2, device="meta"), torch.zeros(2, 2, device="meta"),
                                  torch.zeros(2, dtype=torch.int32, device="meta"), torch.zeros(3, 2, device="meta"), None, 1.0, 0, False)
    # the ctypes layer: shapes first, then the device
    with pytest.raises(ValueError):
        hip.soft_argmax(torch.zeros(5))
    with pytest.raises(ValueError):
        hip.soft_argmax_bwd(hm, torch.zeros(30, 2), torch.zeros(30, 2), torch.zeros(30, dtype=torch.int32), torch.zeros(29, 2))
    with pytest.raises(ValueError):
        hip.coord_l1(torch.zeros(30, 2), torch.zeros(30, dtype=torch.int32), torch.zeros(30, dtype=torch.uint8), 8, 1.0, torch.zeros(1))
    with pytest.raises(ValueError):
        hip.coord_l1(torch.zeros(30, 2), torch.zeros(29, dtype=torch.int32), torch.zeros(30, dtype=torch.uint8), 8, 1.0,
                     torch.zeros(1, dtype=torch.float64))


def test_cpu_tensors_are_refused():
    from egorear_amd import decode, hip
    hm = torch.zeros(2, 15, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        decode.integrate_tensor_2d(hm)
    with pytest.raises(RuntimeError, match="no CPU path"):
        decode.get_max_preds_soft(hm)
    with pytest.raises(RuntimeError, match="no CPU path"):
        decode.decode_joints_2d(hm[None])
    with pytest.raises((NotImplementedError, RuntimeError)):                          # the operator itself: no CPU kernel, no fallback
        decode.soft_argmax_op(hm, 1.0, 0, False, 0.0, False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.soft_argmax(hm)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.coord_l1(torch.zeros(30, 2), torch.zeros(30, dtype=torch.int32), torch.zeros(30, dtype=torch.uint8), 8, 1.0,
                     torch.zeros(1, dtype=torch.float64))


def test_trainer_options_default_to_off():
    from egorear_amd import train
    sig = inspect.signature(train.HeatmapTrainer.__init__).parameters
    assert (sig["w_coord"].default, sig["coord_beta"].default, sig["coord_threshold"].default) == (0.0, 100.0, 1.0)
    assert sig["coord_threshold"].default == inspect.signature(__import__("egorear_amd.metrics", fromlist=["x"]).heatmap_metrics).parameters["threshold"].default

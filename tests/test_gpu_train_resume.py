"""Optimizer checkpoint / resume of the native training step: FusedAdamW.state_dict() is torch.optim.AdamW's own format for the
optimizer the reference's configure_optimizers builds, so a run continues bit for bit after save -> fresh process -> load, a
native checkpoint resumes under torch.optim.AdamW and one torch wrote resumes under the native step; the trainers carry a
half-done accumulation group across a checkpoint."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WARMUP = 4        # updates 2, 3, 4 run at 1/4, 2/4, 3/4 of the rate: the warm-up state matters to the third update


def _heatmap_net():
    from egorear_amd import configs, synth
    from egorear_amd.estimator import EgoPoseFormerHeatmap
    net = EgoPoseFormerHeatmap(**copy.deepcopy(configs.heatmap_cfg()))
    synth.load_synth(net, 42)
    return net.to(DEV)


def _write_grads(opt, seed):
    """Seeded gradients straight into the optimizer's gradient views, global norm ~3.4 (1e-3 * sqrt(11.8 M)) < clip 5: the clip
    coefficient is exactly 1 and the last bits of the atomically summed norm cannot matter."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    for k, _, _, _ in opt.slots:
        v = opt.gviews[k]
        v.copy_(torch.randn(v.shape, device=DEV, generator=gen) * 1e-3)
    return set(opt.gviews)


def _update(opt, seed):
    opt.step(_write_grads(opt, seed))
    torch.cuda.synchronize()
    assert opt.grad_norm() < opt.clip


@pytest.mark.parametrize("decay_all", [True, False])
def test_resumed_optimizer_continues_bit_for_bit(decay_all):
    from egorear_amd import train
    whole = train.FusedAdamW(_heatmap_net(), warmup_iters=WARMUP, decay_all=decay_all)
    for t in range(3):
        _update(whole, 100 + t)
    net1 = _heatmap_net()
    first = train.FusedAdamW(net1, warmup_iters=WARMUP, decay_all=decay_all)
    for t in range(2):
        _update(first, 100 + t)
    first.lr_scale_epoch = 1.0
    sd = first.state_dict()
    assert set(sd) == {"state", "param_groups", "egorear_amd"} and len(sd["param_groups"]) == (1 if decay_all else 2)
    assert all(abs(g["lr"] - first.lr_at(3)) < 1e-15 for g in sd["param_groups"])          # what the warm-up hook leaves for update 3
    assert float(sd["state"][0]["step"]) == 2.0 and "flat_acc" not in sd["egorear_amd"]
    net2 = _heatmap_net()
    net2.load_state_dict(net1.state_dict())
    resumed = train.FusedAdamW(net2, warmup_iters=WARMUP, decay_all=decay_all)
    resumed.load_state_dict(sd)
    assert resumed.steps == whole.steps - 1 == 2
    assert all(resumed.lr_at(t) == whole.lr_at(t) for t in range(1, 8))
    assert torch.equal(resumed.m, first.m) and torch.equal(resumed.v, first.v) and torch.equal(resumed.flat_p, first.flat_p)
    _update(resumed, 102)
    assert resumed.steps == whole.steps == 3
    assert torch.equal(resumed.flat_p, whole.flat_p) and torch.equal(resumed.m, whole.m) and torch.equal(resumed.v, whole.v)
    # a state that does not fit is refused whole
    bad = first.state_dict()
    bad["state"][5]["exp_avg"] = torch.zeros(3, 3, 3, device=DEV)
    name = resumed.state_map.entries[5][2]
    m_before = resumed.m.clone()
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        resumed.load_state_dict(bad)
    assert torch.equal(resumed.m, m_before) and resumed.steps == 3


def _reference_adamw(net, lr, wd, decay_all):
    """The reference's configure_optimizers on clones of the module's parameters.  Returns ([(name, clone)], optimizer)."""
    ps = [(k, torch.nn.Parameter(p.detach().clone())) for k, p in net.named_parameters()]
    if decay_all:
        return ps, torch.optim.AdamW([p for _, p in ps], lr=lr, weight_decay=wd)
    no_decay = [p for k, p in ps if 'norm' in k or 'bn' in k or 'ln' in k or 'bias' in k]
    other = [p for k, p in ps if not ('norm' in k or 'bn' in k or 'ln' in k or 'bias' in k)]
    return ps, torch.optim.AdamW([{"params": no_decay, "weight_decay": 0.0}, {"params": other}], lr=lr, weight_decay=wd)


@pytest.mark.parametrize("decay_all", [True, False])
def test_native_state_resumes_under_torch_adamw(decay_all):
    """The saved dict loads into torch.optim.AdamW; one optimizer.step() of torch and one native update from the same gradients
    move every parameter alike (per-element bounds of test_optimizer_step_matches_reference_adamw: 2e-5 where the step is a
    full-size one, 1e-4 elsewhere)."""
    from egorear_amd import train
    net = _heatmap_net()
    opt = train.FusedAdamW(net, warmup_iters=WARMUP, decay_all=decay_all)
    for t in range(2):
        _update(opt, 200 + t)
    ps, ref = _reference_adamw(net, opt.lr, opt.wd, decay_all)
    ref.load_state_dict(opt.state_dict())
    assert all(abs(g["lr"] - opt.lr * 2 / WARMUP) < 1e-15 for g in ref.param_groups)
    before = opt.flat_p.clone()
    have = _write_grads(opt, 202)
    for k, p in ps:
        p.grad = opt.gviews[k].clone()
    ref.step()
    opt.step(have)
    torch.cuda.synchronize()
    assert float(ref.state[ps[0][1]]["step"]) == 3.0 and opt.steps == 3
    mine = dict(net.named_parameters())
    moved = 0.0
    for k, o, n, _ in opt.slots:
        r = dict(ps)[k].detach()
        d, ref_d = (mine[k].detach() - before[o:o + n].view(r.shape)), (r - before[o:o + n].view(r.shape))
        big = ref_d.abs() >= 0.9e-3
        err = (d - ref_d).abs()
        assert bool((err <= torch.where(big, torch.full_like(err, 2e-5), torch.full_like(err, 1e-4))).all()), (k, float(err.max()))
        moved = max(moved, float(ref_d.abs().max()))
    assert moved > 1e-4                                     # (update 3 at half the rate: the comparison is not between two zeros)


@pytest.mark.parametrize("decay_all", [True, False])
def test_torch_adamw_state_resumes_under_the_native_optimizer(decay_all):
    from egorear_amd import train
    net = _heatmap_net()
    probe = train.FusedAdamW(_heatmap_net(), warmup_iters=WARMUP, decay_all=decay_all)       # (gradient views + the warm-up rule)
    ps, ref = _reference_adamw(net, probe.lr, probe.wd, decay_all)
    for t in (1, 2):
        _write_grads(probe, 300 + t)
        for k, p in ps:
            p.grad = probe.gviews[k].clone()
        ref.step()
        for g in ref.param_groups:                          # the wrapper's hook, after optimizer.step(): the rate of update t + 1
            g["lr"] = probe.lr_at(t + 1)
    sd = ref.state_dict()
    assert "egorear_amd" not in sd
    opt = train.FusedAdamW(net, warmup_iters=WARMUP, decay_all=decay_all)
    opt.load_state_dict(sd)
    assert opt.steps == 2 and abs(opt.lr_scale_epoch - 1.0) < 1e-12 and abs(opt.lr_at(3) - probe.lr_at(3)) < 1e-15
    byname = dict(ps)
    for k, o, n, _ in opt.slots:
        st = ref.state[byname[k]]
        assert torch.equal(opt.m[o:o + n], st["exp_avg"].reshape(-1)) and torch.equal(opt.v[o:o + n], st["exp_avg_sq"].reshape(-1)), k
    # a decayed rate (MultiStepLR's 0.1) is read back from the group's lr
    for g in sd["param_groups"]:
        g["lr"] = 0.1 * probe.lr_at(3)
    opt.load_state_dict(sd)
    assert abs(opt.lr_scale_epoch - 0.1) < 1e-12 and abs(opt.lr_at(3) - 0.1 * probe.lr_at(3)) < 1e-15


def _heatmap_data(seed, B=2):
    from egorear_amd import synth
    from egorear_amd.metrics import generate_target
    return synth.synth_images(B, 2, seed=seed).to(DEV), generate_target(synth.synth_joint_px(B, seed=40 + seed).to(DEV)).contiguous()


def _inside(net, flat):
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
    return all(lo <= p.data_ptr() and p.data_ptr() + p.numel() * 4 <= hi for p in net.parameters())


def test_trainer_checkpoint_inside_an_accumulation_group():
    from egorear_amd import train
    net = _heatmap_net()
    tr = train.HeatmapTrainer(net, accumulate=2)
    tr.opt.lr_scale_epoch = 0.1
    tr.step(*_heatmap_data(0))
    torch.cuda.synchronize()
    sd = tr.state_dict()
    assert set(sd) == {"optimizer", "lr_scale_epoch"} and sd["lr_scale_epoch"] == 0.1
    assert sd["optimizer"]["egorear_amd"]["micro"] == 1 and sd["optimizer"]["egorear_amd"]["accumulate"] == 2
    weights = {k: v.clone() for k, v in net.state_dict().items()}
    net2 = _heatmap_net()
    tr2 = train.HeatmapTrainer(net2, accumulate=2, use_graph=True)
    net2.load_state_dict(weights)
    assert _inside(net2, tr2.opt.flat_p)                    # an in-place load leaves the parameters where they are
    tr2.load_state_dict(sd)
    assert tr2.pending_micro_steps() == 1 and tr2.opt.steps == 0 and tr2.opt.lr_scale_epoch == 0.1
    assert torch.equal(tr2.opt.flat_acc, tr.opt.flat_acc) and tr2.opt.have_group == tr.opt.have_group
    assert torch.equal(tr2.opt.flat_p, tr.opt.flat_p)
    # a load that REPLACES the tensors: load_state_dict brings them home again, values kept
    net2.load_state_dict(weights, assign=True)
    assert not _inside(net2, tr2.opt.flat_p)
    tr2.load_state_dict(sd)
    assert _inside(net2, tr2.opt.flat_p) and torch.equal(tr2.opt.flat_p, tr.opt.flat_p)
    assert tr2.graph is None and tr2._eager_done == 0
    # both finish the group: one update each, from the same sum up to the reverse pass's own run-to-run noise
    tr.step(*_heatmap_data(1))
    tr2.step(*_heatmap_data(1))
    torch.cuda.synchronize()
    assert tr.opt.steps == tr2.opt.steps == 1 and tr2.pending_micro_steps() == 0
    assert abs(tr.opt.grad_norm() - tr2.opt.grad_norm()) <= 1e-4 * tr.opt.grad_norm()
    # a plain torch dict under the Trainer: "lr_scale_epoch" None / absent keeps what the optimizer read from param_groups[0]["lr"]
    plain = {k: v for k, v in tr.opt.state_dict().items() if k != "egorear_amd"}
    for g in plain["param_groups"]:
        g["lr"] = 0.1 * tr.opt.lr * min(1.0, tr.opt.steps / tr.opt.warmup)
    for wrapped in ({"optimizer": plain, "lr_scale_epoch": None}, {"optimizer": plain}):
        tr2.load_state_dict(wrapped)
        assert tr2.opt.steps == 1 and abs(tr2.opt.lr_scale_epoch - 0.1) < 1e-12 and tr2.pending_micro_steps() == 0
    # accumulate = 1 optimizers refuse a half-done group instead of dropping it
    with pytest.raises(ValueError):
        train.HeatmapTrainer(_heatmap_net()).load_state_dict(sd)


def test_half_done_group_is_refused_with_several_ranks(monkeypatch):
    """Inside a group flat_acc is a per-rank partial sum and Lightning saves rank 0 only: saving or loading it with more than one
    rank is refused; between groups the checkpoint goes through."""
    from egorear_amd import dist as D
    from egorear_amd import train
    tr = train.HeatmapTrainer(_heatmap_net(), accumulate=2)
    tr.step(*_heatmap_data(0))
    sd = tr.state_dict()
    monkeypatch.setattr(D, "world_size", lambda pg=None: 2)          # (what a two-rank process group would answer)
    with pytest.raises(RuntimeError, match="partial sum"):
        tr.state_dict()
    with pytest.raises(RuntimeError, match="partial sum"):
        tr.opt.load_state_dict(sd["optimizer"])
    assert tr.pending_micro_steps() == 1
    tr.opt.end_group()
    between = tr.state_dict()
    assert between["optimizer"]["egorear_amd"]["micro"] == 0
    tr.opt.load_state_dict(between["optimizer"])

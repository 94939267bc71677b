"""Gradient accumulation (Trainer(accumulate=k), Lightning's accumulate_grad_batches): the accumulation kernel against torch, the
plumbing of a group of micro-batches bit for bit, the accumulated gradient against the average of the two single-batch
gradients (k accumulated micro-batches are a k-rank data-parallel step), the update against float64 AdamW on the host, graph
replay, and the collectives of a process group: one per stage per UPDATE."""
import copy
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# --------------------------------------------------------------------------- the kernel

def _cap_blocks():
    from egorear_amd import hip_train
    return hip_train.GRAD_ACCUM_MAX_BLOCKS          # EGR_GRAD_ACCUM_MAX_BLOCKS of include/egorear_train.h: the launcher's grid cap


def _sizes():
    # the smallest range; a ragged last block (three full blocks of 256 lanes x 4 floats + one lane); one float4 per lane of the
    # capped grid and 257 more, so that the grid-stride loop goes round a second time in a ragged block
    return [4, 4 * (256 * 3 + 1), 4 * (2048 * 256 + 257)]


def test_the_large_size_is_beyond_the_grid_cap():
    assert _cap_blocks() == 2048 and _sizes()[-1] // 4 > _cap_blocks() * 256


@pytest.fixture(scope="module", params=_sizes())
def operands(request):
    """acc and g as views 4 floats (16 bytes: the least the flat layout guarantees) into larger buffers."""
    n = request.param
    gen = torch.Generator(device=DEV).manual_seed(n)
    a = torch.randn(n + 8, device=DEV, generator=gen)
    g = torch.randn(n + 8, device=DEV, generator=gen)
    assert a.data_ptr() % 32 == 0 and g.data_ptr() % 32 == 0
    return n, a, g


@pytest.mark.parametrize("from_device", [False, True])
def test_modes_against_torch(operands, from_device):
    from egorear_amd import hip_train as T
    n, a0, g0 = operands
    g = g0[4:4 + n]
    assert g.data_ptr() % 16 == 0 and g.data_ptr() % 32 != 0
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    for mode in (0, 1, 2):
        buf = a0.clone()
        acc = buf[4:4 + n]
        before = acc.clone()
        ss = torch.zeros(1, dtype=torch.float64, device=DEV)
        if from_device:
            T.set1_i32(word, mode)
            T.grad_accum(acc, g, word, ss)
        else:
            T.grad_accum(acc, g, mode, ss if mode == 2 else None)
        torch.cuda.synchronize()
        want = g if mode == 0 else before + g
        assert torch.equal(acc, want), (n, mode)                                   # one fp32 rounding per element: exact
        assert torch.equal(buf[:4], a0[:4]) and torch.equal(buf[4 + n:], a0[4 + n:]), (n, mode)       # nothing outside the range
        assert torch.equal(g, g0[4:4 + n])
        if mode == 2:
            ref = float(acc.double().square().sum())
            got = float(ss)
            print(f"n={n} sum of squares {got!r} vs {ref!r}: rel {abs(got - ref) / ref:.3e} (bound {n * 2.0 ** -53:.3e})")
            assert abs(got - ref) <= n * 2.0 ** -53 * ref, (n, got, ref)           # any summation order over non-negative doubles
        else:
            assert float(ss) == 0.0
    # mode 2 ADDS to what the double already holds
    buf = a0.clone()
    ss = torch.full((1,), 3.0, dtype=torch.float64, device=DEV)
    T.grad_accum(buf[4:4 + n], g, 2, ss)
    ref = 3.0 + float(buf[4:4 + n].double().square().sum())
    assert abs(float(ss) - ref) <= (n + 1) * 2.0 ** -53 * ref
    # a device word outside 0..2: the launch does nothing
    if from_device:
        buf = a0.clone()
        T.set1_i32(word, 7)
        T.grad_accum(buf[4:4 + n], g, word, ss)
        torch.cuda.synchronize()
        assert torch.equal(buf, a0)


def test_ranges_outside_the_slot_rules_are_refused():
    from egorear_amd import hip
    from egorear_amd import hip_train as T
    a, g = torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
    ss = torch.zeros(1, dtype=torch.float64, device=DEV)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    for acc, gg in ((a[:6], g[:6]), (a[1:9], g[4:12]), (a[4:12], g[1:9])):         # n % 4 != 0; a pointer off the 16-byte grid
        for mode in (1, word):
            with pytest.raises(hip.LaunchError) as e:
                T.grad_accum(acc, gg, mode, ss)
            assert e.value.code == hip.EINVAL
    with pytest.raises(hip.LaunchError) as e:
        T.grad_accum(a[:8], g[:8], 3, ss)
    assert e.value.code == hip.EINVAL
    torch.cuda.synchronize()
    assert float(a.abs().max()) == 0.0


# --------------------------------------------------------------------------- plumbing, heat-map model

def _heatmap_net():
    from egorear_amd import configs, synth
    from egorear_amd.estimator import EgoPoseFormerHeatmap
    net = EgoPoseFormerHeatmap(**copy.deepcopy(configs.heatmap_cfg()))
    synth.load_synth(net, 42)
    return net.to(DEV)


def _heatmap_data(seed, B=2):
    from egorear_amd import synth
    from egorear_amd.metrics import generate_target
    return synth.synth_images(B, 2, seed=seed).to(DEV), generate_target(synth.synth_joint_px(B, seed=40 + seed).to(DEV)).contiguous()


def test_three_micro_batches_accumulate_bit_for_bit(monkeypatch):
    from egorear_amd import train
    net = _heatmap_net()
    tr = train.HeatmapTrainer(net, accumulate=3)
    opt = tr.opt
    assert opt.flat_acc is not None and opt.flat_acc.shape == opt.flat_g.shape
    assert train.HeatmapTrainer(_heatmap_net()).opt.flat_acc is None                # only when asked for
    nbt = next(k for k, _ in net.named_buffers() if k.endswith("num_batches_tracked"))
    nbt0 = int(dict(net.named_buffers())[nbt])
    p0 = opt.flat_p.clone()
    seen = {}
    update = tr._update_group

    def spy(*a, **k):                     # in front of clip + AdamW
        torch.cuda.synchronize()
        seen["acc"], seen["p"], seen["steps"] = opt.flat_acc.clone(), opt.flat_p.clone(), opt.steps
        return update(*a, **k)
    monkeypatch.setattr(tr, "_update_group", spy)
    grads, steps, losses = [], [], []
    for i in range(3):
        assert tr.pending_micro_steps() == i
        terms, _ = tr.step(*_heatmap_data(i))
        torch.cuda.synchronize()
        grads.append(opt.flat_g.clone())
        steps.append(opt.steps)
        losses.append(float(terms.sum()))
        if i < 2:
            assert torch.equal(opt.flat_p, p0), i                                  # no update, no weight decay, nothing
    assert steps == [0, 0, 1] and tr.pending_micro_steps() == 0
    assert seen["steps"] == 0 and torch.equal(seen["p"], p0)
    assert torch.equal(seen["acc"], (grads[0] + grads[1]) + grads[2])
    assert not torch.equal(opt.flat_p, p0)
    assert int(dict(net.named_buffers())[nbt]) == nbt0 + 3
    assert all(np.isfinite(v) and v > 0 for v in losses)
    # the seed carries 1/3: a micro-batch's gradient is a third of the plain trainer's on the same weights and data, its loss terms are not
    ref = train.HeatmapTrainer(_heatmap_net())
    t_ref, _ = ref.step(*_heatmap_data(0))
    torch.cuda.synchronize()
    assert abs(float(t_ref.sum()) - losses[0]) <= 1e-5 * losses[0]          # (two runs of one forward: the bound the graph tests use)
    n3, n1 = float(grads[0].double().norm()), float(ref.opt.flat_g.double().norm())
    assert abs(3.0 * n3 - n1) <= 1e-4 * n1, (n3, n1)
    # the fused sum of squares is the norm of the accumulated gradient
    assert abs(opt.grad_norm() - float(seen["acc"].double().norm())) <= 1e-6 * opt.grad_norm()


def test_flush_updates_from_a_short_tail():
    from egorear_amd import train
    tr = train.HeatmapTrainer(_heatmap_net(), accumulate=3)
    assert tr.flush() is False and tr.opt.steps == 0
    p0 = tr.opt.flat_p.clone()
    tr.step(*_heatmap_data(0))
    tr.step(*_heatmap_data(1))
    acc = tr.opt.flat_acc.clone()
    assert tr.pending_micro_steps() == 2 and tr.flush() is True
    torch.cuda.synchronize()
    assert tr.pending_micro_steps() == 0 and tr.opt.steps == 1 and not torch.equal(tr.opt.flat_p, p0)
    assert abs(tr.opt.grad_norm() - float(acc.double().norm())) <= 1e-6 * tr.opt.grad_norm()      # the sum as it stands: 1/3 seeds kept
    tr.step(*_heatmap_data(2))                                                    # the next group starts over
    assert tr.pending_micro_steps() == 1 and tr.opt.steps == 1
    torch.cuda.synchronize()
    assert torch.equal(tr.opt.flat_acc, tr.opt.flat_g)


# --------------------------------------------------------------------------- config 5: the two-shard average and the update

def _full_net():
    from egorear_amd import configs, synth
    from egorear_amd.estimator import EgoPoseFormerMVFEX
    net = EgoPoseFormerMVFEX(**copy.deepcopy(configs.pose3d_cfg("ego4view_rw")))
    synth.load_synth(net, 42)
    return net.to(DEV)


def _full_data(seed, B=2):
    from egorear_amd import synth
    from egorear_amd.metrics import generate_target
    return (synth.synth_images(B, 4, seed=10 + seed).to(DEV), synth.synth_coord_trans_mat(B, seed=20 + seed).to(DEV),
            synth.synth_gt_pose(B, seed=30 + seed).to(DEV), generate_target(synth.synth_joint_px(B, seed=40 + seed).to(DEV)).contiguous())


def _sample_idx(numel, n=16):
    step = max(1, numel // n)
    return np.arange(0, numel, step)[:n]


def test_two_accumulated_batches_equal_the_two_shard_average_and_update_like_float64_adamw():
    from egorear_amd import train
    net = _full_net()
    tr = train.Trainer(net, accumulate=2)
    opt = tr.opt
    before = opt.flat_p.clone()
    bufs = []
    for i in range(2):
        bufs.append({k: b.clone() for k, b in net.named_buffers()})                # what this micro-batch's forward saw
        tr.step(*_full_data(i))
    torch.cuda.synchronize()
    assert opt.steps == 1 and tr.pending_micro_steps() == 0
    acc = opt.flat_acc.clone()
    # --- the expected gradient: 0.5 (g_A + g_B) from the un-accumulated path on the same weights
    other = _full_net()
    ref = []
    for i in range(2):
        own = dict(other.named_buffers())
        with torch.no_grad():
            for k, b in bufs[i].items():
                own[k].copy_(b)
        S, _ = train.forward_backward(other, *_full_data(i))
        ref.append({k: g.clone() for k, g in S.pgrads.items()})
    torch.cuda.synchronize()
    shapes = {k: p.shape for k, p in net.named_parameters()}
    checked = 0
    for k, o, n, _ in opt.slots:
        mine = acc[o:o + n]
        if k not in ref[0]:
            assert float(mine.abs().max()) == 0.0, k
            continue
        avg = (0.5 * (ref[0][k] + ref[1][k])).reshape(-1)
        n_ref, norm = float(avg.double().norm()), float(mine.double().norm())
        assert abs(norm - n_ref) <= 1e-4 * n_ref + 1e-7, (k, norm, n_ref)
        idx = torch.from_numpy(_sample_idx(n)).to(DEV)
        np.testing.assert_allclose(mine[idx].cpu().numpy(), avg[idx].cpu().numpy(), rtol=1e-3, atol=1e-5 * max(n_ref, 1e-6), err_msg=k)
        checked += 1
    assert checked > 400
    # --- the update: float64 clip + AdamW (first update: zero moments, full lr) on the host, from the measured flat_acc
    lr, b1, b2, eps, clip = opt.lr, opt.betas[0], opt.betas[1], opt.eps, opt.clip
    total = float(acc.double().square().sum().sqrt())
    assert abs(opt.grad_norm() - total) <= 1e-6 * total
    coef = min(1.0, clip / (total + 1e-6))
    after = opt.flat_p
    bad = []
    for k, o, n, decay in opt.slots:
        idx = _sample_idx(n) + o
        ti = torch.from_numpy(idx).to(DEV)
        p_old, p_new = before[ti].cpu().numpy().astype(np.float64), after[ti].cpu().numpy().astype(np.float64)
        d = (p_new - p_old).astype(np.float32)
        if k not in ref[0]:
            assert (d == 0).all(), k
            continue
        g = acc[ti].cpu().numpy().astype(np.float64) * coef
        m, v = (1 - b1) * g, (1 - b2) * g * g
        p_ref = p_old * (1 - lr * (opt.wd if decay else 0.0))
        p_ref = p_ref - (lr / (1 - b1)) * m / (np.sqrt(v) / np.sqrt(1 - b2) + eps)
        ref_d = (p_ref - p_old).astype(np.float32)
        gn = float(acc[o:o + n].double().norm())
        ok = np.abs(g) > 1e-6 * max(gn, 1e-12)
        big = np.abs(ref_d) >= 0.9e-3
        err = np.abs(d - ref_d)
        u, ur = np.clip(d / 1e-3, -0.999, 0.999), np.clip(ref_d / 1e-3, -0.999, 0.999)
        g_err = 1e-8 * np.abs(u / (1 - np.abs(u)) - ur / (1 - np.abs(ur)))
        g_tol = 4e-3 * max(gn, 1e-3) / np.sqrt(max(n, 1)) + 2e-3 * np.abs(g).max()
        wrong = (err > np.where(big, 2e-5, 1e-4)) & (big | (g_err > g_tol))
        if wrong[ok].any():
            bad.append((k, d[ok], ref_d[ok]))
    assert not bad, f"{len(bad)} parameters moved differently, e.g. {bad[0]}"


# --------------------------------------------------------------------------- graph replay

def test_graphed_micro_steps_follow_the_eager_trajectory_with_two_captures(monkeypatch):
    from egorear_amd import train
    made = []
    real = torch.cuda.CUDAGraph

    def counting(*a, **k):
        g = real(*a, **k)
        made.append(g)
        return g
    monkeypatch.setattr(torch.cuda, "CUDAGraph", counting)
    eager, graphed = train.Trainer(_full_net(), accumulate=2), train.Trainer(_full_net(), accumulate=2, use_graph=True)
    for t in range(6):
        args = _full_data(t)
        le, _ = eager.step(*args)
        lg, _ = graphed.step(*args)
        torch.cuda.synchronize()
        assert abs(float(le.sum()) - float(lg.sum())) <= 1e-5 * abs(float(le.sum())), (t, float(le.sum()), float(lg.sum()))
        assert graphed.pending_micro_steps() == eager.pending_micro_steps() == (t + 1) % 2
    assert graphed.graph is not None and graphed._tail is not None, "capture was refused"
    assert len(made) <= 2, len(made)                       # the micro-step body and the update tail; nothing per micro-step
    assert graphed.opt.steps == eager.opt.steps == 3
    for (k, p), (_, q) in zip(eager.net.named_parameters(), graphed.net.named_parameters()):
        if "k_proj.bias" not in k:
            assert float(((p - q).abs() > 2e-4).float().mean()) < 0.02, k


def test_graph_with_a_process_group_and_accumulation_is_refused_before_anything_runs():
    from egorear_amd import train
    tr = train.HeatmapTrainer(_heatmap_net(), accumulate=2, use_graph=True)
    tr.opt.force_collective = True
    nbt = next(b for k, b in tr.net.named_buffers() if k.endswith("num_batches_tracked"))
    n0 = int(nbt)
    with pytest.raises(NotImplementedError):
        tr.step(*_heatmap_data(0))
    assert int(nbt) == n0 and tr.pending_micro_steps() == 0


# --------------------------------------------------------------------------- one collective per stage per update

def _rccl_accum_worker(port, out):
    """One rank, backend "nccl" (= RCCL), force_collective: the stage all-reduces run through the same async handles as a real job."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        from egorear_amd import train
        tr = train.Trainer(_full_net(), accumulate=2)
        opt = tr.opt
        opt.force_collective = True
        calls, micro = [], [0]
        reduce_stage = opt.reduce_stage

        def counted(stage, *a, **k):
            calls.append((micro[0], stage))
            return reduce_stage(stage, *a, **k)
        opt.reduce_stage = counted
        grads = []
        for i in range(2):
            micro[0] = i + 1
            tr.step(*_full_data(i, B=1))
            torch.cuda.synchronize()
            grads.append(opt.flat_g.clone())
        exact = bool(torch.equal(opt.flat_acc, grads[0] + grads[1]))           # per-stage accumulation covers the whole buffer
        norm_ok = abs(opt.grad_norm() - float(opt.flat_acc.double().norm())) <= 1e-6 * opt.grad_norm()
        res = dict(calls=list(calls), stages=sorted(opt.stage_range), steps=opt.steps, pending=len(opt.pending), exact=exact, norm_ok=norm_ok)
        # an epoch's short tail: one micro-batch (no collective), then flush() - every stage of the pending sum reduced once, then the update
        del calls[:]
        micro[0] = 3
        tr.step(*_full_data(2, B=1))
        torch.cuda.synchronize()
        acc = opt.flat_acc.clone()
        micro[0] = "flush"
        flushed = tr.flush()
        torch.cuda.synchronize()
        res.update(tail_calls=list(calls), flushed=flushed, tail_steps=opt.steps, tail_pending=len(opt.pending), tail_micro=tr.pending_micro_steps(),
                   tail_norm_ok=abs(opt.grad_norm() - float(acc.double().norm())) <= 1e-6 * opt.grad_norm())
        out.put((res, None))
    except Exception as exc:  # noqa: BLE001 - reported to the parent
        out.put((None, f"{type(exc).__name__}: {exc}"))
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def rccl_run():
    """The one-rank RCCL worker, run once for the tests below."""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    p = ctx.Process(target=_rccl_accum_worker, args=(port, out))
    p.start()
    res, err = out.get(timeout=600)
    p.join(timeout=120)
    assert err is None, err
    assert p.exitcode == 0
    return res


def test_every_stage_is_reduced_once_per_update_during_the_last_micro_batch(rccl_run):
    r = rccl_run
    assert r["steps"] == 1 and r["pending"] == 0
    assert len(r["stages"]) >= 2
    assert all(m == 2 for m, _ in r["calls"]), r["calls"]                       # none during the first micro-batch (DDP's no_sync)
    assert sorted(st for _, st in r["calls"]) == r["stages"], (r["calls"], r["stages"])       # every stage exactly once
    assert r["exact"] and r["norm_ok"]


def test_flush_with_a_process_group_reduces_every_stage_of_the_pending_sum(rccl_run):
    """Micro-batches before a group's last one issue no collective, so the short tail's sum is still a per-rank one when flush() is
    called: it must go through the all-reduce, every stage once, before the norm is taken and the update runs."""
    r = rccl_run
    assert r["flushed"] is True and r["tail_steps"] == 2 and r["tail_pending"] == 0 and r["tail_micro"] == 0
    assert all(m == "flush" for m, _ in r["tail_calls"]), r["tail_calls"]       # none during the tail's micro-batch
    assert sorted(st for _, st in r["tail_calls"]) == r["stages"], (r["tail_calls"], r["stages"])
    assert r["tail_norm_ok"]

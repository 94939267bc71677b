"""The half-precision training policy end to end (hip.LaunchPolicy.fast_training()): the stage-3 step (train.Trainer) and
the stage-1 step (train.HeatmapTrainer) at batch 2 on the seeded weights and inputs of tests/test_gpu_train_step.py /
test_gpu_train_stages.py, with the thresholds forced down so that the small batch reaches the kernels the mode changes (role-split
route from one tile up on eight workgroups, split launches and split weight gradients at every size).  The parity contract does NOT
apply to this policy; what is asserted is the launch structure, that the step is a working optimisation step, the policy guard, and
the distance to the default-policy step of the same process on the same inputs.

Deviation from the default step (update 1, same weights, same inputs), measured on the first GPU run of this file and recorded in
DESIGN.md 5l; next to it the same three figures for exact() against default - the project's own noise floor between two arithmetics
that both hold the parity contract:

    stage      policy           |loss - loss_d| / loss_d   |g - g_d| / |g_d| (flat)   worst tensor
    stage 3    fast_training    1.7e-05                      5.8e-04                     1.7e+00 (a k_proj.bias: exactly-zero gradient, rounding noise); median tensor 3.0e-02
    stage 3    exact            4.0e-08                      6.3e-06                     1.9e+00 (a k_proj.bias); median tensor 2.0e-06
    stage 1    fast_training    1.1e-04                      6.8e-04                     7.0e-02 (encoder.backbone.layer_s16.0.bn1.bias); median tensor 2.1e-02
    stage 1    exact            6.1e-08                      1.8e-05                     2.3e-03 (encoder.backbone.layer_s32.1.conv1.weight); median tensor 6.2e-04

The flat-gradient figure is gated at 10 x its measured value (FLAT_GATE below): ReLU masks at rounding level flip with the summation
order and differ between machines, so the margin is wide; the measurement is against the default policy, never against a second run
of the fast one.  Per-tensor figures are printed, not gated."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 2
# 10 x the flat-gradient deviation of fast_training() from the default step measured on the first GPU run (docstring table)
FLAT_GATE = {"stage3": 5.8e-3, "stage1": 6.8e-3}


def _forced(pol):
    return pol.replace(x6_train_min_rows=0, x6_train_min_flops=0.0, wgrad_force=True)


def _make(stage, seed_net={}):
    """(a fresh module on the seeded weights, trainer class, the step's arguments)."""
    from egorear_amd import configs, synth, train
    from egorear_amd.estimator import EgoPoseFormerHeatmap, EgoPoseFormerMVFEX
    from oracle import train_oracle as TO
    if stage not in seed_net:
        if stage == "stage3":
            net = EgoPoseFormerMVFEX(**copy.deepcopy(configs.pose3d_cfg("ego4view_rw")))
            args = (synth.synth_images(B, 4, seed=0), synth.synth_coord_trans_mat(B), synth.synth_gt_pose(B), TO.synth_gt_heatmap(B))
        else:
            net = EgoPoseFormerHeatmap(**copy.deepcopy(configs.heatmap_cfg()))
            args = (synth.synth_images(B, 2, seed=0), TO.synth_gt_heatmap(B))
        synth.load_synth(net, 42)
        seed_net[stage] = (net, tuple(a.to(DEV) for a in args))
    net, args = seed_net[stage]
    return copy.deepcopy(net).to(DEV), (train.Trainer if stage == "stage3" else train.HeatmapTrainer), args


@pytest.fixture(scope="module")
def forced_knobs():
    from egorear_amd import hip
    hip.lib.egr_conv_set_tapx(1, 1, 8)
    yield hip
    hip.lib.egr_conv_set_tapx(1, 256, 256)
    hip.PROFILE = hip.PLAN_LOG = None


@pytest.fixture(scope="module", params=["stage3", "stage1"])
def runs(request, forced_knobs):
    """Two eager updates per policy (default, exact, fast_training - the same forcing), the first one instrumented."""
    hip = forced_knobs
    stage = request.param
    out = {}
    orig = hip.conv2d_wgrad
    for name, pol in (("default", hip.LaunchPolicy()), ("exact", hip.LaunchPolicy().exact()), ("fast", hip.LaunchPolicy.fast_training())):
        net, cls, args = _make(stage)
        before = {k: p.detach().clone() for k, p in net.named_parameters()}
        wg = []

        def spy(*a, **k):
            r = orig(*a, **k)
            wg.append((hip.lib.egr_wgrad_last_kernel(), hip.lib.egr_wgrad_last_planes()))
            return r
        with hip.use_policy(_forced(pol)):
            tr = cls(net)
            hip.conv2d_wgrad, hip.PROFILE, hip.PLAN_LOG = spy, [], []
            try:
                full = args if stage == "stage3" else (args[0], None, None, args[1])
                S, _ = tr._run(*full, update=True)          # (one eager update, as Trainer.step runs it, with the Step in hand)
                tr._eager_done += 1
                tr._invalidate()
                torch.cuda.synchronize()
                tags, plans = [(n, t) for n, *_, t in hip.PROFILE], hip.PLAN_LOG
            finally:
                hip.conv2d_wgrad, hip.PROFILE, hip.PLAN_LOG = orig, None, None
            terms1, have, flat = S.loss_terms.double().cpu().clone(), set(S.pgrads.keys()), tr.opt.flat_g.clone()
            per = {k: tr.opt.gviews[k].clone() for k in have}
            terms2, _ = tr.step(*args)
            torch.cuda.synchronize()
        out[name] = dict(net=net, tr=tr, before=before, wg=wg, tags=tags, plans=plans, terms=[terms1, terms2.double().cpu()], have=have,
                         flat=flat, per=per, sd=tr.state_dict())
    return stage, out


def test_launch_structure(runs, forced_knobs):
    hip = forced_knobs
    stage, r = runs
    d, f = r["default"], r["fast"]
    # the default policy under the same forcing: no one-product launch anywhere
    assert all(p.planes != 1 for _, p in d["plans"]) and all(pl != 1 for _, pl in d["wg"])
    assert not any(t.startswith(("h1 ", "T h1 ")) for _, t in d["tags"])
    # fast_training(): every kind of launch the mode covers took one product at least once
    one = [(t, p) for t, p in f["plans"] if p.planes == 1]
    assert all(p.route == hip.ROUTE_TAPX for _, p in one)
    kinds = {"stats": sum(1 for _, p in one if p.variant // 100 == 11), "masked": sum(1 for _, p in one if p.variant // 100 == 12),
             "plain dgrad / forward": sum(1 for _, p in one if p.variant // 100 == 10)}
    tdg = sum(1 for n, t in f["tags"] if n == "egr_conv2d_nhwc_f32" and t.startswith("T h1 ") and "masked" not in t)
    wk = {k: sum(1 for kk, pl in f["wg"] if kk == k and pl == 1) for k in (1, 2, 3)}
    print(f"{stage}: one-product role-split launches {kinds}, plain data gradients among them {tdg}, one-product weight gradients by kernel {wk}, "
          f"of {len(f['plans'])} conv plans and {len(f['wg'])} weight-gradient calls")
    assert kinds["stats"] >= 1 and kinds["masked"] >= 1 and tdg >= 1, (kinds, tdg)
    assert all(wk[k] >= 1 for k in (1, 2, 3)), wk
    assert not any(pl == 2 for _, pl in f["wg"]), "a split weight gradient in the fp16 scheme stayed on three products"
    # the same launches in the same order; a tag changes only on a role-split conv launch or a weight gradient, and only h2 -> h1
    assert len(d["tags"]) == len(f["tags"]) and len(d["plans"]) == len(f["plans"])
    for (n0, t0), (n1, t1) in zip(d["tags"], f["tags"]):
        assert n0 == n1, (n0, n1)
        if t0 != t1:
            assert n0 in ("egr_conv2d_nhwc_f32", "egr_conv2d_wgrad_f32") and t1.replace("h1 ", "h2 ", 1) == t0, (n0, t0, t1)
    for (t0, p0), (t1, p1) in zip(d["plans"], f["plans"]):
        if p1.planes == 1:
            assert p0.route == hip.ROUTE_TAPX and p0.planes == 2 and p1.variant == p0.variant + 1000 and t1.startswith("h1 ") and t0.startswith("h2 ")
            assert (p0.bm, p0.bn, p0.grid_x, p0.persistent) == (p1.bm, p1.bn, p1.grid_x, p1.persistent)
        else:
            assert t0 == t1 and all(getattr(p0, fl) == getattr(p1, fl) for fl, _ in hip.ConvPlan._fields_), (t0, t1)


def test_step_results(runs):
    stage, r = runs
    d, f = r["default"], r["fast"]
    for t in f["terms"]:
        assert bool(torch.isfinite(t).all()) and len(t) == len(d["terms"][0])
    assert bool(torch.isfinite(f["flat"]).all())
    assert f["have"] == d["have"], sorted(f["have"] ^ d["have"])[:8]            # tensors without a gradient are the default step's
    moved = lambda x: {k for k, p in x["net"].named_parameters() if not torch.equal(p.detach(), x["before"][k])}
    mf, md = moved(f), moved(d)
    assert mf == md, sorted(mf ^ md)[:8]
    firm = {k for k in f["have"] if float(f["per"][k].abs().max()) > 0}
    assert firm <= mf and not (mf - f["have"]), (sorted(firm - mf)[:8], sorted(mf - f["have"])[:8])

    def sig(o):          # keys and shapes of a checkpoint, values aside
        if torch.is_tensor(o):
            return ("tensor", tuple(o.shape), str(o.dtype))
        if isinstance(o, dict):
            return {k: sig(v) for k, v in o.items()}
        if isinstance(o, (list, tuple)):
            return [sig(v) for v in o]
        return type(o).__name__
    assert sig(f["sd"]) == sig(d["sd"])


def test_deviation_from_the_default_step(runs):
    stage, r = runs
    d = r["default"]
    fig = {}
    for name in ("fast", "exact"):
        x = r[name]
        l0, l1 = float(d["terms"][0].sum()), float(x["terms"][0].sum())
        flat = float((x["flat"].double() - d["flat"].double()).norm() / d["flat"].double().norm())
        per = sorted(((float((x["per"][k].double() - d["per"][k].double()).norm() / max(float(d["per"][k].double().norm()), 1e-30)), k)
                      for k in d["have"] if float(d["per"][k].abs().max()) > 0), reverse=True)
        fig[name] = (abs(l1 - l0) / abs(l0), flat, per[0])
        print(f"{stage} {name} against default: relative loss difference {fig[name][0]:.3e}, flat gradient {flat:.3e}, "
              f"worst tensor {per[0][0]:.3e} ({per[0][1]}), median tensor {per[len(per) // 2][0]:.3e}")
    assert fig["fast"][1] > 0.0, "the policy took no effect"
    assert fig["fast"][1] <= FLAT_GATE[stage], (stage, fig["fast"][1], FLAT_GATE[stage])


def test_policy_guard(runs, forced_knobs):
    """A PackCache made under fast_training() is refused under fast() (and under the default), and the reverse - the existing check."""
    hip = forced_knobs
    stage, r = runs
    args = _make(stage)[2]
    for made, others in (("fast", (hip.LaunchPolicy.fast(), hip.LaunchPolicy())), ("default", (hip.LaunchPolicy.fast_training(),))):
        for other in others:
            with hip.use_policy(_forced(other)):
                with pytest.raises(RuntimeError, match="launch policy"):
                    r[made]["tr"].step(*args)
    if stage == "stage1":         # a cache made under fast(): refused under fast_training()
        net, cls, args = _make(stage)
        with hip.use_policy(_forced(hip.LaunchPolicy.fast())):
            tr = cls(net)
            tr.step(*args)
        with hip.use_policy(_forced(hip.LaunchPolicy.fast_training())):
            with pytest.raises(RuntimeError, match="launch policy"):
                tr.step(*args)


@pytest.mark.parametrize("stage", ["stage3", "stage1"])
def test_graph_replay_follows_the_eager_steps(forced_knobs, stage):
    """use_graph under fast_training(): two eager steps, then the captured step replayed - the loss trajectory of four eager steps (the
    criterion of test_stage_trainer_graph_replay_follows_the_eager_steps)."""
    hip = forced_knobs
    traj = []
    with hip.use_policy(_forced(hip.LaunchPolicy.fast_training())):
        for use_graph in (False, True):
            net, cls, args = _make(stage)
            tr = cls(net, use_graph=use_graph)
            vals = []
            for _ in range(4):
                terms, _ = tr.step(*args)
                vals.append(float(terms.sum()))
            assert (tr.graph is not None) == use_graph
            traj.append(vals)
    for a, b in zip(*traj):
        assert abs(a - b) <= 2e-3 * abs(a), traj
    # ... and the loss goes down: the stage-1 condition of that test.  Four stage-3 updates from the seeded weights do not lower the loss
    # under either policy (update 1 runs at the full rate); test_one_batch_overfit holds that condition for stage 3 over 30 updates.
    if stage == "stage1":
        assert traj[0][3] < traj[0][0]


def test_one_batch_overfit(forced_knobs):
    """30 updates on one fixed batch (stage 3, warmup_iters=1, the same initial weights): under both policies the total loss after the
    last update is below the loss at update 0."""
    hip = forced_knobs
    curves = {}
    for name, pol in (("default", hip.LaunchPolicy()), ("fast_training", hip.LaunchPolicy.fast_training())):
        net, cls, args = _make("stage3")
        with hip.use_policy(_forced(pol)):
            tr = cls(net, warmup_iters=1, use_graph=True)
            # (the loss a step returns is the loss BEFORE its update; a replayed step returns the captured tensor: read it at once)
            curves[name] = [float(tr.step(*args)[0].sum()) for _ in range(31)]
        print(f"overfit {name}: loss {curves[name][0]:.4f} -> {curves[name][-1]:.4f} (min {min(curves[name]):.4f})")
    for name, c in curves.items():
        assert all(v == v for v in c) and c[-1] < c[0], (name, c[0], c[-1])

"""The numbering between torch.optim.AdamW's state and the slots of the native optimizer's flat buffers (train.optimizer_state_map,
pack_optimizer_state / unpack_optimizer_state): pure functions of [(name, shape)], checked here without a device against the
parameter lists of the real models (built on the meta device) and against a real torch.optim.AdamW built the reference's way
(pose_3d_mvf_ex.py:219-234 two groups; heatmap.py:151-154 one group) on small stand-ins that keep the real names."""
import copy

import pytest
import torch

from egorear_amd import configs
from egorear_amd.train import (is_no_decay, optimizer_state_map, pack_optimizer_state, unpack_optimizer_state)

HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4)


def _named_shapes(kind):
    from egorear_amd.estimator import EgoPoseFormerHeatmap, EgoPoseFormerMVFEX
    with torch.device("meta"):
        if kind == "full":
            net = EgoPoseFormerMVFEX(**copy.deepcopy(configs.pose3d_cfg("ego4view_rw")))
        else:
            net = EgoPoseFormerHeatmap(**copy.deepcopy(configs.heatmap_cfg()))
    return [(k, tuple(p.shape)) for k, p in net.named_parameters()]


@pytest.fixture(scope="module", params=["full", "heatmap"])
def model(request):
    named = _named_shapes(request.param)
    return request.param, named, request.param == "heatmap"       # (kind, [(name, shape)], decay_all)


def _shrink(named, cap=6):
    """The same names with every dimension cut to at most `cap`: the real models' moments would take gigabytes on the host."""
    return [(k, tuple(min(d, cap) for d in shape)) for k, shape in named]


def _reference_adamw(named, decay_all):
    """torch.optim.AdamW the way the reference's configure_optimizers builds it, on CPU stand-ins."""
    ps = [(k, torch.nn.Parameter(torch.zeros(shape))) for k, shape in named]
    if decay_all:
        return ps, torch.optim.AdamW([p for _, p in ps], lr=HYPER["lr"], weight_decay=HYPER["weight_decay"])
    no_decay = [p for k, p in ps if 'norm' in k or 'bn' in k or 'ln' in k or 'bias' in k]
    other = [p for k, p in ps if not ('norm' in k or 'bn' in k or 'ln' in k or 'bias' in k)]
    return ps, torch.optim.AdamW([{"params": no_decay, "weight_decay": 0.0}, {"params": other}], lr=HYPER["lr"],
                                 weight_decay=HYPER["weight_decay"])


def test_every_parameter_sits_in_exactly_one_group(model):
    kind, named, decay_all = model
    sm = optimizer_state_map(named, decay_all)
    assert len(named) > 50 and len(sm.entries) == len(named)
    flat = [i for g in sm.groups for i in g]
    assert sorted(flat) == list(range(len(named))) and flat == list(range(len(named)))     # a permutation, numbered 0.. across the groups
    assert [e[0] for e in sm.entries] == list(range(len(named)))
    assert sorted(e[2] for e in sm.entries) == sorted(k for k, _ in named)
    shapes = dict(named)
    for i, g, k, shape, o, n in sm.entries:
        assert i in sm.groups[g] and tuple(shape) == shapes[k] and n == torch.Size(shapes[k]).numel() and o % 4 == 0
    if decay_all:
        assert len(sm.groups) == 1 and sm.decay == [True]
        assert [e[2] for e in sm.entries] == [k for k, _ in named]                          # parameters() order
    else:
        assert len(sm.groups) == 2 and sm.decay == [False, True]
        for i, g, k, *_ in sm.entries:
            assert (g == 0) == is_no_decay(k), k
        for g in (0, 1):                                                                    # named_parameters() order inside a group
            assert [e[2] for e in sm.entries if e[1] == g] == [k for k, _ in named if is_no_decay(k) == (g == 0)]
        assert sm.groups[0] and sm.groups[1]
    # the slots tile the flat buffer without overlap
    spans = sorted((o, o + n) for _, _, _, _, o, n in sm.entries)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= sm.total


def test_numbering_is_the_reference_optimizers(model):
    """The index torch gives a parameter (position in the concatenated `params` lists) is the map's."""
    kind, named, decay_all = model
    small = _shrink(named)
    ps, opt = _reference_adamw(small, decay_all)
    sm = optimizer_state_map(small, decay_all)
    by_id = {id(p): k for k, p in ps}
    torch_names = [by_id[id(p)] for g in opt.param_groups for p in g["params"]]
    assert torch_names == [e[2] for e in sm.entries]
    assert [len(g["params"]) for g in opt.param_groups] == [len(g) for g in sm.groups]
    assert [g["weight_decay"] for g in opt.param_groups] == [HYPER["weight_decay"] if d else 0.0 for d in sm.decay]


def _random_state(sm, seed=0):
    gen = torch.Generator().manual_seed(seed)
    m, v = torch.zeros(sm.total), torch.zeros(sm.total)
    for _, _, _, _, o, n in sm.entries:           # (the alignment gaps between slots stay zero, as in the optimizer's buffers)
        m[o:o + n] = torch.randn(n, generator=gen)
        v[o:o + n] = torch.rand(n, generator=gen)
    return m, v


def test_state_loads_into_torch_adamw_and_round_trips(model):
    kind, named, decay_all = model
    small = _shrink(named)
    sm = optimizer_state_map(small, decay_all)
    m, v = _random_state(sm)
    extra = {"steps": 7, "lr_scale_epoch": 0.1, "accumulate": 2, "micro": 0}
    sd = pack_optimizer_state(sm, m, v, 7, 1e-3 * 7 / 500, extra=extra, **HYPER)
    assert set(sd) == {"state", "param_groups", "egorear_amd"}
    ps, opt = _reference_adamw(small, decay_all)
    opt.load_state_dict(sd)                                         # the extra top-level key is present during the load
    shapes = dict(small)
    for i, _, k, shape, o, n in sm.entries:
        st = opt.state[ps_by_name(ps, k)]
        assert float(st["step"]) == 7.0
        assert torch.equal(st["exp_avg"], m[o:o + n].view(shapes[k])) and torch.equal(st["exp_avg_sq"], v[o:o + n].view(shapes[k]))
    assert all(abs(g["lr"] - 1e-3 * 7 / 500) < 1e-15 for g in opt.param_groups)
    ps2, opt2 = _reference_adamw(small, decay_all)                  # and torch steps from it (on a copy: torch.optim keeps the
    opt2.load_state_dict(copy.deepcopy(sd))                         # loaded tensors themselves and updates them in place)
    for _, p in ps2:
        p.grad = torch.ones_like(p)
    opt2.step()
    assert float(opt2.state[ps2[0][1]]["step"]) == 8.0
    # state -> flat -> state, from our dict and from what torch hands back (its group keys differ by version: ignored)
    for src in (sd, _reference_loaded(small, decay_all, sd)):
        m2, v2 = torch.full((sm.total,), 9.0), torch.full((sm.total,), 9.0)
        steps, lr0 = unpack_optimizer_state(sm, src, m2, v2)
        assert steps == 7 and abs(lr0 - 1e-3 * 7 / 500) < 1e-15
        assert torch.equal(m2, m) and torch.equal(v2, v)
        again = pack_optimizer_state(sm, m2, v2, steps, lr0, **HYPER)
        for i in sd["state"]:
            for key in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(again["state"][i][key], sd["state"][i][key]), (i, key)


def ps_by_name(ps, name):
    return dict(ps)[name]


def _reference_loaded(small, decay_all, sd):
    _, opt = _reference_adamw(small, decay_all)
    opt.load_state_dict(copy.deepcopy(sd))
    return opt.state_dict()


def test_missing_moments_load_as_zero_and_unknown_group_keys_are_ignored(model):
    kind, named, decay_all = model
    small = _shrink(named)
    sm = optimizer_state_map(small, decay_all)
    m, v = _random_state(sm, 1)
    sd = pack_optimizer_state(sm, m, v, 3, 1e-3, **HYPER)
    gone = sm.entries[len(sm.entries) // 2]
    del sd["state"][gone[0]]                                        # torch creates state lazily: a tensor without a gradient has none
    for g in sd["param_groups"]:
        g["some_future_switch"] = None
    m2, v2 = torch.ones(sm.total), torch.ones(sm.total)
    steps, _ = unpack_optimizer_state(sm, sd, m2, v2)
    o, n = gone[4], gone[5]
    assert steps == 3 and float(m2[o:o + n].abs().max()) == 0.0 and float(v2[o:o + n].abs().max()) == 0.0
    m[o:o + n], v[o:o + n] = 0.0, 0.0
    assert torch.equal(m2, m) and torch.equal(v2, v)


def test_wrong_shape_or_count_raises_and_names_the_offender(model):
    kind, named, decay_all = model
    small = _shrink(named)
    sm = optimizer_state_map(small, decay_all)
    m, v = _random_state(sm, 2)
    sd = pack_optimizer_state(sm, m, v, 3, 1e-3, **HYPER)
    victim = next(e for e in sm.entries if e[5] > 1)
    sd["state"][victim[0]]["exp_avg_sq"] = torch.zeros(victim[5] + 1)
    m2, v2 = torch.full((sm.total,), 5.0), torch.full((sm.total,), 5.0)
    with pytest.raises(ValueError, match=victim[2].replace(".", r"\.")):
        unpack_optimizer_state(sm, sd, m2, v2)
    assert float(m2.min()) == 5.0 and float(v2.min()) == 5.0        # nothing was written
    sd = pack_optimizer_state(sm, m, v, 3, 1e-3, **HYPER)
    sd["param_groups"][-1]["params"] = sd["param_groups"][-1]["params"][:-1]
    with pytest.raises(ValueError, match=sm.entries[-1][2].replace(".", r"\.")):
        unpack_optimizer_state(sm, sd, m2, v2)
    sd = pack_optimizer_state(sm, m, v, 3, 1e-3, **HYPER)
    sd["param_groups"] = sd["param_groups"] + [dict(sd["param_groups"][0], params=[])]
    with pytest.raises(ValueError):
        unpack_optimizer_state(sm, sd, m2, v2)

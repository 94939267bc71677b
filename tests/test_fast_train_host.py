"""The half-precision training policy on the host: what the conv dispatch plans when EGR_W_F16X1T rides on
EGR_W_F16X2 | EGR_W_F16X1, what egr_conv2d_wgrad_ex_f32 accepts before it touches a device, and the LaunchPolicy that selects the mode.
No device is touched: egr_conv_plan with the fake aligned pointers of tests/test_conv_plan.py over the fp16-scheme rows of its table
(tests/golden/conv_plan_cases.json), and a weight-gradient call that is refused by its argument checks.

Against the plan of the same row under EGR_W_F16X2 alone: a role-split row with a mask, a statistics epilogue or the transposed flag
keeps every field but planes (2 -> 1) and variant (+ 1000); a role-split forward row moves as it does under EGR_W_F16X1; every other row
- another route, a refusal - is equal."""
import ctypes as C
import importlib.util
import json
import os

import pytest

from egorear_amd import hip

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("conv_plan_cases", os.path.join(REPO, "tools", "conv_plan_cases.py"))
cpc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cpc)

ROWS = [r for r in json.load(open(cpc.TABLE))["cases"] if r.get("fmt", cpc.F16X2) & cpc.F16X2]
CASES = [cpc.case(**{k: v for k, v in r.items() if k not in ("expect", "launch")}) for r in ROWS]
# rows the table may lack: a plain and a masked stride-1 data gradient and a statistics epilogue that the role-split route takes, forced
# from one tile up (the route's default thresholds are sized for batch 32)
FORCED = (("set_tapx", [1, 1, 8]),)
EXTRA = [cpc.case(name="dgrad plain 64 -> 64", n=8, hw=(32, 32), cin=64, cout=64, k=3, transposed=1, act=0, scale=0, shift=0, knobs=FORCED),
         cpc.case(name="dgrad plain + res 128 -> 128", n=8, hw=(32, 32), cin=128, cout=128, k=3, transposed=1, act=0, scale=0, shift=0, res=1, knobs=FORCED),
         cpc.case(name="dgrad masked 64 -> 64", n=8, hw=(32, 32), cin=64, cout=64, k=3, transposed=1, mask=1, knobs=FORCED),
         cpc.case(name="stats 64 -> 128 s2", n=8, hw=(16, 16), cin=64, cout=128, k=3, stride=2, scale=0, shift=0, bn=1 << 20, knobs=FORCED)]
FIELDS = [n for n, _ in hip.ConvPlan._fields_]
TRAIN = hip.W_F16X1 | hip.W_F16X1T


def plan_of(c, bits):
    cpc.reset_knobs(hip)
    try:
        cpc.set_knobs(hip, c["knobs"])
        d, p, ws_n, aux = cpc.build_call(hip, c)
        d.w_format |= bits
        rc, pl = hip.conv_plan(d, p["x"], p["w"], p["y"], scale=p["scale"], shift=p["shift"], res=p["res"], rowscale=p["rowscale"],
                               rowmask=p["rowmask"], mask=p["mask"], workspace=p["workspace"], workspace_floats=ws_n, aux=aux)
        return rc, {f: getattr(pl, f) for f in FIELDS}
    finally:
        cpc.reset_knobs(hip)


def test_the_training_bit_moves_every_role_split_plan_to_one_product_and_nothing_else():
    assert (hip.W_F16X2, hip.W_F16X1, hip.W_F16X1T) == (4, 8, 16)
    rest = lambda p: {f: v for f, v in p.items() if f not in ("planes", "variant")}
    kinds = {"stats": 0, "masked": 0, "transposed": 0, "forward": 0, "other": 0}
    variants = set()
    for c in CASES + EXTRA:
        rc0, p0 = plan_of(c, 0)
        rc1, p1 = plan_of(c, hip.W_F16X1)
        rct, pt = plan_of(c, TRAIN)
        assert rct == rc0 == rc1, c["name"]
        if rc0 != 0:
            kinds["other"] += 1
            continue
        if p0["route"] != hip.ROUTE_TAPX:
            assert pt == p0, (c["name"], p0, pt)
            kinds["other"] += 1
        elif c["mask"] or c["bn"] or c["transposed"]:
            assert p1 == p0, c["name"]          # (EGR_W_F16X1 alone: the plan it has today)
            assert p0["planes"] == 2 and pt["planes"] == 1 and pt["variant"] == p0["variant"] + 1000, (c["name"], p0, pt)
            assert rest(pt) == rest(p0), (c["name"], p0, pt)
            tr = p0["variant"] // 100
            assert tr == (1 if c["bn"] else (2 if c["mask"] else 0)), c["name"]
            kinds["stats" if c["bn"] else ("masked" if c["mask"] else "transposed")] += 1
            variants.add(pt["variant"])
        else:
            assert pt == p1 and p1["planes"] == 1 and p1["variant"] == p0["variant"] + 1000 and rest(p1) == rest(p0), c["name"]
            kinds["forward"] += 1
    assert all(kinds.values()), kinds
    assert any(1100 <= v < 1200 for v in variants) and any(1200 <= v for v in variants) and any(v < 1100 for v in variants), variants


def test_the_training_bit_needs_both_other_bits():
    c = next(c for c in CASES if c["name"] == "fwd b64 h2 G2 M524288 N64 K576 k3s1 cin64")
    d, p, ws_n, aux = cpc.build_call(hip, c)
    for fmt, want in ((4 | 16, hip.EINVAL), (16, hip.EINVAL), (1 | 16, hip.EINVAL), (8 | 16, hip.EINVAL), (4 | 8 | 16, 0), (4 | 8, 0), (4, 0)):
        d.w_format = fmt
        rc, _ = hip.conv_plan(d, p["x"], p["w"], p["y"], scale=p["scale"], shift=p["shift"], workspace=p["workspace"], workspace_floats=ws_n, aux=aux)
        assert rc == want, (fmt, rc)


def test_the_weight_gradient_entry_checks_the_one_product_bit_before_any_device_call():
    d = hip.ConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.kh, d.kw, d.stride, d.pad, d.ho, d.wo = 8, 32, 32, 64, 64, 3, 3, 1, 1, 32, 32
    d.ldx = d.ldy = 64
    d.xmap = d.ymap = hip.NMap(8, 32 * 32 * 64, 0)
    d.rmap = hip.NMap(1, 0, 0)
    d.groups = 1
    fake = [cpc.BASE * (i + 1) for i in range(6)]          # x, dy, dw, workspace, two records: none is dereferenced on the host
    call = lambda fmt, rx, ry: (setattr(d, "w_format", fmt),
                                hip.lib.egr_conv2d_wgrad_ex_f32(C.byref(d), fake[0], fake[1], fake[2], None, fake[3], 1 << 24, 0, rx, ry, None))[1]
    assert call(1 | 4 | 8, None, None) == hip.ENULL
    assert call(1 | 2 | 4 | 8, None, None) == hip.ENULL
    assert call(1 | 8, None, None) == hip.EINVAL
    assert call(1 | 8, fake[4], fake[5]) == hip.EINVAL
    assert call(1 | 2 | 8, fake[4], fake[5]) == hip.EINVAL
    assert hip.lib.egr_wgrad_last_planes() in (0, 1, 2, 3)


def test_fast_training_policy_object():
    default = hip.LaunchPolicy()
    assert default.train_one_product is False and hip.LaunchPolicy.fast().train_one_product is False
    assert default.exact().train_one_product is False
    ft = hip.LaunchPolicy.fast_training()
    assert ft == default.fast().replace(train_one_product=True) and ft.train_one_product is True and ft.w_format == "f16"
    assert default.replace(chain=False).fast_training().chain is False            # on an object: its own fields
    assert ft.pack_key() != hip.LaunchPolicy.fast().pack_key() != default.pack_key()
    assert hip.LaunchPolicy.from_env({"EGR_W_FORMAT": "f16", "EGR_TRAIN_FORMAT": "f16"}) == ft
    assert hip.LaunchPolicy.from_env({"EGR_W_FORMAT": "f16"}) == hip.LaunchPolicy.fast()
    for env in ({"EGR_TRAIN_FORMAT": "f16"}, {"EGR_W_FORMAT": "f16x2", "EGR_TRAIN_FORMAT": "f16"}, {"EGR_W_FORMAT": "bf16x3", "EGR_TRAIN_FORMAT": "f16"}):
        with pytest.raises(ValueError):
            hip.LaunchPolicy.from_env(env)
    assert hip.LaunchPolicy.from_env({}) == default

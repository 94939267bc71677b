"""The opt-in fast policy on the host: what the conv dispatch plans when EGR_W_F16X1 rides on EGR_W_F16X2, and the
LaunchPolicy that selects it.  No device is touched: egr_conv_plan with the fake aligned pointers of tests/test_conv_plan.py, over
the fp16-scheme rows of its table (tests/golden/conv_plan_cases.json).

A forward row on the role-split route keeps route, tile, grid and walk and names the one-product form (planes 1, variant + 1000);
every other row - another route, a refusal, a training epilogue, a data gradient - gets exactly the plan it gets without the bit."""
import importlib.util
import json
import os

from egorear_amd import hip

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("conv_plan_cases", os.path.join(REPO, "tools", "conv_plan_cases.py"))
cpc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cpc)

ROWS = [r for r in json.load(open(cpc.TABLE))["cases"] if r.get("fmt", cpc.F16X2) & cpc.F16X2]       # (a row holds what differs from case()'s defaults)
CASES = [cpc.case(**{k: v for k, v in r.items() if k not in ("expect", "launch")}) for r in ROWS]
FIELDS = [n for n, _ in hip.ConvPlan._fields_]


def plan_of(c, bit):
    cpc.reset_knobs(hip)
    try:
        cpc.set_knobs(hip, c["knobs"])
        d, p, ws_n, aux = cpc.build_call(hip, c)
        d.w_format |= bit
        rc, pl = hip.conv_plan(d, p["x"], p["w"], p["y"], scale=p["scale"], shift=p["shift"], res=p["res"], rowscale=p["rowscale"],
                               rowmask=p["rowmask"], mask=p["mask"], workspace=p["workspace"], workspace_floats=ws_n, aux=aux)
        return rc, {f: getattr(pl, f) for f in FIELDS}
    finally:
        cpc.reset_knobs(hip)


def test_the_bit_moves_forward_role_split_plans_to_one_product_and_nothing_else():
    assert hip.W_F16X1 == 8 and hip.W_F16X2 == 4
    fast_rows = same_rows = 0
    for c in CASES:
        rc0, p0 = plan_of(c, 0)
        rc1, p1 = plan_of(c, hip.W_F16X1)
        assert rc1 == rc0, c["name"]
        if rc0 != 0:
            same_rows += 1
            continue
        forward = not c["mask"] and not c["bn"] and not c["transposed"]
        if p0["route"] == hip.ROUTE_TAPX and forward:
            assert p0["planes"] == 2 and p1["planes"] == 1 and p1["variant"] == p0["variant"] + 1000 and p0["variant"] < 100, c["name"]
            assert {f: v for f, v in p1.items() if f not in ("planes", "variant")} == {f: v for f, v in p0.items() if f not in ("planes", "variant")}, c["name"]
            fast_rows += 1
        else:
            assert p1 == p0, (c["name"], p0, p1)
            same_rows += 1
    assert fast_rows >= 1 and same_rows >= 1, (fast_rows, same_rows)
    # rows of each kind that must not move: a training epilogue and a data gradient on the role-split route, and another route
    kinds = {"train": 0, "transposed": 0, "other": 0}
    for c in CASES:
        rc0, p0 = plan_of(c, 0)
        if rc0 == 0 and p0["route"] == hip.ROUTE_TAPX and (c["mask"] or c["bn"]):
            kinds["train"] += 1
        elif rc0 == 0 and p0["route"] == hip.ROUTE_TAPX and c["transposed"]:
            kinds["transposed"] += 1
        elif rc0 == 0 and p0["route"] != hip.ROUTE_TAPX:
            kinds["other"] += 1
    assert kinds["train"] and kinds["other"], kinds


def test_the_bit_goes_with_the_fp16_scheme_only():
    c = next(c for c in CASES if c["name"] == "fwd b64 h2 G2 M524288 N64 K576 k3s1 cin64")
    d, p, ws_n, aux = cpc.build_call(hip, c)
    for fmt, want in ((hip.W_F16X1, hip.EINVAL), (hip.W_F16X1 | 1, hip.EINVAL), (hip.W_F16X1 | hip.W_F16X2, 0), (hip.W_F16X2, 0)):
        d.w_format = fmt
        rc, _ = hip.conv_plan(d, p["x"], p["w"], p["y"], scale=p["scale"], shift=p["shift"], workspace=p["workspace"], workspace_floats=ws_n, aux=aux)
        assert rc == want, (fmt, rc)


def test_fast_policy_object():
    default = hip.LaunchPolicy()
    f = hip.LaunchPolicy.fast()
    assert f == default.fast() and default.replace(chain=False).fast().chain is False      # on the class: the default policy's; on an object: its own
    assert f.w_format == "f16" and f.h2 is True and f.layer_h2 is True and f.fp16_scheme
    assert f.pack_key() != default.pack_key()
    assert hip.LaunchPolicy.from_env({"EGR_W_FORMAT": "f16"}) == hip.LaunchPolicy().fast()
    assert hip.LaunchPolicy().fast().replace(w_format="f16x2") == default            # nothing but the format differs
    # the default is what it was
    assert (default.w_format, default.h2, default.layer_h2, default.x6_min_rows, default.x6_min_flops, default.chain, default.wgrad_x6) == \
        ("f16x2", True, True, 4096, 5e8, True, True)
    assert hip.LaunchPolicy.from_env({}) == default and default.fp16_scheme and not default.exact().fp16_scheme
    assert hip.LaunchPolicy.from_env({"EGR_W_FORMAT": "bf16x3"}).h2 is False

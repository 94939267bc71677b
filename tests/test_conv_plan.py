"""The conv dispatch, checked on the CPU: egr_conv_plan says what egr_conv2d_nhwc[_ex]_f32 / egr_conv2d_masked[_ex]_f32 would launch - route,
tile, variant, grid, split-K - without touching a device (fake aligned pointers, as tests/test_hip_binding.py).

The table tests/golden/conv_plan_cases.json holds the inputs and, as `expect` and `launch`, the route or refusal code and the launch
(kernel, grid, split-K, ...) the commit named in its `recorded_from` made for them - tools/conv_plan_cases.py records them through
the launch entry points with the HIP launch calls replaced.  The plan, and the launches of this checkout, must reproduce every row.
"""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

from egorear_amd import hip

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("conv_plan_cases", os.path.join(REPO, "tools", "conv_plan_cases.py"))
cpc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cpc)

_env = [v for v in os.environ if v.startswith(("EGR_CONV_", "EGR_SPLITK_"))]
assert not _env, f"unset {_env}: the table holds the decisions under the default knobs, and these tests leave the knobs at their defaults"
TABLE = json.load(open(cpc.TABLE))
EXPECT = [r["expect"] for r in TABLE["cases"]]           # >= 0: route, < 0: EGR_E* code
CASES = [cpc.case(**{k: v for k, v in r.items() if k not in ("expect", "launch")}) for r in TABLE["cases"]]
FIELDS = [n for n, _ in hip.ConvPlan._fields_]


def plan_of(c):
    cpc.reset_knobs(hip)
    try:
        cpc.set_knobs(hip, c["knobs"])
        d, p, ws_n, aux = cpc.build_call(hip, c)
        rc, pl = hip.conv_plan(d, p["x"], p["w"], p["y"], scale=p["scale"], shift=p["shift"], res=p["res"], rowscale=p["rowscale"],
                               rowmask=p["rowmask"], mask=p["mask"], workspace=p["workspace"], workspace_floats=ws_n, aux=aux)
        if aux is not None and hasattr(aux, "_tiles"):
            assert aux._tiles.value == -1, "egr_conv_plan wrote through bn_tiles_out"
        return rc, {f: getattr(pl, f) for f in FIELDS}
    finally:
        cpc.reset_knobs(hip)


@pytest.fixture(scope="module")
def plans():
    return [plan_of(c) for c in CASES]


def test_table_is_recorded_from_one_commit():
    assert len(TABLE["recorded_from"]) == 40, "recorded from a clean checkout of one commit"
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)


def test_route_table_against_the_parent(plans):
    wrong = []
    for c, want, (rc, pl) in zip(CASES, EXPECT, plans):
        got = rc if rc != 0 else pl["route"]
        if got != want:
            wrong.append((c["name"], want, got))
    assert not wrong, f"{len(wrong)} of {len(CASES)} rows: {wrong[:10]}"
    assert set(EXPECT) == set(range(7)) | {hip.EINVAL, hip.ENULL, hip.EWORKSPACE}


def test_plan_says_what_the_parent_launched(plans):
    """Tile, grid, workgroup size, split-K and the kind of reduction of every row, against what the parent's entry points launched."""
    wrong = []
    for c, r, (rc, pl) in zip(CASES, TABLE["cases"], plans):
        if rc != 0:
            continue
        kernel, gx, gy, gz, block, tm, tn, split, kps, red = r["launch"]
        got = [pl["grid_x"], pl["grid_y"], pl["grid_z"], pl["block"], pl["tiles_m"] if tm is not None else None, pl["tiles_n"] if tn is not None else None,
               pl["split_k"] if split is not None else None, pl["ktiles_per_split"] if kps is not None else None, 2 * pl["fused_reduce"] + pl["reduce_pass"]]
        if kernel.startswith("conv_igemm"):         # <BM, BN, ...>
            got += [pl["bm"], pl["bn"]]
            r = r["launch"][1:] + [int(v) for v in kernel.split("<")[1].split(",")[:2]]
        else:
            r = r["launch"][1:]
        if ("x6p_kernel" in kernel) != bool(pl["persistent"] and pl["route"] == hip.ROUTE_SPLIT_TILED) or got != r:
            wrong.append((c["name"], kernel, r, got))
    assert not wrong, f"{len(wrong)} rows: {wrong[:5]}"


def test_launches_equal_the_parents_and_reach_every_kernel(tmp_path):
    """The recorder on THIS checkout - the launch entry points themselves, the launch calls taken by tools/conv_launch_shim.hip - gives the
    table again: same kernel (name with template arguments), grid, workgroup size and plan-dependent kernel arguments for every row,
    same set of kernels in the library, and no kernel that no row launches (dead code, or a missing row)."""
    out = tmp_path / "table.json"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "conv_plan_cases.py"), "--record", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    mine = json.load(open(out))
    assert mine["kernels"] == TABLE["kernels"]
    diff = [(a["name"], a.get("launch"), b.get("launch")) for a, b in zip(TABLE["cases"], mine["cases"]) if a != b]
    assert not diff and len(mine["cases"]) == len(TABLE["cases"]), diff[:5]
    launched = {c["launch"][0] for c in TABLE["cases"] if "launch" in c}
    assert any(c["launch"][-1] == 1 for c in TABLE["cases"] if "launch" in c)           # (splitk_reduce_kernel, the second launch)
    assert launched | {"splitk_reduce_kernel"} == set(TABLE["kernels"]), sorted(set(TABLE["kernels"]) ^ launched)


def test_plan_invariants(plans):
    for c, (rc, pl) in zip(CASES, plans):
        if rc != 0:
            continue
        name = c["name"]
        d, p, ws_n, aux = cpc.build_call(hip, c)
        npad, groups = (c["cout"] + 31) // 32 * 32, c["groups"]
        M = c["n"] * c["ho"] * c["wo"] // (4 if pl["cls_mode"] else 1)
        ktiles = c["k"] * c["k"] * c["cin"] // 32
        route = pl["route"]
        # tiles cover M x Npad, exactly where the route works on whole tiles
        assert pl["tiles_m"] * pl["bm"] >= M > (pl["tiles_m"] - 1) * pl["bm"] and pl["tiles_n"] * pl["bn"] >= npad > (pl["tiles_n"] - 1) * pl["bn"], name
        if route in (hip.ROUTE_TAP, hip.ROUTE_TAP2, hip.ROUTE_TAPX):
            assert pl["tiles_m"] * pl["bm"] == M and pl["tiles_n"] * pl["bn"] == npad, name
        if route in (hip.ROUTE_STREAM_1X1, hip.ROUTE_SMALL_F32):
            assert pl["tiles_n"] * pl["bn"] == npad, name
        tiles = pl["tiles_m"] * pl["tiles_n"]
        # the grid: one workgroup per tile, or fewer walking them
        if route == hip.ROUTE_TAPX:
            blocks = dict(c["knobs"]).get("set_tapx", [1, -1, 256])[2]
            blocks = 256 if blocks <= 0 else blocks
            assert (pl["grid_y"], pl["grid_z"], pl["block"]) == (1, 1, 512) and pl["grid_x"] == min(tiles * groups, blocks), name
            assert pl["persistent"] == (tiles * groups > blocks), name
        elif route == hip.ROUTE_STREAM_1X1:
            assert (pl["grid_y"], pl["grid_z"], pl["block"]) == (pl["tiles_n"], groups, 512), name
            assert 1 <= pl["grid_x"] <= max(1, 256 // (pl["tiles_n"] * groups)) and pl["grid_x"] * 8 < pl["tiles_m"] + 8, name
            assert pl["grid_x"] * pl["grid_y"] * pl["grid_z"] <= max(256, pl["tiles_n"] * groups), name
        else:
            assert pl["grid_z"] == groups and pl["block"] == 256, name
            assert pl["grid_y"] == (4 if pl["cls_mode"] else pl["split_k"]), name
            if pl["persistent"]:
                assert route == hip.ROUTE_SPLIT_TILED and pl["grid_x"] % 8 == 0 and 8 <= pl["grid_x"] < tiles and pl["bm"] * pl["bn"] > 128 * 64, name
                assert ktiles <= dict(c["knobs"]).get("set_persist", [512, 4])[1] or dict(c["knobs"])["set_persist"][1] < 0 and ktiles <= 4, name
            else:
                assert pl["grid_x"] == tiles, name
        # split-K: tiled routes only, no empty slice, slabs fit the workspace
        assert pl["split_k"] >= 1 and pl["split_k"] * pl["ktiles_per_split"] >= ktiles > (pl["split_k"] - 1) * pl["ktiles_per_split"], name
        if pl["split_k"] > 1:
            assert route in (hip.ROUTE_F32_TILED, hip.ROUTE_SPLIT_TILED) and not pl["cls_mode"], name
            assert p["workspace"] is not None and p["workspace"] % 16 == 0 and pl["split_k"] * M * npad * groups <= ws_n, name
            assert pl["reduce_pass"] + pl["fused_reduce"] == 1 and not (pl["fused_reduce"] and pl["persistent"]), name
            assert not pl["fused_reduce"] or tiles * groups <= 2048, name
        else:
            assert pl["reduce_pass"] == 0 and pl["fused_reduce"] == 0, name
        if c["split_k"] > 1 and not pl["cls_mode"]:
            assert pl["split_k"] == -(-ktiles // -(-ktiles // min(c["split_k"], ktiles))), name
        assert pl["planes"] == {0: 0, 1: 3, 4: 2}[c["fmt"]], name
        assert pl["cls_mode"] in (0, 1) and (not pl["cls_mode"] or (c["transposed"] and c["stride"] == 2)), name
        # the statistics slabs: one per M tile, within the caller's capacity
        if c["bn"]:
            assert pl["bn_slabs"] == pl["tiles_m"] and groups * pl["tiles_m"] * 3 * c["cout"] <= c["bn"] and pl["split_k"] == 1, name
        else:
            assert pl["bn_slabs"] == 0, name


def test_plan_entry_refuses_like_the_launch_entries():
    c = next(c for c in CASES if c["name"] == "fwd b64 h2 G2 M524288 N64 K576 k3s1 cin64")
    d, p, ws_n, aux = cpc.build_call(hip, c)
    import ctypes as C
    args = [C.byref(d), p["x"], p["w"], p["scale"], p["shift"], None, None, None, None, p["y"], p["workspace"], ws_n, C.byref(aux)]
    assert hip.lib.egr_conv_plan(*args, None) == hip.ENULL
    assert hip.lib.egr_conv_plan(None, *args[1:], C.byref(hip.ConvPlan())) == hip.ENULL
    assert hip.lib.egr_conv_last_kernel() in range(7)

"""The case table of the conv dispatch (tests/golden/conv_plan_cases.json): how a row becomes a call, and the recorder of the expected column.

    python tools/conv_plan_cases.py --table IN.json --record OUT.json      # in a checkout of the commit whose decisions are to be recorded

A row holds the arguments of case() that differ from its defaults, `expect` - the route (>= 0) or the EGR_E* code (< 0) - and `launch`,
what was launched (see record()).  New rows are added to the table by hand, then recorded.

The recorder uses only entry points that exist before and after the plan / launch split: it calls egr_conv2d_nhwc_ex_f32 /
egr_conv2d_masked_ex_f32 with fake aligned pointers (none is dereferenced on the host) in a process where tools/conv_launch_shim.hip
stands in for the HIP launch calls - nothing is launched, with or without a GPU in the machine.  A refusal returns its EGR_E* code;
otherwise the route is left in egr_conv_last_kernel() and the shim holds kernel, grid and the plan-dependent kernel arguments.

tests/test_conv_plan.py reads the same table, asks egr_conv_plan instead, and runs this recorder on its own checkout.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(REPO, "tests", "golden", "conv_plan_cases.json")
F32, BF16X3, F16X2 = 0, 1, 4
NO_DEVICE = 100          # hipErrorNoDevice
BASE = 0x10000000        # fake device addresses, 16-byte aligned, 256 MiB apart
OPERANDS = ("x", "w", "y", "scale", "shift", "res", "rowscale", "rowmask", "mask", "workspace", "w_descale", "amax_in", "amax_out", "bn_partials")


def case(*, name, n, hw, cin, cout, k=1, stride=1, fmt=F16X2, groups=1, act=1, res=0, transposed=0, mask=0, scale=1, shift=1, bn=0,
         split_k=0, ws=1 << 26, out_nchw=0, rowscale=0, rowmask=0, amax_out=1, ldy=None, ldr=None, misalign=None, null=None, knobs=(), in_hw=None):
    """A table row in full.  hw: output size (ho, wo); the input size follows from stride (forward: ho * stride, transposed: ho / stride) unless
    in_hw says otherwise.  bn: capacity of the statistics buffer in doubles (0: no statistics epilogue).  ws: workspace floats (0: NULL).
    misalign: {operand: byte offset}; null: operands passed as NULL although the call needs them."""
    ho, wo = hw
    knobs = [(kn, list(args)) for kn, args in knobs]
    pad = k // 2
    if in_hw is None:
        in_hw = (ho // stride, wo // stride) if transposed else (ho * stride, wo * stride)
    if mask:
        scale = shift = 0
        act = 0
    if bn:
        act = 0
    return {"name": name, "n": n, "h": in_hw[0], "w": in_hw[1], "ho": ho, "wo": wo, "cin": cin, "cout": cout, "k": k, "stride": stride, "pad": pad,
            "fmt": fmt, "groups": groups, "act": act, "res": res, "transposed": transposed, "mask": mask, "scale": scale, "shift": shift,
            "bn": bn, "split_k": split_k, "ws": ws, "out_nchw": out_nchw, "rowscale": rowscale, "rowmask": rowmask, "amax_out": amax_out,
            "ldy": ldy, "ldr": ldr, "misalign": misalign or {}, "null": list(null or ()), "knobs": [list(kn) for kn in knobs]}


def build_call(hip, c):
    """(ConvDesc, {operand: address or None}, workspace_floats, ConvAux or None) of a table row: dense NHWC tensors, the images of all
    groups back to back."""
    d = hip.ConvDesc()
    n, h, w, ho, wo, cin, cout, k, g = c["n"], c["h"], c["w"], c["ho"], c["wo"], c["cin"], c["cout"], c["k"], c["groups"]
    npad, K = (cout + 31) // 32 * 32, k * k * cin
    d.n, d.h, d.w, d.cin, d.cout, d.kh, d.kw, d.stride, d.pad, d.ho, d.wo = n, h, w, cin, cout, k, k, c["stride"], c["pad"], ho, wo
    ldy = c["ldy"] or cout
    ldr = c["ldr"] or cout
    d.ldx, d.ldy, d.ldr = cin, (0 if c["out_nchw"] else ldy), ldr
    d.xmap = hip.NMap(n, h * w * cin, 0)
    d.ymap = hip.NMap(n, cout * ho * wo if c["out_nchw"] else ho * wo * ldy, 0)
    rh, rw = (ho // 2, wo // 2) if c["res"] == 3 else (ho, wo)
    d.rmap = hip.NMap(n, rh * rw * ldr, 0) if c["res"] else hip.NMap(1, 0, 0)
    d.act, d.res_mode, d.out_nchw, d.split_k, d.transposed, d.w_format = c["act"], c["res"], c["out_nchw"], c["split_k"], c["transposed"], c["fmt"]
    d.groups = g
    if g > 1:
        cfp = (npad // 32 + 3) // 4 * 4
        d.gx, d.gy, d.gr, d.gp = n * h * w * cin, n * ho * wo * ldy, n * rh * rw * ldr, npad
        d.gw = {F32: npad * K, BF16X3: cfp * (K // 32) * 3072, F16X2: cfp * (K // 32) * 2048}[c["fmt"]]
        d.grs = d.grm = n * ho * wo
    h2 = c["fmt"] == F16X2
    present = {"x": 1, "w": 1, "y": 1, "scale": c["scale"], "shift": c["shift"], "res": c["res"], "rowscale": c["rowscale"],
               "rowmask": c["rowmask"], "mask": c["mask"], "workspace": c["ws"] > 0, "w_descale": h2, "amax_in": h2,
               "amax_out": c["amax_out"] and not c["out_nchw"], "bn_partials": c["bn"] > 0}
    p = {nm: (BASE * (i + 1) + c["misalign"].get(nm, 0) if present[nm] and nm not in c["null"] else None) for i, nm in enumerate(OPERANDS)}
    aux = None
    if h2 or p["amax_out"] or c["bn"]:
        aux = hip.ConvAux(p["w_descale"], p["amax_in"], p["amax_out"], p["bn_partials"], None, c["bn"])
        if c["bn"] and "bn_tiles_out" not in c["null"]:
            aux._tiles = C.c_int32(-1)           # (host memory: the launch entry points write the slab count here)
            aux.bn_tiles_out = C.addressof(aux._tiles)
    return d, p, c["ws"], aux


KNOBS = {"set_tap": "egr_conv_set_tap", "set_tapx": "egr_conv_set_tapx", "force_config": "egr_conv_force_config",
         "set_persist": "egr_conv_set_persist", "set_splitk_fused": "egr_conv_set_splitk_fused"}


def set_knobs(hip, knobs):
    for name, args in knobs:
        assert getattr(hip.lib, KNOBS[name])(*args) == 0, (name, args)


def reset_knobs(hip):
    """The defaults of a process started without EGR_CONV_* / EGR_SPLITK_* in its environment."""
    set_knobs(hip, [("set_tap", [1]), ("set_tapx", [1, 256, 256]), ("force_config", [-1]), ("set_persist", [512, 4]), ("set_splitk_fused", [0])])


class ShimRec(C.Structure):
    _fields_ = [("stub", C.c_uint64), ("grid", C.c_uint32 * 3), ("block", C.c_uint32 * 3)] + \
               [(n, C.c_int32) for n in ("split_k", "ktiles_per_split", "tiles_m", "tiles_n", "has_cnt")]


def load_shim(build_dir):
    """Compiles tools/conv_launch_shim.hip against THIS checkout's ConvArgs and loads it ahead of the library: from here on no conv
    launch of this process reaches a device.  Returns (shim, {stub offset: kernel name})."""
    sys.path.insert(0, REPO)
    from egorear_amd.csrc import build as B
    so = os.path.join(build_dir, "conv_launch_shim.so")
    subprocess.run([B._hipcc()] + B.FLAGS + ["-shared", "--cuda-host-only", os.path.join(REPO, "tools", "conv_launch_shim.hip"), "-o", so], check=True)
    shim = C.CDLL(so, mode=C.RTLD_GLOBAL)
    names = {}
    for line in subprocess.run(["nm", "-C", B.LIB], capture_output=True, text=True, check=True).stdout.splitlines():
        addr, kind, name = line.split(" ", 2)
        if kind in "dD" and name.endswith("(egrc::ConvArgs)"):          # the kernels' host-side handles
            names[int(addr, 16)] = name[:-len("(egrc::ConvArgs)")].replace("void ", "").replace("(anonymous namespace)::", "").replace(" ", "")
    return shim, names


def record(hip, shim, names, rows):
    """`names`: every kernel of the library that takes ConvArgs (the table's `kernels`).  Per row (expect, launch): the EGR_E* code (< 0) of a refusal and None, else the route (>= 0) the call took and what it launched -
    [kernel, grid x, y, z, workgroup size, M tiles, N tiles, split_k, ktiles_per_split, reduction: 0 none / 1 second launch / 2 fused].
    Fields the launch leaves unset are null: the tile counts of the streaming route, the split of the streaming and the small one."""
    out = []
    recs = (ShimRec * 8)()
    for row in rows:
        c = case(**row)
        reset_knobs(hip)
        set_knobs(hip, c["knobs"])
        d, p, ws_n, aux = build_call(hip, c)
        a = C.byref(aux) if aux is not None else None
        if c["mask"]:
            rc = hip.lib.egr_conv2d_masked_ex_f32(C.byref(d), p["x"], p["w"], p["res"], p["mask"], p["y"], p["workspace"], ws_n, a, None)
        else:
            rc = hip.lib.egr_conv2d_nhwc_ex_f32(C.byref(d), p["x"], p["w"], p["scale"], p["shift"], p["res"], p["rowscale"], p["rowmask"], p["y"],
                                                p["workspace"], ws_n, a, None)
        n = shim.shim_take(recs)
        assert rc <= 0 and n == (0 if rc else n) and (rc < 0 or 1 <= n <= 2), (c["name"], rc, n)
        if rc < 0:
            out.append((rc, None))
            continue
        route, r = hip.lib.egr_conv_last_kernel(), recs[0]
        assert list(r.block)[1:] == [1, 1] and (n == 1 or names[recs[1].stub] == "splitk_reduce_kernel"), c["name"]
        split = [None, None] if route in (4, 5) else [r.split_k, r.ktiles_per_split]
        out.append((route, [names[r.stub]] + list(r.grid) + [r.block[0]] +
                    ([None, None] if route == 4 else [r.tiles_m, r.tiles_n]) + split + [2 if r.has_cnt else n - 1]))
    reset_knobs(hip)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--table", metavar="IN.json", default=TABLE, help="the table whose rows are run (default: the committed one)")
    ap.add_argument("--record", metavar="OUT.json", required=True, help="where to write the table with the expected columns of THIS checkout's library")
    ap.add_argument("--build-dir", default=None, help="where the shim is built (default: next to OUT.json)")
    args = ap.parse_args()
    rows = [{k: v for k, v in r.items() if k not in ("expect", "launch")} for r in json.load(open(args.table))["cases"]]
    env = [v for v in os.environ if v.startswith(("EGR_CONV_", "EGR_SPLITK_"))]
    assert not env, f"unset {env}: the table is recorded from the default knobs"
    shim, names = load_shim(args.build_dir or os.path.dirname(os.path.abspath(args.record)))
    from egorear_amd import hip
    shim.shim_take.argtypes = [C.POINTER(ShimRec)]
    got = record(hip, shim, names, rows)
    head = subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    dirty = subprocess.run(["git", "-C", REPO, "status", "--porcelain", "--untracked-files=no"], capture_output=True, text=True).stdout.strip()
    with open(args.record, "w") as f:
        f.write('{"recorded_from": "%s%s",\n "kernels": %s,\n "cases": [\n' % (head, " (modified)" if dirty else "", json.dumps(sorted(names.values()))))
        f.write(",\n".join("  " + json.dumps(dict(c, expect=e, **({"launch": l} if l else {})), separators=(",", ":")) for c, (e, l) in zip(rows, got)))
        f.write("\n ]}\n")
    print(f"{len(rows)} rows -> {args.record}")


if __name__ == "__main__":
    main()

"""Error of the two model-free 3-D decoders against known points -> profiles/volume_accuracy.json (the table of DESIGN.md 5o).

    python tools/volume_accuracy.py [--frames 10] [--device] [--out profiles/volume_accuracy.json]

The bumps of the triangulation's bump_maps fixture (tests/test_gpu_triangulate.py: sigma 1 on 64 x 64 maps at the syn rig's projections
of random points, seed 77, 15 joints a frame; the first two frames are that test's), decoded by `decode_joints_3d` (soft-argmax at
beta 100, triangulation) and by the volumetric chain around its pose (40 cm cube, beta 100, grid 16 and 32), with four views and with
the two front cameras.  Without --device the float64 statements of tests/fisheye_statement.py and tests/volume_statement.py are evaluated
on the CPU (imported, not restated here); with --device the kernels run (decode.decode_joints_3d_volumetric).  Errors are Euclidean, in cm:
mean, 95th percentile, maximum."""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

BETA, THR, CUBE, GRIDS, HM = 100.0, 0.5, 40.0, (16, 32), 64


def stats(err):
    import torch
    return {"mean": round(float(err.mean()), 3), "p95": round(float(torch.quantile(err, 0.95)), 3), "max": round(float(err.max()), 3),
            "n": int(err.numel())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "volume_accuracy.json"))
    a = ap.parse_args()
    import torch
    import fisheye_statement as FS
    import volume_statement as VS
    g = torch.Generator().manual_seed(77)
    cams = FS.rig()
    B, J = a.frames, 15
    pts = FS.random_points(B, J, g)
    res = {"frames": B, "joints": J, "maps": [HM, HM], "cube_cm": CUBE, "beta": BETA, "threshold": THR,
           "arithmetic": "kernels on the device" if a.device else "float64 statements on the CPU", "rows": {}}
    if a.device:
        if not torch.cuda.is_available():
            raise SystemExit("volume_accuracy --device: needs the GPU")
        from egorear_amd import decode
    for V in (4, 2):
        rec = FS.records(cams[:V])
        hm = FS.bumps(pts, rec, None, HM, HM).float().contiguous()
        rows = {}
        if a.device:
            for G in GRIDS:
                vol, tri, _ = decode.decode_joints_3d_volumetric(hm.to("cuda:0"), cams[:V], None, G, CUBE, BETA, BETA, THR)
                torch.cuda.synchronize()
                assert bool(vol.valid.all())
                rows["decode_joints_3d"] = stats((tri.pose.double().cpu() - pts).norm(dim=-1).view(-1))
                rows[f"volumetric grid {G}"] = stats((vol.pose.double().cpu() - pts).norm(dim=-1).view(-1))
        else:
            c64, m64 = FS.soft_argmax_statement(hm.double(), BETA)
            p3, _, _, ok3 = FS.statement(c64, m64, rec, None, 1.0 / HM, 1.0 / HM)
            assert bool(ok3.all())
            rows["decode_joints_3d"] = stats((p3 - pts).norm(dim=-1).view(-1))
            for G in GRIDS:
                pose = torch.cat([VS.statement(hm[b:b + 1].double(), m64[b:b + 1], p3[b:b + 1], rec, None, G, CUBE, BETA, THR)["pose"]
                                  for b in range(B)])               # (a frame at a time: the float64 temporaries of grid 32 are large)
                rows[f"volumetric grid {G}"] = stats((pose - pts).norm(dim=-1).view(-1))
        res["rows"][f"{V} views"] = rows
        for name, s in rows.items():
            print(f"| {V} views | {name} | {res['arithmetic']} | {s['mean']:.2f} | {s['p95']:.2f} | {s['max']:.2f} |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

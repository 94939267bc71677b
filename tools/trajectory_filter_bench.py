"""Time the causal fixed-lag trajectory filter -> profiles/trajectory_filter.json.

    python tools/trajectory_filter_bench.py [--inputs 4] [--rounds 30] [--out profiles/trajectory_filter.json]

One process, J = 15, streams of random walks with 30 % of the frames dropped (tools/trajectory_bench.py's), every state warmed by 64
frames first so that the ring is full:
  - egr_trajectory_filter_f32, one frame a call (C = 1), at lag 0 / 4 / 8 / 16, gate off and at 2 cm, for N = 1 and N = 64 streams;
  - one call of C = 8 frames, and egr_trajectory_filter_tail_f32, at lag 8;
  - decode.decode_stream_3d (three launches) on (64, 4, 15, 64, 64) maps next to decode.decode_joints_3d (two);
  - what a user has without the filter: egr_trajectory_smooth_f32 run again on the window of the last T = 64 frames, in the same run.
The method is tools/trajectory_bench.py's: each launch rotates over `inputs` distinct inputs, one rotation is captured into a hipGraph
so that the kernels run back to back without the host's enqueue time between them, the graphs are replayed in turn `rounds` times, each
replay between two device events; median and minimum.  A replay feeds `inputs` more frames into the states, as a stream does.  There is
no target: the numbers and the ratio to the window re-solve are reported as measured."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

J = 15
STREAMS = (1, 64)
LAGS = (0, 4, 8, 16)
ACCEL, VEL, GATE, MAX_GAP, WINDOW = 10.0, 0.0, 2.0, 8, 64
BETA, THR, MIN_DET = 100.0, 0.5, 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trajectory_filter.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("trajectory_filter_bench: needs the GPU (nothing is measured without one)")
    import fisheye_statement as FS
    import trajectory_bench as TB
    from egorear_amd import decode, hip
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    cams = FS.rig()

    launches = {}
    for N in STREAMS:
        clips = [tuple(t.to(dev) for t in TB.random_clip(N, WINDOW, gen, torch)) for _ in range(a.inputs)]
        frames = [(p[:, -1:].contiguous(), w[:, -1:].contiguous()) for p, w in clips]
        chunks = [(p[:, -8:].contiguous(), w[:, -8:].contiguous()) for p, w in clips]

        def warmed(lag, gate, N=N, clips=clips):
            state = hip.trajectory_filter_state(N, J, lag, dev)
            hip.trajectory_filter(state, clips[0][0], clips[0][1], None, None, lag, VEL, ACCEL, gate, MAX_GAP)
            return state

        for lag in LAGS:
            for gate in (0.0, GATE):
                state = warmed(lag, gate)
                launches[f"egr_trajectory_filter_f32 C 1, lag {lag}, gate {gate:g} (N {N})"] = (
                    lambda i, s=state, f=frames, lag=lag, gate=gate: hip.trajectory_filter(s, f[i][0], f[i][1], None, None, lag, VEL, ACCEL, gate,
                                                                                          MAX_GAP))
        state = warmed(8, GATE)
        launches[f"egr_trajectory_filter_f32 C 8, lag 8, gate {GATE:g} (N {N})"] = (
            lambda i, s=state, c=chunks: hip.trajectory_filter(s, c[i][0], c[i][1], None, None, 8, VEL, ACCEL, GATE, MAX_GAP))
        tails = [warmed(8, GATE) for _ in range(a.inputs)]
        launches[f"egr_trajectory_filter_tail_f32 lag 8 (N {N})"] = (
            lambda i, t=tails, N=N: hip.trajectory_filter_tail(t[i], N, J, 8, VEL, ACCEL, MAX_GAP))
        launches[f"egr_trajectory_smooth_f32 plain, window T {WINDOW} (N {N})"] = (
            lambda i, d=clips: hip.trajectory_smooth(d[i][0], d[i][1], None, VEL, ACCEL, 0.0, 0, MAX_GAP))
    truth, maps, _, _ = TB.rendered_clip(64, list(decode.HEATMAP_PARENTS_15), FS.records(cams), gen, torch, FS)
    maps = maps.contiguous().to(dev)                                                   # (64, 4, 15, 64, 64): 64 streams, one frame each
    chain_maps = [maps] + [(maps + 0.01 * torch.randn(maps.shape, generator=gen).to(dev)).contiguous() for _ in range(a.inputs - 1)]
    stream = decode.new_track_filter(64, J, 8, dev, ACCEL, VEL, GATE, MAX_GAP)
    for _ in range(16):
        decode.decode_stream_3d(stream, chain_maps[0], cams, None, BETA, THR, MIN_DET)
    launches[f"decode_stream_3d (64 streams, lag 8, gate {GATE:g})"] = lambda i: decode.decode_stream_3d(stream, chain_maps[i], cams, None, BETA, THR, MIN_DET)
    launches["decode_joints_3d (64 frames)"] = lambda i: decode.decode_joints_3d(chain_maps[i], cams, None, BETA, THR, MIN_DET)

    times = TB.graph_times(launches, a.inputs, a.rounds, torch)
    res = {"joints": J, "accel_weight": ACCEL, "vel_weight": VEL, "gate_cm": GATE, "max_gap": MAX_GAP, "window": WINDOW, "dropped_frames": 0.3,
           "chain_maps": [64, 4, J, FS.HM, FS.HM], "inputs": a.inputs, "rounds": a.rounds, "device": hip.device_arch(), "library": hip.version(),
           "method": "one rotation over the inputs per hipGraph, graphs replayed in turn, device events around each replay; every replay feeds "
                     "`inputs` more frames into a state warmed by 64", "launches": {}}
    for name in launches:
        med, mn = statistics.median(times[name]), min(times[name])
        res["launches"][name] = {"median_us": round(med, 2), "min_us": round(mn, 2)}
        print(f"{name:64s} median {med:9.2f} us  min {mn:9.2f} us")
    L = res["launches"]
    res["window_resolve_over_filter_step"] = {
        f"lag {lag}, gate {gate:g} (N {N})": round(L[f"egr_trajectory_smooth_f32 plain, window T {WINDOW} (N {N})"]["median_us"] /
                                                    L[f"egr_trajectory_filter_f32 C 1, lag {lag}, gate {gate:g} (N {N})"]["median_us"], 2)
        for N in STREAMS for lag in LAGS for gate in (0.0, GATE)}
    res["stream_chain_over_decode_3d"] = round(L[f"decode_stream_3d (64 streams, lag 8, gate {GATE:g})"]["median_us"] /
                                               L["decode_joints_3d (64 frames)"]["median_us"], 3)
    print("window re-solve / filter step:", res["window_resolve_over_filter_step"])
    print("stream chain / per-frame decode:", res["stream_chain_over_decode_3d"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""The causal fixed-lag trajectory filter on the GPU (egr_trajectory_filter_f32, egr_trajectory_filter_tail_f32, egorear_amd/decode.py,
DESIGN.md 5w) against the float64 statement of tests/filter_statement.py: dense prefix solves of tests/trajectory_statement.py.

Yardstick: fisheye_statement's - a HIP output may deviate from the float64 statement (on the same fp32 operands) by at most MARGIN = 8 x
the deviation of the float32 evaluation of that statement, with a floor of 4 ulp (fp32) of the output's largest magnitude.  Where the
float32 evaluation does not factor or is not finite the floor alone holds; the kernel eliminates in fp64 and can meet it.  With the
gate on, a weight is a discontinuous function of the operands where an observation sits at the gate's radius, so the pose is also
compared with the PLAIN float64 prefix solves at the kernel's own returned weights, under the same yardstick: that comparison has no
discontinuity in it.  cond(A) of every prefix system used is computed on the CPU and held below 1e10."""
import itertools

import pytest
import torch

import filter_statement as FL
import fisheye_statement as FS
import trajectory_statement as TS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = FS.MARGIN
MAX_LAG = 64
# (N, T, J): the band is narrower than five where T < 5; at (1, 65, 3) the ring wraps many times; (5, 9, 15) is 75 tracks, two workgroups
SHAPES = [(1, 1, 1), (2, 2, 3), (1, 3, 2), (2, 4, 15), (1, 5, 16), (1, 33, 4), (1, 65, 3), (5, 9, 15)]
CASES = [c for c in TS.CASES if c != "nonfinite"]
LAMBDAS = [(0.0, 10.0), (1.0, 0.0), (0.5, 100.0), (0.0, 1000.0)]          # (lambda_v, lambda_a)
GATES = (0.0, 2.0)
VALUES = ("pose", "residual", "weight")
NAMES = ("pose", "valid", "residual", "weight", "frame")
_SCENES, _REFS = {}, {}


def lags(T):
    """0, 1, 2, 8 and the whole clip - nothing comes out before the tail - as far as the kernel's limit of 64 goes: at T = 65 the
    largest lag is 64, one row does come out before the tail, and the "nothing before the tail" case is not reached for that shape
    (it is for the seven others)."""
    return sorted({0, 1, 2, 8, min(T, MAX_LAG)})


def scene(shape, case):
    if (shape, case) not in _SCENES:
        _SCENES[shape, case] = TS.scene(*shape, case)
    return _SCENES[shape, case]


def reference(shape, case, lam, gate, used=None):
    """The prefix solves in float64 and float32 on the case's fp32 operands, computed once and shared (never modified; `outputs` reads a
    lag and a max_gap off them); "f32" is the float64 one where the float32 evaluation does not factor or is not finite: its own
    deviation is then 0 and the floor alone holds.  With `used` (the kernel's weights): the plain solves at those weights, not cached."""
    key = (shape, case, lam, gate)
    if used is None and key in _REFS:
        return _REFS[key]
    sc = scene(shape, case)
    f64 = FL.prefixes(sc["pose"], sc["weight"], sc["obs"], lam[0], lam[1], gate, used=used)
    f32 = FL.try_prefixes(sc["pose"], sc["weight"], sc["obs"], lam[0], lam[1], gate, dt=torch.float32, used=used)
    ref = {"f64": f64, "f32": f64 if f32 is None else f32, "f32_failed": f32 is None, "cond": FL.condition(f64, lam[0], lam[1])}
    if used is None:
        _REFS[key] = ref
    return ref


def dev(t):
    return None if t is None else t.to(DEV)


def cut(t, a, b):
    return None if t is None else t[:, a:b].contiguous()


def feed(sc, lam, lag, gate, gap, chunks=None, state=None, reset_at=None):
    """The stream of a scene through hip.trajectory_filter in calls of the given lengths (None: one call) ->
    (steps (N, T, J, ...), tail (N, lag, J, ...), state): dictionaries of CPU tensors, the state still on the device."""
    from egorear_amd import hip
    pose, weight, obs = dev(sc["pose"]), dev(sc["weight"]), dev(sc["obs"])
    N, T, J = pose.shape[:3]
    state = hip.trajectory_filter_state(N, J, lag, DEV) if state is None else state
    parts, at = [], 0
    for c in (chunks or [T]):
        reset = None if reset_at is None or reset_at[0] != at else dev(reset_at[1])
        parts.append(hip.trajectory_filter(state, cut(pose, at, at + c), cut(weight, at, at + c), cut(obs, at, at + c), reset, lag, lam[0], lam[1],
                                           gate, gap))
        at += c
    assert at == T
    tail = hip.trajectory_filter_tail(state, N, J, lag, lam[0], lam[1], gap)
    torch.cuda.synchronize()
    steps = {k: torch.cat([p[i] for p in parts], 1).cpu() for i, k in enumerate(NAMES)}
    return steps, dict(zip(NAMES, (t.cpu() for t in tail))), state


def whole(steps, tail, lag):
    """Frames 0..T-1, each as it came out: from the arrival that described it, the last `lag` from the tail."""
    T = steps["pose"].shape[1]
    return {k: torch.cat((steps[k][:, lag:], tail[k][:, max(lag - T, 0):]), 1) for k in NAMES}


def both(ref_out):
    steps, tail = ref_out
    return {k: torch.cat((steps[k], tail[k]), 1) for k in NAMES}


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_statement(shape, case):
    sc = scene(shape, case)
    N, T, J = shape
    base = TS.base_weights(sc["pose"], sc["weight"], sc["obs"])[0]
    bad, worst = [], {}
    for i, (lam, gate) in enumerate(itertools.product(LAMBDAS, GATES)):
        ref = reference(shape, case, lam, gate)
        print(f"{shape} {case} lambda {lam} gate {gate}: largest cond(A) of a prefix {ref['cond']:.3e}"
              f"{', float32 evaluation failed' if ref['f32_failed'] else ''}")
        assert ref["cond"] <= 1e10, (shape, case, lam, gate, ref["cond"])
        own = None
        for k, lag in enumerate(lags(T)):
            # every lag meets every max_gap over i = 0..7, every lambda (two consecutive i) and every gate (i even / odd) over the lags
            gap = (0, 3, T)[(i + k) % 3]
            steps, tail, _ = feed(sc, lam, lag, gate, gap)
            got = {name: torch.cat((steps[name], tail[name]), 1) for name in NAMES}
            f64, f32 = both(FL.outputs(ref["f64"], lag, gap)), both(FL.outputs(ref["f32"], lag, gap))
            tag = (shape, case, lam, gate, lag, gap)
            assert torch.equal(got["valid"].bool(), f64["valid"]), tag
            assert torch.equal(got["frame"], f64["frame"]), tag
            print(f"  lag {lag} max_gap {gap}: {int(f64['valid'].sum())} of {f64['valid'].numel()} rows valid")
            for name in VALUES:
                assert bool(torch.isfinite(got[name]).all()), tag + (name,)
                err, allowed = FS.yardstick(name, got[name], f32[name], f64[name])
                worst[name] = max(worst.get(name, 0.0), err / allowed if allowed else 0.0)
                if not err <= allowed:
                    bad.append(tag + (name, err, allowed))
            blank = (got["frame"] < 0).unsqueeze(-1)                                   # a row that describes no frame is zeros
            for name in VALUES + ("valid",):
                v = got[name].float()
                assert float((v.flatten(2).abs() * blank).sum()) == 0.0, tag + (name,)
            # the weights as the kernel assigned them, frame by frame: they do not depend on the lag, bit for bit
            full = whole(steps, tail, lag)
            used = torch.where(full["weight"] > 0, full["weight"], base)                # (an unsolvable prefix writes 0: the gate had no say)
            if own is None:
                own = used
                if gate > 0:
                    mine = reference(shape, case, lam, gate, used=used)
            assert torch.equal(used, own), tag
            if gate > 0:
                p64, p32 = both(FL.outputs(mine["f64"], lag, gap)), both(FL.outputs(mine["f32"], lag, gap))
                err, allowed = FS.yardstick("pose at its own weights", got["pose"], p32["pose"], p64["pose"])
                worst["own"] = max(worst.get("own", 0.0), err / allowed if allowed else 0.0)
                if not err <= allowed:
                    bad.append(tag + ("pose at its own weights", err, allowed))
    print(f"{shape} {case}: largest deviation / allowance {', '.join(f'{k} {v:.3g}' for k, v in worst.items())}")
    assert not bad, bad


@pytest.mark.parametrize("case", ["dense", "gaps", "mask"])
@pytest.mark.parametrize("shape", SHAPES)
def test_with_the_clip_as_lag_the_tail_is_stationary_and_the_clip_smoothers(shape, case):
    from egorear_amd import hip
    sc = scene(shape, case)
    N, T, J = shape
    lag = min(max(T - 1, 1), MAX_LAG)                                                  # >= T - 1: every frame comes from the last prefix
    for lam in LAMBDAS:
        steps, tail, _ = feed(sc, lam, lag, 0.0, T)
        x = whole(steps, tail, lag)
        assert x["pose"].shape == (N, T, J, 3) and x["frame"].tolist() == [list(range(T))] * N
        g, allowed, _ = TS.stationarity(x["pose"], sc["weight"], sc["obs"], sc["pose"], lam[0], lam[1])
        worst = g.abs().amax(-1)
        ratio = float(torch.where(allowed > 0, worst / allowed.clamp_min(1e-300), torch.zeros_like(worst)).max())
        clip = hip.trajectory_smooth(dev(sc["pose"]), dev(sc["weight"]), dev(sc["obs"]), lam[0], lam[1], 0.0, 0, T)
        torch.cuda.synchronize()
        print(f"{shape} {case} lambda {lam}: stationarity, largest |g_i| / allowance {ratio:.3g}")
        assert bool((worst <= MARGIN * allowed).all()), (shape, case, lam, ratio)
        for name, other in zip(("pose", "valid", "residual", "weight"), clip):
            other = other.cpu()
            if name == "valid":
                assert torch.equal(x[name], other), (shape, case, lam)
                continue
            # (the residual is a difference of positions: where the track passes through its observations it is rounding noise of
            # the positions' size, so its floor is the pose's)
            diff, floor = float((x[name] - other).abs().max()), 4.0 * FS.ulp32(float((clip[0] if name == "residual" else other).abs().max()))
            print(f"    {name}: |filter - trajectory_smooth| {diff:.3e}, 4 ulp floor {floor:.3e}, bit-equal: {torch.equal(x[name], other)}")
            assert diff <= floor, (shape, case, lam, name, diff, floor)


def test_the_bits_do_not_depend_on_how_a_stream_is_cut_into_calls():
    for case, lam, lag, gate in (("gaps", (0.0, 10.0), 4, 2.0), ("glitch", (0.5, 100.0), 8, 1.0), ("mask", (1.0, 0.0), 0, 0.0),
                                 ("sparse", (0.0, 1000.0), 2, 2.0)):
        sc = scene((2, 23, 15), case)
        T = 23
        one = feed(sc, lam, lag, gate, 3)
        for chunks in ([1] * T, [3] * 7 + [2], [1, 7, T - 8]):
            other = feed(sc, lam, lag, gate, 3, chunks)
            for a, b in zip(one[:2], other[:2]):
                for name in NAMES:
                    assert torch.equal(a[name], b[name]), (case, chunks, name)
            assert torch.equal(one[2], other[2]), (case, chunks, "state")
        assert bool(one[0]["valid"].any()) and bool(torch.isfinite(one[2]).all())


def test_reset_starts_a_stream_anew_and_leaves_the_others_alone():
    from egorear_amd import hip
    lam, lag, gate, at = (0.0, 10.0), 3, 2.0, 9
    sc = scene((3, 20, 5), "gaps")
    flags = torch.tensor([0, 1, 0], dtype=torch.uint8)
    steps, tail, state = feed(sc, lam, lag, gate, 3, [at, 20 - at], reset_at=(at, flags))
    plain_steps, plain_tail, _ = feed(sc, lam, lag, gate, 3, [at, 20 - at])
    later = {k: (None if sc[k] is None else sc[k][1:2, at:].contiguous()) for k in ("pose", "weight", "obs")}
    fresh_steps, fresh_tail, fresh = feed(later, lam, lag, gate, 3)
    # the chain, the pending frames and the counts are a new stream's - and so is the ring here, every slot of which the 9 rows committed
    # since the reset have overwritten (a slot none has reached keeps the earlier stream's row, which nothing reads)
    assert torch.equal(state[:, 5:10], fresh)
    for name in NAMES:
        assert torch.equal(steps[name][1:2, at:], fresh_steps[name]) and torch.equal(tail[name][1:2], fresh_tail[name]), name
        for n in (0, 2):                                                               # the other two: untouched, bit for bit
            assert torch.equal(steps[name][n], plain_steps[name][n]) and torch.equal(tail[name][n], plain_tail[name][n]), name
        assert torch.equal(steps[name][:, :at], plain_steps[name][:, :at])
    assert steps["frame"][1, at:].tolist() == [-1] * lag + list(range(20 - at - lag)) and not torch.equal(steps["pose"][1, at:], plain_steps["pose"][1, at:])
    # a state of zeros is the empty stream, and a reset of every stream gives what a new state gives
    state = hip.trajectory_filter_state(3, 5, lag, DEV)
    feed(sc, lam, lag, gate, 3, state=state)
    again = feed(sc, lam, lag, gate, 3, state=state, reset_at=(0, torch.ones(3, dtype=torch.uint8)))
    new = feed(sc, lam, lag, gate, 3)
    for a, b in zip(again[:2], new[:2]):
        assert all(torch.equal(a[name], b[name]) for name in NAMES)


@pytest.mark.parametrize("shape", [(2, 4, 15), (1, 33, 4), (5, 9, 15)])
def test_what_is_planted_in_a_gap_reaches_no_output_and_no_state(shape):
    sc = scene(shape, "nonfinite")
    for (lam, gate), lag in zip(itertools.product(LAMBDAS, GATES), itertools.cycle(lags(shape[1]))):
        got, twin = feed(sc, lam, lag, gate, 3), feed(sc["twin"], lam, lag, gate, 3)
        for a, b in zip(got[:2], twin[:2]):
            for name in NAMES:
                assert bool(torch.isfinite(a[name].float()).all()), (shape, lam, gate, lag, name)
                assert torch.equal(a[name], b[name]), (shape, lam, gate, lag, name)
        assert bool(torch.isfinite(got[2]).all()) and torch.equal(got[2], twin[2]), (shape, lam, gate, lag, "state")


def test_one_captured_decode_stream_3d_replays_for_every_frame():
    from egorear_amd import decode
    g = torch.Generator().manual_seed(91)
    cams = FS.rig()
    N, T, J = 2, 12, 15
    pts = TS.motion(N, T, J, g)
    hm = FS.bumps(pts.view(N * T, J, 3), FS.records(cams), None, FS.HM, FS.HM).float().view(N, T, 4, J, FS.HM, FS.HM).contiguous()
    for n, t, j in ((0, 2, 3), (0, 3, 3), (1, 0, 7), (1, 5, 14), (0, 4, 0)):            # lost by three views: the triangulation gives them up
        hm[n, t, 1:, j] = 0.0
    hm = hm.to(DEV)
    kw = dict(accel_weight=10.0, vel_weight=0.5, gate_cm=2.0, max_gap=2)
    eager_state, piece_state, graph_state = (decode.new_track_filter(N, J, 3, DEV, **kw) for _ in range(3))
    eager = [decode.decode_stream_3d(eager_state, hm[:, t], cams) for t in range(T)]
    pieces = []
    for t in range(T):
        joints, _ = decode.decode_joints_3d(hm[:, t].contiguous(), cams)
        pieces.append((joints, decode.filter_trajectory(piece_state, joints.pose, None, joints.valid)))
    torch.cuda.synchronize()
    static = hm[:, 0].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                      # one stream, no parallel branches
        out = decode.decode_stream_3d(graph_state, static, cams)
    assert float(graph_state.tensor.abs().sum()) == 0.0                                # captured, not run
    for t in range(T):
        static.copy_(hm[:, t])
        graph.replay()
        torch.cuda.synchronize()
        for a, b, c in zip(out[0] + out[1], eager[t][0] + eager[t][1], pieces[t][0] + pieces[t][1]):
            assert torch.equal(a, b) and torch.equal(a, c), t
    assert torch.equal(graph_state.tensor, eager_state.tensor) and torch.equal(graph_state.tensor, piece_state.tensor)
    last = eager[-1][1]
    assert last.frame.tolist() == [T - 1 - 3] * N and last.valid.dtype == torch.bool and bool(last.valid.all())
    rest = decode.filter_tail(eager_state)
    assert rest.pose.shape == (N, 3, J, 3) and rest.frame.tolist() == [[T - 3, T - 2, T - 1]] * N
    filled = torch.stack([e[1].pose for e in eager[3:]] + list(rest.pose.unbind(1)), 1)    # frames 0..T-1 as they came out
    err = (filled.double().cpu() - pts).norm(dim=-1)
    print(f"mean error of the filtered stream {float(err.mean()):.4e} cm, in the frames the triangulation gave up "
          f"{[round(float(err[n, t, j]), 4) for n, t, j in ((0, 2, 3), (0, 3, 3), (1, 0, 7), (1, 5, 14), (0, 4, 0))]}")
    assert bool(torch.isfinite(err).all())


def test_the_tail_leaves_the_state_alone_and_ends_in_the_causal_estimate():
    from egorear_amd import hip
    sc = scene((2, 23, 15), "gaps")
    pose, weight = dev(sc["pose"]), dev(sc["weight"])
    N, T, J = 2, 23, 15
    for lam, lag, gate in (((0.0, 10.0), 4, 2.0), ((0.5, 100.0), 8, 0.0), ((1.0, 0.0), 1, 2.0)):
        state, causal = hip.trajectory_filter_state(N, J, lag, DEV), hip.trajectory_filter_state(N, J, 0, DEV)
        quiet = hip.trajectory_filter_state(N, J, lag, DEV)                            # the same stream, no tail in between
        differ, largest = {"pose": 0, "residual": 0, "weight": 0}, {"pose": 0.0, "residual": 0.0, "weight": 0.0}
        for t in range(T):
            args = (cut(pose, t, t + 1), cut(weight, t, t + 1), None, None)
            hip.trajectory_filter(state, *args, lag, lam[0], lam[1], gate, 3)
            hip.trajectory_filter(quiet, *args, lag, lam[0], lam[1], gate, 3)
            now = hip.trajectory_filter(causal, *args, 0, lam[0], lam[1], gate, 3)     # lag 0: the step's output is the present
            before = state.clone()
            tail = hip.trajectory_filter_tail(state, N, J, lag, lam[0], lam[1], 3)
            assert torch.equal(state, before) and torch.equal(state, quiet), (lam, lag, t)
            assert tail[4][:, -1].tolist() == [t] * N and torch.equal(tail[1][:, -1], now[1][:, 0])
            for name, a, b in (("pose", tail[0], now[0]), ("residual", tail[2], now[2]), ("weight", tail[3], now[3])):
                # (the residual's floor is the pose's: a difference of positions)
                diff, floor = float((a[:, -1] - b[:, 0]).abs().max()), 4.0 * FS.ulp32(float((now[0] if name == "residual" else b).abs().max()))
                differ[name] += 0 if torch.equal(a[:, -1], b[:, 0]) else 1
                largest[name] = max(largest[name], diff)
                assert diff <= floor, (lam, lag, t, name, diff, floor)
        print(f"lambda {lam} lag {lag} gate {gate}: the tail's last row against the lag-0 step over {T} frames - frames not bit-equal "
              f"{differ}, largest difference {({k: f'{v:.3e}' for k, v in largest.items()})}")


def test_bad_launches_are_refused():
    from egorear_amd import hip
    sc = scene((2, 4, 15), "dense")
    p, w = dev(sc["pose"]), dev(sc["weight"])
    state = hip.trajectory_filter_state(2, 15, 4, DEV)
    good = dict(lag=4, vel_weight=0.0, accel_weight=10.0, gate=0.0, max_gap=8)
    for kw in ({"vel_weight": -1.0}, {"accel_weight": 0.0}, {"gate": -1.0}, {"gate": float("nan")}, {"max_gap": -1}, {"lag": 5}, {"lag": 65},
               {"accel_weight": float("nan")}):
        with pytest.raises(ValueError):
            hip.trajectory_filter(state, p, w, None, None, **dict(good, **kw))
    with pytest.raises(ValueError):
        hip.trajectory_filter(state, p, w[:, :3], None, None, **good)
    with pytest.raises(ValueError):
        hip.trajectory_filter(state, p.transpose(1, 2), None, None, None, **good)
    with pytest.raises(ValueError):
        hip.trajectory_filter(state.float(), p, None, None, None, **good)
    with pytest.raises(ValueError):
        hip.trajectory_filter_tail(state, 2, 15, 5)
    assert float(state.abs().sum()) == 0.0                                             # nothing was launched

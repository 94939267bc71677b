"""CPU-side checks of the causal fixed-lag trajectory filter (egorear_amd/decode.py): the statements of
tests/filter_statement.py, which the GPU tests compare the kernels with, are held to known answers - a line comes back as the line at
every lag, a constant as the constant, with lag >= T - 1 the tail is the clip smoother's answer, the streaming banded loop agrees with
the dense prefix solves, the gate lowers the error at the glitches, the solvable rule on its corners - and the Python layers are
checked as far as they go without a device: every parameter, shape and state error is a ValueError before any launch, the operators'
fake implementations give the documented shapes and dtypes, the library exports the three entries and refuses bad arguments itself."""
import ctypes
import itertools

import pytest
import torch

import filter_statement as FL
import fisheye_statement as FS
import trajectory_statement as TS

META = lambda *s, **k: torch.empty(*s, device="meta", **k)
SHAPES = [(1, 1, 1), (2, 2, 3), (1, 3, 2), (2, 4, 15), (1, 5, 16), (1, 33, 4), (1, 65, 3)]
LAMBDAS = [(0.0, 10.0), (1.0, 0.0), (0.5, 100.0), (0.0, 1000.0)]
LAGS = (0, 1, 2, 8)


# --------------------------------------------------------------------------- the statements on known answers

@pytest.mark.parametrize("T", [3, 5, 33])
def test_observations_on_a_line_return_the_line_at_every_lag(T):
    g = torch.Generator().manual_seed(T)
    N, J = 2, 4
    t = torch.arange(T, dtype=torch.float64).view(1, T, 1, 1)
    line = FS.random_points(N, J, g).unsqueeze(1) + 0.3 * torch.randn(N, 1, J, 3, generator=g, dtype=torch.float64) * t
    weight = 0.5 + torch.rand(N, T, J, generator=g, dtype=torch.float64)
    weight[torch.rand(N, T, J, generator=g) < 0.5] = 0.0
    weight[:, 0], weight[:, 1] = 1.0, 0.7                                             # two frames seen from the second arrival on
    planted = line.clone()
    planted[weight == 0] = float("nan")                                               # what stands in a gap is never read
    for la, gate in itertools.product((1.0, 1000.0), (0.0, 2.0)):
        pre = FL.prefixes(planted, weight, None, 0.0, la, gate)
        for lag in (0, 1, 2, 8):
            for (steps, tail), kind in ((FL.outputs(pre, lag, T), "dense"), (FL.streaming(planted, weight, None, 0.0, la, lag, gate, T), "loop")):
                worst = 0.0
                for t_arr in range(max(lag, 1), T):                                   # once two frames have been seen
                    assert steps["frame"][:, t_arr].tolist() == [t_arr - lag] * N
                    worst = max(worst, float((steps["pose"][:, t_arr] - line[:, t_arr - lag]).abs().max()))
                    assert bool(steps["valid"][:, t_arr].all()) and float(steps["residual"][:, t_arr].max()) <= 1e-6
                for i in range(lag):
                    if T - lag + i >= 0:
                        worst = max(worst, float((tail["pose"][:, i] - line[:, T - lag + i]).abs().max()))
                # (a prefix extrapolates from as few as two observations: cond(A) reaches 1e7 at lambda_a = 1000, times 2.2e-16 times
                # coordinates of 100 cm is 2e-7 cm - the 1e-6 cm that the two statements are held to against each other)
                assert worst <= 1e-6, (la, gate, lag, kind, worst)
                first = max(lag, 1)
                assert first >= T or torch.equal(steps["weight"][:, first:], weight[:, first - lag:T - lag])     # on the line no gate bites


def test_a_constant_stream_returns_the_constant():
    g = torch.Generator().manual_seed(5)
    N, T, J = 2, 20, 3
    const = FS.random_points(N, J, g).unsqueeze(1).expand(N, T, J, 3).contiguous()
    obs = (torch.rand(N, T, J, generator=g) < 0.4).to(torch.uint8)
    obs[:, 0] = 1
    for lv, lag in itertools.product((0.1, 100.0), (0, 3)):
        for steps, tail in (FL.run(const, None, obs, lv, 0.0, lag), FL.streaming(const, None, obs, lv, 0.0, lag)):
            assert float((steps["pose"][:, lag:] - const[:, :T - lag]).abs().max()) <= 1e-9
            assert lag == 0 or float((tail["pose"] - const[:, T - lag:]).abs().max()) <= 1e-9
            assert steps["frame"][0].tolist() == [-1] * lag + list(range(T - lag)) and float(steps["pose"][:, :lag].abs().sum()) == 0.0


@pytest.mark.parametrize("case", ["dense", "gaps", "mask", "sparse", "ends"])
def test_with_the_whole_clip_as_lag_the_tail_is_the_clip_smoother(case):
    for shape, (lv, la) in itertools.product(((1, 1, 1), (2, 2, 3), (1, 3, 2), (2, 4, 15), (1, 33, 4)), LAMBDAS):
        sc = TS.scene(*shape, case)
        T = shape[1]
        clip = TS.smooth(sc["pose"], sc["weight"], sc["obs"], lv, la, max_gap=3)
        for lag in (max(T - 1, 1), T, T + 2):
            steps, tail = FL.run(sc["pose"], sc["weight"], sc["obs"], lv, la, lag, 0.0, 3)
            rows = slice(lag - T, lag)                                                 # the rows that are frames 0..T-1
            if lag >= T:
                assert float(steps["pose"].abs().sum()) == 0.0 and bool((steps["frame"] == -1).all()) and not bool(steps["valid"].any())
                assert bool((tail["frame"][:, :lag - T] == -1).all()) and float(tail["pose"][:, :lag - T].abs().sum()) == 0.0
                for name in ("pose", "residual", "weight"):
                    assert float((tail[name][:, rows] - clip[name]).abs().max()) <= 1e-9, (shape, case, lv, la, lag, name)
                assert torch.equal(tail["valid"][:, rows], clip["valid"])
            else:                                                                      # lag = T - 1: frame 0 came out at the last arrival
                assert float((torch.cat((steps["pose"][:, -1:], tail["pose"]), 1) - clip["pose"]).abs().max()) <= 1e-9
                assert torch.equal(torch.cat((steps["valid"][:, -1:], tail["valid"]), 1), clip["valid"])


@pytest.mark.parametrize("shape", SHAPES)
def test_the_streaming_loop_agrees_with_the_dense_prefix_solves(shape):
    worst, worst_cond = 0.0, 1.0
    for case in ("dense", "gaps", "mask", "sparse"):
        sc = TS.scene(*shape, case)
        for (lv, la), gate in itertools.product(LAMBDAS, (0.0, 2.0)):
            pre = FL.prefixes(sc["pose"], sc["weight"], sc["obs"], lv, la, gate)
            cond = FL.condition(pre, lv, la)
            worst_cond = max(worst_cond, cond)
            assert cond <= 1e10, (shape, case, lv, la, gate, cond)
            for i, lag in enumerate(LAGS):
                gap = (0, 3, shape[1])[i % 3]
                for a, b in zip(FL.outputs(pre, lag, gap), FL.streaming(sc["pose"], sc["weight"], sc["obs"], lv, la, lag, gate, gap)):
                    assert torch.equal(a["valid"], b["valid"]) and torch.equal(a["frame"], b["frame"]), (shape, case, lv, la, gate, lag)
                    for name in ("pose", "residual", "weight"):
                        if a[name].numel():
                            worst = max(worst, float((a[name] - b[name]).abs().max()))
    print(f"{shape}: |streaming loop - dense prefix solves| {worst:.3e} cm, largest cond(A) of a prefix {worst_cond:.3e}")
    assert worst <= 1e-6


# --------------------------------------------------------------------------- the gate

def test_the_gate_lowers_the_error_at_the_glitches_and_keeps_every_weight_positive():
    sc = TS.scene(2, 64, 15, "glitch")
    truth = sc["truth"]
    at = (sc["pose"].double() - truth).norm(dim=-1) > 20.0                             # the 90 glitches
    assert int(at.sum()) == 90
    base, _ = TS.base_weights(sc["pose"].double(), sc["weight"].double(), None)
    figures = {}
    for gate in (0.0, 2.0):
        pre = FL.prefixes(sc["pose"], sc["weight"], None, 0.0, 10.0, gate)
        assert float(pre["u"].min()) > 0.0 and bool((pre["u"] <= base).all())           # never zero or negative, never raised
        for lag in (0, 4, 8):
            steps, tail = FL.outputs(pre, lag, 8)
            x = torch.cat((steps["pose"][:, lag:], tail["pose"]), 1)                   # frames 0..T-1, each as it came out
            err = (x - truth).norm(dim=-1)
            figures[gate, lag] = (float(err.mean()), float(err[at].mean()))
    for lag in (0, 4, 8):
        print(f"lag {lag}: mean error no gate {figures[0.0, lag][0]:.3f} / gate 2 cm {figures[2.0, lag][0]:.3f} cm, at the glitches "
              f"{figures[0.0, lag][1]:.3f} / {figures[2.0, lag][1]:.3f} cm")
        assert figures[2.0, lag][1] < figures[0.0, lag][1]


def test_a_huge_gate_changes_nothing_bit_for_bit():
    for case, (lv, la) in (("glitch", (0.0, 10.0)), ("gaps", (0.5, 100.0))):
        sc = TS.scene(2, 17, 3, case)
        for dt in (torch.float64, torch.float32):
            off, on = (FL.prefixes(sc["pose"], sc["weight"], sc["obs"], lv, la, gate, dt) for gate in (0.0, 1e30))
            assert torch.equal(off["u"], on["u"]) and all(torch.equal(a, b) for a, b in zip(off["x"], on["x"]))
        for a, b in zip(FL.streaming(sc["pose"], sc["weight"], sc["obs"], lv, la, 4, 0.0), FL.streaming(sc["pose"], sc["weight"], sc["obs"], lv, la, 4, 1e30)):
            assert all(torch.equal(a[k], b[k]) for k in FL.FIELDS)


# --------------------------------------------------------------------------- the solvable rule on prefixes

def test_the_solvable_rule_on_prefixes_and_a_late_first_observation():
    g = torch.Generator().manual_seed(3)
    T = 9
    pose = torch.randn(1, T, 1, 3, generator=g)
    # lambda_v = 0: the prefixes of one and two frames need every frame; from three frames on two observations are enough
    obs = torch.tensor([1, 0, 0, 1, 1, 1, 1, 1, 1], dtype=torch.uint8).view(1, T, 1)
    for fn in (FL.run, FL.streaming):
        steps, _ = fn(pose, None, obs, 0.0, 10.0, 0, 0.0, 8)
        assert steps["valid"].flatten().tolist() == [True, False, False] + [True] * 6
        assert float(steps["pose"][:, 1:3].abs().sum()) == 0.0 and float(steps["pose"][:, 0].abs().sum()) > 0.0
        assert steps["frame"].flatten().tolist() == list(range(T))                     # the row is there, as zeros
        # lambda_v > 0: one observation is enough, from the frame it arrives in
        steps, _ = fn(pose, None, obs, 1.0, 0.0, 0, 0.0, 8)
        assert bool(steps["valid"].all())
        assert float((steps["pose"][0, 2, 0] - pose[0, 0, 0].double()).abs().max()) <= 1e-12     # the one observation, held
    # a first observation that comes late: zeros and valid False until then, the clip smoother's frames afterwards
    late = torch.zeros(1, T, 1, dtype=torch.uint8)
    late[0, 4:] = 1
    for (lv, la), lag in itertools.product(((0.0, 10.0), (1.0, 0.0)), (0, 2)):
        first = 4 if lv > 0 else 5                                                     # the arrival that makes the prefix solvable
        for fn in (FL.run, FL.streaming):
            steps, tail = fn(pose, None, late, lv, la, lag, 0.0, 2)
            assert not bool(steps["valid"][:, :first].any()) and float(steps["pose"][:, :first].abs().sum()) == 0.0
            assert float(steps["weight"][:, :first].abs().sum()) == 0.0
            for t in range(first, T):
                want = TS.smooth(pose[:, :t + 1], None, late[:, :t + 1], lv, la, max_gap=2)
                assert float((steps["pose"][:, t] - want["pose"][:, t - lag]).abs().max()) <= 1e-9
                assert torch.equal(steps["valid"][:, t], want["valid"][:, t - lag])
            assert steps["valid"][0, first:, 0].tolist() == [first + i - lag >= 2 for i in range(T - first)]  # frames 2, 3 are within max_gap of 4


# --------------------------------------------------------------------------- the Python layers without a device

def _state(N=2, J=3, lag=4, **kw):
    from egorear_amd import decode
    return decode.new_track_filter(N, J, lag, "meta", **kw)


def test_every_bad_parameter_shape_and_state_is_a_value_error_before_any_launch():
    from egorear_amd import decode, hip
    for kw in ({"lag": -1}, {"lag": 65}, {"lag": 1.0}, {"lag": True}, {"N": 0}, {"J": 0}, {"accel_weight": 0.0}, {"accel_weight": -1.0},
               {"vel_weight": -1.0}, {"vel_weight": float("nan")}, {"accel_weight": float("inf")}, {"gate_cm": -1.0}, {"gate_cm": float("nan")},
               {"gate_cm": float("inf")}, {"gate_cm": "x"}, {"max_gap": -1}, {"max_gap": 1.5}, {"N": 1 << 20, "J": 1 << 10, "lag": 64}):
        with pytest.raises(ValueError):
            _state(**kw)
    with pytest.raises(ValueError):
        decode.new_track_filter(2, 3, 4, "cpu")
    with pytest.raises(ValueError):
        hip.trajectory_filter_state(2, 3, 4, "cpu")
    assert hip.trajectory_filter_state_slots(0) == 23 and hip.trajectory_filter_state_slots(64) == 23 + 640
    st = _state()
    assert st.tensor.shape == (63, 6) and st.tensor.dtype == torch.float64 and (st.N, st.J, st.lag, st.max_gap) == (2, 3, 4, 8)
    good = (META(2, 5, 3, 3), META(2, 5, 3), META(2, 5, 3, dtype=torch.uint8), META(2, dtype=torch.uint8))
    decode.filter_trajectory(st, *good)
    bad = ((META(2, 5, 3), None, None, None), (META(2, 5, 3, 2), None, None, None), (META(2, 0, 3, 3), None, None, None),
           (META(3, 5, 3, 3), None, None, None), (META(2, 5, 4, 3), None, None, None), (META(2, 5, 3, 3, dtype=torch.float64), None, None, None),
           (good[0], META(2, 5, 4), None, None), (good[0], META(2, 5, 3, dtype=torch.float64), None, None), (good[0], None, META(2, 5, 3), None),
           (good[0], None, META(2, 4, 3, dtype=torch.uint8), None), (good[0], None, None, META(3, dtype=torch.uint8)),
           (good[0], None, None, META(2)), (good[0], None, None, META(2, 1, dtype=torch.uint8)))
    for p, w, o, r in bad:
        if p.dim() == 4:
            with pytest.raises(ValueError):
                decode.filter_trajectory(st, p, w, o, r)
        with pytest.raises(ValueError):
            hip.trajectory_filter(st.tensor, p, w, o, r, 4, 0.0, 10.0, 0.0, 8)
        with pytest.raises(ValueError):
            decode.trajectory_filter_op(st.tensor, p, w, o, r, 4, 0.0, 10.0, 0.0, 8)
    # a state that does not fit the call: another lag, another shape, another dtype, other parameters, not a state at all
    for other in (st._replace(lag=5), st._replace(N=3), st._replace(J=2), st._replace(tensor=META(63, 6)), st._replace(tensor=META(6, 63, dtype=torch.float64)),
                  st._replace(tensor=META(63, 12, dtype=torch.float64)[:, ::2]), st._replace(accel_weight=0.0), st._replace(gate_cm=-1.0),
                  st._replace(max_gap=-1), st.tensor, None):
        with pytest.raises(ValueError):
            decode.filter_trajectory(other, good[0])
        with pytest.raises(ValueError):
            decode.filter_tail(other)
        with pytest.raises(ValueError):
            decode.decode_stream_3d(other, META(2, 4, 3, 16, 16), FS.rig())
    for kw in ({"lag": 5}, {"vel_weight": -1.0}, {"accel_weight": 0.0}, {"gate": -1.0}, {"gate": float("nan")}, {"max_gap": -1}, {"lag": 65}):
        args = dict(dict(lag=4, vel_weight=0.0, accel_weight=10.0, gate=0.0, max_gap=8), **kw)
        with pytest.raises(ValueError):
            hip.trajectory_filter(st.tensor, good[0], None, None, None, **args)
        if "gate" not in kw:
            with pytest.raises(ValueError):
                hip.trajectory_filter_tail(st.tensor, 2, 3, args["lag"], args["vel_weight"], args["accel_weight"], args["max_gap"])
    with pytest.raises(ValueError):
        hip.trajectory_filter_tail(st.tensor, 3, 3, 4)
    for hm in (META(2, 4, 3, 16), META(2, 5, 1, 3, 16, 16), META(2, 5, 5, 3, 16, 16), META(3, 4, 3, 16, 16), META(2, 4, 4, 16, 16)):
        with pytest.raises(ValueError):
            decode.decode_stream_3d(st, hm, FS.rig()[:min(max(hm.shape[-4], 2), 4)])
    with pytest.raises(ValueError):
        decode.decode_stream_3d(st, META(2, 5, 4, 3, 16, 16), FS.rig(), META(10, 4, 4, 4))


def test_cpu_tensors_are_refused():
    from egorear_amd import decode, hip
    state, pose = torch.zeros(63, 6, dtype=torch.float64), torch.zeros(2, 1, 3, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.trajectory_filter(state, pose, lag=4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.trajectory_filter_tail(state, 2, 3, 4)
    st = decode.TrackFilterState(state, 2, 3, 4, 10.0, 0.0, 0.0, 8)
    with pytest.raises(ValueError, match="no CPU path"):
        decode.filter_trajectory(st, pose)
    with pytest.raises(ValueError, match="no CPU path"):
        decode.filter_trajectory(_state(), pose)                                       # the state on the device, the pose not
    with pytest.raises(ValueError, match="no CPU path"):
        decode.filter_tail(st)
    with pytest.raises(ValueError, match="no CPU path"):
        decode.decode_stream_3d(st, torch.zeros(2, 4, 3, 16, 16), FS.rig())
    with pytest.raises((NotImplementedError, RuntimeError)):                         # the operators themselves: no CPU kernel, no fallback
        decode.trajectory_filter_op(state, pose, None, None, None, 4, 0.0, 10.0, 0.0, 8)
    with pytest.raises((NotImplementedError, RuntimeError)):
        decode.trajectory_filter_tail_op(state, 2, 3, 4, 0.0, 10.0, 8)


def test_the_operators_fakes_give_the_documented_shapes_and_dtypes():
    from egorear_amd import decode
    for name in ("trajectory_filter", "trajectory_filter_tail"):
        assert hasattr(torch.ops.egorear_amd, name), name
    for (N, C, J), lag in itertools.product(((1, 1, 1), (2, 3, 15), (64, 8, 15)), (0, 1, 8, 64)):
        st = _state(N, J, lag, gate_cm=2.0, vel_weight=0.5)
        assert st.tensor.shape == (23 + 10 * lag, N * J)
        for with_w, with_o, with_r in ((True, True, True), (False, False, False), (True, False, True)):
            pose = META(N, C, J, 3).requires_grad_()
            weight = META(N, C, J).requires_grad_() if with_w else None
            obs = META(N, C, J, dtype=torch.uint8) if with_o else None
            reset = META(N, dtype=torch.uint8) if with_r else None
            out = decode.trajectory_filter_op(st.tensor, pose.detach(), None if weight is None else weight.detach(), obs, reset, lag, 0.5, 10.0,
                                              2.0, 8)
            assert out[0].shape == (N, C, J, 3) and out[1].shape == out[2].shape == out[3].shape == (N, C, J) and out[4].shape == (N, C)
            assert [t.dtype for t in out] == [torch.float32, torch.uint8, torch.float32, torch.float32, torch.int64]
            step = decode.filter_trajectory(st, pose, weight, None if obs is None else obs.view(torch.bool),
                                            None if reset is None else reset.view(torch.bool))
            assert isinstance(step, decode.TrackStep) and step._fields == ("pose", "valid", "residual", "weight", "frame")
            assert not any(t.requires_grad for t in step)                              # nothing is differentiable
            assert step.pose.shape == (N, C, J, 3) and step.valid.dtype == torch.bool and step.frame.shape == (N, C)
        one = decode.filter_trajectory(st, META(N, J, 3), META(N, J), META(N, J, dtype=torch.bool))      # (N, J, 3): one frame
        assert one.pose.shape == (N, J, 3) and one.valid.shape == one.residual.shape == one.weight.shape == (N, J) and one.frame.shape == (N,)
        tail = decode.trajectory_filter_tail_op(st.tensor, N, J, lag, 0.5, 10.0, 8)
        assert tail[0].shape == (N, lag, J, 3) and tail[1].shape == tail[2].shape == tail[3].shape == (N, lag, J) and tail[4].shape == (N, lag)
        assert [t.dtype for t in tail] == [torch.float32, torch.uint8, torch.float32, torch.float32, torch.int64]
        rest = decode.filter_tail(st)
        assert isinstance(rest, decode.TrackStep) and rest.pose.shape == (N, lag, J, 3) and rest.valid.dtype == torch.bool
    cams = FS.rig()
    st = _state(2, 15, 4)
    joints, step = decode.decode_stream_3d(st, META(2, 3, 4, 15, 64, 64), cams)
    assert isinstance(joints, decode.Joints3D) and isinstance(step, decode.TrackStep)
    assert joints.pose.shape == step.pose.shape == (2, 3, 15, 3) and joints.residual.shape == (2, 3, 4, 15) and step.frame.shape == (2, 3)
    joints, step = decode.decode_stream_3d(st, META(2, 3, 15, 32, 32), cams[:3], META(2, 3, 4, 4))
    assert joints.pose.shape == step.pose.shape == (2, 15, 3) and joints.cost.shape == (2, 15) and step.frame.shape == (2,)


def test_decode_stream_3d_traces_as_three_operators():
    import torch._dynamo as dynamo
    from egorear_amd import decode
    cams = FS.rig()
    st = _state(2, 15, 4, gate_cm=2.0)

    def serving_side(state, hm):
        joints, step = decode.decode_stream_3d(decode.TrackFilterState(state, 2, 15, 4, 10.0, 0.0, 2.0, 8), hm, cams)
        return step.pose, step.valid, step.frame, joints.valid

    hm = META(2, 4, 15, 64, 64)
    serving_side(st.tensor, hm)                                                        # (warms the record cache: the upload is not traced)
    dynamo.reset()
    ex = dynamo.explain(serving_side)(st.tensor, hm)
    assert ex.graph_break_count == 0 and ex.graph_count == 1, ex
    targets = [str(nd.target) for g in ex.graphs for nd in g.graph.nodes if nd.op == "call_function"]
    for name in ("egorear_amd.soft_argmax", "egorear_amd.triangulate", "egorear_amd.trajectory_filter"):
        assert sum(name in t for t in targets) == 1, (name, targets)


def test_the_library_exports_the_three_entries_and_refuses_bad_arguments_itself():
    from egorear_amd import hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ("egr_trajectory_filter_state_slots", "egr_trajectory_filter_f32", "egr_trajectory_filter_tail_f32"):
        assert name in hip.EXPORTS and hasattr(lib, name), name
    slots = hip.lib.egr_trajectory_filter_state_slots
    assert slots(0) == 23 and slots(8) == 103 and slots(64) == 663 and slots(-1) == hip.EINVAL and slots(65) == hip.EINVAL
    assert all(slots(lag) == hip.trajectory_filter_state_slots(lag) for lag in range(65))
    p = ctypes.c_void_p(64)                                                            # pointers that are never followed

    def step(N=1, C=1, J=2, lag=4, lv=0.0, la=10.0, gate=0.0, gap=8, pose=p, state=p, out=p, frame=p):
        return hip.lib.egr_trajectory_filter_f32(pose, None, None, None, state, N, C, J, lag, lv, la, gate, gap, out, p, p, p, frame, None)

    assert step(pose=None) == hip.ENULL and step(state=None) == hip.ENULL and step(out=None) == hip.ENULL and step(frame=None) == hip.ENULL
    for kw in ({"N": 0}, {"C": 0}, {"C": 4097}, {"J": 0}, {"lag": -1}, {"lag": 65}, {"N": 1 << 16, "C": 1 << 10, "J": 1 << 5},
               {"N": 1 << 12, "J": 1 << 10, "lag": 64}, {"lv": -1.0}, {"la": 0.0}, {"la": float("nan")}, {"lv": float("inf")}, {"gate": -1.0},
               {"gate": float("nan")}, {"gate": float("inf")}, {"gap": -1}):
        assert step(**kw) == hip.EINVAL, kw

    def tail(N=1, J=2, lag=4, lv=0.0, la=10.0, gap=8, state=p, out=p, frame=p):
        return hip.lib.egr_trajectory_filter_tail_f32(state, N, J, lag, lv, la, gap, out, p, p, p, frame, None)

    assert tail(state=None) == hip.ENULL and tail(out=None) == hip.ENULL and tail(frame=None) == hip.ENULL
    for kw in ({"N": 0}, {"J": 0}, {"lag": -1}, {"lag": 65}, {"N": 1 << 12, "J": 1 << 10, "lag": 64}, {"la": 0.0}, {"lv": -1.0}, {"gap": -1}):
        assert tail(**kw) == hip.EINVAL, kw
    assert tail(lag=0) == 0                                                            # no rows: nothing is launched

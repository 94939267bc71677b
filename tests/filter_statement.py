"""The float64 statement of the causal fixed-lag trajectory filter (egr_trajectory_filter_f32 / egr_trajectory_filter_tail_f32,
DESIGN.md 5w), built on trajectory_statement.  Not a test module: test_trajectory_filter_host.py, test_gpu_trajectory_filter.py and the
tools import it.

A stream is one joint's observations z_0, z_1, ... with the base weights w_t of TS.base_weights.  The used weights are u_t = w_t, or
with gate = delta > 0
    u_t = w_t min(1, delta / |z_t - p_t|),   p_t = frame t of the plain solution over the frames 0..t with the weights u_0..u_{t-1}, 0,
wherever TS.solvable admits that system (else u_t = w_t); a weight is fixed once assigned.  x^(t) is TS.smooth's plain solution over
the frames 0..t with the weights u.  The arrival of frame t outputs stream frame t - lag once t >= lag; the tail after T frames is
the frames max(T - lag, 0) .. T - 1 of x^(T-1).

  prefixes    the weights u and every x^(t) by DENSE prefix solves (TS.smooth, one call a prefix), in the dtype asked for (float64: the
              statement; float32: the evaluation that sets the yardstick's allowance).  They do not depend on lag or max_gap.
  outputs     what the arrivals and the tail give at a lag and a max_gap, read off the prefixes.
  streaming   a second statement of another kind: the banded elimination as a causal recursion - rows <= t - 2 committed with interior
              coefficients, the last two rows redone with the prefix's boundary coefficients, `lag` rows substituted back - as a Python
              loop in float64."""
import torch

import trajectory_statement as TS

FIELDS = ("pose", "valid", "residual", "weight", "frame")


_PENALTY = {}


def _plain(z, u, lv, la, dt):
    """TS.smooth's plain form on observations z with the weights u as they are (both already selected: u = 0 and z = 0 in a gap), from
    the same pieces - TS.solvable, TS.penalty, TS.solve_tracks - without the energy and the validity pass, and with the penalty matrix
    of a length built once: dict(pose, ok, residual)."""
    T = u.shape[1]
    if (T, lv, la, dt) not in _PENALTY:
        _PENALTY[T, lv, la, dt] = TS.penalty(T, lv, la, dt)
    ok = TS.solvable(u, lv)
    A = torch.diag_embed(u.permute(0, 2, 1)) + _PENALTY[T, lv, la, dt]
    A = torch.where(ok[..., None, None], A, torch.eye(T, dtype=dt).expand_as(A))
    x = TS.solve_tracks(A, (u.unsqueeze(-1) * z).permute(0, 2, 1, 3)).permute(0, 2, 1, 3)
    x = torch.where(ok.view(ok.shape[0], 1, ok.shape[1], 1), x, torch.zeros_like(x))
    r = torch.sqrt(torch.where(u > 0, ((x - z) ** 2).sum(-1), torch.zeros_like(u)))
    return {"pose": x, "ok": ok, "residual": torch.where(ok.unsqueeze(1), r, torch.zeros_like(r))}


def prefixes(pose, weight, obs, lv, la, gate=0.0, dt=torch.float64, used=None):
    """dict(w, z, u (N, T, J), x: list of x^(t) (N, t + 1, J, 3), ok: list of (N, J) bool, residual: list of (N, t + 1, J)).  With `used`
    (N, T, J) those weights are taken as u and no gate is evaluated: the plain prefix solves at given weights."""
    pose = pose.to(dt)
    w, z = TS.base_weights(pose, None if weight is None else weight.to(dt), obs)
    N, T, J = w.shape
    u = w.clone() if used is None else torch.where(w > 0, used.to(dt), torch.zeros_like(w))
    X, OK, R = [], [], []
    for t in range(T):
        if gate > 0 and used is None:
            trial = torch.cat((u[:, :t], torch.zeros_like(u[:, :1])), 1)
            known = TS.solvable(trial, lv) & (w[:, t] > 0)
            if bool(known.any()):
                p = _plain(z[:, :t + 1], trial, lv, la, dt)["pose"][:, t]
                r = torch.sqrt(((z[:, t] - p) ** 2).sum(-1))
                far = known & (r > gate)
                u[:, t] = torch.where(far, w[:, t] * (gate / torch.where(far, r, torch.ones_like(r))), w[:, t])
        out = _plain(z[:, :t + 1], u[:, :t + 1], lv, la, dt)
        X.append(out["pose"])
        OK.append(out["ok"])
        R.append(out["residual"])
    return {"w": w, "z": z, "u": u, "x": X, "ok": OK, "residual": R}


def try_prefixes(*args, **kw):
    """`prefixes`, or None where an evaluation does not factor or is not finite (float32 on an ill-conditioned prefix)."""
    try:
        pre = prefixes(*args, **kw)
    except RuntimeError:
        return None
    return pre if all(bool(torch.isfinite(x).all()) for x in pre["x"]) and bool(torch.isfinite(pre["u"]).all()) else None


def _blank(N, rows, J, dt):
    return {"pose": torch.zeros(N, rows, J, 3, dtype=dt), "valid": torch.zeros(N, rows, J, dtype=torch.bool),
            "residual": torch.zeros(N, rows, J, dtype=dt), "weight": torch.zeros(N, rows, J, dtype=dt),
            "frame": torch.full((N, rows), -1, dtype=torch.int64)}


def _row(out, i, pre, t, s, max_gap):
    """Row i of `out`: frame s of the prefix 0..t."""
    ok = pre["ok"][t]
    near = pre.setdefault("near", {})                                                  # TS.validity of a prefix, once per (t, max_gap)
    if (t, max_gap) not in near:
        near[t, max_gap] = TS.validity(pre["w"][:, :t + 1], torch.ones_like(ok), max_gap)
    out["pose"][:, i] = pre["x"][t][:, s]
    out["valid"][:, i] = near[t, max_gap][:, s] & ok
    out["residual"][:, i] = pre["residual"][t][:, s]
    out["weight"][:, i] = torch.where(ok, pre["u"][:, s], torch.zeros_like(pre["u"][:, s]))
    out["frame"][:, i] = s


def outputs(pre, lag, max_gap):
    """(steps, tail): the arrivals' rows (N, T, J, ...) - row t describes frame t - lag, frame -1 and zeros while t < lag - and the tail's
    rows (N, lag, J, ...), row i frame T - lag + i, -1 and zeros before the stream's start."""
    N, T, J = pre["w"].shape
    dt = pre["w"].dtype
    steps, tail = _blank(N, T, J, dt), _blank(N, lag, J, dt)
    for t in range(lag, T):
        _row(steps, t, pre, t, t - lag, max_gap)
    for i in range(lag):
        if T - lag + i >= 0:
            _row(tail, i, pre, T - 1, T - lag + i, max_gap)
    return steps, tail


def run(pose, weight, obs, lv, la, lag, gate=0.0, max_gap=8, dt=torch.float64):
    return outputs(prefixes(pose, weight, obs, lv, la, gate, dt), lag, max_gap)


def condition(pre, lv, la):
    """The largest 2-norm condition number over every prefix system the statement solved (1 when none was solvable)."""
    worst = 1.0
    for t, ok in enumerate(pre["ok"]):
        if bool(ok.any()):
            A = TS.matrices(pre["u"][:, :t + 1].double(), ok, lv, la)[ok]
            worst = max(worst, max(float(torch.linalg.cond(a)) for a in A))
    return worst


# --------------------------------------------------------------------------- the streaming banded loop

def _coefficients(t, to_end, lv, la):
    """Row t of the penalty of a prefix whose last row is t + to_end (TS.band written for that length)."""
    a, b, c = TS.band(t + to_end + 1, lv, la)
    return a[t], b[t], c[t]


class _Chain:
    """The elimination's carried state over (N, J) tracks: the last two pivots, sub-diagonals and reduced right-hand sides."""

    def __init__(self, N, J):
        zero = torch.zeros(N, J, dtype=torch.float64)
        self.d1, self.d2, self.e1, self.f1, self.f2 = zero, zero, zero, zero, zero
        self.y1, self.y2 = torch.zeros(N, J, 3, dtype=torch.float64), torch.zeros(N, J, 3, dtype=torch.float64)

    def copy(self):
        other = _Chain.__new__(_Chain)
        other.__dict__.update(self.__dict__)                                           # (tensors are replaced, never written in place)
        return other

    def step(self, diag, b, c, rhs):
        d = diag - self.e1 ** 2 * self.d1 - self.f2 ** 2 * self.d2
        e = (b - self.f1 * self.d1 * self.e1) / d
        f = c / d
        y = rhs - self.e1.unsqueeze(-1) * self.y1 - self.f2.unsqueeze(-1) * self.y2
        self.d2, self.d1, self.f2, self.f1, self.e1 = self.d1, d, self.f1, f, e
        self.y2, self.y1 = self.y1, y
        return e, f, y / d.unsqueeze(-1)


def streaming(pose, weight, obs, lv, la, lag, gate=0.0, max_gap=8):
    """(steps, tail) as `outputs` gives them, float64, frame after frame with a state that does not grow: the chain after the final rows,
    the last two frames, and the last `lag` final rows."""
    w, z = TS.base_weights(pose.double(), None if weight is None else weight.double(), obs)
    N, T, J = w.shape
    far = float(1 << 30)
    steps, tail = _blank(N, T, J, torch.float64), _blank(N, lag, J, torch.float64)
    chain, pend, ring, seen = _Chain(N, J), [], {}, torch.zeros(N, J, dtype=torch.int64)
    since = torch.full((N, J), far, dtype=torch.float64)

    def boundary(n, gating, before):
        """e, q of the rows n - 2 and n - 1 of the prefix of n frames on a copy of the chain; with `gating` pend[-1] is weighed first."""
        pr = chain.copy()
        ea, qa = torch.zeros(N, J, dtype=torch.float64), torch.zeros(N, J, 3, dtype=torch.float64)
        if n >= 2:
            a, b, c = _coefficients(n - 2, 1, lv, la)
            ea, _, qa = pr.step(a + pend[0]["u"], b, c, pend[0]["u"].unsqueeze(-1) * pend[0]["z"])
        a, b, c = _coefficients(n - 1, 0, lv, la)
        new = pend[-1]
        if gating:
            _, _, p = pr.copy().step(a + torch.zeros(N, J, dtype=torch.float64), b, c, torch.zeros(N, J, 3, dtype=torch.float64))
            known = (before >= 1) if lv > 0 else ((before >= 2) if n >= 3 else torch.zeros(N, J, dtype=torch.bool))
            r = torch.sqrt(((p - new["z"]) ** 2).sum(-1))
            hit = known & (new["u"] > 0) & (r > gate)                                   # (r is NaN or inf where the system is singular)
            new["u"] = torch.where(hit, new["u"] * (gate / torch.where(hit, r, torch.ones_like(r))), new["u"])
        _, _, qb = pr.step(a + new["u"], b, c, new["u"].unsqueeze(-1) * new["z"])
        return ea, qa, qb

    def substitute(n, ea, qa, qb, rows, emit):
        """x of the rows n - 1, n - 2, ... (`rows` of them at the most) of the prefix of n frames; emit(i, x, frame record, gap)."""
        ok = (seen >= 1) if lv > 0 else ((seen >= 2) if n >= 3 else (seen == n))
        x1, x2 = torch.zeros(N, J, 3, dtype=torch.float64), torch.zeros(N, J, 3, dtype=torch.float64)
        until = torch.full((N, J), far, dtype=torch.float64)
        for i in range(rows):
            s = n - 1 - i
            if s < 0:
                break
            rec = pend[-1] if i == 0 else pend[0] if i == 1 else ring[s % lag]
            e, f, q = (0.0 * ea, 0.0 * ea, qb) if i == 0 else (ea, 0.0 * ea, qa) if i == 1 else (rec["e"], rec["f"], rec["q"])
            x = q - e.unsqueeze(-1) * x1 - f.unsqueeze(-1) * x2
            until = torch.where(rec["u"] > 0, torch.zeros_like(until), (until + 1).clamp(max=far))
            emit(i, torch.where(ok.unsqueeze(-1), x, torch.zeros_like(x)), rec, torch.minimum(rec["since"], until), ok)
            x2, x1 = x1, x

    def write(out, row, s, x, rec, gap, ok):
        zero = torch.zeros(N, J, dtype=torch.float64)
        out["pose"][:, row] = x
        out["valid"][:, row] = ok & (gap <= max_gap)
        out["residual"][:, row] = torch.where(ok & (rec["u"] > 0), torch.sqrt(((x - rec["z"]) ** 2).sum(-1)), zero)
        out["weight"][:, row] = torch.where(ok, rec["u"], zero)
        out["frame"][:, row] = s

    for t in range(T):
        if t >= 2:                                                                     # row t - 2 is final
            a, b, c = _coefficients(t - 2, 2, lv, la)
            old = pend.pop(0)
            e, f, q = chain.step(a + old["u"], b, c, old["u"].unsqueeze(-1) * old["z"])
            if lag > 0:
                ring[(t - 2) % lag] = dict(old, e=e, f=f, q=q)
        before = seen
        since = torch.where(w[:, t] > 0, torch.zeros_like(since), (since + 1).clamp(max=far))
        pend.append({"u": w[:, t].clone(), "z": z[:, t], "since": since})
        seen = (seen + (w[:, t] > 0)).clamp(max=2)
        ea, qa, qb = boundary(t + 1, gate > 0, before)
        if t >= lag:
            substitute(t + 1, ea, qa, qb, lag + 1,
                       lambda i, x, rec, gap, ok: write(steps, t, t - lag, x, rec, gap, ok) if i == lag else None)
    if T >= 1 and lag > 0:
        ea, qa, qb = boundary(T, False, None)
        substitute(T, ea, qa, qb, lag, lambda i, x, rec, gap, ok: write(tail, lag - 1 - i, T - 1 - i, x, rec, gap, ok))
    return steps, tail

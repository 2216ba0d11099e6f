"""Float64 restatement of the orientation filter and the contact trust (mpcqp_attitude),
batched with NumPy: one tick of the gyro / accelerometer filter of doc/state_estimation_kf.md
(section 2, the document's first stage) and the stance-phase trust ramp for B robots, the
record's packing, the known-answer input builders and a seeded generator of test
trajectories.  The reference has no code for either, so there is no program to record a
fixture from: this restatement of the tick as include/mpcqp.h states it is the oracle,
checked against known answers (tests/test_att.py).  It is written as NumPy wants it (cross
products, a scalar-vector quaternion product, linalg norms), not in the kernel's order of
operations, so the two differ by rounding."""
import numpy as np

import kin_ref

STRIDE = 8              # MPCQP_ATT_STRIDE
Q, INIT, BIAS = slice(0, 4), 4, slice(5, 8)
STATUS_NONFINITE = 4
DEFAULTS = dict(dt=0.001, gravity=9.81, kappa_ref=0.1, bias_gain=0.0, trust_window=0.2, touch_threshold=0.0)
# name: (period, stance offsets, stance durations); WRAP is a custom gait whose swing offset
# (offset + duration) passes the period for legs FL and RR
TROTTING10 = (10, (0, 5, 5, 0), (5, 5, 5, 5))
STANDING = (16, (0, 0, 0, 0), (16, 16, 16, 16))
WRAP = (10, (7, 2, 2, 7), (6, 6, 6, 6))
# csrc/mpcqp_attitude_robot.h compiled for the host against this restatement over
# make_trajectory(8, 400, seed=7): the record's largest norm-wise error (the quaternion taken
# up to sign) over ticks and robots, as tests/test_att.py measures and prints it -- the
# problem's rounding sensitivity d, from which tests/test_gpu_att.py takes its bound
D_Q = 5.6e-16


def gait_records(gaits):
    return np.array([[g[0], *g[1], *g[2]] for g in gaits], np.int32)


def quat_mul(p, q):
    """Hamilton product of [B,4] (w, x, y, z) quaternions."""
    pw, pv, qw, qv = p[:, :1], p[:, 1:], q[:, :1], q[:, 1:]
    return np.concatenate([pw * qw - np.sum(pv * qv, 1, keepdims=True), pw * qv + qw * pv + np.cross(pv, qv)], 1)


def quat_exp(theta):
    """[B,3] rotation vectors -> [B,4] unit quaternions; (1, theta / 2) below 1e-8."""
    t = np.linalg.norm(theta, axis=1, keepdims=True)
    small = t < 1e-8
    ts = np.where(small, 1.0, t)
    return np.where(small, np.concatenate([np.ones_like(t), 0.5 * theta], 1),
                    np.concatenate([np.cos(0.5 * ts), np.sin(0.5 * ts) * theta / ts], 1))


def up(q):
    """R(q)^T e_z [B,3]: the third row of kin_ref.quat2matrix_eigen."""
    return kin_ref.quat2matrix_eigen(q)[:, 2, :]


def gate(accel, gravity=9.81):
    """gamma [B] = clamp(1 - | |a| - g | / g, 0, 1), 0 for a = 0."""
    n = np.linalg.norm(np.asarray(accel).astype(np.float64), axis=1)
    return np.where(n > 0, np.clip(1.0 - np.abs(n - gravity) / gravity, 0.0, 1.0), 0.0)


def as_was(state):
    """The record the outputs of a refused tick are formed from: identity if not initialised."""
    out = state.copy()
    fresh = state[:, INIT] == 0.0
    out[fresh] = 0.0
    out[fresh, 0] = 1.0
    return out


def tick_step(state, gyro, accel, constants=None):
    """One orientation tick.  state [B,STRIDE], gyro / accel [B,3] (float32 values).  Returns
    (new state, ok [B]); a robot with a non-finite gyro, accel or record value keeps its record."""
    c = dict(DEFAULTS, **(constants or {}))
    state = np.asarray(state, np.float64)
    w, a = np.asarray(gyro).astype(np.float64), np.asarray(accel).astype(np.float64)
    ok = np.isfinite(w).all(1) & np.isfinite(a).all(1) & np.isfinite(state).all(1)
    with np.errstate(all="ignore"):
        n = np.linalg.norm(a, axis=1, keepdims=True)
        m = np.where(n > 0, a / np.where(n > 0, n, 1.0), 0.0)
        # the first tick of a record: the shortest arc with zero yaw
        first = np.concatenate([1.0 + m[:, 2:3], m[:, 1:2], -m[:, 0:1], np.zeros_like(n)], 1)
        first = first / np.linalg.norm(first, axis=1, keepdims=True)
        first = np.where(m[:, 2:3] < -1.0 + 1e-12, [[0.0, 1.0, 0.0, 0.0]], first)
        first = np.where(n > 0, first, [[1.0, 0.0, 0.0, 0.0]])
        # a tick of an initialised record
        q, b = state[:, Q], state[:, BIAS]
        e = np.cross(m, up(q))
        gamma = gate(a, c["gravity"])[:, None]
        omega = w - b + c["kappa_ref"] * gamma * e
        nb = b - c["bias_gain"] * gamma * e * c["dt"]
        nq = quat_mul(q, quat_exp(omega * c["dt"]))
        nq = nq / np.linalg.norm(nq, axis=1, keepdims=True)
    fresh = (state[:, INIT] == 0.0)[:, None]
    new = np.concatenate([np.where(fresh, first, nq), np.ones_like(n), np.where(fresh, 0.0, nb)], 1)
    return np.where(ok[:, None], new, state), ok


def gait_trust(tick, ibm, gait, window=0.2):
    """tick [B], gait [B,9] -> trust [B,4] float64: 0 in swing (swing_ref.swing_state's
    integers), 1 for a leg that never swings, the ramp min(1, phi / w, (1 - phi) / w) in stance."""
    tick = np.asarray(tick, np.int64)[:, None]
    g = np.asarray(gait, np.int64)
    period, off, dur = g[:, :1], g[:, 1:5], g[:, 5:9]
    valid = (period > 0) & (ibm > 0)
    span = np.where(valid, ibm * period, 1)
    nsw = (period - dur) * ibm
    nst = dur * ibm
    cs = ((tick % span) - (off + dur) * ibm) % span
    swing = valid & (nsw > 0) & (cs >= 1) & (cs <= nsw)
    k = np.where(cs == 0, nst, cs - nsw)
    ramps = valid & (nsw > 0) & ~swing & (nst > 0) & (window > 0)
    with np.errstate(all="ignore"):
        phi = (k - 0.5) / np.where(nst > 0, nst, 1)
        ramp = np.minimum(1.0, np.minimum(phi / window, (1.0 - phi) / window)) if window > 0 else 1.0 + 0 * phi
    return np.where(swing, 0.0, np.where(ramps, ramp, 1.0))


def attitude_step(state, inputs, constants=None):
    """One launch.  state [B,STRIDE]; inputs: gyro, accel [B,3] and optionally tick [B], gait
    [B,9] with ibm, and touch [B,4].  Returns (new state, dict(quat [B,4], gyro_out [B,3],
    trust [B,4] or None, status [B])), float64 (status int32)."""
    c = dict(DEFAULTS, **(constants or {}))
    state = np.asarray(state, np.float64)
    B = state.shape[0]
    new, ok = tick_step(state, inputs["gyro"], inputs["accel"], c)
    touch = inputs.get("touch")
    touch_ok = np.ones(B, bool)
    if touch is not None:
        touch = np.asarray(touch).astype(np.float64)
        touch_ok = np.isfinite(touch).all(1)
    ok = ok & touch_ok
    new = np.where(ok[:, None], new, state)
    src = np.where(ok[:, None], new, as_was(state))
    trust = None
    if inputs.get("gait") is not None or touch is not None:
        trust = np.ones((B, 4))
        if inputs.get("gait") is not None:
            trust = gait_trust(inputs["tick"], int(inputs["ibm"]), inputs["gait"], c["trust_window"])
        if touch is not None:
            with np.errstate(invalid="ignore"):
                trust = np.where(touch > c["touch_threshold"], trust, 0.0)
            trust = np.where(touch_ok[:, None], trust, 0.0)
    with np.errstate(invalid="ignore"):
        gyro_out = np.asarray(inputs["gyro"]).astype(np.float64) - src[:, BIAS]
    return new, dict(quat=src[:, Q].copy(), gyro_out=gyro_out, trust=trust,
                     status=np.where(ok, 0, STATUS_NONFINITE).astype(np.int32))


def seeded(quat, bias=None):
    """Records [B,STRIDE] initialised with quat [B,4] (and bias [B,3])."""
    quat = np.atleast_2d(np.asarray(quat, np.float64))
    rec = np.zeros((quat.shape[0], STRIDE))
    rec[:, Q], rec[:, INIT] = quat, 1.0
    if bias is not None:
        rec[:, BIAS] = bias
    return rec


def run(traj, constants=None, state=None, keys=("tick", "gait", "ibm", "touch")):
    """Every tick of a trajectory: ([T+1,B,STRIDE] records with the start first, list of
    outputs).  `keys`: which of the optional inputs are passed on."""
    B = traj[0]["gyro"].shape[0]
    state = np.zeros((B, STRIDE)) if state is None else state
    states, outs = [state], []
    for inp in traj:
        state, out = attitude_step(state, select(inp, keys), constants)
        states.append(state)
        outs.append(out)
    return np.stack(states), outs


def select(inp, keys):
    return {k: v for k, v in inp.items() if k in ("gyro", "accel") or k in keys}


def norm_err(a, ref):
    return kin_ref.norm_err(a, ref)


def record_err(rec, ref):
    """Norm-wise error of one record [STRIDE], the quaternion taken up to sign (q and -q are
    one rotation, and the sign is not canonicalised)."""
    flip = np.asarray(rec, np.float64).copy()
    flip[Q] = -flip[Q]
    return min(norm_err(rec, ref), norm_err(flip, ref))


def quat_err(q, ref):
    q = np.asarray(q, np.float64)
    return min(norm_err(q, ref), norm_err(-q, ref))


# ---- the known answers of tests/test_att.py, shared with the device tests

def rotvec_matrix(r):
    """exp([r]x) by Rodrigues' formula, [3,3]."""
    r = np.asarray(r, np.float64)
    t = np.linalg.norm(r)
    K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]) / t
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def known_tilt(B=1):
    """(a): from identity, zero gyro, accel = float32(R_t^T (0, 0, g)), kappa_ref 50, dt 0.002,
    400 ticks: R^T e_z converges to a / |a|."""
    a = np.float32(rotvec_matrix([0.3, -0.4, 0.2]).T @ [0, 0, 9.81])
    return dict(state=seeded(np.tile([1.0, 0, 0, 0], (B, 1))), gyro=np.zeros((B, 3), np.float32),
                accel=np.tile(a, (B, 1)), constants=dict(kappa_ref=50.0, dt=0.002), ticks=400)


def known_gyro_only(B=1):
    """(b): rate 1.7 rad/s about (1, 2, -2) / 3, accel of norm 2.5 g (gamma = 0), 500 ticks of
    0.002 s from identity: q is the closed-form exponential of the float32 rate."""
    w = np.float32(1.7 * np.array([1.0, 2.0, -2.0]) / 3.0)
    a = np.float32([0.0, 0.0, 2.5 * 9.81])
    angle = w.astype(np.float64) * (500 * 0.002)
    return dict(state=seeded(np.tile([1.0, 0, 0, 0], (B, 1))), gyro=np.tile(w, (B, 1)), accel=np.tile(a, (B, 1)),
                constants=dict(dt=0.002), ticks=500, answer=quat_exp(angle[None])[0])


def known_bias(B=1):
    """(d): level and at rest, a constant gyro reading (0.02, -0.03, 0) that is all bias,
    kappa_ref 20, bias_gain 40, dt 0.002, 20 000 ticks: b converges to it and the tilt to 0."""
    w = np.float32([0.02, -0.03, 0.0])
    return dict(state=seeded(np.tile([1.0, 0, 0, 0], (B, 1))), gyro=np.tile(w, (B, 1)),
                accel=np.tile(np.float32([0, 0, 9.81]), (B, 1)),
                constants=dict(kappa_ref=20.0, bias_gain=40.0, dt=0.002), ticks=20000, answer=w.astype(np.float64))


def make_trajectory(B, T, seed):
    """Seeded raw-sensor streams for T ticks of B robots: a list of T input dicts (gyro, accel,
    touch float32; tick, gait int32; ibm).  Smooth random body rates are integrated to a true
    orientation (kept in "truth"); gyro = rate + a constant bias + noise; accel =
    R^T (g e_z + a_lin) with a_lin a gentle sway, bursts that drive gamma to 0 and stretches
    that leave it inside (0, 1); the gaits TROTTING10, STANDING and WRAP alternate over the
    robots, every robot on a tick offset of its own; ibm is 20 on ticks 0-7, 16-23, ... and 1
    on the others; touch is mostly firm contact with drops to 0, faint and negative readings."""
    rng = np.random.default_rng(seed)
    f = np.float32
    dt = DEFAULTS["dt"]
    t = dt * np.arange(T)[:, None]
    ph = rng.uniform(0, 2 * np.pi, (B, 3))
    rate = np.stack([0.9 * np.cos(9 * t + ph[:, 0]), 0.6 * np.cos(7 * t + ph[:, 1]), 0.3 + 0.2 * np.sin(5 * t + ph[:, 2])], -1)
    rpy0 = rng.uniform([-0.3, -0.3, -1.0], [0.3, 0.3, 1.0], (B, 3))
    q = quat_exp(rpy0 * [1, 0, 0])
    q = quat_mul(quat_exp(rpy0 * [0, 0, 1]), quat_mul(quat_exp(rpy0 * [0, 1, 0]), q))
    bias = rng.uniform(-0.02, 0.02, (B, 3))
    kind = rng.integers(0, 10, (T, B))
    kind[0] = 9                                          # the first reading, which sets the start, is a quiet one
    sway = 0.4 * np.sin(11 * t[..., None] + ph[None])
    scale = np.where(kind == 0, 40.0, np.where(kind <= 3, 8.0, 1.0))[..., None]   # bursts, stretches, sway
    a_lin = sway * scale + (kind == 0)[..., None] * np.array([0.0, 0.0, 25.0])
    a_lin[0] = 0.0
    gait = gait_records([(TROTTING10, STANDING, WRAP)[b % 3] for b in range(B)])
    offset = rng.integers(0, 400, B)
    tkind = rng.integers(0, 12, (T, B, 4))
    touch = np.where(tkind == 0, 0.0, np.where(tkind == 1, 0.3, np.where(tkind == 2, -0.1, 1.0)))
    traj = []
    for i in range(T):
        R = kin_ref.quat2matrix_eigen(q)
        accel = np.einsum("bcr,bc->br", R, np.array([0.0, 0.0, DEFAULTS["gravity"]]) + a_lin[i])
        gyro = rate[i] + bias + 1e-3 * rng.standard_normal((B, 3))
        traj.append(dict(gyro=gyro.astype(f), accel=accel.astype(f), touch=touch[i].astype(f),
                         tick=(i + offset).astype(np.int32), gait=gait, ibm=20 if (i // 8) % 2 == 0 else 1,
                         truth=q.copy()))
        q = quat_mul(q, quat_exp(rate[i] * dt))
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
    return traj


# ---- edge inputs shared by tests/test_att.py (the header on the host) and
# tests/test_gpu_att_edges.py (the device)
TRUST_WINDOWS = (0.2, 0.0, 0.5, 1e-300)
G32 = np.float32(9.81)
# first tick: n = 0; straight down; still under the m_z < -1 + 1e-12 threshold in float64; just
# above it, where the shortest arc is nearly singular (twice); a subnormal; tiny; huge; sideways
FIRST_ACCEL = np.float32([[0, 0, 0], [0, 0, -9.81], [0, 1e-5, -9.81], [1e-3, 0, -9.81], [1e-2, 1e-2, -9.81],
                          [0, 0, 1e-44], [1e-30, 0, 0], [3e38, 0, 0], [9.81, 0, 0]])
# the gate: |a| = g, 2 g (float32(19.62) is just past it), beyond (gamma = 0: rows 2, 3), tiny, huge
GATE_ACCEL = np.float32([[0, 0, 9.81], [0, 0, 19.62], [0, 0, 19.63], [0, 0, 25], [1e-30, 0, 0], [3e38, 0, 0]])
GATE_CLOSED = (2, 3)
GATE_CONSTANTS = dict(kappa_ref=2.0)
TILT = np.array([0.96, 0.18, -0.2, 0.07]) / np.linalg.norm([0.96, 0.18, -0.2, 0.07])
# either side of |theta| = 1e-8 at dt = 1e-3, and 0
SWITCH_GYRO = np.float32([[0.9e-5, 0, 0], [1.1e-5, 0, 0], [0, 0, 0]])
LARGE_RATES = np.float32([1e3, 5e3, 2e4])       # |theta| up to 23 rad per tick at dt = 1e-3
HUGE_RATES = np.float32([1e6, 3e38])
SEED_NORMS = (2.0, 1e-3, 1e-160)
MISUSE_NORMS = (0.0, 1e150)


def rate_rows(w):
    w = np.asarray(w, np.float32)
    return np.stack([w, -w / np.float32(2), w / np.float32(4)], 1).astype(np.float32)


def trust_edges(ibm):
    """The leg controller's decision table (swing_ref.decision_edges) for one
    iterations_between_mpc, a robot per row: (tick [B] int32, gait [B,9] int32)."""
    import swing_ref
    rows = swing_ref.decision_edges()[ibm]
    return np.array([t for t, _ in rows], np.int32), np.stack([r for _, r in rows]).astype(np.int32)


def level(B):
    """gyro 0, accel (0, 0, g) for B robots."""
    return dict(gyro=np.zeros((B, 3), np.float32), accel=np.tile(np.float32([0, 0, 9.81]), (B, 1)))


def touch_at_threshold(threshold=0.25):
    """[3,4] float32: the threshold exactly, one float32 below, one above (the threshold is a
    float32 value, so the comparison in float64 is exact)."""
    t = np.float32(threshold)
    return np.stack([np.full(4, v, np.float32) for v in (t, np.nextafter(t, np.float32(-1)), np.nextafter(t, np.float32(1)))])

"""Float64 NumPy restatement of one leg-controller tick, batched over robots x legs:
what mpcqp_leg_torques computes (include/mpcqp.h), written from the math of the
reference's Gait.get_swing_state, SwingFootTrajectoryGenerator and LegController
(gait.py:102-121, swing_foot_trajectory_generator.py:38-129, leg_controller.py:75-90).
tests/test_swing.py pins it to the reference's recorded run (tests/golden/swing.npz);
the GPU tests use it where that fixture cannot reach (large batches, other
iterations_between_mpc, custom gaits)."""
import numpy as np

STRIDE = 32                                        # MPCQP_SWING_STRIDE
ARMED, REMAIN, INIT, FINAL = 0, 1, slice(2, 5), slice(5, 8)   # per-leg slots of swing_mem


def quat2matrix_f32(quat):
    """[B,4] (w, x, y, z) float32 -> [B,3,3] float32, every product and sum rounded to
    float32 (the reference's quat2matrix on a float32 quaternion)."""
    q = np.asarray(quat, np.float32)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    two = np.float32(2)
    ww, xx, yy, zz = w * w, x * x, y * y, z * z
    R = np.stack([((ww + xx) - yy) - zz, two * (x * y - w * z), two * (w * y + x * z),
                  two * (w * z + x * y), ((ww - xx) + yy) - zz, two * (y * z - w * x),
                  two * (x * z - w * y), two * (w * x + y * z), ((ww - xx) - yy) + zz], axis=1)
    return R.reshape(-1, 3, 3).astype(np.float32)


def swing_state(tick, ibm, gait):
    """tick [B], gait [B,9] -> (swing [B,4] bool, finished [B,4] bool, value [B,4]).

    The decisions are integer: a leg swings on the (period - dur) * ibm control
    iterations after its stance ends, the first of them excluded (swing state 0) and the
    one after the last included (swing state 1, "finished"); the swing offset wraps per
    leg.  The value is the reference's division on its float32 phase."""
    tick = np.asarray(tick, np.int64)[:, None]
    g = np.asarray(gait, np.int64)
    period, off, dur = g[:, :1], g[:, 1:5], g[:, 5:9]
    span = ibm * period
    nsw = (period - dur) * ibm
    c = tick % span
    cs = (c - (off + dur) * ibm) % span
    swing = (nsw > 0) & (cs >= 1) & (cs <= nsw)
    finished = swing & (cs == nsw)
    phase = (c / span).astype(np.float32).astype(np.float64)
    so = off / period + dur / period
    so = np.where(so > 1.0, so - (np.ceil(so) - 1.0), so)     # into [0, 1]: whole periods off, either way
    so = np.where(so < 0.0, so - np.floor(so), so)
    sd = 1.0 - dur / period
    s = phase - so
    s = np.where(s < 0.0, s + 1.0, s)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = s / sd
        v = np.where(v > 0.0, v, cs / np.maximum(nsw, 1))
    return swing, finished, np.where(swing, v, 0.0)


def curve(t_swing, cur, init, fin, swing_height):
    """The cubic Hermite through init, mid, final at the float32 breaks [0, T/2, T] with
    zero velocity at each; cur clamped to the breaks.  t_swing, cur [...];
    init, fin [..., 3] -> position, velocity [..., 3]."""
    t_swing = np.asarray(t_swing, np.float64)
    t1 = (t_swing / 2.0).astype(np.float32).astype(np.float64)
    t2 = t_swing.astype(np.float32).astype(np.float64)
    t = np.clip(cur, 0.0, t2)
    second = t >= t1
    h = np.where(second, t2 - t1, t1)
    x = np.where(second, t - t1, t)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(h > 0, x / h, 0.0)
        rate = np.where(h > 0, 6.0 * u * (1.0 - u) / h, 0.0)
    blend = (3.0 - 2.0 * u) * u * u
    mid = (init + fin) / 2.0
    mid[..., 2] = swing_height
    a = np.where(second[..., None], mid, init)
    d = np.where(second[..., None], fin - mid, mid - init)
    return a + d * blend[..., None], d * rate[..., None]


class SwingRef:
    """B robots' swing generators and leg controller.  ``mem`` [B,4,8] is swing_mem."""

    def __init__(self, B, dt_control=0.001, gravity=9.81, swing_height=0.1, kp=700.0, kd=20.0,
                 touchdown_z=-0.0255, vel_gain=0.03):
        self.B = B
        self.dt_control, self.gravity, self.swing_height = dt_control, gravity, swing_height
        self.touchdown_z, self.vel_gain = touchdown_z, vel_gain
        self.Kp = self._gain(kp)
        self.Kd = self._gain(kd)
        self.mem = np.zeros((B, 4, 8))

    def _gain(self, k):
        k = np.asarray(k, np.float64)
        if k.ndim <= 1:       # a scalar, or one scalar per robot
            return np.broadcast_to(k.reshape(-1, 1, 1), (self.B, 1, 1)) * np.eye(3)
        return np.broadcast_to(k, (self.B, 3, 3))

    def step(self, tick, ibm, gait, pos, vel, R, v_body, yaw_rate, thighs, pos_feet, foot_pos_base,
             foot_vel_base, jac, u0):
        """One control iteration.  R [B,3,3] is R_base.  Returns a dict of tau [B,12]
        float32, swing [B,4] bool, swing_state [B,4], pos_target / vel_target [B,4,3], cur [B,4]
        (the time the curve is asked for, -inf for a stance leg)."""
        f8 = np.float64
        pos, vel, R = np.asarray(pos, f8), np.asarray(vel, f8), np.asarray(R, f8)
        vb, yr = np.asarray(v_body, f8), np.asarray(yaw_rate, f8)
        th, pf = np.asarray(thighs, f8), np.asarray(pos_feet, f8)
        g = np.asarray(gait, np.int64)
        swing, finished, value = swing_state(tick, ibm, g)
        dt_mpc = self.dt_control * ibm
        t_swing = (dt_mpc * (g[:, 0] - g[:, 5]))[:, None]          # the first leg's duration
        t_stance = (dt_mpc * g[:, 5])[:, None]
        mem = self.mem
        first = mem[:, :, ARMED] == 0.0
        remaining = np.where(first, t_swing, mem[:, :, REMAIN] - self.dt_control)
        # foothold
        theta = yr[:, None] * 0.5 * t_stance
        ct, st = np.cos(theta), np.sin(theta)
        a = np.stack([ct * th[..., 0] - st * th[..., 1], st * th[..., 0] + ct * th[..., 1], th[..., 2]], axis=-1)
        a = a + vb[:, None, :] * remaining[..., None]
        Ra = np.einsum("brc,blc->blr", R, a)
        vdes = np.einsum("brc,bc->br", R, vb)
        fin = pos[:, None, :] + Ra + 0.5 * t_stance[..., None] * vel[:, None, :] \
            + self.vel_gain * (vel - vdes)[:, None, :]
        kc = 0.5 * pos[:, 2] / self.gravity
        fin[..., 0] += (kc * (vel[:, 1] * yr))[:, None]
        fin[..., 1] += (kc * (-vel[:, 0] * yr))[:, None]
        fin[..., 2] = self.touchdown_z
        init = np.where(first[..., None], pf, mem[:, :, INIT])
        # only legs in swing advance
        sw = swing[..., None]
        mem[:, :, REMAIN] = np.where(swing, remaining, mem[:, :, REMAIN])
        mem[:, :, INIT] = np.where(sw, init, mem[:, :, INIT])
        mem[:, :, FINAL] = np.where(sw, fin, mem[:, :, FINAL])
        mem[:, :, ARMED] = np.where(swing, np.where(finished, 0.0, 1.0), mem[:, :, ARMED])
        p, v = curve(t_swing, t_swing - remaining, init, fin, self.swing_height)
        pt = np.einsum("bcr,blc->blr", R, p - pos[:, None, :])      # R^T (p - pos_base)
        vt = np.einsum("bcr,blc->blr", R, v - vel[:, None, :])
        pt, vt = np.where(sw, pt, 0.0), np.where(sw, vt, 0.0)
        # torques
        rot = lambda x: np.einsum("brc,blc->blr", R, np.asarray(x, f8))
        ep = rot(pt) - rot(foot_pos_base)
        ev = rot(vt) - rot(foot_vel_base)
        e = np.einsum("brc,blc->blr", self.Kp, ep) + np.einsum("brc,blc->blr", self.Kd, ev)
        J = np.asarray(jac, f8)
        tau_sw = np.einsum("blcr,blc->blr", J, e)                    # J^T e
        tau_st = np.einsum("blcr,blc->blr", J, -np.asarray(u0, f8).reshape(-1, 4, 3))
        tau = np.where(sw, tau_sw, tau_st).reshape(-1, 12).astype(np.float32)
        cur = np.where(swing, t_swing - remaining, -np.inf)          # the curve's time, before its clamp
        return dict(tau=tau, swing=swing, swing_state=value, pos_target=pt, vel_target=vt, cur=cur)


def run_ref(inp, gait, ticks, ibm, mem0=None, **kw):
    """T ticks of B robots (make_inputs-style arrays, ticks [T,B]) through SwingRef(B, **kw)
    from the generator state mem0 [B,STRIDE] (default: zeros): arrays [T,B,...] and the
    final mem."""
    ticks = np.asarray(ticks)
    T, B = ticks.shape
    ref = SwingRef(B, **kw)
    if mem0 is not None:
        ref.mem[:] = np.asarray(mem0, np.float64).reshape(B, 4, 8)
    outs = []
    for t in range(T):
        outs.append(ref.step(ticks[t], ibm, gait, inp["pos"][t], inp["vel"][t], inp["rot"][t], inp["v_body"],
                             inp["yaw_rate"], inp["thighs"], inp["pos_feet"][t], inp["foot_pos_base"][t],
                             inp["foot_vel_base"][t], inp["jac"], inp["u0"]))
    o = {k: np.stack([x[k] for x in outs]) for k in outs[0]}
    o["mem"] = ref.mem.reshape(B, STRIDE).copy()
    return o


def norm_err(a, ref, eps=1e-12):
    """max|a - ref| / max(max|ref|, eps)."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(a - ref)) / max(float(np.max(np.abs(ref))), eps)) if ref.size else 0.0


# ---- the reference's recorded run (tests/golden/swing.npz, made by
# tests/golden/make_golden_swing.py) ------------------------------------------------

def load_fixture(name="swing.npz"):
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)
    return {k: v for k, v in np.load(path).items()}


def fixture_inputs(fx):
    """A fixture's inputs as make_inputs-style [T,B,...] arrays, R_base by the float32
    quat2matrix."""
    B, T = fx["tau"].shape[:2]
    tb = lambda a: np.ascontiguousarray(np.swapaxes(a, 0, 1))
    inp = {k: tb(fx[k]) for k in ("quat", "pos", "vel", "pos_feet", "foot_pos_base", "foot_vel_base")}
    inp["rot"] = quat2matrix_f32(inp["quat"].reshape(-1, 4)).reshape(T, B, 3, 3)
    for k in ("v_body", "yaw_rate", "thighs", "jac", "u0"):
        inp[k] = fx[k]
    return inp


def empty_sequence(fx):
    """The arrays a run of the fixture sequence fills: per tick tau, swing_state and the
    targets, and swing_mem [B,4,8] after every check_every-th tick."""
    B, T = fx["tau"].shape[:2]
    nck = fx["ck_first"].shape[1]
    return dict(tau=np.zeros((B, T, 12), np.float32), swing_state=np.zeros((B, T, 4)),
                pos_target=np.zeros((B, T, 4, 3)), vel_target=np.zeros((B, T, 4, 3)),
                ck_mem=np.zeros((B, nck, 4, 8)))


def compare_fixture(fx, seq):
    """Decisions exact, values norm-wise per robot: returns {quantity: [B] errors}.

    Gait.STANDING's reference swing state is 0 / 0 = nan at phase 0, which the
    reference's leg controller takes for a swing with zero targets; here such a leg is in
    stance (deviations), so those (robot, tick) entries are only checked to
    be stance and are left out of the value comparison."""
    ref_ss = fx["swing_state"]
    bad = np.isnan(ref_ss)
    assert not (seq["swing_state"][bad] != 0).any(), "a leg whose stance fills the period swings"
    ref_mask = np.where(bad, False, ref_ss > 0)
    assert np.array_equal(seq["swing_state"] > 0, ref_mask), "swing mask differs from the reference"
    armed = seq["ck_mem"][..., ARMED] != 0.0
    assert np.array_equal(~armed, fx["ck_first"]), "first-swing flags differ at the checkpoints"
    keep = ~bad.any(axis=2)                      # [B,T]
    errs = {}
    B = ref_ss.shape[0]
    # a generator that has never swung holds the reference's initial zeros / stale values
    # only where it has run: compare the latched state of legs that have swung at all
    ran = np.cumsum(ref_mask, axis=1)[:, ::int(fx["check_every"])] > 0    # [B,nck,4]
    for name, a, ref in (("tau", seq["tau"], fx["tau"]), ("swing_state", seq["swing_state"], ref_ss),
                         ("pos_target", seq["pos_target"], fx["pos_target"]),
                         ("vel_target", seq["vel_target"], fx["vel_target"])):
        errs[name] = np.array([norm_err(a[b][keep[b]], ref[b][keep[b]]) for b in range(B)])
    for name, a, ref in (("remaining", seq["ck_mem"][..., REMAIN], fx["ck_remaining"]),
                         ("init", seq["ck_mem"][..., INIT], fx["ck_init"]),
                         ("final", seq["ck_mem"][..., FINAL], fx["ck_final"])):
        errs[name] = np.array([norm_err(a[b][ran[b]], ref[b][ran[b]]) for b in range(B)])
    return errs


def make_inputs(B, T, seed, tilt=None, vz=None, yaw=None, thigh_z=None):
    """Seeded float32 kinematic inputs for T ticks of B robots (arrays [T,B,...]; the
    per-robot constants [B,...]): a wobbling, yawing base, moving feet, a random
    Jacobian and contact forces per robot.

    tilt, vz, yaw, thigh_z: (lo, hi) magnitudes, each with a random sign, that replace the
    base's mean roll and pitch (default within 0.15), the commanded body z velocity
    (default 0), the commanded yaw rate (default within 0.8) and the thighs' z (default 0;
    per leg different) -- none of them near 0, so that every robot's torques depend on the
    terms they feed.  They are drawn from a stream of their own: the other arrays are
    those of the defaults."""
    rng = np.random.default_rng(seed)
    rng2 = np.random.default_rng([seed, 1])
    signed = lambda r, *size: rng2.uniform(r[0], r[1], size) * rng2.choice([-1.0, 1.0], size)
    f4 = np.float32
    t = np.arange(T)[:, None]
    rpy0 = rng.uniform([-0.15, -0.15, -3.1], [0.15, 0.15, 3.1], (B, 3))
    if tilt is not None:
        rpy0[:, :2] = signed(tilt, B, 2)
    rpy = rpy0[None] + np.stack(
        [0.05 * np.sin(0.3 * t + np.zeros(B)), 0.04 * np.cos(0.2 * t + np.zeros(B)), 0.02 * t + np.zeros(B)], -1)
    c, s = np.cos(rpy / 2), np.sin(rpy / 2)
    cr, cp, cy, sr, sp, sy = c[..., 0], c[..., 1], c[..., 2], s[..., 0], s[..., 1], s[..., 2]
    quat = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy,
                     cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], -1).astype(f4)
    v_body = np.stack([rng.uniform(-0.5, 1.5, B), rng.uniform(-0.4, 0.4, B),
                       np.zeros(B) if vz is None else signed(vz, B)], 1)
    pos = (np.stack([rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), np.full(B, 0.38)], 1)[None]
           + 0.001 * t[..., None] * v_body[None] + np.stack([0 * t, 0 * t, 0.01 * np.sin(0.4 * t)], -1)).astype(f4)
    vel = (v_body[None] + rng.uniform(-0.3, 0.3, (T, B, 3))).astype(f4)
    sign = np.array([[1, 1], [1, -1], [-1, 1], [-1, -1]], float)
    thighs = np.tile(np.c_[0.24 * sign[:, 0], 0.134 * sign[:, 1], np.zeros(4)], (B, 1, 1))
    if thigh_z is not None:
        thighs[..., 2] = signed(thigh_z, B, 4)
    thighs = thighs.astype(f4)
    ph = rng.uniform(0, 6.28, (B, 4, 3))
    tt = t[..., None]
    foot_pos_base = (thighs[None] + np.stack([0.08 * np.sin(0.15 * tt + ph[None, ..., 0]),
                                              0.03 * np.cos(0.1 * tt + ph[None, ..., 1]),
                                              -0.32 + 0.04 * np.sin(0.2 * tt + ph[None, ..., 2])], -1)).astype(f4)
    R = quat2matrix_f32(quat.reshape(-1, 4)).reshape(T, B, 3, 3)
    pos_feet = (pos[:, :, None, :] + np.einsum("tbrc,tblc->tblr", R, foot_pos_base)).astype(f4)
    yaw_rate = rng.uniform(-0.8, 0.8, B)
    if yaw is not None:
        yaw_rate = signed(yaw, B)
    return dict(quat=quat, pos=pos, vel=vel, rot=R, v_body=v_body, yaw_rate=yaw_rate,
                thighs=thighs, pos_feet=pos_feet, foot_pos_base=foot_pos_base,
                foot_vel_base=rng.uniform(-1, 1, (T, B, 4, 3)).astype(f4),
                jac=rng.standard_normal((B, 4, 3, 3)).astype(f4), u0=rng.uniform(-40, 120, (B, 12)).astype(f4))


def root_states(quat, pos, vel):
    """Isaac Gym actor root states [..., 13]: pos, quat (x, y, z, w), lin_vel, ang_vel."""
    return np.concatenate([pos, quat[..., 1:4], quat[..., 0:1], vel, np.zeros_like(pos)], -1).astype(np.float32)


# ---- everything off its default at once (tests/test_gpu_swing_edges.py; tests/test_swing.py
# checks on the CPU that each of these moves every robot's torques) --------------------------

# full, non-symmetric gains: nine distinct entries each, off-diagonals >= 10 % of the diagonal
EDGE_KP = np.array([[610.0, 95.0, -120.0], [-78.0, 540.0, 140.0], [160.0, -90.0, 720.0]])
EDGE_KD = np.array([[18.0, 3.2, -2.4], [-4.1, 15.0, 2.9], [3.6, -2.7, 22.0]])
EDGE_CONSTS = dict(dt_control=0.0025, gravity=3.72, swing_height=0.06, touchdown_z=0.031, vel_gain=0.11)
EDGE_RANGES = dict(tilt=(0.2, 0.35), vz=(0.3, 0.6), yaw=(1.0, 2.5), thigh_z=(0.02, 0.08))
EDGE_IBM = 2
# 10-segment records: the two Gait members and one with per-leg different durations whose
# second leg's swing offset passes the period
EDGE_GAITS = ((10, (0, 5, 5, 0), (5, 5, 5, 5)), (10, (5, 0, 5, 0), (5, 5, 5, 5)), (10, (0, 7, 5, 2), (5, 6, 5, 3)))


def edge_case(B, seed=None):
    """B robots with everything the default inputs leave at zero or at its default switched
    on: thigh z, commanded z velocity, large yaw rate and tilt (EDGE_RANGES), the records
    EDGE_GAITS in turn at iterations_between_mpc = 2 (a swing lasts 6 to 14 calls) and every
    tick from -1 + (b % 5) for 26 calls: each leg runs one whole swing with the tick before
    it, its finishing tick and the re-arm after it.  Returns (inp, gait [B,9], ticks [T,B])."""
    T = 26
    inp = make_inputs(B, T, seed=300 + B if seed is None else seed, **EDGE_RANGES)
    gait = np.array([[g[0], *g[1], *g[2]] for g in (EDGE_GAITS[b % len(EDGE_GAITS)] for b in range(B))], np.int32)
    ticks = np.arange(-1, T - 1)[:, None] + (np.arange(B) % 5)[None]
    return inp, gait, ticks


def edge_one_tick(B, tick, seed):
    """Edge inputs for one call of B robots, the records EDGE_GAITS in turn, every generator
    70 % through a swing (all three records swing for 0.025 s under EDGE_CONSTS): a first
    call from zeros would evaluate the curve at its start, where the foothold -- and with it
    gravity, touchdown_z, vel_gain, thigh z -- has no say.  Returns (inp, gait [B,9],
    ticks [1,B], mem0 [B,STRIDE])."""
    inp = make_inputs(B, 1, seed=seed, **EDGE_RANGES)
    mem0 = np.zeros((B, 4, 8))
    mem0[..., ARMED], mem0[..., REMAIN] = 1.0, 0.3 * 0.025 + EDGE_CONSTS["dt_control"]
    mem0[..., INIT] = inp["pos_feet"][0].astype(np.float64) + np.array([-0.02, 0.01, 0.0])
    gait = np.array([[g[0], *g[1], *g[2]] for g in (EDGE_GAITS[b % len(EDGE_GAITS)] for b in range(B))], np.int32)
    return inp, gait, np.full((1, B), tick), mem0.reshape(B, STRIDE)


# ---- tick and record edges of the swing decision (tests/test_swing.py on the g++ build,
# tests/test_gpu_swing_edges.py on the device) ----------------------------------------------

def decide_exact(tick, ibm, rec, leg):
    """(swing, finished, cs, nsw) of one leg in Python's unbounded integers -- no NumPy, no
    fixed width, nothing shared with swing_state above.  include/mpcqp.h: a leg swings for
    1 <= cs <= nsw, cs = (tick mod span) shifted by the leg's swing offset (off + dur) * ibm,
    nsw = (period - dur) * ibm, span = ibm * period; never for a malformed record
    (period <= 0) or a leg whose stance fills the period (nsw <= 0)."""
    tick, ibm, period, off, dur = int(tick), int(ibm), int(rec[0]), int(rec[1 + leg]), int(rec[5 + leg])
    if period <= 0:
        return False, False, 0, 0
    span = ibm * period
    nsw = (period - dur) * ibm
    if nsw <= 0:
        return False, False, 0, nsw
    cs = ((tick % span) - (off + dur) * ibm) % span          # Python's % is never negative here
    swing = 1 <= cs <= nsw
    return swing, swing and cs == nsw, cs, nsw


def decision_edges():
    """{ibm: [(tick, record[9])]}: every record of the table at every tick of
    -2^31, -1, 0, span - 1, span, 2^31 - 1 that an int32 holds.  ibm = 2^20 with
    period = 2^11 makes span = 2^31, one past int32."""
    small = dict(
        period_1=(1, (0, 0, 0, 0), (0, 1, 0, 1)),
        dur_0=(10, (0, 3, 5, 9), (0, 5, 0, 5)),
        dur_is_period_on_leg_1=(10, (0, 5, 5, 0), (5, 10, 5, 5)),
        offset_wraps=(10, (0, 7, 5, 2), (5, 6, 5, 3)),
        negative_offset=(10, (-3, 5, -12, 0), (5, 5, 5, 5)),
        # malformed: durations chosen so that only the period check keeps them from swinging
        period_0=(0, (0, 5, 5, 0), (-2, -2, -2, -2)),
        period_minus_3=(-3, (0, 1, 1, 0), (-5, -5, -5, -5)))
    big = dict(
        period_1=small["period_1"],
        trot=(2048, (0, 1024, 1024, 0), (1024, 1024, 1024, 1024)),
        dur_0=(2048, (0, 3, 5, 9), (0, 1024, 0, 1024)),
        dur_is_period_on_leg_1=(2048, (0, 1024, 1024, 0), (1024, 2048, 1024, 1024)),
        offset_wraps=(2048, (0, 1500, 1024, 2), (1024, 1200, 1024, 3)),
        negative_offset=(2048, (-3, 1024, -2500, 0), (1024, 1024, 1024, 1024)),
        period_0=small["period_0"], period_minus_3=small["period_minus_3"])
    table = {}
    for ibm, recs in ((1, small), (20, small), (2 ** 20, big)):
        rows = []
        for period, off, dur in recs.values():
            span = ibm * (period if period > 0 else 10)
            for tick in (-2 ** 31, -1, 0, span - 1, span, 2 ** 31 - 1):
                if -2 ** 31 <= tick < 2 ** 31:
                    rows.append((tick, np.array([period, *off, *dur], np.int32)))
        table[ibm] = rows
    return table

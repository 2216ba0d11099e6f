"""Float64 NumPy restatement of one terrain-plane tick, batched over robots: what
mpcqp_terrain computes (include/mpcqp.h), written from RobotData.update_terrain_normal
(utils/robot_data.py:186-228) with the two deviations of DESIGN.md 4.4g -- the eigenvector is
numpy.linalg.eigh's column, and the first tick seeds the history with all four feet -- and the
accept-or-hold rules.  tests/test_terrain.py pins it to known answers and to the reference's
recorded run (tests/golden/terrain.npz); it is the oracle of tests/test_gpu_terrain.py.

Also GroundSwingRef, swing_ref.SwingRef on a ground plane (mpcqp_set_ground), and a seeded
generator of trajectories."""
import numpy as np

import swing_ref

STRIDE = 20                                          # MPCQP_TERRAIN_STRIDE
HIST, INIT, N, D, FITTED = slice(0, 12), 12, slice(13, 16), 16, 17
STATUS_OK, STATUS_NONFINITE = 0, 4
SWING_STATE, ROOT_STATES, GROUND = 1, 2, 4            # MPCQP_TERRAIN_SWING_STATE, _ROOT_STATES, _GROUND
TOUCHDOWN_Z = -0.0255                                # mpcqp_set_swing's default
DEFAULTS = dict(contact_threshold=0.5, flat_tol=1e-3, cos_max_tilt=0.5, blend=1.0)
TROT10 = np.array([10, 0, 5, 5, 0, 5, 5, 5, 5], np.int32)   # Gait.TROTTING10 (gait.py:17)

# The host-compiled header against this file over make_trajectory(8, 120, seed=11) and over
# GPU_TRAJECTORY: the largest difference of n (max norm; n is unit) and of d relative to
# max(1, |mu|), over ticks and robots, as tests/test_terrain.py::
# test_header_matches_the_restatement measures and prints it (1.11e-15 and 1.04e-15).  The
# device build of the same text is held to 10 D_N (tests/test_gpu_terrain.py).
D_N = 1.1e-15
GPU_TRAJECTORY = dict(B=131, T=24, seed=5)    # tests/test_gpu_terrain.py: 2 W + 3 robots, 24 ticks


def contact_decision(values, constants=None, swing_rule=False):
    """[B,4] float32 -> bool: value > contact_threshold (a NaN is no contact), or with
    swing_rule the leg controller's stance, not (swing_state > 0)."""
    c = dict(DEFAULTS, **(constants or {}))
    v = np.asarray(values, np.float32)
    with np.errstate(invalid="ignore"):
        return ~(v > 0) if swing_rule else v.astype(np.float64) > c["contact_threshold"]


def as_was(state):
    """The records the outputs of refused robots are formed from."""
    out = np.array(state, np.float64)
    cold = out[:, INIT] == 0.0
    out[cold] = 0.0
    out[cold, 15] = 1.0
    return out


def fit(hist):
    """hist [B,4,3] -> mu [B,3], l [B,3] ascending, n_fit [B,3] with n_z >= 0."""
    mu = hist.mean(axis=1)
    X = hist - mu[:, None, :]
    S = np.einsum("bir,bis->brs", X, X)
    l, V = np.linalg.eigh(S)
    n = V[:, :, 0].copy()                      # the column of the smallest eigenvalue
    n[n[:, 2] < 0] *= -1.0
    return mu, l, n


def tick_step(state, feet, contact, constants=None):
    """One tick.  state [B,20] float64, feet [B,4,3] float32, contact [B,4] bool ->
    (state after the tick [B,20], ok [B]); a refused robot keeps its record."""
    c = dict(DEFAULTS, **(constants or {}))
    st = np.array(state, np.float64)
    B = st.shape[0]
    f = np.asarray(feet, np.float32).astype(np.float64).reshape(B, 4, 3)
    cont = np.asarray(contact, bool)
    init = st[:, INIT] != 0.0
    take = cont | ~init[:, None]
    ok = np.where(init, np.isfinite(st).all(axis=1), True)
    ok &= (np.isfinite(f).all(axis=2) | ~take).all(axis=1)
    hist = np.where(take[..., None], f, st[:, HIST].reshape(B, 4, 3))
    hist = np.where(ok[:, None, None], hist, 0.0)
    n_old = np.where(init[:, None], st[:, N], [0.0, 0.0, 1.0])
    mu, l, nf = fit(hist)
    fitted = (l[:, 2] > 0) & (l[:, 1] - l[:, 0] > c["flat_tol"] * l[:, 2]) & (nf[:, 2] >= c["cos_max_tilt"])
    nb = (1.0 - c["blend"]) * n_old + c["blend"] * nf
    ln = np.linalg.norm(nb, axis=1)
    fitted &= ln > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.where(fitted[:, None], nb / ln[:, None], n_old)
    new = np.zeros_like(st)
    new[:, HIST] = hist.reshape(B, 12)
    new[:, INIT] = 1.0
    new[:, N] = n
    new[:, D] = np.einsum("bk,bk->b", n, mu)
    new[:, FITTED] = fitted
    return np.where(ok[:, None], new, st), ok


def ground_plane(n, d, touchdown_z=TOUCHDOWN_Z):
    """The plane handed to the swing leg under MPCQP_TERRAIN_GROUND, [B,4] float32: the swing leg
    places a foothold at touchdown_z + ground(x, y), so (n, d - n_z touchdown_z) puts it on
    n . p = d, the plane through the latched foot centres."""
    n, d = np.asarray(n, np.float64), np.asarray(d, np.float64)
    return np.concatenate([n, (d - n[:, 2] * touchdown_z)[:, None]], axis=1).astype(np.float32)


def terrain_step(state, inp, constants=None, ground=False, touchdown_z=TOUCHDOWN_Z):
    """A launch: inp has pos_feet, contact or swing_state, optionally quat (or root_states)
    and robot [B,16].  Returns (state, outputs): normal, plane, normal_base (with a
    quaternion), status, robot (with a robot) as the kernel stores them.  ``ground``:
    MPCQP_TERRAIN_GROUND, plane is ground_plane(n, d, touchdown_z)."""
    swing_rule = "swing_state" in inp
    cont = contact_decision(inp["swing_state"] if swing_rule else inp["contact"], constants, swing_rule)
    new, ok = tick_step(state, inp["pos_feet"], cont, constants)
    src = np.where(ok[:, None], new, as_was(state))
    out = dict(normal=src[:, N].astype(np.float32),
               plane=ground_plane(src[:, N], src[:, D], touchdown_z) if ground
               else np.concatenate([src[:, N], src[:, D:D + 1]], axis=1).astype(np.float32),
               status=np.where(ok, STATUS_OK, STATUS_NONFINITE).astype(np.int32))
    quat = None
    if inp.get("root_states") is not None:
        quat = np.asarray(inp["root_states"], np.float32)[:, [6, 3, 4, 5]]
    elif inp.get("quat") is not None:
        quat = np.asarray(inp["quat"], np.float32)
    if quat is not None:
        R = swing_ref.quat2matrix_f32(quat).astype(np.float64)
        out["normal_base"] = np.einsum("bcr,bc->br", R, src[:, N]).astype(np.float32)
    if inp.get("robot") is not None:
        rob = np.array(inp["robot"], np.float32)
        rob[:, 9:12] = out["normal"]
        out["robot"] = rob
    return new, out


def run(traj, constants=None, swing_rule=True, state0=None, **kw):
    """make_trajectory's ticks through terrain_step from zero records: states [T,B,20] and
    the outputs stacked [T,B,...]."""
    B = traj[0]["pos_feet"].shape[0]
    st = np.zeros((B, STRIDE)) if state0 is None else np.array(state0, np.float64)
    states, outs = [], []
    for t in traj:
        inp = dict(pos_feet=t["pos_feet"], quat=t["quat"])
        inp["swing_state" if swing_rule else "contact"] = t["swing_state"] if swing_rule else t["contact"]
        st, o = terrain_step(st, inp, constants, **kw)
        states.append(st)
        outs.append(o)
    return np.stack(states), {k: np.stack([o[k] for o in outs]) for k in outs[0]}


def spread(hist):
    """(l1 - l0) / l2 of the history's scatter, [B]."""
    _, l, _ = fit(np.asarray(hist, np.float64).reshape(-1, 4, 3))
    return (l[:, 1] - l[:, 0]) / l[:, 2]


def make_trajectory(B, T, seed, ibm=2, flat_tol=DEFAULTS["flat_tol"]):
    """T ticks of B robots walking a trot (TROT10 at iterations_between_mpc = ibm) on planes:
    a list of dicts with pos_feet [B,4,3] float32, swing_state / contact [B,4] float32 (contact
    = 1 in stance), quat [B,4] float32, tick, and the true unit normal `n_true` [B,3].

    The planes are tilted 0 .. 0.9 rad (robot 0 exactly level) at any azimuth, the bases stand
    out to +-50 m at any yaw and move, positions are rounded to float32, and each foot's z
    carries noise of 1e-6 .. 1e-2 m (a magnitude per robot, log-uniform).  Asserted here:
    every tick's history has (l1 - l0) / l2 >= 0.05, which also keeps it a factor 2 and more
    off flat_tol, so that a rounding difference cannot flip a decision."""
    rng = np.random.default_rng(seed)
    tilt = rng.uniform(0.0, 0.9, B)
    tilt[0] = 0.0
    if B > 1:
        tilt[1] = 0.9
    az = rng.uniform(-np.pi, np.pi, B)
    n_true = np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], axis=1)
    d_true = rng.uniform(-5.0, 5.0, B)
    base0 = rng.uniform(-50.0, 50.0, (B, 2))
    yaw0 = rng.uniform(-np.pi, np.pi, B)
    speed = rng.uniform(-0.5, 0.5, (B, 2))
    noise = 10.0 ** rng.uniform(-6.0, -2.0, B)
    corners = np.array([[0.2, 0.13], [0.2, -0.13], [-0.2, 0.13], [-0.2, -0.13]])   # FL, FR, RL, RR
    gait = np.tile(TROT10, (B, 1))
    traj = []
    state = np.zeros((B, STRIDE))
    for t in range(T):
        yaw = yaw0 + 0.002 * t
        cy, sy = np.cos(yaw), np.sin(yaw)
        rot = np.stack([np.stack([cy, -sy], -1), np.stack([sy, cy], -1)], axis=1)        # [B,2,2]
        xy = base0[:, None, :] + 0.004 * t * speed[:, None, :] + np.einsum("brc,lc->blr", rot, corners)
        xy = xy + rng.uniform(-0.01, 0.01, (B, 4, 2))
        z = (d_true[:, None] - n_true[:, None, 0] * xy[..., 0] - n_true[:, None, 1] * xy[..., 1]) / n_true[:, None, 2]
        z = z + noise[:, None] * rng.uniform(-1.0, 1.0, (B, 4))
        pos_feet = np.concatenate([xy, z[..., None]], axis=-1).astype(np.float32)
        tick = np.full(B, t, np.int32)
        swing, _, value = swing_ref.swing_state(tick, ibm, gait)
        half = 0.5 * yaw
        quat = np.stack([np.cos(half), 0.05 * np.sin(az), 0.05 * np.cos(az), np.sin(half)], axis=1)
        quat = (quat / np.linalg.norm(quat, axis=1, keepdims=True)).astype(np.float32)
        step = dict(pos_feet=pos_feet, swing_state=value.astype(np.float32),
                    contact=(~swing).astype(np.float32), quat=quat, tick=tick, n_true=n_true)
        state, ok = tick_step(state, pos_feet, ~swing, dict(flat_tol=flat_tol))
        ratio = spread(state[:, HIST])
        assert ok.all() and (ratio >= 0.05).all() and (ratio > 2.0 * flat_tol).all(), (t, ratio.min())
        traj.append(step)
    return traj


def norm_err(state, ref):
    """The largest difference of n (max norm) and of d relative to max(1, |mu|) between two
    sets of records [..., 20]."""
    a, r = np.asarray(state, np.float64).reshape(-1, STRIDE), np.asarray(ref, np.float64).reshape(-1, STRIDE)
    mu = np.linalg.norm(r[:, HIST].reshape(-1, 4, 3).mean(axis=1), axis=1)
    en = np.abs(a[:, N] - r[:, N]).max() if a.size else 0.0
    ed = (np.abs(a[:, D] - r[:, D]) / np.maximum(1.0, mu)).max() if a.size else 0.0
    return float(max(en, ed))


class GroundSwingRef(swing_ref.SwingRef):
    """SwingRef on a ground plane (include/mpcqp.h mpcqp_set_ground): ``ground`` [B,4] (n, d)
    per robot; a row that is non-finite or has n_z <= 0 is no plane.  A leg in swing places its
    foothold at z = touchdown_z + ground(fin) (swing_ref.py:125) and the apex of its curve at
    swing_height + (ground(init) + ground(fin)) / 2 (swing_ref.py:133)."""

    def __init__(self, B, ground=None, **kw):
        super().__init__(B, **kw)
        g = np.zeros((B, 4)) if ground is None else np.asarray(ground, np.float32).astype(np.float64)
        with np.errstate(invalid="ignore"):
            self.on = np.isfinite(g).all(axis=1) & (g[:, 2] > 0)
        self.ground = np.where(self.on[:, None], g, [0.0, 0.0, 1.0, 0.0])

    def set_ground(self, ground):
        """Another set of planes [B,4], as a caller's write into the buffer of mpcqp_set_ground."""
        g = np.asarray(ground, np.float32).astype(np.float64)
        with np.errstate(invalid="ignore"):
            self.on = np.isfinite(g).all(axis=1) & (g[:, 2] > 0)
        self.ground = np.where(self.on[:, None], g, [0.0, 0.0, 1.0, 0.0])

    def height(self, p):
        """ground(x, y) of p [B,4,3] -> [B,4]; 0 without a plane."""
        g = self.ground[:, None, :]
        return (g[..., 3] - g[..., 0] * p[..., 0] - g[..., 1] * p[..., 1]) / g[..., 2]

    def step(self, tick, ibm, gait, pos, vel, R, v_body, yaw_rate, thighs, pos_feet, foot_pos_base,
             foot_vel_base, jac, u0):
        f8 = np.float64
        pos, vel, R = np.asarray(pos, f8), np.asarray(vel, f8), np.asarray(R, f8)
        vb, yr = np.asarray(v_body, f8), np.asarray(yaw_rate, f8)
        th, pf = np.asarray(thighs, f8), np.asarray(pos_feet, f8)
        g = np.asarray(gait, np.int64)
        swing, finished, value = swing_ref.swing_state(tick, ibm, g)
        dt_mpc = self.dt_control * ibm
        t_swing = (dt_mpc * (g[:, 0] - g[:, 5]))[:, None]
        t_stance = (dt_mpc * g[:, 5])[:, None]
        mem = self.mem
        ARMED, REMAIN, INIT_, FINAL = swing_ref.ARMED, swing_ref.REMAIN, swing_ref.INIT, swing_ref.FINAL
        first = mem[:, :, ARMED] == 0.0
        remaining = np.where(first, t_swing, mem[:, :, REMAIN] - self.dt_control)
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
        init = np.where(first[..., None], pf, mem[:, :, INIT_])
        on = self.on[:, None]
        gf, gi = self.height(fin), self.height(init)
        fin[..., 2] = np.where(on, self.touchdown_z + gf, self.touchdown_z)
        apex = np.where(on, self.swing_height + (gi + gf) / 2.0, self.swing_height)
        sw = swing[..., None]
        mem[:, :, REMAIN] = np.where(swing, remaining, mem[:, :, REMAIN])
        mem[:, :, INIT_] = np.where(sw, init, mem[:, :, INIT_])
        mem[:, :, FINAL] = np.where(sw, fin, mem[:, :, FINAL])
        mem[:, :, ARMED] = np.where(swing, np.where(finished, 0.0, 1.0), mem[:, :, ARMED])
        p, v = swing_ref.curve(t_swing, t_swing - remaining, init, fin, apex)
        pt = np.einsum("bcr,blc->blr", R, p - pos[:, None, :])
        vt = np.einsum("bcr,blc->blr", R, v - vel[:, None, :])
        pt, vt = np.where(sw, pt, 0.0), np.where(sw, vt, 0.0)
        rot = lambda x: np.einsum("brc,blc->blr", R, np.asarray(x, f8))
        ep = rot(pt) - rot(foot_pos_base)
        ev = rot(vt) - rot(foot_vel_base)
        e = np.einsum("brc,blc->blr", self.Kp, ep) + np.einsum("brc,blc->blr", self.Kd, ev)
        J = np.asarray(jac, f8)
        tau_sw = np.einsum("blcr,blc->blr", J, e)
        tau_st = np.einsum("blcr,blc->blr", J, -np.asarray(u0, f8).reshape(-1, 4, 3))
        tau = np.where(sw, tau_sw, tau_st).reshape(-1, 12).astype(np.float32)
        cur = np.where(swing, t_swing - remaining, -np.inf)
        return dict(tau=tau, swing=swing, swing_state=value, pos_target=pt, vel_target=vt, cur=cur)


# ---- the closed loop with the terrain stage: plant -> controller -> terrain -> controller on the
# CPU oracles (plant_ref.closed_loop with plane= and terrain=), recorded in
# tests/golden/terrain_loop.npz by tests/golden/make_golden_terrain_loop.py

LOOP = dict(robot="aliengo", gait="trot10", horizon=10, ibm=20)
LOOP_TICKS = 800
# (name, tilt in rad, the compass direction in which the ground climbs in degrees (0: ahead of
# the robot), forward command in m/s, start).  start "ground": the stand pose with its feet on
# the plane, the premise of the stage (a latched stance foot is a sample of the ground); "drop":
# plant_ref.closed_loop's own start at the preset's height, the feet 0.023 m in the air.
LOOP_SCENARIOS = (("level, standing", 0.0, 0, 0.0, "ground"), ("level, 0.5 m/s", 0.0, 0, 0.5, "ground"),
                  ("uphill 0.1 rad, standing", 0.1, 0, 0.0, "ground"), ("uphill 0.1 rad, 0.3 m/s", 0.1, 0, 0.3, "ground"),
                  ("cross-slope 0.1 rad, 0.3 m/s", 0.1, 90, 0.3, "ground"),
                  ("downhill 0.1 rad, 0.3 m/s", 0.1, 180, 0.3, "ground"),
                  ("uphill 0.2 rad, standing", 0.2, 0, 0.0, "ground"), ("uphill 0.2 rad, 0.3 m/s", 0.2, 0, 0.3, "ground"),
                  ("level, 0.5 m/s, dropped", 0.0, 0, 0.5, "drop"), ("uphill 0.1 rad, 0.3 m/s, dropped", 0.1, 0, 0.3, "drop"))
LOOP_LEVEL = (0, 1)                                          # the scenarios of the level-ground comparison
LOOP_FIGURES = ("height", "tilt", "speed", "normal", "foothold", "touchdown", "fitted")


def loop_planes(scenarios=LOOP_SCENARIOS, ground_z=TOUCHDOWN_Z):
    """[B,4] float32, the plant's ground per scenario: (n, ground_z), n = (-sin tilt cos az,
    -sin tilt sin az, cos tilt) (plant_ref.tilt_pose)."""
    tilt = np.array([s[1] for s in scenarios], np.float64)
    az = np.deg2rad(np.array([s[2] for s in scenarios], np.float64))
    n = np.stack([-np.sin(tilt) * np.cos(az), -np.sin(tilt) * np.sin(az), np.cos(tilt)], axis=1)
    n[np.abs(n) < 1e-16] = 0.0                               # sin(pi), cos(pi / 2)
    return np.concatenate([n, np.full((len(tilt), 1), ground_z)], axis=1).astype(np.float32)


def loop_heights(scenarios=LOOP_SCENARIOS, robot="aliengo", preset=0.38):
    """[B] float32: the base height of the level stand pose each scenario starts from, before
    plant_ref.tilt_pose turns it onto the plane."""
    import plant_ref
    params = plant_ref._presets()
    geom = params.pack_leg_geometry(params.LEG_GEOMETRY[robot], 1)
    on_ground = plant_ref.stand_pose(1, geom, plant_ref.Params())[0][0, 2]
    return np.array([on_ground if s[4] == "ground" else preset for s in scenarios], np.float32)


def closed_loop_terrain(scenarios=LOOP_SCENARIOS, stage=True, ground=True, ticks=LOOP_TICKS, constants=None):
    """plant_ref.closed_loop over the scenarios, one robot each: with the terrain stage (``ground``:
    under MPCQP_TERRAIN_GROUND) or without.  Returns the run with ``planes``."""
    import plant_ref
    planes = loop_planes(scenarios)
    run = plant_ref.closed_loop([s[3] for s in scenarios], ticks, plane=planes, terrain_ground=ground,
                                terrain=dict(constants or {}) if stage else None,
                                heights=loop_heights(scenarios, LOOP["robot"]), **LOOP)
    run["planes"] = planes
    return run


def clean_ticks(swing, touch):
    """swing [T,B,4] bool, touch [T,B,4] (the plant's, after the tick's step) -> [T,B] bool: every
    point of the history after the update of tick t was latched while its foot stood on the
    ground.  The stage latches by the schedule (~swing); a foot whose stance has begun by the
    schedule and that is still coming down -- it lands three ticks late in this loop -- is latched
    in the air, millimetres up, until it lands, and so is a foot that the seed tick takes in
    mid-air.  Whether it stood is the plant's touch after the step of tick t - 1, the pose that
    the pos_feet of tick t show (for tick 0 the pose it starts in: touch after reset is not
    logged, so a foot counts as standing where it touches after the first step and is in stance)."""
    touch = np.asarray(touch) != 0
    stance = ~np.asarray(swing, bool)
    before = np.concatenate([touch[:1], touch[:-1]], axis=0)
    ok = np.zeros(stance.shape, bool)
    ok[0] = before[0] & stance[0]
    for t in range(1, len(ok)):
        ok[t] = np.where(stance[t], before[t], ok[t - 1])
    return ok.all(axis=2)


def foothold_offsets(foothold, planes):
    """The vertical distance of every foothold [T,B,4,3] from the plant's plane [B,4]."""
    pl = np.asarray(planes, np.float32).astype(np.float64)[None, :, None, :]
    f = np.asarray(foothold, np.float64)
    return f[..., 2] - (pl[..., 3] - pl[..., 0] * f[..., 0] - pl[..., 1] * f[..., 1]) / pl[..., 2]


def loop_figures(run, height=0.38, last=500):
    """Per robot [B]:
      height, tilt, speed   plant_ref.summary's three: worst |height - desired|, worst roll /
                            pitch, mean forward speed along x over the last ticks
      start                 the first clean tick (clean_ticks): every foot latched on the ground
      clean                 the share of clean ticks from there on
      foothold              the worst vertical distance from the plant's plane of a swing leg's
                            foothold over the ticks t > start whose plane, the one the update of
                            tick t - 1 left, was clean
      touchdown             the same over the last tick of every swing that begins after start:
                            the foothold the leg comes down on
      foothold_any          the same over every swing tick after start, clean or not
    and with the stage
      normal                the largest difference (max norm) of the fitted normal, rounded to
                            float32, from the plane's float32 normal over the clean ticks
      normal_any            the same over every tick from start on
      fitted                the share of ticks with an accepted fit."""
    import plant_ref
    h, tilt, speed = plant_ref.summary(run, height=height, last=last)
    swing = np.asarray(run["swing"], bool)
    T, B = swing.shape[:2]
    clean = clean_ticks(swing, run["touch"])
    assert clean.any(axis=0).all()
    start = np.argmax(clean, axis=0)
    t = np.arange(T)[:, None]
    after = t > start[None, :]
    prev_clean = np.concatenate([np.zeros((1, B), bool), clean[:-1]], axis=0)
    off = np.abs(foothold_offsets(run["foothold"], run["planes"]))
    worst = lambda mask: np.where(mask, off, 0.0).max(axis=(0, 2))
    begins = swing & ~np.concatenate([np.zeros((1, B, 4), bool), swing[:-1]], axis=0)
    begun_after = np.zeros_like(swing)                        # in a swing that began after start
    for k in range(1, T):
        begun_after[k] = swing[k] & np.where(begins[k], after[k][:, None], begun_after[k - 1])
    ends = begun_after & ~np.concatenate([swing[1:], np.ones((1, B, 4), bool)], axis=0)
    assert ends.any(axis=(0, 2)).all()
    fig = dict(height=h, tilt=tilt, speed=speed, start=start,
               clean=np.array([clean[start[b]:, b].mean() for b in range(B)]),
               foothold=worst(swing & (after & prev_clean)[..., None]), touchdown=worst(ends),
               foothold_any=worst(swing & after[..., None]))
    if "plane" in run:
        n32 = run["plane"][:, :, :3].astype(np.float32).astype(np.float64)
        err = np.abs(n32 - run["planes"][None, :, :3].astype(np.float64)).max(axis=2)
        fig["normal"] = np.where(clean, err, 0.0).max(axis=0)
        fig["normal_any"] = np.where(t >= start[None, :], err, 0.0).max(axis=0)
        fig["fitted"] = run["fitted"].mean(axis=0)
    return fig

"""Float64 / integer NumPy restatement of the sensor model and of the push (mpcqp_sensors,
mpcqp_push, include/mpcqp_disturb_abi.h), batched over robots: Philox4x32-10 in unsigned
integers, Box-Muller and the tick in float64, the impulse on the plant's record.  The reference
has no such component (its scripts read a simulator's sensors as they come); this file is the
oracle of csrc/mpcqp_sensors_robot.h and of the kernels of csrc/mpcqp_sensors.h.

Record layout (STRIDE float64 words per robot): b_g 3, b_a 3, initialised, count, id, the four
feet's touch histories (integers below 2^32); words 13..15 are kept.
"""
import numpy as np

import plant_ref

STRIDE = 16                                          # MPCQP_SENSE_STRIDE
BIAS_G, BIAS_A, INIT, COUNT, ID, HIST, WORDS = 0, 3, 6, 7, 8, 9, 13
STATUS_OK, STATUS_NONFINITE = 0, 4
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
# the issue's known answers: (counter, key, output)
KNOWN = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
          (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
MEMS = dict(sigma_gyro=2e-3, sigma_accel=5e-2, walk_gyro=1e-5, walk_accel=1e-4, bias0_gyro=5e-3, bias0_accel=5e-2,
            sigma_q=0.0, sigma_qd=5e-2, q_lsb=2.0 * np.pi / 2 ** 14, touch_lag=2, p_drop=0.0)


class Params:
    """The constants of mpcqp_set_sensors and the dt_control of mpcqp_set_planner."""

    def __init__(self, seed=0, sigma_gyro=0.0, sigma_accel=0.0, walk_gyro=0.0, walk_accel=0.0, bias0_gyro=0.0,
                 bias0_accel=0.0, sigma_q=0.0, sigma_qd=0.0, q_lsb=0.0, touch_lag=0, p_drop=0.0, dt=0.001):
        self.seed = int(seed)
        self.sigma_gyro, self.sigma_accel, self.walk_gyro, self.walk_accel = map(float, (sigma_gyro, sigma_accel, walk_gyro, walk_accel))
        self.bias0_gyro, self.bias0_accel, self.sigma_q, self.sigma_qd = map(float, (bias0_gyro, bias0_accel, sigma_q, sigma_qd))
        self.q_lsb, self.touch_lag, self.p_drop, self.dt = float(q_lsb), int(touch_lag), float(p_drop), float(dt)

    def constants(self):
        return {k: getattr(self, k) for k in MEMS}


def valid(seed=0, touch_lag=0, p_drop=0.0, **c):
    """Whether mpcqp_set_sensors accepts the constants."""
    vals = [float(v) for v in c.values()] + [float(p_drop)]
    return (all(np.isfinite(v) and v >= 0.0 for v in vals) and 0 <= int(touch_lag) <= 31 and float(p_drop) < 1.0)


def philox(counter, key):
    """Philox4x32-10: counter [...,4], key [...,2] (integers below 2^32) -> [...,4] uint32."""
    c = [np.asarray(counter)[..., k].astype(np.uint64) for k in range(4)]
    k0, k1 = (np.asarray(key)[..., k].astype(np.uint64) for k in range(2))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, -1).astype(np.uint32)


def log(x):
    """ln x for normal x > 0 in IEEE operations alone, the header's sense_log operation by
    operation (fdlibm's evaluation): the same bits as the host and the device build."""
    b = np.ascontiguousarray(x, np.float64).view(np.uint64)
    k = (b >> np.uint64(52)).astype(np.int64) - 1023
    m = b & np.uint64(0xFFFFFFFFFFFFF)
    up = m >= np.uint64(0x6A09E667F3BCD)
    k = k + up
    xm = (m | (np.where(up, np.uint64(1022), np.uint64(1023)) << np.uint64(52))).view(np.float64)
    f, dk = xm - 1.0, k.astype(np.float64)
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01))
    t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)))
    R, hfsq = t2 + t1, 0.5 * f * f
    return dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + dk * 1.90821492927058770002e-10)) - f)


def sincos_turn(u):
    """(sin, cos) of 2 pi u for u in [0, 1], the header's sense_sincos_turn operation by operation."""
    u = np.asarray(u, np.float64)
    kf = np.floor(4.0 * u + 0.5)
    y = 6.283185307179586 * (u - 0.25 * kf)
    z = y * y
    rs = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))
    s = y + (z * y) * (-1.66666666666666324348e-01 + z * rs)
    rc = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 + z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))))
    c = 1.0 - (0.5 * z - z * rc)
    q = kf.astype(np.int64) & 3
    return np.choose(q, [s, c, -s, -c]), np.choose(q, [c, -s, -c, s])


def normals(w0, w1):
    """Two words -> two standard normals by Box-Muller in float64."""
    u0 = (w0.astype(np.float64) + 0.5) * 2.0 ** -32
    u1 = (w1.astype(np.float64) + 0.5) * 2.0 ** -32
    r = np.sqrt(-2.0 * log(u0))
    sn, cs = sincos_turn(u1)
    return r * cs, r * sn


def _add(x, add):
    """x + add, and x itself where add is zero (the sign of a zero stays)."""
    return np.where(add == 0.0, x, x + add)


def new_state(B, ids=None):
    st = np.zeros((B, STRIDE))
    st[:, ID] = np.arange(B) if ids is None else ids
    return st


def draws(state, P):
    """The 16 blocks of every robot's next call: [B,16,4] uint32."""
    B = len(state)
    count = state[:, COUNT].astype(np.uint64)
    ctr = np.zeros((B, 16, 4), np.uint64)
    ctr[:, :, 0] = (count & MASK)[:, None]
    ctr[:, :, 1] = (count >> np.uint64(32))[:, None]
    ctr[:, :, 2] = (state[:, ID].astype(np.uint64) & MASK)[:, None]
    ctr[:, :, 3] = np.arange(16)
    key = np.array([P.seed & 0xFFFFFFFF, P.seed >> 32], np.uint64)
    return philox(ctr, np.broadcast_to(key, (B, 16, 2)))


def tick(state, P, gyro=None, accel=None, dofs=None, touch=None, scale=None):
    """One call of mpcqp_sensors on state [B,STRIDE], in place.  Inputs float32 (gyro, accel
    [B,3], dofs [B,12,2], touch [B,4]), each None to leave the group out.  Returns a dict of the
    float32 outputs of the groups given, plus status [B] int32."""
    B = len(state)
    f4 = np.float32
    ins = dict(gyro=gyro, accel=accel, dofs=dofs, touch=touch)
    ins = {k: None if v is None else np.asarray(v, f4).reshape(B, -1) for k, v in ins.items()}
    s = np.ones(B) if scale is None else np.asarray(scale, f4).astype(np.float64)
    with np.errstate(invalid="ignore"):
        bad = ~(np.isfinite(s) & (s >= 0.0)) | ~np.isfinite(state[:, :WORDS]).all(1)
        # the words read as integers lie in their integer's range
        bad |= ~((state[:, COUNT] >= 0) & (state[:, COUNT] < 2.0 ** 53))
        ints = state[:, [ID, HIST, HIST + 1, HIST + 2, HIST + 3]]
        bad |= ~((ints >= 0) & (ints < 2.0 ** 32)).all(1)
        for v in ins.values():
            if v is not None:
                bad |= ~np.isfinite(v).all(1)
    ok = ~bad
    safe = np.where(bad[:, None], 0.0, state)
    safe[:, ID] = np.where(bad, 0.0, state[:, ID])
    w = draws(safe, P)
    s = np.where(bad, 0.0, s)
    init = safe[:, INIT] != 0.0
    out = {}
    with np.errstate(all="ignore"):
        # joints: block j, words 0, 1
        zq, zqd = normals(w[:, :12, 0], w[:, :12, 1])
        if ins["dofs"] is not None:
            d = ins["dofs"].reshape(B, 12, 2).astype(np.float64)
            q = _add(d[..., 0], (s * P.sigma_q)[:, None] * zq)
            if P.q_lsb > 0.0:
                q = np.rint(q / P.q_lsb) * P.q_lsb
            qd = _add(d[..., 1], (s * P.sigma_qd)[:, None] * zqd)
            m = np.stack([q, qd], -1).astype(f4)
            out["dofs"] = np.where(ok[:, None, None], m, ins["dofs"].reshape(B, 12, 2))
        # IMU axes: block 12 + a, words 0, 1 white, words 2, 3 walk
        zg, za = normals(w[:, 12:15, 0], w[:, 12:15, 1])
        zwg, zwa = normals(w[:, 12:15, 2], w[:, 12:15, 3])
        sd = np.sqrt(P.dt)
        bg, ba = safe[:, BIAS_G:BIAS_G + 3], safe[:, BIAS_A:BIAS_A + 3]
        bg = np.where(init[:, None], _add(bg, ((s * P.walk_gyro) * sd)[:, None] * zwg), (s * P.bias0_gyro)[:, None] * zwg)
        ba = np.where(init[:, None], _add(ba, ((s * P.walk_accel) * sd)[:, None] * zwa), (s * P.bias0_accel)[:, None] * zwa)
        for name, b, sig, z in (("gyro", bg, P.sigma_gyro, zg), ("accel", ba, P.sigma_accel, za)):
            if ins[name] is not None:
                m = _add(ins[name].astype(np.float64), b + (s * sig)[:, None] * z).astype(f4)
                out[name] = np.where(ok[:, None], m, ins[name])
        # feet: block 15, word f
        hist = safe[:, HIST:HIST + 4].astype(np.uint64)
        if ins["touch"] is not None:
            now = (ins["touch"] > 0).astype(np.uint64)
            hist = np.where(init[:, None], ((hist << np.uint64(1)) | now) & MASK, now * MASK)
            on = ((hist >> np.uint64(P.touch_lag)) & np.uint64(1)) != 0
            on &= ~(w[:, 15, :].astype(np.uint64) < np.uint64(int(np.floor(P.p_drop * 2.0 ** 32))))
            out["touch"] = np.where(ok[:, None], on.astype(f4), ins["touch"])
    state[ok, BIAS_G:BIAS_G + 3] = bg[ok]
    state[ok, BIAS_A:BIAS_A + 3] = ba[ok]
    state[ok, HIST:HIST + 4] = hist[ok].astype(np.float64)
    state[ok, INIT] = 1.0
    state[ok, COUNT] += 1.0
    out["status"] = np.where(bad, STATUS_NONFINITE, STATUS_OK).astype(np.int32)
    return out


def push(rec, impulse, robot, point=None):
    """mpcqp_push on the plant records rec [B,plant_ref.STRIDE], in place: v += J / m,
    w += I_w^-1 ((Rq r) x J) with I_w^-1 = Rq I^-1 Rq^T applied as the plant applies it.  Returns
    status [B] int32."""
    pr = plant_ref
    B = len(rec)
    J = np.asarray(impulse, np.float32).astype(np.float64).reshape(B, 3)
    rb = np.asarray(robot, np.float32).astype(np.float64)
    Ii, det = pr._inv3(pr.inertia(robot))
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(J).all(1) | ~np.isfinite(rec[:, :pr.WORDS]).all(1) | ~np.isfinite(rb[:, :8]).all(1)
        bad |= ~(rb[:, 0] > 0.0) | ~(np.abs(det) > 0.0) | ~(np.sum(rec[:, pr.QUAT:pr.QUAT + 4] ** 2, -1) > 0.0)
        v = _add(rec[:, pr.VEL:pr.VEL + 3], J / rb[:, 0:1])
        w = rec[:, pr.OMEGA:pr.OMEGA + 3].copy()
        if point is not None:
            r = np.asarray(point, np.float32).astype(np.float64).reshape(B, 3)
            bad |= ~np.isfinite(r).all(1)
            Rq = pr._rot(np.where(bad[:, None], np.array([1.0, 0, 0, 0]), rec[:, pr.QUAT:pr.QUAT + 4]))
            t = np.cross(pr._mv(Rq, r), J)
            w = _add(w, pr._mv(Rq, pr._mv(Ii, pr._mtv(Rq, t))))
        bad |= ~np.isfinite(v).all(1) | ~np.isfinite(w).all(1)
    ok = ~bad
    rec[ok, pr.VEL:pr.VEL + 3] = v[ok]
    rec[ok, pr.OMEGA:pr.OMEGA + 3] = w[ok]
    return np.where(bad, STATUS_NONFINITE, STATUS_OK).astype(np.int32)


# ---- the sensed closed loop on the CPU oracles

# the loop's fleet (tests/golden/disturb_loop.npz): scales of the preset for the first four robots,
# lateral impulses (N s, at the centre of mass, world y) at tick PUSH_TICK for the others, which
# are noise-free (scale 0: the encoder step and the touch lag stay, as for every robot): 0, 2, 4
# and 8 N s, and 1 N s, half the largest of them that recovers, for the device's loop to repeat
LOOP_SCALES = (0.0, 1.0, 2.0, 4.0, 0.0, 0.0, 0.0, 0.0, 0.0)
LOOP_PUSHES = (0.0, 0.0, 0.0, 0.0, 0.0, 2.0, 4.0, 8.0, 1.0)
LOOP_TICKS, LOOP_SETTLE, PUSH_TICK, LOOP_SEED = 600, 50, 400, 7
HEIGHT_BOUND, TILT_BOUND = 0.05, 0.1                # tests/test_gpu_plant.py's sensing-chain bounds
FIGURES = ("height", "roll", "pitch", "speed", "est_error", "within", "recovered")


def closed_loop_sensed(scales=LOOP_SCALES, pushes=LOOP_PUSHES, ticks=LOOP_TICKS, settle=LOOP_SETTLE,
                       push_tick=PUSH_TICK, constants=None, seed=LOOP_SEED, command=0.5, robot="aliengo",
                       gait="trot10", horizon=10, ibm=20):
    """plant -> sensors -> att_ref -> est_ref -> controller oracles -> plant_ref.plant_step, one
    robot per entry of ``scales`` / ``pushes``: plant_ref.closed_loop's loop with the controller
    fed the estimated root and the sensed joints.  The robots start standing on the ground and
    the estimator settles for ``settle`` ticks under the standing torques first, as
    tests/test_gpu_plant.py's sensing-chain test does.  Returns per-tick arrays: body [T,B,13]
    (the plant record's body words), est [T,B,13], and ok [T,B]."""
    import att_ref
    import est_ref
    import kin_ref
    import swing_ref
    from mpcqp.params import LEG_GEOMETRY, ROBOT_PRESETS, SWING_PRESETS, gait_record, pack_leg_geometry, pack_robot
    from oracle import cpu_port
    from oracle.planner import PlannerOracle, gait_table, quat2matrix, world_velocity
    pr = plant_ref
    par = pr.Params()
    P = Params(seed=seed, dt=par.dt_control, **(MEMS if constants is None else constants))
    B = len(scales)
    scale = np.asarray(scales, np.float32)
    f4 = np.float32
    geom = pack_leg_geometry(LEG_GEOMETRY[robot], B)
    rrec = np.tile(pack_robot(ROBOT_PRESETS[robot]), (B, 1)).astype(f4)
    height = ROBOT_PRESETS[robot]["height"]
    grec = gait_record(gait)
    period, off, dur = int(grec[0]), tuple(int(x) for x in grec[1:5]), tuple(int(x) for x in grec[5:9])
    gaits = np.tile(grec, (B, 1))
    sw = SWING_PRESETS[robot]
    swing = swing_ref.SwingRef(B, dt_control=par.dt_control, gravity=par.gravity, swing_height=sw["swing_height"],
                               kp=sw["kp"], kd=sw["kd"])
    planners = [PlannerOracle(horizon, height, dt_control=par.dt_control, gravity=par.gravity) for _ in range(B)]
    vb = np.stack([np.full(B, float(command)), np.zeros(B), np.zeros(B)], 1)
    yr = np.zeros(B)
    root, dofs = pr.stand_pose(B, geom, par)                # the feet on the ground
    rec = pr.reset(root, dofs, geom, par)
    sense = new_state(B)
    att = np.zeros((B, att_ref.STRIDE))
    est = np.zeros((B, est_ref.STRIDE))
    est_c = dict(contact_height=par.ground_z)
    out = dict(gyro=np.zeros((B, 3), f4), accel=np.zeros((B, 3), f4), dofs=dofs, touch=rec[:, pr.CONTACT:pr.CONTACT + 4].astype(f4))

    def sensed(out, it):
        nonlocal att, est
        m = tick(sense, P, gyro=out["gyro"], accel=out["accel"], dofs=out["dofs"], touch=out["touch"], scale=scale)
        att, a = att_ref.attitude_step(att, dict(gyro=m["gyro"], accel=m["accel"], tick=np.full(B, it), gait=gaits, ibm=ibm,
                                                 touch=m["touch"]))
        d = m["dofs"].reshape(B, 12, 2)
        est, e = est_ref.estimate_step(est, dict(quat=a["quat"].astype(f4), gyro=a["gyro_out"].astype(f4), accel=m["accel"],
                                                 q=d[..., 0], qdot=d[..., 1], trust=a["trust"].astype(f4), geom=geom), est_c)
        bad = (m["status"] != 0) | (a["status"] != 0) | (e["status"] != 0)
        return e["root_states"].astype(f4), d, bad

    _, _, Jb = kin_ref.chain(geom, dofs[:, :, 0])
    m0 = float(rrec[0, 0])
    stand = np.einsum("blcr,c->blr", Jb, -np.array([0, 0, m0 * par.gravity / 4])).reshape(B, 12).astype(f4)
    for it in range(settle):
        out = pr.plant_step(rec, stand, rrec, geom, par)
        sensed(out, it)
    u0 = np.zeros((B, 12), f4)
    J = np.zeros((B, 3), f4)
    J[:, 1] = np.asarray(pushes, f4)
    log = dict(body=[], est=[], ok=[])
    for t in range(ticks):
        seen, d, bad = sensed(out, t)
        quat = np.concatenate([seen[:, 6:7], seen[:, 3:6]], 1)
        pos, vel, omega = seen[:, 0:3], seen[:, 7:10], seen[:, 10:13]
        kin = kin_ref.kinematics(geom, quat, pos, vel, omega, d[..., 0], d[..., 1])
        k32 = {k: v.astype(f4) for k, v in kin.items()}
        mpc = t % ibm == 0
        x0 = np.zeros((B, 13), f4)
        xref = np.zeros((B, horizon, 13), f4)
        for b in range(B):
            o = planners[b]
            x0[b] = o.update_robot_state(quat[b], pos[b], omega[b], vel[b])
            vw = world_velocity(quat2matrix(quat[b]), vb[b])
            o.integrate(vw, yr[b])
            if mpc:
                xref[b] = o.reference_trajectory(vw, yr[b])
        if mpc:
            ct = np.tile(gait_table(period, off, dur, (t // ibm) % period, horizon), (B, 1, 1))
            U, its, _, _ = cpu_port.solve_batch(dict(x0=x0, xref=xref, contact=ct, feet=k32["feet"], robot=rrec), horizon)
            u0 = U[:, :12].astype(f4)
            bad = bad | (its < 0)
        o = swing.step(np.full(B, t), ibm, gaits, pos, vel, swing_ref.quat2matrix_f32(quat), vb, yr, k32["thighs"],
                       k32["pos_feet"], k32["foot_pos_base"], k32["foot_vel_base"], k32["jac"], u0)
        if t == push_tick:
            bad = bad | (push(rec, J, rrec) != 0)
        out = pr.plant_step(rec, o["tau"], rrec, geom, par)
        log["body"].append(rec[:, :13].copy())
        log["est"].append(seen.copy())
        log["ok"].append(~bad & (out["status"] == 0) & np.isfinite(rec).all(1) & np.isfinite(o["tau"]).all(1))
    return {k: np.stack(v) for k, v in log.items()}


def loop_figures(body, est, ok, dt=0.001, height=0.38, last=300, tail=100):
    """Per robot from body [T,B,13] (pos, quat w x y z, vel, omega) and est [T,B,13] (root-state
    layout): worst |height - desired|, worst |roll| and |pitch|, the forward speed over the last
    ``last`` ticks, the worst error of the estimated position, whether the robot stayed within
    the sensing-chain test's bounds on every tick (`within`) and whether it is within them over
    the last ``tail`` ticks with every status OK throughout (`recovered`)."""
    rp = [plant_ref.euler_zyx(b[:, 3:7]) for b in body]
    roll, pitch = np.abs(np.stack([r for r, _ in rp])), np.abs(np.stack([p for _, p in rp]))
    herr = np.abs(body[:, :, 2] - height)
    inside = (herr < HEIGHT_BOUND) & (np.maximum(roll, pitch) < TILT_BOUND) & np.isfinite(body).all(2)
    fine = ok.all(0)
    return dict(height=herr.max(0), roll=roll.max(0), pitch=pitch.max(0),
                speed=(body[-1, :, 0] - body[-1 - last, :, 0]) / (last * dt),
                est_error=np.abs(est[:, :, 0:3] - body[:, :, 0:3]).max((0, 2)),
                within=inside.all(0) & fine, recovered=inside[-tail:].all(0) & fine)

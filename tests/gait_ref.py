"""Integer restatement of the gait scheduler (mpcqp_gait_schedule, include/mpcqp_gait_abi.h) in
NumPy and plain loops, with the automatic choice, and ``closed_loop_scheduled``: the control loop
on the repository's CPU oracles (plant_ref, kin_ref, oracle.planner, oracle.cpu_port,
swing_ref.SwingRef) with a per-robot gait, tick and command under this scheduler.

The reference changes gait by hand (scripts/mujoco_aliengo.py:121-155: fresh objects, iter_counter
back at 0); this file is the oracle of csrc/mpcqp_gait_robot.h.  Nothing here is shared with the
header: the seam test is written in Python's unbounded integers from the rule, and
``seam_by_counts`` counts a third way, from swing_ref.decide_exact.
"""
import math

import numpy as np

import swing_ref

STRIDE = 8                                           # MPCQP_SCHED_STRIDE
CUR, PENDING, SINCE, SWITCHES, CALM, LAST = range(6)
ADVANCE = 1                                          # MPCQP_GAIT_ADVANCE
GAIT_MAX, MAX_PERIOD = 16, 2048
OK, NONFINITE, UNSUPPORTED = 0, 4, 5
INT_MAX = 2 ** 31 - 1

# the three custom records of the tests beside params.GAITS: stance offsets past the period,
# one leg whose stance fills the period, a one-segment period
CUSTOM = ((10, (7, 12, 12, 7), (5, 5, 5, 5)), (10, (0, 5, 5, 0), (5, 10, 5, 5)), (1, (0, 0, 0, 0), (0, 1, 0, 1)))
# no segment of it is free of a mid-swing leg: two legs swing all the time, one segment apart
NO_ENTRY = (4, (0, 1, 0, 0), (0, 0, 4, 4))


def record(g):
    """[9] int from (period, offsets, durations) or a flat record."""
    if len(g) == 3:
        return np.array([g[0], *g[1], *g[2]], np.int64)
    return np.asarray(g, np.int64).reshape(9)


def mid_swing(t, ibm, g, leg):
    """Leg `leg` of record g is past its first swing tick and before its last at tick t."""
    P, off, dur = int(g[0]), int(g[1 + leg]), int(g[5 + leg])
    if P <= 0 or ibm <= 0:
        return False
    nsw = (P - dur) * ibm
    if nsw <= 0:
        return False
    span = ibm * P
    cs = (int(t) % span - (off + dur) * ibm) % span
    return 1 <= cs < nsw


def seam(t, ibm, g):
    return int(t) % ibm == 0 and not any(mid_swing(t, ibm, g, l) for l in range(4))


def seam_by_counts(t, ibm, g):
    """The same from swing_ref.decide_exact's counters, the leg controller's own decision."""
    if int(t) % ibm:
        return False
    for leg in range(4):
        swing, finished, cs, nsw = swing_ref.decide_exact(t, ibm, g, leg)
        if swing and not finished:
            return False
    return True


def entry(g):
    """The smallest segment whose first tick is a seam, in segment units as the rule states it:
    k = (s - off - dur) mod P in {0} or [P - dur, P - 1] for every leg with dur < P; None: no such."""
    P = int(g[0])
    for s in range(P):
        ok = True
        for leg in range(4):
            off, dur = int(g[1 + leg]), int(g[5 + leg])
            if dur < P:
                k = (s - off - dur) % P
                ok = ok and (k == 0 or P - dur <= k <= P - 1)
        if ok:
            return s
    return None


def valid(g):
    P = int(g[0])
    if not 1 <= P <= MAX_PERIOD:
        return False
    return all(0 <= int(g[5 + l]) <= P and abs(int(g[1 + l])) <= 4 * P for l in range(4))


def library(gaits):
    """[count, 10] int64: each record and its entry segment; ValueError as mpcqp_set_gaits refuses."""
    recs = [record(g) for g in gaits]
    if not 1 <= len(recs) <= GAIT_MAX:
        raise ValueError("count")
    rows = []
    for g in recs:
        if not valid(g) or entry(g) is None:
            raise ValueError(f"record {g.tolist()}")
        rows.append(np.r_[g, entry(g)])
    return np.stack(rows)


class Constants:
    """mpcqp_set_gait_schedule's."""

    def __init__(self, min_hold=0, idle=-1, move=-1, v_go=0.0, v_stop=0.0, w_go=0.0, w_stop=0.0, dwell=0):
        self.min_hold, self.idle, self.move, self.dwell = int(min_hold), int(idle), int(move), int(dwell)
        self.v_go, self.v_stop, self.w_go, self.w_stop = float(v_go), float(v_stop), float(w_go), float(w_stop)


def auto_choice(c, vx, vy, yaw, pending, calm):
    """(ok, pending, calm) of one robot and one call."""
    if not (math.isfinite(vx) and math.isfinite(vy) and math.isfinite(yaw)):
        return False, pending, calm
    v2, w = vx * vx + vy * vy, abs(yaw)
    if v2 > c.v_go * c.v_go or w > c.w_go:
        return True, c.move, 0
    if v2 <= c.v_stop * c.v_stop and w <= c.w_stop:
        calm = min(calm + 1, INT_MAX)
        return True, (c.idle if calm >= c.dwell else pending), calm
    return True, pending, 0


def schedule(lib, c, flags, ibm, want, state, gait, tick, swing_mem=None, vel_body_des=None, yaw_rate_des=None):
    """One call of mpcqp_gait_schedule, in place on state [B,8], gait [B,9], tick [B] (int32
    arrays) and swing_mem [B,32] float64 (or None); want [B] or None (the automatic choice, from
    vel_body_des [B,3] and yaw_rate_des [B]).  Returns (iteration, switched, status) [B] int32."""
    B = len(tick)
    count = len(lib)
    sw, st = np.zeros(B, np.int32), np.zeros(B, np.int32)
    t = tick.astype(np.int64)
    s = state.astype(np.int64)
    live = ~((t < 0) | ((t == INT_MAX) if flags & ADVANCE else False))      # the others are left as they are
    st[~live] = UNSUPPORTED
    if flags & ADVANCE:
        t[live] += 1
        s[live, SINCE] = np.minimum(s[live, SINCE] + 1, INT_MAX)
    bad = np.zeros(B, bool)
    if want is not None:
        w = np.asarray(want, np.int64)
        inside = (w >= 0) & (w < count)
        s[live & inside, PENDING] = w[live & inside]
        st[live & ~inside & (w != -1)] = UNSUPPORTED
    else:
        for b in np.flatnonzero(live):
            ok, s[b, PENDING], s[b, CALM] = auto_choice(c, float(vel_body_des[b][0]), float(vel_body_des[b][1]),
                                                        float(yaw_rate_des[b]), int(s[b, PENDING]), int(s[b, CALM]))
            if not ok:
                st[b], bad[b] = NONFINITE, True
    asks = (live & ~bad & (s[:, PENDING] != s[:, CUR]) & (s[:, PENDING] >= 0) & (s[:, PENDING] < count)
            & (s[:, SINCE] >= c.min_hold) & (t % ibm == 0))
    for b in np.flatnonzero(asks):
        if seam(t[b], ibm, gait[b]):
            p = int(s[b, PENDING])
            gait[b] = lib[p, :9]
            s[b, LAST] = t[b]
            t[b] = int(lib[p, 9]) * ibm
            if swing_mem is not None:
                swing_mem[b, 0::8] = 0.0
            s[b, CUR], s[b, SINCE] = p, 0
            s[b, SWITCHES] = (s[b, SWITCHES] + 1 + 2 ** 31) % 2 ** 32 - 2 ** 31
            sw[b] = 1
    tick[live] = t[live]
    state[live] = s[live]
    P = gait[:, 0].astype(np.int64)
    span = np.where(P > 0, P, 1) * ibm
    it = np.where(P > 0, (t % span) // ibm, 0).astype(np.int32)
    return it, sw, st


# ---- the closed loop under the scheduler, on the CPU oracles

# The plan of the recorded run (tests/golden/gait_switch.npz): Aliengo, N = 10, ibm = 20, 1400
# ticks.  Per robot: the gait it starts in, its forward command from tick 0, and (tick, gait,
# command) requests written before that tick's call; the last robot runs the automatic choice
# (standing / trot10, go above 0.1 m/s, stop at 0.05 m/s, dwell 50) on (tick, command) changes.
PLAN_GAITS = ("standing", "trot10", "pace10", "trot16")
PLAN = (
    dict(initial="standing", command=0.0, requests=((313, "trot10", 0.5), (1017, "standing", 0.0))),
    dict(initial="trot10", command=0.5, requests=((537, "standing", 0.0),)),
    dict(initial="trot10", command=0.5, requests=((450, "pace10", 0.5),)),
    dict(initial="standing", command=0.0, requests=((200, "trot16", 0.3), (900, "trot10", 0.6))),
    dict(initial="trot10", command=0.5, requests=()),
    dict(initial="standing", command=0.0, auto=True, commands=((250, 0.5), (900, 0.0))),
)
PLAN_AUTO = dict(idle="standing", move="trot10", v_go=0.1, v_stop=0.05, w_go=0.1, w_stop=0.05, dwell=50)
PLAN_TICKS = 1400
PLAN_SWITCHES = ((320, 1020), (600,), (500,), (200, 1000), (), (260, 960))


def plan_events(plan, gaits):
    """{tick: [(robot, library index or None, command)]} of a plan."""
    ev = {}
    for b, p in enumerate(plan):
        for t, g, v in p.get("requests", ()):
            ev.setdefault(int(t), []).append((b, gaits.index(g), float(v)))
        for t, v in p.get("commands", ()):
            ev.setdefault(int(t), []).append((b, None, float(v)))
    return ev


def closed_loop_scheduled(plan, ticks, gaits=PLAN_GAITS, auto=PLAN_AUTO, robot="aliengo", horizon=10, ibm=20,
                          par=None, min_hold=0):
    """plant_ref.closed_loop with a per-robot gait, tick and command under the scheduler: plant
    outputs -> kin_ref -> oracle.planner -> oracle.cpu_port (MPC ticks) -> swing_ref.SwingRef ->
    plant_step, with ``schedule`` ahead of each iteration.  A robot with ``auto`` is scheduled by
    the automatic choice (a second call of ``schedule`` on its rows, as a second launch would).
    Returns per-tick arrays height, roll, pitch, x [T,B], solve_ok, finite [T,B] bool, switched
    [T,B], and ``switch_ticks``: per robot the iterations at which it switched."""
    import os
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pympc-quadruped_amd")
    for p in (os.path.dirname(pkg), pkg):
        if p not in sys.path:
            sys.path.insert(0, p)
    from mpcqp.params import LEG_GEOMETRY, ROBOT_PRESETS, SWING_PRESETS, gait_record, pack_leg_geometry, pack_robot
    from oracle import cpu_port
    from oracle.planner import PlannerOracle, gait_table, quat2matrix, world_velocity
    import kin_ref
    import plant_ref as pr

    par = par or pr.Params()
    B = len(plan)
    gaits = tuple(gaits)
    lib = library([gait_record(g) for g in gaits])
    c = Constants(min_hold=min_hold, idle=gaits.index(auto["idle"]), move=gaits.index(auto["move"]),
                  **{k: auto[k] for k in ("v_go", "v_stop", "w_go", "w_stop", "dwell")})
    is_auto = np.array([bool(p.get("auto")) for p in plan])
    geom = pack_leg_geometry(LEG_GEOMETRY[robot], B)
    rrec = np.tile(pack_robot(ROBOT_PRESETS[robot]), (B, 1)).astype(np.float32)
    height = ROBOT_PRESETS[robot]["height"]
    sw = SWING_PRESETS[robot]
    swing = swing_ref.SwingRef(B, dt_control=par.dt_control, gravity=par.gravity, swing_height=sw["swing_height"],
                               kp=sw["kp"], kd=sw["kd"])
    planners = [PlannerOracle(horizon, height, dt_control=par.dt_control, gravity=par.gravity) for _ in range(B)]
    state = np.zeros((B, STRIDE), np.int32)
    state[:, CUR] = state[:, PENDING] = [gaits.index(p["initial"]) for p in plan]
    gait = lib[state[:, CUR], :9].astype(np.int32)
    tick = np.zeros(B, np.int32)
    want = np.full(B, -1, np.int32)
    vb = np.zeros((B, 3))
    vb[:, 0] = [p["command"] for p in plan]
    yr = np.zeros(B)
    events = plan_events(plan, gaits)
    root, dofs = pr.stand_pose(B, geom, par, height=height)
    rec = pr.reset(root, dofs, geom, par)
    u0 = np.zeros((B, 12), np.float32)
    f4 = np.float32
    log = dict(height=[], roll=[], pitch=[], x=[], solve_ok=[], finite=[], switched=[])
    ok = np.ones(B, bool)
    for t in range(ticks):
        for b, w, v in events.get(t, ()):
            vb[b, 0] = v
            if w is not None:
                want[b] = w
        mem = swing.mem.reshape(B, 32)
        flags = ADVANCE if t > 0 else 0
        switched = np.zeros(B, np.int32)
        for rows, wnt in ((~is_auto, want), (is_auto, None)):
            if rows.any():
                s2, g2, t2, m2 = state[rows], gait[rows], tick[rows], mem[rows]
                _, sw_, st_ = schedule(lib, c, flags, ibm, None if wnt is None else wnt[rows], s2, g2, t2, m2,
                                       vb[rows], yr[rows])
                assert (st_ == OK).all()
                state[rows], gait[rows], tick[rows], mem[rows] = s2, g2, t2, m2
                switched[rows] = sw_
        swing.mem[:] = mem.reshape(B, 4, 8)
        quat = np.concatenate([root[:, 6:7], root[:, 3:6]], 1)
        pos, vel, omega = root[:, 0:3], root[:, 7:10], root[:, 10:13]
        kin = kin_ref.kinematics(geom, quat, pos, vel, omega, dofs[..., 0], dofs[..., 1])
        k32 = {k: v.astype(f4) for k, v in kin.items()}
        mpc = t % ibm == 0
        assert (tick % ibm == t % ibm).all()
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
            ct = np.stack([gait_table(int(g[0]), tuple(int(x) for x in g[1:5]), tuple(int(x) for x in g[5:9]),
                                      (int(tk) // ibm) % int(g[0]), horizon) for g, tk in zip(gait, tick)])
            bt = dict(x0=x0, xref=xref, contact=ct, feet=k32["feet"], robot=rrec)
            U, it, _, _ = cpu_port.solve_batch(bt, horizon)
            u0 = U[:, :12].astype(f4)
            ok = it >= 0
        out = swing.step(tick.copy(), ibm, gait, pos, vel, swing_ref.quat2matrix_f32(quat), vb, yr, k32["thighs"],
                         k32["pos_feet"], k32["foot_pos_base"], k32["foot_vel_base"], k32["jac"], u0)
        res = pr.plant_step(rec, out["tau"], rrec, geom, par)
        root, dofs = res["root"], res["dofs"]
        roll, pitch = pr.euler_zyx(rec[:, pr.QUAT:pr.QUAT + 4])
        log["height"].append(rec[:, 2].copy())
        log["roll"].append(roll)
        log["pitch"].append(pitch)
        log["x"].append(rec[:, 0].copy())
        log["solve_ok"].append(ok.copy())
        log["finite"].append(np.isfinite(rec).all(1) & np.isfinite(out["tau"]).all(1) & (res["status"] == 0))
        log["switched"].append(switched)
    run = {k: np.stack(v) for k, v in log.items()}
    run["dt"] = par.dt_control
    run["switch_ticks"] = [np.flatnonzero(run["switched"][:, b]).tolist() for b in range(B)]
    return run


def phases(switch_ticks, ticks):
    """[(first, last + 1)] of the phases between a robot's switches."""
    edges = [0, *switch_ticks, ticks]
    return [(a, b) for a, b in zip(edges[:-1], edges[1:])]


def figures(x, height, roll, pitch, switch_ticks, dt, desired=0.38, last=200):
    """Per robot: worst |height - desired|, worst |roll|, |pitch|, and the mean forward speed over
    the last ``last`` ticks of each phase (x, height, roll, pitch: [T,B]; x sampled after each
    iteration's plant step)."""
    T, B = x.shape
    err = np.abs(height - desired).max(0)
    tilt = np.maximum(np.abs(roll), np.abs(pitch)).max(0)
    speeds = []
    for b in range(B):
        row = []
        for a, e in phases(switch_ticks[b], T):
            n = min(last, e - a - 1)
            row.append((x[e - 1, b] - x[e - 1 - n, b]) / (n * dt))
        speeds.append(row)
    return err, tilt, speeds

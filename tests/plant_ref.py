"""Float64 NumPy restatement of the rigid-body plant (mpcqp_plant, include/mpcqp_plant_abi.h),
batched over robots: a single rigid body on four massless legs with point feet, the model the
MPC assumes with the nonlinear rotation kept and the contact decided by the ground.  The
reference has no such component (its scripts call a simulator); this file is the oracle of
csrc/mpcqp_plant_robot.h, and ``closed_loop`` wires it to the repository's CPU oracles of the
controller (oracle.planner, oracle.cpu_port, swing_ref.SwingRef, kin_ref) so that a test can
show that the controller walks.

Record layout (STRIDE float64 words per robot): pos 3, quat (w, x, y, z) 4, vel 3, omega 3
(world frame), foot positions 12 (world), foot velocities 12, contact 4, flag word, tick count.
"""
import numpy as np

import kin_ref

STRIDE = 48                                         # MPCQP_PLANT_STRIDE
POS, QUAT, VEL, OMEGA, FEET, FVEL, CONTACT, FLAGS, TICK = 0, 3, 7, 10, 13, 25, 37, 41, 42
WORDS = 43
IK_EPS = 2.0 ** -90                                 # the knee clamp: cos(calf) in [-1 + eps, 1 - eps]
IK_TINY = 1e-30                                     # floor of y^2 + z^2 - d^2 (uz^2)
BAND = 1e-9                                         # "near a switching threshold"
STATUS_OK, STATUS_NONFINITE = 0, 4
# the closed loop's commands (forward speed, m/s) and what closed_loop(COMMANDS, 1000) gives on
# Aliengo, TROTTING10, N = 10 (tests/test_plant.py asserts them): worst |height - 0.38| and worst
# |roll|, |pitch| over all ticks, mean forward speed over the last 500 ticks
COMMANDS = (0.0, 0.5, 1.0)
CLOSED_LOOP = dict(height=(0.01086, 0.01094, 0.01109), tilt=(3.3e-8, 0.0336, 0.0854), speed=(0.0, 0.5210, 1.0442))


class Params:
    """The constants of mpcqp_set_plant and mpcqp_set_planner."""

    def __init__(self, dt_control=0.001, gravity=9.81, foot_mass=0.15, substeps=1, ground_z=-0.0255,
                 contact_tol=1e-4):
        self.dt_control, self.gravity, self.foot_mass = float(dt_control), float(gravity), float(foot_mass)
        self.substeps, self.ground_z, self.contact_tol = int(substeps), float(ground_z), float(contact_tol)


def planes(B, par, plane=None):
    """[B,4] (n, d), the plane n . p = d (mpcqp_set_ground's convention); None: level at ground_z."""
    if plane is None:
        return np.tile(np.array([0.0, 0.0, 1.0, par.ground_z]), (B, 1))
    return np.asarray(plane, np.float32).astype(np.float64).reshape(B, 4)


def ik(geom, p):
    """Foot positions p [B,4,3] in the base frame -> (q [B,4,3], clamped [B,4] bool): the knee
    bent back (calf < 0), the branch of the reference's 0.8 / -1.6 crouch."""
    g = np.asarray(geom, np.float64)
    p = np.asarray(p, np.float64)
    hx, hy, d = kin_ref.SX * g[:, 0:1], kin_ref.SY * g[:, 1:2], kin_ref.SY * g[:, 2:3]
    l1, l2 = g[:, 3:4], g[:, 4:5]
    x, y, z = p[..., 0] - hx, p[..., 1] - hy, p[..., 2]
    r2 = (y * y + z * z) - d * d
    low = ~(r2 >= IK_TINY)
    uz = -np.sqrt(np.where(low, IK_TINY, r2))
    q1 = np.arctan2(z, y) - np.arctan2(uz, d)
    # a = 2 l1 l2 (1 - c3), b = 2 l1 l2 (1 + c3), c3 the law of cosines' cos(calf): the clamp on
    # c3 is applied to them, where eps can be far below a double's spacing at 1
    L2 = x * x + uz * uz
    k2 = (2.0 * l1) * l2 + 0.0 * L2
    lim = k2 * IK_EPS
    a, b = (l1 + l2) * (l1 + l2) - L2, L2 - (l1 - l2) * (l1 - l2)
    hi = ~(a >= lim)
    lo = ~hi & ~(b >= lim)
    # a + b = 4 l1 l2: a clamped end takes the other with it, as the clamp of c3 does
    a, b = np.where(hi, lim, np.where(lo, 2.0 * k2 - lim, a)), np.where(hi, 2.0 * k2 - lim, np.where(lo, lim, b))
    sa, sb, tot = np.sqrt(a), np.sqrt(b), a + b
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(tot > 0.0, 1.0 / tot, 0.0)
    s3, c3 = -(((2.0 * sa) * sb) * inv), (b - a) * inv
    q3 = -(2.0 * np.arctan2(sa, sb))
    q2 = np.arctan2(-x, -uz) - np.arctan2(l2 * s3, l1 + l2 * c3)
    return np.stack([q1, q2, q3], -1), low | hi | lo


def _inv3(M):
    """Cofactor inverse of [...,3,3] (the header's formula), and the determinant."""
    a, b, c, d, e, f, g, h, i = (M[..., r, k] for r in range(3) for k in range(3))
    c00, c01, c02 = e * i - f * h, c * h - b * i, b * f - c * e
    c10, c11, c12 = f * g - d * i, a * i - c * g, c * d - a * f
    c20, c21, c22 = d * h - e * g, b * g - a * h, a * e - b * d
    det = (a * c00 + b * c10) + c * c20
    with np.errstate(divide="ignore", invalid="ignore"):
        r = 1.0 / det
        inv = np.stack([np.stack([c00, c01, c02], -1), np.stack([c10, c11, c12], -1),
                        np.stack([c20, c21, c22], -1)], -2) * r[..., None, None]
    return inv, det


def inertia(robot):
    """[B,3,3] float64 from the float32 robot record (mass, ixx, ixy, ixz, iyy, iyz, izz, mu)."""
    r = np.asarray(robot, np.float32).astype(np.float64)
    return np.stack([r[:, 1], r[:, 2], r[:, 3], r[:, 2], r[:, 4], r[:, 5], r[:, 3], r[:, 5], r[:, 6]], -1).reshape(-1, 3, 3)


def _rot(quat):
    return kin_ref.quat2matrix_eigen(quat)


def _mv(M, x):
    return np.einsum("...rc,...c->...r", M, x)


def _mtv(M, x):
    return np.einsum("...cr,...c->...r", M, x)


def _leg_state(geom, Rq, pos, feet):
    """IK and the base-frame Jacobian inverse of the four legs: q [B,4,3], clamped, Jb^-1."""
    r = feet - pos[:, None]
    pb = np.einsum("bcr,blc->blr", Rq, r)
    q, cl = ik(geom, pb)
    _, _, Jb = kin_ref.chain(geom, q.reshape(len(q), 12))
    Ji, _ = _inv3(Jb)
    return r, q, cl, Ji


def substep(rec, tau, robot, geom, plane, par, h, margins=None, trace=None):
    """One substep of length h on the records rec [B,STRIDE], in place.  Returns (F / m [B,3],
    the specific force of the accelerometer, in the world frame; clamped [B,4]).  ``margins``,
    a list, receives the distance of every decision from its switching threshold; ``trace``, a
    list, the decisions themselves (trace_step)."""
    B = rec.shape[0]
    tau = np.asarray(tau, np.float64).reshape(B, 4, 3)
    rb = np.asarray(robot, np.float32).astype(np.float64)
    m, mu = rb[:, 0], rb[:, 7]
    I = inertia(robot)
    Ii, _ = _inv3(I)
    n, d = plane[:, None, :3], plane[:, None, 3]
    gvec = np.array([0.0, 0.0, -par.gravity])
    pos, quat, v, w = rec[:, POS:POS + 3].copy(), rec[:, QUAT:QUAT + 4].copy(), rec[:, VEL:VEL + 3].copy(), rec[:, OMEGA:OMEGA + 3].copy()
    pf, vf = rec[:, FEET:FEET + 12].reshape(B, 4, 3).copy(), rec[:, FVEL:FVEL + 12].reshape(B, 4, 3).copy()
    ct = rec[:, CONTACT:CONTACT + 4] != 0.0
    Rq = _rot(quat)
    r, q, cl, Ji = _leg_state(geom, Rq, pos, pf)
    # g = J^-T tau = Rq Jb^-T tau: the force the leg puts on its foot
    g = np.einsum("brc,blc->blr", Rq, np.einsum("blcr,blc->blr", Ji, tau))
    f = -g
    fn = np.sum(n * f, -1)
    release = ct & ~(fn > 0.0)
    pinned = ct & ~release
    ft = f - fn[..., None] * n
    ftn = np.sqrt(np.sum(ft * ft, -1))
    cap = mu[:, None] * fn
    over = pinned & (ftn > cap)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(over, cap / ftn, 1.0)
    f_pin = fn[..., None] * n + scale[..., None] * ft
    # a released foot goes on as a free foot in the same substep, from rest: it was pinned in the
    # world (a pinned foot's stored velocity is zero).  Starting it at the velocity of its body
    # point instead re-lands it every substep under a descending hip, and the loop falls
    vf = np.where(release[..., None], 0.0, vf)
    free = ~pinned
    a = g / par.foot_mass + gvec
    vf_new = vf + h * a
    pf_new = pf + h * vf_new
    s = np.sum(n * pf_new, -1) - d
    vn = np.sum(n * vf_new, -1)
    land = free & (s <= 0.0) & (vn < 0.0)
    pf_new = np.where(land[..., None], pf_new - s[..., None] * n, pf_new)
    vf_new = np.where(land[..., None], 0.0, vf_new)
    pf = np.where(free[..., None], pf_new, pf)
    vf = np.where(free[..., None], vf_new, 0.0)
    ct_new = pinned | land
    F = np.where(pinned[..., None], f_pin, -g)
    if margins is not None:
        # n . f = 0; a leg whose three torques are exactly zero has g = 0 exactly on any build
        margins.append(np.where(ct & (tau != 0.0).any(-1), np.abs(fn), np.inf))
        margins.append(np.where(pinned, np.abs(ftn - cap), np.inf))                        # the cone edge
        margins.append(np.where(free & (vn < 0.0), np.abs(s), np.inf))                     # the plane
    M = np.cross(r, F)
    SF = (F[:, 0] + F[:, 1]) + (F[:, 2] + F[:, 3])
    SM = (M[:, 0] + M[:, 1]) + (M[:, 2] + M[:, 3])
    spec = SF / m[:, None]
    v = v + h * (spec + gvec)
    # rotation: the angular momentum L = I_w w is advanced by the moment and held through the
    # rotation (w = I_w'^-1 L' on the new attitude), so free flight conserves it to rounding;
    # the attitude turns by the explicit predictor w + h I_w^-1 (M - w x L)
    L = _mv(Rq, _mv(I, _mtv(Rq, w)))
    ws = w + h * _mv(Rq, _mv(Ii, _mtv(Rq, SM - np.cross(w, L))))
    pos = pos + h * v
    if trace is not None:
        trace.append(dict(pinned=pinned, over=over, release=release, land=land, t=np.sqrt(np.sum((h * ws) ** 2, -1))))
    quat = quat_step(quat, h * ws)
    Rn = _rot(quat)
    w = _mv(Rn, _mv(Ii, _mtv(Rn, L + h * SM)))
    rec[:, POS:POS + 3], rec[:, QUAT:QUAT + 4], rec[:, VEL:VEL + 3], rec[:, OMEGA:OMEGA + 3] = pos, quat, v, w
    rec[:, FEET:FEET + 12], rec[:, FVEL:FVEL + 12] = pf.reshape(B, 12), vf.reshape(B, 12)
    rec[:, CONTACT:CONTACT + 4] = ct_new.astype(np.float64)
    return spec, cl


def quat_step(quat, th):
    """exp(th) (x) quat, normalised; quat (w, x, y, z), th [B,3] a world-frame rotation vector."""
    t2 = np.sum(th * th, -1)
    t = np.sqrt(t2)
    small = t < 1e-6
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(small, 0.5 - t2 / 48.0, np.sin(0.5 * t) / t)
    c = np.where(small, 1.0 - t2 / 8.0, np.cos(0.5 * t))
    ax, ay, az = s * th[:, 0], s * th[:, 1], s * th[:, 2]
    w, x, y, z = quat[:, 0], quat[:, 1], quat[:, 2], quat[:, 3]
    nw = ((c * w - ax * x) - ay * y) - az * z
    nx = ((c * x + ax * w) + ay * z) - az * y
    ny = ((c * y - ax * z) + ay * w) + az * x
    nz = ((c * z + ax * y) - ay * x) + az * w
    q = np.stack([nw, nx, ny, nz], -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return q / np.sqrt(np.sum(q * q, -1))[:, None]


def outputs(rec, geom, spec, par):
    """The kernel's outputs from the records: root [B,13] and dofs [B,12,2] float32, gyro, accel
    [B,3] and touch [B,4] float32, and the IK clamp bits of the output pose [B,4]."""
    B = rec.shape[0]
    pos, quat, v, w = rec[:, POS:POS + 3], rec[:, QUAT:QUAT + 4], rec[:, VEL:VEL + 3], rec[:, OMEGA:OMEGA + 3]
    pf, vf = rec[:, FEET:FEET + 12].reshape(B, 4, 3), rec[:, FVEL:FVEL + 12].reshape(B, 4, 3)
    Rq = _rot(quat)
    r, q, cl, Ji = _leg_state(geom, Rq, pos, pf)
    rel = (vf - v[:, None]) - np.cross(w[:, None], r)
    qd = _mv(Ji, np.einsum("bcr,blc->blr", Rq, rel))
    f4 = np.float32
    root = np.concatenate([pos, quat[:, 1:4], quat[:, 0:1], v, w], -1).astype(f4)
    dofs = np.stack([q.reshape(B, 12), qd.reshape(B, 12)], -1).astype(f4)
    return dict(root=root, dofs=dofs, gyro=_mtv(Rq, w).astype(f4), accel=_mtv(Rq, spec).astype(f4),
                touch=(rec[:, CONTACT:CONTACT + 4] != 0.0).astype(f4), clamped=cl)


def refused(rec, tau, robot):
    """[B] bool: a non-finite torque, a non-finite or non-invertible record."""
    rb = np.asarray(robot, np.float32).astype(np.float64)
    _, det = _inv3(inertia(robot))
    qn = np.sum(rec[:, QUAT:QUAT + 4] ** 2, -1)
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(np.asarray(tau, np.float64).reshape(len(rec), -1)).all(-1)
        bad |= ~np.isfinite(rec[:, :WORDS]).all(-1) | ~np.isfinite(rb[:, :8]).all(-1)
        bad |= ~(rb[:, 0] > 0.0) | ~(np.abs(det) > 0.0) | ~(qn > 0.0)
    return bad


def plant_step(rec, tau, robot, geom, par, plane=None, margins=None, trace=None):
    """One control iteration (par.substeps substeps of dt_control / substeps) on rec [B,STRIDE],
    in place.  Returns the outputs dict plus status [B] int32."""
    B = rec.shape[0]
    geom = np.asarray(geom, np.float64)
    pl = planes(B, par, plane)
    with np.errstate(invalid="ignore"):
        bad = refused(rec, tau, robot) | ~np.isfinite(np.asarray(geom)[:, :5]).all(-1) | ~np.isfinite(pl).all(-1)
    work = rec.copy()
    h = par.dt_control / par.substeps
    cl = np.zeros((B, 4), bool)
    with np.errstate(all="ignore"):
        for _ in range(par.substeps):
            spec, c = substep(work, tau, robot, geom, pl, par, h, margins, trace)
            cl |= c
        out = outputs(work, geom, spec, par)
        cl |= out["clamped"]
        work[:, FLAGS] = (cl * np.array([1, 2, 4, 8])).sum(-1).astype(np.float64)
        work[:, TICK] = rec[:, TICK] + 1.0
        res = np.concatenate([work[:, :WORDS]] + [out[k].reshape(B, -1) for k in ("root", "dofs", "gyro", "accel")], 1)
        bad |= ~np.isfinite(res).all(-1)
        if bad.any():
            rest = np.tile(np.array([0.0, 0.0, par.gravity]), (B, 1))
            old = outputs(rec, geom, rest, par)
            for k in out:
                out[k][bad] = old[k][bad]
    keep = ~bad
    rec[keep] = work[keep]
    out["status"] = np.where(bad, STATUS_NONFINITE, STATUS_OK).astype(np.int32)
    return out


def reset(root, dofs, geom, par, plane=None):
    """Records [B,STRIDE] from a pose in the loop's own tensors: feet by forward kinematics,
    foot velocities zero, contact where the foot is within contact_tol of the plane."""
    root = np.asarray(root, np.float32).astype(np.float64)
    B = root.shape[0]
    q = np.asarray(dofs, np.float32).astype(np.float64).reshape(B, 12, 2)[..., 0]
    geom = np.asarray(geom, np.float64)
    pl = planes(B, par, plane)
    rec = np.zeros((B, STRIDE))
    quat = np.concatenate([root[:, 6:7], root[:, 3:6]], 1)
    rec[:, POS:POS + 3], rec[:, QUAT:QUAT + 4] = root[:, 0:3], quat
    rec[:, VEL:VEL + 3], rec[:, OMEGA:OMEGA + 3] = root[:, 7:10], root[:, 10:13]
    p, _, _ = kin_ref.chain(geom, q)
    feet = root[:, None, 0:3] + np.einsum("brc,blc->blr", _rot(quat), p)
    rec[:, FEET:FEET + 12] = feet.reshape(B, 12)
    s = np.sum(pl[:, None, :3] * feet, -1) - pl[:, None, 3]
    rec[:, CONTACT:CONTACT + 4] = (s <= par.contact_tol).astype(np.float64)
    return rec


def stand_pose(B, geom, par, height=None, q=(0.0, 0.7, -1.4)):
    """root [B,13], dofs [B,12,2] float32 of a level robot with every leg at q; height None puts
    the feet on level ground at ground_z."""
    geom = np.asarray(geom, np.float64)
    dofs = np.zeros((B, 12, 2), np.float32)
    dofs[:, :, 0] = np.tile(np.asarray(q, np.float32), 4)
    root = np.zeros((B, 13), np.float32)
    root[:, 6] = 1.0
    if height is None:
        p, _, _ = kin_ref.chain(geom, dofs[:, :, 0])
        height = par.ground_z - p[:, :, 2].min(1)
    root[:, 2] = height
    return root, dofs


def euler_zyx(quat):
    """[B,4] (w, x, y, z) -> roll, pitch [B]."""
    w, x, y, z = (quat[:, k] for k in range(4))
    return np.arctan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y)), np.arcsin(np.clip(2 * (w * y - z * x), -1, 1))


def tilt_pose(root, tilt, azimuth, par):
    """A level pose turned rigidly about the origin onto a slope: root [B,13] float32 (stand_pose's),
    tilt [B] rad, azimuth [B] rad, the compass direction in which the ground climbs (0: along +x,
    uphill for a robot that walks forward; pi / 2: it climbs to the robot's left; pi: downhill).
    Position, velocities and quaternion are turned by the rotation R that takes e_z to
    n = (-sin tilt cos az, -sin tilt sin az, cos tilt); a point at height ground_z over the level
    ground lies on n . p = ground_z afterwards.  Returns (root [B,13] float32, plane [B,4]
    float32 = (R e_z, ground_z))."""
    root = np.asarray(root, np.float32).astype(np.float64)
    B = root.shape[0]
    tilt, az = np.broadcast_to(np.asarray(tilt, np.float64), (B,)), np.broadcast_to(np.asarray(azimuth, np.float64), (B,))
    axis = np.stack([np.sin(az), -np.cos(az), np.zeros(B)], -1)                      # z x n / |z x n|
    qt = np.concatenate([np.cos(tilt / 2)[:, None], np.sin(tilt / 2)[:, None] * axis], -1)
    Rt = _rot(qt)
    out = root.copy()
    for k in (0, 7, 10):
        out[:, k:k + 3] = _mv(Rt, root[:, k:k + 3])
    q = _quat_mul(qt, np.concatenate([root[:, 6:7], root[:, 3:6]], 1))
    out[:, 3:6], out[:, 6] = q[:, 1:4], q[:, 0]
    plane = np.concatenate([Rt[:, :, 2], np.full((B, 1), par.ground_z)], 1).astype(np.float32)
    return out.astype(np.float32), plane


def closed_loop(commands, ticks, robot="aliengo", gait="trot10", horizon=10, ibm=20, par=None, record_tau=False,
                heights=None, plane=None, terrain=None, terrain_ground=True):
    """The control loop on the CPU oracles, one robot per entry of ``commands`` (forward speeds,
    m/s): plant outputs -> kin_ref -> oracle.planner -> oracle.cpu_port (MPC ticks) ->
    swing_ref.SwingRef -> plant_step.  Returns per-tick arrays: height, roll, pitch, x [T,B],
    solve_ok [T,B] bool, finite [T,B] bool, touch [T,B,4]; with record_tau also tau [T,B,12]
    float32 and the starting records.  ``heights``: each robot's starting base height (default:
    the preset's desired height).

    ``plane`` [B,4]: the plant's ground, (n, ground_z) of tilt_pose, whose rotation the stand pose
    is started under; None: level.  ``terrain``: a dict of terrain constants (may be empty) runs
    the terrain stage in the order of ``ctl.step(...); ter.update()``: the tick's swing leg
    (terrain_ref.GroundSwingRef) and the tick's solve read the plane and the normal that the
    previous tick's update left; after the plant's step terrain_ref.tick_step runs on the float32
    pos_feet the controller saw and on ~swing, and (n, d) go, rounded to float32, to the swing leg
    (under ``terrain_ground`` as terrain_ref.ground_plane, MPCQP_TERRAIN_GROUND; without it the
    fitted (n, d) itself) and to words 9..11 of the robot records.  The run then also holds plane
    [T,B,4] float64 (the record's n, d) and fitted [T,B]; with a plane or a stage it holds swing
    [T,B,4] (the stage latches ~swing) and foothold [T,B,4,3], every leg's swing memory after the
    tick.  With both left out nothing of this is touched."""
    import os
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pympc-quadruped_amd")
    for p in (os.path.dirname(pkg), pkg):
        if p not in sys.path:
            sys.path.insert(0, p)
    from mpcqp.params import LEG_GEOMETRY, ROBOT_PRESETS, SWING_PRESETS, gait_record, pack_leg_geometry, pack_robot
    from oracle import cpu_port
    from oracle.planner import PlannerOracle, gait_table, quat2matrix, world_velocity
    import swing_ref

    par = par or Params()
    cmd = np.asarray(commands, np.float64)
    B = len(cmd)
    geom = pack_leg_geometry(LEG_GEOMETRY[robot], B)
    rrec = np.tile(pack_robot(ROBOT_PRESETS[robot]), (B, 1)).astype(np.float32)
    height = ROBOT_PRESETS[robot]["height"]
    grec = gait_record(gait)
    period, off, dur = int(grec[0]), tuple(int(x) for x in grec[1:5]), tuple(int(x) for x in grec[5:9])
    gaits = np.tile(grec, (B, 1))
    sw = SWING_PRESETS[robot]
    swing_kw = dict(dt_control=par.dt_control, gravity=par.gravity, swing_height=sw["swing_height"], kp=sw["kp"],
                    kd=sw["kd"])
    if terrain is None:
        swing = swing_ref.SwingRef(B, **swing_kw)
    else:
        import terrain_ref
        swing = terrain_ref.GroundSwingRef(B, **swing_kw)
        ter_state = np.zeros((B, terrain_ref.STRIDE))
    planners = [PlannerOracle(horizon, height, dt_control=par.dt_control, gravity=par.gravity) for _ in range(B)]
    vb = np.stack([cmd, np.zeros(B), np.zeros(B)], 1)
    yr = np.zeros(B)
    root, dofs = stand_pose(B, geom, par, height=height if heights is None else np.asarray(heights, np.float32))
    if plane is not None:
        pl = np.asarray(plane, np.float32).reshape(B, 4).astype(np.float64)
        # the pose is turned onto the plane the caller gives (tilt and azimuth read back from its
        # float32 words: the pose is off it by their rounding, which the first landing takes up)
        root, _ = tilt_pose(root, np.arctan2(np.hypot(pl[:, 0], pl[:, 1]), pl[:, 2]), np.arctan2(-pl[:, 1], -pl[:, 0]), par)
        plane = pl.astype(np.float32)
    rec = reset(root, dofs, geom, par, plane)
    rec0 = rec.copy()
    u0 = np.zeros((B, 12), np.float32)
    f4 = np.float32
    log = dict(height=[], roll=[], pitch=[], x=[], solve_ok=[], finite=[], touch=[], tau=[], plane=[], fitted=[],
               swing=[], foothold=[])
    ok = np.ones(B, bool)
    for t in range(ticks):
        quat = np.concatenate([root[:, 6:7], root[:, 3:6]], 1)
        pos, vel, omega = root[:, 0:3], root[:, 7:10], root[:, 10:13]
        kin = kin_ref.kinematics(geom, quat, pos, vel, omega, dofs[..., 0], dofs[..., 1])
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
            bt = dict(x0=x0, xref=xref, contact=ct, feet=k32["feet"], robot=rrec)
            U, it, _, _ = cpu_port.solve_batch(bt, horizon)
            u0 = U[:, :12].astype(f4)
            ok = it >= 0
        out = swing.step(np.full(B, t), ibm, gaits, pos, vel, swing_ref.quat2matrix_f32(quat), vb, yr, k32["thighs"],
                         k32["pos_feet"], k32["foot_pos_base"], k32["foot_vel_base"], k32["jac"], u0)
        tau = out["tau"]
        res = plant_step(rec, tau, rrec, geom, par, plane)
        root, dofs = res["root"], res["dofs"]
        if terrain is not None:
            ter_state, ter_ok = terrain_ref.tick_step(ter_state, k32["pos_feet"], ~out["swing"], terrain)
            n, d = ter_state[:, terrain_ref.N], ter_state[:, terrain_ref.D]
            swing.set_ground(terrain_ref.ground_plane(n, d, swing.touchdown_z) if terrain_ground
                             else np.concatenate([n, d[:, None]], 1).astype(f4))
            rrec[:, 9:12] = n.astype(f4)
            log["plane"].append(ter_state[:, 13:17].copy())
            log["fitted"].append((ter_state[:, terrain_ref.FITTED] != 0.0) & ter_ok)
        if terrain is not None or plane is not None:
            log["swing"].append(out["swing"].copy())
            log["foothold"].append(swing.mem[:, :, swing_ref.FINAL].copy())
        roll, pitch = euler_zyx(rec[:, QUAT:QUAT + 4])
        log["height"].append(rec[:, 2].copy())
        log["roll"].append(roll)
        log["pitch"].append(pitch)
        log["x"].append(rec[:, 0].copy())
        log["solve_ok"].append(ok.copy())
        log["finite"].append(np.isfinite(rec).all(1) & np.isfinite(tau).all(1) & (res["status"] == 0))
        log["touch"].append(res["touch"].copy())
        if record_tau:
            log["tau"].append(tau.copy())
    res = {k: np.stack(v) for k, v in log.items() if v}
    res["rec0"], res["rec"], res["dt"] = rec0, rec, par.dt_control
    return res


def summary(run, height=0.38, last=500):
    """Per robot: worst |height - desired|, worst |roll|, |pitch| over all ticks, and the mean
    forward speed over the last ``last`` ticks."""
    x = run["x"]
    speed = (x[-1] - x[-1 - last]) / (last * run["dt"])
    tilt = np.maximum(np.abs(run["roll"]), np.abs(run["pitch"])).max(0)
    return np.abs(run["height"] - height).max(0), tilt, speed


# ---- seeded single-tick states shared by tests/test_plant.py (the header on the host) and
# tests/test_gpu_plant.py (the device)

CASES = ("stance", "friction clamp", "release", "swing", "touchdown")


def make_states(B, seed, par=None, robot="aliengo"):
    """B seeded robots one tick long, every leg drawn from CASES: a stance leg whose reaction
    lies inside the cone, one whose reaction leaves it, one that pulls (released this tick), a
    leg in the air, a leg that lands this tick.  Returns dict(rec [B,STRIDE], tau [B,12] float32,
    robot [B,16] float32, geom [B,8], case [B,4])."""
    import os
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pympc-quadruped_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    from mpcqp.params import LEG_GEOMETRY, ROBOT_PRESETS, pack_leg_geometry, pack_robot
    par = par or Params()
    rng = np.random.default_rng(seed)
    geom = pack_leg_geometry(LEG_GEOMETRY[robot], B)
    rrec = np.tile(pack_robot(ROBOT_PRESETS[robot]), (B, 1)).astype(np.float32)
    case = rng.integers(0, len(CASES), (B, 4))
    case[0] = (0, 1, 2, 3)                                  # every case at least once in any batch
    case[-1] = (4, 0, 3, 1)
    rpy = rng.uniform([-0.1, -0.1, -3.0], [0.1, 0.1, 3.0], (B, 3))
    c, s = np.cos(rpy / 2), np.sin(rpy / 2)
    quat = np.stack([c[:, 0] * c[:, 1] * c[:, 2] + s[:, 0] * s[:, 1] * s[:, 2],
                     s[:, 0] * c[:, 1] * c[:, 2] - c[:, 0] * s[:, 1] * s[:, 2],
                     c[:, 0] * s[:, 1] * c[:, 2] + s[:, 0] * c[:, 1] * s[:, 2],
                     c[:, 0] * c[:, 1] * s[:, 2] - s[:, 0] * s[:, 1] * c[:, 2]], -1)
    pos = rng.uniform([-1, -1, 0.33], [1, 1, 0.38], (B, 3))
    pos[:, 2] += par.ground_z
    vel, omega = rng.uniform(-0.5, 0.5, (B, 3)), rng.uniform(-1, 1, (B, 3))
    Rq = _rot(quat)
    q0 = np.tile([0.0, 0.75, -1.5], (B, 4, 1)) + rng.uniform(-0.25, 0.25, (B, 4, 3))
    p, _, _ = kin_ref.chain(geom, q0.reshape(B, 12))
    feet = pos[:, None] + np.einsum("brc,blc->blr", Rq, p)
    h = par.dt_control / par.substeps
    contact = case <= 2
    fvel = np.where(contact[..., None], 0.0, rng.uniform(-1, 1, (B, 4, 3)))
    drop = rng.uniform(0.2, 1.0, (B, 4))                    # a landing foot: 0.3 .. 0.7 of a substep above the plane
    fvel[..., 2] = np.where(case == 4, -drop, fvel[..., 2])
    feet[..., 2] = np.where(contact, par.ground_z, np.where(case == 4, par.ground_z + rng.uniform(0.3, 0.7, (B, 4)) * h * drop,
                                                            par.ground_z + rng.uniform(0.01, 0.1, (B, 4))))
    rec = np.zeros((B, STRIDE))
    rec[:, POS:POS + 3], rec[:, QUAT:QUAT + 4], rec[:, VEL:VEL + 3], rec[:, OMEGA:OMEGA + 3] = pos, quat, vel, omega
    rec[:, FEET:FEET + 12], rec[:, FVEL:FVEL + 12] = feet.reshape(B, 12), fvel.reshape(B, 12)
    rec[:, CONTACT:CONTACT + 4] = contact
    rec[:, TICK] = rng.integers(0, 1000, B)
    # torques: J^T (-f) for the reaction wanted of a leg in contact, a small swing torque otherwise
    _, q, _, Ji = _leg_state(geom, Rq, pos, feet)
    _, _, Jb = kin_ref.chain(geom, q.reshape(B, 12))
    fz = rng.uniform(20, 70, (B, 4))
    ang = rng.uniform(0, 2 * np.pi, (B, 4))
    ratio = np.where(case == 1, rng.uniform(0.9, 1.6, (B, 4)), rng.uniform(0.0, 0.55, (B, 4)))   # mu = 0.7
    fz = np.where(case == 2, -rng.uniform(1, 30, (B, 4)), fz)
    f = np.stack([ratio * np.abs(fz) * np.cos(ang), ratio * np.abs(fz) * np.sin(ang), fz], -1)
    J = np.einsum("brk,blkc->blrc", Rq, Jb)
    tau = np.einsum("blcr,blc->blr", J, -f)
    tau = np.where(contact[..., None], tau, rng.uniform(-2, 2, (B, 4, 3)))
    return dict(rec=rec, tau=tau.reshape(B, 12).astype(np.float32), robot=rrec, geom=geom, case=case)


def near_threshold(rec, tau, robot, geom, par, plane=None):
    """[B] bool: the restatement places a decision of this tick within BAND of its threshold
    (n . f = 0, the cone edge, the plane)."""
    margins = []
    plant_step(rec.copy(), tau, robot, geom, par, plane, margins)
    return (np.min(np.stack(margins), 0) < BAND).any(-1)


def record_error(a, ref):
    """Norm-wise error per robot over the record's 41 real words (flag word and tick count are
    compared exactly by the callers), max|a - ref| / max|ref|."""
    a, ref = np.asarray(a)[:, :FLAGS], np.asarray(ref)[:, :FLAGS]
    return np.abs(a - ref).max(1) / np.maximum(np.abs(ref).max(1), 1e-300)


# ---- seeded sets off make_states' slice of the input space (tests/test_plant.py runs them through
# the host-compiled header, tests/test_gpu_plant_edges.py on the device): a mixed fleet on
# per-robot slopes, legs at the inverse kinematics' clamps, rotations slow enough for the small
# branch of quat_step

KINDS = ("hi", "lo", "low")
# the clamped legs of robot b: pattern b mod 17 -- every single leg once per kind, the two side
# pairs, the two diagonal pairs, all four: flag words 1, 2, 4, 8 (x 3), 5, 10, 6, 9, 15
CLAMP_WORDS = (1, 2, 4, 8) * 3 + (5, 10, 6, 9, 15)


def _presets():
    import os
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pympc-quadruped_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    from mpcqp import params
    return params


def fleet(B, robots=("a1", "aliengo")):
    """geom [B,8] and robot records [B,16] float32 of the presets taken in turn, robot by robot."""
    params = _presets()
    geom = np.stack([params.pack_leg_geometry(params.LEG_GEOMETRY[robots[b % len(robots)]]) for b in range(B)])
    rrec = np.stack([params.pack_robot(params.ROBOT_PRESETS[robots[b % len(robots)]]) for b in range(B)]).astype(np.float32)
    return geom, rrec


def _quat_mul(a, b):
    """a (x) b, (w, x, y, z)."""
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def _level_scene(rng, B, par, geom, mu, case):
    """make_states' draw on level ground with every length in units of the robot's own reach
    l_thigh + l_calf (Aliengo's 0.5 m gives make_states' ranges: base 0.33 .. 0.38 m over the
    ground, a swing foot 0.01 .. 0.1 m) and the cone ratio relative to its own mu: 1.2 .. 2.2
    of the cone for a friction clamp, below 0.8 of it otherwise.  Returns the level scene and
    the reaction f [B,4,3] wanted of a leg in contact."""
    reach = geom[:, 3] + geom[:, 4]
    rpy = rng.uniform([-0.1, -0.1, -3.0], [0.1, 0.1, 3.0], (B, 3))
    c, s = np.cos(rpy / 2), np.sin(rpy / 2)
    quat = np.stack([c[:, 0] * c[:, 1] * c[:, 2] + s[:, 0] * s[:, 1] * s[:, 2],
                     s[:, 0] * c[:, 1] * c[:, 2] - c[:, 0] * s[:, 1] * s[:, 2],
                     c[:, 0] * s[:, 1] * c[:, 2] + s[:, 0] * c[:, 1] * s[:, 2],
                     c[:, 0] * c[:, 1] * s[:, 2] - s[:, 0] * s[:, 1] * c[:, 2]], -1)
    pos = rng.uniform([-1, -1, 0.66], [1, 1, 0.76], (B, 3))
    pos[:, 2] = par.ground_z + pos[:, 2] * reach
    vel, omega = rng.uniform(-0.5, 0.5, (B, 3)), rng.uniform(-1, 1, (B, 3))
    q0 = np.tile([0.0, 0.75, -1.5], (B, 4, 1)) + rng.uniform(-0.25, 0.25, (B, 4, 3))
    p, _, _ = kin_ref.chain(geom, q0.reshape(B, 12))
    feet = pos[:, None] + np.einsum("brc,blc->blr", _rot(quat), p)
    h = par.dt_control / par.substeps
    contact = case <= 2
    fvel = np.where(contact[..., None], 0.0, rng.uniform(-1, 1, (B, 4, 3)))
    drop = rng.uniform(0.2, 1.0, (B, 4))                    # a landing foot: 0.3 .. 0.7 of a substep above the plane
    fvel[..., 2] = np.where(case == 4, -drop, fvel[..., 2])
    lift = np.where(contact, 0.0, np.where(case == 4, rng.uniform(0.3, 0.7, (B, 4)) * h * drop,
                                           rng.uniform(0.02, 0.2, (B, 4)) * reach[:, None]))
    feet[..., 2] = par.ground_z + lift
    fz = rng.uniform(20, 70, (B, 4))
    ang = rng.uniform(0, 2 * np.pi, (B, 4))
    ratio = mu[:, None] * np.where(case == 1, rng.uniform(1.2, 2.2, (B, 4)), rng.uniform(0.0, 0.8, (B, 4)))
    fz = np.where(case == 2, -rng.uniform(1, 30, (B, 4)), fz)
    f = np.stack([ratio * np.abs(fz) * np.cos(ang), ratio * np.abs(fz) * np.sin(ang), fz], -1)
    swing = rng.uniform(-2, 2, (B, 4, 3))
    tick = rng.integers(0, 1000, B)
    return dict(pos=pos, quat=quat, vel=vel, omega=omega, feet=feet, fvel=fvel, contact=contact, lift=lift, f=f,
                swing=swing, tick=tick)


def _records(sc, geom):
    """The records of a scene, and tau [B,12] float32: J^T (-f) for the reaction wanted of a leg
    in contact, the swing torque otherwise."""
    B = len(sc["pos"])
    rec = np.zeros((B, STRIDE))
    rec[:, POS:POS + 3], rec[:, QUAT:QUAT + 4] = sc["pos"], sc["quat"]
    rec[:, VEL:VEL + 3], rec[:, OMEGA:OMEGA + 3] = sc["vel"], sc["omega"]
    rec[:, FEET:FEET + 12], rec[:, FVEL:FVEL + 12] = sc["feet"].reshape(B, 12), sc["fvel"].reshape(B, 12)
    rec[:, CONTACT:CONTACT + 4] = sc["contact"]
    rec[:, TICK] = sc["tick"]
    Rq = _rot(sc["quat"])
    _, q, _, _ = _leg_state(geom, Rq, sc["pos"], sc["feet"])
    _, _, Jb = kin_ref.chain(geom, q.reshape(B, 12))
    J = np.einsum("brk,blkc->blrc", Rq, Jb)
    tau = np.where(sc["contact"][..., None], np.einsum("blcr,blc->blr", J, -sc["f"]), sc["swing"])
    return rec, tau.reshape(B, 12).astype(np.float32)


def _cases(rng, B):
    case = rng.integers(0, len(CASES), (B, 4))
    case[0] = (0, 1, 2, 3)                                  # every case at least once in any batch
    case[-1] = (4, 0, 3, 1)
    return case


def make_mixed_states(B, seed, par=None, tilt_max=0.3):
    """A mixed fleet on per-robot slopes: A1 and Aliengo robot by robot, the mass scaled by
    0.8 .. 1.2, mu in 0.4 .. 0.9, the inertia's off-diagonal words in +-2e-3, and each robot's
    own ground plane.  Every robot is drawn on level ground (_level_scene) and the whole scene
    is then turned rigidly about the origin by the rotation that takes z to the robot's normal
    (tilt 0.02 .. tilt_max rad, any azimuth): joint torques, n . f and the cone ratio are
    unchanged, so every leg keeps its case.  The plane (n, ground_z) is rounded to float32 first
    and every foot is then put at its height over the *rounded* plane, n . p - d with the float32
    words as they are, a contact foot at 0.  Returns make_states' dict plus plane [B,4] float32."""
    par = par or Params()
    rng = np.random.default_rng(seed)
    geom, rrec = fleet(B)
    rrec[:, 0] *= rng.uniform(0.8, 1.2, B).astype(np.float32)
    rrec[:, 7] = rng.uniform(0.4, 0.9, B)
    rrec[:, [2, 3, 5]] = rng.uniform(-2e-3, 2e-3, (B, 3))
    case = _cases(rng, B)
    sc = _level_scene(rng, B, par, geom, rrec[:, 7].astype(np.float64), case)
    tilt, az = rng.uniform(0.02, tilt_max, B), rng.uniform(0, 2 * np.pi, B)
    n = np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], -1)
    axis = np.stack([-np.sin(az), np.cos(az), np.zeros(B)], -1)                     # z x n, unit length
    qt = np.concatenate([np.cos(tilt / 2)[:, None], np.sin(tilt / 2)[:, None] * axis], -1)
    Rt = _rot(qt)
    assert np.abs(Rt[:, :, 2] - n).max() < 1e-15
    for k in ("pos", "vel", "omega"):
        sc[k] = _mv(Rt, sc[k])
    for k in ("feet", "fvel", "f"):
        sc[k] = np.einsum("brc,blc->blr", Rt, sc[k])
    sc["quat"] = _quat_mul(qt, sc["quat"])
    plane = np.concatenate([n, np.full((B, 1), par.ground_z)], 1).astype(np.float32)
    n32, d32 = plane[:, None, :3].astype(np.float64), plane[:, None, 3].astype(np.float64)
    for _ in range(2):
        s = np.sum(n32 * sc["feet"], -1) - d32
        sc["feet"] = sc["feet"] - ((s - sc["lift"]) / np.sum(n32 * n32, -1))[..., None] * n32
    rec, tau = _records(sc, geom)
    return dict(rec=rec, tau=tau, robot=rrec, geom=geom, case=case, plane=plane)


def make_clamped_states(B, seed, par=None):
    """A mixed fleet on level ground whose robot b has the legs of flag word
    CLAMP_WORDS[b mod 17] at a clamp of the inverse kinematics -- a single leg (the first twelve
    patterns) at the clamp of kind KINDS[(b mod 17) // 4], the legs of a pair or all four at
    KINDS[(b + leg) mod 3]:
      hi   the foot 0.2 m beyond the stretched leg, held out level ahead of the hip
      lo   the foot 0.4 |l_thigh - l_calf| from the thigh joint, inside the folded leg's reach
           (every calf is shortened to 0.9 of its preset: with equal links the folded leg reaches
           the thigh joint itself, and only a foot within 1e-14 m of it is clamped)
      low  the foot half the thigh offset from the hip axis, inside the hip's cylinder
    A clamped leg is free, at rest and carries exactly zero torque (J_b^-1 is near 1e14 there:
    with zero torque its force on the body is exactly zero on any build); the other legs carry
    make_states' cases.  ``feet_ok`` [B,4,3] are the feet of the ordinary draw, within reach.
    Returns make_states' dict plus word [B] (the flag word wanted), kind [B,4] and feet_ok."""
    par = par or Params()
    rng = np.random.default_rng(seed)
    geom, rrec = fleet(B)
    geom[:, 4] *= 0.9
    case = _cases(rng, B)
    sc = _level_scene(rng, B, par, geom, rrec[:, 7].astype(np.float64), case)
    word = np.array([CLAMP_WORDS[b % len(CLAMP_WORDS)] for b in range(B)])
    bit = (word[:, None] >> np.arange(4)) & 1 != 0
    pat = np.arange(B) % len(CLAMP_WORDS)
    kind = np.where(pat[:, None] < 12, pat[:, None] // 4, (np.arange(B)[:, None] + np.arange(4)) % 3)
    g = geom
    l1, l2, d = g[:, 3:4], g[:, 4:5], kin_ref.SY * g[:, 2:3]
    q1 = rng.uniform(-0.3, 0.3, (B, 4))
    q2 = -kin_ref.SX * rng.uniform(1.3, 1.5, (B, 4))          # the leg held out level, away from the body
    q = np.stack([q1, q2, np.zeros((B, 4))], -1)
    p, pth, _ = kin_ref.chain(g, q.reshape(B, 12))
    u = (p - pth) / (l1 + l2)[..., None]                      # unit length, in the leg's plane
    hip = np.stack([kin_ref.SX * g[:, 0:1], kin_ref.SY * g[:, 1:2] + 0 * q1, 0 * q1], -1)
    target = np.where((kind == 0)[..., None], pth + (l1 + l2 + 0.2)[..., None] * u,
                      np.where((kind == 1)[..., None], pth + (0.4 * np.abs(l1 - l2))[..., None] * u,
                               hip + np.stack([-0.3 * kin_ref.SX * (l1 + l2), 0.5 * d * np.cos(q1), 0.5 * d * np.sin(q1)], -1)))
    world = sc["pos"][:, None] + np.einsum("brc,blc->blr", _rot(sc["quat"]), target)
    feet_ok = sc["feet"].copy()
    sc["feet"] = np.where(bit[..., None], world, sc["feet"])
    sc["fvel"] = np.where(bit[..., None], 0.0, sc["fvel"])
    sc["contact"] = sc["contact"] & ~bit
    sc["swing"] = np.where(bit[..., None], 0.0, sc["swing"])
    rec, tau = _records(sc, geom)
    case = np.where(bit, -1, case)
    return dict(rec=rec, tau=tau, robot=rrec, geom=geom, case=case, word=word, kind=kind, clamped=bit, feet_ok=feet_ok)


def make_slow_states(B, seed, par=None):
    """Rotations slow enough for the small branch of quat_step, |h w*| < 1e-6.  An ordinary
    torque turns a robot far faster within one tick (h^2 I^-1 M is near 1e-4 rad), so three
    quarters of the set are built for it, robot b by b mod 4:
      0     at rest: omega exactly 0, a level body turned about z alone, the symmetric stand (every
            leg at (0, 0.7, -1.4)) with all four legs in stance under equal vertical reactions
            m g / 4 -- b mod 8 == 4: under no torque at all, where every force and moment is
            exactly zero and |h w*| is exactly 0 on any build
      1, 2  in the air: make_states' robot with every leg free, omega and the torques scaled by
            1e-4: |h w*| near 1e-7, the small branch with a rotation that is not zero
      3     make_states' robot with omega scaled by 1e-4: the large branch
    Returns make_states' dict plus still [B] and zero [B] (b mod 4 == 0, b mod 8 == 4)."""
    par = par or Params()
    rng = np.random.default_rng(seed)
    geom, rrec = fleet(B, robots=("aliengo",))
    case = _cases(rng, B)
    kind = np.arange(B) % 4
    case[(kind == 1) | (kind == 2)] = 3
    case[kind == 0] = 0
    sc = _level_scene(rng, B, par, geom, rrec[:, 7].astype(np.float64), case)
    sc["omega"] *= 1e-4
    air = (kind == 1) | (kind == 2)
    sc["swing"][air] *= 1e-4
    still = kind == 0
    ns = int(still.sum())
    yaw = np.array([[1.0, 0, 0, 0], [0, 0, 0, 1.0], [0.6, 0, 0, 0.8], [0.8, 0, 0, -0.6]])[np.arange(ns) % 4]
    root, dofs = stand_pose(ns, geom[still], par)
    sc["quat"][still], sc["omega"][still], sc["vel"][still] = yaw, 0.0, 0.0
    sc["pos"][still, 2] = root[:, 2].astype(np.float64)
    p, _, _ = kin_ref.chain(geom[still], dofs[:, :, 0])
    sc["feet"][still] = sc["pos"][still][:, None] + np.einsum("brc,blc->blr", _rot(yaw), p)
    sc["f"][still] = np.array([0.0, 0.0, 1.0]) * (rrec[still, 0].astype(np.float64) * par.gravity / 4)[:, None, None]
    rec, tau = _records(sc, geom)
    zero = np.arange(B) % 8 == 4
    tau[zero] = 0.0
    return dict(rec=rec, tau=tau, robot=rrec, geom=geom, case=case, still=still, zero=zero)


def trace_step(rec, tau, robot, geom, par, plane=None):
    """What the restatement decides in one tick, per substep: a list of dicts with pinned, over
    (the cone clamp), release, land [B,4] bool and t [B] = |h w*|, the turn of quat_step.  rec is
    left as it is."""
    trace = []
    plant_step(rec.copy(), tau, robot, geom, par, plane, trace=trace)
    return trace

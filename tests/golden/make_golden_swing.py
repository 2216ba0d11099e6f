"""Generate tests/golden/swing.npz FROM THE REFERENCE ITSELF (see make_golden.py: runs
only where the reference tree is present).

One robot per Gait member is driven for T control iterations through the reference's
own Gait, SwingFootTrajectoryGenerator and LegController objects, exactly as the loop
body of scripts/isaacgym_a1.py:137-162 drives them, with a plain attribute object in
place of RobotData.  iteration_between_mpc = 4 (set before gait is imported: Gait
captures it when the Enum is created), dt_control = 0.001.

pydrake is not importable here: the PiecewisePolynomial the generator asks for is a
stand-in whose CubicHermite is scipy.interpolate.CubicHermiteSpline and whose value /
derivative(1).value clamp to the break range as Drake's do.  The cubic Hermite through
given values and derivatives is unique, so the stand-in differs from Drake by rounding
only.

Recorded: the per-tick inputs (float32, as the reference saw them), swing_state, both
swing-foot targets and the 12 torques per tick, and at every 8th tick the generators'
private state (remaining time, first-swing flag, init, final) in float64.  Robots 0-2
run with Kp_swing = 700 I, robots 3-5 with 200 I (robot_configs.py:36,55).

Gait.STANDING's swing state is 0 / 0 = nan at phase 0 (gait.py:116-119: swing duration
0), which LegController.update takes as "swing" (leg_controller.py:78) with zero
targets; the fixture records that as the reference produced it, the tests skip those
entries (deviations).

A second entry, tests/golden/swing_edges.npz, is the same run where swing.npz cannot
see a mistake: full, non-symmetric Kp_swing / Kd_swing (nine distinct entries each, two
gain groups), thigh positions with the z a hip angle gives them (per leg different), a
commanded body velocity with a z part, wider yaw rates and base tilts, and
LinearMpcConfig.gravity, LinearMpcConfig.dt_control and AliengoConfig.swing_height off
their defaults (the generators and the Gait members read them when they are constructed,
so they are set first); iteration_between_mpc = 2, every tick of two periods of the
16-segment gaits plus 4, the generators' state at every 2nd tick.  touchdown_z and
vel_gain are literals in the reference (swing_foot_trajectory_generator.py:116,120) and
stay what they are.  Each entry runs in a process of its own, because the Gait members
capture the constants when the module is imported.

Usage:  python tests/golden/make_golden_swing.py            (both files)
        python tests/golden/make_golden_swing.py edges      (one of: swing, edges)
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, stub_reference  # noqa: E402

# ibm: iteration_between_mpc; T: two periods of the 16-segment gaits plus a few ticks; check:
# the generators' private state is recorded every check-th tick
ENTRIES = {
    "swing": dict(out="swing.npz", ibm=4, T=136, check=8, seed=31337, edges=False),
    "edges": dict(out="swing_edges.npz", ibm=2, T=68, check=2, seed=27182, edges=True,
                  dt_control=0.002, gravity=3.72, swing_height=0.07),
}
# the two gain groups of the edges entry (robots 0-2, robots 3-5)
KP_EDGES = np.array([[[700.0, 92.0, -110.0], [-80.0, 640.0, 130.0], [150.0, -88.0, 760.0]],
                     [[200.0, -35.0, 28.0], [42.0, 230.0, -31.0], [-26.0, 55.0, 170.0]]])
KD_EDGES = np.array([[[20.0, 3.5, -2.5], [-4.0, 17.0, 2.4], [3.1, -2.8, 23.0]],
                     [[12.0, -1.9, 2.6], [1.5, 14.0, -3.3], [-2.1, 1.7, 9.0]]])


class _Curve:
    def __init__(self, spline, lo, hi):
        self._s, self._lo, self._hi = spline, lo, hi

    def value(self, t):
        return np.asarray(self._s(min(max(float(t), self._lo), self._hi))).reshape(-1, 1)

    def derivative(self, n):
        return _Curve(self._s.derivative(n), self._lo, self._hi)


class PiecewisePolynomial:
    @staticmethod
    def CubicHermite(breaks, samples, derivs):
        from scipy.interpolate import CubicHermiteSpline
        x = np.asarray(breaks, dtype=np.float64).reshape(-1)
        return _Curve(CubicHermiteSpline(x, np.asarray(samples, dtype=np.float64),
                                         np.asarray(derivs, dtype=np.float64), axis=1), x[0], x[-1])


class _RobotData:
    """The RobotData attributes set_foot_placement / compute_traj_swingfoot /
    LegController.update read (robot_data.py:59-190), set directly."""


def _signed(rng, lo, hi, size=None):
    """Magnitudes in [lo, hi] with a random sign: none of them near 0."""
    return rng.uniform(lo, hi, size) * rng.choice([-1.0, 1.0], size)


def main(entry):
    cfg = ENTRIES[entry]
    IBM, T, CHECK, edges = cfg["ibm"], cfg["T"], cfg["check"], cfg["edges"]
    sys.path.insert(0, f"{REF}/config")
    import linear_mpc_configs
    linear_mpc_configs.LinearMpcConfig.iteration_between_mpc = IBM
    for k in ("dt_control", "gravity"):
        if k in cfg:
            setattr(linear_mpc_configs.LinearMpcConfig, k, cfg[k])
    LinearMpcConfig, robot_configs, mpc, gait = stub_reference(16)
    if "swing_height" in cfg:
        robot_configs.AliengoConfig.swing_height = cfg["swing_height"]
    sys.modules["pydrake.all"].PiecewisePolynomial = PiecewisePolynomial
    try:
        import matplotlib.pyplot  # noqa: F401
    except ImportError:
        mpl = types.ModuleType("matplotlib")
        mpl.pyplot = types.ModuleType("matplotlib.pyplot")
        sys.modules.update({"matplotlib": mpl, "matplotlib.pyplot": mpl.pyplot})
    import kinematics
    import leg_controller
    import swing_foot_trajectory_generator as sftg

    members = list(gait.Gait)
    B = len(members)
    rng = np.random.default_rng(cfg["seed"])
    f32 = np.float32
    quat = np.zeros((B, T, 4), f32)
    pos = np.zeros((B, T, 3), f32)
    vel = np.zeros((B, T, 3), f32)
    pos_feet = np.zeros((B, T, 4, 3), f32)
    foot_pos_base = np.zeros((B, T, 4, 3), f32)
    foot_vel_base = np.zeros((B, T, 4, 3), f32)
    thighs = np.zeros((B, 4, 3), f32)
    jac = rng.standard_normal((B, 4, 3, 3)).astype(f32)
    u0 = rng.uniform(-40, 120, (B, 12)).astype(f32)
    v_body = np.zeros((B, 3))
    yaw_rate = np.zeros(B)
    if edges:
        kp, kd = np.repeat(KP_EDGES, 3, axis=0), np.repeat(KD_EDGES, 3, axis=0)      # [B,3,3]
    else:
        kp = np.array([700.0] * 3 + [200.0] * 3)
        kd = np.full(B, 20.0)
    swing_state = np.zeros((B, T, 4))
    pos_target = np.zeros((B, T, 4, 3))
    vel_target = np.zeros((B, T, 4, 3))
    tau = np.zeros((B, T, 12), f32)
    nck = (T + CHECK - 1) // CHECK
    ck_remaining = np.zeros((B, nck, 4))
    ck_first = np.zeros((B, nck, 4), bool)
    ck_init = np.zeros((B, nck, 4, 3))
    ck_final = np.zeros((B, nck, 4, 3))
    sign = np.array([[1, 1], [1, -1], [-1, 1], [-1, -1]], float)
    priv = "_SwingFootTrajectoryGenerator__"
    for b, member in enumerate(members):
        v_body[b] = [rng.uniform(-0.5, 1.5), rng.uniform(-0.4, 0.4), 0.0]
        yaw_rate[b] = rng.uniform(-0.8, 0.8)
        thighs[b] = np.c_[0.24 * sign[:, 0], 0.134 * sign[:, 1], np.zeros(4)]
        rpy0 = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.15, 0.15), rng.uniform(-3.1, 3.1)])
        p0 = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), 0.38])
        ph = rng.uniform(0, 6.28, (4, 3))
        if edges:
            # what BatchedController.step feeds and swing.npz leaves at zero or small: thigh z =
            # d sin(q_hip), a commanded z velocity, a yaw rate and a tilt well away from 0
            v_body[b][2] = _signed(rng, 0.3, 0.6)
            yaw_rate[b] = _signed(rng, 1.0, 2.5)
            thighs[b, :, 2] = _signed(rng, 0.02, 0.08, 4)
            rpy0[:2] = _signed(rng, 0.2, 0.35, 2)
            lc = leg_controller.LegController(kp[b].copy(), kd[b].copy())
        else:
            lc = leg_controller.LegController(np.diag([kp[b]] * 3), np.diag([kd[b]] * 3))
        gens = [sftg.SwingFootTrajectoryGenerator(leg) for leg in range(4)]
        jv = np.zeros((4, 3, 18), f32)
        for leg in range(4):
            jv[leg, :, 6 + 3 * leg:9 + 3 * leg] = jac[b, leg]
        for t in range(T):
            # a wobbling, yawing, drifting base (as make_golden.gen_planner) and moving feet
            r, p, y = rpy0 + np.array([0.05 * np.sin(0.3 * t), 0.04 * np.cos(0.2 * t), 0.02 * t])
            cr, sr, cp, sp, cy, sy = np.cos(r / 2), np.sin(r / 2), np.cos(p / 2), np.sin(p / 2), \
                np.cos(y / 2), np.sin(y / 2)
            quat[b, t] = [cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy,
                          cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy]
            pos[b, t] = p0 + np.array([0.001 * t * v_body[b][0], 0.001 * t * v_body[b][1], 0.01 * np.sin(0.4 * t)])
            vel[b, t] = [v_body[b][0] + rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-.1, .1)]
            rd = _RobotData()
            rd.pos_base = pos[b, t]
            rd.lin_vel_base = vel[b, t]
            rd.R_base = kinematics.quat2matrix(quat[b, t])      # robot_data.py:75
            foot_pos_base[b, t] = thighs[b] + np.stack(
                [0.08 * np.sin(0.15 * t + ph[:, 0]), 0.03 * np.cos(0.1 * t + ph[:, 1]),
                 -0.32 + 0.04 * np.sin(0.2 * t + ph[:, 2])], axis=1)
            foot_vel_base[b, t] = rng.uniform(-1.0, 1.0, (4, 3))
            pos_feet[b, t] = pos[b, t] + foot_pos_base[b, t] @ np.asarray(rd.R_base, f32).T
            rd.base_pos_base_thighs = [thighs[b, leg] for leg in range(4)]
            rd.pos_feet = [pos_feet[b, t, leg] for leg in range(4)]
            rd.base_pos_base_feet = [foot_pos_base[b, t, leg] for leg in range(4)]
            rd.base_vel_base_feet = [foot_vel_base[b, t, leg] for leg in range(4)]
            rd.Jv_feet = [jv[leg] for leg in range(4)]
            vel_base_des, yaw_turn_rate_des = v_body[b].copy(), float(yaw_rate[b])

            # ---- the loop body of isaacgym_a1.py:137-162
            member.set_iteration(IBM, t)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)   # STANDING: 0 / 0 at phase 0
                swing_states = member.get_swing_state()
                pos_targets = np.zeros((4, 3))
                vel_targets = np.zeros((4, 3))
                for leg in range(4):
                    if swing_states[leg] > 0:
                        gens[leg].set_foot_placement(rd, member, vel_base_des, yaw_turn_rate_des)
                        pos_targets[leg], vel_targets[leg] = gens[leg].compute_traj_swingfoot(rd, member)
                    cmds = lc.update(rd, u0[b], swing_states, pos_targets, vel_targets)
            swing_state[b, t] = swing_states
            pos_target[b, t] = pos_targets
            vel_target[b, t] = vel_targets
            tau[b, t] = cmds
            if t % CHECK == 0:
                k = t // CHECK
                for leg, g in enumerate(gens):
                    ck_remaining[b, k, leg] = getattr(g, priv + "remaining_swing_time")
                    ck_first[b, k, leg] = getattr(g, priv + "is_first_swing")
                    ck_init[b, k, leg] = np.asarray(getattr(g, priv + "footpos_init"), float).reshape(3)
                    ck_final[b, k, leg] = np.asarray(getattr(g, priv + "footpos_final"), float).reshape(3)
    gait_rec = np.array([[m.num_segment, *m.stance_offsets, *m.stance_durations] for m in members], np.int32)
    out = os.path.join(HERE, cfg["out"])
    np.savez_compressed(
        out, member=np.array([m._name_ for m in members]), gait=gait_rec, iterations_between_mpc=IBM,
        dt_control=LinearMpcConfig.dt_control, gravity=float(LinearMpcConfig.gravity),
        swing_height=float(robot_configs.AliengoConfig.swing_height), touchdown_z=-0.0255, vel_gain=0.03,
        kp=kp, kd=kd, quat=quat, pos=pos, vel=vel, v_body=v_body, yaw_rate=yaw_rate, thighs=thighs,
        pos_feet=pos_feet, foot_pos_base=foot_pos_base, foot_vel_base=foot_vel_base, jac=jac, u0=u0,
        swing_state=swing_state, pos_target=pos_target,
        vel_target=vel_target, tau=tau, check_every=CHECK, ck_remaining=ck_remaining,
        ck_first=ck_first, ck_init=ck_init, ck_final=ck_final)
    nan = np.isnan(swing_state)
    print(f"{out}: {os.path.getsize(out)} bytes, B={B} T={T}, swing ticks per robot "
          f"{[(int((swing_state[b] > 0).sum())) for b in range(B)]}, nan swing states {int(nan.sum())} "
          f"(robots {sorted(set(np.nonzero(nan)[0].tolist()))}), re-arms at swing_state == 1: "
          f"{int((swing_state == 1.0).sum())}")


if __name__ == "__main__":
    if len(sys.argv) > 1:
        main(sys.argv[1])
    else:
        import subprocess
        for name in ENTRIES:
            subprocess.run([sys.executable, os.path.abspath(__file__), name], check=True)

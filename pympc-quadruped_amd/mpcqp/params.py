"""Problem constants and per-robot parameter packing.

Constants restate the reference's configuration classes:
  LinearMpcConfig  -- config/linear_mpc_configs.py:4-24 (Q, R, mu, g, horizon)
  AliengoConfig    -- config/robot_configs.py:44-60
  A1Config         -- config/robot_configs.py:63-79 (inertia x10 at :73)
  dt = 0.05        -- hard-coded in ModelPredictiveController (mpc.py:38)
Gaits restate linear_mpc/gait.py:16-22 (+ the commented BOUNDING8 at :20).
"""
import numpy as np

# state weights: r, p, y, x, y, z, wx, wy, wz, vx, vy, vz, g   (linear_mpc_configs.py:19)
Q_DIAG = (5., 5., 10., 10., 10., 50., 0.01, 0.01, 0.2, 0.2, 0.2, 0.2, 0.)
R_DIAG = (1e-5,) * 12                                          # linear_mpc_configs.py:20
DT_MPC = 0.05                                                  # mpc.py:38
GRAVITY = 9.81                                                 # linear_mpc_configs.py:13
MU = 0.7                                                       # linear_mpc_configs.py:15

# per-robot parameter record (float32 x ROBOT_STRIDE), consumed by the kernel
ROBOT_STRIDE = 16
R_MASS, R_IXX, R_IXY, R_IXZ, R_IYY, R_IYZ, R_IZZ, R_MU, R_FZMAX, R_NX, R_NY, R_NZ = range(12)


def _inertia(ixx, ixy, ixz, iyy, iyz, izz, scale=1.0):
    # make_com_inertial_matrix (utils/dynamics.py:3-18) stores float32; A1 scales
    # the float32 matrix by 10 in float32 (robot_configs.py:73)
    m = np.array([ixx, ixy, ixz, iyy, iyz, izz], dtype=np.float32)
    return m * np.float32(scale) if scale != 1.0 else m


ROBOT_PRESETS = {
    "aliengo": dict(mass=9.042, height=0.38, fz_max=500.0, mu=MU,
                    inertia=_inertia(0.033260231, -0.000451628, 0.000487603,
                                     0.16117211, 4.8356e-05, 0.17460442)),
    "a1": dict(mass=4.713, height=0.42, fz_max=500.0, mu=MU,
               inertia=_inertia(0.01683993, 8.3902e-05, 0.000597679,
                                0.056579028, 2.5134e-05, 0.064713601, scale=10)),
}

# swing constants: swing_height, Kp_swing, Kd_swing (diagonal)   robot_configs.py:35-37,54-56
SWING_PRESETS = {"aliengo": dict(swing_height=0.1, kp=200.0, kd=20.0),
                 "a1": dict(swing_height=0.1, kp=700.0, kd=20.0)}

# hip x offset, hip y + thigh y offset (a1.urdf:90,212,254; aliengo.urdf:99,254,297)
HIP_OFFSETS = {"a1": (0.183, 0.047 + 0.08505), "aliengo": (0.2399, 0.051 + 0.083)}

# leg geometry (hip_x, hip_y, thigh_y, l_thigh, l_calf): the xyz of the FL hip, thigh, calf
# and foot joints (a1.urdf:212,254,282,310; aliengo.urdf:254,297,326,355); the other legs
# mirror it (x sign + + - -, y sign + - + - for FL, FR, RL, RR)
LEG_GEOMETRY = {"a1": (0.183, 0.047, 0.08505, 0.2, 0.2), "aliengo": (0.2399, 0.051, 0.083, 0.25, 0.25)}
KIN_STRIDE = 8      # MPCQP_KIN_STRIDE: float64 geometry record per robot
PLANT_STRIDE = 48   # MPCQP_PLANT_STRIDE: float64 plant record per robot (mpcqp_plant_abi.h)
LEG_NAMES = ("FL", "FR", "RL", "RR")
LEG_SIGNS = ((1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0))

# name: (period, stance offsets, stance durations)    linear_mpc/gait.py:16-22
GAITS = {
    "standing": (16, (0, 0, 0, 0), (16, 16, 16, 16)),
    "trot16": (16, (0, 8, 8, 0), (8, 8, 8, 8)),
    "trot10": (10, (0, 5, 5, 0), (5, 5, 5, 5)),
    "jump16": (16, (0, 0, 0, 0), (4, 4, 4, 4)),
    "bound8": (8, (4, 4, 0, 0), (4, 4, 4, 4)),      # commented out at gait.py:20
    "pace16": (16, (8, 0, 8, 0), (8, 8, 8, 8)),
    "pace10": (10, (5, 0, 5, 0), (5, 5, 5, 5)),
}


# Gait enum member names (gait.py:16-22) -> GAITS keys
GAIT_MEMBERS = {"STANDING": "standing", "TROTTING16": "trot16", "TROTTING10": "trot10",
                "JUMPING16": "jump16", "PACING16": "pace16", "PACING10": "pace10", "BOUNDING8": "bound8"}


def gait_record(gait):
    """One MPCQP_GAIT_STRIDE record: [period, offsets[4], durations[4]] int32.

    ``gait`` is a GAITS key, a Gait enum member name, or a (period, offsets,
    durations) triple."""
    if isinstance(gait, str):
        period, offsets, durations = GAITS[GAIT_MEMBERS.get(gait, gait)]
    else:
        period, offsets, durations = gait
    rec = np.array([period, *offsets, *durations], dtype=np.int32)
    if rec.shape != (9,) or rec[0] <= 0:
        raise ValueError(f"bad gait {gait!r}")
    return rec


def pack_robot(preset, normal=(0.0, 0.0, 1.0), mu=None, fz_max=None):
    """One robot record: [mass, ixx, ixy, ixz, iyy, iyz, izz, mu, fz_max, nx, ny, nz, 0...]."""
    rec = np.zeros(ROBOT_STRIDE, dtype=np.float32)
    rec[R_MASS] = preset["mass"]
    rec[R_IXX:R_IZZ + 1] = preset["inertia"]
    rec[R_MU] = preset["mu"] if mu is None else mu
    rec[R_FZMAX] = preset["fz_max"] if fz_max is None else fz_max
    rec[R_NX:R_NZ + 1] = normal
    return rec


def pack_leg_geometry(geometry, batch=None):
    """MPCQP_KIN_STRIDE records (float64): [hip_x, hip_y, thigh_y, l_thigh, l_calf, 0, 0, 0].

    ``geometry`` is a LEG_GEOMETRY key, five numbers, or a [B,5] array (a mixed fleet).
    Returns [KIN_STRIDE] for one robot, [B, KIN_STRIDE] with ``batch`` (one record is
    repeated) or for a [B,5] array."""
    if isinstance(geometry, str):
        geometry = LEG_GEOMETRY[geometry]
    g = np.asarray(geometry, dtype=np.float64)
    if g.shape[-1:] != (5,) or g.ndim > 2 or not np.isfinite(g).all():
        raise ValueError("leg geometry: five finite numbers (hip_x, hip_y, thigh_y, l_thigh, l_calf) per robot")
    rec = np.zeros(g.shape[:-1] + (KIN_STRIDE,), dtype=np.float64)
    rec[..., :5] = g
    if batch is not None:
        if rec.ndim == 1:
            rec = np.tile(rec, (int(batch), 1))
        elif rec.shape[0] != int(batch):
            raise ValueError(f"leg geometry: expected one record or {batch}, got {rec.shape[0]}")
    return np.ascontiguousarray(rec)


def leg_geometry_from_urdf(path):
    """(hip_x, hip_y, thigh_y, l_thigh, l_calf) from a URDF file, read from the FL chain
    ``FL_hip_joint`` -> ``FL_thigh_joint`` -> ``FL_calf_joint`` -> ``FL_foot_fixed``.

    Raises ValueError unless all four legs have the topology the kinematics kernel
    assumes: hip / thigh / calf revolute about x / y / y, the foot fixed, every joint rpy
    zero, and the offsets of FR, RL, RR the mirror images of FL's."""
    import xml.etree.ElementTree as ET
    joints = {j.get("name"): j for j in ET.parse(path).getroot().iter("joint") if j.get("type") is not None}

    def vec(text, what):
        v = [float(x) for x in (text or "0 0 0").split()]
        if len(v) != 3:
            raise ValueError(f"{what}: expected three numbers, got {text!r}")
        return v

    def read(leg, part, axis):
        name = f"{leg}_{part}"
        j = joints.get(name)
        if j is None:
            raise ValueError(f"{path}: no joint {name}")
        origin = j.find("origin")
        xyz = vec(origin.get("xyz") if origin is not None else None, name + " xyz")
        rpy = vec(origin.get("rpy") if origin is not None else None, name + " rpy")
        if any(r != 0.0 for r in rpy):
            raise ValueError(f"{name}: joint rpy {rpy} is not zero")
        if axis is None:
            if j.get("type") != "fixed":
                raise ValueError(f"{name}: expected a fixed joint, got {j.get('type')}")
        else:
            ax = j.find("axis")
            got = vec(ax.get("xyz") if ax is not None else "1 0 0", name + " axis")   # URDF's default axis
            if j.get("type") not in ("revolute", "continuous") or got != axis:
                raise ValueError(f"{name}: expected a revolute joint about {axis}, got {j.get('type')} about {got}")
        return xyz

    chains = {}
    for leg in LEG_NAMES:
        chains[leg] = (read(leg, "hip_joint", [1.0, 0.0, 0.0]), read(leg, "thigh_joint", [0.0, 1.0, 0.0]),
                       read(leg, "calf_joint", [0.0, 1.0, 0.0]), read(leg, "foot_fixed", None))
    hip, thigh, calf, foot = chains["FL"]
    geom = (hip[0], hip[1], thigh[1], -calf[2], -foot[2])
    if hip[2] != 0.0 or thigh[0] != 0.0 or thigh[2] != 0.0 or calf[:2] != [0.0, 0.0] or foot[:2] != [0.0, 0.0]:
        raise ValueError(f"FL: joint offsets {chains['FL']} are not (x, y, 0), (0, y, 0), (0, 0, -l1), (0, 0, -l2)")
    if min(geom) <= 0.0:
        raise ValueError(f"FL: expected positive hip_x, hip_y, thigh_y and link lengths, got {geom}")
    for leg, (sx, sy) in zip(LEG_NAMES, LEG_SIGNS):
        want = ([sx * geom[0], sy * geom[1], 0.0], [0.0, sy * geom[2], 0.0], [0.0, 0.0, -geom[3]],
                [0.0, 0.0, -geom[4]])
        if chains[leg] != want:
            raise ValueError(f"{leg}: joint offsets {chains[leg]} do not mirror FL's {want}")
    return geom


def robot_from_config(robot_config, mu=MU, normal=(0.0, 0.0, 1.0)):
    """Pack a reference RobotConfig class (robot_configs.py:32-79) into a record."""
    I = np.asarray(robot_config.base_inertia_base, dtype=np.float32)
    preset = dict(mass=float(robot_config.mass_base), fz_max=float(robot_config.fz_max), mu=mu,
                  inertia=np.array([I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]],
                                   dtype=np.float32))
    return pack_robot(preset, normal=normal)

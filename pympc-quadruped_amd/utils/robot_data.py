"""Drop-in ``RobotData`` backed by the MI355X engine.

Same module name, class name, constructor and ``update`` signature as the reference's
``utils/robot_data.py`` (RobotData, robot_data.py:10-184), so that
``scripts/mujoco_aliengo.py`` and ``scripts/isaacgym_a1.py`` run unchanged after
``sys.path.append('../utils'); from robot_data import RobotData``.

What changes underneath: Pinocchio's forward kinematics and frame Jacobians
(robot_data.py:91-92,117-133) are one ``mpcqp_kinematics`` launch for B = 1 -- the closed
form of the hip-x / thigh-y / calf-y leg, with the five lengths read from the URDF by
``mpcqp.params.leg_geometry_from_urdf`` (which refuses any other leg).  One upload and one
readback per ``update``.  Nothing here imports pinocchio.

Behaviour kept from the reference:
  * the attributes its consumers read: pos_base, lin_vel_base, quat_base, ang_vel_base,
    R_base, rpy_base, q, qdot, pos_feet, pos_base_feet, base_pos_base_feet,
    base_vel_base_feet, base_pos_base_thighs (lists of four 3-vectors) and Jv_feet (four
    3 x 18 arrays: columns 0:3 = Rq, 3:6 = -Rq [p]x, the leg's block at 6 + 3 leg, zeros
    elsewhere -- Pinocchio's LOCAL_WORLD_ALIGNED layout, assembled on the host);
  * base_vel_base_feet multiplies those body-frame free-flyer columns by the world-frame
    lin_vel_base / ang_vel_base (robot_data.py:158-167; DESIGN.md, deviations);
  * ``state_estimation=True`` raises NotImplementedError in ``update`` (robot_data.py:80-81).

What differs: the measurements are taken as float32 (the dtype Isaac Gym's tensors have,
isaacgym_a1.py:121-132), so R_base = quat2matrix(quat_base) is in float32 arithmetic
whatever the caller passed.  base_Jv_feet, pos_thighs, X_base and the terrain-normal
methods have no caller in the reference and raise NotImplementedError.
"""
import math
import os
import sys

import numpy as np

_PKG = os.environ.get("MPCQP_PATH", os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from mpcqp.params import leg_geometry_from_urdf, pack_leg_geometry  # noqa: E402


def quat2ZYXangle(quat):
    """utils/kinematics.py:40-49 -- (w, x, y, z) -> [roll, pitch, yaw]."""
    q = np.asarray(quat).reshape(-1)
    roll = math.atan2(2 * (q[0] * q[1] + q[2] * q[3]), 1 - 2 * (q[1] ** 2 + q[2] ** 2))
    pitch = math.asin(2 * (q[0] * q[2] - q[3] * q[1]))
    yaw = math.atan2(2 * (q[0] * q[3] + q[1] * q[2]), 1 - 2 * (q[2] ** 2 + q[3] ** 2))
    return [roll, pitch, yaw]


def quat2matrix(quat):
    """utils/kinematics.py:51-71 -- (w, x, y, z) -> R, in the quaternion's own dtype."""
    q = np.asarray(quat).reshape(-1)
    return np.array([
        [q[0]**2 + q[1]**2 - q[2]**2 - q[3]**2, 2 * (q[1] * q[2] - q[0] * q[3]), 2 * (q[0] * q[2] + q[1] * q[3])],
        [2 * (q[0] * q[3] + q[1] * q[2]), q[0]**2 - q[1]**2 + q[2]**2 - q[3]**2, 2 * (q[2] * q[3] - q[0] * q[1])],
        [2 * (q[1] * q[3] - q[0] * q[2]), 2 * (q[0] * q[1] + q[2] * q[3]), q[0]**2 - q[1]**2 - q[2]**2 + q[3]**2]])


def _free_flyer_rotation(quat):
    """Eigen's quaternion-to-matrix formula in float64 on (w, x, y, z) as given: the
    rotation Pinocchio's free-flyer joint uses (robot_data.py:85-92)."""
    w, x, y, z = (float(v) for v in quat)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def _skew(p):
    return np.array([[0.0, -p[2], p[1]], [p[2], 0.0, -p[0]], [-p[1], p[0], 0.0]])


# float32 offsets of the upload (quat, pos, vel, omega, R_base, q, qdot) and of the readback
_IN = dict(quat=(0, 4), pos=(4, 7), vel=(7, 10), omega=(10, 13), rot=(13, 22), q=(22, 34), qdot=(34, 46))
_OUT = dict(feet=(0, 12), thighs=(12, 24), pos_feet=(24, 36), foot_pos_base=(36, 48), foot_vel_base=(48, 60),
            jac=(60, 96))


class RobotData():

    def __init__(self, robot_model, state_estimation=False):
        self.state_estimation = state_estimation
        self.leg_geometry = leg_geometry_from_urdf(robot_model)
        self._engine = None

    def _get_engine(self):
        if self._engine is None:
            import torch
            from mpcqp import LinearMpc
            e = LinearMpc(horizon=1, device=os.environ.get("MPCQP_DEVICE", "cuda:0"))
            self._geom = torch.as_tensor(pack_leg_geometry(self.leg_geometry, 1)).to(e.device)
            self._in_host = torch.zeros((46,), dtype=torch.float32, pin_memory=True)
            self._out_host = torch.zeros((96,), dtype=torch.float32, pin_memory=True)
            self._in_dev = torch.zeros((46,), dtype=torch.float32, device=e.device)
            self._out_dev = torch.zeros((96,), dtype=torch.float32, device=e.device)
            i = {k: self._in_dev[a:b] for k, (a, b) in _IN.items()}
            o = {k: self._out_dev[a:b] for k, (a, b) in _OUT.items()}
            self._launch = e.bind_kinematics(self._geom, i["quat"], i["pos"], i["vel"], i["omega"], i["rot"], i["q"],
                                             i["qdot"], **o)
            self._engine = e
        return self._engine

    def update(self, pos_base, lin_vel_base, quat_base, ang_vel_base, q, qdot):
        if self.state_estimation:
            raise NotImplementedError
        f4 = lambda a, n: np.asarray(a, dtype=np.float32).reshape(n)
        self.pos_base = f4(pos_base, 3)
        self.lin_vel_base = f4(lin_vel_base, 3)
        self.quat_base = f4(quat_base, 4)
        self.ang_vel_base = f4(ang_vel_base, 3)
        self.R_base = quat2matrix(self.quat_base)                  # robot_data.py:75
        self.rpy_base = np.array(quat2ZYXangle(self.quat_base))    # :76
        self.q = f4(q, 12)
        self.qdot = f4(qdot, 12)

        import torch
        e = self._get_engine()
        h = self._in_host.numpy()
        for k, v in (("quat", self.quat_base), ("pos", self.pos_base), ("vel", self.lin_vel_base),
                     ("omega", self.ang_vel_base), ("rot", self.R_base.reshape(9)), ("q", self.q),
                     ("qdot", self.qdot)):
            h[_IN[k][0]:_IN[k][1]] = v
        stream = torch.cuda.current_stream(e.device)
        self._in_dev.copy_(self._in_host, non_blocking=True)
        self._launch(stream)
        self._out_host.copy_(self._out_dev, non_blocking=True)
        stream.synchronize()
        out = self._out_host.numpy().astype(np.float64)
        rows = lambda k: [r.copy() for r in out[_OUT[k][0]:_OUT[k][1]].reshape(4, 3)]
        self.pos_feet = rows("pos_feet")                           # :99
        self.pos_base_feet = rows("feet")                          # :101
        self.base_pos_base_feet = rows("foot_pos_base")            # :103
        self.base_vel_base_feet = rows("foot_vel_base")            # :104
        self.base_pos_base_thighs = rows("thighs")                 # :108
        # Jv_feet (:117-133) from the device's blocks: the free-flyer columns are Rq and
        # -Rq [p]x with p the foot in the base frame, p = Rq^-1 (Rq p)
        Rq = _free_flyer_rotation(self.quat_base)
        jac = out[_OUT["jac"][0]:_OUT["jac"][1]].reshape(4, 3, 3)
        self.Jv_feet = []
        for leg in range(4):
            Jv = np.zeros((3, 18))
            Jv[:, 0:3] = Rq
            Jv[:, 3:6] = -Rq @ _skew(np.linalg.solve(Rq, self.pos_base_feet[leg]))
            Jv[:, 6 + 3 * leg:9 + 3 * leg] = jac[leg]
            self.Jv_feet.append(Jv)

    def _no_caller(self, name):
        raise NotImplementedError(f"RobotData.{name} has no caller in the reference and is not provided")

    @property
    def base_Jv_feet(self):
        self._no_caller("base_Jv_feet")

    @property
    def pos_thighs(self):
        self._no_caller("pos_thighs")

    @property
    def X_base(self):
        self._no_caller("X_base")

    def init_contact_history(self):
        self._no_caller("init_contact_history")

    def update_terrain_normal(self, cur_contact_state):
        self._no_caller("update_terrain_normal")

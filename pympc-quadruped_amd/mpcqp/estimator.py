"""Batched base-state estimator on the device: the sensor side of the control loop.

``BatchedEstimator`` is B copies of the Kalman filter the reference derives in
doc/state_estimation_kf.md (second stage, after MIT Cheetah 3) and leaves unbuilt
(``RobotData.update`` raises NotImplementedError for ``state_estimation=True``): it fuses
the accelerometer with the leg kinematics of the feet in contact, from the sensor set
scripts/mujoco_aliengo.py:101-118 collects, in one HIP launch per control iteration
(include/mpcqp.h mpcqp_estimate).  Its output is a root-state tensor in the simulator's
layout, so

    root = est.update(quat, gyro, accel, dof_states, trust)
    tau = ctl.step(it, v_des, yaw_rate, root, dof_states)

closes the loop for a caller who has the orientation and the contact trust.  A caller with
the raw sensors -- gyro, accelerometer, joint encoders and the gait clock or a touch sensor --
uses

    root = est.update_from_imu(gyro, accel, dof_states, tick=it)
    tau = ctl.step(it, v_des, yaw_rate, root, dof_states)

which runs the doc's first stage (the orientation filter) and the stance-phase trust ramp in
one more launch ahead of the filter (include/mpcqp.h mpcqp_attitude), so that nothing is
computed on the host.
"""
import numpy as np
import torch

from ._lib import ATT_STRIDE, EST_STRIDE
from .engine import LinearMpc
from .params import LEG_GEOMETRY, gait_record, pack_leg_geometry

NX = 18        # x = [p_b, v_b, p_1 .. p_4]
_INIT = 18     # the record's `initialised` word
_P = 24        # P[18][18], row-major
_ATT_INIT = 4  # the orientation record's `initialised` word (q at 0, gyro bias at 5)


class BatchedEstimator:
    """Args:
      batch:    number of robots B
      robot:    preset name, used for the leg geometry and for an engine of its own
      geometry: leg geometry: a LEG_GEOMETRY key, (hip_x, hip_y, thigh_y, l_thigh, l_calf)
                or a [B,5] array for a mixed fleet; default the robot preset's
      engine:   a LinearMpc to share (``BatchedController.engine``), so that estimator and
                controller run on one context; default a new one on ``device``
      controller: a BatchedController: ``update_from_imu`` takes its gait records and its
                iterations_between_mpc for the contact trust, and its engine is shared unless
                ``engine`` is given
      attitude: constants of ``update_from_imu``'s orientation filter and trust, any of
                LinearMpc.set_attitude's (kappa_ref, bias_gain, trust_window, touch_threshold,
                dt, gravity); dt and gravity default to the estimator's
      constants: any of LinearMpc.set_estimator's (dt, gravity, sigma_p, sigma_v, sigma_f,
                r_p, r_v, r_z, suspicion, p0, contact_height); they are the engine's, so
                a shared engine has one set
    """

    def __init__(self, batch, robot="a1", geometry=None, device="cuda:0", engine=None, controller=None,
                 attitude=None, **constants):
        self.B = int(batch)
        if geometry is None:
            if not (isinstance(robot, str) and robot in LEG_GEOMETRY):
                raise ValueError("no leg geometry: pass geometry= (params.LEG_GEOMETRY, leg_geometry_from_urdf)")
            geometry = robot
        if engine is None and controller is not None:
            engine = controller.engine
        self.engine = engine if engine is not None else LinearMpc(robot=robot, device=device)
        if constants or not hasattr(self.engine, "estimator_constants"):
            self.engine.set_estimator(**constants)
        if attitude or not hasattr(self.engine, "attitude_constants"):
            c = self.engine.estimator_constants
            self.engine.set_attitude(**dict(dict(dt=c["dt"], gravity=c["gravity"]), **(attitude or {})))
        dev = self.engine.device
        self.device = dev
        B = self.B
        self.geometry = torch.as_tensor(pack_leg_geometry(geometry, B)).to(dev)
        if self.geometry.shape[0] != B:
            raise ValueError(f"expected {B} geometry records, got {self.geometry.shape[0]}")
        self.est_state = torch.zeros((B, EST_STRIDE), dtype=torch.float64, device=dev)
        self.root_states = torch.zeros((B, 13), dtype=torch.float32, device=dev)
        self.feet_world = torch.zeros((B, 4, 3), dtype=torch.float32, device=dev)
        self.status = torch.zeros((B,), dtype=torch.int32, device=dev)
        # update_from_imu: the orientation records and what the attitude launch hands to the filter
        self.att_state = torch.zeros((B, ATT_STRIDE), dtype=torch.float64, device=dev)
        self.quat = torch.zeros((B, 4), dtype=torch.float32, device=dev)
        self.gyro_corrected = torch.zeros((B, 3), dtype=torch.float32, device=dev)
        self.trust = torch.zeros((B, 4), dtype=torch.float32, device=dev)
        self.attitude_status = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.tick_count = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.gait = self.iterations_between_mpc = None
        if controller is not None:
            if controller.B != B:
                raise ValueError(f"the controller has {controller.B} robots, the estimator {B}")
            self.gait, self.iterations_between_mpc = controller.gait, controller.iterations_between_mpc

    def _f32(self, t, shape):
        t = torch.as_tensor(t)
        if not (t.dtype == torch.float32 and t.is_contiguous() and t.device == self.device):
            t = t.to(self.device, torch.float32).contiguous()
        if t.numel() != int(np.prod(shape)):
            raise ValueError(f"expected {list(shape)}, got {tuple(t.shape)}")
        return t

    def update(self, quat, gyro, accel, dof_states=None, trust=None, q=None, qdot=None):
        """One tick for every robot; returns root_states [B,13] (device, Isaac Gym layout).

        quat [B,4] (w, x, y, z), gyro / accel [B,3] in the body frame, trust [B,4] in [0, 1]
        (1 = foot in contact), and either dof_states [B,12,2] (or [B*12,2]) or q / qdot
        [B,12].  Also fills self.feet_world [B,4,3] and self.status [B]."""
        B = self.B
        if trust is None:
            raise ValueError("update: trust is required")
        if (dof_states is None) == (q is None) or (q is None) != (qdot is None):
            raise ValueError("update: give dof_states, or q and qdot")
        kw = dict(dof_states=self._f32(dof_states, (B, 12, 2))) if dof_states is not None else \
            dict(q=self._f32(q, (B, 12)), qdot=self._f32(qdot, (B, 12)))
        self.engine.estimate(self.est_state, self._f32(quat, (B, 4)), self._f32(gyro, (B, 3)),
                             self._f32(accel, (B, 3)), self._f32(trust, (B, 4)), self.geometry,
                             root_states=self.root_states, feet_world=self.feet_world, status=self.status, **kw)
        return self.root_states

    def _i32(self, t, shape):
        t = torch.as_tensor(t)
        if not (t.dtype == torch.int32 and t.is_contiguous() and t.device == self.device):
            t = t.to(self.device, torch.int32).contiguous()
        if t.numel() != int(np.prod(shape)):
            raise ValueError(f"expected {list(shape)}, got {tuple(t.shape)}")
        return t

    def update_from_imu(self, gyro, accel, dof_states=None, tick=None, gait=None, iterations_between_mpc=None,
                        touch=None, trust=None, q=None, qdot=None):
        """``update`` from the raw sensors: one launch of the orientation filter and the contact
        trust (LinearMpc.attitude) into self.quat, self.gyro_corrected, self.trust and
        self.attitude_status, then the filter's launch on those buffers; returns root_states
        [B,13].

        gyro / accel [B,3] in the body frame and dof_states (or q / qdot) as for ``update``.
        The trust comes from the gait clock -- ``tick``, the control-iteration counter of
        ``BatchedController.step`` (an int, or a [B] int32 device tensor), with ``gait`` ([B,9]
        int32 records, or one gait as params.gait_record takes it) and
        ``iterations_between_mpc``, both defaulting to the controller's given at construction
        -- and / or from ``touch`` [B,4], the touch sensor.  An explicit ``trust`` [B,4]
        bypasses the computed one."""
        B = self.B
        if (dof_states is None) == (q is None) or (q is None) != (qdot is None):
            raise ValueError("update_from_imu: give dof_states, or q and qdot")
        kw = dict(dof_states=self._f32(dof_states, (B, 12, 2))) if dof_states is not None else \
            dict(q=self._f32(q, (B, 12)), qdot=self._f32(qdot, (B, 12)))
        acc = self._f32(accel, (B, 3))
        att = dict(quat=self.quat, gyro_out=self.gyro_corrected, status=self.attitude_status)
        if trust is not None:
            trust = self._f32(trust, (B, 4))
        else:
            if gait is None:
                gait = self.gait
            elif not isinstance(gait, torch.Tensor):
                gait = np.tile(gait_record(gait), (B, 1))
            if gait is not None and tick is not None:
                ibm = self.iterations_between_mpc if iterations_between_mpc is None else iterations_between_mpc
                if ibm is None:
                    raise ValueError("update_from_imu: iterations_between_mpc is required with a gait")
                if isinstance(tick, torch.Tensor):
                    tk = self._i32(tick, (B,))
                else:
                    tk = self.tick_count.fill_(int(tick))
                att.update(tick=tk, gait=self._i32(gait, (B, 9)), iterations_between_mpc=int(ibm))
            elif touch is None:
                raise ValueError("update_from_imu: the trust needs tick and gait (or controller=), touch, or trust=")
            if touch is not None:
                att["touch"] = self._f32(touch, (B, 4))
            att["trust"] = trust = self.trust
        self.engine.attitude(self.att_state, self._f32(gyro, (B, 3)), acc, **att)
        self.engine.estimate(self.est_state, self.quat, self.gyro_corrected, acc, trust, self.geometry,
                             root_states=self.root_states, feet_world=self.feet_world, status=self.status, **kw)
        return self.root_states

    def reset(self, robots=None, pos=None, quat=None):
        """Zero the records of all or some robots: the next update starts them from x = 0,
        P = p0 I, and the next update_from_imu takes the orientation from the accelerometer.
        With ``pos`` ([3] or one row per robot reset) the base position is seeded
        and the record marked initialised, with P = diag(r_p 1_3, p0 1_15): the seeded
        position is trusted like one leg measurement, so the first update places the feet
        (variance p0) around it and not the base between the feet's zeros.  With ``quat``
        ([4] or one row per robot reset, (w, x, y, z)) the orientation record is seeded with
        it, normalised, and a zero gyro bias."""
        idx = slice(None) if robots is None else robots
        self.est_state[idx] = 0.0
        self.att_state[idx] = 0.0
        if quat is not None:
            n = self.att_state[idx].shape[0]
            rec = torch.zeros((n, ATT_STRIDE), dtype=torch.float64, device=self.device)
            qq = torch.as_tensor(quat, dtype=torch.float64).to(self.device).expand(n, 4)
            rec[:, 0:4] = qq / qq.norm(dim=1, keepdim=True)
            rec[:, _ATT_INIT] = 1.0
            self.att_state[idx] = rec
        if pos is not None:
            n = self.est_state[idx].shape[0]
            rec = torch.zeros((n, EST_STRIDE), dtype=torch.float64, device=self.device)
            rec[:, 0:3] = torch.as_tensor(pos, dtype=torch.float64).to(self.device)
            rec[:, _INIT] = 1.0
            c = self.engine.estimator_constants
            var = torch.full((NX,), float(c["p0"]), dtype=torch.float64, device=self.device)
            var[0:3] = float(c["r_p"])
            rec[:, _P:_P + NX * NX] = torch.diag(var).reshape(-1)
            self.est_state[idx] = rec

    @property
    def position(self):
        """p_b [B,3] float64, a view of the records."""
        return self.est_state[:, 0:3]

    @property
    def velocity(self):
        """v_b [B,3] float64, a view of the records."""
        return self.est_state[:, 3:6]

    @property
    def covariance(self):
        """P [B,18,18] float64, a view of the records."""
        return self.est_state[:, _P:_P + NX * NX].view(self.B, NX, NX)

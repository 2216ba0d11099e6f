"""Batched control tick on the device: the loop body the reference runs per robot.

``BatchedController`` is B copies of the reference's per-robot objects -- one
``Gait``, one ``ModelPredictiveController``, four ``SwingFootTrajectoryGenerator``s and
one ``LegController`` -- advanced together, so a whole fleet's control iteration is
four HIP launches on an MPC tick and three (kinematics, plan, leg_torques) on the
others, with every intermediate resident in HBM:

  mpcqp_kinematics      RobotData.update                             robot_data.py:59-108
  mpcqp_plan            Gait.set_iteration / get_gait_table          gait.py:76-100
                        ModelPredictiveController.update_robot_state mpc.py:55-79
                        update_mpc_if_needed integrators, X_ref      mpc.py:81-170
  mpcqp_solve           _solve_mpc on MPC ticks                      mpc.py:262-290
  mpcqp_leg_torques     Gait.get_swing_state                         gait.py:102-121
                        set_foot_placement, compute_traj_swingfoot
                                            swing_foot_trajectory_generator.py:38-129
                        LegController.update, both branches          leg_controller.py:75-90
  mpcqp_stance_torques  LegController stance branch alone            leg_controller.py:86-89

The per-robot Python loop it replaces is scripts/isaacgym_a1.py:117-162 (which
copies every robot's root state to the host, ``.cpu().numpy()``); ``tick`` and
``leg_torques`` take the simulator's root-state tensor as it lies on the device
(SURVEY §8 f3).  ``step`` is the whole loop body on the simulator's two state tensors,
with nothing computed by the caller; ``step_fused`` is the same tick, bit for bit, through
one C call (mpcqp_step: one launch on a tick between two solves).  ``tick`` and
``leg_torques`` remain for callers with kinematics of their own, ``torques`` for callers that
run their own swing controller.
"""
import numpy as np
import torch

from ._lib import PLAN_REFERENCE, PLAN_STRIDE, STEP_MPC, SWING_STRIDE
from .engine import LinearMpc
from .params import (DT_MPC, LEG_GEOMETRY, Q_DIAG, R_DIAG, ROBOT_PRESETS, SWING_PRESETS, gait_record,
                     pack_leg_geometry)


class BatchedController:
    """Args:
      batch:    number of robots B
      horizon:  MPC horizon N (linear_mpc_configs.py:11)
      robot:    preset name / RobotConfig class / packed record, or [B,16] records
      gait:     one gait (GAITS key, Gait member name, or (period, offsets, durations))
                or a list of B of them
      iterations_between_mpc: linear_mpc_configs.py:7 (20)
      dt_control: linear_mpc_configs.py:6 (0.001)
      height:   desired CoM height(s) (robot_configs.py:23,42); default from the preset
      warm_start: remember each robot's active set between MPC ticks (LinearMpc.set_warm_start)
      swing:    swing constants for ``leg_torques``: a dict with any of swing_height, Kp, Kd,
                touchdown_z, vel_gain (LinearMpc.set_swing).  Default: the robot preset's or the
                RobotConfig class's swing_height / Kp_swing / Kd_swing (robot_configs.py:35-37,
                54-56); a packed record carries none and gets the engine's defaults
      geometry: leg geometry for ``step``: a LEG_GEOMETRY key, (hip_x, hip_y, thigh_y, l_thigh,
                l_calf) or a [B,5] array for a mixed fleet (params.leg_geometry_from_urdf reads
                one from a URDF).  Default: the robot preset's; without a preset name and
                without geometry, ``step`` raises
    """

    def __init__(self, batch, horizon=16, robot="aliengo", gait="trot10", iterations_between_mpc=20,
                 dt_control=0.001, gravity=9.81, height=None, dt=DT_MPC, Q=Q_DIAG, R=R_DIAG,
                 device="cuda:0", max_iter=0, max_stance=0, warm_start=True, swing=None, geometry=None):
        self.B = int(batch)
        self.N = int(horizon)
        self.iterations_between_mpc = int(iterations_between_mpc)
        per_robot = not isinstance(robot, str) and np.ndim(robot) == 2
        self.engine = LinearMpc(horizon=self.N, robot=None if per_robot else robot, dt=dt, Q=Q, R=R,
                                device=device, max_iter=max_iter, max_stance=max_stance)
        self.engine.set_planner(dt_control=dt_control, gravity=gravity)
        if warm_start:   # the fleet is solved tick after tick: remember each robot's active set
            self.engine.set_warm_start(int(batch))
        if swing is None:
            if isinstance(robot, str):
                sw = SWING_PRESETS[robot]
                swing = dict(swing_height=sw["swing_height"], Kp=sw["kp"], Kd=sw["kd"])
            elif hasattr(robot, "Kp_swing"):
                swing = dict(swing_height=robot.swing_height, Kp=robot.Kp_swing, Kd=robot.Kd_swing)
        if swing:
            self.engine.set_swing(**swing)
        dev = self.engine.device
        self.device = dev
        B, N = self.B, self.N
        if per_robot:
            self.robot = torch.as_tensor(np.asarray(robot, dtype=np.float32)).to(dev).contiguous()
        else:
            rec = self.engine.default_robot
            self.robot = torch.as_tensor(np.tile(rec, (B, 1))).to(dev).contiguous()
        single = isinstance(gait, str) or (isinstance(gait, (tuple, list)) and len(gait) == 3
                                           and np.isscalar(gait[0]) and not isinstance(gait[0], str))
        gaits = [gait] * B if single else list(gait)
        if len(gaits) != B:
            raise ValueError(f"expected one gait or {B} of them, got {len(gaits)}")
        g = np.stack([gait_record(x) for x in gaits])
        self.gait = torch.as_tensor(g).to(dev).contiguous()
        self._period = self.gait[:, 0].clone()
        if height is None:
            if isinstance(robot, str):
                height = ROBOT_PRESETS[robot].get("height", 0.38)
            elif hasattr(robot, "base_height_des"):
                height = robot.base_height_des
            else:
                raise ValueError("height is required for a packed robot record")
        self.height = torch.as_tensor(np.broadcast_to(np.asarray(height, dtype=np.float32), (B,)).copy()).to(dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.plan_state = torch.zeros((B, PLAN_STRIDE), dtype=torch.float64, device=dev)
        self.x0 = torch.zeros((B, 13), **f32)
        self.xref = torch.zeros((B, N, 13), **f32)
        self.contact = torch.zeros((B, N, 4), **f32)
        self.u0 = torch.zeros((B, 12), **f32)
        self.tau = torch.zeros((B, 12), **f32)
        self.status = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.iterations = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.iteration = torch.zeros((B,), dtype=torch.int32, device=dev)
        # leg_torques: the swing generators' state, each robot's control-iteration counter
        # and the optional outputs
        self.swing_mem = torch.zeros((B, SWING_STRIDE), dtype=torch.float64, device=dev)
        self.tick_count = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.swing_state = torch.zeros((B, 4), **f32)
        self.pos_target = torch.zeros((B, 4, 3), **f32)
        self.vel_target = torch.zeros((B, 4, 3), **f32)
        # step: the leg geometry and the six outputs of the kinematics
        if geometry is None and isinstance(robot, str) and robot in LEG_GEOMETRY:
            geometry = robot
        self.geometry = None if geometry is None else torch.as_tensor(pack_leg_geometry(geometry, B)).to(dev)
        self.feet = torch.zeros((B, 4, 3), **f32)
        self.thighs = torch.zeros((B, 4, 3), **f32)
        self.pos_feet = torch.zeros((B, 4, 3), **f32)
        self.foot_pos_base = torch.zeros((B, 4, 3), **f32)
        self.foot_vel_base = torch.zeros((B, 4, 3), **f32)
        self.jac = torch.zeros((B, 4, 3, 3), **f32)

    def reset(self, robots=None):
        """First-run semantics again (mpc.py:56-60,84-87; first swing,
        swing_foot_trajectory_generator.py:19-24) for all or some robots."""
        if robots is None:
            self.plan_state.zero_()
            self.swing_mem.zero_()
        else:
            self.plan_state[robots] = 0.0
            self.swing_mem[robots] = 0.0

    def _f32(self, t):
        """``t`` as a contiguous float32 tensor on the device: ``t`` itself, with no copy, when
        it already is one."""
        if t.dtype == torch.float32 and t.is_contiguous() and t.device == self.device:
            return t
        return t.to(self.device, torch.float32).contiguous()

    def _cmd(self, v, shape):
        t = torch.as_tensor(v, dtype=torch.float64)
        return t.to(self.device).expand(shape).contiguous()

    def tick(self, iter_counter, vel_body_des, yaw_rate_des, feet, root_states=None, quat=None, pos=None,
             omega=None, vel=None, rot=None):
        """One control iteration for every robot; returns u0 [B,12] (device).

        The contact forces are re-solved when ``iter_counter % iterations_between_mpc
        == 0`` and held otherwise (mpc.py:95-106).  feet [B,4,3] are the foot positions
        relative to the CoM in the world frame (robot_data.pos_base_feet)."""
        B = self.B
        ibm = self.iterations_between_mpc
        mpc_tick = iter_counter % ibm == 0
        flags = PLAN_REFERENCE if mpc_tick else 0
        if mpc_tick:
            # gait.py:76-78: iteration = floor(iter / iterations_between_mpc) % period
            torch.remainder(torch.full_like(self._period, iter_counter // ibm), self._period, out=self.iteration)
        vb = self._cmd(vel_body_des, (B, 3))
        yr = self._cmd(yaw_rate_des, (B,))
        if root_states is not None:
            rs = self._f32(root_states)
            self.engine.plan(flags, self.plan_state, self.x0, vb, yr, root_states=rs, gait=self.gait,
                             iteration=self.iteration, height_des=self.height, xref=self.xref,
                             contact=self.contact)
        else:
            c = [self._f32(t) for t in (quat, pos, omega, vel)]
            r = self._f32(rot) if rot is not None else None
            self.engine.plan(flags, self.plan_state, self.x0, vb, yr, quat=c[0], pos=c[1], omega=c[2],
                             vel=c[3], rot=r, gait=self.gait, iteration=self.iteration,
                             height_des=self.height, xref=self.xref, contact=self.contact)
        if mpc_tick:
            ft = self._f32(feet)
            self.engine.solve_raw(B, self.x0, self.xref, self.contact, ft, self.robot, self.u0,
                                  status=self.status, iters=self.iterations)
        return self.u0

    def torques(self, jac, stance):
        """Stance-leg joint torques into self.tau (leg_controller.py:86-89).

        jac [B,4,3,3]: each leg's 3x3 block of its foot Jacobian; stance [B,4] > 0 for
        legs whose swing state is 0 (leg_controller.py:77).  Swing-leg entries of tau
        keep whatever the swing controller wrote."""
        j, s = self._f32(jac), self._f32(stance)
        self.engine.stance_torques(j, s, self.u0, self.tau, stance_stride=s.shape[-1])
        return self.tau

    def leg_torques(self, iter_counter, vel_body_des, yaw_rate_des, thighs, pos_feet, foot_pos_base, foot_vel_base,
                    jac, root_states=None, quat=None, pos=None, vel=None, rot=None):
        """All 12 joint torques of every robot into self.tau: the rest of the loop body
        after ``tick`` (isaacgym_a1.py:137-162) in one launch, with no host read.

        ``iter_counter``: the control-iteration counter of ``tick``; an int is written to
        the device counters ``self.tick_count`` (one fill), None leaves them to the caller
        (per-robot offsets, or a captured graph that advances them on the device).
        thighs [B,4,3] hip positions in the base frame, pos_feet [B,4,3] feet in the world
        frame, foot_pos_base / foot_vel_base [B,4,3] feet relative to the base in the base
        frame, jac [B,4,3,3] as for ``torques``.  Legs in swing (self.swing_state > 0) get
        the swing PD law on the generated targets (self.pos_target, self.vel_target),
        the others Jv^T (-f) from self.u0."""
        B = self.B
        if iter_counter is not None:
            self.tick_count.fill_(int(iter_counter))
        vb = self._cmd(vel_body_des, (B, 3))
        yr = self._cmd(yaw_rate_des, (B,))
        th, pf, fp, fv, j = [self._f32(t) for t in (thighs, pos_feet, foot_pos_base, foot_vel_base, jac)]
        kw = dict(swing_state=self.swing_state, pos_target=self.pos_target, vel_target=self.vel_target)
        if root_states is not None:
            kw["root_states"] = self._f32(root_states)
        else:
            c = [self._f32(t) for t in (quat, pos, vel)]
            kw.update(quat=c[0], pos=c[1], vel=c[2], rot=self._f32(rot) if rot is not None else None)
        self.engine.leg_torques(self.tick_count, self.iterations_between_mpc, vb, yr, self.gait, th, pf, fp, fv, j,
                                self.u0, self.swing_mem, self.tau, **kw)
        return self.tau

    def kinematics(self, root_states, dof_states):
        """RobotData.update (robot_data.py:59-108) for every robot in one launch, from the
        simulator's actor root states [B,13] and dof states [B,12,2] (or [B*12,2], as Isaac
        Gym hands them out) into self.feet, thighs, pos_feet, foot_pos_base, foot_vel_base
        and jac."""
        if self.geometry is None:
            raise ValueError("no leg geometry: pass geometry= (params.LEG_GEOMETRY, leg_geometry_from_urdf)")
        rs, ds = self._f32(root_states), self._f32(dof_states)
        if rs.shape != (self.B, 13) or ds.numel() != self.B * 24:
            raise ValueError(f"expected root_states [{self.B},13] and dof_states [{self.B},12,2], got "
                             f"{tuple(rs.shape)} and {tuple(ds.shape)}")
        self.engine.kinematics(self.geometry, root_states=rs, dof_states=ds, feet=self.feet, thighs=self.thighs,
                               pos_feet=self.pos_feet, foot_pos_base=self.foot_pos_base,
                               foot_vel_base=self.foot_vel_base, jac=self.jac)
        return rs

    def step(self, iter_counter, vel_body_des, yaw_rate_des, root_states, dof_states):
        """The whole loop body of isaacgym_a1.py:117-162 for every robot, nothing computed by
        the caller: kinematics, then ``tick``, then ``leg_torques``; returns tau [B,12]
        (device).  root_states [B,13] and dof_states [B,12,2] are Isaac Gym's actor
        root-state and dof-state tensors as they lie on the device."""
        rs = self.kinematics(root_states, dof_states)
        self.tick(iter_counter, vel_body_des, yaw_rate_des, self.feet, root_states=rs)
        return self.leg_torques(iter_counter, vel_body_des, yaw_rate_des, self.thighs, self.pos_feet,
                                self.foot_pos_base, self.foot_vel_base, self.jac, root_states=rs)

    def set_command(self, vel_body_des, yaw_rate_des):
        """Store the command on the device once: ``step_fused`` then takes None for both and
        uploads nothing per call.  Tensors that already are contiguous float64 device tensors
        of shape [B,3] / [B] are kept as they are (writing into them changes the command)."""
        self._command = (self._cmd_fused(vel_body_des, (self.B, 3)), self._cmd_fused(yaw_rate_des, (self.B,)))
        return self._command

    def _cmd_fused(self, v, shape):
        if (isinstance(v, torch.Tensor) and v.dtype == torch.float64 and v.device == self.device
                and tuple(v.shape) == shape and v.is_contiguous()):
            return v
        return self._cmd(v, shape)

    def step_fused(self, iter_counter, vel_body_des, yaw_rate_des, root_states, dof_states, outputs=False,
                   mpc_tick=None):
        """``step`` in one C call (mpcqp_step): one launch on a tick between two solves, and on
        an MPC tick (``iter_counter % iterations_between_mpc == 0``) the plan with the
        reference, the solve and the leg controller enqueued together; returns tau [B,12]
        (device).  It leaves u0, x0, plan_state, swing_mem, status and iterations -- on an MPC
        tick xref, contact and feet too -- bitwise as ``step`` does.

        ``vel_body_des`` / ``yaw_rate_des``: contiguous float64 device tensors of shape [B,3] /
        [B] go through with no copy, anything else is converted as for ``step``; None for both
        uses what ``set_command`` stored.  ``iter_counter``: an int reaches the kernel as an
        argument (no fill; ``self.tick_count`` is left alone); None uses ``self.tick_count``,
        each robot's own counter kept by the caller, and ``mpc_tick`` then says whether this
        tick solves (left at None too, the first robot's counter is read back to decide, which
        waits for the device).  ``outputs=True`` also fills self.thighs, pos_feet, foot_pos_base,
        foot_vel_base, jac, swing_state, pos_target and vel_target, and self.feet on every
        tick; with False those attributes keep whatever an earlier call left (self.feet: the
        last MPC tick's)."""
        if self.geometry is None:
            raise ValueError("no leg geometry: pass geometry= (params.LEG_GEOMETRY, leg_geometry_from_urdf)")
        dev, B = self.device, self.B
        rs, ds = self._f32(root_states), self._f32(dof_states)
        if rs.shape != (B, 13) or ds.numel() != B * 24:
            raise ValueError(f"expected root_states [{B},13] and dof_states [{B},12,2], got "
                             f"{tuple(rs.shape)} and {tuple(ds.shape)}")
        if vel_body_des is None and yaw_rate_des is None:
            if getattr(self, "_command", None) is None:
                raise ValueError("no command: pass vel_body_des and yaw_rate_des, or call set_command first")
            vb, yr = self._command
        else:
            vb, yr = self._cmd_fused(vel_body_des, (B, 3)), self._cmd_fused(yaw_rate_des, (B,))
        ibm = self.iterations_between_mpc
        per_robot = iter_counter is None
        it = 0 if per_robot else int(iter_counter)
        if mpc_tick is None:
            mpc_tick = (int(self.tick_count[0]) if per_robot and B else it) % ibm == 0
        mpc_tick = bool(mpc_tick)
        # the pointer tuple is built once per set of buffers (the simulator's tensors and a
        # stored command keep their addresses from tick to tick)
        key = (rs.data_ptr(), ds.data_ptr(), vb.data_ptr(), yr.data_ptr(), bool(outputs), per_robot, mpc_tick)
        cache = self.__dict__.setdefault("_fused", {})
        launch = cache.get(key)
        if launch is None:
            if len(cache) >= 8:
                cache.clear()
            opt = dict(thighs=self.thighs, pos_feet=self.pos_feet, foot_pos_base=self.foot_pos_base,
                       foot_vel_base=self.foot_vel_base, jac=self.jac, swing_state=self.swing_state,
                       pos_target=self.pos_target, vel_target=self.vel_target) if outputs else {}
            launch = cache[key] = self.engine.bind_step(
                rs, ds, self.geometry, vb, yr, self.gait, self.plan_state, self.swing_mem, self.x0, self.u0,
                self.tau, tick=self.tick_count if per_robot else None, height_des=self.height, robot=self.robot,
                xref=self.xref, contact=self.contact, feet=self.feet if mpc_tick or outputs else None,
                status=self.status, iters=self.iterations, **opt)
        launch(STEP_MPC if mpc_tick else 0, it, ibm, torch.cuda.current_stream(dev))
        return self.tau

"""Batched rigid-body plant on the device: the stage that turns joint torques back into the
simulator's two state tensors, so that a fleet's control loop closes with nothing on the host.

``BatchedPlant`` is B single rigid bodies on massless legs with point feet -- the model the MPC
assumes, with the nonlinear rotation kept and the contact decided by the ground -- advanced by
one control iteration per call, one HIP launch (include/mpcqp_plant_abi.h mpcqp_plant).  The
reference's scripts hand this stage to a simulator (gym.simulate, sim.step()).  With a controller

    plant = BatchedPlant(B, controller=ctl)
    root, dofs = plant.reset()
    for it in range(T):
        tau = ctl.step_fused(it, v_des, yaw_rate, root, dofs)
        root, dofs = plant.step(tau)

is the whole loop; ``plant.gyro``, ``plant.accel`` and ``plant.touch`` feed
``BatchedEstimator.update_from_imu`` where the controller is to run on an estimated state.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import PLANT_STRIDE
from .engine import LinearMpc
from .params import ROBOT_PRESETS, pack_leg_geometry

_POS, _QUAT, _VEL, _OMEGA, _FEET, _FVEL, _CONTACT, _FLAGS, _TICK = 0, 3, 7, 10, 13, 25, 37, 41, 42


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class BatchedPlant:
    """Args:
      batch:      number of robots B
      robot:      preset name (mass, inertia, friction, leg geometry, default height) or [B,16]
                  records; with a controller its records are taken instead
      controller: a BatchedController: its engine (context), leg geometry and robot records are
                  shared.  A BatchedTerrain registered on it fits the plane the *controller*
                  believes in; the plant's ground is ``plane`` alone
      engine:     a LinearMpc to share without a controller; default a new one on ``device``
      geometry:   as for BatchedController; default the controller's, or the preset's
      plane:      the ground, [B,4] or [4] (n, d) with n . p = d and n of unit length (the
                  convention of LinearMpc.set_ground); None: level at ``ground_z``
      constants:  any of foot_mass, substeps, ground_z, contact_tol (mpcqp_set_plant; they are
                  the engine's, so a shared engine has one set); dt_control and gravity are the
                  engine's planner constants
    """

    def __init__(self, batch, robot="aliengo", controller=None, engine=None, geometry=None, plane=None,
                 device="cuda:0", **constants):
        self.B = B = int(batch)
        if controller is not None and controller.B != B:
            raise ValueError(f"the controller has {controller.B} robots, the plant {B}")
        if engine is None and controller is not None:
            engine = controller.engine
        self.engine = engine if engine is not None else LinearMpc(robot=robot if isinstance(robot, str) else None,
                                                                  device=device)
        self.controller = controller
        dev = self.device = self.engine.device
        self.lib, self._ctx = self.engine.lib, self.engine._ctx
        if constants:
            self.set_constants(**constants)
        if controller is not None:
            self.robot = controller.robot
            self.geometry = controller.geometry
            self.height = controller.height
        else:
            if isinstance(robot, str):
                rec = np.tile(self.engine.default_robot, (B, 1))
                height = ROBOT_PRESETS[robot].get("height", 0.38)
            else:
                rec, height = np.asarray(robot, dtype=np.float32).reshape(B, -1), None
            self.robot = torch.as_tensor(np.ascontiguousarray(rec, dtype=np.float32)).to(dev)
            self.geometry = None
            self.height = None if height is None else torch.full((B,), height, dtype=torch.float32, device=dev)
        if geometry is not None or self.geometry is None:
            if geometry is None and not isinstance(robot, str):
                raise ValueError("no leg geometry: pass geometry= (params.LEG_GEOMETRY, leg_geometry_from_urdf)")
            self.geometry = torch.as_tensor(pack_leg_geometry(robot if geometry is None else geometry, B)).to(dev)
        self.plane = None
        if plane is not None:
            p = torch.as_tensor(plane, dtype=torch.float32).to(dev)
            self.plane = p.expand(B, 4).contiguous() if p.dim() == 1 else p.reshape(B, 4).contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        self.state = torch.zeros((B, PLANT_STRIDE), dtype=torch.float64, device=dev)
        self.state[:, _QUAT] = 1.0
        self.root = torch.zeros((B, 13), **f32)
        self.root[:, 6] = 1.0
        self.dofs = torch.zeros((B, 12, 2), **f32)
        self.gyro = torch.zeros((B, 3), **f32)
        self.accel = torch.zeros((B, 3), **f32)
        self.touch = torch.zeros((B, 4), **f32)
        self.status = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.push_status = torch.zeros((B,), dtype=torch.int32, device=dev)
        self._bound = {}

    def set_constants(self, foot_mass=None, substeps=None, ground_z=None, contact_tol=None):
        """mpcqp_set_plant.  A constant that is not given keeps its last value (they are kept on
        the engine, whose they are: ``engine.plant_constants``); at first foot_mass 0.15,
        substeps 1, contact_tol 1e-4 and a ground_z that follows the swing leg's touchdown_z until
        one is given.  A non-finite value, a non-positive foot_mass or substeps outside 1..16
        raises and keeps the previous constants."""
        last = getattr(self.engine, "plant_constants", None) or dict(foot_mass=0.15, substeps=1, ground_z=None,
                                                                     contact_tol=1e-4)
        new = dict(last)
        for k, v in (("foot_mass", foot_mass), ("substeps", substeps), ("ground_z", ground_z), ("contact_tol", contact_tol)):
            if v is not None:
                new[k] = v
        if new["ground_z"] is None and new == last:
            self.engine.plant_constants = new     # nothing given: the library's own defaults stand
            return
        gz = new["ground_z"] if new["ground_z"] is not None else getattr(self.engine, "touchdown_z", -0.0255)
        _lib.check(self._ctx, self.lib.mpcqp_set_plant(self._ctx, float(new["foot_mass"]), int(new["substeps"]), float(gz),
                                                       float(new["contact_tol"])), "mpcqp_set_plant")
        self.engine.plant_constants = new

    def _stream(self, stream):
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        return ctypes.c_void_p(s.cuda_stream)

    def reset(self, height=None, q=(0.0, 0.7, -1.4), root_states=None, dof_states=None, stream=None):
        """Fill the records from a pose and return (root, dofs), the tensors ``step`` keeps
        writing.  Default pose: level at the origin at ``height`` (None: the controller's or the
        preset's desired height), every leg at q = (hip, thigh, calf), at rest; or any
        root_states [B,13] / dof_states [B,12,2].  Feet come from forward kinematics, and a foot
        within contact_tol of the ground starts in contact (mpcqp_plant_reset)."""
        B = self.B
        if root_states is None:
            if height is None:
                if self.height is None:
                    raise ValueError("reset: height is required without a preset or a controller")
                height = self.height
            self.root.zero_()
            self.root[:, 6] = 1.0
            self.root[:, 2] = torch.as_tensor(height, dtype=torch.float32).to(self.device)
        else:
            self.root.copy_(torch.as_tensor(root_states).to(self.device, torch.float32).reshape(B, 13))
        if dof_states is None:
            self.dofs.zero_()
            self.dofs[:, :, 0] = torch.tensor(list(q) * 4, dtype=torch.float32, device=self.device)
        else:
            self.dofs.copy_(torch.as_tensor(dof_states).to(self.device, torch.float32).reshape(B, 12, 2))
        _lib.check(self._ctx, self.lib.mpcqp_plant_reset(self._ctx, B, _ptr(self.root), _ptr(self.dofs),
                                                         _ptr(self.geometry), _ptr(self.plane), _ptr(self.state),
                                                         self._stream(stream)), "mpcqp_plant_reset")
        self.gyro.zero_()
        self.accel.zero_()
        self.touch.copy_(self.contact)
        self.status.zero_()
        return self.root, self.dofs

    def bind_step(self, tau):
        """``step`` with its checks made and its device pointers resolved once: returns
        ``launch(stream)`` (see LinearMpc.bind_predict), e.g. for capture into a HIP graph."""
        if not (tau.dtype == torch.float32 and tau.is_contiguous() and tau.device == self.device
                and tau.numel() == self.B * 12):
            raise ValueError(f"plant: tau must be a contiguous float32 tensor of shape [{self.B}, 12] on "
                             f"{self.device}, got {tau.dtype} {tuple(tau.shape)} on {tau.device}")
        lib, ctx = self.lib, self._ctx
        args = (ctx, self.B, 0, _ptr(tau), _ptr(self.robot), _ptr(self.geometry), _ptr(self.plane), _ptr(self.state),
                _ptr(self.root), _ptr(self.dofs), _ptr(self.gyro), _ptr(self.accel), _ptr(self.touch),
                _ptr(self.status))

        def launch(stream):
            _lib.check(ctx, lib.mpcqp_plant(*args, ctypes.c_void_p(stream.cuda_stream)), "mpcqp_plant")
        launch.buffers = (tau, self.robot, self.geometry, self.plane, self.state)
        return launch

    def step(self, tau, stream=None):
        """One control iteration of every robot under tau [B,12] (float32, device; usually
        ``controller.tau``): returns (root [B,13], dofs [B,12,2]), the same tensors every call.
        Also fills gyro, accel, touch and status.  The pointer tuple is bound once per tau
        buffer."""
        key = tau.data_ptr()
        launch = self._bound.get(key)
        if launch is None:
            if len(self._bound) >= 8:
                self._bound.clear()
            if not (tau.dtype == torch.float32 and tau.is_contiguous() and tau.device == self.device):
                tau = tau.to(self.device, torch.float32).contiguous()
                launch = self.bind_step(tau)          # a converted copy: not cached
            else:
                launch = self._bound[key] = self.bind_step(tau)
        launch(torch.cuda.current_stream(self.device) if stream is None else stream)
        return self.root, self.dofs

    def bind_push(self, impulse, point=None):
        """``push`` with its checks made and its device pointers resolved once: returns
        ``launch(stream)`` (see ``bind_step``), e.g. for capture into a HIP graph; the caller
        writes the impulses into the bound tensor between two launches."""
        for name, t in (("impulse", impulse), ("point", point)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_contiguous()
                                      and t.device == self.device and t.numel() == self.B * 3):
                what = f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', 'the host')}"
                raise ValueError(f"plant: {name} must be a contiguous float32 tensor of shape [{self.B}, 3] on "
                                 f"{self.device}, got {what}")
        lib, ctx = self.lib, self._ctx
        args = (ctx, self.B, _ptr(impulse), _ptr(point), _ptr(self.robot), _ptr(self.state), _ptr(self.push_status))

        def launch(stream):
            _lib.check(ctx, lib.mpcqp_push(*args, ctypes.c_void_p(stream.cuda_stream)), "mpcqp_push")
        launch.buffers = (impulse, point, self.robot, self.state)
        return launch

    def push(self, impulse, point=None, stream=None):
        """An impulse on every robot's record, one launch (mpcqp_push): ``impulse`` [B,3] or [3]
        in the world frame, N s, acting at ``point`` [B,3] or [3] in the body frame from the
        centre of mass (None: at the centre of mass): v += J / m, w += I_w^-1 ((Rq r) x J).  Feet
        and contacts are not touched (a pinned foot stays pinned) and a zero impulse leaves the
        record bit by bit.  A force F over one tick is the impulse F dt_control, given every
        tick; ``accel`` does not see an impulse.  Fills ``push_status`` [B] int32: STATUS_NONFINITE
        for a robot with a non-finite impulse, point, record or result, which is left untouched.
        Anything but a float32 device tensor [B,3] is converted on each call."""
        def dev(t):
            if t is None or (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_contiguous()
                             and t.device == self.device and t.numel() == self.B * 3):
                return t
            t = torch.as_tensor(t, dtype=torch.float32).to(self.device)
            return (t.expand(self.B, 3) if t.dim() == 1 else t.reshape(self.B, 3)).contiguous()
        self.bind_push(dev(impulse), dev(point))(torch.cuda.current_stream(self.device) if stream is None else stream)

    # ---- views of the records
    @property
    def contact(self):
        """[B,4] float64, 1 where the foot is in contact (the record's flags; ``touch`` is the
        float32 output of the last step)."""
        return self.state[:, _CONTACT:_CONTACT + 4]

    @property
    def feet_world(self):
        """The feet in the world frame [B,4,3] float64."""
        return self.state[:, _FEET:_FEET + 12].view(self.B, 4, 3)

    @property
    def foot_vel_world(self):
        return self.state[:, _FVEL:_FVEL + 12].view(self.B, 4, 3)

    @property
    def flags(self):
        """[B] float64: bit l set where leg l's inverse kinematics was clamped in the last step."""
        return self.state[:, _FLAGS]

    @property
    def ticks(self):
        """[B] float64: the number of accepted steps since reset."""
        return self.state[:, _TICK]

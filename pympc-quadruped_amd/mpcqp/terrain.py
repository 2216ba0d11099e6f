"""Batched terrain plane on the device: the ground under each robot, from its own feet.

``BatchedTerrain`` is B copies of ``RobotData.update_terrain_normal`` (utils/robot_data.py:
186-228), which the reference defines and never calls: it latches each foot's world position
while the foot is in contact, fits a plane to the four latched points and hands the result
to the two parts of the loop that otherwise assume level ground -- the friction cones of the
solve, through the surface normal in the robot record, and the swing leg's foothold and
apex, through the ground plane registered on the engine -- in one HIP launch per control
iteration (include/mpcqp.h mpcqp_terrain).  With a controller

    ter = BatchedTerrain(B, controller=ctl)
    tau = ctl.step(it, v_des, yaw_rate, root, dof_states); ter.update()

is the whole loop on a slope (with ``step_fused``, call it with ``outputs=True`` so that
``ctl.pos_feet`` and ``ctl.swing_state`` are filled).
"""
import numpy as np
import torch

from ._lib import TERRAIN_STRIDE
from .engine import LinearMpc

_HIST, _INIT, _N, _D, _FITTED = 0, 12, 13, 16, 17


class BatchedTerrain:
    """Args:
      batch:      number of robots B
      controller: a BatchedController: ``update`` takes its pos_feet and swing_state by
                  default, and its engine is shared unless ``engine`` is given
      engine:     a LinearMpc to share; default the controller's, or a new one on ``device``
      attach:     with a controller, write the normal into ``controller.robot`` (words 9..11,
                  read by the next solve's cone rows) and register ``plane`` as the swing
                  leg's ground (LinearMpc.set_ground)
      ground:     what ``plane`` is.  "feet" (the default when attached): the latched points
                  are foot centres, where the swing leg's footholds belong, and ``plane`` is
                  (n, d - n_z touchdown_z), the ground under them by the swing leg's own
                  touchdown_z -- a foothold then lies on the fitted plane, and level ground
                  walks as with no terrain stage.  "surface" (the default otherwise): ``plane``
                  is the fitted (n, d) itself, for a simulator whose foot centres ride
                  -touchdown_z above the surface that the latched points lie on
      constants:  any of LinearMpc.set_terrain's (contact_threshold, flat_tol, cos_max_tilt,
                  blend); they are the engine's, so a shared engine has one set
    """

    def __init__(self, batch, controller=None, engine=None, device="cuda:0", attach=True, ground=None,
                 **constants):
        self.B = B = int(batch)
        if controller is not None and controller.B != B:
            raise ValueError(f"the controller has {controller.B} robots, the terrain {B}")
        if engine is None and controller is not None:
            engine = controller.engine
        self.engine = engine if engine is not None else LinearMpc(device=device)
        if constants or not hasattr(self.engine, "terrain_constants"):
            self.engine.set_terrain(**constants)
        self.controller = controller
        dev = self.device = self.engine.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.terrain_state = torch.zeros((B, TERRAIN_STRIDE), dtype=torch.float64, device=dev)
        self._normal = torch.zeros((B, 3), **f32)
        self._normal[:, 2] = 1.0
        self._plane = torch.zeros((B, 4), **f32)
        self._plane[:, 2] = 1.0
        self._normal_base = torch.zeros((B, 3), **f32)
        self._status = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.robot = None
        attached = controller is not None and attach
        if ground is None:
            ground = "feet" if attached else "surface"
        if ground not in ("feet", "surface"):
            raise ValueError(f"ground must be 'feet' or 'surface', got {ground!r}")
        self.ground = ground
        if attached:
            self.robot = controller.robot
            self.engine.set_ground(self._plane)

    def _f32(self, t, shape):
        t = torch.as_tensor(t)
        if not (t.dtype == torch.float32 and t.is_contiguous() and t.device == self.device):
            t = t.to(self.device, torch.float32).contiguous()
        if t.numel() != int(np.prod(shape)):
            raise ValueError(f"expected {list(shape)}, got {tuple(t.shape)}")
        return t

    def update(self, pos_feet=None, contact=None, swing_state=None, quat=None, root_states=None):
        """One tick for every robot; returns normal [B,3] (device).

        pos_feet [B,4,3]: the feet in the world frame; contact [B,4] (> contact_threshold:
        in contact) or swing_state [B,4] (not > 0: in contact).  With a controller they
        default to its pos_feet and swing_state, as its last ``step`` left them.  quat [B,4]
        (w, x, y, z) or root_states [B,13] also fills ``normal_base``.  Also fills ``plane``,
        ``status`` and, attached, the controller's robot records."""
        B, ctl = self.B, self.controller
        if pos_feet is None:
            if ctl is None:
                raise ValueError("update: pos_feet is required without a controller")
            pos_feet = ctl.pos_feet
        if contact is None and swing_state is None:
            if ctl is None:
                raise ValueError("update: contact or swing_state is required without a controller")
            swing_state = ctl.swing_state
        kw = {}
        if contact is not None:
            kw["contact"] = self._f32(contact, (B, 4))
        else:
            kw["swing_state"] = self._f32(swing_state, (B, 4))
        if quat is not None:
            kw.update(quat=self._f32(quat, (B, 4)), normal_base=self._normal_base)
        elif root_states is not None:
            kw.update(root_states=self._f32(root_states, (B, 13)), normal_base=self._normal_base)
        self.engine.terrain(self.terrain_state, self._f32(pos_feet, (B, 4, 3)), robot=self.robot,
                            normal=self._normal, plane=self._plane, status=self._status,
                            ground=self.ground == "feet", **kw)
        return self._normal

    def reset(self, robots=None):
        """Zero the records of all or some robots: the next update seeds their history with
        all four feet.  Their outputs return to (0, 0, 1, 0), on which the swing leg walks as
        with no ground registered."""
        idx = slice(None) if robots is None else robots
        self.terrain_state[idx] = 0.0
        level = torch.tensor([0.0, 0.0, 1.0, 0.0], dtype=torch.float32, device=self.device)
        self._plane[idx] = level
        self._normal[idx] = level[:3]
        if self.robot is not None:
            self.robot[idx, 9:12] = level[:3]

    @property
    def normal(self):
        """n [B,3] float32, unit length, n_z > 0."""
        return self._normal

    @property
    def plane(self):
        """(n, d) [B,4] float32: the plane n . p = d through the centroid of the history; with
        ground="feet" its fourth word is d - n_z touchdown_z, the swing leg's ground."""
        return self._plane

    @property
    def normal_base(self):
        """R_base^T n [B,3] float32, as the last update with quat or root_states left it."""
        return self._normal_base

    @property
    def history(self):
        """The latched feet [B,4,3] float64, a view of the records."""
        return self.terrain_state[:, _HIST:_HIST + 12].view(self.B, 4, 3)

    @property
    def fitted(self):
        """[B] bool: the last update's fit was accepted."""
        return self.terrain_state[:, _FITTED] != 0.0

    @property
    def status(self):
        """[B] int32: STATUS_OK, or STATUS_NONFINITE for a robot whose last update was refused."""
        return self._status

"""Batched gait scheduler on the device: the stage that owns each robot's gait record and
control-iteration counter, so that a fleet can stand, walk, change gait and stop per robot while
the loop runs with nothing on the host.

``BatchedGaitScheduler`` replaces what the reference does by hand between two runs -- fresh
``Gait`` objects and ``iter_counter`` back at 0 (scripts/mujoco_aliengo.py:121-155; gait.py:76-121)
-- by one HIP launch per control iteration (include/mpcqp_gait_abi.h mpcqp_gait_schedule) that
advances every robot's counter and replaces a robot's record by a library entry only at a tick
where no leg is between its first and its last swing tick.  With a controller and a plant

    sched = BatchedGaitScheduler(B, controller=ctl, gaits=("standing", "trot10", "pace10"), initial="standing")
    root, dofs = plant.reset()
    for it in range(T):
        sched.update(advance=it > 0)                       # may switch some robots; owns ctl.tick_count
        tau = ctl.step_fused(None, None, None, root, dofs, mpc_tick=it % ctl.iterations_between_mpc == 0)
        root, dofs = plant.step(tau)

is the whole loop; ``sched.request("trot10", robots=[2, 5])`` at any iteration is honoured at the
robots' next seam.  A switch leaves ``tick mod iterations_between_mpc`` as it was, so the one
``mpc_tick`` flag stays right for every robot.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import GAIT_ADVANCE, GAIT_MAX, GAIT_STRIDE, SCHED_STRIDE, SWING_STRIDE
from .engine import LinearMpc
from .params import gait_record

_CUR, _PENDING, _SINCE, _SWITCHES, _CALM, _LAST = range(6)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class BatchedGaitScheduler:
    """Args:
      batch:      number of robots B
      controller: a BatchedController: its engine (context) is shared and its ``gait``,
                  ``tick_count`` and ``swing_mem`` are adopted in place -- their addresses do not
                  change, so ``step_fused``'s bound launches stay valid -- and ``auto`` reads the
                  command ``set_command`` stored
      gaits:      the library: up to 16 params.GAITS keys, Gait member names or (period, offsets,
                  durations) triples (mpcqp_set_gaits; it is the engine's, so a shared engine has
                  one library)
      initial:    the gait every robot starts in, or a sequence of B: a library entry by name,
                  triple or index
      engine:     a LinearMpc to share without a controller; default a new one on ``device``
      iterations_between_mpc: without a controller (default 20); the controller's otherwise
      min_hold:   ``set_constants``
    """

    def __init__(self, batch, controller=None, gaits=("standing", "trot10"), initial=0, engine=None,
                 iterations_between_mpc=None, device="cuda:0", min_hold=0):
        self.B = B = int(batch)
        if controller is not None and controller.B != B:
            raise ValueError(f"the controller has {controller.B} robots, the scheduler {B}")
        if engine is None and controller is not None:
            engine = controller.engine
        self.engine = engine if engine is not None else LinearMpc(device=device)
        self.controller = controller
        dev = self.device = self.engine.device
        self.lib, self._ctx = self.engine.lib, self.engine._ctx
        if iterations_between_mpc is None:
            iterations_between_mpc = controller.iterations_between_mpc if controller is not None else 20
        self.iterations_between_mpc = int(iterations_between_mpc)
        self.set_gaits(gaits)
        self._constants = dict(min_hold=0, idle=-1, move=-1, v_go=0.0, v_stop=0.0, w_go=0.0, w_stop=0.0, dwell=0)
        self._auto_from = None
        i32 = dict(dtype=torch.int32, device=dev)
        if controller is not None:
            self.gait, self.tick, self.swing_mem = controller.gait, controller.tick_count, controller.swing_mem
        else:
            self.gait = torch.zeros((B, GAIT_STRIDE), **i32)
            self.tick = torch.zeros((B,), **i32)
            self.swing_mem = torch.zeros((B, SWING_STRIDE), dtype=torch.float64, device=dev)
        self.sched_state = torch.zeros((B, SCHED_STRIDE), **i32)
        self.want = torch.full((B,), -1, **i32)
        self.iteration = controller.iteration if controller is not None else torch.zeros((B,), **i32)
        self._switched = torch.zeros((B,), **i32)
        self._status = torch.zeros((B,), **i32)
        init = [initial] * B if isinstance(initial, (str, int, np.integer)) or self._is_triple(initial) else list(initial)
        if len(init) != B:
            raise ValueError(f"initial: expected one gait or {B} of them, got {len(init)}")
        self._initial = torch.as_tensor(np.array([self.index(g) for g in init], np.int32)).to(dev)
        if min_hold:
            self.set_constants(min_hold=min_hold)
        self.reset()

    @staticmethod
    def _is_triple(g):
        return (isinstance(g, (tuple, list)) and len(g) == 3 and np.isscalar(g[0]) and not isinstance(g[0], str)
                and np.ndim(g[1]) == 1)

    def set_gaits(self, gaits):
        """mpcqp_set_gaits: the library, 1 .. 16 records, each with 1 <= period <= 2048,
        0 <= duration <= period, |offset| <= 4 period and a segment at which it can be entered.
        Anything else raises and keeps the previous library."""
        gaits = list(gaits)
        if not 1 <= len(gaits) <= GAIT_MAX:
            raise ValueError(f"the library holds 1 .. {GAIT_MAX} gaits, got {len(gaits)}")
        recs = np.ascontiguousarray(np.stack([gait_record(g) for g in gaits]), dtype=np.int32)
        _lib.check(self._ctx, self.lib.mpcqp_set_gaits(self._ctx, len(gaits), recs.ctypes.data_as(ctypes.c_void_p)),
                   "mpcqp_set_gaits")
        self.records = recs
        self.names = [g if isinstance(g, str) else None for g in gaits]
        self._library = torch.as_tensor(recs).to(self.device)

    def index(self, gait):
        """The library index of a name, a triple or an index."""
        if isinstance(gait, (int, np.integer)):
            if not 0 <= int(gait) < len(self.records):
                raise ValueError(f"gait index {gait} outside the library of {len(self.records)}")
            return int(gait)
        if isinstance(gait, str) and gait in self.names:
            return self.names.index(gait)
        rec = gait_record(gait)
        for i, r in enumerate(self.records):
            if np.array_equal(r, rec):
                return i
        raise ValueError(f"gait {gait!r} is not in the library")

    def set_constants(self, min_hold=None):
        """mpcqp_set_gait_schedule's min_hold: the control iterations a robot keeps a gait before
        it may switch again (at first 0).  Not given, it keeps its last value; a negative one raises
        and keeps the previous constants."""
        new = dict(self._constants)
        if min_hold is not None:
            new["min_hold"] = int(min_hold)
        self._set(new)

    def _set(self, new):
        _lib.check(self._ctx, self.lib.mpcqp_set_gait_schedule(
            self._ctx, int(new["min_hold"]), int(new["idle"]), int(new["move"]), float(new["v_go"]), float(new["v_stop"]),
            float(new["w_go"]), float(new["w_stop"]), int(new["dwell"])), "mpcqp_set_gait_schedule")
        self._constants = new

    def auto(self, idle, move, v_go, v_stop, w_go=float("inf"), w_stop=float("inf"), dwell=0, start=0):
        """Turn on the automatic choice from the controller's stored command (``set_command``):
        ``move`` when vx^2 + vy^2 > v_go^2 or |yaw rate| > w_go, ``idle`` once the command has been
        at or below both stop thresholds for ``dwell`` consecutive calls; in between the latched
        request stays.  w_go / w_stop default to thresholds no yaw rate passes (the largest float64).
        ``start``: the robots from this row on are automatic and the rows before it follow
        ``request`` (two launches per update); 0: the whole fleet.  ``idle=None`` turns it off."""
        if idle is None:
            self._set(dict(self._constants, idle=-1, move=-1))
            self._auto_from = None
            return
        big = np.finfo(np.float64).max
        w_go, w_stop = min(float(w_go), big), min(float(w_stop), big)
        if not 0 <= int(start) < self.B:
            raise ValueError(f"auto: start {start} outside 0 .. {self.B - 1}")
        if self.controller is None or getattr(self.controller, "_command", None) is None:
            raise ValueError("auto: the controller has no stored command (set_command)")
        self._set(dict(self._constants, idle=self.index(idle), move=self.index(move), v_go=v_go, v_stop=v_stop,
                       w_go=w_go, w_stop=w_stop, dwell=dwell))
        self._auto_from = int(start)

    def request(self, gait, robots=None):
        """Write the request on the device: a name, triple or index for all robots or for
        ``robots`` (indices, a slice or a mask), a sequence of B of them, -1 / None for no new
        request, or a device int32 tensor [B], which is kept and used in place from then on (the
        caller writes library indices or -1 into it, e.g. between two replays of a graph)."""
        if isinstance(gait, torch.Tensor):
            if not (gait.dtype == torch.int32 and gait.device == self.device and gait.is_contiguous()
                    and tuple(gait.shape) == (self.B,)):
                raise ValueError(f"request: expected a contiguous int32 tensor [{self.B}] on {self.device}")
            self.want = gait
            return
        one = lambda g: -1 if g is None or (isinstance(g, (int, np.integer)) and int(g) == -1) else self.index(g)
        if isinstance(gait, (str, int, np.integer)) or gait is None or self._is_triple(gait):
            if robots is None:
                self.want.fill_(one(gait))
            else:
                self.want[robots] = one(gait)
            return
        idx = [one(g) for g in gait]
        if robots is not None or len(idx) != self.B:
            raise ValueError(f"request: a sequence must hold one gait per robot ({self.B})")
        self.want.copy_(torch.as_tensor(np.array(idx, np.int32)))

    def bind_update(self, advance=True, iteration=False):
        """``update`` with its checks made and its device pointers resolved once: returns
        ``launch(stream)`` (see BatchedPlant.bind_step), e.g. for capture into a HIP graph.  The
        ``want`` tensor, the controller's command and the automatic choice are bound as they are
        now.  ``iteration=True`` also fills ``self.iteration`` ((tick / ibm) mod period, what
        mpcqp_plan takes), which costs every robot divisions; ``step_fused`` does not need it."""
        lib, ctx, B, ibm = self.lib, self._ctx, self.B, self.iterations_between_mpc
        flags = GAIT_ADVANCE if advance else 0
        k = self._auto_from
        vb = yr = None
        if k is not None:
            vb, yr = self.controller._command
        at = lambda t, row, stride, size: None if t is None else ctypes.c_void_p(t.data_ptr() + row * stride * size)

        def rows(first, count, auto):
            return (ctx, count, flags, ibm, None if auto else at(self.want, first, 1, 4),
                    at(vb, first, 3, 8) if auto else None, at(yr, first, 1, 8) if auto else None,
                    at(self.sched_state, first, SCHED_STRIDE, 4), at(self.gait, first, GAIT_STRIDE, 4),
                    at(self.tick, first, 1, 4), at(self.swing_mem, first, SWING_STRIDE, 8),
                    at(self.iteration, first, 1, 4) if iteration else None, at(self._switched, first, 1, 4),
                    at(self._status, first, 1, 4))
        if k is None:
            calls = [rows(0, B, False)]
        elif k == 0:
            calls = [rows(0, B, True)]
        else:
            calls = [rows(0, k, False), rows(k, B - k, True)]

        def launch(stream):
            s = ctypes.c_void_p(stream.cuda_stream)
            for args in calls:
                _lib.check(ctx, lib.mpcqp_gait_schedule(*args, s), "mpcqp_gait_schedule")
        launch.buffers = (self.want, vb, yr, self.sched_state, self.gait, self.tick, self.swing_mem)
        return launch

    def update(self, advance=True, stream=None, iteration=False):
        """The one launch per control iteration: advance every robot's counter (``advance=False``
        on the first call after a reset) and switch the robots whose request can be honoured at
        this tick.  Fills ``switched`` and ``status``.  The pointer tuple is bound once per set of
        buffers."""
        cmd = getattr(self.controller, "_command", None) if self._auto_from is not None else None
        key = (bool(advance), bool(iteration), self.want.data_ptr(), self._auto_from,
               None if cmd is None else (cmd[0].data_ptr(), cmd[1].data_ptr()))
        cache = self.__dict__.setdefault("_bound", {})
        launch = cache.get(key)
        if launch is None:
            if len(cache) >= 8:
                cache.clear()
            launch = cache[key] = self.bind_update(advance, iteration)
        launch(torch.cuda.current_stream(self.device) if stream is None else stream)

    def reset(self, robots=None):
        """Zero the records and ticks of all or some robots, write their initial gait record and
        withdraw their requests.  With a controller, call its ``reset`` for the same robots too
        (plan_state, swing_mem)."""
        idx = slice(None) if robots is None else robots
        self.sched_state[idx] = 0
        self.sched_state[idx, _CUR] = self._initial[idx]
        self.sched_state[idx, _PENDING] = self._initial[idx]
        self.gait[idx] = self._library[self._initial[idx].long()]
        self.tick[idx] = 0
        self.want[idx] = -1
        self._switched[idx] = 0
        self._status[idx] = 0

    # ---- views of the records
    @property
    def current(self):
        """[B] int32: the library index in force (-1: a record set by hand)."""
        return self.sched_state[:, _CUR]

    @property
    def pending(self):
        """[B] int32: the latched request; equal to ``current`` where nothing is pending."""
        return self.sched_state[:, _PENDING]

    @property
    def since(self):
        """[B] int32: control iterations since the robot's last switch (saturating)."""
        return self.sched_state[:, _SINCE]

    @property
    def switches(self):
        """[B] int32: the number of switches since reset."""
        return self.sched_state[:, _SWITCHES]

    @property
    def last_tick(self):
        """[B] int32: the robot's tick just before its last switch."""
        return self.sched_state[:, _LAST]

    @property
    def switched(self):
        """[B] int32: 1 where the last update switched."""
        return self._switched

    @property
    def status(self):
        """[B] int32: STATUS_OK, STATUS_UNSUPPORTED (a request outside the library, a tick that
        cannot advance) or STATUS_NONFINITE (a non-finite command under the automatic choice)."""
        return self._status

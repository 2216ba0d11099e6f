"""Batched sensor model on the device: the stage between the plant and the sensing chain, so
that a fleet's estimator and controller see what sensors would report instead of the plant's
exact state -- and so that robots given the same command stop being copies of one another.

``BatchedSensors`` is one HIP launch per control iteration (include/mpcqp_disturb_abi.h
mpcqp_sensors): white noise and a bias (drawn at turn-on, then a random walk) on the gyro and
the accelerometer, white noise and a quantisation step on the encoders, a lag and dropouts on
the touch sensors.  Every draw is a pure function of (seed, robot id, the robot's count of
calls) through Philox4x32-10, so a run is reproducible word for word and tests/disturb_ref.py
restates it on the CPU.  The reference has no such component: its scripts read a simulator's
sensors as they come (gym.simulate, sim.step()).  With a plant, an estimator and a controller

    sens = BatchedSensors(B, plant=plant, seed=7, preset="mems")
    root, dofs = plant.step(tau)
    sens.update()
    root_est = est.update_from_imu(sens.gyro, sens.accel, sens.dofs, tick=ctl.tick_count, touch=sens.touch)
    tau = ctl.step_fused(None, None, None, root_est, sens.dofs, ...)

is the loop.  ``plant.push(impulse)`` (mpcqp_push) is the other input of a robustness experiment.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import SENSE_STRIDE
from .engine import LinearMpc

_BIAS_G, _BIAS_A, _INIT, _COUNT, _ID, _HIST = 0, 3, 6, 7, 8, 9

_ZERO = dict(sigma_gyro=0.0, sigma_accel=0.0, walk_gyro=0.0, walk_accel=0.0, bias0_gyro=0.0, bias0_accel=0.0,
             sigma_q=0.0, sigma_qd=0.0, q_lsb=0.0, touch_lag=0, p_drop=0.0)

# One plausible set of figures for a small MEMS IMU, 14-bit joint encoders and a debounced foot
# switch.  They are plausible orders of magnitude, not measurements of any device: gyro white
# noise 2e-3 rad/s and accelerometer 5e-2 m/s^2 per sample, bias walks 1e-5 rad/s and 1e-4 m/s^2
# per sqrt(s), turn-on biases 5e-3 rad/s and 5e-2 m/s^2 (1 sigma), joint-rate noise 5e-2 rad/s,
# an encoder step of 2 pi / 2^14 rad, a touch signal two control iterations late, no dropouts.
SENSOR_PRESETS = {
    "mems": dict(_ZERO, sigma_gyro=2e-3, sigma_accel=5e-2, walk_gyro=1e-5, walk_accel=1e-4, bias0_gyro=5e-3,
                 bias0_accel=5e-2, sigma_qd=5e-2, q_lsb=2.0 * math.pi / 2 ** 14, touch_lag=2),
}


def _ptr(t, row=0, words=1):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + row * words * t.element_size())


class BatchedSensors:
    """Args:
      batch:   number of robots B
      plant:   a BatchedPlant: its engine (context) is shared and its gyro, accel, dofs and touch
               are the inputs ``update`` reads
      engine:  a LinearMpc to share without a plant; default a new one on ``device``
      seed:    0 .. 2^64 - 1, the generator's key
      preset:  a SENSOR_PRESETS key (plausible figures, not measurements of a device) or None
               for all constants zero, the identity
      scale:   None, or [B] float32 (a tensor is kept and read in place on every update, anything
               else is copied): multiplies every sigma, walk and bias0 of that robot, so one run
               sweeps noise levels across a fleet; not q_lsb, touch_lag or p_drop
      constants: any of sigma_gyro, sigma_accel, walk_gyro, walk_accel, bias0_gyro, bias0_accel,
               sigma_q, sigma_qd, q_lsb, touch_lag, p_drop over the preset (mpcqp_set_sensors;
               they are the engine's, so a shared engine has one set); dt_control is the
               engine's planner constant
    """

    def __init__(self, batch, plant=None, engine=None, seed=0, preset=None, scale=None, device="cuda:0", **constants):
        self.B = B = int(batch)
        if plant is not None and plant.B != B:
            raise ValueError(f"the plant has {plant.B} robots, the sensors {B}")
        if engine is None and plant is not None:
            engine = plant.engine
        self.engine = engine if engine is not None else LinearMpc(device=device)
        self.plant = plant
        dev = self.device = self.engine.device
        self.lib, self._ctx = self.engine.lib, self.engine._ctx
        if preset is not None and preset not in SENSOR_PRESETS:
            raise ValueError(f"unknown sensor preset {preset!r}: {sorted(SENSOR_PRESETS)}")
        self.set_constants(seed=seed, **dict(_ZERO if preset is None else SENSOR_PRESETS[preset], **constants))
        f32 = dict(dtype=torch.float32, device=dev)
        self.state = torch.zeros((B, SENSE_STRIDE), dtype=torch.float64, device=dev)
        self.gyro = torch.zeros((B, 3), **f32)
        self.accel = torch.zeros((B, 3), **f32)
        self.dofs = torch.zeros((B, 12, 2), **f32)
        self.touch = torch.zeros((B, 4), **f32)
        self._status = torch.zeros((B,), dtype=torch.int32, device=dev)
        if scale is None or isinstance(scale, torch.Tensor):
            self.scale = scale
        else:
            self.scale = torch.as_tensor(np.asarray(scale, np.float32).reshape(B)).to(dev)
        self._bound = {}
        self.reset()

    def set_constants(self, seed=None, **constants):
        """mpcqp_set_sensors.  A constant that is not given keeps its last value (they are kept on
        the engine, whose they are: ``engine.sensor_constants``); at first all are zero and the
        seed is 0.  A non-finite or negative value, a touch_lag outside 0..31 or a p_drop outside
        [0, 1) raises and keeps the previous constants."""
        unknown = set(constants) - set(_ZERO)
        if unknown:
            raise TypeError(f"unknown sensor constants {sorted(unknown)}")
        new = dict(getattr(self.engine, "sensor_constants", None) or dict(_ZERO, seed=0))
        new.update(constants)
        if seed is not None:
            new["seed"] = int(seed)
        if not 0 <= new["seed"] < 2 ** 64:
            raise ValueError("the seed lies in 0 .. 2^64 - 1")
        _lib.check(self._ctx, self.lib.mpcqp_set_sensors(
            self._ctx, new["seed"], *(float(new[k]) for k in ("sigma_gyro", "sigma_accel", "walk_gyro", "walk_accel",
                                                             "bias0_gyro", "bias0_accel", "sigma_q", "sigma_qd", "q_lsb")),
            int(new["touch_lag"]), float(new["p_drop"])), "mpcqp_set_sensors")
        self.engine.sensor_constants = new

    @property
    def constants(self):
        return dict(self.engine.sensor_constants)

    def reset(self, robots=None):
        """Zero the records of all or some robots (indices, a slice or a mask) and write their id,
        the row index: their next update draws a fresh turn-on bias and starts their touch
        histories from the reading it sees, with the draws of call 0."""
        idx = slice(None) if robots is None else robots
        ids = torch.arange(self.B, dtype=torch.float64, device=self.device)
        self.state[idx] = 0.0
        self.state[idx, _ID] = ids[idx]
        self._status[idx] = 0

    def _inputs(self, gyro, accel, dofs, touch):
        if self.plant is not None:
            gyro = self.plant.gyro if gyro is None else gyro
            accel = self.plant.accel if accel is None else accel
            dofs = self.plant.dofs if dofs is None else dofs
            touch = self.plant.touch if touch is None else touch
        return gyro, accel, dofs, touch

    def bind_update(self, gyro=None, accel=None, dofs=None, touch=None, first=0, count=None):
        """``update`` with its checks made and its device pointers resolved once: returns
        ``launch(stream)`` (see BatchedPlant.bind_step), e.g. for capture into a HIP graph.  The
        inputs default to the plant's; without a plant an input that is None is left out together
        with its output.  An input may be the output buffer itself (``sens.gyro`` ...).
        ``first``, ``count``: the rows [first, first + count) alone, through offset pointers; each
        robot draws what the whole-batch call draws, since its id is in its record."""
        B = self.B
        count = B - first if count is None else count
        if not (0 <= first and 0 <= count and first + count <= B):
            raise ValueError(f"sensors: rows [{first}, {first + count}) outside the batch of {B}")
        gyro, accel, dofs, touch = self._inputs(gyro, accel, dofs, touch)
        for name, t, n in (("gyro", gyro, 3), ("accel", accel, 3), ("dofs", dofs, 24), ("touch", touch, 4),
                           ("scale", self.scale, 1)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_contiguous()
                                      and t.device == self.device and t.numel() == B * n):
                what = f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', 'the host')}"
                raise ValueError(f"sensors: {name} must be a contiguous float32 tensor of {B} x {n} values on "
                                 f"{self.device}, got {what}")
        lib, ctx = self.lib, self._ctx
        out = lambda t, o, n: _ptr(None if t is None else o, first, n)
        args = (ctx, count, 0, _ptr(gyro, first, 3), _ptr(accel, first, 3), _ptr(dofs, first, 24), _ptr(touch, first, 4),
                _ptr(self.scale, first, 1), _ptr(self.state, first, SENSE_STRIDE), out(gyro, self.gyro, 3),
                out(accel, self.accel, 3), out(dofs, self.dofs, 24), out(touch, self.touch, 4),
                _ptr(self._status, first, 1))

        def launch(stream):
            _lib.check(ctx, lib.mpcqp_sensors(*args, ctypes.c_void_p(stream.cuda_stream)), "mpcqp_sensors")
        launch.buffers = (gyro, accel, dofs, touch, self.scale, self.state)
        return launch

    def update(self, gyro=None, accel=None, dofs=None, touch=None, stream=None):
        """The one launch per control iteration: fills ``gyro``, ``accel``, ``dofs``, ``touch`` and
        ``status`` from the plant's outputs (or the tensors given) and advances every accepted
        robot's record.  The pointer tuple is bound once per set of buffers."""
        ins = self._inputs(gyro, accel, dofs, touch)
        key = tuple(None if t is None else t.data_ptr() for t in ins + (self.scale,))
        launch = self._bound.get(key)
        if launch is None:
            if len(self._bound) >= 8:
                self._bound.clear()
            launch = self._bound[key] = self.bind_update(*ins)
        launch(torch.cuda.current_stream(self.device) if stream is None else stream)

    # ---- views of the records
    @property
    def bias_gyro(self):
        """[B,3] float64: the gyro's bias in force (rad/s)."""
        return self.state[:, _BIAS_G:_BIAS_G + 3]

    @property
    def bias_accel(self):
        """[B,3] float64: the accelerometer's bias in force (m/s^2)."""
        return self.state[:, _BIAS_A:_BIAS_A + 3]

    @property
    def count(self):
        """[B] float64: the number of accepted updates since reset."""
        return self.state[:, _COUNT]

    @property
    def history(self):
        """[B,4] float64: each foot's last 32 readings as an integer, bit k the reading k calls ago."""
        return self.state[:, _HIST:_HIST + 4]

    @property
    def status(self):
        """[B] int32: STATUS_OK, or STATUS_NONFINITE for a robot with a non-finite input, scale or
        record word (or a count, id or history outside its integer's range), whose record is
        untouched and whose outputs are its inputs."""
        return self._status

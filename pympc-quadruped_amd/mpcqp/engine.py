"""Batched convex-MPC QP engine (host side).

``LinearMpc(...).solve(state, xref, contact_schedule, feet=...)`` formulates
and solves B independent reference MPC QPs in one HIP launch and returns the
first-step ground-reaction forces u0[B, 12] -- the batched form of
``ModelPredictiveController._solve_mpc(...)[0:12]``
(/root/reference/linear_mpc/mpc.py:262-290, :99).

torch-ROCm tensors are storage only: inputs are moved (zero-copy when they are
already contiguous float32 tensors on the engine's device) and the compute is
the HIP kernel behind ``libmpcqp.so`` (include/mpcqp.h).  There is no CPU path.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .params import (DT_MPC, Q_DIAG, R_DIAG, ROBOT_PRESETS, ROBOT_STRIDE, pack_robot)


def _weights(W, n, name):
    """(diagonal, full) from a length-n vector or an n x n matrix: ``full`` is the
    row-major float64 matrix when it has off-diagonal entries (mpcqp_set_weights),
    else None (the diagonal fast path; mpc.py:50,52 build Qbar / Rbar by kron)."""
    W = np.asarray(W, dtype=np.float64)
    if W.shape == (n,):
        return W, None
    if W.shape == (n, n):
        if np.any(W - np.diag(np.diag(W)) != 0.0):
            if not np.allclose(W, W.T, rtol=0.0, atol=1e-12 * max(np.abs(W).max(), 1e-300)):
                raise ValueError(f"{name} is not symmetric")
            return np.diag(W).copy(), np.ascontiguousarray(W)
        return np.diag(W).copy(), None
    raise ValueError(f"{name}: expected ({n},) or ({n}, {n}), got {W.shape}")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


class SolveResult:
    """u0[B,12] plus optional U[B,N,12], status[B], iterations[B] (device tensors)."""

    def __init__(self, u0, U, status, iters):
        self.u0, self.U, self.status, self.iterations = u0, U, status, iters


class PredictResult:
    """What ``LinearMpc.predict`` returns (include/mpcqp_predict_abi.h mpcqp_predict), device tensors: X
    [B,N,13] float32, the predicted states x_1 .. x_N; cost, cost_free, cone_margin and
    swing_residual [B] float64, views of the one ``report`` tensor [B,PREDICT_REPORT]; status [B]
    int32 (STATUS_OK or STATUS_NONFINITE, whose X and report are zeros).  ``cost - cost_free`` is
    the QP's objective 1/2 U^T H U + g^T U."""

    def __init__(self, X, report, status):
        self.X, self.report, self.status = X, report, status
        self.cost, self.cost_free = report[:, 0], report[:, 1]
        self.cone_margin, self.swing_residual = report[:, 2], report[:, 3]


class CertifyResult:
    """What ``LinearMpc.certify`` returns (include/mpcqp_certify_abi.h mpcqp_certify), device
    tensors: G [B,N,12] float32, the gradient H U + g of the QP's objective phi at U; objective,
    gap, lower and worst [B] float64, views of the one ``report`` tensor [B,CERTIFY_REPORT];
    status [B] int32 (STATUS_OK or STATUS_NONFINITE, whose G and report are zeros).
    ``lower = objective - gap`` never exceeds the optimum phi*; for a feasible U
    ``objective - phi* <= gap``.  The gap is a first-order bound: tight at the optimum and loose
    far from it."""

    def __init__(self, G, report, status):
        self.G, self.report, self.status = G, report, status
        self.objective, self.gap = report[:, 0], report[:, 1]
        self.lower, self.worst = report[:, 2], report[:, 3]


class LinearMpc:
    """Batched reference MPC: one QP per robot, solved on one MI355X.

    Args:
      horizon:  N (LinearMpcConfig.horizon, config/linear_mpc_configs.py:11)
      robot:    default per-robot parameters: a preset name ("a1", "aliengo"),
                a reference RobotConfig class, or a packed [16] record.
      dt:       model step (hard-coded 0.05 in mpc.py:38)
      Q, R:     weights (linear_mpc_configs.py:19-20): [13] / [12] diagonals or full
                symmetric 13 x 13 / 12 x 12 matrices (set_weights)
      device:   torch device of the HIP context (default cuda:0)
      max_iter: active-set iteration cap per robot (0 = engine default)
      max_stance: optional promise of at most this many stance foot-steps per
                robot (lets the engine skip larger capacity classes)
    """

    def __init__(self, horizon=16, robot="aliengo", dt=DT_MPC, Q=Q_DIAG, R=R_DIAG,
                 device="cuda:0", max_iter=0, max_stance=0):
        self.horizon = int(horizon)
        if not 1 <= self.horizon <= _lib.MAX_HORIZON:
            raise ValueError(f"horizon {self.horizon} outside the engine's 1..{_lib.MAX_HORIZON} "
                             "(MPCQP_MAX_HORIZON, include/mpcqp.h)")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("LinearMpc runs on a HIP device only (no CPU path)")
        self.lib = _lib.load()
        p = _lib.default_params(self.horizon)
        p.dt = float(dt)
        p.max_iter = int(max_iter)
        qd, qf = _weights(Q, 13, "Q")
        rd, rf = _weights(R, 12, "R")
        for i, v in enumerate(qd):
            p.q_diag[i] = float(v)
        for i, v in enumerate(rd):
            p.r_diag[i] = float(v)
        self.params = p
        ctx = ctypes.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _lib.check(None, self.lib.mpcqp_create(ctypes.byref(p), int(idx), ctypes.byref(ctx)),
                   "mpcqp_create")
        self._ctx = ctx
        if qf is not None or rf is not None:
            self.set_weights(Q, R)
        self._hint = (0, 0)
        if max_stance:
            self.set_stance_hint(max_stance)
        self.default_robot = self._robot_record(robot)

    def set_weights(self, Q, R):
        """Replace the cost weights (include/mpcqp.h mpcqp_set_weights): diagonals or full
        symmetric matrices (every capacity class takes any symmetric Q and R; a cross-leg R
        runs the interior-point class's 12 x 12 stage-weight instantiations)."""
        qd, qf = _weights(Q, 13, "Q")
        rd, rf = _weights(R, 12, "R")
        qm = np.ascontiguousarray(qf if qf is not None else np.diag(qd), dtype=np.float64)
        rm = np.ascontiguousarray(rf if rf is not None else np.diag(rd), dtype=np.float64)
        _lib.check(self._ctx, self.lib.mpcqp_set_weights(self._ctx, qm.ctypes.data, rm.ctypes.data),
                   "mpcqp_set_weights")
        self.weights = (qm, rm)

    def set_stance_hint(self, max_stance):
        """Promise at most ``max_stance`` stance foot-steps per robot in the following
        solves (0 = no promise): capacity classes above 3 * max_stance variables are
        not launched.  A robot breaking the promise gets MPCQP_STATUS_TOO_LARGE."""
        self.set_stance_range(0, max_stance)

    def set_stance_range(self, min_stance, max_stance):
        """Promise between ``min_stance`` and ``max_stance`` stance foot-steps per robot
        (include/mpcqp.h): only the capacity classes the range can need are launched,
        the first of them directly on the batch (the drop-in passes the exact count)."""
        rng = (int(min_stance), int(max_stance))
        if rng != getattr(self, "_hint", None):
            _lib.check(self._ctx, self.lib.mpcqp_set_stance_range(self._ctx, *rng), "set_stance_range")
            self._hint = rng

    def set_order(self, mode):
        """Dispatch order of the following solves (include/mpcqp.h mpcqp_set_order): 1 (the
        default) deals each launch's robots to workgroups largest predicted solve time first,
        0 keeps the batch order.  Results are bitwise the same either way."""
        _lib.check(self._ctx, self.lib.mpcqp_set_order(self._ctx, int(mode)), "mpcqp_set_order")

    def set_warm_start(self, capacity):
        """Remember each robot's verified active set between solves (include/mpcqp.h
        mpcqp_set_warm_start): robot b of every later solve starts the interior-point class
        (n > 128, e.g. Gait.STANDING at N = 16) from the rows its previous solve had active,
        and runs the interior point only when they fail the KKT check.  For callers that
        solve the same robots tick after tick; results do not depend on it.  ``capacity`` =
        robots remembered (robot indices 0 .. capacity - 1), 0 disables.  Returns the
        engine-owned device memory (uint8 [capacity, WARM_BYTES]); zero it to forget.
        Replacing it releases the previous memory to torch's allocator on the current
        stream: call it between solves issued on that stream."""
        cap = int(capacity)
        if cap < 0:
            raise ValueError("capacity must be >= 0")
        mem = torch.zeros((cap, _lib.WARM_BYTES), dtype=torch.uint8, device=self.device) if cap else None
        _lib.check(self._ctx, self.lib.mpcqp_set_warm_start(self._ctx, mem.data_ptr() if cap else None, cap),
                   "mpcqp_set_warm_start")
        self._warm = mem   # the context holds its pointer: keep it alive
        return mem

    def __del__(self):
        ctx = getattr(self, "_ctx", None)
        if ctx is not None and ctx.value:
            try:
                self.lib.mpcqp_destroy(ctx)
            except Exception:
                pass
            self._ctx = None

    @staticmethod
    def _robot_record(robot):
        if robot is None:
            return None
        if isinstance(robot, str):
            return pack_robot(ROBOT_PRESETS[robot])
        if hasattr(robot, "mass_base"):
            from .params import robot_from_config
            return robot_from_config(robot)
        rec = np.asarray(robot, dtype=np.float32).reshape(-1)
        if rec.shape[0] != ROBOT_STRIDE:
            raise ValueError(f"robot record must have {ROBOT_STRIDE} entries")
        return rec

    def _dev(self, a, shape, name):
        t = torch.as_tensor(a)
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(t.shape) != tuple(shape):
            try:
                t = t.reshape(shape)
            except RuntimeError:
                raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
        return t

    def _stream_ptr(self, stream):
        """The launch stream of a call as the ABI's ``void* stream``: ``stream``, or the
        device's current stream for None."""
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        return ctypes.c_void_p(stream.cuda_stream)

    def solve(self, state, xref, contact_schedule, feet, robot=None, return_all=False, stream=None):
        """Formulate + solve B QPs.

        state:            [B,13] x0 (mpc.py:65-77) -- x0[2] is the yaw of the model
        xref:             [B,N,13] or [B,13N] reference (mpc.py:154-168)
        contact_schedule: [B,N,4] or [B,4N] gait table (gait.py:81-100)
        feet:             [B,4,3] foot positions relative to the CoM, world frame
        robot:            [B,16] per-robot records, or one record / preset for all
        Returns u0 [B,12] (device tensor), or a SolveResult if return_all.
        """
        st = torch.as_tensor(state)
        B = int(st.shape[0]) if st.dim() == 2 else 1
        N = self.horizon
        cur = torch.cuda.current_stream(self.device)
        if stream is None:
            stream = cur
        elif stream != cur:
            # inputs produced (or copied below) on the current stream must be ready
            # before the launch stream reads them
            stream.wait_stream(cur)
        with torch.cuda.stream(stream):
            return self._solve_on(stream, state, xref, contact_schedule, feet, robot, return_all, B, N)

    def _solve_on(self, stream, state, xref, contact_schedule, feet, robot, return_all, B, N):
        x0 = self._dev(state, (B, 13), "state")
        xr = self._dev(xref, (B, N, 13), "xref")
        ct = self._dev(contact_schedule, (B, N, 4), "contact_schedule")
        ft = self._dev(feet, (B, 4, 3), "feet")
        if robot is None:
            if self.default_robot is None:
                raise ValueError("no robot parameters")
            rb = torch.as_tensor(np.tile(self.default_robot, (B, 1)))
        else:
            r = robot if not isinstance(robot, str) and not hasattr(robot, "mass_base") else None
            if r is None:
                rb = torch.as_tensor(np.tile(self._robot_record(robot), (B, 1)))
            else:
                rt = torch.as_tensor(r)
                rb = rt.reshape(1, -1).expand(B, -1) if rt.dim() == 1 else rt
        rb = self._dev(rb, (B, ROBOT_STRIDE), "robot")
        u0 = torch.empty((B, 12), dtype=torch.float32, device=self.device)
        U = torch.empty((B, N, 12), dtype=torch.float32, device=self.device) if return_all else None
        status = torch.empty((B,), dtype=torch.int32, device=self.device)
        iters = torch.empty((B,), dtype=torch.int32, device=self.device)
        code = self.lib.mpcqp_solve(self._ctx, B, _ptr(x0), _ptr(xr), _ptr(ct), _ptr(ft), _ptr(rb),
                                    _ptr(u0), _ptr(U), _ptr(status), _ptr(iters),
                                    ctypes.c_void_p(stream.cuda_stream))
        _lib.check(self._ctx, code, "mpcqp_solve")
        # the caching allocator must not hand these blocks to other streams' work
        # before the launch has finished with them
        for t in (x0, xr, ct, ft, rb, u0, U, status, iters):
            if t is not None and t.numel():
                t.record_stream(stream)
        if return_all:
            return SolveResult(u0, U, status, iters)
        return u0

    def solve_raw(self, B, x0, xref, contact, feet, robot, u0, U=None, status=None, iters=None,
                  stream=None):
        """Zero-overhead launch on preallocated contiguous float32 device tensors."""
        s = self._stream_ptr(stream)
        code = self.lib.mpcqp_solve(self._ctx, int(B), _ptr(x0), _ptr(xref), _ptr(contact),
                                    _ptr(feet), _ptr(robot), _ptr(u0), _ptr(U), _ptr(status),
                                    _ptr(iters), s)
        _lib.check(self._ctx, code, "mpcqp_solve")

    def bind_solve(self, B, x0, xref, contact, feet, robot, u0, U=None, status=None, iters=None):
        """solve_raw with its device pointers resolved once: returns ``launch(stream)``.
        For callers that reuse the same preallocated buffers every tick (the drop-in
        controller): the per-call cost is then one ctypes call."""
        lib, ctx = self.lib, self._ctx
        args = (ctx, int(B), _ptr(x0), _ptr(xref), _ptr(contact), _ptr(feet), _ptr(robot), _ptr(u0), _ptr(U),
                _ptr(status), _ptr(iters))
        keep = (x0, xref, contact, feet, robot, u0, U, status, iters)   # the pointers' owners stay alive

        def launch(stream):
            _lib.check(ctx, lib.mpcqp_solve(*args, ctypes.c_void_p(stream.cuda_stream)), "mpcqp_solve")
        launch.buffers = keep
        return launch

    def predict(self, state, xref, contact_schedule, feet, U, robot=None, stream=None):
        """The trajectory the QP believes the force sequence ``U`` produces, its tracking cost,
        cone margin and swing residual (include/mpcqp_predict_abi.h mpcqp_predict; com_traj = Sx x0 + Su U,
        mpc.py:293-294), for B robots in one launch.

        state, xref, contact_schedule, feet, robot: as for ``solve``.  U: [B,N,12] or [B,12N],
        usually ``solve(..., return_all=True).U``; every entry is used as given.  Returns a
        PredictResult (device tensors)."""
        return PredictResult(*self._evaluate(self.predict_raw, 13, _lib.PREDICT_REPORT, state, xref, contact_schedule,
                                             feet, U, robot, stream))

    def _evaluate(self, raw, out_cols, report_words, state, xref, contact_schedule, feet, U, robot, stream):
        """What predict and certify share: the inputs brought to the device, the three outputs
        allocated ([B,N,out_cols] float32, the report, the status) and ``raw`` launched on them."""
        st = torch.as_tensor(state)
        B = int(st.shape[0]) if st.dim() == 2 else 1
        N = self.horizon
        cur = torch.cuda.current_stream(self.device)
        if stream is None:
            stream = cur
        elif stream != cur:
            stream.wait_stream(cur)   # as solve: inputs made on the current stream must be ready
        with torch.cuda.stream(stream):
            x0 = self._dev(state, (B, 13), "state")
            xr = self._dev(xref, (B, N, 13), "xref")
            ct = self._dev(contact_schedule, (B, N, 4), "contact_schedule")
            ft = self._dev(feet, (B, 4, 3), "feet")
            Ut = self._dev(U, (B, N, 12), "U")
            if robot is None or isinstance(robot, str) or hasattr(robot, "mass_base"):
                rec = self.default_robot if robot is None else self._robot_record(robot)
                if rec is None:
                    raise ValueError("no robot parameters")
                rb = torch.as_tensor(np.tile(rec, (B, 1)))
            else:
                rt = torch.as_tensor(robot)
                rb = rt.reshape(1, -1).expand(B, -1) if rt.dim() == 1 else rt
            rb = self._dev(rb, (B, ROBOT_STRIDE), "robot")
            out = torch.empty((B, N, out_cols), dtype=torch.float32, device=self.device)
            report = torch.empty((B, report_words), dtype=torch.float64, device=self.device)
            status = torch.empty((B,), dtype=torch.int32, device=self.device)
            raw(B, x0, xr, ct, ft, rb, Ut, out, report, status, stream=stream)
            for t in (x0, xr, ct, ft, rb, Ut, out, report, status):
                if t.numel():
                    t.record_stream(stream)
        return out, report, status

    def _eval_args(self, call, B, x0, xref, contact, feet, robot, U, out_name, out, out_cols, report, report_words,
                   status):
        """The argument tuple of mpcqp_predict / mpcqp_certify after the checks every caller
        shares: contiguous tensors of the right dtype and size on the engine's device (the kernel
        reads and writes B rows of each); the three outputs may be None."""
        B, N = int(B), self.horizon
        f32 = torch.float32
        for name, t, shape, dtype, need in (
                ("x0", x0, (B, 13), f32, True), ("xref", xref, (B, N, 13), f32, True),
                ("contact", contact, (B, N, 4), f32, True), ("feet", feet, (B, 4, 3), f32, True),
                ("robot", robot, (B, ROBOT_STRIDE), f32, True), ("U", U, (B, N, 12), f32, True),
                (out_name, out, (B, N, out_cols), f32, False), ("report", report, (B, report_words), torch.float64, False),
                ("status", status, (B,), torch.int32, False)):
            if t is None:
                if need:
                    raise ValueError(f"{call}: {name} is required")
                continue
            if not (t.dtype == dtype and t.is_contiguous() and t.device == self.device
                    and t.numel() == int(np.prod(shape))):
                raise ValueError(f"{call}: {name} must be a contiguous {dtype} tensor of shape {list(shape)} on "
                                 f"{self.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        return (self._ctx, B, 0, _ptr(x0), _ptr(xref), _ptr(contact), _ptr(feet), _ptr(robot), _ptr(U), _ptr(out),
                _ptr(report), _ptr(status))

    def _predict_args(self, B, x0, xref, contact, feet, robot, U, X, report, status):
        """The argument tuple of mpcqp_predict after the checks every caller shares."""
        return self._eval_args("predict", B, x0, xref, contact, feet, robot, U, "X", X, 13, report,
                               _lib.PREDICT_REPORT, status)

    def predict_raw(self, B, x0, xref, contact, feet, robot, U, X=None, report=None, status=None, stream=None):
        """mpcqp_predict on preallocated contiguous device tensors (float32; report [B,PREDICT_REPORT]
        float64, status [B] int32): one launch on ``stream`` (default: the current stream), no
        allocation or synchronisation.  X, report and status are each optional; a tensor of the
        wrong dtype, size or device raises ValueError."""
        args = self._predict_args(B, x0, xref, contact, feet, robot, U, X, report, status)
        _lib.check(self._ctx, self.lib.mpcqp_predict(*args, self._stream_ptr(stream)), "mpcqp_predict")

    def bind_predict(self, B, x0, xref, contact, feet, robot, U, X=None, report=None, status=None):
        """predict_raw with its checks made and its device pointers resolved once: returns
        ``launch(stream)`` (see bind_solve), e.g. for capture into a HIP graph."""
        lib, ctx = self.lib, self._ctx
        args = self._predict_args(B, x0, xref, contact, feet, robot, U, X, report, status)
        keep = (x0, xref, contact, feet, robot, U, X, report, status)   # the pointers' owners stay alive

        def launch(stream):
            _lib.check(ctx, lib.mpcqp_predict(*args, ctypes.c_void_p(stream.cuda_stream)), "mpcqp_predict")
        launch.buffers = keep
        return launch

    def certify(self, state, xref, contact_schedule, feet, U, robot=None, stream=None):
        """How far the force sequence ``U`` is from the QP's optimum (include/mpcqp_certify_abi.h
        mpcqp_certify), for B robots in one launch: the gradient G = H U + g of the objective
        phi(U) = cost - cost_free, phi(U) itself, and the duality gap the friction pyramids give in
        closed form, with ``lower = objective - gap <= phi*`` for any finite U and
        ``0 <= phi(U) - phi* <= gap`` for a feasible one.  The gap is a first-order bound: tight
        at the optimum and loose far from it.

        Arguments as for ``predict``.  Returns a CertifyResult (device tensors)."""
        return CertifyResult(*self._evaluate(self.certify_raw, 12, _lib.CERTIFY_REPORT, state, xref, contact_schedule,
                                             feet, U, robot, stream))

    def _certify_args(self, B, x0, xref, contact, feet, robot, U, G, report, status):
        """The argument tuple of mpcqp_certify after the checks every caller shares."""
        return self._eval_args("certify", B, x0, xref, contact, feet, robot, U, "G", G, 12, report,
                               _lib.CERTIFY_REPORT, status)

    def certify_raw(self, B, x0, xref, contact, feet, robot, U, G=None, report=None, status=None, stream=None):
        """mpcqp_certify on preallocated contiguous device tensors (float32; G [B,N,12]; report
        [B,CERTIFY_REPORT] float64, status [B] int32): one launch on ``stream`` (default: the
        current stream), no allocation or synchronisation.  G, report and status are each
        optional; a tensor of the wrong dtype, size or device raises ValueError."""
        args = self._certify_args(B, x0, xref, contact, feet, robot, U, G, report, status)
        _lib.check(self._ctx, self.lib.mpcqp_certify(*args, self._stream_ptr(stream)), "mpcqp_certify")

    def bind_certify(self, B, x0, xref, contact, feet, robot, U, G=None, report=None, status=None):
        """certify_raw with its checks made and its device pointers resolved once: returns
        ``launch(stream)`` (see bind_solve), e.g. for capture into a HIP graph."""
        lib, ctx = self.lib, self._ctx
        args = self._certify_args(B, x0, xref, contact, feet, robot, U, G, report, status)
        keep = (x0, xref, contact, feet, robot, U, G, report, status)   # the pointers' owners stay alive

        def launch(stream):
            _lib.check(ctx, lib.mpcqp_certify(*args, ctypes.c_void_p(stream.cuda_stream)), "mpcqp_certify")
        launch.buffers = keep
        return launch

    # ---- the hot path's callers on the device (include/mpcqp.h) ----

    def set_planner(self, dt_control=0.001, gravity=9.81, max_pos_error=0.1):
        """Planner constants (linear_mpc_configs.py:6,13; mpc.py:121).  A non-finite value, or a
        negative dt_control / max_pos_error, raises and keeps the previous constants."""
        _lib.check(self._ctx, self.lib.mpcqp_set_planner(self._ctx, float(dt_control), float(gravity),
                                                         float(max_pos_error)), "mpcqp_set_planner")

    def plan(self, flags, plan_state, x0, vel_body_des, yaw_rate_des, quat=None, pos=None, omega=None,
             vel=None, rot=None, root_states=None, gait=None, iteration=None, height_des=None, xref=None,
             contact=None, stream=None):
        """One control iteration of state packing + pose integration, and on an MPC
        tick the reference trajectory and gait table (mpc.py:55-170, gait.py:76-100).
        ``flags``: True / PLAN_REFERENCE on an MPC tick, PLAN_NO_INTEGRATE to skip the
        integrators (include/mpcqp.h).

        Every argument is a preallocated contiguous device tensor (float32, except
        plan_state / vel_body_des / yaw_rate_des float64 and gait / iteration int32);
        ``root_states`` [B,13] (Isaac Gym layout) replaces quat/pos/omega/vel/rot."""
        s = self._stream_ptr(stream)
        B = int(plan_state.shape[0])
        if root_states is not None:
            code = self.lib.mpcqp_plan_root_states(
                self._ctx, B, int(flags), _ptr(root_states), _ptr(vel_body_des), _ptr(yaw_rate_des),
                _ptr(gait), _ptr(iteration), _ptr(height_des), _ptr(plan_state), _ptr(x0), _ptr(xref),
                _ptr(contact), s)
        else:
            code = self.lib.mpcqp_plan(
                self._ctx, B, int(flags), _ptr(quat), _ptr(pos), _ptr(omega), _ptr(vel), _ptr(rot),
                _ptr(vel_body_des), _ptr(yaw_rate_des), _ptr(gait), _ptr(iteration), _ptr(height_des),
                _ptr(plan_state), _ptr(x0), _ptr(xref), _ptr(contact), s)
        _lib.check(self._ctx, code, "mpcqp_plan")

    def bind_plan(self, plan_state, x0, vel_body_des, yaw_rate_des, quat, pos, omega, vel, rot, height_des,
                  xref):
        """plan() (split state inputs) with its device pointers resolved once: returns
        ``launch(flags, stream)`` (see bind_solve)."""
        lib, ctx = self.lib, self._ctx
        B = int(plan_state.shape[0])
        head = (_ptr(quat), _ptr(pos), _ptr(omega), _ptr(vel), _ptr(rot), _ptr(vel_body_des), _ptr(yaw_rate_des),
                _ptr(None), _ptr(None), _ptr(height_des), _ptr(plan_state), _ptr(x0), _ptr(xref), _ptr(None))
        keep = (plan_state, x0, vel_body_des, yaw_rate_des, quat, pos, omega, vel, rot, height_des, xref)

        def launch(flags, stream):
            _lib.check(ctx, lib.mpcqp_plan(ctx, B, int(flags), *head, ctypes.c_void_p(stream.cuda_stream)),
                       "mpcqp_plan")
        launch.buffers = keep
        return launch

    def stance_torques(self, jac, stance, u0, tau, stance_stride=4, stream=None):
        """tau = Jv_leg^T (-f_leg) for stance legs (leg_controller.py:86-89).

        jac [B,4,3,3] float32 (each leg's 3x3 Jacobian block), stance [B, >=4]
        (> 0 = stance) read with ``stance_stride``, u0 / tau [B,12]."""
        s = self._stream_ptr(stream)
        B = int(u0.shape[0])
        code = self.lib.mpcqp_stance_torques(self._ctx, B, _ptr(jac), _ptr(stance), int(stance_stride), _ptr(u0),
                                             _ptr(tau), s)
        _lib.check(self._ctx, code, "mpcqp_stance_torques")

    def set_swing(self, swing_height=0.1, Kp=None, Kd=None, touchdown_z=-0.0255, vel_gain=0.03):
        """Swing constants (include/mpcqp.h mpcqp_set_swing): the curve's apex height (a world
        z, robot_configs.py:54), the PD gains -- a scalar, a diagonal or a 3 x 3 matrix, None
        keeps the current one (robot_configs.py:55-56) -- the foothold's world z and the gain
        of its velocity-error term (swing_foot_trajectory_generator.py:116,120).  Like
        set_planner, every call sets all three scalars (an omitted one returns to its default);
        launches already issued keep the constants they were issued with."""
        def gain(k):
            if k is None:
                return None
            k = np.asarray(k, dtype=np.float64)
            if k.ndim == 0:
                k = k * np.eye(3)
            elif k.ndim == 1:
                k = np.diag(k)
            if k.shape != (3, 3):
                raise ValueError("a swing gain is a scalar, 3 diagonal entries or a 3 x 3 matrix")
            return np.ascontiguousarray(k)
        kp, kd = gain(Kp), gain(Kd)
        code = self.lib.mpcqp_set_swing(self._ctx, float(swing_height), kp.ctypes.data if kp is not None else None,
                                        kd.ctypes.data if kd is not None else None, float(touchdown_z),
                                        float(vel_gain))
        _lib.check(self._ctx, code, "mpcqp_set_swing")
        self.touchdown_z = float(touchdown_z)   # the plant's level ground follows it until it is given one

    def leg_torques(self, tick, iterations_between_mpc, vel_body_des, yaw_rate_des, gait, thighs, pos_feet,
                    foot_pos_base, foot_vel_base, jac, u0, swing_mem, tau, quat=None, pos=None, vel=None, rot=None,
                    root_states=None, swing_state=None, pos_target=None, vel_target=None, stream=None):
        """All 12 joint torques of every robot for one control iteration (include/mpcqp.h
        mpcqp_leg_torques; isaacgym_a1.py:137-162): swing state, foot placement, swing
        trajectory, swing PD and stance torques in one launch.

        Every argument is a preallocated contiguous device tensor: tick [B] / gait [B,9]
        int32, vel_body_des [B,3] / yaw_rate_des [B] / swing_mem [B,SWING_STRIDE] float64,
        the rest float32 (thighs, pos_feet, foot_pos_base, foot_vel_base [B,4,3], jac
        [B,4,3,3], u0 / tau [B,12]).  ``root_states`` [B,13] (Isaac Gym layout) replaces
        quat/pos/vel/rot.  swing_state [B,4], pos_target / vel_target [B,4,3] are optional
        outputs."""
        s = self._stream_ptr(stream)
        B = int(tau.shape[0])
        tail = (_ptr(vel_body_des), _ptr(yaw_rate_des), _ptr(gait), _ptr(thighs), _ptr(pos_feet),
                _ptr(foot_pos_base), _ptr(foot_vel_base), _ptr(jac), _ptr(u0), _ptr(swing_mem), _ptr(tau),
                _ptr(swing_state), _ptr(pos_target), _ptr(vel_target), s)
        if root_states is not None:
            code = self.lib.mpcqp_leg_torques_root_states(self._ctx, B, 0, _ptr(tick), int(iterations_between_mpc),
                                                          _ptr(root_states), *tail)
        else:
            code = self.lib.mpcqp_leg_torques(self._ctx, B, 0, _ptr(tick), int(iterations_between_mpc), _ptr(quat),
                                              _ptr(pos), _ptr(vel), _ptr(rot), *tail)
        _lib.check(self._ctx, code, "mpcqp_leg_torques")

    def kinematics(self, geom, q=None, qdot=None, quat=None, pos=None, vel=None, omega=None, rot=None,
                   root_states=None, dof_states=None, feet=None, thighs=None, pos_feet=None, foot_pos_base=None,
                   foot_vel_base=None, jac=None, stream=None):
        """Leg kinematics of every robot (include/mpcqp.h mpcqp_kinematics; RobotData.update,
        robot_data.py:59-108): foot and thigh positions, foot Jacobians and foot velocities
        in one launch -- the ``feet`` of ``solve`` and the five kinematic inputs of
        ``leg_torques``.

        Every argument is a preallocated contiguous device tensor: geom [B,KIN_STRIDE]
        float64 (params.pack_leg_geometry), the rest float32.  Inputs: quat [B,4] (w, x, y,
        z), pos / vel / omega [B,3], optional rot [B,3,3], q / qdot [B,12]; or ``root_states``
        [B,13] and ``dof_states`` [B,12,2] (Isaac Gym layout) in their place.  Outputs, each
        optional: feet, thighs, pos_feet, foot_pos_base, foot_vel_base [B,4,3], jac
        [B,4,3,3]."""
        s = self._stream_ptr(stream)
        B = int(geom.shape[0])
        tail = (_ptr(geom), _ptr(feet), _ptr(thighs), _ptr(pos_feet), _ptr(foot_pos_base), _ptr(foot_vel_base),
                _ptr(jac), s)
        if (root_states is None) != (dof_states is None):
            raise ValueError("kinematics: root_states and dof_states go together")
        if root_states is not None:
            code = self.lib.mpcqp_kinematics_root_states(self._ctx, B, 0, _ptr(root_states), _ptr(dof_states), *tail)
        else:
            code = self.lib.mpcqp_kinematics(self._ctx, B, 0, _ptr(quat), _ptr(pos), _ptr(vel), _ptr(omega),
                                             _ptr(rot), _ptr(q), _ptr(qdot), *tail)
        _lib.check(self._ctx, code, "mpcqp_kinematics")

    def bind_kinematics(self, geom, quat, pos, vel, omega, rot, q, qdot, feet=None, thighs=None, pos_feet=None,
                        foot_pos_base=None, foot_vel_base=None, jac=None):
        """kinematics() (split state inputs) with its device pointers resolved once: returns
        ``launch(stream)`` (see bind_solve)."""
        lib, ctx = self.lib, self._ctx
        B = int(geom.shape[0])
        keep = (quat, pos, vel, omega, rot, q, qdot, geom, feet, thighs, pos_feet, foot_pos_base, foot_vel_base, jac)
        args = (ctx, B, 0) + tuple(_ptr(t) for t in keep)

        def launch(stream):
            _lib.check(ctx, lib.mpcqp_kinematics(*args, ctypes.c_void_p(stream.cuda_stream)), "mpcqp_kinematics")
        launch.buffers = keep
        return launch

    def step(self, flags, iter_counter, iterations_between_mpc, root_states, dof_states, geom, vel_body_des,
             yaw_rate_des, gait, plan_state, swing_mem, x0, u0, tau, tick=None, height_des=None, robot=None,
             xref=None, contact=None, feet=None, status=None, iters=None, thighs=None, pos_feet=None,
             foot_pos_base=None, foot_vel_base=None, jac=None, swing_state=None, pos_target=None,
             vel_target=None, stream=None):
        """One whole control iteration of every robot in one call (include/mpcqp.h mpcqp_step;
        isaacgym_a1.py:117-162): with ``flags`` 0 one launch -- kinematics, state packing, pose
        integration and all 12 joint torques, the kinematic arrays never leaving the registers
        unless asked for; with STEP_MPC the plan with the reference, the solve and the leg
        controller on the fresh u0, enqueued by one call.  Bitwise what ``kinematics``, ``plan``,
        ``solve_raw`` and ``leg_torques`` give on the same buffers.

        Every argument is a preallocated contiguous device tensor, as for those four:
        root_states [B,13] and dof_states [B,12,2] (Isaac Gym layout).  ``tick`` [B] int32 is
        each robot's counter; None gives every robot the scalar ``iter_counter``.  height_des,
        robot, xref, contact and feet are needed with STEP_MPC only; the last eight are
        optional outputs."""
        self.bind_step(root_states, dof_states, geom, vel_body_des, yaw_rate_des, gait, plan_state, swing_mem, x0,
                       u0, tau, tick=tick, height_des=height_des, robot=robot, xref=xref, contact=contact,
                       feet=feet, status=status, iters=iters, thighs=thighs, pos_feet=pos_feet,
                       foot_pos_base=foot_pos_base, foot_vel_base=foot_vel_base, jac=jac, swing_state=swing_state,
                       pos_target=pos_target, vel_target=vel_target)(
            flags, iter_counter, iterations_between_mpc,
            stream if stream is not None else torch.cuda.current_stream(self.device))

    def bind_step(self, root_states, dof_states, geom, vel_body_des, yaw_rate_des, gait, plan_state, swing_mem, x0,
                  u0, tau, tick=None, height_des=None, robot=None, xref=None, contact=None, feet=None, status=None,
                  iters=None, thighs=None, pos_feet=None, foot_pos_base=None, foot_vel_base=None, jac=None,
                  swing_state=None, pos_target=None, vel_target=None):
        """step() with its device pointers resolved once: returns ``launch(flags, iter_counter,
        iterations_between_mpc, stream)`` (see bind_solve)."""
        lib, ctx = self.lib, self._ctx
        B = int(tau.shape[0])
        keep = (root_states, dof_states, geom, vel_body_des, yaw_rate_des, gait, height_des, robot, plan_state,
                swing_mem, x0, xref, contact, feet, u0, tau, status, iters, thighs, pos_feet, foot_pos_base,
                foot_vel_base, jac, swing_state, pos_target, vel_target)
        tk = _ptr(tick)
        tail = tuple(_ptr(t) for t in keep)
        fn = lib.mpcqp_step

        def launch(flags, iter_counter, iterations_between_mpc, stream):
            code = fn(ctx, B, flags, iter_counter, tk, iterations_between_mpc, *tail, stream.cuda_stream)
            if code:
                _lib.check(ctx, code, "mpcqp_step")
        launch.buffers = keep + (tick,)
        return launch

    def set_estimator(self, dt=0.001, gravity=9.81, sigma_p=0.001, sigma_v=0.0098, sigma_f=0.002, r_p=0.001,
                      r_v=0.1, r_z=0.001, suspicion=100.0, p0=100.0, contact_height=0.0):
        """Estimator constants (include/mpcqp.h mpcqp_set_estimator; doc/state_estimation_kf.md):
        time step and gravity, the process rates of base position, base velocity and feet, the
        measurement variances of the leg position, leg velocity and contact-height rows, the
        suspicion factor of an untrusted foot, the initial variance and the contact height.
        Like set_swing, every call sets all of them (an omitted one returns to its default);
        an invalid value raises and keeps the previous constants."""
        code = self.lib.mpcqp_set_estimator(self._ctx, float(dt), float(gravity), float(sigma_p), float(sigma_v),
                                            float(sigma_f), float(r_p), float(r_v), float(r_z), float(suspicion),
                                            float(p0), float(contact_height))
        _lib.check(self._ctx, code, "mpcqp_set_estimator")
        self.estimator_constants = dict(dt=dt, gravity=gravity, sigma_p=sigma_p, sigma_v=sigma_v, sigma_f=sigma_f,
                                        r_p=r_p, r_v=r_v, r_z=r_z, suspicion=suspicion, p0=p0,
                                        contact_height=contact_height)

    def estimate(self, est_state, quat, gyro, accel, trust, geom, q=None, qdot=None, dof_states=None,
                 root_states=None, feet_world=None, status=None, stream=None):
        """One tick of every robot's base-state Kalman filter (include/mpcqp.h mpcqp_estimate):
        IMU and leg kinematics in, base position / velocity and the feet in the world frame
        out, in one launch on the current stream.

        Every argument is a preallocated contiguous device tensor: est_state [B,EST_STRIDE]
        and geom [B,KIN_STRIDE] float64, status [B] int32, the rest float32.  Inputs: quat
        [B,4] (w, x, y, z), gyro / accel [B,3] (body frame), trust [B,4], q / qdot [B,12] or
        ``dof_states`` [B,12,2] in their place.  Outputs, each optional: root_states [B,13]
        (Isaac Gym layout, what the ``*_root_states`` calls read), feet_world [B,4,3],
        status [B]."""
        s = self._stream_ptr(stream)
        if (dof_states is None) == (q is None):
            raise ValueError("estimate: give q and qdot, or dof_states")
        B = int(est_state.shape[0])
        flags, jq, jqd = (_lib.EST_DOF_STATES, dof_states, None) if dof_states is not None else (0, q, qdot)
        code = self.lib.mpcqp_estimate(self._ctx, B, flags, _ptr(quat), _ptr(gyro), _ptr(accel), _ptr(jq), _ptr(jqd),
                                       _ptr(trust), _ptr(geom), _ptr(est_state), _ptr(root_states),
                                       _ptr(feet_world), _ptr(status), s)
        _lib.check(self._ctx, code, "mpcqp_estimate")

    def set_attitude(self, dt=0.001, gravity=9.81, kappa_ref=0.1, bias_gain=0.0, trust_window=0.2,
                     touch_threshold=0.0):
        """Constants of ``attitude`` (include/mpcqp.h mpcqp_set_attitude; doc/state_estimation_kf.md
        section 2): time step and gravity, the correction gain kappa_ref (1/s) that pulls pitch
        and roll towards the accelerometer, the gain of the gyro-bias estimate (0: none), the
        trust window as a fraction of the stance and the touch threshold.  Like set_estimator,
        every call sets all of them; an invalid value raises and keeps the previous constants."""
        code = self.lib.mpcqp_set_attitude(self._ctx, float(dt), float(gravity), float(kappa_ref), float(bias_gain),
                                           float(trust_window), float(touch_threshold))
        _lib.check(self._ctx, code, "mpcqp_set_attitude")
        self.attitude_constants = dict(dt=dt, gravity=gravity, kappa_ref=kappa_ref, bias_gain=bias_gain,
                                       trust_window=trust_window, touch_threshold=touch_threshold)

    def attitude(self, att_state, gyro, accel, tick=None, iterations_between_mpc=0, gait=None, touch=None,
                 quat=None, gyro_out=None, trust=None, status=None, stream=None):
        """One tick of every robot's orientation filter, and the contact trust of its feet
        (include/mpcqp.h mpcqp_attitude): gyro and accelerometer in, the ``quat`` and ``trust``
        of ``estimate`` out, in one launch on the current stream.

        Every argument is a preallocated contiguous device tensor: att_state [B,ATT_STRIDE]
        float64, tick [B] / gait [B,9] / status [B] int32, the rest float32.  Inputs: gyro /
        accel [B,3] (body frame); for the trust, tick and gait with ``iterations_between_mpc``
        (as for ``leg_torques``) and / or touch [B,4].  Outputs, each optional: quat [B,4]
        (w, x, y, z), gyro_out [B,3] (gyro less the estimated bias), trust [B,4], status [B]."""
        s = self._stream_ptr(stream)
        B = int(att_state.shape[0])
        code = self.lib.mpcqp_attitude(self._ctx, B, 0, _ptr(gyro), _ptr(accel), _ptr(tick),
                                       int(iterations_between_mpc), _ptr(gait), _ptr(touch), _ptr(att_state),
                                       _ptr(quat), _ptr(gyro_out), _ptr(trust), _ptr(status), s)
        _lib.check(self._ctx, code, "mpcqp_attitude")

    def set_terrain(self, contact_threshold=0.5, flat_tol=1e-3, cos_max_tilt=0.5, blend=1.0):
        """Constants of ``terrain`` (include/mpcqp.h mpcqp_set_terrain): the contact threshold, the
        tolerance below which the latched feet count as collinear ((l1 - l0) <= flat_tol l2, the
        fit is held), the cosine of the steepest plane accepted and the weight of a new fit in
        the normal (1: no filter, as the reference).  Like set_attitude, every call sets all of
        them; an invalid value raises and keeps the previous constants."""
        code = self.lib.mpcqp_set_terrain(self._ctx, float(contact_threshold), float(flat_tol), float(cos_max_tilt),
                                          float(blend))
        _lib.check(self._ctx, code, "mpcqp_set_terrain")
        self.terrain_constants = dict(contact_threshold=contact_threshold, flat_tol=flat_tol,
                                      cos_max_tilt=cos_max_tilt, blend=blend)

    def set_ground(self, plane):
        """The swing leg's ground (include/mpcqp.h mpcqp_set_ground): ``plane`` [capacity,4]
        float32 on the device, (n, d) per robot as ``terrain`` writes it, read by every later
        ``leg_torques`` and ``step`` launch; robot b < capacity places its foothold and its swing
        apex on it.  None disables.  The engine keeps the tensor alive."""
        if plane is None:
            code = self.lib.mpcqp_set_ground(self._ctx, None, 0)
        else:
            if not (plane.dtype == torch.float32 and plane.is_contiguous() and plane.dim() == 2
                    and plane.shape[1] == 4 and plane.device == self.device):
                raise ValueError("set_ground: plane must be a contiguous float32 [capacity,4] tensor on the engine's device")
            code = self.lib.mpcqp_set_ground(self._ctx, _ptr(plane), int(plane.shape[0]))
        _lib.check(self._ctx, code, "mpcqp_set_ground")
        self._ground = plane   # the context holds its pointer: keep it alive

    def terrain(self, terrain_state, pos_feet, contact=None, swing_state=None, quat=None, root_states=None,
                robot=None, normal=None, plane=None, normal_base=None, status=None, stream=None, ground=False):
        """One tick of every robot's terrain plane (include/mpcqp.h mpcqp_terrain): the feet in the
        world frame and their contact state in, the ground plane fitted to the feet last in
        contact out, in one launch on the current stream.

        Every argument is a preallocated contiguous device tensor: terrain_state
        [B,TERRAIN_STRIDE] float64, status [B] int32, the rest float32.  Inputs: pos_feet
        [B,4,3]; contact [B,4] (in contact above the threshold) or ``swing_state`` [B,4] in its
        place (in contact where not > 0); for normal_base, quat [B,4] (w, x, y, z) or
        ``root_states`` [B,13].  ``robot`` [B,16]: its words 9..11, the cone rows' surface
        normal, are overwritten.  Outputs, each optional: normal [B,3], plane [B,4] (n, d),
        normal_base [B,3], status [B].  ``ground`` (MPCQP_TERRAIN_GROUND): plane is written as
        the swing leg's ground, (n, d - n_z touchdown_z), so that a foothold of ``set_ground``
        lies on the fitted plane.  A tensor of another size, dtype or device, or one
        that is not contiguous, raises ValueError: the kernel reads and writes B rows of each."""
        s = self._stream_ptr(stream)
        if (contact is None) == (swing_state is None):
            raise ValueError("terrain: give contact or swing_state")
        if quat is not None and root_states is not None:
            raise ValueError("terrain: give quat or root_states, not both")
        if terrain_state.dim() != 2 or terrain_state.shape[1] != _lib.TERRAIN_STRIDE:
            raise ValueError(f"terrain: terrain_state must be [B,{_lib.TERRAIN_STRIDE}]")
        B = int(terrain_state.shape[0])
        f32, i32 = torch.float32, torch.int32
        for name, t, shape, dtype in (
                ("terrain_state", terrain_state, (B, _lib.TERRAIN_STRIDE), torch.float64),
                ("pos_feet", pos_feet, (B, 4, 3), f32), ("contact", contact, (B, 4), f32),
                ("swing_state", swing_state, (B, 4), f32), ("quat", quat, (B, 4), f32),
                ("root_states", root_states, (B, 13), f32), ("robot", robot, (B, ROBOT_STRIDE), f32),
                ("normal", normal, (B, 3), f32), ("plane", plane, (B, 4), f32),
                ("normal_base", normal_base, (B, 3), f32), ("status", status, (B,), i32)):
            if t is None:
                if name == "pos_feet":
                    raise ValueError("terrain: pos_feet is required")
                continue
            if not (t.dtype == dtype and t.is_contiguous() and t.device == self.device
                    and t.numel() == int(np.prod(shape))):
                raise ValueError(f"terrain: {name} must be a contiguous {dtype} tensor of shape {list(shape)} on "
                                 f"{self.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        flags = _lib.TERRAIN_GROUND if ground else 0
        if swing_state is not None:
            flags, contact = flags | _lib.TERRAIN_SWING_STATE, swing_state
        if root_states is not None:
            flags, quat = flags | _lib.TERRAIN_ROOT_STATES, root_states
        code = self.lib.mpcqp_terrain(self._ctx, B, flags, _ptr(pos_feet), _ptr(contact), _ptr(quat),
                                      _ptr(terrain_state), _ptr(robot), _ptr(normal), _ptr(plane),
                                      _ptr(normal_base), _ptr(status), s)
        _lib.check(self._ctx, code, "mpcqp_terrain")

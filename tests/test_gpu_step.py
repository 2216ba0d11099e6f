"""GPU: mpcqp_step / BatchedController.step_fused -- the control tick in one C call -- against
the three-launch path of the same build (BatchedController.step: mpcqp_kinematics, mpcqp_plan,
on MPC ticks mpcqp_solve, mpcqp_leg_torques), which is itself pinned to kin.npz, swing.npz,
planner.npz, kin_ref, swing_ref and the QP oracle.

The requirement is bitwise equality, not a tolerance: both paths call the same header
functions (kin_leg, plan_robot / plan_rows, swing_leg_control) on the same float32 inputs with
FP contraction off, the fused kernel rounds each kinematic value to float32 exactly where
mpcqp_kinematics_kernel's store does, and both enqueue the same solve.  NaN compares equal to
NaN: every comparison is on the bit patterns.

The one check that does not go through the three-launch path is the anchor at the end: tau on
ticks between two solves against swing_ref fed kin_ref's outputs rounded to float32, under the
device bound of tests/test_gpu_swing.py (4.61e-7 norm-wise per robot).  Measured on the MI355X:
1.72e-7 at worst over 65 robots x 24 ticks (2784 swing leg-ticks); every other comparison of
this file is exact.

Horizon 10, iterations_between_mpc = 2, 44 ticks: 22 MPC ticks and more than two whole
TROTTING10 cycles (20 ticks each), so every leg meets its first swing tick, mid-swing ticks,
its finishing tick and stance.  Robots cycle through every Gait member (STANDING never
swings), A1 and Aliengo leg geometry mixed as in tests/golden/kin.npz, whose rows the inputs
start from and drift away from smoothly with the tick.
"""
import ctypes
import functools

import numpy as np
import pytest

# torch first: it brings its own HIP runtime, which must be loaded before libmpcqp.so
torch = pytest.importorskip("torch")

import kin_ref  # noqa: E402
import swing_ref  # noqa: E402
from helpers import DEV, _dev  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
N, IBM, T = 10, 2, 44
BATCHES = (1, 3, 64, 65, 130)    # alone, a partial workgroup, one exactly, one robot past it, three with a tail

STATE = ("tau", "u0", "x0", "plan_state", "swing_mem", "status", "iterations")
SWING_OUT = ("swing_state", "pos_target", "vel_target")
KIN_OUT = ("thighs", "pos_feet", "foot_pos_base", "foot_vel_base", "jac")
MPC_OUT = ("xref", "contact", "feet")
OPTIONAL = SWING_OUT + KIN_OUT


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def snapshot(ctl, names):
    return {k: getattr(ctl, k).cpu().numpy().copy() for k in names}


def gait_names(B):
    from mpcqp.params import GAIT_MEMBERS
    names = list(GAIT_MEMBERS)                      # every Gait member, STANDING first
    return [names[b % len(names)] for b in range(B)]


@functools.lru_cache(maxsize=None)
def sequence(B, bad=None):
    """Seeded inputs for T ticks of B robots: root states [T,B,13], dof states [T,B,12,2]
    (float32), the commands [B,3] / [B] (float64) and the geometry [B,5].  ``bad``: that robot's
    root state carries a NaN from tick 5 on."""
    fx = kin_ref.load_fixture()
    rows = np.arange(B) % len(fx["quat"])
    rng = np.random.default_rng(20)
    ph = rng.uniform(0, 2 * np.pi, (130, 20))[:B]
    dirs = rng.standard_normal((130, 4))[:B]
    cmd = rng.uniform([-0.4, -0.3, 0.0, -0.6], [1.2, 0.3, 0.0, 0.6], (130, 4))[:B]
    t = np.arange(T)[:, None]
    quat = fx["quat"][rows][None] + 0.02 * np.sin(0.21 * t + ph[:, 0])[..., None] * dirs[None]
    quat = quat / np.linalg.norm(quat, axis=-1, keepdims=True)
    vel = fx["vel"][rows][None] + 0.05 * np.sin(0.17 * t + ph[:, 1])[..., None]
    pos = fx["pos"][rows][None] + 0.001 * t[..., None] * fx["vel"][rows][None]
    omega = fx["omega"][rows][None] + 0.05 * np.cos(0.13 * t + ph[:, 2])[..., None]
    q = fx["q"][rows][None] + 0.06 * np.sin(0.3 * t[..., None] + ph[None, :, 3:15])
    qdot = fx["qdot"][rows][None] + 0.3 * np.cos(0.3 * t[..., None] + ph[None, :, 3:15])
    f4 = np.float32
    rs = kin_ref.root_states(quat.astype(f4), pos.astype(f4), vel.astype(f4), omega.astype(f4))
    ds = kin_ref.dof_states(q, qdot)
    if bad is not None:
        rs[5:, bad, 1] = np.nan
    return dict(rs=rs, ds=ds, vb=np.ascontiguousarray(cmd[:, :3]), yr=np.ascontiguousarray(cmd[:, 3]),
                geom=fx["geom"][rows])


def controller(B, **kw):
    from mpcqp.controller import BatchedController
    return BatchedController(B, horizon=N, robot="a1", gait=gait_names(B), iterations_between_mpc=IBM,
                             geometry=sequence(B)["geom"], **kw)


def names_at(it, outputs=True):
    mpc = it % IBM == 0
    n = STATE + (OPTIONAL if outputs else ())
    return n + (MPC_OUT if mpc else (("feet",) if outputs else ()))


@functools.lru_cache(maxsize=None)
def reference(B, bad=None):
    """The three-launch path, computed once per batch size: after every tick, every buffer
    ``step`` leaves."""
    seq = sequence(B, bad)
    ctl = controller(B)
    vb, yr = _dev(seq["vb"]), _dev(seq["yr"])
    out = []
    for it in range(T):
        ctl.step(it, vb, yr, _dev(seq["rs"][it]), _dev(seq["ds"][it]))
        torch.cuda.synchronize()
        out.append(snapshot(ctl, STATE + OPTIONAL + MPC_OUT))
    return out


def assert_same(got, want, names, tag, robots=None):
    for k in names:
        a, b = got[k], want[k]
        if robots is not None:
            a, b = a[robots], b[robots]
        assert same(a, b), (tag, k, int((_bits(a) != _bits(b)).sum()), "entries differ")


@pytest.mark.parametrize("B", BATCHES)
def test_control_two_step_runs_agree(B):
    """Two controllers with identical arguments, both driven by ``step``: bitwise the same at
    every tick.  A mismatch further down is then the fused path's, not the solve's."""
    seq, ref = sequence(B), reference(B)
    ctl = controller(B)
    vb, yr = _dev(seq["vb"]), _dev(seq["yr"])
    for it in range(T):
        ctl.step(it, vb, yr, _dev(seq["rs"][it]), _dev(seq["ds"][it]))
        torch.cuda.synchronize()
        assert_same(snapshot(ctl, STATE + OPTIONAL + MPC_OUT), ref[it], STATE + OPTIONAL + MPC_OUT, ("step", B, it))


@pytest.mark.parametrize("B", BATCHES)
def test_sequence_is_bitwise_the_three_launch_path(B):
    seq, ref = sequence(B), reference(B)
    ctl = controller(B)
    vb, yr = _dev(seq["vb"]), _dev(seq["yr"])
    swung, umax, tmax = np.zeros((B, 4), bool), np.zeros(B), np.zeros(B)
    for it in range(T):
        tau = ctl.step_fused(it, vb, yr, _dev(seq["rs"][it]), _dev(seq["ds"][it]), outputs=True)
        torch.cuda.synchronize()
        assert tau is ctl.tau
        names = names_at(it)
        assert_same(snapshot(ctl, names), ref[it], names, ("fused", B, it))
        swung |= ref[it]["swing_state"] > 0
        umax = np.maximum(umax, np.abs(ref[it]["u0"]).max(axis=1))
        tmax = np.maximum(tmax, np.abs(ref[it]["tau"]).max(axis=1))
    # not a comparison of zeros: the robots carry weight, command torque and -- but for the
    # STANDING ones -- have swung every leg
    standing = np.array([g == "STANDING" for g in gait_names(B)])
    assert (umax > 1.0).all() and (tmax > 1e-2).all()
    assert swung[~standing].all() and not swung[standing].any()


def pad_buffers(ctl, names, fill_all=()):
    """Replaces the controller's buffers by the first B rows of buffers three rows longer,
    the rest SENTINEL (``fill_all``: the first B rows too).  Returns the long buffers."""
    full = {}
    for k in names:
        old = getattr(ctl, k)
        f = torch.full((ctl.B + 3,) + tuple(old.shape[1:]), SENTINEL, dtype=old.dtype, device=old.device)
        if k not in fill_all:
            f[:ctl.B] = old
        full[k] = f
        setattr(ctl, k, f[:ctl.B])
    return full


@pytest.mark.parametrize("B", (3, 65))
def test_null_outputs_and_padding(B):
    """outputs=False: tau and all state are the same bits, every optional buffer and the three
    rows behind every written buffer keep their sentinel (SENTINEL / pad as in
    tests/test_gpu_kin.py)."""
    seq, ref = sequence(B), reference(B)
    ctl = controller(B)
    full = pad_buffers(ctl, STATE + MPC_OUT + OPTIONAL, fill_all=OPTIONAL)
    vb, yr = _dev(seq["vb"]), _dev(seq["yr"])
    for it in range(T):
        ctl.step_fused(it, vb, yr, _dev(seq["rs"][it]), _dev(seq["ds"][it]))
        torch.cuda.synchronize()
        names = names_at(it, outputs=False)
        assert_same(snapshot(ctl, names), ref[it], names, ("no outputs", B, it))
    for k in STATE + MPC_OUT:
        assert (full[k][B:] == SENTINEL).all(), (k, "padding written")
        assert not (full[k][:B] == SENTINEL).all(), (k, "never written")
    for k in OPTIONAL:
        assert (full[k] == SENTINEL).all(), (k, "an optional output was written with outputs=False")
    # and with outputs=True the padding of the optional buffers stays too
    ctl.step_fused(T, vb, yr, _dev(seq["rs"][0]), _dev(seq["ds"][0]), outputs=True)
    torch.cuda.synchronize()
    for k in OPTIONAL:
        assert (full[k][B:] == SENTINEL).all() and not (full[k][:B] == SENTINEL).all(), k


def test_scalar_counter_equals_a_filled_tick_array():
    B = 65
    seq = sequence(B)
    a, b = controller(B), controller(B)
    vb, yr = _dev(seq["vb"]), _dev(seq["yr"])
    for it in range(12):
        rs, ds = _dev(seq["rs"][it]), _dev(seq["ds"][it])
        a.step_fused(it, vb, yr, rs, ds, outputs=True)
        b.tick_count.fill_(it)
        # mpc_tick left out (ticks 4 and 5): the first robot's counter is read back to decide
        b.step_fused(None, vb, yr, rs, ds, outputs=True, mpc_tick=None if it in (4, 5) else it % IBM == 0)
        torch.cuda.synchronize()
        names = names_at(it)
        assert_same(snapshot(b, names), snapshot(a, names), names, ("tick array", it))
    assert (a.tick_count == 0).all()       # the scalar form leaves the counters alone


def test_per_robot_counters():
    """Each robot on its own counter (iter_counter=None): equal to kinematics + plan (+ solve)
    + leg_torques(iter_counter=None) by hand on the same counters, the plan on an MPC tick given
    iteration = floor(tick / ibm) mod period per robot -- so ``contact`` is each robot's own
    window of its gait."""
    from mpcqp._lib import PLAN_REFERENCE
    B = 65
    seq = sequence(B)
    a, h = controller(B), controller(B)
    vb, yr = _dev(seq["vb"]), _dev(seq["yr"])
    offs = (np.arange(B) * 3) % 41 - 4           # negative counters too
    period = h.gait[:, 0].cpu().numpy()
    windows = set()
    for it in range(12):
        rs, ds = _dev(seq["rs"][it]), _dev(seq["ds"][it])
        mpc = it % IBM == 0
        ticks = (it + offs).astype(np.int32)
        a.tick_count.copy_(_dev(ticks))
        a.step_fused(None, vb, yr, rs, ds, outputs=True, mpc_tick=mpc)
        h.kinematics(rs, ds)
        h.iteration.copy_(_dev((np.floor_divide(ticks, IBM) % period).astype(np.int32)))
        h.engine.plan(PLAN_REFERENCE if mpc else 0, h.plan_state, h.x0, vb, yr, root_states=rs, gait=h.gait,
                      iteration=h.iteration, height_des=h.height, xref=h.xref, contact=h.contact)
        if mpc:
            h.engine.solve_raw(B, h.x0, h.xref, h.contact, h.feet, h.robot, h.u0, status=h.status,
                               iters=h.iterations)
        h.tick_count.copy_(_dev(ticks))
        h.leg_torques(None, vb, yr, h.thighs, h.pos_feet, h.foot_pos_base, h.foot_vel_base, h.jac, root_states=rs)
        torch.cuda.synchronize()
        names = STATE + OPTIONAL + (MPC_OUT if mpc else ("feet",))
        assert_same(snapshot(a, names), snapshot(h, names), names, ("per-robot counters", it))
        if mpc:
            trot = a.contact.cpu().numpy()[2::7]            # the TROTTING10 robots
            windows |= {tuple(r.reshape(-1)) for r in trot}
    assert len(windows) > 3                                  # the robots' gait windows differ


def test_a_bad_robot_stays_alone():
    """One robot of 65 with a NaN in its root state from tick 5 on: its own outputs are
    ``step``'s (NaN bits included), every other robot's bits are those of the run without it."""
    B, bad = 65, 63
    seq, ref, clean = sequence(B, bad), reference(B, bad), reference(B)
    ctl = controller(B)
    vb, yr = _dev(seq["vb"]), _dev(seq["yr"])
    others = np.arange(B) != bad
    for it in range(T):
        ctl.step_fused(it, vb, yr, _dev(seq["rs"][it]), _dev(seq["ds"][it]), outputs=True)
        torch.cuda.synchronize()
        names = names_at(it)
        got = snapshot(ctl, names)
        assert_same(got, ref[it], names, ("bad robot", it))
        assert_same(got, clean[it], names, ("beside the bad robot", it), robots=others)
    assert np.isnan(got["x0"][bad]).any() and np.isfinite(got["tau"][others]).all()


def test_anchor_swing_ref_on_kin_ref():
    """Ticks between two solves with a fixed u0: tau against swing_ref fed kin_ref's outputs
    rounded to float32 (the construction at the end of tests/test_gpu_kin.py), norm-wise per
    robot under the device bound of tests/test_gpu_swing.py.  Nothing here goes through the
    three-launch path."""
    from test_gpu_swing import BOUND
    from mpcqp.params import SWING_PRESETS, gait_record
    B, ticks = 65, 24
    seq = sequence(B)
    ctl = controller(B)
    u0 = np.random.default_rng(3).uniform(-40, 120, (B, 12)).astype(np.float32)
    ctl.u0.copy_(_dev(u0))
    sw = SWING_PRESETS["a1"]
    ref = swing_ref.SwingRef(B, kp=sw["kp"], kd=sw["kd"], swing_height=sw["swing_height"])
    gait = np.stack([gait_record(g) for g in gait_names(B)])
    vb, yr = _dev(seq["vb"]), _dev(seq["yr"])
    worst, swings = 0.0, 0
    for it in range(ticks):
        rs, ds = seq["rs"][it], seq["ds"][it]
        ctl.step_fused(it, vb, yr, _dev(rs), _dev(ds), mpc_tick=False)
        torch.cuda.synchronize()
        tau = ctl.tau.cpu().numpy()
        quat = np.concatenate([rs[:, 6:7], rs[:, 3:6]], 1)
        kin = kin_ref.kinematics(seq["geom"], quat, rs[:, 0:3], rs[:, 7:10], rs[:, 10:13], ds[..., 0], ds[..., 1])
        k32 = {k: v.astype(np.float32) for k, v in kin.items()}
        want = ref.step(np.full(B, it), IBM, gait, rs[:, 0:3], rs[:, 7:10], swing_ref.quat2matrix_f32(quat),
                        seq["vb"], seq["yr"], k32["thighs"], k32["pos_feet"], k32["foot_pos_base"],
                        k32["foot_vel_base"], k32["jac"], u0)
        swings += int(want["swing"].sum())
        for b in range(B):
            e = swing_ref.norm_err(tau[b], want["tau"][b])
            worst = max(worst, e)
            assert e <= BOUND, (it, b, e)
    print(f"\nanchor: worst norm-wise tau error {worst:.2e} (bound {BOUND:.2e}), {swings} swing leg-ticks")
    assert swings > 100 and torch.equal(ctl.u0.cpu(), torch.as_tensor(u0))     # u0 is only read


def test_misuse_through_the_raw_binding():
    """Every refusal of mpcqp_step: MPCQP_ERR_ARG with a message, nothing written; batch == 0 is
    MPCQP_OK; the context works afterwards."""
    from mpcqp import _lib
    B = 4
    seq = sequence(B)
    ctl = controller(B)
    lib, ctx = ctl.engine.lib, ctl.engine._ctx
    rs, ds = _dev(seq["rs"][0]), _dev(seq["ds"][0])
    vb, yr = _dev(seq["vb"]), _dev(seq["yr"])
    ctl.tau.fill_(SENTINEL)
    ctl.plan_state.fill_(SENTINEL)
    order = ("root_states", "dof_states", "geom", "vb", "yr", "gait", "height", "robot", "plan_state", "swing_mem",
             "x0", "xref", "contact", "feet", "u0", "tau", "status", "iters")
    bufs = dict(root_states=rs, dof_states=ds, geom=ctl.geometry, vb=vb, yr=yr, gait=ctl.gait, height=ctl.height,
                robot=ctl.robot, plan_state=ctl.plan_state, swing_mem=ctl.swing_mem, x0=ctl.x0, xref=ctl.xref,
                contact=ctl.contact, feet=ctl.feet, u0=ctl.u0, tau=ctl.tau, status=ctl.status,
                iters=ctl.iterations)

    def call(batch=B, flags=0, ibm=IBM, **override):
        p = {k: v.data_ptr() for k, v in bufs.items()}
        p.update(override)
        return lib.mpcqp_step(ctx, batch, flags, 3, None, ibm, *[ctypes.c_void_p(p[k]) for k in order],
                              *([None] * 8), None)

    def refused(code, what):
        assert code == _lib.ERR_ARG, what
        assert lib.mpcqp_last_error(ctx), what

    refused(call(flags=2), "unknown flags")
    refused(call(flags=_lib.STEP_MPC | 4), "unknown flags beside a known one")
    refused(call(batch=-1), "batch < 0")
    refused(call(ibm=0), "iterations_between_mpc < 1")
    for k in ("root_states", "dof_states", "geom", "vb", "yr", "gait", "plan_state", "swing_mem", "x0", "u0", "tau"):
        for flags in (0, _lib.STEP_MPC):
            refused(call(flags=flags, **{k: 0}), (k, flags))
    for k in ("height", "robot", "xref", "contact", "feet"):
        refused(call(flags=_lib.STEP_MPC, **{k: 0}), k)
    for flags in (0, _lib.STEP_MPC):
        refused(call(flags=flags, swing_mem=ctl.swing_mem.data_ptr() + 8), "swing_mem off 16 bytes")
    assert lib.mpcqp_step(ctx, 0, 0, 0, None, IBM, *([None] * 27)) == _lib.MPCQP_OK
    torch.cuda.synchronize()
    assert (ctl.tau == SENTINEL).all() and (ctl.plan_state == SENTINEL).all()
    assert not ctl.swing_mem.any() and not ctl.x0.any()
    # the context still works: the MPC-only pointers, status and iters may be NULL with flags == 0
    ctl.plan_state.zero_()
    none = dict(height=0, robot=0, xref=0, contact=0, feet=0, status=0, iters=0)
    assert call(**none) == _lib.MPCQP_OK
    torch.cuda.synchronize()
    assert torch.isfinite(ctl.tau).all() and (ctl.tau != SENTINEL).all() and ctl.plan_state[:, 5].eq(1.0).all()
    assert call(flags=_lib.STEP_MPC) == _lib.MPCQP_OK
    torch.cuda.synchronize()
    assert torch.isfinite(ctl.u0).all() and torch.isfinite(ctl.tau).all() and float(ctl.u0.abs().max()) > 1.0


def test_commands_and_engine_step():
    """Commands: device float64 tensors go through uncopied, lists are converted as ``step``
    converts them, set_command stores them once; LinearMpc.step is the same call unbound."""
    B = 3
    seq = sequence(B)
    a, b, c, d = (controller(B) for _ in range(4))
    rs, ds = _dev(seq["rs"][1]), _dev(seq["ds"][1])
    cmd, rate = [0.5, 0.1, 0.0], 0.2
    a.step(1, cmd, rate, rs, ds)
    b.step_fused(1, cmd, rate, rs, ds, outputs=True)
    vb, yr = c.set_command(cmd, rate)
    assert vb.dtype == torch.float64 and tuple(vb.shape) == (B, 3) and tuple(yr.shape) == (B,)
    v2, y2 = c.set_command(vb, yr)
    assert v2 is vb and y2 is yr                                 # device float64 tensors: no copy
    c.step_fused(1, None, None, rs, ds, outputs=True)
    with pytest.raises(ValueError, match="set_command"):
        d.step_fused(1, None, None, rs, ds)
    d.engine.step(0, 1, IBM, rs, ds, d.geometry, vb, yr, d.gait, d.plan_state, d.swing_mem, d.x0, d.u0, d.tau,
                  **{k: getattr(d, k) for k in OPTIONAL})
    torch.cuda.synchronize()
    names = STATE + OPTIONAL
    for other in (b, c, d):
        assert_same(snapshot(other, names), snapshot(a, names), names, "commands")

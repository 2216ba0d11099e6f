"""GPU: mpcqp_plant / BatchedPlant -- the rigid-body plant on the device -- against the float64
restatement tests/plant_ref.py, and the control loop closed on the device: step_fused -> plant ->
step_fused with nothing on the host, from the true state and from the estimated one.

Bounds.  The record is float64 on both sides; the device's sin, cos, atan2 and sqrt chain differ from
libm in the last places.  DEVICE_BOUND is ten times the worst norm-wise error per robot measured on
the first green run of the single ticks, capped at 1e-9 (the figures stand beside it below).  The
float32 outputs are compared with the restatement's float32 roundings under one float32 ulp of
the row's largest value, 2^-23: values that close round to the same or to adjacent numbers.
Contact flags, flag word and call count are compared exactly; a state that the restatement alone
places within 1e-9 of a switching threshold (n . f = 0, the cone edge, the plane) is left out, at
most 2 % of them.

Measured on the MI355X: single ticks 7.29e-16 at worst, every float32 output equal to the
restatement's rounding; substeps = 4 against four ticks at dt / 4 bitwise equal; the 200-tick
replay 8.4e-17 per tick at worst with all eight robots compared to the end; the closed loop at
(0, 0.5, 1.0) m/s height error 0.01086 / 0.01094 / 0.01109 m, roll / pitch 6.2e-8 / 0.0336 /
0.0854 rad, speed 1e-10 / 0.5210 / 1.0442 m/s (the CPU loop's to five digits: the device solve
and the oracle's agree far below a contact event's reach); the sensing chain at 0.5 m/s height
error 0.0235 m, roll / pitch 0.0344 rad, speed 0.550 m/s over the last 300 ticks, the estimate
within 0.0055 m and 0.0070 m/s of plant.root.

The closed loop is held to the CPU oracle loop's recorded figures (plant_ref.CLOSED_LOOP, asserted
by tests/test_plant.py): the two loops drift apart sample by sample at contact events, the
gait-averaged quantities do not.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

# torch first: it brings its own HIP runtime, which must be loaded before libmpcqp.so
torch = pytest.importorskip("torch")

import kin_ref  # noqa: E402
import plant_ref as pr  # noqa: E402
from helpers import DEV, _dev  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
N = 10
# ten times the worst single-tick error of the first green run on the MI355X (1.04e-16 at B = 1,
# 5.40e-16 at B = 16, 7.29e-16 at B = 67), under the cap of 1e-9
DEVICE_BOUND = 7.3e-15
F32_BOUND = 2.0 ** -23
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plant_tau.npz")


def _bits(t):
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def pair(B, **constants):
    """A controller (Aliengo, TROTTING10, N = 10) and a plant on its context."""
    from mpcqp.controller import BatchedController
    from mpcqp.plant import BatchedPlant
    ctl = BatchedController(B, horizon=N, robot="aliengo", gait="TROTTING10")
    plant = BatchedPlant(B, controller=ctl, **dict(dict(foot_mass=0.15, substeps=1, ground_z=-0.0255, contact_tol=1e-4),
                                                   **constants))
    return ctl, plant


@functools.lru_cache(maxsize=None)
def states():
    """The CPU test's seeded single-tick states (tests/test_plant.py, substeps 1) and what the
    restatement makes of them, computed once."""
    par = pr.Params()
    st = pr.make_states(512, seed=6, par=par)
    near = pr.near_threshold(st["rec"], st["tau"], st["robot"], st["geom"], par)
    ref = st["rec"].copy()
    want = pr.plant_step(ref, st["tau"], st["robot"], st["geom"], par)
    return st, near, ref, want


def run_device(plant, rec, tau, robot=None, geom=None):
    """One mpcqp_plant call on the given records; returns the records and outputs as NumPy."""
    plant.state.copy_(_dev(rec))
    if robot is not None:
        plant.robot = _dev(robot, torch.float32)
    if geom is not None:
        plant.geometry = _dev(geom, torch.float64)
    plant._bound.clear()
    plant.step(_dev(tau, torch.float32))
    torch.cuda.synchronize()
    out = {k: getattr(plant, k).cpu().numpy().copy() for k in ("root", "dofs", "gyro", "accel", "touch", "status")}
    return plant.state.cpu().numpy().copy(), out


@pytest.mark.parametrize("B", [1, 16, 67])
def test_single_ticks_match_the_restatement(B):
    """B = 67: four whole wavefronts of 16 robots and a last one of 3 (a partial quad group);
    1 and 16: one quad, one whole wavefront.  Measured on the MI355X: see DEVICE_BOUND."""
    st, near, ref, want = states()
    idx = np.r_[np.arange(B - 1), 511]                     # the two rows that hold every case are in
    _, plant = pair(B)
    got_rec, got = run_device(plant, st["rec"][idx], st["tau"][idx], st["robot"][idx], st["geom"][idx])
    keep = ~near[idx]
    assert near[idx].mean() <= 0.02
    err = pr.record_error(got_rec, ref[idx])[keep]
    print(f"\nB = {B}: record, norm-wise per robot: worst {err.max():.2e} (bound {DEVICE_BOUND:g})")
    assert (got["status"] == 0).all()
    assert np.array_equal(got_rec[keep, pr.CONTACT:pr.WORDS], ref[idx][keep, pr.CONTACT:pr.WORDS])
    assert np.array_equal(got_rec[:, pr.WORDS:], st["rec"][idx][:, pr.WORDS:])          # the padding is kept
    assert err.max() <= DEVICE_BOUND
    for k in ("root", "dofs", "gyro", "accel"):
        e = max(kin_ref.norm_err(got[k][b], want[k][idx][b]) for b in np.flatnonzero(keep))
        print(f"{k}: worst {e:.2e} (bound {F32_BOUND:.2e})")
        assert e <= F32_BOUND, k
    assert np.array_equal(got["touch"][keep], want["touch"][idx][keep])


def test_substeps_4_is_four_ticks_at_a_quarter_of_dt():
    st, near, _, _ = states()
    B = 67
    idx = np.arange(B)
    ctl, plant = pair(B, substeps=4)
    rec4, out4 = run_device(plant, st["rec"][idx], st["tau"][idx], st["robot"][idx], st["geom"][idx])
    plant.set_constants(substeps=1)
    ctl.engine.set_planner(dt_control=0.001 / 4)
    rec1 = st["rec"][idx]
    for _ in range(4):
        rec1, out1 = run_device(plant, rec1, st["tau"][idx])
    # near a threshold by the restatement at this substep length
    par = pr.Params(substeps=4)
    keep = ~pr.near_threshold(st["rec"][idx], st["tau"][idx], st["robot"][idx], st["geom"][idx], par)
    err = pr.record_error(rec4, rec1)[keep]
    print(f"\nsubsteps = 4 against four ticks at dt / 4: worst {err.max():.2e}")
    assert keep.mean() >= 0.98 and err.max() <= DEVICE_BOUND
    assert np.array_equal(rec4[keep, pr.CONTACT:pr.FLAGS], rec1[keep, pr.CONTACT:pr.FLAGS])
    assert np.array_equal(rec4[:, pr.TICK] + 3, rec1[:, pr.TICK])
    assert (out4["status"] == 0).all() and np.array_equal(out4["touch"][keep], out1["touch"][keep])


def test_open_loop_replay_of_200_ticks():
    """Eight robots replay the torques recorded from the CPU oracle loop at 0.5 m/s
    (tests/golden/plant_tau.npz): contact flags equal on every tick, the record within
    DEVICE_BOUND x the tick count."""
    fx = np.load(GOLDEN)
    tau, rec = fx["tau"], fx["rec0"].copy()
    T, B = tau.shape[:2]
    par = pr.Params()
    st = pr.make_states(B, seed=0, par=par)                # Aliengo's records
    _, plant = pair(B)
    plant.state.copy_(_dev(rec))
    tau_dev = _dev(tau)
    alive = np.ones(B, bool)
    worst = 0.0
    for t in range(T):
        alive &= ~pr.near_threshold(rec, tau[t], st["robot"], st["geom"], par)
        pr.plant_step(rec, tau[t], st["robot"], st["geom"], par)
        plant.step(tau_dev[t])
        got = plant.state.cpu().numpy()
        assert np.array_equal(got[alive, pr.CONTACT:pr.WORDS], rec[alive, pr.CONTACT:pr.WORDS]), t
        err = pr.record_error(got, rec)[alive].max()
        worst = max(worst, err / (t + 1))
        assert err <= DEVICE_BOUND * (t + 1), (t, err)
    print(f"\n200-tick replay: worst record error per tick {worst:.2e}; {alive.sum()} of {B} robots compared to the end")
    assert alive.sum() >= B - 1 and (plant.status == 0).all()
    assert np.array_equal(rec, fx["rec_end"])              # the restatement is the one that made the fixture


def _loop(ctl, plant, commands, ticks, root_of=None):
    """ticks iterations of step_fused; plant.step on the device with nothing read back inside
    the loop.  Returns the body words of the record per tick [T,B,13] and whether every status
    (solve, plant) was OK."""
    B = ctl.B
    vb = torch.zeros((B, 3), dtype=torch.float64, device=DEV)
    vb[:, 0] = torch.as_tensor(commands, dtype=torch.float64)
    ctl.set_command(vb, 0.0)
    hist = torch.zeros((ticks, B, 13), dtype=torch.float64, device=DEV)
    bad = torch.zeros((B,), dtype=torch.int32, device=DEV)
    root, dofs = plant.root, plant.dofs
    for it in range(ticks):
        seen = root if root_of is None else root_of(it)
        ctl.step_fused(it, None, None, seen, dofs)
        plant.step(ctl.tau)
        hist[it] = plant.state[:, :13]
        bad |= ctl.status | plant.status
    torch.cuda.synchronize()
    return hist.cpu().numpy(), bad.cpu().numpy()


def _figures(hist, dt=0.001, last=500):
    roll, pitch = zip(*(pr.euler_zyx(h[:, 3:7]) for h in hist))
    tilt = np.maximum(np.abs(roll), np.abs(pitch))
    speed = (hist[-1, :, 0] - hist[-1 - last, :, 0]) / (last * dt)
    return np.abs(hist[:, :, 2] - 0.38).max(0), tilt.max(0), speed, np.abs(hist[:, :, 2] - 0.38), tilt


def test_the_closed_loop_walks_on_the_device():
    """B = 6 at (0, 0, 0.5, 0.5, 1.0, 1.0) m/s, 1000 ticks: every status OK, the CPU loop's hard
    conditions on every tick, each robot's worst height error and roll / pitch within twice the
    CPU oracle loop's recorded values, its mean speed over the last 500 ticks within 0.05 m/s of
    the CPU loop's; the two robots of a pair agree bitwise."""
    commands = np.repeat(pr.COMMANDS, 2)
    ctl, plant = pair(6)
    plant.reset()
    hist, bad = _loop(ctl, plant, commands, 1000)
    height, tilt, speed, herr, tilts = _figures(hist)
    print(f"\nclosed loop on the device at {commands}:\n  height error {height}\n  roll / pitch {tilt}\n  speed {speed}")
    assert np.isfinite(hist).all() and (bad == 0).all()
    assert (herr < 0.05).all() and (tilts < 0.1).all()
    for k in range(3):
        assert np.array_equal(hist[:, 2 * k], hist[:, 2 * k + 1]), f"the pair at {pr.COMMANDS[k]} m/s differs"
    want = {k: np.repeat(v, 2) for k, v in pr.CLOSED_LOOP.items()}
    assert (height <= 2 * want["height"]).all()
    # at command 0 the loop is symmetric and its roll / pitch is rounding noise of the solver, not a
    # gait quantity: 3.3e-8 rad on the CPU oracle loop, 6.2e-8 measured on the MI355X.  That row
    # gets an absolute floor of 1e-6 rad in place of twice a noise figure; the rows that walk keep
    # the factor of two (measured 0.0336 and 0.0854 against limits of 0.0672 and 0.1708)
    assert (tilt <= np.maximum(2 * want["tilt"], 1e-6)).all()
    assert (np.abs(speed - want["speed"]) <= 0.05).all()


def test_the_sensing_chain_closes_the_loop():
    """600 ticks at 0.5 m/s with the controller fed the estimated root:
    plant.gyro / accel / dofs / touch -> update_from_imu -> step_fused -> plant.  The robot starts
    standing on the ground and the estimator settles on it for 50 ticks first (from an all-zero
    record its height is unknown until a foot is trusted).  The robot does not fall; the
    estimate's error against plant.root is printed, nothing is asserted on it."""
    from mpcqp.estimator import BatchedEstimator
    B = 4
    ctl, plant = pair(B)
    par = pr.Params()
    geom = plant.geometry.cpu().numpy()
    root0, _ = pr.stand_pose(B, geom, par)                  # the feet on the ground
    plant.reset(height=float(root0[0, 2]))
    assert plant.contact.all()
    est = BatchedEstimator(B, robot="aliengo", controller=ctl, contact_height=par.ground_z)
    # settle: the plant stands under J^T (-m g / 4 z) while the estimator runs
    _, _, Jb = kin_ref.chain(geom, plant.dofs[:, :, 0].cpu().numpy())
    m = float(plant.robot[0, 0])
    stand = _dev(np.einsum("blcr,c->blr", Jb, -np.array([0, 0, m * par.gravity / 4])).reshape(B, 12), torch.float32)
    for it in range(50):
        plant.step(stand)
        est.update_from_imu(plant.gyro, plant.accel, plant.dofs, tick=it, touch=plant.touch)
    errs = []

    def seen(it):
        r = est.update_from_imu(plant.gyro, plant.accel, plant.dofs, tick=it, touch=plant.touch)
        errs.append((r - plant.root).abs())
        return r
    hist, bad = _loop(ctl, plant, [0.5] * B, 600, root_of=seen)
    height, tilt, speed, herr, tilts = _figures(hist, last=300)
    e = torch.stack(errs).cpu().numpy()
    print(f"\nsensing chain, 600 ticks at 0.5 m/s: height error {height}, roll / pitch {tilt}, speed {speed}\n"
          f"  estimate against plant.root: position {e[:, :, 0:3].max():.4f} m (x {e[:, :, 0].max():.4f}, "
          f"z {e[:, :, 2].max():.4f}), velocity {e[:, :, 7:10].max():.4f} m/s")
    assert np.isfinite(hist).all() and (bad == 0).all() and (est.status == 0).all()
    assert (herr < 0.05).all() and (tilts < 0.1).all()


def test_graph_capture_replays_the_eager_loop_bitwise():
    """step_fused (a tick between two solves) and plant.step captured once and replayed 19 times
    leave bitwise the records of 19 eager iterations.  Single stream; each robot's tick counter
    lives on the device and is advanced inside the captured region."""
    B = 6
    runs = []
    for graphed in (False, True):
        ctl, plant = pair(B)
        plant.reset()
        vb = torch.zeros((B, 3), dtype=torch.float64, device=DEV)
        vb[:, 0] = 0.5
        ctl.set_command(vb, 0.0)
        ctl.step_fused(0, None, None, plant.root, plant.dofs)          # the solve of tick 0
        plant.step(ctl.tau)
        ctl.tick_count.fill_(1)

        def iteration():
            ctl.step_fused(None, None, None, plant.root, plant.dofs, mpc_tick=False)
            plant.step(ctl.tau)
            ctl.tick_count.add_(1)
        if graphed:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                iteration()
            for _ in range(19):
                g.replay()
        else:
            for _ in range(19):
                iteration()
        torch.cuda.synchronize()
        runs.append([_bits(t) for t in (plant.state, plant.root, plant.dofs, plant.touch, ctl.tau, ctl.swing_mem,
                                        ctl.plan_state, ctl.tick_count)])
        assert (plant.status == 0).all() and float(plant.ticks[0]) == 20.0
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_a_nan_torque_refuses_one_robot_alone():
    st, _, _, _ = states()
    B, bad, bad2 = 67, 41, 66
    idx = np.arange(B)
    _, plant = pair(B)
    clean_rec, clean = run_device(plant, st["rec"][idx], st["tau"][idx], st["robot"][idx], st["geom"][idx])
    tau = st["tau"][idx].copy()
    tau[bad, 7] = np.nan
    rec0 = st["rec"][idx].copy()
    rec0[bad2, pr.CONTACT + 1] = np.nan                    # a non-finite contact word: refused like any other
    rec, out = run_device(plant, rec0, tau)
    others = (idx != bad) & (idx != bad2)
    assert out["status"][bad] == 4 and out["status"][bad2] == 4 and (out["status"][others] == 0).all()
    assert np.array_equal(rec[bad2].view(np.uint64), rec0[bad2].view(np.uint64))
    assert np.array_equal(rec[bad].view(np.uint64), st["rec"][bad].view(np.uint64))       # bitwise untouched
    assert np.array_equal(rec[others].view(np.uint64), clean_rec[others].view(np.uint64))
    for k in ("root", "dofs", "gyro", "accel", "touch"):
        assert np.array_equal(out[k][others].view(np.uint32), clean[k][others].view(np.uint32)), k
    assert np.array_equal(out["root"][bad, :3], st["rec"][bad, :3].astype(np.float32))     # from the untouched record
    assert np.array_equal(out["touch"][bad], st["rec"][bad, pr.CONTACT:pr.CONTACT + 4].astype(np.float32))


def test_misuse_through_the_raw_binding():
    """Every refusal of mpcqp_plant, mpcqp_plant_reset and mpcqp_set_plant: MPCQP_ERR_ARG with a
    message and nothing written (a record misaligned by 8 bytes among them); batch == 0 is
    MPCQP_OK; refused constants stay; the context works afterwards."""
    from mpcqp import _lib
    st, _, _, _ = states()
    B = 5
    idx = np.arange(B)
    ctl, plant = pair(B)
    want_rec, want = run_device(plant, st["rec"][idx], st["tau"][idx], st["robot"][idx], st["geom"][idx])
    lib, ctx = plant.lib, plant._ctx
    big = torch.zeros((B * pr.STRIDE + 2,), dtype=torch.float64, device=DEV)
    big[:B * pr.STRIDE] = _dev(st["rec"][idx]).reshape(-1)
    plant.state = big[:B * pr.STRIDE].view(B, pr.STRIDE)
    tau = _dev(st["tau"][idx])
    order = ("tau", "robot", "geom", "plane", "state", "root", "dofs", "gyro", "accel", "touch", "status")
    bufs = dict(tau=tau, robot=plant.robot, geom=plant.geometry, state=plant.state, root=plant.root, dofs=plant.dofs,
                gyro=plant.gyro, accel=plant.accel, touch=plant.touch, status=plant.status)
    for t in (plant.root, plant.dofs, plant.gyro, plant.accel, plant.touch):
        t.fill_(SENTINEL)
    before = plant.state.clone()

    def call(batch=B, flags=0, **override):
        p = {k: v.data_ptr() for k, v in bufs.items()}
        p["plane"] = 0
        p.update(override)
        return lib.mpcqp_plant(ctx, batch, flags, *[ctypes.c_void_p(p[k]) if p[k] else None for k in order], None)

    def refused(code, what):
        assert code == _lib.ERR_ARG and lib.mpcqp_last_error(ctx), what

    refused(call(flags=1), "unknown flags")
    refused(call(batch=-1), "batch < 0")
    for k in ("tau", "robot", "geom", "state", "root", "dofs"):
        refused(call(**{k: 0}), k)
    refused(call(state=plant.state.data_ptr() + 8), "plant_state off 16 bytes")
    refused(call(dofs=plant.dofs.data_ptr() + 4), "dof_states off 8 bytes")
    assert call(batch=0) == _lib.MPCQP_OK
    rs = lambda **o: lib.mpcqp_plant_reset(ctx, o.get("batch", B), *[
        ctypes.c_void_p(o.get(k, v)) if o.get(k, v) else None
        for k, v in (("root", plant.root.data_ptr()), ("dofs", plant.dofs.data_ptr()), ("geom", plant.geometry.data_ptr()),
                     ("plane", 0), ("state", plant.state.data_ptr()))], None)
    refused(rs(batch=-1), "reset: batch < 0")
    for k in ("root", "dofs", "geom", "state"):
        refused(rs(**{k: 0}), f"reset: {k}")
    refused(rs(state=plant.state.data_ptr() + 8), "reset: plant_state off 16 bytes")
    assert rs(batch=0) == _lib.MPCQP_OK
    sp = lambda *a: lib.mpcqp_set_plant(ctx, *a)
    for args in ((0.0, 1, -0.0255, 1e-4), (-1.0, 1, -0.0255, 1e-4), (float("nan"), 1, -0.0255, 1e-4),
                 (float("inf"), 1, -0.0255, 1e-4), (0.15, 0, -0.0255, 1e-4), (0.15, 17, -0.0255, 1e-4),
                 (0.15, 1, float("nan"), 1e-4), (0.15, 1, -0.0255, float("inf"))):
        refused(sp(*args), args)
    torch.cuda.synchronize()
    assert torch.equal(plant.state, before)
    for t in (plant.root, plant.dofs, plant.gyro, plant.accel, plant.touch):
        assert (t == SENTINEL).all()
    # the context still works, with the constants it had; the optional outputs may be NULL
    assert call(gyro=0, accel=0, touch=0, status=0) == _lib.MPCQP_OK
    torch.cuda.synchronize()
    assert np.array_equal(_bits(plant.state), want_rec.view(np.uint64))
    assert np.array_equal(_bits(plant.root), want["root"].view(np.uint32)) and (plant.gyro == SENTINEL).all()


def test_reset_fills_the_records_from_a_pose():
    B = 67
    ctl, plant = pair(B)
    par = pr.Params()
    root, dofs = plant.reset()
    torch.cuda.synchronize()
    geom = plant.geometry.cpu().numpy()
    want = pr.reset(root.cpu().numpy(), dofs.cpu().numpy(), geom, par)
    got = plant.state.cpu().numpy()
    assert np.abs(got - want).max() <= 1e-12 and np.array_equal(got[:, pr.CONTACT:], want[:, pr.CONTACT:])
    assert not got[:, pr.CONTACT:pr.CONTACT + 4].any() and float(root[0, 2]) == np.float32(0.38)
    # on the ground, and on the plant's own plane rather than a fitted one
    h = float(pr.stand_pose(1, geom[:1], par)[0][0, 2])
    plant.reset(height=h)
    assert plant.contact.all() and plant.touch.all() and plant.feet_world.shape == (B, 4, 3)
    assert float(plant.feet_world[:, :, 2].sub(par.ground_z).abs().max()) < 1e-7
    # a constant that is not given keeps its last value: the ground moved to z = 0.1 stays there
    # through a call that sets the substeps alone
    plant.set_constants(ground_z=0.1)
    plant.set_constants(substeps=2)
    assert plant.engine.plant_constants == dict(foot_mass=0.15, substeps=2, ground_z=0.1, contact_tol=1e-4)
    plant.reset(height=h + 0.1 - par.ground_z)        # the feet at z = 0.1: on the moved ground, 0.1255 over the first
    assert plant.contact.all()
    plant.reset(height=h + 0.2 - par.ground_z)        # the feet at z = 0.2: over the moved ground
    assert not plant.contact.any()

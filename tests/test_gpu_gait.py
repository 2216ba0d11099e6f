"""GPU: mpcqp_gait_schedule -- every robot's gait record and control-iteration counter advanced
and switched at safe ticks in one launch -- against the integer restatement tests/gait_ref.py
(bitwise: every buffer is integers or untouched words), through the leg controller across two
switches against swing_ref.SwingRef, in a captured graph, and closing the loop with step_fused
and the plant against the CPU oracle loop's recorded figures (tests/golden/gait_switch.npz).

The leg controller's tolerance is tests/test_gpu_swing.py's BOUND, read from there.  The closed
loop is held to the hard limits of tests/test_gpu_plant.py (0.05 m, 0.1 rad; the pacing robot to
twice its recorded roll), to twice the CPU loop's recorded figures and to its switch ticks
exactly.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

# torch first: it brings its own HIP runtime, which must be loaded before libmpcqp.so
torch = pytest.importorskip("torch")

import gait_ref as gr  # noqa: E402
import plant_ref as pr  # noqa: E402
import swing_ref  # noqa: E402
from helpers import DEV, _dev  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -77
N = 10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gait_switch.npz")


def _bits(t):
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def all_gaits():
    from mpcqp.params import GAITS
    return [tuple(g) for g in GAITS.values()] + list(gr.CUSTOM)


@functools.lru_cache(maxsize=None)
def library():
    return gr.library(all_gaits()).astype(np.int32)


def scheduler(B, gaits=None, ibm=20, **kw):
    from mpcqp.gait import BatchedGaitScheduler
    return BatchedGaitScheduler(B, gaits=all_gaits() if gaits is None else gaits, iterations_between_mpc=ibm, device=DEV, **kw)


class Raw:
    """The buffers of one mpcqp_gait_schedule call with `pad` extra rows of a sentinel, and the
    call through the raw binding."""

    def __init__(self, sched, B, pad=0, seed=0):
        self.lib, self.ctx, self.B, self.pad = sched.lib, sched._ctx, B, pad
        i32 = dict(dtype=torch.int32, device=DEV)
        rows = B + pad
        self.state = torch.full((rows, 8), SENTINEL, **i32)
        self.gait = torch.full((rows, 9), SENTINEL, **i32)
        self.tick = torch.full((rows,), SENTINEL, **i32)
        rng = np.random.default_rng(seed)
        self.pattern = rng.integers(1, 2 ** 62, (rows, 32), dtype=np.int64)
        self.mem = _dev(self.pattern.view(np.float64))
        self.want = torch.full((rows,), SENTINEL, **i32)
        self.iteration = torch.full((rows,), SENTINEL, **i32)
        self.switched = torch.full((rows,), SENTINEL, **i32)
        self.status = torch.full((rows,), SENTINEL, **i32)
        self.vb = torch.full((rows, 3), float(SENTINEL), dtype=torch.float64, device=DEV)
        self.yr = torch.full((rows,), float(SENTINEL), dtype=torch.float64, device=DEV)

    order = ("want", "vb", "yr", "state", "gait", "tick", "mem", "iteration", "switched", "status")

    def call(self, flags, ibm, batch=None, auto=False, **override):
        p = {k: getattr(self, k).data_ptr() for k in self.order}
        if auto:
            p["want"] = 0
        else:
            p["vb"] = p["yr"] = 0
        p.update(override)
        return self.lib.mpcqp_gait_schedule(self.ctx, self.B if batch is None else batch, flags, ibm,
                                            *[ctypes.c_void_p(p[k]) if p[k] else None for k in self.order], None)

    def host(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy().copy() for k in self.order}


# ---- bitwise against the restatement

@pytest.mark.parametrize("ibm", [1, 3, 20])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_every_buffer_matches_the_restatement_on_every_tick(B, ibm):
    """Ten gaits (the seven named ones and the three custom records), seeded starting ticks
    congruent mod ibm, seeded requests that change about every 17 ticks (-1 and the current index
    among them), three spans of the longest gait: gait, tick, sched_state, all 32 words of
    swing_mem, iteration, switched and status equal gait_ref's on every tick, and the three rows
    past the batch keep their sentinel."""
    lib = library()
    sched = scheduler(B, ibm=ibm)
    raw = Raw(sched, B, pad=3, seed=B * 31 + ibm)
    rng = np.random.default_rng(1000 * B + ibm)
    cur = rng.integers(0, len(lib), B)
    state = np.zeros((B, 8), np.int32)
    state[:, gr.CUR] = state[:, gr.PENDING] = cur
    state[:, 6:8] = rng.integers(-99, 99, (B, 2))
    gait = lib[cur, :9].copy()
    tick = (rng.integers(0, 50, B) * ibm + int(rng.integers(0, ibm))).astype(np.int32)
    want = np.full(B, -1, np.int32)
    residue = int(tick[0]) % ibm
    mem = raw.pattern[:B].copy().view(np.float64)
    raw.state[:B], raw.gait[:B], raw.tick[:B], raw.want[:B] = _dev(state), _dev(gait), _dev(tick), _dev(want)
    T = 3 * 16 * ibm
    c = gr.Constants()
    wants = []
    for k in range(T):
        change = rng.random(B) < 1.0 / 17.0
        want = np.where(change, rng.integers(-1, len(lib), B), want).astype(np.int32)
        wants.append(want)
    wants = _dev(np.stack(wants))
    snap = []
    for k in range(T):
        raw.want[:B].copy_(wants[k])
        assert raw.call(gr.ADVANCE if k else 0, ibm) == 0
        snap.append([raw.state.clone(), raw.gait.clone(), raw.tick.clone(), raw.mem.clone(), raw.iteration.clone(),
                     raw.switched.clone(), raw.status.clone()])
    torch.cuda.synchronize()
    wants = wants.cpu().numpy()
    switches = 0
    for k in range(T):
        it, sw, st = gr.schedule(lib, c, gr.ADVANCE if k else 0, ibm, wants[k], state, gait, tick, mem)
        got = [t.cpu().numpy() for t in snap[k]]
        for name, g, r in zip(("state", "gait", "tick", "iteration", "switched", "status"),
                              (got[0], got[1], got[2], got[4], got[5], got[6]), (state, gait, tick, it, sw, st)):
            assert np.array_equal(g[:B], r), (name, k)
            assert (g[B:] == SENTINEL).all(), (name, k)
        assert np.array_equal(got[3][:B].view(np.int64), mem.view(np.int64)), ("swing_mem", k)
        assert np.array_equal(got[3][B:].view(np.int64), raw.pattern[B:]), ("swing_mem rows past the batch", k)
        assert (st == 0).all()
        switches += int(sw.sum())
    print(f"\nB = {B}, ibm = {ibm}: {switches} switches in {T} ticks")
    assert switches >= B // 2                 # about two per robot
    assert (tick % ibm == (residue + T - 1) % ibm).all()      # one fleet-wide MPC-tick flag stays right


# ---- misuse

def test_misuse_through_the_raw_binding():
    """Every MPCQP_ERR_ARG case returns it with a message and nothing written; batch == 0 is
    MPCQP_OK; refused libraries and constants leave the previous ones in force; the context works
    afterwards."""
    from mpcqp import _lib
    B = 5
    sched = scheduler(B)
    lib, ctx = sched.lib, sched._ctx
    raw = Raw(sched, B)
    before = raw.host()

    def refused(code, what):
        assert code == _lib.ERR_ARG and lib.mpcqp_last_error(ctx), what

    refused(raw.call(2, 20), "unknown flags")
    refused(raw.call(1, 20, batch=-1), "batch < 0")
    refused(raw.call(1, 0), "ibm < 1")
    for k in ("state", "gait", "tick"):
        refused(raw.call(1, 20, **{k: 0}), k)
    refused(raw.call(1, 20, state=raw.state.data_ptr() + 4), "sched_state off 16 bytes")
    refused(raw.call(1, 20, mem=raw.mem.data_ptr() + 8), "swing_mem off 16 bytes")
    refused(raw.call(1, 20, auto=True), "want NULL with the automatic choice disabled")
    assert raw.call(1, 20, batch=0) == _lib.MPCQP_OK
    # the library: refusals keep the ten gaits
    recs = lambda gaits: np.ascontiguousarray(np.stack([gr.record(g) for g in gaits]), np.int32)
    sg = lambda count, r: lib.mpcqp_set_gaits(ctx, count, None if r is None else r.ctypes.data_as(ctypes.c_void_p))
    trot = (10, (0, 5, 5, 0), (5, 5, 5, 5))
    refused(sg(0, recs([trot])), "count 0")
    refused(sg(17, recs([trot] * 17)), "count 17")
    refused(sg(1, None), "no records")
    for bad in ((0, (0,) * 4, (0,) * 4), (2049, (0,) * 4, (1,) * 4), (10, (0, 5, 5, 0), (5, -1, 5, 5)), (10, (0,) * 4, (5, 11, 5, 5)),
                (10, (0, 41, 5, 0), (5,) * 4), gr.NO_ENTRY):
        refused(sg(2, recs([trot, bad])), bad)
    # the constants
    ss = lambda *a: lib.mpcqp_set_gait_schedule(ctx, *a)
    for args in ((-1, -1, -1, 0.0, 0.0, 0.0, 0.0, 0), (0, 10, 2, 0.2, 0.1, 0.2, 0.1, 0), (0, 0, 10, 0.2, 0.1, 0.2, 0.1, 0),
                 (0, 0, -1, 0.2, 0.1, 0.2, 0.1, 0), (0, -2, 2, 0.2, 0.1, 0.2, 0.1, 0), (0, 0, 2, 0.1, 0.2, 0.2, 0.1, 0),
                 (0, 0, 2, 0.2, -0.1, 0.2, 0.1, 0), (0, 0, 2, 0.2, 0.1, 0.1, 0.2, 0), (0, 0, 2, 0.2, 0.1, 0.2, -0.1, 0),
                 (0, 0, 2, 0.2, 0.1, 0.2, 0.1, -1), (0, 0, 2, float("nan"), 0.1, 0.2, 0.1, 0),
                 (0, 0, 2, float("inf"), 0.1, 0.2, 0.1, 0), (0, -1, -1, 0.0, 0.0, float("nan"), 0.0, 0)):
        refused(ss(*args), args)
    refused(raw.call(1, 20, auto=True), "the refused constants did not turn the automatic choice on")
    after = raw.host()
    for k in raw.order:
        assert np.array_equal(_bits(torch.as_tensor(before[k])), _bits(torch.as_tensor(after[k]))), k
    # the automatic choice on: it needs both command pointers
    assert ss(0, 0, 2, 0.2, 0.1, 0.2, 0.1, 0) == _lib.MPCQP_OK
    refused(raw.call(1, 20, auto=True, vb=0), "automatic without vel_body_des")
    refused(raw.call(1, 20, auto=True, yr=0), "automatic without yaw_rate_des")
    # the context still works with the library it had: a standing robot asked for entry 9 switches
    # to the tenth record, and the optional arguments may be NULL
    raw.state.zero_()
    raw.gait.copy_(_dev(np.tile(library()[0, :9], (B, 1))))
    raw.tick.fill_(19)
    raw.want.fill_(9)
    assert raw.call(1, 20, mem=0, iteration=0, switched=0, status=0) == _lib.MPCQP_OK
    got = raw.host()
    assert (got["gait"] == library()[9, :9]).all() and (got["tick"] == library()[9, 9] * 20).all()
    assert np.array_equal(got["mem"].view(np.int64), raw.pattern) and (got["status"] == SENTINEL).all()
    # an entry tick beyond INT32_MAX: the first custom record enters at segment 2
    refused(raw.call(1, 2 ** 30 + 1), "e(g) * ibm beyond INT32_MAX")
    assert raw.call(1, 2 ** 29) == _lib.MPCQP_OK
    # a scheduler on a context without a library
    from mpcqp import LinearMpc
    eng = LinearMpc(horizon=N, robot="aliengo", device=DEV)
    bare = Raw(sched, B)
    bare.lib, bare.ctx = eng.lib, eng._ctx
    assert bare.call(1, 20) == _lib.ERR_ARG and eng.lib.mpcqp_last_error(eng._ctx)
    torch.cuda.synchronize()


def test_a_refused_robot_leaves_its_neighbours_alone():
    """A want outside the library, a negative tick, INT32_MAX under advance (UNSUPPORTED) and, under
    the automatic choice, a non-finite command (NONFINITE): the robot's status, its record as the
    rule leaves it, and every other robot bitwise as in a run without the bad values."""
    B, ibm = 67, 20
    lib = library()
    sched = scheduler(B, ibm=ibm)
    lb, ctx = sched.lib, sched._ctx
    rng = np.random.default_rng(5)
    cur = rng.integers(0, len(lib), B)
    state = np.zeros((B, 8), np.int32)
    state[:, gr.CUR] = state[:, gr.PENDING] = cur
    gait = lib[cur, :9].copy()
    tick = (rng.integers(0, 30, B) * ibm + ibm - 1).astype(np.int32)          # the call lands every robot on an aligned tick
    want = rng.integers(0, len(lib), B).astype(np.int32)

    def run(tick, want, auto=False, vb=None):
        raw = Raw(sched, B, seed=3)
        raw.state.copy_(_dev(state)), raw.gait.copy_(_dev(gait)), raw.tick.copy_(_dev(tick)), raw.want.copy_(_dev(want))
        if auto:
            raw.vb.copy_(_dev(vb)), raw.yr.zero_()
        assert raw.call(gr.ADVANCE, ibm, auto=auto) == 0
        return raw.host()
    clean = run(tick, want)
    assert clean["switched"].sum() > 5 and (clean["status"] == 0).all()
    t2, w2 = tick.copy(), want.copy()
    w2[[3, 64]] = (10, -5)
    t2[[0, 40]] = (-1, gr.INT_MAX)
    t2[66] = -2 ** 31
    bad = [0, 3, 40, 64, 66]
    got = run(t2, w2)
    ok = np.setdiff1d(np.arange(B), bad)
    assert (got["status"][bad] == gr.UNSUPPORTED).all() and (got["status"][ok] == 0).all()
    for k in ("state", "gait", "tick", "iteration", "switched"):
        assert np.array_equal(got[k][ok], clean[k][ok]), k
    assert np.array_equal(got["mem"][ok].view(np.int64), clean["mem"][ok].view(np.int64))
    assert np.array_equal(got["tick"][[0, 40, 66]], [-1, gr.INT_MAX, -2 ** 31])
    assert np.array_equal(got["state"][[0, 40, 66]], state[[0, 40, 66]]) and (got["switched"][bad] == 0).all()
    assert np.array_equal(got["tick"][[3, 64]], tick[[3, 64]] + 1) and (got["state"][[3, 64], gr.PENDING] == cur[[3, 64]]).all()
    # the same through the restatement
    s, g, t, m = state.copy(), gait.copy(), t2.copy(), Raw(sched, B, seed=3).pattern.view(np.float64).copy()
    it, sw, st = gr.schedule(lib, gr.Constants(), gr.ADVANCE, ibm, w2, s, g, t, m)
    for k, r in (("state", s), ("gait", g), ("tick", t), ("iteration", it), ("switched", sw), ("status", st)):
        assert np.array_equal(got[k], r), k
    # the automatic choice: idle 0, move 2; a NaN and an inf among commands of 0 and 1 m/s
    assert lb.mpcqp_set_gait_schedule(ctx, 0, 0, 2, 0.2, 0.1, 0.2, 0.1, 0) == 0
    vb = np.zeros((B, 3))
    vb[::2, 0] = 1.0
    clean = run(tick, want, auto=True, vb=vb)
    v2 = vb.copy()
    v2[7, 1], v2[65, 0] = np.nan, np.inf
    got = run(tick, want, auto=True, vb=v2)
    ok = np.setdiff1d(np.arange(B), [7, 65])
    assert (got["status"][[7, 65]] == gr.NONFINITE).all() and (got["status"][ok] == 0).all()
    for k in ("state", "gait", "tick", "iteration", "switched"):
        assert np.array_equal(got[k][ok], clean[k][ok]), k
    assert (got["switched"][[7, 65]] == 0).all() and np.array_equal(got["tick"][[7, 65]], tick[[7, 65]] + 1)
    assert np.array_equal(got["state"][[7, 65], 2], [1, 1]) and np.array_equal(got["gait"][[7, 65]], gait[[7, 65]])
    c = gr.Constants(idle=0, move=2, v_go=0.2, v_stop=0.1, w_go=0.2, w_stop=0.1, dwell=0)
    s, g, t = state.copy(), gait.copy(), tick.copy()
    it, sw, st = gr.schedule(lib, c, gr.ADVANCE, ibm, None, s, g, t, None, v2, np.zeros(B))
    for k, r in (("state", s), ("gait", g), ("tick", t), ("iteration", it), ("switched", sw), ("status", st)):
        assert np.array_equal(got[k], r), k
    assert sw.sum() > 5


# ---- the leg controller across two switches

def test_leg_controller_across_two_switches():
    """mpcqp_leg_torques on the scheduler's (gait, tick, swing_mem), B = 5, on swing_ref's seeded
    inputs, ibm = 4: trot10 -> pace10 -> bound8 with requests at staggered ticks.  tau,
    swing_state and swing_mem agree with SwingRef driven by gait_ref within the bound of
    tests/test_gpu_swing.py; the mask and the armed flags are exact."""
    from test_gpu_swing import BOUND, _engine
    B, ibm, T = 5, 4, 150
    gaits = ("trot10", "pace10", "bound8")
    eng = _engine()
    from mpcqp.gait import BatchedGaitScheduler
    sched = BatchedGaitScheduler(B, engine=eng, gaits=gaits, initial="trot10", iterations_between_mpc=ibm)
    from mpcqp.params import GAITS
    lib = gr.library([gr.record(GAITS[g]) for g in gaits]).astype(np.int32)
    inp = swing_ref.make_inputs(B, T, seed=77)
    f4, f8 = torch.float32, torch.float64
    per_tick = {k: _dev(inp[k], f4) for k in ("quat", "pos", "vel", "pos_feet", "foot_pos_base", "foot_vel_base")}
    const = {k: _dev(inp[k], f4) for k in ("thighs", "jac", "u0")}
    vb, yr = _dev(inp["v_body"], f8), _dev(inp["yaw_rate"], f8)
    tau = torch.zeros((T, B, 12), dtype=f4, device=DEV)
    ss = torch.zeros((T, B, 4), dtype=f4, device=DEV)
    asks = {13 + 3 * b: (b, 1) for b in range(B)}
    asks.update({85 + 5 * b: (b, 2) for b in range(B)})
    ref = swing_ref.SwingRef(B, kp=700.0, kd=20.0)
    state = np.zeros((B, 8), np.int32)
    gait, tick, want = np.tile(lib[0, :9], (B, 1)).astype(np.int32), np.zeros(B, np.int32), np.full(B, -1, np.int32)
    outs, sw_dev, sw_ref = [], [], []
    for k in range(T):
        if k in asks:
            b, g = asks[k]
            sched.request(gaits[g], robots=[b])
            want[b] = g
        sched.update(advance=k > 0)
        sw_dev.append(sched.switched.clone())
        eng.leg_torques(sched.tick, ibm, vb, yr, sched.gait, const["thighs"], per_tick["pos_feet"][k], per_tick["foot_pos_base"][k],
                        per_tick["foot_vel_base"][k], const["jac"], const["u0"], sched.swing_mem, tau[k], quat=per_tick["quat"][k],
                        pos=per_tick["pos"][k], vel=per_tick["vel"][k], swing_state=ss[k])
        mem = ref.mem.reshape(B, 32)
        _, sw, st = gr.schedule(lib, gr.Constants(), gr.ADVANCE if k else 0, ibm, want, state, gait, tick, mem)
        sw_ref.append(sw)
        outs.append(ref.step(tick.copy(), ibm, gait, inp["pos"][k], inp["vel"][k], inp["rot"][k], inp["v_body"], inp["yaw_rate"],
                             inp["thighs"], inp["pos_feet"][k], inp["foot_pos_base"][k], inp["foot_vel_base"][k], inp["jac"],
                             inp["u0"]))
    torch.cuda.synchronize()
    assert np.array_equal(torch.stack(sw_dev).cpu().numpy(), np.stack(sw_ref)) and (np.stack(sw_ref).sum(0) == 2).all()
    assert np.array_equal(sched.gait.cpu().numpy(), gait) and np.array_equal(sched.tick.cpu().numpy(), tick)
    assert np.array_equal(sched.sched_state.cpu().numpy(), state) and (sched.current.cpu().numpy() == 2).all()
    o = {k: np.stack([x[k] for x in outs]) for k in ("tau", "swing", "swing_state")}
    got_tau, got_ss = tau.cpu().numpy(), ss.cpu().numpy()
    assert np.array_equal(got_ss > 0, o["swing"])
    worst = {}
    for name, a, r in (("tau", got_tau, o["tau"]), ("swing_state", got_ss, o["swing_state"])):
        worst[name] = max(swing_ref.norm_err(a[:, b], r[:, b]) for b in range(B))
    m, r = sched.swing_mem.cpu().numpy().reshape(B, 4, 8), ref.mem
    assert np.array_equal(m[..., 0], r[..., 0])
    worst["mem"] = max(swing_ref.norm_err(m[b], r[b]) for b in range(B))
    print(f"\nleg controller across two switches: {worst} (bound {BOUND:g})")
    assert max(worst.values()) <= BOUND


# ---- the loop: step_fused and the plant

def fleet(plan=gr.PLAN, gaits=gr.PLAN_GAITS):
    """A controller (Aliengo, N = 10), a plant and a scheduler on one context, for a plan."""
    from mpcqp.controller import BatchedController
    from mpcqp.gait import BatchedGaitScheduler
    from mpcqp.plant import BatchedPlant
    B = len(plan)
    ctl = BatchedController(B, horizon=N, robot="aliengo", gait=[p["initial"] for p in plan])
    plant = BatchedPlant(B, controller=ctl, foot_mass=0.15, substeps=1, ground_z=-0.0255, contact_tol=1e-4)
    sched = BatchedGaitScheduler(B, controller=ctl, gaits=gaits, initial=[p["initial"] for p in plan])
    vb = torch.zeros((B, 3), dtype=torch.float64, device=DEV)
    vb[:, 0] = torch.as_tensor([p["command"] for p in plan], dtype=torch.float64)
    ctl.set_command(vb, 0.0)
    return ctl, plant, sched, vb


def run_plan(ctl, plant, sched, vb, plan, gaits, ticks, root_of=None):
    """ticks iterations of sched.update; step_fused; plant.step with the plan's requests and
    commands written on the device ahead of their iteration and nothing read back inside the loop.
    Returns the body words of the record per tick [T,B,13], switched [T,B] and the or of every
    status."""
    B = ctl.B
    events = gr.plan_events(plan, tuple(gaits))
    hist = torch.zeros((ticks, B, 13), dtype=torch.float64, device=DEV)
    switched = torch.zeros((ticks, B), dtype=torch.int32, device=DEV)
    bad = torch.zeros((B,), dtype=torch.int32, device=DEV)
    ibm = ctl.iterations_between_mpc
    for it in range(ticks):
        for b, w, v in events.get(it, ()):
            vb[b, 0] = v
            if w is not None:
                sched.request(w, robots=[b])
        sched.update(advance=it > 0)
        seen = plant.root if root_of is None else root_of(it)
        ctl.step_fused(None, None, None, seen, plant.dofs, mpc_tick=it % ibm == 0)
        plant.step(ctl.tau)
        hist[it] = plant.state[:, :13]
        switched[it] = sched.switched
        bad |= ctl.status | plant.status | sched.status
    torch.cuda.synchronize()
    return hist.cpu().numpy(), switched.cpu().numpy(), bad.cpu().numpy()


def _figures(hist, switched, dt=0.001):
    roll, pitch = (np.stack(x) for x in zip(*(pr.euler_zyx(h[:, 3:7]) for h in hist)))
    sw = [np.flatnonzero(switched[:, b]).tolist() for b in range(hist.shape[1])]
    return gr.figures(hist[:, :, 0], hist[:, :, 2], roll, pitch, sw, dt) + (sw, roll, pitch)


def test_the_scheduled_closed_loop_on_the_device():
    """gait_ref.PLAN, B = 6 (four robots asked to change gait at arbitrary ticks, one that trots
    throughout, one under the automatic choice), Aliengo, N = 10, 1400 iterations of sched.update;
    step_fused; plant.step: the switch ticks are the recorded ones exactly (320 / 1020, 600, 500,
    200 / 1000, none, 260 / 960), every plant, solve and scheduler status is OK, the hard limits
    0.05 m / 0.1 rad hold for all but the pacing robot, each robot's worst height error and roll /
    pitch are within twice the CPU loop's recorded figure (floor 1e-6) and its phase speeds within
    0.05 m/s of the recorded ones."""
    fx = dict(np.load(GOLDEN))
    ctl, plant, sched, vb = fleet()
    sched.auto(start=5, **gr.PLAN_AUTO)
    plant.reset()
    hist, switched, bad = run_plan(ctl, plant, sched, vb, gr.PLAN, gr.PLAN_GAITS, gr.PLAN_TICKS)
    err, tilt, speeds, sw, roll, pitch = _figures(hist, switched)
    for b in range(len(gr.PLAN)):
        print(f"robot {b}: switches {sw[b]}, height error {err[b]:.4f} m (recorded {fx['height_error'][b]:.4f}), roll / pitch "
              f"{tilt[b]:.4f} rad (recorded {fx['tilt'][b]:.4f}), phase speeds {np.round(speeds[b], 4).tolist()} "
              f"(recorded {np.round(fx['phase_speed'][b], 4).tolist()})")
    assert tuple(tuple(s) for s in sw) == gr.PLAN_SWITCHES
    assert sw == [[int(x) for x in row if x >= 0] for row in fx["switch_ticks"]]
    assert np.isfinite(hist).all() and (bad == 0).all()
    pacing = 2
    others = [b for b in range(len(gr.PLAN)) if b != pacing]
    assert (np.abs(hist[:, :, 2] - 0.38) < 0.05).all()
    assert (np.abs(roll[:, others]) < 0.1).all() and (np.abs(pitch[:, others]) < 0.1).all()
    assert (err <= 2 * fx["height_error"]).all()
    assert (tilt <= np.maximum(2 * fx["tilt"], 1e-6)).all()
    for b, row in enumerate(speeds):
        assert (np.abs(np.array(row) - fx["phase_speed"][b, :len(row)]) <= 0.05).all(), (b, row)
    assert np.array_equal(sched.switches.cpu().numpy(), [2, 1, 1, 2, 0, 2])
    assert np.array_equal(sched.current.cpu().numpy(), [0, 0, 2, 1, 1, 0])


def test_the_sensing_chain_across_two_switches():
    """B = 2, stand -> trot10 at 0.5 m/s (asked at 313, entered at 320) -> stand (asked at 717, at 720), 900 iterations with
    the controller fed est.update_from_imu(..., tick=ctl.tick_count, touch=plant.touch).  The
    robots start standing on the ground and the estimator settles for 50 ticks first, as in
    tests/test_gpu_plant.py's sensing-chain test, which allows what this one allows: every status
    OK and the hard limits 0.05 m / 0.1 rad; the estimate's error against plant.root is printed."""
    import kin_ref
    from mpcqp.estimator import BatchedEstimator
    plan = tuple(dict(initial="standing", command=0.0, requests=((313, "trot10", 0.5), (717, "standing", 0.0))) for _ in range(2))
    B = len(plan)
    ctl, plant, sched, vb = fleet(plan)
    par = pr.Params()
    geom = plant.geometry.cpu().numpy()
    root0, _ = pr.stand_pose(B, geom, par)
    plant.reset(height=float(root0[0, 2]))
    assert plant.contact.all()
    est = BatchedEstimator(B, robot="aliengo", controller=ctl, contact_height=par.ground_z)
    _, _, Jb = kin_ref.chain(geom, plant.dofs[:, :, 0].cpu().numpy())
    m = float(plant.robot[0, 0])
    stand = _dev(np.einsum("blcr,c->blr", Jb, -np.array([0, 0, m * par.gravity / 4])).reshape(B, 12), torch.float32)
    for it in range(50):
        plant.step(stand)
        est.update_from_imu(plant.gyro, plant.accel, plant.dofs, tick=ctl.tick_count, touch=plant.touch)
    errs = []
    bad_est = torch.zeros((B,), dtype=torch.int32, device=DEV)

    def seen(it):
        r = est.update_from_imu(plant.gyro, plant.accel, plant.dofs, tick=ctl.tick_count, touch=plant.touch)
        errs.append((r - plant.root).abs())
        bad_est.__ior__(est.status | est.attitude_status)
        return r
    hist, switched, bad = run_plan(ctl, plant, sched, vb, plan, gr.PLAN_GAITS, 900, root_of=seen)
    err, tilt, speeds, sw, roll, pitch = _figures(hist, switched)
    e = torch.stack(errs).cpu().numpy()
    print(f"\nsensing chain across two switches {sw}: height error {err}, roll / pitch {tilt}, phase speeds {speeds}\n"
          f"  estimate against plant.root: position {e[:, :, 0:3].max():.4f} m (x {e[:, :, 0].max():.4f}, "
          f"z {e[:, :, 2].max():.4f}), velocity {e[:, :, 7:10].max():.4f} m/s")
    assert sw == [[320, 720], [320, 720]]
    assert np.isfinite(hist).all() and (bad == 0).all() and (bad_est.cpu().numpy() == 0).all()
    assert (np.abs(hist[:, :, 2] - 0.38) < 0.05).all() and (np.abs(roll) < 0.1).all() and (np.abs(pitch) < 0.1).all()


def test_graph_capture_replays_the_eager_loop_bitwise():
    """bind_update, the between-solves step_fused launch and plant.bind_step captured once on one
    stream and replayed across a seam -- with a request written into the want tensor between two
    replays -- leave bitwise what the eager loop leaves.  The solve launches stay outside the
    capture: on an MPC tick, which every seam is, the scheduler's launch is replayed from a graph
    of its own (the switch happens inside a replay) and step_fused and the plant run eagerly."""
    plan = tuple(dict(initial="trot10", command=0.5) for _ in range(4))
    gaits = ("standing", "trot10", "pace10")
    runs = []
    for graphed in (False, True):
        ctl, plant, sched, vb = fleet(plan, gaits)
        B = ctl.B
        plant.reset()
        want = torch.full((B,), -1, dtype=torch.int32, device=DEV)
        sched.request(want)
        update, step = sched.bind_update(advance=True), plant.bind_step(ctl.tau)

        def between():
            s = torch.cuda.current_stream(DEV)
            update(s)
            ctl.step_fused(None, None, None, plant.root, plant.dofs, mpc_tick=False)
            step(s)
        g = gu = None
        seen = []
        for it in range(130):
            if it == 37:
                want[:2] = torch.tensor([2, 0], dtype=torch.int32, device=DEV)      # honoured at the seam at 100
            if it % ctl.iterations_between_mpc == 0:
                if it == 0:
                    sched.update(advance=False)
                elif not graphed:
                    update(torch.cuda.current_stream(DEV))
                else:
                    if gu is None:
                        torch.cuda.synchronize()
                        gu = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(gu):
                            update(torch.cuda.current_stream(DEV))
                    gu.replay()
                ctl.step_fused(None, None, None, plant.root, plant.dofs, mpc_tick=True)
                plant.step(ctl.tau)
            elif not graphed:
                between()
            else:
                if g is None:
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        between()
                g.replay()
            seen.append(sched.switched.clone())
        torch.cuda.synchronize()
        sw = torch.stack(seen).cpu().numpy()
        assert [np.flatnonzero(sw[:, b]).tolist() for b in range(B)] == [[100], [100], [], []]
        assert (plant.status == 0).all() and (ctl.status == 0).all() and (sched.status == 0).all()
        runs.append([_bits(t) for t in (plant.state, plant.root, plant.dofs, ctl.tau, ctl.swing_mem, ctl.plan_state,
                                        ctl.tick_count, ctl.gait, sched.sched_state)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_python_surface_on_the_device():
    """request in its forms, reset of some robots, min_hold, the views; a refused library and a
    refused constant raise and keep what was there."""
    from mpcqp._lib import MpcqpError
    sched = scheduler(4, gaits=("standing", "trot10", "pace10"), initial="standing")
    assert sched.current.tolist() == [0] * 4 and sched.gait[0].tolist() == gr.record((16, (0,) * 4, (16,) * 4)).tolist()
    sched.request("trot10")
    sched.request(2, robots=[3])
    sched.request((16, (0, 0, 0, 0), (16, 16, 16, 16)), robots=slice(0, 1))
    sched.update(advance=False)
    assert sched.switched.tolist() == [0, 1, 1, 1] and sched.current.tolist() == [0, 1, 1, 2] and sched.tick.tolist() == [0] * 4
    sched.request(["standing", None, -1, "trot10"])
    sched.set_constants(min_hold=30)
    for _ in range(20):
        sched.update()
    assert sched.switched.tolist() == [0] * 4 and sched.pending.tolist() == [0, 1, 1, 1] and sched.since.tolist() == [20] * 4
    sched.set_constants(min_hold=0)
    sched.update(iteration=True)
    assert sched.tick.tolist() == [21] * 4 and sched.iteration.tolist() == [1] * 4
    sched.reset(robots=[1])
    assert sched.tick.tolist() == [21, 0, 21, 21] and sched.current.tolist() == [0, 0, 1, 2] and sched.want.tolist() == [0, -1, -1, 1]
    with pytest.raises(MpcqpError):
        sched.set_gaits([gr.NO_ENTRY])
    with pytest.raises(MpcqpError):
        sched.set_constants(min_hold=-1)
    with pytest.raises(ValueError):
        sched.request("bound8")
    sched.update()
    assert sched.status.tolist() == [0] * 4 and sched.tick.tolist() == [22, 1, 22, 22]

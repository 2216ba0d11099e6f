"""GPU: mpcqp_leg_torques -- swing state, foot placement, swing trajectory and all 12
joint torques of every robot in one launch -- against the reference's recorded run
(tests/golden/swing.npz) and the float64 restatement tests/swing_ref.py.

Tolerance (norm-wise per robot, max|a - a_ref| / max|a_ref|).  Measured on the CPU
against swing.npz (tests/test_swing.py prints them):
    tests/swing_ref.py                         1.152e-07  (tau; targets 6.0e-08, final 2.6e-09)
    csrc/mpcqp_swing_leg.h compiled with g++   1.152e-07  (the same figures)
Both carry the reference's float32 intermediates under NumPy 2.2 promotion, its
float32 break points and scipy standing in for Drake; the largest is one float32 ulp
of the float32 torques.  The device bound is 4 x the larger, BOUND = 4.61e-07 (above
the two-ulp floor 2.4e-07, under the project's 1e-5 regression guard).  The same bound
holds against swing_ref, from which the device differs by float64 rounding and the
float32 rounding of its outputs (measured on the MI355X against swing.npz, all three
input variants alike: tau 1.15e-07, pos_target 7.0e-08, vel_target 5.7e-08, swing_state
2.0e-08, foothold 2.6e-09, remaining time and lift-off position exact).  Masks, flags and stance entries have no tolerance:
a stance entry of tau is bitwise what mpcqp_stance_torques writes (no ulp needed).
"""
import numpy as np
import pytest

# torch first: it brings its own HIP runtime, which must be loaded before libmpcqp.so
# pulls in the system's (a CPU test file collected ahead of this one loads the library)
torch = pytest.importorskip("torch")

import swing_ref  # noqa: E402
from swing_ref import norm_err, run_ref  # noqa: E402
from helpers import DEV, _dev  # noqa: E402

pytestmark = pytest.mark.gpu

BOUND = 4.61e-7


def _engine(kp=700.0, kd=20.0, **kw):
    from mpcqp import LinearMpc
    eng = LinearMpc(horizon=10, robot="aliengo", device=DEV)
    eng.set_planner(dt_control=0.001, gravity=9.81)
    eng.set_swing(Kp=kp, Kd=kd, **kw)
    return eng


def run_device(eng, inp, gait, ticks, ibm, layout="split", groups=None, pad=0, sentinel=-77.0, mem_every=0,
               swing=None, mem0=None):
    """Run T ticks of B robots on the device.  inp: swing_ref.make_inputs-style arrays
    (per-tick [T,B,...] or per-robot [B,...]); ticks [T,B].  groups: [(slice, Kp, Kd)] launched
    one after the other with their own gains (default: one launch per tick) and the scalars
    `swing` (set_swing keywords; default: set_swing's defaults).  The output buffers have
    `pad` extra rows filled with `sentinel`, returned too.  mem0 [B,STRIDE]: the generator
    state the run starts from (default: zeros)."""
    ticks = np.asarray(ticks, np.int32)
    T, B = ticks.shape
    f4, f8 = torch.float32, torch.float64
    per_tick = {k: _dev(inp[k], f4) for k in ("quat", "pos", "vel", "rot", "pos_feet", "foot_pos_base",
                                              "foot_vel_base")}
    rs = _dev(swing_ref.root_states(inp["quat"], inp["pos"], inp["vel"]), f4)
    const = {k: _dev(inp[k], f4) for k in ("thighs", "jac", "u0")}
    vb, yr = _dev(inp["v_body"], f8), _dev(inp["yaw_rate"], f8)
    g, tk = _dev(gait, torch.int32), _dev(ticks, torch.int32)
    full = lambda *s, dt=f4: torch.full(s, sentinel, dtype=dt, device=DEV)
    tau, ss = full(T, B + pad, 12), full(T, B + pad, 4)
    pt, vt = full(T, B + pad, 4, 3), full(T, B + pad, 4, 3)
    mem = full(B + pad, swing_ref.STRIDE, dt=f8)
    mem[:B] = 0.0 if mem0 is None else _dev(mem0, f8).reshape(B, swing_ref.STRIDE)
    cks = []
    for t in range(T):
        for sl, kp, kd in (groups or [(slice(0, B), None, None)]):
            if kp is not None:
                eng.set_swing(Kp=kp, Kd=kd, **(swing or {}))
            kw = dict(root_states=rs[t, sl]) if layout == "root" else dict(
                quat=per_tick["quat"][t, sl], pos=per_tick["pos"][t, sl], vel=per_tick["vel"][t, sl],
                rot=per_tick["rot"][t, sl] if layout == "rot" else None)
            eng.leg_torques(tk[t, sl], ibm, vb[sl], yr[sl], g[sl], const["thighs"][sl], per_tick["pos_feet"][t, sl],
                            per_tick["foot_pos_base"][t, sl], per_tick["foot_vel_base"][t, sl], const["jac"][sl],
                            const["u0"][sl], mem[:B][sl], tau[t, :B][sl], swing_state=ss[t, :B][sl],
                            pos_target=pt[t, :B][sl], vel_target=vt[t, :B][sl], **kw)
        if mem_every and t % mem_every == 0:
            cks.append(mem[:B].clone())
    torch.cuda.synchronize()
    out = dict(tau=tau, swing_state=ss, pos_target=pt, vel_target=vt, mem=mem)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    if cks:
        out["ck_mem"] = torch.stack(cks, 1).cpu().numpy().reshape(B, len(cks), 4, 8)
    return out


def assert_matches_ref(out, ref, B, tag=""):
    """Mask exact, values within BOUND per robot (over the ticks of the run)."""
    assert np.array_equal(out["swing_state"][:, :B] > 0, ref["swing"]), tag
    for k in ("tau", "swing_state", "pos_target", "vel_target"):
        for b in range(B):
            e = norm_err(out[k][:, b], ref[k][:, b])
            assert e <= BOUND, (tag, k, b, e)
    # the generator state: flags exact, the rest per robot
    m, r = out["mem"][:B].reshape(B, 4, 8), ref["mem"].reshape(B, 4, 8)
    assert np.array_equal(m[..., 0], r[..., 0]), tag
    for b in range(B):
        e = norm_err(m[b], r[b])
        assert e <= BOUND, (tag, "mem", b, e)


@pytest.fixture(scope="module")
def fx():
    return swing_ref.load_fixture()


@pytest.fixture(scope="module")
def fx_inputs(fx):
    """The fixture's inputs as [T,B,...] arrays, R_base by the float32 quat2matrix."""
    return swing_ref.fixture_inputs(fx)


def fixture_sequence_checks(fx, fx_inputs, layout, eng, groups, swing=None):
    """A recorded run of the reference through one input layout: mask exact on every tick,
    first-swing flags exact at the checkpoints, tau / targets / swing_state / checkpointed
    swing_mem within BOUND; for "split" also the stance entries bitwise those of
    mpcqp_stance_torques on the same inputs."""
    B, T = fx["tau"].shape[:2]
    ibm, every = int(fx["iterations_between_mpc"]), int(fx["check_every"])
    ticks = np.tile(np.arange(T)[:, None], (1, B))
    out = run_device(eng, fx_inputs, fx["gait"], ticks, ibm, layout=layout, groups=groups, mem_every=every,
                     swing=swing)
    seq = {k: np.swapaxes(out[k], 0, 1) for k in ("tau", "swing_state", "pos_target", "vel_target")}
    seq["ck_mem"] = out["ck_mem"]
    errs = swing_ref.compare_fixture(fx, seq)          # asserts the mask and the flags
    print("\n" + layout + ": " + ", ".join(f"{k} {float(v.max()):.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert (v <= BOUND).all(), (layout, k, v)
    if layout != "split":
        return
    # stance entries against mpcqp_stance_torques, tick by tick
    jac, u0 = _dev(fx["jac"]), _dev(fx["u0"])
    stance = _dev((out["swing_state"] == 0).astype(np.float32))       # [T,B,4]
    tau2 = torch.full((T, B, 12), 5.0, dtype=torch.float32, device=DEV)
    for t in range(T):
        eng.stance_torques(jac, stance[t], u0, tau2[t])
    torch.cuda.synchronize()
    st = np.repeat(out["swing_state"] == 0, 3, axis=2)
    assert st.any() and (~st).any()
    assert np.array_equal(out["tau"][st].view(np.uint32), tau2.cpu().numpy()[st].view(np.uint32))


@pytest.mark.parametrize("layout", ["split", "root", "rot"])
def test_fixture_sequence(fx, fx_inputs, layout):
    """The reference's recorded run, B = 6, through both input layouts and once more with
    R_base supplied: mask exact on every tick, first-swing flags exact at the checkpoints,
    tau / targets / swing_state / checkpointed swing_mem within BOUND; stance entries
    bitwise those of mpcqp_stance_torques on the same inputs."""
    eng = _engine(swing_height=float(fx["swing_height"]), touchdown_z=float(fx["touchdown_z"]),
                  vel_gain=float(fx["vel_gain"]))
    groups = [(slice(0, 3), float(fx["kp"][0]), float(fx["kd"][0])), (slice(3, 6), float(fx["kp"][3]),
                                                                      float(fx["kd"][3]))]
    assert (fx["kp"][:3] == fx["kp"][0]).all() and (fx["kp"][3:] == fx["kp"][3]).all()
    fixture_sequence_checks(fx, fx_inputs, layout, eng, groups)


@pytest.mark.parametrize("B", [1, 65, 257])
def test_tail_workgroup_and_masking(B):
    """B = 1, 65, 257 (not multiples of the 64 robots a workgroup owns) against swing_ref
    for 3 ticks around a lift-off and 3 around a touchdown of TROTTING10 at the reference's
    iterations_between_mpc = 20, every gait in the batch; nothing is written past row B."""
    from mpcqp.params import GAITS, gait_record
    names = ["trot10"] + [k for k in GAITS if k != "trot10"]
    gait = np.stack([gait_record(names[b % len(names)]) for b in range(B)])
    t_seq = [100, 101, 102, 199, 200, 201]
    ticks = np.tile(np.array(t_seq)[:, None], (1, B))
    inp = swing_ref.make_inputs(B, len(t_seq), seed=100 + B)
    for layout in ("split", "root"):
        out = run_device(_engine(), inp, gait, ticks, 20, layout=layout, pad=3, sentinel=-77.0)
        ref = run_ref(inp, gait, ticks, 20)
        assert ref["swing"][:, 0].any() and not ref["swing"][:, 0].all()
        assert_matches_ref(out, ref, B, tag=(B, layout))
        for k in ("tau", "swing_state", "pos_target", "vel_target"):
            assert (out[k][:, B:] == -77.0).all(), k
        assert (out["mem"][B:] == -77.0).all()


class _LegCall:
    """mpcqp_leg_torques / _root_states through the C ABI for B robots on one tick: every
    argument a valid device buffer (the outputs with 3 extra rows, all SENTINEL) unless
    overridden, None = NULL."""
    SENTINEL = -77.0

    def __init__(self, eng, B, seed, tick=120):
        import ctypes
        from mpcqp.params import GAITS, gait_record
        self.eng, self.B, self.ctypes = eng, B, ctypes
        names = ["trot10"] + [k for k in GAITS if k != "trot10"]
        inp = swing_ref.make_inputs(B, 1, seed=seed)
        f4, f8 = torch.float32, torch.float64
        self.t = {k: _dev(inp[k][0], f4) for k in ("quat", "pos", "vel", "pos_feet", "foot_pos_base", "foot_vel_base")}
        self.t.update({k: _dev(inp[k], f4) for k in ("thighs", "jac", "u0")})
        self.t.update(rot=None, rs=_dev(swing_ref.root_states(inp["quat"], inp["pos"], inp["vel"])[0], f4),
                      vb=_dev(inp["v_body"], f8), yr=_dev(inp["yaw_rate"], f8),
                      gait=_dev(np.stack([gait_record(names[b % len(names)]) for b in range(B)]), torch.int32),
                      tick=torch.full((B,), tick, dtype=torch.int32, device=DEV))
        self.fresh()

    def fresh(self):
        B = self.B
        full = lambda *s: torch.full(s, self.SENTINEL, dtype=torch.float32, device=DEV)
        self.out = dict(tau=full(B + 3, 12), swing_state=full(B + 3, 4), pos_target=full(B + 3, 4, 3),
                        vel_target=full(B + 3, 4, 3))
        self.mem = torch.full((B + 3, swing_ref.STRIDE), self.SENTINEL, dtype=torch.float64, device=DEV)
        self.mem[:B] = 0.0

    def __call__(self, root=False, batch=None, flags=0, ibm=20, **kw):
        a = dict(self.t, mem=self.mem, **self.out)
        a.update(kw)
        ptr = lambda x: None if x is None else self.ctypes.c_void_p(x.data_ptr())
        tail = [ptr(a[k]) for k in ("vb", "yr", "gait", "thighs", "pos_feet", "foot_pos_base", "foot_vel_base", "jac",
                                    "u0", "mem", "tau", "swing_state", "pos_target", "vel_target")]
        lib, ctx, batch = self.eng.lib, self.eng._ctx, self.B if batch is None else batch
        if root:
            return lib.mpcqp_leg_torques_root_states(ctx, batch, flags, ptr(a["tick"]), ibm, ptr(a["rs"]), *tail, None)
        return lib.mpcqp_leg_torques(ctx, batch, flags, ptr(a["tick"]), ibm, *(ptr(a[k]) for k in ("quat", "pos", "vel", "rot")),
                                     *tail, None)

    def read(self):
        torch.cuda.synchronize()
        return dict({k: v.cpu().numpy() for k, v in self.out.items()}, mem=self.mem.cpu().numpy())


def test_argument_errors():
    """Every MPCQP_ERR_ARG branch of the leg-torque launch, each with its word in
    mpcqp_last_error, B = 5; batch = 0 is a successful no-op; a refused call runs nothing."""
    from mpcqp import _lib
    eng = _engine()
    c = _LegCall(eng, 5, seed=51)
    odd = torch.zeros((5 * swing_ref.STRIDE + 1,), dtype=torch.float64, device=DEV)[1:]      # 8 bytes off a 16-byte line
    assert odd.data_ptr() % 16 == 8
    required = ("tick", "quat", "pos", "vel", "vb", "yr", "gait", "thighs", "pos_feet", "foot_pos_base", "foot_vel_base",
                "jac", "u0", "mem", "tau")
    refused = [(dict(batch=-1), "batch"), (dict(batch=-1, root=True), "batch"), (dict(flags=1), "flags"),
               (dict(flags=2, root=True), "flags"), (dict(ibm=0), "iterations_between_mpc"),
               (dict(ibm=-20, root=True), "iterations_between_mpc"), (dict(mem=odd), "aligned"),
               (dict(mem=odd, root=True), "aligned"), (dict(rs=None, root=True), "null")]
    refused += [({k: None}, "null") for k in required]
    refused += [({k: None, "root": True}, "null") for k in required if k not in ("quat", "pos", "vel")]
    for kw, word in refused:
        assert c(**kw) == _lib.ERR_ARG, kw
        assert word in eng.lib.mpcqp_last_error(eng._ctx).decode(), (kw, eng.lib.mpcqp_last_error(eng._ctx))
    assert c(batch=0) == 0 and c(batch=0, root=True) == 0 and c(batch=0, quat=None, tau=None) == 0
    o = c.read()
    assert all((o[k] == c.SENTINEL).all() for k in c.out) and (o["mem"][:5] == 0).all() and (o["mem"][5:] == c.SENTINEL).all()
    assert c() == 0                                               # the same buffers serve a good call
    o = c.read()
    assert all((o[k][:5] != c.SENTINEL).all() and (o[k][5:] == c.SENTINEL).all() for k in c.out)
    assert (o["mem"][:5] != 0).any() and (o["mem"][5:] == c.SENTINEL).all()


@pytest.mark.parametrize("layout", ["split", "root"])
def test_nullable_outputs_absent(layout):
    """swing_state, pos_target and vel_target NULL in turn, B = 5 on a tick with legs in swing:
    tau, swing_mem and the other outputs are bitwise those of the full launch, and the absent
    buffer keeps its sentinel."""
    eng = _engine()
    c = _LegCall(eng, 5, seed=52)
    root = layout == "root"
    assert c(root=root) == 0
    want = c.read()
    assert (want["swing_state"][:5] > 0).any() and (want["swing_state"][:5] == 0).any()
    for skip in ("swing_state", "pos_target", "vel_target"):
        c.fresh()
        absent = c.out[skip]
        assert c(root=root, **{skip: None}) == 0
        got = c.read()
        assert (got[skip] == c.SENTINEL).all() and absent is c.out[skip], skip
        for k in want:
            if k != skip:
                assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (skip, k)


def test_reference_defaults_two_periods():
    """iterations_between_mpc = 20, TROTTING10, B = 3 with different per-robot tick
    offsets, 420 ticks (two full periods and a bit): every leg lifts off, lands and
    re-arms at least twice."""
    from mpcqp.params import gait_record
    B, T = 3, 420
    gait = np.tile(gait_record("TROTTING10"), (B, 1))
    ticks = np.arange(T)[:, None] + np.array([0, 7, 133])[None]
    inp = swing_ref.make_inputs(B, T, seed=9)
    out = run_device(_engine(kp=200.0), inp, gait, ticks, 20, layout="root")
    ref = run_ref(inp, gait, ticks, 20, kp=200.0)
    rearm = (ref["swing_state"] >= 1.0).sum(axis=0)
    assert (rearm >= 2).all()
    assert_matches_ref(out, ref, B)


def test_custom_gait_wraps_the_swing_offset_per_leg():
    """offset + duration > period on leg 1 only: that leg's swing window wraps around the
    period, the other three keep theirs (the reference would shift all four)."""
    from mpcqp.params import gait_record
    ibm, period = 4, 10
    off, dur = (0, 7, 5, 2), (5, 6, 5, 3)
    assert [o + d > period for o, d in zip(off, dur)] == [False, True, False, False]
    gait = gait_record((period, off, dur))[None]
    T = 2 * ibm * period + 5
    ticks = np.arange(T)[:, None]
    inp = swing_ref.make_inputs(1, T, seed=17)
    out = run_device(_engine(), inp, gait, ticks, ibm)
    ref = run_ref(inp, gait, ticks, ibm)
    assert_matches_ref(out, ref, 1)
    # the windows, written out: a leg swings on ticks c with 1 <= (c - (off + dur) * ibm) mod 40 <= (10 - dur) * ibm
    c = np.arange(T) % (ibm * period)
    for leg in range(4):
        cs = (c - (off[leg] + dur[leg]) * ibm) % (ibm * period)
        want = (cs >= 1) & (cs <= (period - dur[leg]) * ibm)
        assert np.array_equal(out["swing_state"][:, 0, leg] > 0, want), leg


def _controller_inputs(B, T, seed):
    inp = swing_ref.make_inputs(B, T, seed)
    rs = swing_ref.root_states(inp["quat"], inp["pos"], inp["vel"])
    return inp, rs


def test_partial_reset():
    """reset(robots) clears those robots' swing_mem and leaves the others' untouched; the
    reset robots latch init again on their next swing tick."""
    from mpcqp.controller import BatchedController
    B, ibm = 4, 4
    ctl = BatchedController(B, horizon=10, robot="aliengo", gait="trot10", iterations_between_mpc=ibm)
    inp, rs = _controller_inputs(B, 8, seed=3)
    d = lambda k, t: _dev(inp[k][t])
    step = lambda t, it: ctl.leg_torques(it, inp["v_body"], inp["yaw_rate"], _dev(inp["thighs"]), d("pos_feet", t),
                                         d("foot_pos_base", t), d("foot_vel_base", t), _dev(inp["jac"]),
                                         root_states=_dev(rs[t]))
    for t in range(4):                     # ticks 1..4: legs 1 and 2 swing (stance offsets 5)
        step(t, 1 + t)
    before = ctl.swing_mem.cpu().numpy().reshape(B, 4, 8)
    assert (before[:, 1:3, 0] == 1.0).all() and (before[:, [0, 3], 0] == 0.0).all()
    assert np.array_equal(before[:, 1:3, 2:5], inp["pos_feet"][0][:, 1:3].astype(np.float64))
    ctl.reset([1, 3])
    after = ctl.swing_mem.cpu().numpy().reshape(B, 4, 8)
    assert np.array_equal(after[[0, 2]], before[[0, 2]]) and (after[[1, 3]] == 0).all()
    step(4, 5)
    m = ctl.swing_mem.cpu().numpy().reshape(B, 4, 8)
    now = inp["pos_feet"][4].astype(np.float64)
    assert np.array_equal(m[[1, 3]][:, 1:3, 2:5], now[[1, 3]][:, 1:3])          # latched again
    assert np.array_equal(m[[0, 2]][:, 1:3, 2:5], before[[0, 2]][:, 1:3, 2:5])  # kept
    assert (m[[1, 3]][:, 1:3, 1] > m[[0, 2]][:, 1:3, 1]).all()                  # a fresh swing time


def test_batched_controller_leg_torques_after_tick():
    """tick() then leg_torques() for a mixed-gait batch: 12 finite torques per robot, the
    swing entries from the PD law on the generated targets, the stance entries from u0."""
    from mpcqp.controller import BatchedController
    from mpcqp.params import SWING_PRESETS
    names = ["trot10", "pace10", "standing", "jump16", "trot16", "pace16"]
    B, ibm = 12, 20
    gsel = [names[b % len(names)] for b in range(B)]
    ctl = BatchedController(B, horizon=10, robot="a1", gait=gsel, iterations_between_mpc=ibm)
    inp, rs = _controller_inputs(B, 2, seed=21)
    feet = _dev(inp["pos_feet"][0] - inp["pos"][0][:, None, :])
    it = 120      # an MPC tick inside a swing of trot10 legs 0 and 3
    ctl.tick(it, inp["v_body"], inp["yaw_rate"], feet, root_states=_dev(rs[0]))
    tau = ctl.leg_torques(it, inp["v_body"], inp["yaw_rate"], _dev(inp["thighs"]), _dev(inp["pos_feet"][0]),
                          _dev(inp["foot_pos_base"][0]), _dev(inp["foot_vel_base"][0]), _dev(inp["jac"]),
                          root_states=_dev(rs[0]))
    torch.cuda.synchronize()
    tau = tau.cpu().numpy()
    assert tau.shape == (B, 12) and np.isfinite(tau).all()
    u0 = ctl.u0.cpu().numpy()
    ss = ctl.swing_state.cpu().numpy()
    sw = ss > 0
    want_mask, _, _ = swing_ref.swing_state(np.full(B, it), ibm, ctl.gait.cpu().numpy())
    assert np.array_equal(sw, want_mask) and sw.any() and (~sw).any() and not sw[2].any()
    J = inp["jac"].astype(np.float64)
    R = inp["rot"][0].astype(np.float64)
    pt, vt = ctl.pos_target.cpu().numpy().astype(np.float64), ctl.vel_target.cpu().numpy().astype(np.float64)
    rot = lambda x: np.einsum("brc,blc->blr", R, x.astype(np.float64))
    g = SWING_PRESETS["a1"]
    e = g["kp"] * (rot(pt) - rot(inp["foot_pos_base"][0])) + g["kd"] * (rot(vt) - rot(inp["foot_vel_base"][0]))
    pd = np.einsum("blcr,blc->blr", J, e)
    st = np.einsum("blcr,blc->blr", J, -u0.reshape(B, 4, 3).astype(np.float64))
    t3 = tau.reshape(B, 4, 3)
    for b in range(B):
        # the targets read back are float32 (6e-8 each) and the PD error cancels them against the
        # foot state: the project's 1e-5 regression guard, not BOUND
        if sw[b].any():
            assert norm_err(t3[b][sw[b]], pd[b][sw[b]]) < 1e-5, b
        if (~sw[b]).any():
            assert norm_err(t3[b][~sw[b]], st[b][~sw[b]]) <= BOUND, b


def test_graph_capture_replays_with_fresh_ticks():
    """plan + leg_torques for B = 64 captured into one graph and replayed 5 times while the
    device tick tensor advances: the same tau as 5 eager calls."""
    from mpcqp._lib import PLAN_STRIDE
    from mpcqp.params import GAITS, gait_record
    B, ibm, reps = 64, 4, 5
    names = list(GAITS)
    gait = _dev(np.stack([gait_record(names[b % len(names)]) for b in range(B)]), torch.int32)
    inp = swing_ref.make_inputs(B, 1, seed=33)
    rs = _dev(swing_ref.root_states(inp["quat"], inp["pos"], inp["vel"])[0])
    vb, yr = _dev(inp["v_body"], torch.float64), _dev(inp["yaw_rate"], torch.float64)
    c = {k: _dev(inp[k]) for k in ("thighs", "jac", "u0")}
    c.update({k: _dev(inp[k][0]) for k in ("pos_feet", "foot_pos_base", "foot_vel_base")})
    eng = _engine()

    def buffers():
        return dict(plan=torch.zeros((B, PLAN_STRIDE), dtype=torch.float64, device=DEV),
                    x0=torch.zeros((B, 13), device=DEV), mem=torch.zeros((B, swing_ref.STRIDE), dtype=torch.float64,
                                                                         device=DEV),
                    tau=torch.zeros((B, 12), device=DEV), tick=torch.full((B,), 17, dtype=torch.int32, device=DEV))

    def launch(bf, stream=None):
        eng.plan(0, bf["plan"], bf["x0"], vb, yr, root_states=rs, stream=stream)
        eng.leg_torques(bf["tick"], ibm, vb, yr, gait, c["thighs"], c["pos_feet"], c["foot_pos_base"],
                        c["foot_vel_base"], c["jac"], c["u0"], bf["mem"], bf["tau"], root_states=rs, stream=stream)

    eager, taus = buffers(), []
    for _ in range(reps):
        launch(eager)
        taus.append(eager["tau"].clone())
        eager["tick"] += 1
    torch.cuda.synchronize()
    bf = buffers()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch(bf, stream=s)
    for r in range(reps):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(bf["tau"], taus[r]), r
        bf["tick"] += 1
    assert torch.equal(bf["mem"], eager["mem"]) and torch.equal(bf["plan"], eager["plan"])
    assert len({t.cpu().numpy().tobytes() for t in taus}) == reps     # the ticks did advance the result

"""GPU: mpcqp_leg_torques where tests/test_gpu_swing.py cannot see a mistake -- full
non-symmetric PD gains, thigh z and commanded z velocity, every constant off its default,
the second half of the curve at the batch tails, the integer edges of the swing decision,
the edges of the generator state, non-finite inputs and the mpcqp_set_swing contract.

Tolerance (norm-wise per robot, max|a - a_ref| / max|a_ref|), by the rule of
tests/test_gpu_swing.py.  Measured on the CPU (tests/test_swing.py prints them):
                                               swing.npz    swing_edges.npz
    tests/swing_ref.py                         1.152e-07    1.123e-07  (tau; targets 2.7e-08, final 1.2e-08)
    csrc/mpcqp_swing_leg.h compiled with g++   1.152e-07    1.123e-07  (the same figures)
Four times the larger figure against swing_edges.npz is 4.49e-07, below the project's
BOUND = 4.61e-07, so the device bound stays BOUND, against the fixture and against
swing_ref alike.

Masks, finished flags, `armed`, stance entries of tau and everything a launch must not
touch have no tolerance.  The bound on swing_state in test_tick_and_record_edges is derived
there.  tests/test_swing.py::test_edge_inputs_move_every_robots_torques shows on the CPU
that each thing tested here against swing_ref moves every robot's torques by at least
100 x BOUND when it is wrong.

Measured on the MI355X (printed by the tests):
    swing_edges.npz, split / root / rot alike:  tau 1.12e-07, swing_state 1.99e-08, pos_target 3.87e-08,
                                                vel_target 5.32e-08, foothold 1.18e-08, remaining time and
                                                lift-off position exact
    swing_ref, B = 1 / 63 / 64 / 65 (split and root alike), the worst of them:
                                                tau 5.91e-08, swing_state 2.98e-08, pos_target 5.83e-08,
                                                vel_target 5.69e-08, swing_mem 2.2e-16
"""
import numpy as np
import pytest

# torch first: see tests/test_gpu_swing.py
torch = pytest.importorskip("torch")

import swing_ref  # noqa: E402
from swing_ref import ARMED, EDGE_CONSTS, EDGE_IBM, EDGE_KD, EDGE_KP, FINAL, INIT, REMAIN, STRIDE, norm_err, run_ref  # noqa: E402
from test_gpu_swing import BOUND, DEV, _dev, _engine, assert_matches_ref, fixture_sequence_checks, run_device  # noqa: E402

pytestmark = pytest.mark.gpu

EDGE_KW = dict(EDGE_CONSTS, kp=EDGE_KP, kd=EDGE_KD)                  # SwingRef's keywords
EDGE_SWING = {k: EDGE_CONSTS[k] for k in ("swing_height", "touchdown_z", "vel_gain")}
OUTS = ("tau", "swing_state", "pos_target", "vel_target", "mem")
TROT = (10, (0, 5, 5, 0), (5, 5, 5, 5))
PACE = (10, (5, 0, 5, 0), (5, 5, 5, 5))


def _edge_engine(kp=EDGE_KP, kd=EDGE_KD, **consts):
    c = dict(EDGE_CONSTS, **consts)
    eng = _engine(kp, kd, swing_height=c["swing_height"], touchdown_z=c["touchdown_z"], vel_gain=c["vel_gain"])
    eng.set_planner(dt_control=c["dt_control"], gravity=c["gravity"])
    return eng


def _records(recs, B):
    return np.array([[g[0], *g[1], *g[2]] for g in (recs[b % len(recs)] for b in range(B))], np.int32)


_one_tick = swing_ref.edge_one_tick


def _launch(eng, case, **kw):
    inp, gait, ticks, mem0 = case
    return run_device(eng, inp, gait, ticks, EDGE_IBM, **dict(dict(mem0=mem0), **kw))


def _ref(case, **kw):
    inp, gait, ticks, mem0 = case
    return run_ref(inp, gait, ticks, EDGE_IBM, mem0=mem0, **dict(EDGE_KW, **kw))


def _report(tag, out, ref, B):
    worst = {k: max(norm_err(out[k][:, b], ref[k][:, b]) for b in range(B))
             for k in ("tau", "swing_state", "pos_target", "vel_target")}
    worst["mem"] = max(norm_err(out["mem"][b], ref["mem"][b]) for b in range(B))
    print(f"\n{tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---- 1. the second recorded run of the reference ---------------------------------------------

@pytest.fixture(scope="module")
def fxe():
    return swing_ref.load_fixture("swing_edges.npz")


@pytest.fixture(scope="module")
def fxe_inputs(fxe):
    return swing_ref.fixture_inputs(fxe)


@pytest.mark.parametrize("layout", ["split", "root", "rot"])
def test_edges_fixture_sequence(fxe, fxe_inputs, layout):
    """tests/golden/swing_edges.npz -- the reference's own objects with full non-symmetric gains
    in two groups, thigh z, a commanded z velocity and gravity, dt_control and swing_height off
    their defaults -- with the assertions of test_fixture_sequence."""
    eng = _engine()
    eng.set_planner(dt_control=float(fxe["dt_control"]), gravity=float(fxe["gravity"]))
    swing = dict(swing_height=float(fxe["swing_height"]), touchdown_z=float(fxe["touchdown_z"]),
                 vel_gain=float(fxe["vel_gain"]))
    kp, kd = fxe["kp"], fxe["kd"]
    assert (kp[:3] == kp[0]).all() and (kp[3:] == kp[3]).all() and (kd[:3] == kd[0]).all() and (kd[3:] == kd[3]).all()
    groups = [(slice(0, 3), kp[0], kd[0]), (slice(3, 6), kp[3], kd[3])]
    fixture_sequence_checks(fxe, fxe_inputs, layout, eng, groups, swing=swing)


# ---- 2. everything off its default at once, at the batch tails -------------------------------

@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_everything_off_default_at_the_tail(B):
    """B around the 64 robots of a workgroup against swing_ref on swing_ref.edge_case: full
    gains, all five constants off their defaults, thigh z, commanded z velocity, and every
    tick of one whole swing of every leg with the ticks either side -- the curve's second
    segment, the finishing tick and the re-arm are all reached by every robot; nothing is
    written past row B."""
    inp, gait, ticks = swing_ref.edge_case(B)
    ref = run_ref(inp, gait, ticks, EDGE_IBM, **EDGE_KW)
    t1 = np.float32(EDGE_CONSTS["dt_control"] * EDGE_IBM * (gait[:, 0] - gait[:, 5]) / 2.0).astype(np.float64)
    assert (ref["cur"] >= t1[None, :, None]).any(axis=(0, 2)).all()            # mid -> final
    fin = np.stack([swing_ref.swing_state(tk, EDGE_IBM, gait)[1] for tk in ticks])      # [T,B,4], the integers'
    assert fin.any(axis=0).all()                                               # every leg finishes
    first = fin.argmax(axis=0)                                                 # [B,4]: its first finishing call
    again = np.array([[ref["swing"][first[b, l] + 1:, b, l].any() for l in range(4)] for b in range(B)])
    assert again.any(axis=1).all()                                             # and every robot re-arms a leg
    for layout in ("split", "root"):
        out = run_device(_edge_engine(), inp, gait, ticks, EDGE_IBM, layout=layout, pad=3, sentinel=-77.0)
        _report(f"B={B} {layout}", out, ref, B)
        assert_matches_ref(out, ref, B, tag=(B, layout))
        for k in ("tau", "swing_state", "pos_target", "vel_target"):
            assert (out[k][:, B:] == -77.0).all(), k
        assert (out["mem"][B:] == -77.0).all()


# ---- 3. tick and record edges, known answers ---------------------------------------------------

@pytest.mark.parametrize("ibm", [1, 20, 2 ** 20])
def test_tick_and_record_edges(ibm):
    """swing_ref.decision_edges in one launch, each robot with its own (tick, record): ticks
    -2^31, -1, 0, span - 1, span, 2^31 - 1; period 1, duration 0, a stance that fills the period
    on one leg only, an offset that wraps, negative offsets, period 0 and -3; ibm = 2^20 with
    period 2^11 makes span = 2^31.  The expected decisions are Python integers
    (swing_ref.decide_exact; a few of them by hand below).  Mask, finished flag and `armed`
    exact.  For span <= 2^20, |swing_state - cs / nsw| <= 2^-24 / (1 - dur / period): the only
    inexact step is the float32 phase, half an ulp <= 2^-25, divided by the swing fraction
    1 - dur / period; doubled (which also covers the float32 rounding of the output, <= 2^-25).
    For larger spans decisions only, and swing_state finite and > 0 on a swinging leg.  A leg
    not in swing -- malformed, never swinging, or merely in stance on this tick -- has
    swing_state 0, targets 0, tau bitwise mpcqp_stance_torques' and its 64 bytes of swing_mem
    bitwise the non-zero pattern they held."""
    rows = swing_ref.decision_edges()[ibm]
    B = len(rows)
    ticks = np.array([[r[0] for r in rows]], np.int64)
    gait = np.stack([r[1] for r in rows])
    inp = swing_ref.make_inputs(B, 1, seed=400, **swing_ref.EDGE_RANGES)
    mem0 = (3.0 + 0.125 * np.arange(B * STRIDE)).reshape(B, STRIDE)            # armed != 0: a swing continues
    eng = _edge_engine()
    out = run_device(eng, inp, gait, ticks, ibm, mem0=mem0, pad=3)
    stance_tau = torch.full((B, 12), 5.0, dtype=torch.float32, device=DEV)
    eng.stance_torques(_dev(inp["jac"]), torch.ones((B, 4), device=DEV), _dev(inp["u0"]), stance_tau)
    torch.cuda.synchronize()
    stance_tau = stance_tau.cpu().numpy().reshape(B, 4, 3)
    tau, ss = out["tau"][0, :B].reshape(B, 4, 3), out["swing_state"][0, :B]
    mem, m0 = out["mem"][:B].reshape(B, 4, 8), mem0.reshape(B, 4, 8)
    seen = dict(swing=0, finished=0, stance=0, never=0)
    for b, (tick, rec) in enumerate(rows):
        for l in range(4):
            sw, fin, cs, nsw = swing_ref.decide_exact(tick, ibm, rec, l)
            tag = (ibm, tick, rec.tolist(), l)
            assert (ss[b, l] > 0) == sw, tag
            if not sw:
                seen["never" if rec[0] <= 0 or nsw <= 0 else "stance"] += 1
                assert ss[b, l] == 0 and (out["pos_target"][0, b, l] == 0).all() and (out["vel_target"][0, b, l] == 0).all()
                assert _same_bits(tau[b, l], stance_tau[b, l]), tag
                assert _same_bits(mem[b, l], m0[b, l]), tag
                continue
            seen["finished" if fin else "swing"] += 1
            assert mem[b, l, ARMED] == (0.0 if fin else 1.0), tag
            assert np.isfinite(tau[b, l]).all() and np.isfinite(mem[b, l]).all(), tag
            assert mem[b, l, REMAIN] == m0[b, l, REMAIN] - EDGE_CONSTS["dt_control"], tag
            assert np.array_equal(mem[b, l, INIT], m0[b, l, INIT]), tag       # an armed leg keeps its lift-off
            if ibm * int(rec[0]) <= 2 ** 20:
                assert abs(float(ss[b, l]) - cs / nsw) <= 2.0 ** -24 / (1.0 - int(rec[5 + l]) / int(rec[0])), tag
            else:
                assert np.isfinite(ss[b, l]) and ss[b, l] > 0, tag
    assert all(v > 0 for v in seen.values()), seen
    for k in ("tau", "swing_state", "pos_target", "vel_target"):
        assert (out[k][:, B:] == -77.0).all(), k
    # some of the table by hand: TROTTING10, 20 iterations per MPC step, span 200
    rec = np.array([TROT[0], *TROT[1], *TROT[2]])
    assert swing_ref.decide_exact(-1, 20, rec, 0) == (True, False, 99, 100)
    assert swing_ref.decide_exact(-2 ** 31, 20, rec, 0) == (True, False, 52, 100)
    assert swing_ref.decide_exact(2 ** 31 - 1, 20, rec, 1) == (True, False, 47, 100)
    assert swing_ref.decide_exact(100, 20, rec, 1) == (True, True, 100, 100)
    assert swing_ref.decide_exact(2 ** 31 - 1, 2 ** 20, (2048, 0, 0, 0, 0, 1024, 0, 0, 0), 0) == (True, False, 2 ** 30 - 1, 2 ** 30)


# ---- 4. edges of the generator state -------------------------------------------------------------

def test_armed_minus_zero_and_armed_two():
    """armed = -0.0 is a first swing (the lift-off position is latched, the remaining time
    starts at the swing time, whatever the slots held); armed = 2.0 -- anything but zero --
    continues the swing it finds.  B = 3: zeros, -0.0 over garbage, 2.0 over a swing half done;
    three ticks of TROTTING10 with legs 1 and 2 in swing, against swing_ref."""
    B, ibm = 3, EDGE_IBM
    inp = swing_ref.make_inputs(B, 3, seed=410, **swing_ref.EDGE_RANGES)
    gait, ticks = _records([TROT], B), np.tile(np.array([5, 6, 7])[:, None], (1, B))
    t_swing = EDGE_CONSTS["dt_control"] * ibm * 5
    mem0 = np.zeros((B, 4, 8))
    mem0[1, :, ARMED], mem0[1, :, REMAIN], mem0[1, :, INIT], mem0[1, :, FINAL] = -0.0, 9.0, 5.0, -6.0
    lift = inp["pos_feet"][0, 2].astype(np.float64) + 0.01
    mem0[2, :, ARMED], mem0[2, :, REMAIN], mem0[2, :, INIT] = 2.0, 0.5 * t_swing, lift
    assert np.signbit(mem0[1, :, ARMED]).all()
    out = run_device(_edge_engine(), inp, gait, ticks, ibm, mem0=mem0.reshape(B, STRIDE))
    ref = run_ref(inp, gait, ticks, ibm, mem0=mem0, **EDGE_KW)
    assert np.array_equal(ref["swing"][0], np.tile([False, True, True, False], (B, 1)))
    assert_matches_ref(out, ref, B)
    m = out["mem"].reshape(B, 4, 8)
    sw = [1, 2]
    assert np.array_equal(m[1][sw][:, INIT], inp["pos_feet"][0, 1][sw].astype(np.float64))     # latched on tick 5
    assert np.array_equal(m[2][sw][:, INIT], lift[sw])                                          # kept
    dt = EDGE_CONSTS["dt_control"]
    assert (m[1][sw][:, REMAIN] == (t_swing - dt) - dt).all() and (m[2][sw][:, REMAIN] == ((0.5 * t_swing - dt) - dt) - dt).all()
    assert (m[:, sw, ARMED] == 1.0).all()
    assert _same_bits(m[:, [0, 3]], mem0[:, [0, 3]])                                            # stance legs: untouched


def test_skipped_finishing_tick():
    """The call at cs == nsw never comes (ticks with tick % 10 == 0 are left out, which are the
    finishing ticks of every leg of TROTTING10 and PACING10 at 2 iterations per MPC step): the
    leg stays armed into its next swing, the countdown goes on below zero, the curve clamps at
    its end -- the foothold, at rest in the world, so vel_target = R^T (0 - vel)."""
    B, ibm = 2, EDGE_IBM
    t_seq = [t for t in range(1, 46) if t % 10 != 0]
    T = len(t_seq)
    inp = swing_ref.make_inputs(B, T, seed=420, **swing_ref.EDGE_RANGES)
    gait, ticks = _records([TROT, PACE], B), np.tile(np.array(t_seq)[:, None], (1, B))
    out = run_device(_edge_engine(), inp, gait, ticks, ibm)
    ref = run_ref(inp, gait, ticks, ibm, **EDGE_KW)
    t2 = float(np.float32(EDGE_CONSTS["dt_control"] * ibm * 5))
    assert not (ref["swing_state"] >= 1.0).any()
    late = ref["cur"] > t2                                   # [T,B,4]: the second swing of a leg, still counting down
    assert late.any(axis=0).all()
    assert (ref["mem"].reshape(B, 4, 8)[..., REMAIN] < 0).all() and (ref["mem"].reshape(B, 4, 8)[..., ARMED] == 1.0).all()
    assert_matches_ref(out, ref, B)
    m = out["mem"].reshape(B, 4, 8)
    assert (m[..., ARMED] == 1.0).all() and (m[..., REMAIN] < 0).all()
    want = np.einsum("tbcr,tbc->tbr", inp["rot"].astype(np.float64), -inp["vel"].astype(np.float64))   # R^T (-vel)
    want = np.broadcast_to(want[:, :, None, :], (T, B, 4, 3))
    for b in range(B):
        assert norm_err(out["vel_target"][:, b][late[:, b]], want[:, b][late[:, b]]) <= BOUND, b
    # and the foot is held at the foothold: pos_target = R^T (final - pos)
    fin = ref["mem"].reshape(B, 4, 8)[..., FINAL]
    p = np.einsum("bcr,blc->blr", inp["rot"][-1].astype(np.float64), fin - inp["pos"][-1].astype(np.float64)[:, None])
    for b in range(B):
        assert norm_err(out["pos_target"][-1, b][late[-1, b]], p[b][late[-1, b]]) <= BOUND, b
    assert late[-1].any(axis=1).all()


def test_dt_control_zero():
    """mpcqp_set_planner allows dt_control = 0: the swing time is 0, both segments of the curve
    have no length, and every output is finite and swing_ref's."""
    B = 5
    inp, gait, ticks = swing_ref.edge_case(B)
    out = run_device(_edge_engine(dt_control=0.0), inp, gait, ticks, EDGE_IBM)
    ref = run_ref(inp, gait, ticks, EDGE_IBM, **dict(EDGE_KW, dt_control=0.0))
    assert ref["swing"].any(axis=0).all() and all(np.isfinite(ref[k]).all() for k in ("tau", "pos_target", "vel_target"))
    assert all(np.isfinite(out[k]).all() for k in OUTS)
    assert (out["mem"].reshape(B, 4, 8)[..., REMAIN] == 0).all()
    assert_matches_ref(out, ref, B)


# ---- 5. a non-finite input stays with its robot ----------------------------------------------------

BAD = 63


def _isolation_case():
    """B = 65 on tick 5: robot 63 (TROTTING10) has legs 1 and 2 in swing, 0 and 3 in stance."""
    case = _one_tick(65, 5, seed=430)
    assert case[1][BAD].tolist() == [TROT[0], *TROT[1], *TROT[2]]
    return case


def _poisoned(inp, key, index):
    a = inp[key].copy()
    a[index] = np.nan
    return dict(inp, **{key: a})


@pytest.mark.parametrize("layout", ["split", "root"])
def test_nonfinite_input_stays_with_its_robot(layout):
    """A NaN in robot 63's pos, vel, vel_body_des, yaw_rate_des or one swing leg's thighs, B = 65
    (robot 63 is the last of the first workgroup, 64 the only one of the second): every other
    robot -- 62 and 64 by name -- is bitwise the clean launch, so are robot 63's stance legs
    (the stance branch reads none of these), and the swing legs the value feeds are NaN."""
    case = _isolation_case()
    eng = _edge_engine()
    clean = _launch(eng, case, layout=layout)
    ref = _ref(case)
    assert (ref["cur"][0, BAD, 1:3] >= 0.0125).all()            # the foothold feeds the targets
    assert (clean["swing_state"][0, BAD] > 0).tolist() == [False, True, True, False]
    assert all(np.isfinite(clean[k]).all() for k in OUTS)
    per_leg = lambda o, k: (o[k][0] if k != "mem" else o[k]).reshape(65, 4, -1)
    others = [b for b in range(65) if b != BAD]
    cases = [("pos", (0, BAD, 1), [1, 2]), ("vel", (0, BAD, 0), [1, 2]), ("v_body", (BAD, 2), [1, 2]),
             ("yaw_rate", (BAD,), [1, 2]), ("thighs", (BAD, 1, 0), [1])]
    for key, index, fed in cases:
        out = _launch(eng, (_poisoned(case[0], key, index),) + case[1:], layout=layout)
        for k in OUTS:
            got, want = per_leg(out, k), per_leg(clean, k)
            assert _same_bits(got[others], want[others]), (key, k)
            assert _same_bits(got[62], want[62]) and _same_bits(got[64], want[64]), (key, k)
            keep = [l for l in range(4) if l not in fed]                 # the stance legs, and a swing leg not fed
            assert _same_bits(got[BAD][keep], want[BAD][keep]), (key, k)
        assert np.isnan(per_leg(out, "tau")[BAD][fed]).all(), key
        assert np.isnan(per_leg(out, "pos_target")[BAD][fed]).all(), key
        assert (per_leg(out, "swing_state")[BAD][fed] > 0).all(), key   # the decision is the integers'


def test_nonfinite_values_nobody_reads_change_nothing():
    """A NaN quaternion when R_base is supplied, and NaN payloads in a stance leg's swing_mem:
    every output of every robot is bitwise the clean launch, and the payloads are still there."""
    case = _isolation_case()
    eng = _edge_engine()
    clean = _launch(eng, case, layout="rot")
    out = _launch(eng, (_poisoned(case[0], "quat", (0, BAD)),) + case[1:], layout="rot")
    for k in OUTS:
        assert _same_bits(out[k], clean[k]), k
    payload = np.array([0x7FF8DEAD0000BEE0 + i for i in range(8)], np.uint64).view(np.float64)
    mem0 = case[3].copy().reshape(65, 4, 8)
    mem0[BAD, 0], mem0[BAD, 3] = payload, payload[::-1]
    out = _launch(eng, case, layout="rot", mem0=mem0.reshape(65, STRIDE))
    for k in OUTS[:-1]:
        assert _same_bits(out[k], clean[k]), k
    m = out["mem"].reshape(65, 4, 8)
    assert _same_bits(m[BAD][[0, 3]], mem0[BAD][[0, 3]])
    m[BAD, [0, 3]] = case[3].reshape(65, 4, 8)[BAD, [0, 3]]
    assert _same_bits(m, clean["mem"].reshape(65, 4, 8))


# ---- 6. the mpcqp_set_swing contract -----------------------------------------------------------------

def test_set_swing_refuses_nonfinite_and_keeps_the_constants():
    """A non-finite swing_height, touchdown_z, vel_gain, Kp entry or Kd entry: MPCQP_ERR_ARG with
    its word in mpcqp_last_error, and the next launch is bitwise a launch under the previous
    constants -- although every other argument of the refused call was finite and different."""
    from mpcqp import _lib
    case = _one_tick(5, 5, seed=440)
    eng = _edge_engine()
    want = _launch(eng, case)
    other_kp, other_kd = np.ascontiguousarray(EDGE_KP.T * 0.5), np.ascontiguousarray(EDGE_KD.T * 2.0)
    good = dict(swing_height=0.2, Kp=other_kp, Kd=other_kd, touchdown_z=0.5, vel_gain=0.4)

    def call(**kw):
        a = dict(good, **kw)
        return eng.lib.mpcqp_set_swing(eng._ctx, a["swing_height"], a["Kp"].ctypes.data, a["Kd"].ctypes.data,
                                       a["touchdown_z"], a["vel_gain"])

    def with_entry(m, i, v):
        m = m.copy()
        m.reshape(-1)[i] = v
        return m

    refused = [dict(swing_height=np.nan), dict(swing_height=np.inf), dict(touchdown_z=np.nan), dict(touchdown_z=-np.inf),
               dict(vel_gain=np.nan), dict(Kp=with_entry(other_kp, 5, np.nan)), dict(Kp=with_entry(other_kp, 8, np.inf)),
               dict(Kd=with_entry(other_kd, 0, np.nan)), dict(Kd=with_entry(other_kd, 7, -np.inf))]
    for kw in refused:
        assert call(**kw) == _lib.ERR_ARG, kw
        assert "non-finite" in eng.lib.mpcqp_last_error(eng._ctx).decode(), kw
        got = _launch(eng, case)
        for k in OUTS:
            assert _same_bits(got[k], want[k]), (kw, k)
    with pytest.raises(_lib.MpcqpError):
        eng.set_swing(swing_height=float("nan"))
    # the same call with every value finite is taken, and changes the result
    assert call() == 0
    got = _launch(eng, case)
    assert not _same_bits(got["tau"], want["tau"])
    ref = _ref(case, swing_height=0.2, kp=other_kp, kd=other_kd, touchdown_z=0.5, vel_gain=0.4)
    assert_matches_ref(got, ref, 5)


def test_set_swing_keeps_absent_gains_and_defaults_absent_scalars():
    """LinearMpc.set_swing: Kp = None / Kd = None keep the matrix in force, an omitted scalar
    returns to its default -- bitwise an engine that was given all of it explicitly."""
    case = _one_tick(5, 5, seed=441)
    a = _edge_engine()
    before = _launch(a, case)
    a.set_swing(swing_height=EDGE_CONSTS["swing_height"])           # gains kept, touchdown_z and vel_gain default
    got = _launch(a, case)
    b = _edge_engine()
    b.set_swing(swing_height=EDGE_CONSTS["swing_height"], Kp=EDGE_KP, Kd=EDGE_KD, touchdown_z=-0.0255, vel_gain=0.03)
    want = _launch(b, case)
    for k in OUTS:
        assert _same_bits(got[k], want[k]), k
    assert not _same_bits(got["tau"], before["tau"])
    ref = _ref(case, touchdown_z=-0.0255, vel_gain=0.03)
    assert_matches_ref(got, ref, 5)
    a.set_swing(Kd=EDGE_KD.T)                                       # Kp kept, every scalar default
    ref = _ref(case, kd=EDGE_KD.T, swing_height=0.1, touchdown_z=-0.0255, vel_gain=0.03)
    assert_matches_ref(_launch(a, case), ref, 5)


def test_set_swing_gain_shapes():
    """A scalar gain is k I, three entries are a diagonal, a 3 x 3 matrix is itself (row-major,
    not transposed): each against swing_ref with that matrix.  Anything else is a ValueError
    and changes nothing."""
    case = _one_tick(5, 5, seed=442)
    eng = _edge_engine()
    given = [(350.0, 350.0 * np.eye(3), 11.0, 11.0 * np.eye(3)),
             ([300.0, 500.0, 700.0], np.diag([300.0, 500.0, 700.0]), (9.0, 14.0, 21.0), np.diag([9.0, 14.0, 21.0])),
             (EDGE_KP.tolist(), EDGE_KP, EDGE_KD.astype(np.float32), EDGE_KD.astype(np.float32).astype(np.float64)),
             (np.asfortranarray(EDGE_KP), EDGE_KP, EDGE_KD.T.copy().T, EDGE_KD)]
    for kp, kp_m, kd, kd_m in given:
        eng.set_swing(Kp=kp, Kd=kd, **EDGE_SWING)
        ref = _ref(case, kp=kp_m, kd=kd_m)
        assert_matches_ref(_launch(eng, case), ref, 5, tag=str(np.shape(kp)))
    want = _launch(eng, case)
    for bad in (np.ones((2, 2)), np.ones(4), np.ones(9), np.ones((3, 3, 1)), np.ones((1, 3, 3)), np.ones((3, 4))):
        with pytest.raises(ValueError):
            eng.set_swing(Kp=bad, **EDGE_SWING)
        with pytest.raises(ValueError):
            eng.set_swing(Kd=bad, **EDGE_SWING)
    got = _launch(eng, case)
    for k in OUTS:
        assert _same_bits(got[k], want[k]), k


def test_controller_passes_full_gains_to_the_kernel():
    """BatchedController(..., swing=dict(Kp=<full matrix>, ...), dt_control, gravity): one
    leg_torques call at B = 5 against swing_ref with the same constants."""
    from mpcqp.controller import BatchedController
    B = 5
    case = _one_tick(B, 5, seed=443)
    inp, gait, ticks, mem0 = case
    ctl = BatchedController(B, horizon=10, robot="aliengo", gait=[swing_ref.EDGE_GAITS[b % 3] for b in range(B)],
                            iterations_between_mpc=EDGE_IBM, dt_control=EDGE_CONSTS["dt_control"],
                            gravity=EDGE_CONSTS["gravity"], swing=dict(Kp=EDGE_KP, Kd=EDGE_KD, **EDGE_SWING))
    assert np.array_equal(ctl.gait.cpu().numpy(), gait)
    ctl.u0.copy_(_dev(inp["u0"]))
    ctl.swing_mem.copy_(_dev(mem0))
    rs = swing_ref.root_states(inp["quat"], inp["pos"], inp["vel"])[0]
    tau = ctl.leg_torques(5, inp["v_body"], inp["yaw_rate"], _dev(inp["thighs"]), _dev(inp["pos_feet"][0]),
                          _dev(inp["foot_pos_base"][0]), _dev(inp["foot_vel_base"][0]), _dev(inp["jac"]),
                          root_states=_dev(rs))
    torch.cuda.synchronize()
    out = dict(tau=tau.cpu().numpy()[None], swing_state=ctl.swing_state.cpu().numpy()[None],
               pos_target=ctl.pos_target.cpu().numpy()[None], vel_target=ctl.vel_target.cpu().numpy()[None],
               mem=ctl.swing_mem.cpu().numpy())
    ref = _ref(case)
    assert ref["swing"].any(axis=(0, 2)).all() and not ref["swing"].all()
    assert_matches_ref(out, ref, B)

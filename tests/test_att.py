"""CPU: the orientation filter and the contact trust (mpcqp_attitude) without a GPU -- the ABI
surface, the float64 restatement tests/att_ref.py against known answers (the reference has
no code for either, so att_ref is the oracle of tests/test_gpu_att.py), and the per-robot
header csrc/mpcqp_attitude_robot.h compiled with g++ and driven through ctypes against it.

Measured here (printed by the tests):
  known answers on att_ref: (a) tilt convergence |R^T e_z - a / |a|| 2.8e-16; (b) gyro only,
    q against the closed-form exponential 1.7e-16, bitwise equal with kappa_ref = 0; (c) first
    tick |R^T e_z - a / |a|| 2.2e-16 on eight named directions, 5.4e-16 over 200 random
    directions and magnitudes (see the test); (d) bias 3.4e-16, tilt 1.7e-17; (e) trust against
    the closed form 2.8e-16.
  the host-compiled header against att_ref over make_trajectory(8, 400, seed=7): the record
    d = 5.6e-16 norm-wise (the quaternion up to sign), largest over ticks and robots
    (att_ref.D_Q), quat 3.1e-08 at its float32 store, gyro_out bitwise the gyro (b = 0), trust
    bitwise equal; with the bias estimate on (BIAS_ON, 100 ticks) record 2.5e-16, quat 3.0e-08,
    gyro_out 5.8e-08.  d stays at a few ulps over 400 ticks, well inside the 4 T eps argued
    for it: the two forms round differently in a few operations per tick, the differences are
    as often up as down, and the renormalisation of every tick removes their component along q.
  tilt of the estimate against the generator's true orientation after 400 ticks: 8.7e-03 rad.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import att_edge_checks
import att_ref
from helpers import _declared, host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpcqp.h")
NEW_SYMBOLS = {"mpcqp_attitude", "mpcqp_set_attitude"}
KNOWN = 1e-12
F32_FLOOR = 2.4e-7      # two float32 ulps norm-wise, the project's floor for a float32 store
EPS = 2.0 ** -52
SENTINEL = -77
BIAS_ON = dict(kappa_ref=2.0, bias_gain=0.5)

SHIM = r'''
#include "mpcqp_attitude_robot.h"
// a launch of mpcqp_attitude_kernel, robot after robot; c: dt, gravity, kappa_ref, bias_gain,
// trust_window, touch_threshold
extern "C" void launch(const double* c, int B, const float* gyro, const float* accel, const int32_t* tick, int ibm,
                       const int32_t* gait, const float* touch, double* st, float* quat, float* gyro_out,
                       float* trust, int32_t* status) {
  const AttParams ap{c[0], c[1], c[2], c[3], c[4], c[5]};
  for (int b = 0; b < B; ++b)
    att_robot(ap, (size_t)b, gyro, accel, tick, ibm, gait, touch, st, quat, gyro_out, trust, status);
}
extern "C" double trust(int tick, int ibm, int period, int off, int dur, double window) {
  return att_trust(tick, ibm, period, off, dur, window);
}
extern "C" int decide(int tick, int ibm, int period, int off, int dur) {
  double v;
  return swing_decide(tick, ibm, period, off, dur, &v);
}
extern "C" int stride(void) { return ATT_STRIDE; }
'''


def test_header_declares_the_attitude_entry_points_and_binding_agrees():
    from mpcqp import _lib
    assert NEW_SYMBOLS <= _declared()
    assert _declared() == set(_lib.EXPORTED_SYMBOLS)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.mpcqp_abi_version() == 6     # additive: the ABI version stays


def test_record_constants_match_binding(robot):
    from mpcqp import _lib
    src = open(HEADER).read()
    assert int(re.search(r"#define MPCQP_ATT_STRIDE (\d+)", src).group(1)) == _lib.ATT_STRIDE == att_ref.STRIDE == 8
    assert robot.stride() == 8 and att_ref.STATUS_NONFINITE == _lib.STATUS_NONFINITE
    assert "mpcqp_attitude computes both" in src       # the estimator's comment points at the new call


def test_null_ctx_is_an_error_code():
    from mpcqp import _lib
    lib = _lib.load()
    assert lib.mpcqp_attitude(None, 1, 0, None, None, None, 20, *([None] * 8)) == -1
    assert lib.mpcqp_set_attitude(None, *([1.0] * 6)) == -1


# ---- known answers on att_ref

def _run_known(k):
    st = k["state"]
    for _ in range(k["ticks"]):
        st, ok = att_ref.tick_step(st, k["gyro"], k["accel"], k["constants"])
    return st


def test_known_answer_tilt_convergence():
    """(a)"""
    k = att_ref.known_tilt()
    st = _run_known(k)
    a = k["accel"][0].astype(np.float64)
    err = np.abs(att_ref.up(st[:, att_ref.Q])[0] - a / np.linalg.norm(a)).max()
    print(f"\n(a) tilt convergence: {err:.2e}")
    assert err < KNOWN and abs(np.linalg.norm(st[0, att_ref.Q]) - 1) < KNOWN


def test_known_answer_gyro_only():
    """(b)"""
    k = att_ref.known_gyro_only()
    assert att_ref.gate(k["accel"])[0] == 0.0
    st = _run_known(k)
    err = att_ref.quat_err(st[0, att_ref.Q], k["answer"])
    print(f"\n(b) gyro only: {err:.2e}")
    assert err < KNOWN
    off = _run_known(dict(k, constants=dict(k["constants"], kappa_ref=0.0)))
    assert np.array_equal(st, off)                      # gamma = 0: the accelerometer has no say


def test_known_answer_first_tick():
    """(c): R^T e_z = a / |a| to 4e-16 on the tilt of (a), the axes and three everyday
    readings.  Over 200 random directions and magnitudes the float64 evaluation of the formula
    itself reaches 5.4e-16 (14 of the 200 pass 4e-16; the exact q rounded to float64 gives
    3.3e-16 through the same check), so those are held to what its rounding explains, with
    u = 2^-53: a / |a| carries 1.25 u per component, the normalised q 3 u, a product of two of
    its components doubled 7 u of a value below 1, the check's own a / |a| 1.25 u: 9 u = 1e-15."""
    named = np.float32([att_ref.known_tilt()["accel"][0], [0, 0, 9.81], [9.81, 0, 0], [0, 9.81, 0], [0, -9.81, 0],
                        [3, -4, 12], [0.5, -0.3, 9.7], [-2.0, 1.5, 8.0]])
    rng = np.random.default_rng(3)
    rand = rng.standard_normal((200, 3)).astype(np.float32) * rng.uniform(0.1, 30, (200, 1)).astype(np.float32)
    a = np.concatenate([named, rand])
    st, ok = att_ref.tick_step(np.zeros((208, 8)), np.ones((208, 3), np.float32), a)
    a64 = a.astype(np.float64)
    errs = np.abs(att_ref.up(st[:, att_ref.Q]) - a64 / np.linalg.norm(a64, axis=1, keepdims=True)).max(1)
    print(f"\n(c) first tick: named {errs[:8].max():.2e}, random {errs[8:].max():.2e}")
    assert errs[:8].max() <= 4e-16 and errs[8:].max() <= 9 * 2.0 ** -53 and ok.all()
    assert (st[:, 3] == 0).all() and (st[:, att_ref.INIT] == 1).all() and (st[:, att_ref.BIAS] == 0).all()
    st0 = st
    special = np.float32([[0, 0, 0], [0, 0, -9.81]])
    st, _ = att_ref.tick_step(np.zeros((2, 8)), np.zeros((2, 3), np.float32), special)
    assert st[:, :5].tolist() == [[1, 0, 0, 0, 1], [0, 1, 0, 0, 1]]
    # no integration on the first tick: the gyro has no say
    assert np.array_equal(att_ref.tick_step(np.zeros((208, 8)), np.zeros((208, 3), np.float32), a)[0], st0)


def test_known_answer_bias():
    """(d)"""
    k = att_ref.known_bias()
    st = _run_known(k)
    eb = np.abs(st[0, att_ref.BIAS] - k["answer"]).max()
    tilt = np.abs(att_ref.up(st[:, att_ref.Q])[0] - [0, 0, 1]).max()
    print(f"\n(d) bias: {eb:.2e}, tilt {tilt:.2e}")
    assert eb < 1e-9 and tilt < 1e-9


def test_known_answer_trust():
    """(e)"""
    c = np.arange(400)
    tr = att_ref.gait_trust(c, 20, att_ref.gait_records([att_ref.TROTTING10] * 400), 0.2)[:, 0]
    cm = c % 200
    want = np.where((cm >= 1) & (cm <= 100), np.minimum(1.0, np.minimum((cm - 0.5) / 20, (100.5 - cm) / 20)), 0.0)
    err = np.abs(tr - want).max()
    print(f"\n(e) trust: {err:.2e}")
    assert err < KNOWN and (tr[cm == 0] == 0).all() and (tr[(cm >= 101)] == 0).all() and (tr[(cm >= 1) & (cm <= 100)] > 0).all()
    assert (att_ref.gait_trust(c, 20, att_ref.gait_records([att_ref.STANDING] * 400), 0.2) == 1).all()
    hard = att_ref.gait_trust(c, 20, att_ref.gait_records([att_ref.TROTTING10] * 400), 0.0)
    assert set(np.unique(hard)) == {0.0, 1.0} and np.array_equal(hard[:, 0] > 0, tr > 0)


def test_touch_gates_the_trust():
    traj = att_ref.make_trajectory(6, 3, seed=1)
    inp = traj[0]
    touch = inp["touch"].astype(np.float64)
    _, both = att_ref.attitude_step(np.zeros((6, 8)), inp)
    _, gait = att_ref.attitude_step(np.zeros((6, 8)), att_ref.select(inp, ("tick", "gait", "ibm")))
    _, only = att_ref.attitude_step(np.zeros((6, 8)), att_ref.select(inp, ("touch",)))
    _, none = att_ref.attitude_step(np.zeros((6, 8)), att_ref.select(inp, ()))
    assert np.array_equal(only["trust"], (touch > 0).astype(float)) and none["trust"] is None
    assert np.array_equal(both["trust"], np.where(touch > 0, gait["trust"], 0.0))
    _, high = att_ref.attitude_step(np.zeros((6, 8)), att_ref.select(inp, ("touch",)), dict(touch_threshold=0.5))
    assert np.array_equal(high["trust"], (touch > 0.5).astype(float)) and not np.array_equal(high["trust"], only["trust"])


@pytest.fixture(scope="module")
def oracle():
    traj = att_ref.make_trajectory(8, 400, seed=7)
    return traj, *att_ref.run(traj)


def test_trajectory_covers_the_cases(oracle):
    traj, states, outs = oracle
    gamma = np.stack([att_ref.gate(t["accel"]) for t in traj])
    assert (gamma == 0).any() and ((gamma > 0) & (gamma < 1)).any()
    tr = np.stack([att_ref.attitude_step(np.zeros((8, 8)), att_ref.select(t, ("tick", "gait", "ibm")))[1]["trust"]
                   for t in traj])
    assert (tr == 0).any() and ((tr > 0) & (tr < 1)).any() and (tr == 1).any()
    g = traj[0]["gait"]
    never = g[:, 5:9] >= g[:, :1]
    assert never.any() and (tr[:, never] == 1).all()                       # a leg that never swings
    assert ((g[:, 1:5] + g[:, 5:9]) > g[:, :1]).any() and not never.all()  # a swing offset that wraps
    assert {t["ibm"] for t in traj} == {1, 20}
    touch = np.stack([t["touch"] for t in traj])
    assert (touch == 0).any() and (touch < 0).any() and ((touch > 0) & (touch < 1)).any() and (touch == 1).any()
    assert all(t[k].dtype == np.float32 for t in traj[:2] for k in ("gyro", "accel", "touch"))
    # the filter follows the true tilt: the generator's sensors are those of its orientation
    tilt = max(np.abs(att_ref.up(states[-1][:, att_ref.Q]) - att_ref.up(traj[-1]["truth"])).max(), 0.0)
    print(f"\ntilt of the estimate against the truth after 400 ticks: {tilt:.2e}")
    assert tilt < 0.02      # the gyro bias (0.02 rad/s) over 0.4 s, the sway, the noise


# ---- the header on the host

@pytest.fixture(scope="module")
def robot():
    lib = host_build(SHIM, name="att")
    lib.trust.restype = ctypes.c_double
    lib.trust.argtypes = [ctypes.c_int] * 5 + [ctypes.c_double]
    lib.launch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                           ctypes.c_int] + [ctypes.c_void_p] * 7
    lib.launch.restype = None
    return lib


def host_launch(lib, state, inp, constants=None, pad=2, skip=()):
    """A launch on the host, on `state` [B + pad, STRIDE] in place; the outputs come back with
    their `pad` sentinel rows."""
    B = state.shape[0] - pad
    c = dict(att_ref.DEFAULTS, **(constants or {}))
    cv = np.array([c[k] for k in ("dt", "gravity", "kappa_ref", "bias_gain", "trust_window", "touch_threshold")])
    out = dict(quat=np.full((B + pad, 4), SENTINEL, np.float32), gyro_out=np.full((B + pad, 3), SENTINEL, np.float32),
               trust=np.full((B + pad, 4), SENTINEL, np.float32), status=np.full(B + pad, SENTINEL, np.int32))
    if "gait" not in inp and "touch" not in inp:
        skip = tuple(skip) + ("trust",)
    ptr = lambda a: None if a is None else a.ctypes.data
    keep = {k: (np.ascontiguousarray(inp[k]) if k in inp else None) for k in ("gyro", "accel", "tick", "gait", "touch")}
    lib.launch(ptr(cv), B, ptr(keep["gyro"]), ptr(keep["accel"]), ptr(keep["tick"]), int(inp.get("ibm", 0)),
               ptr(keep["gait"]), ptr(keep["touch"]), ptr(state), *(None if k in skip else ptr(v) for k, v in out.items()))
    return out


def test_header_follows_the_restatement(robot, oracle):
    """The record against att_ref over 8 robots x 400 ticks: d, recorded as att_ref.D_Q.  The
    bound asserted is what rounding explains: the two forms round differently in a handful of
    operations per tick (the quaternion product, the normalisation, one ulp of sin / cos), a
    few eps; the correction contracts pitch and roll by kappa dt = 1e-4 per tick, which is
    nothing over 400 ticks, and yaw not at all, so the differences add up over the T ticks at
    worst: 4 T eps = 3.6e-13."""
    traj, states, outs = oracle
    B, T = 8, len(traj)
    st = np.full((B + 2, 8), float(SENTINEL))
    st[:B] = 0.0
    worst = dict(record=0.0, quat=0.0, gyro_out=0.0)
    for i in range(T):
        o = host_launch(robot, st, traj[i])
        assert (o["status"][:B] == 0).all() and (st[:B, 4] == 1).all()
        assert (st[B:] == SENTINEL).all() and all((v[B:] == SENTINEL).all() for v in o.values())
        assert np.array_equal(o["trust"][:B], outs[i]["trust"].astype(np.float32))          # bitwise
        for b in range(B):
            worst["record"] = max(worst["record"], att_ref.record_err(st[b], states[i + 1][b]))
            worst["quat"] = max(worst["quat"], att_ref.quat_err(o["quat"][b], outs[i]["quat"][b]))
            worst["gyro_out"] = max(worst["gyro_out"], att_ref.norm_err(o["gyro_out"][b], outs[i]["gyro_out"][b]))
    print("\nheader on the host against att_ref, 8 robots x 400 ticks: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["record"] < 4 * T * EPS
    assert worst["record"] <= 4 * att_ref.D_Q            # the recorded figure still describes it
    assert worst["quat"] <= F32_FLOOR and worst["gyro_out"] <= F32_FLOOR


def test_header_follows_the_restatement_with_a_bias_estimate(robot, oracle):
    """The same with the bias estimate on and a stronger correction (BIAS_ON), 100 ticks: the
    bias words of the record and gyro_out = w_b - b take part."""
    traj = oracle[0][:100]
    states, outs = att_ref.run(traj, BIAS_ON)
    st = np.zeros((10, 8))
    worst = dict(record=0.0, quat=0.0, gyro_out=0.0)
    for i, inp in enumerate(traj):
        o = host_launch(robot, st, inp, BIAS_ON)
        for b in range(8):
            worst["record"] = max(worst["record"], att_ref.record_err(st[b], states[i + 1][b]))
            worst["quat"] = max(worst["quat"], att_ref.quat_err(o["quat"][b], outs[i]["quat"][b]))
            worst["gyro_out"] = max(worst["gyro_out"], att_ref.norm_err(o["gyro_out"][b], outs[i]["gyro_out"][b]))
    print("\nwith a bias estimate, 8 robots x 100 ticks: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert np.abs(st[:8, 5:8]).min() > 0 and not np.array_equal(o["gyro_out"][:8], inp["gyro"])
    assert worst["record"] <= 4 * att_ref.D_Q and worst["quat"] <= F32_FLOOR and worst["gyro_out"] <= F32_FLOOR


@pytest.mark.parametrize("keys", [("tick", "gait", "ibm"), ("touch",), ()])
def test_header_with_inputs_and_outputs_absent(robot, oracle, keys):
    """Without the touch sensor, without the gait, without both (then no trust); each nullable
    output absent in turn is not written."""
    traj = oracle[0]
    states, outs = att_ref.run(traj[:12], keys=keys)
    for skip in ((), ("quat",), ("gyro_out",), ("trust",), ("status",)):
        st = np.zeros((10, 8))
        for i in range(12):
            o = host_launch(robot, st, att_ref.select(traj[i], keys), skip=skip)
            for k in ("quat", "gyro_out", "trust"):
                if k in skip or outs[i][k] is None:
                    assert (o[k] == SENTINEL).all(), (k, skip)
                elif k == "trust":
                    assert np.array_equal(o[k][:8], outs[i][k].astype(np.float32))
                else:
                    assert max(att_ref.quat_err(o[k][b], outs[i][k][b]) for b in range(8)) <= F32_FLOOR
            assert (o["status"] == SENTINEL).all() if "status" in skip else (o["status"][:8] == 0).all()
        assert max(att_ref.record_err(st[b], states[-1][b]) for b in range(8)) <= 4 * att_ref.D_Q


def test_header_known_answers_and_constants(robot):
    for k, check in ((att_ref.known_tilt(3), "tilt"), (att_ref.known_gyro_only(3), "gyro")):
        st = np.vstack([k["state"], np.zeros((2, 8))])
        inp = dict(gyro=k["gyro"], accel=k["accel"])
        for _ in range(k["ticks"]):
            host_launch(robot, st, inp, k["constants"])
        if check == "tilt":
            a = k["accel"][0].astype(np.float64)
            assert np.abs(att_ref.up(st[:3, :4]) - a / np.linalg.norm(a)).max() < KNOWN
        else:
            assert max(att_ref.quat_err(st[b, :4], k["answer"]) for b in range(3)) < KNOWN
    # every constant reaches the tick
    traj = att_ref.make_trajectory(4, 3, seed=5)
    start = att_ref.run(traj[:2])[0][-1]
    mine = dict(dt=0.002, gravity=9.0, kappa_ref=3.0, bias_gain=2.0, trust_window=0.35, touch_threshold=0.5)
    st = np.vstack([start, np.zeros((2, 8))])
    inp = dict(traj[2], touch=np.tile(np.float32([0.3, 1.0, 1.0, 0.3]), (4, 1)))
    o = host_launch(robot, st, inp, mine)
    ref, ro = att_ref.attitude_step(start, inp, mine)
    assert max(att_ref.record_err(st[b], ref[b]) for b in range(4)) <= 4 * att_ref.D_Q
    assert np.array_equal(o["trust"][:4], ro["trust"].astype(np.float32))
    for name in mine:
        other = att_ref.attitude_step(start, inp, {k: v for k, v in mine.items() if k != name})
        assert not (np.array_equal(other[0], ref) and np.array_equal(other[1]["trust"], ro["trust"])), name


def test_trust_agrees_with_the_leg_controller(robot):
    """For every Gait member, ibm 1 and 20 and every tick of two periods: trust == 0 exactly
    when swing_decide (csrc/mpcqp_swing_leg.h, what mpcqp_leg_torques runs) returns a swing
    state; the header's trust is att_ref's bitwise."""
    from mpcqp import params
    gaits = [params.GAITS[v] for v in params.GAIT_MEMBERS.values()] + [att_ref.WRAP]
    n = 0
    for period, offs, durs in gaits:
        for ibm in (1, 20):
            ticks = np.arange(2 * period * ibm)
            ref = att_ref.gait_trust(ticks, ibm, att_ref.gait_records([(period, offs, durs)] * len(ticks)), 0.2)
            for leg in range(4):
                for t in ticks:
                    tr = robot.trust(int(t), ibm, period, offs[leg], durs[leg], 0.2)
                    assert (tr == 0.0) == (robot.decide(int(t), ibm, period, offs[leg], durs[leg]) > 0)
                    assert tr == ref[t, leg] and 0.0 <= tr <= 1.0
                    n += 1
    # malformed records never swing: trust 1, as swing_decide says stance
    for bad in ((0, 0, 5), (10, 0, 12), (10, 0, 10), (-3, 0, 1)):
        assert robot.trust(7, 20, *bad, 0.2) == 1.0 and robot.decide(7, 20, *bad) == 0
    assert robot.trust(7, 0, 10, 0, 5, 0.2) == 1.0 and robot.trust(-7, 20, 10, 0, 5, 0.2) == robot.trust(193, 20, 10, 0, 5, 0.2)
    assert n > 10000


@pytest.mark.parametrize("key", ["gyro", "accel", "touch", "record"])
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_non_finite_input_leaves_that_robot_alone(robot, key, value):
    """Robot 1 gets status 4 and keeps its record, its outputs come from the record as it was,
    a bad touch zeroes its trusts, and robots 0, 2, 3 are bitwise unaffected -- on att_ref and
    on the header alike; from a running record and from an all-zero one."""
    traj = att_ref.make_trajectory(4, 6, seed=3)
    for start in (att_ref.run(traj[:5])[0][-1], np.zeros((4, 8))):
        inp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in traj[5].items()}
        start = start.copy()
        clean_ref, oc_ref = att_ref.attitude_step(start, traj[5])
        if key == "record":
            start[1, 6] = value
        else:
            inp[key][1, 2] = value
        new, out = att_ref.attitude_step(start, inp)
        st = np.vstack([start, np.zeros((2, 8))])
        o = host_launch(robot, st, inp)
        clean = np.vstack([start, np.zeros((2, 8))])      # the same launch without the bad value; robot 1's
        clean[1] = 0.0                                    # record (poisoned for key == "record") does not enter its trust
        oc = host_launch(robot, clean, traj[5])
        keep = [0, 2, 3]
        for got_state, got, ref_state, ref_out in ((new, out, clean_ref, oc_ref), (st[:4], o, clean[:4], oc)):
            assert got["status"][:4].tolist() == [0, 4, 0, 0], key
            assert np.array_equal(got_state[1], start[1], equal_nan=True)
            assert np.array_equal(got_state[keep], ref_state[keep])
            assert all(np.array_equal(got[k][:4][keep], ref_out[k][:4][keep]) for k in ("quat", "gyro_out", "trust"))
            was = att_ref.as_was(start)[1]
            assert np.array_equal(np.float32(got["quat"][1]), np.float32(was[:4]), equal_nan=True)
            if key in ("accel", "touch"):
                assert np.array_equal(np.float32(got["gyro_out"][1]), np.float32(inp["gyro"][1].astype(np.float64) - was[5:8]))
            if key == "touch":
                assert (got["trust"][1] == 0).all()
            else:
                assert np.array_equal(np.float32(got["trust"][1]), np.float32(ref_out["trust"][1]))


# ---- the CPU twins of tests/test_gpu_att_edges.py: the checks of tests/att_edge_checks.py
# on the host build of the header, so that each assertion made on the device is shown to hold
# for correct code without one

@pytest.fixture(scope="module")
def edge_launch(robot):
    def launch(state, inp, constants):
        st = np.vstack([state, np.full((2, att_ref.STRIDE), float(SENTINEL))])
        out = host_launch(robot, st, att_ref.select(inp, ("tick", "gait", "ibm", "touch")), constants)
        assert (st[-2:] == SENTINEL).all() and all((v[-2:] == SENTINEL).all() for v in out.values())
        return st, out
    return launch


@pytest.mark.parametrize("ibm", [1, 20, 2 ** 20])
def test_edge_trust_on_the_decision_table(edge_launch, ibm):
    """3a.  B = 42, 42, 43 rows; windows 0.2, 0, 0.5, 1e-300."""
    assert len(att_ref.trust_edges(ibm)[0]) == (43 if ibm == 2 ** 20 else 42)
    for window in att_ref.TRUST_WINDOWS:
        att_edge_checks.check_trust_table(edge_launch, ibm, window)


def test_edge_trust_exact_restatement_catches_a_float32_ramp():
    """The exact check matters: phi formed in float32 at nst = 2^30 would be out by 2^-24
    relative at least somewhere on the table -- k - 1/2 does not fit a float32 there."""
    tick, gait = att_ref.trust_edges(2 ** 20)
    worst = 0.0
    for b in range(len(tick)):
        for leg in range(4):
            swing, _, cs, nsw = att_edge_checks.swing_ref.decide_exact(tick[b], 2 ** 20, gait[b], leg)
            nst = int(gait[b, 5 + leg]) * 2 ** 20
            exact = att_edge_checks.trust_exact(tick[b], 2 ** 20, gait[b], leg, 0.2)
            if swing or exact in (0, 1):
                continue
            k = nst if cs == 0 else cs - nsw
            phi = np.float32(np.float32(k) - np.float32(0.5)) / np.float32(nst)
            got = min(np.float32(1), phi / np.float32(0.2), (np.float32(1) - phi) / np.float32(0.2))
            worst = max(worst, abs(float(got) - float(exact)) / float(exact))
    assert worst >= 100 * 2.0 ** -24


def test_edge_touch_threshold(edge_launch):
    att_edge_checks.check_touch_threshold(edge_launch)


def test_edge_first_tick(edge_launch):
    first, later = att_edge_checks.check_first_tick(edge_launch)
    print(f"\nfirst tick on the host: {first:.2e}, after 5 ticks {later:.2e}")


def test_edge_gate_and_switch(edge_launch):
    gate, switch = att_edge_checks.check_gate_and_switch(edge_launch)
    print(f"\ngate corners on the host: {gate:.2e}, small-angle switch {switch:.2e}")


def test_edge_large_rotation(edge_launch):
    large, huge = att_edge_checks.check_large_rotation(edge_launch)
    print(f"\nlarge rotation on the host: {large:.2e}; at 1e6 and 3e38 rad/s (both sides glibc) "
          + ", ".join(f"{v:.2e}" for v in huge))


def test_edge_seeded_records(edge_launch):
    seeded = att_edge_checks.check_seeded_records(edge_launch)
    print(f"\nseeded quaternions of norm 2, 1e-3, 1e-160 on the host: {seeded:.2e}")


def test_edge_refusal_across_a_workgroup(edge_launch):
    att_edge_checks.check_refusal_across_a_workgroup(edge_launch)

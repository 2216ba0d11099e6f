"""CPU: the swing half of the leg controller (mpcqp_leg_torques) without a GPU -- its
ABI surface, the float64 restatement tests/swing_ref.py and the host-compiled per-leg
header csrc/mpcqp_swing_leg.h, both against the reference's two recorded runs
(tests/golden/swing.npz, and swing_edges.npz with full gains, thigh z, commanded z
velocity and constants off their defaults), the curve's known answers, the decision's
integer edges, and that the inputs of tests/test_gpu_swing_edges.py can tell a wrong
kernel from a right one.

Measured here (norm-wise per robot, max over robots and quantities; printed by the two
fixture tests): see CPU_BOUND below and the docstring of tests/test_gpu_swing.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import _declared, host_build
import swing_ref
from swing_ref import SwingRef, quat2matrix_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpcqp.h")

# The restatements differ from the recorded run by the reference's float32
# intermediates under NumPy 2.2 promotion, its float32 break points and scipy standing
# in for Drake: a few float32 roundings (2^-24 = 6e-8 each) through a PD law whose
# error terms cancel by about an order of magnitude.  Anything above this bound wants
# an explanation, not a wider bound.
CPU_BOUND = 2.5e-6

SHIM = r'''
#include "mpcqp_swing_leg.h"
extern "C" int decide(int tick, int ibm, int period, int off, int dur, double* value) {
  return swing_decide(tick, ibm, period, off, dur, value);
}
extern "C" void curve(double t_swing, double cur, const double* init, const double* fin, double height, double* p,
                      double* v) {
  swing_curve(t_swing, cur, init, fin, height, p, v);
}
// one leg's share of one control iteration, as mpcqp_leg_torque_kernel strings the header together
// cst: dt_control, gravity, swing_height, touchdown_z, vel_gain
extern "C" int leg_tick(int tick, int ibm, const int* gait, int leg, const double* cst, const double* Kp,
                        const double* Kd, const double* pos, const double* vel, const double* R, const double* vb,
                        double yr, const double* thigh, const double* pfoot, const double* fpb, const double* fvb,
                        const float* J, const float* f, double* mem, float* tau, double* sv, double* pt,
                        double* vt) {
  const int st = swing_decide(tick, ibm, gait[0], gait[1 + leg], gait[5 + leg], sv);
  for (int k = 0; k < 3; ++k) pt[k] = vt[k] = 0.0;
  if (st == SWING_STANCE) {
    for (int j = 0; j < 3; ++j) tau[j] = -(J[j] * f[0] + J[3 + j] * f[1] + J[6 + j] * f[2]);
    return st;
  }
  double t_swing, t_stance, Jd[9], tq[3];
  for (int k = 0; k < 9; ++k) Jd[k] = J[k];
  swing_times(cst[0], ibm, gait[0], gait[5], &t_swing, &t_stance);
  swing_leg_step(mem, st == SWING_FINISHED, cst[0], t_swing, t_stance, pos, vel, R, vb, yr, thigh, pfoot, cst[1],
                 cst[4], cst[3], cst[2], pt, vt);
  swing_pd(R, Kp, Kd, Jd, pt, vt, fpb, fvb, tq);
  for (int k = 0; k < 3; ++k) tau[k] = (float)tq[k];
  return st;
}
'''


NEW_SYMBOLS = {"mpcqp_leg_torques", "mpcqp_leg_torques_root_states", "mpcqp_set_swing"}


def test_header_declares_the_swing_entry_points_and_binding_agrees():
    from mpcqp import _lib
    assert NEW_SYMBOLS <= _declared()
    assert _declared() == set(_lib.EXPORTED_SYMBOLS)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.mpcqp_abi_version() == 6     # additive: the ABI version stays


def test_swing_stride_matches_binding():
    from mpcqp import _lib
    src = open(HEADER).read()
    assert int(re.search(r"#define MPCQP_SWING_STRIDE (\d+)", src).group(1)) == _lib.SWING_STRIDE == 32
    assert swing_ref.STRIDE == _lib.SWING_STRIDE


def test_null_ctx_is_an_error_code():
    from mpcqp import _lib
    lib = _lib.load()
    assert lib.mpcqp_leg_torques(None, 1, 0, None, 20, *([None] * 19)) == -1
    assert lib.mpcqp_leg_torques_root_states(None, 1, 0, None, 20, *([None] * 16)) == -1
    assert lib.mpcqp_set_swing(None, 0.1, None, None, -0.0255, 0.03) == -1


@pytest.fixture(scope="module")
def fx():
    return swing_ref.load_fixture()


@pytest.fixture(scope="module")
def fxe():
    return swing_ref.load_fixture("swing_edges.npz")


@pytest.fixture(scope="module")
def leg():
    lib = host_build(SHIM, name="swing")
    dp, fp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
    lib.decide.argtypes = [ctypes.c_int] * 5 + [dp]
    lib.curve.argtypes = [ctypes.c_double, ctypes.c_double, dp, dp, ctypes.c_double, dp, dp]
    lib.leg_tick.argtypes = [ctypes.c_int, ctypes.c_int, ip, ctypes.c_int, dp, dp, dp, dp, dp, dp, dp,
                             ctypes.c_double, dp, dp, dp, dp, fp, fp, dp, fp, dp, dp, dp]
    lib.dp, lib.fp, lib.ip = dp, fp, ip
    return lib


def _report(tag, errs):
    worst = max(float(v.max()) for v in errs.values())
    print(f"\n{tag}: " + ", ".join(f"{k} {float(v.max()):.2e}" for k, v in errs.items()) + f" -> worst {worst:.3e}")
    return worst


def _gain3(k):
    k = np.asarray(k, np.float64)
    return np.ascontiguousarray(k if k.ndim == 2 else np.eye(3) * k)


def _restatement_run(fx):
    B, T = fx["tau"].shape[:2]
    ibm, every = int(fx["iterations_between_mpc"]), int(fx["check_every"])
    ref = SwingRef(B, dt_control=float(fx["dt_control"]), gravity=float(fx["gravity"]),
                   swing_height=float(fx["swing_height"]), kp=fx["kp"], kd=fx["kd"],
                   touchdown_z=float(fx["touchdown_z"]), vel_gain=float(fx["vel_gain"]))
    seq = swing_ref.empty_sequence(fx)
    for t in range(T):
        o = ref.step(np.full(B, t), ibm, fx["gait"], fx["pos"][:, t], fx["vel"][:, t],
                     quat2matrix_f32(fx["quat"][:, t]), fx["v_body"], fx["yaw_rate"], fx["thighs"],
                     fx["pos_feet"][:, t], fx["foot_pos_base"][:, t], fx["foot_vel_base"][:, t], fx["jac"], fx["u0"])
        for k in ("tau", "swing_state", "pos_target", "vel_target"):
            seq[k][:, t] = o[k]
        if t % every == 0:
            seq["ck_mem"][:, t // every] = ref.mem
    return seq


def test_restatement_reproduces_the_reference_run(fx):
    """swing_ref against swing.npz: the swing mask on every tick and the first-swing flags
    at the checkpoints exactly, the values within CPU_BOUND."""
    worst = _report("swing_ref vs swing.npz", swing_ref.compare_fixture(fx, _restatement_run(fx)))
    assert worst < CPU_BOUND


def _header_run(fx, leg):
    B, T = fx["tau"].shape[:2]
    ibm, every = int(fx["iterations_between_mpc"]), int(fx["check_every"])
    dp, fp, ip = leg.dp, leg.fp, leg.ip
    d = lambda a: np.ascontiguousarray(a, np.float64)
    seq = swing_ref.empty_sequence(fx)
    cst = d([fx["dt_control"], fx["gravity"], fx["swing_height"], fx["touchdown_z"], fx["vel_gain"]])
    mem = np.zeros((B, 4, 8))
    tau, sv, pt, vt = np.zeros(3, np.float32), ctypes.c_double(), np.zeros(3), np.zeros(3)
    for b in range(B):
        Kp, Kd = _gain3(fx["kp"][b]), _gain3(fx["kd"][b])
        gait = np.ascontiguousarray(fx["gait"][b], np.int32)
        vb = d(fx["v_body"][b])
        for t in range(T):
            R = d(quat2matrix_f32(fx["quat"][b:b + 1, t])[0]).reshape(9)
            pos, vel = d(fx["pos"][b, t]), d(fx["vel"][b, t])
            for l in range(4):
                th, pf = d(fx["thighs"][b, l]), d(fx["pos_feet"][b, t, l])
                fpb, fvb = d(fx["foot_pos_base"][b, t, l]), d(fx["foot_vel_base"][b, t, l])
                J = np.ascontiguousarray(fx["jac"][b, l], np.float32).reshape(9)
                f = np.ascontiguousarray(fx["u0"][b, 3 * l:3 * l + 3], np.float32)
                m = mem[b, l]
                leg.leg_tick(t, ibm, gait.ctypes.data_as(ip), l, cst.ctypes.data_as(dp), Kp.ctypes.data_as(dp),
                             Kd.ctypes.data_as(dp), pos.ctypes.data_as(dp), vel.ctypes.data_as(dp),
                             R.ctypes.data_as(dp), vb.ctypes.data_as(dp), float(fx["yaw_rate"][b]),
                             th.ctypes.data_as(dp), pf.ctypes.data_as(dp), fpb.ctypes.data_as(dp),
                             fvb.ctypes.data_as(dp), J.ctypes.data_as(fp), f.ctypes.data_as(fp),
                             m.ctypes.data_as(dp), tau.ctypes.data_as(fp), ctypes.byref(sv), pt.ctypes.data_as(dp),
                             vt.ctypes.data_as(dp))
                seq["tau"][b, t, 3 * l:3 * l + 3] = tau
                seq["swing_state"][b, t, l] = sv.value
                seq["pos_target"][b, t, l] = pt
                seq["vel_target"][b, t, l] = vt
            if t % every == 0:
                seq["ck_mem"][b, t // every] = mem[b]
    return seq


def test_host_compiled_header_reproduces_the_reference_run(fx, leg):
    """csrc/mpcqp_swing_leg.h compiled with g++ and driven tick by tick: the same checks."""
    worst = _report("mpcqp_swing_leg.h (g++) vs swing.npz", swing_ref.compare_fixture(fx, _header_run(fx, leg)))
    assert worst < CPU_BOUND


def _edges_fixture_is_what_the_issue_asks(fxe):
    """The second fixture's own promises: full non-symmetric gains in two groups, thigh z,
    commanded z velocity and the three constants off their defaults."""
    kp, kd = fxe["kp"], fxe["kd"]
    assert kp.shape == kd.shape == (6, 3, 3)
    for k in (kp, kd):
        assert (k[:3] == k[0]).all() and (k[3:] == k[3]).all() and not (k[0] == k[3]).any()
        for m in (k[0], k[3]):
            assert len(set(m.reshape(-1).tolist())) == 9 and not np.allclose(m, m.T)
            off = np.abs(m[~np.eye(3, dtype=bool)])
            assert off.min() >= 0.1 * np.abs(np.diag(m)).max()
    th = fxe["thighs"][..., 2]
    assert (np.abs(th) >= 0.02).all() and (np.abs(th) <= 0.08).all() and len(set(th.reshape(-1).tolist())) == th.size
    assert (np.abs(fxe["v_body"][:, 2]) >= 0.3).all()
    assert (float(fxe["dt_control"]), float(fxe["gravity"]), float(fxe["swing_height"])) == (0.002, 3.72, 0.07)
    assert int(fxe["iterations_between_mpc"]) == 2 and int(fxe["check_every"]) == 2
    members = [str(m) for m in fxe["member"]]
    assert "STANDING" in members and "TROTTING10" in members       # one never swings, one has unequal phases
    golden = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(os.path.join(golden, "swing_edges.npz")) <= os.path.getsize(os.path.join(golden, "swing.npz"))


def test_restatement_reproduces_the_edges_run(fxe):
    """swing_ref against swing_edges.npz -- full gains, thigh z, commanded z velocity, gravity,
    dt_control and swing_height off their defaults: the same checks as against swing.npz."""
    _edges_fixture_is_what_the_issue_asks(fxe)
    worst = _report("swing_ref vs swing_edges.npz", swing_ref.compare_fixture(fxe, _restatement_run(fxe)))
    assert worst < CPU_BOUND


def test_host_compiled_header_reproduces_the_edges_run(fxe, leg):
    """csrc/mpcqp_swing_leg.h compiled with g++ against swing_edges.npz."""
    worst = _report("mpcqp_swing_leg.h (g++) vs swing_edges.npz",
                    swing_ref.compare_fixture(fxe, _header_run(fxe, leg)))
    assert worst < CPU_BOUND


def test_edge_inputs_move_every_robots_torques():
    """What tests/test_gpu_swing_edges.py compares with swing_ref can fail: on its exact
    inputs and tick sequences (swing_ref.edge_case at B = 1, 63, 64, 65, and the single calls
    of swing_ref.edge_one_tick), transposing Kp or
    Kd, putting any of the five constants back to its default, or zeroing the thighs' z or
    the commanded z velocity moves swing_ref's tau of EVERY robot by at least 100 x the
    device bound, norm-wise.  On the second fixture's inputs the same holds for every robot
    that swings at all (STANDING does not)."""
    bound = 100 * 4.61e-7
    defaults = dict(dt_control=0.001, gravity=9.81, swing_height=0.1, touchdown_z=-0.0255, vel_gain=0.03)

    def changes(inp, kw):
        yield "Kp^T", inp, dict(kw, kp=np.swapaxes(np.asarray(kw["kp"]), -1, -2))
        yield "Kd^T", inp, dict(kw, kd=np.swapaxes(np.asarray(kw["kd"]), -1, -2))
        for k, v in defaults.items():
            assert kw[k] != v
            yield k, inp, dict(kw, **{k: v})
        for name, key in (("thigh z", "thighs"), ("v_body z", "v_body")):
            a = inp[key].copy()
            a[..., 2] = 0
            yield name, dict(inp, **{key: a}), kw

    def check(tag, inp, gait, ticks, ibm, kw, robots, mem0=None):
        base = swing_ref.run_ref(inp, gait, ticks, ibm, mem0=mem0, **kw)
        for name, inp2, kw2 in changes(inp, kw):
            o = swing_ref.run_ref(inp2, gait, ticks, ibm, mem0=mem0, **kw2)
            moved = np.array([swing_ref.norm_err(o["tau"][:, b], base["tau"][:, b]) for b in robots])
            print(f"{tag} {name}: min over robots {moved.min():.2e}")
            assert (moved >= bound).all(), (tag, name, moved.min())

    for B in (1, 63, 64, 65):
        inp, gait, ticks = swing_ref.edge_case(B)
        kw = dict(swing_ref.EDGE_CONSTS, kp=swing_ref.EDGE_KP, kd=swing_ref.EDGE_KD)
        check(f"B={B}", inp, gait, ticks, swing_ref.EDGE_IBM, kw, range(B))
    for B, seed in ((5, 440), (5, 441), (5, 442), (5, 443), (65, 430)):      # the single calls from a swing under way
        inp, gait, ticks, mem0 = swing_ref.edge_one_tick(B, 5, seed)
        check(f"one call, B={B} seed {seed}", inp, gait, ticks, swing_ref.EDGE_IBM, kw, range(B), mem0=mem0)
    fxe = swing_ref.load_fixture("swing_edges.npz")
    B, T = fxe["tau"].shape[:2]
    kw = dict(dt_control=float(fxe["dt_control"]), gravity=float(fxe["gravity"]), swing_height=float(fxe["swing_height"]),
              touchdown_z=0.031, vel_gain=0.11, kp=fxe["kp"], kd=fxe["kd"])
    swings = [b for b in range(B) if (np.nan_to_num(fxe["swing_state"][b]) > 0).any()]
    assert len(swings) == B - 1
    check("swing_edges.npz", swing_ref.fixture_inputs(fxe), fxe["gait"], np.tile(np.arange(T)[:, None], (1, B)),
          int(fxe["iterations_between_mpc"]), kw, swings)


def _curve(leg, T, cur, init, fin, h):
    dp = leg.dp
    i, f = np.ascontiguousarray(init, np.float64), np.ascontiguousarray(fin, np.float64)
    p, v = np.zeros(3), np.zeros(3)
    leg.curve(T, cur, i.ctypes.data_as(dp), f.ctypes.data_as(dp), h, p.ctypes.data_as(dp), v.ctypes.data_as(dp))
    return p, v


def test_curve_known_answers(leg):
    """init with zero velocity at 0, mid (z = swing_height) with zero velocity at T / 2,
    final at T, clamped outside [0, T] -- in the header and in the restatement alike."""
    T, h = 0.02, 0.1
    init, fin = np.array([0.3, -0.2, -0.02]), np.array([0.5, -0.1, -0.0255])
    mid = np.array([0.4, -0.15, h])
    t1, t2 = float(np.float32(T / 2)), float(np.float32(T))     # the float32 break points
    for cur, want in ((0.0, init), (t1, mid), (t2, fin), (-0.3, init), (T + 0.3, fin)):
        p, v = _curve(leg, T, cur, init, fin, h)
        pr, vr = swing_ref.curve(np.float64(T), np.float64(cur), init.copy(), fin.copy(), h)
        for pp, vv in ((p, v), (pr, vr)):
            assert np.allclose(pp, want, rtol=0, atol=1e-15), (cur, pp, want)
            assert np.allclose(vv, 0.0, rtol=0, atol=1e-12), (cur, vv)
    # between the breaks the foot moves: monotone in x, above both ends in z
    p, v = _curve(leg, T, 0.25 * T, init, fin, h)
    assert init[0] < p[0] < mid[0] and v[0] > 0 and v[2] > 0 and p[2] > init[2]
    pr, vr = swing_ref.curve(np.float64(T), np.float64(0.25 * T), init.copy(), fin.copy(), h)
    assert np.allclose(p, pr, rtol=1e-14) and np.allclose(v, vr, rtol=1e-13)


def test_decisions_of_header_and_restatement_agree(leg):
    """Every Gait member and two custom records (one leg's swing offset past the period;
    unequal durations) at iterations_between_mpc 1, 4 and 20, over two periods: the same
    stance / swing / finished decision and the same value."""
    from mpcqp.params import GAITS, gait_record
    recs = [gait_record(k) for k in GAITS] + [gait_record((10, (0, 7, 5, 2), (5, 6, 5, 3))),
                                               gait_record((12, (0, 6, 3, 9), (9, 9, 9, 9)))]
    sv = ctypes.c_double()
    for rec in recs:
        for ibm in (1, 4, 20):
            for tick in range(0, 2 * ibm * int(rec[0]) + 3):
                sw, fin, val = swing_ref.swing_state(np.array([tick]), ibm, rec[None])
                for l in range(4):
                    st = leg.decide(tick, ibm, int(rec[0]), int(rec[1 + l]), int(rec[5 + l]), ctypes.byref(sv))
                    assert (st != 0) == bool(sw[0, l]) and (st == 2) == bool(fin[0, l]), (rec, ibm, tick, l)
                    assert sv.value == val[0, l]
                    assert (sv.value > 0) == (st != 0) and (not fin[0, l] or abs(sv.value - 1.0) < 1e-6)
    # the integer edges (swing_ref.decision_edges: ticks at +-2^31, -1, 0 and around the span;
    # period 1, duration 0, a stance that fills the period on one leg, wrapping and negative
    # offsets, malformed periods; span up to 2^31) against Python's own integers
    for ibm, rows in swing_ref.decision_edges().items():
        for tick, rec in rows:
            for l in range(4):
                sw, fin, cs, nsw = swing_ref.decide_exact(tick, ibm, rec, l)
                sv.value = -1.0
                st = leg.decide(tick, ibm, int(rec[0]), int(rec[1 + l]), int(rec[5 + l]), ctypes.byref(sv))
                assert st == (2 if fin else 1 if sw else 0), (ibm, tick, rec, l, st, cs, nsw)
                if not sw:
                    assert sv.value == 0.0
                elif ibm * int(rec[0]) <= 2 ** 20:
                    # the float32 phase is the only inexact step: half an ulp, <= 2^-25, divided by the
                    # swing fraction; doubled
                    tol = 2.0 ** -24 / (1.0 - int(rec[5 + l]) / int(rec[0]))
                    assert abs(sv.value - cs / nsw) <= tol, (ibm, tick, rec, l, sv.value, cs / nsw)
                else:
                    assert np.isfinite(sv.value) and sv.value > 0
                if rec[0] > 0:       # the restatement says the same, value included
                    rsw, rfin, rval = swing_ref.swing_state(np.array([tick]), ibm, rec[None])
                    assert (bool(rsw[0, l]), bool(rfin[0, l]), rval[0, l]) == (sw, fin, sv.value)
    # some of them by hand: TROTTING10 at 20 iterations per MPC step, span 200
    trot = (10, (0, 5, 5, 0), (5, 5, 5, 5))
    rec = np.array([trot[0], *trot[1], *trot[2]])
    assert swing_ref.decide_exact(-1, 20, rec, 0) == (True, False, 99, 100)        # c = 199
    assert swing_ref.decide_exact(-1, 20, rec, 1)[0] is False                      # cs = 199
    assert swing_ref.decide_exact(-2 ** 31, 20, rec, 0) == (True, False, 52, 100)         # -2^31 mod 200 = 152
    assert swing_ref.decide_exact(-2 ** 31, 20, rec, 1) == (False, False, 152, 100)
    assert swing_ref.decide_exact(2 ** 31 - 1, 20, rec, 1) == (True, False, 47, 100)       # 2^31 - 1 mod 200 = 47
    assert swing_ref.decide_exact(2 ** 31 - 1, 20, rec, 0) == (False, False, 147, 100)
    assert swing_ref.decide_exact(100, 20, rec, 1) == (True, True, 100, 100)               # the finishing tick


def test_standing_never_swings_and_never_touches_swing_mem(leg):
    from mpcqp.params import gait_record
    rec = gait_record("standing")
    ref = SwingRef(1)
    ref.mem[:] = 7.0                                    # a sentinel the tick must leave alone
    rng = np.random.default_rng(5)
    r = lambda *s: rng.standard_normal(s)
    for tick in range(0, 4 * 16 * 2 + 1):
        o = ref.step(np.array([tick]), 4, rec[None], r(1, 3), r(1, 3), np.eye(3)[None], r(1, 3), r(1), r(1, 4, 3),
                     r(1, 4, 3), r(1, 4, 3), r(1, 4, 3), r(1, 4, 3, 3), r(1, 12))
        assert not o["swing"].any() and (o["swing_state"] == 0).all()
        assert (o["pos_target"] == 0).all() and (o["vel_target"] == 0).all()
        sv = ctypes.c_double(1.0)
        assert leg.decide(tick, 4, 16, 0, 16, ctypes.byref(sv)) == 0 and sv.value == 0.0
    assert (ref.mem == 7.0).all()

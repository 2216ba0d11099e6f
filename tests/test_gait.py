"""CPU: the gait scheduler (mpcqp_gait_schedule) without a GPU -- the ABI and Python surface, the
per-robot header csrc/mpcqp_gait_robot.h compiled with g++ and driven through ctypes against the
integer restatement tests/gait_ref.py and a direct count from swing_counts, the invariants the
rule promises along each run, the library's checks, the automatic choice, the scheduled closed
loop on the CPU oracles against its recorded figures (tests/golden/gait_switch.npz), and the
kernel's resource remarks on one device-only compile.

Measured here (printed by the tests):
  the closed loop (Aliengo, N = 10, ibm = 20, 1400 iterations, gait_ref.PLAN):
    robot  switches at   worst |height - 0.38|   worst |roll|, |pitch|
    0      320, 1020     0.0109 m                0.0365 rad
    1      600           0.0109                  0.0336
    2      500           0.0121                  0.2326  (pacing rocks, stays up)
    3      200, 1000     0.0117                  0.0298
    4      --            0.0109                  0.0336  (trots throughout)
    5      260, 960      0.0109                  0.0369  (the automatic choice)
  mpcqp_gait_kernel: ScratchSize 0, no vector or scalar register spilled, LDS 0.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import gait_ref as gr
import swing_ref
from helpers import _vp, host_build, kernel_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAIT_HEADER = os.path.join(ROOT, "include", "mpcqp_gait_abi.h")
GAIT_LDS = 0           # only a lane that switches reads the library, nothing is staged
IBMS = (1, 3, 20)

SHIM = r'''
#include "mpcqp_gait_robot.h"
// a launch of mpcqp_gait_kernel, robot after robot; ip: count, ibm, flags, min_hold, idle, move,
// dwell; dp: v_go^2, v_stop^2, w_go, w_stop
extern "C" void sched(int B, const int* ip, const double* dp, const int* lib, const int* want, const double* vb,
                      const double* yr, int* state, int* gait, int* tick, double* swing_mem, int* iteration,
                      int* switched, int* status) {
  GaitParams gp{ip[0], ip[1], ip[2], ip[3], ip[4], ip[5], ip[6], dp[0], dp[1], dp[2], dp[3]};
  auto fetch = [lib](int w, int* rec) {
    for (int k = 0; k < GAIT_LIB_WORDS; ++k) rec[k] = lib[GAIT_LIB_WORDS * w + k];
  };
  for (int b = 0; b < B; ++b)
    gait_robot(gp, (size_t)b, want, vb, yr, state, gait, tick, swing_mem, iteration, switched, status, fetch);
}
extern "C" int library(int count, const int* records, int* lib, int* which) { return gait_library(count, records, lib, which); }
extern "C" int entry(const int* g) { return gait_entry(g); }
extern "C" int seam(int t, int ibm, const int* g) { return gait_seam(t, ibm, g); }
extern "C" int counts(int t, int ibm, int period, int off, int dur, long long* cs, long long* nsw) {
  return swing_counts(t, ibm, period, off, dur, cs, nsw);
}
extern "C" int iteration_of(int t, int ibm, int period) { return gait_iteration(t, ibm, period); }
extern "C" int stride(void) { return SCHED_STRIDE; }
extern "C" int lib_words(void) { return GAIT_LIB_WORDS; }
extern "C" int lib_max(void) { return GAIT_LIB_MAX; }
'''


@pytest.fixture(scope="module")
def header():
    return host_build(SHIM, ("-O2", "-std=c++17", "-ffp-contract=off"), "gait")


def all_gaits():
    """The ten records of the tests: the seven of params.GAITS and gait_ref.CUSTOM."""
    from mpcqp.params import GAITS
    return [gr.record(g) for g in GAITS.values()] + [gr.record(g) for g in gr.CUSTOM]


def header_library(header, gaits):
    """(code, which, lib [16,10] int32) of the header's gait_library."""
    recs = np.ascontiguousarray(np.stack([gr.record(g) for g in gaits]), np.int32) if len(gaits) else np.zeros((0, 9), np.int32)
    lib = np.full((16, 10), -7, np.int32)
    which = ctypes.c_int(-9)
    code = header.library(len(gaits), _vp(recs), _vp(lib), ctypes.byref(which))
    return code, which.value, lib


def run_header(header, lib, c, flags, ibm, want, state, gait, tick, swing_mem=None, vb=None, yr=None, outputs=True):
    """gait_ref.schedule's call through the host-compiled header: in place on int32 arrays."""
    B = len(tick)
    for a in (state, gait, tick):
        assert a.dtype == np.int32 and a.flags.c_contiguous
    ip = np.array([len(lib), ibm, flags, c.min_hold, c.idle, c.move, c.dwell], np.int32)
    dp = np.array([c.v_go * c.v_go, c.v_stop * c.v_stop, c.w_go, c.w_stop], np.float64)
    full = np.zeros((16, 10), np.int32)
    full[:len(lib)] = lib
    it, sw, st = (np.full(B, -3, np.int32) for _ in range(3))
    w = None if want is None else np.ascontiguousarray(want, np.int32)
    v = None if vb is None else np.ascontiguousarray(vb, np.float64)
    y = None if yr is None else np.ascontiguousarray(yr, np.float64)
    header.sched(B, _vp(ip), _vp(dp), _vp(full), _vp(w), _vp(v), _vp(y), _vp(state), _vp(gait), _vp(tick), _vp(swing_mem),
                 _vp(it) if outputs else None, _vp(sw) if outputs else None, _vp(st) if outputs else None)
    return it, sw, st


# ---- the ABI and Python surface

def test_constants_agree(header):
    from mpcqp import _lib
    src = open(GAIT_HEADER).read()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", src).group(1))
    assert define("MPCQP_SCHED_STRIDE") == _lib.SCHED_STRIDE == gr.STRIDE == header.stride() == 8
    assert define("MPCQP_GAIT_MAX") == _lib.GAIT_MAX == gr.GAIT_MAX == header.lib_max() == 16
    assert define("MPCQP_GAIT_ADVANCE") == _lib.GAIT_ADVANCE == gr.ADVANCE == 1
    assert header.lib_words() == 10
    assert (gr.OK, gr.NONFINITE, gr.UNSUPPORTED) == (_lib.STATUS_OK, _lib.STATUS_NONFINITE, _lib.STATUS_UNSUPPORTED)


def test_null_ctx_is_an_error_code():
    """Every call refuses a NULL context with -1.  The other misuse rules need a context, which
    needs a device: tests/test_gpu_gait.py checks them."""
    from mpcqp import _lib
    lib = _lib.load()
    assert lib.mpcqp_set_gaits(None, 1, None) == -1
    assert lib.mpcqp_set_gait_schedule(None, 0, -1, -1, 0.0, 0.0, 0.0, 0.0, 0) == -1
    assert lib.mpcqp_gait_schedule(None, 1, 0, 20, *([None] * 11)) == -1


def test_python_surface():
    import mpcqp
    from mpcqp.gait import BatchedGaitScheduler
    assert "BatchedGaitScheduler" in mpcqp.__all__ and mpcqp.BatchedGaitScheduler is BatchedGaitScheduler
    for name in ("request", "auto", "set_constants", "update", "bind_update", "reset", "set_gaits"):
        assert getattr(BatchedGaitScheduler, name).__doc__
    for name in ("current", "pending", "since", "switches", "switched", "status"):
        assert isinstance(getattr(BatchedGaitScheduler, name), property)


# ---- seams: the header, the restatement and a direct count from swing_counts

def counted_seam(header, t, ibm, g):
    """From swing_counts itself: aligned, and no leg with 1 <= cs < nsw."""
    if t % ibm:
        return False
    cs, nsw = ctypes.c_longlong(), ctypes.c_longlong()
    for leg in range(4):
        if header.counts(int(t), ibm, int(g[0]), int(g[1 + leg]), int(g[5 + leg]), ctypes.byref(cs), ctypes.byref(nsw)):
            if 1 <= cs.value < nsw.value:
                return False
    return True


@pytest.mark.parametrize("ibm", IBMS)
def test_seams_agree_three_ways(header, ibm):
    """Every tick of two spans of each of the ten records: gait_seam of the header, gait_ref.seam,
    gait_ref.seam_by_counts (the leg controller's decision in unbounded integers) and the count
    from swing_counts agree; every record has a seam, and the named ones have one at tick 0."""
    for n, g in enumerate(all_gaits()):
        g32 = np.ascontiguousarray(g, np.int32)
        span = int(g[0]) * ibm
        seams = []
        for t in range(2 * span + 1):
            a, b = bool(header.seam(t, ibm, _vp(g32))), gr.seam(t, ibm, g)
            assert a == b == gr.seam_by_counts(t, ibm, g) == counted_seam(header, t, ibm, g), (g.tolist(), ibm, t)
            if a:
                seams.append(t)
        assert seams and (n >= 7 or seams[0] == 0)
        assert seams[0] == gr.entry(g) * ibm == header.entry(_vp(g32)) * ibm


# ---- the header against the restatement: every ordered pair, every request tick

def _run_pair_batch(header, old, ibm, gaits, lib):
    """Robots (new gait j, request tick r): all start in `old` at its entry tick and ask for j
    before the call of iteration r, r over two spans of `old`; run until every robot has had a
    span and a half after its request.  Returns the per-call streams of the header's run after
    holding every buffer to the restatement's on every call."""
    g_old = lib[old, :9]
    span = int(g_old[0]) * ibm
    others = [j for j in range(len(gaits)) if j != old]
    new = np.repeat(others, 2 * span).astype(np.int32)
    ask = np.tile(np.arange(2 * span), len(others))
    B = len(new)
    T = 2 * span + span + span // 2 + 2
    c = gr.Constants()
    rng = np.random.default_rng(old * 100 + ibm)
    pattern = rng.integers(1, 2 ** 62, (B, 32), dtype=np.int64).view(np.float64)       # finite, non-zero bit patterns
    state = np.zeros((B, 8), np.int32)
    state[:, gr.CUR] = state[:, gr.PENDING] = old
    state[:, 6:8] = rng.integers(-99, 99, (B, 2))
    bufs = []
    for _ in range(2):
        bufs.append(dict(state=state.copy(), gait=np.tile(g_old, (B, 1)).astype(np.int32),
                         tick=np.full(B, int(lib[old, 9]) * ibm, np.int32), mem=pattern.copy()))
    h, r = bufs
    want = np.full(B, -1, np.int32)
    ticks, gaits_t, sw_t = [], [], []
    for k in range(T):
        want[ask == k] = new[ask == k]
        flags = gr.ADVANCE if k > 0 else 0
        got = run_header(header, lib, c, flags, ibm, want, h["state"], h["gait"], h["tick"], h["mem"])
        ref = gr.schedule(lib, c, flags, ibm, want, r["state"], r["gait"], r["tick"], r["mem"])
        for a, b, name in zip(got, ref, ("iteration", "switched", "status")):
            assert np.array_equal(a, b), (name, old, ibm, k)
        for name in ("state", "gait", "tick"):
            assert np.array_equal(h[name], r[name]), (name, old, ibm, k)
        assert np.array_equal(h["mem"].view(np.int64), r["mem"].view(np.int64)), ("swing_mem", old, ibm, k)
        assert (got[2] == 0).all()
        ticks.append(h["tick"].copy())
        gaits_t.append(h["gait"].copy())
        sw_t.append(got[1].copy())
    return dict(tick=np.stack(ticks), gait=np.stack(gaits_t), switched=np.stack(sw_t), state=h["state"], mem=h["mem"],
                pattern=pattern, new=new, ask=ask, state0=state, span=span)


def _cs(tick, ibm, gait):
    """cs and nsw [.., 4] of swing_counts, in NumPy's int64."""
    g = gait.astype(np.int64)
    P, off, dur = g[..., :1], g[..., 1:5], g[..., 5:9]
    span = ibm * P
    nsw = (P - dur) * ibm
    return (tick.astype(np.int64)[..., None] % span - (off + dur) * ibm) % span, nsw


@pytest.mark.parametrize("ibm", IBMS)
def test_header_matches_the_restatement_and_keeps_the_invariants(header, ibm):
    """Every ordered pair of the ten records, every tick of two spans of the old gait as the
    request tick: the header and gait_ref agree on every record word, gait word, tick, swing_mem
    word, iteration, switched and status of every call.  Along each run:
      every robot switches exactly once, at the first seam of its old gait at or after its request
        (counted from swing_counts), to its new gait's entry tick;
      (tick - global iteration) mod ibm never changes;
      no leg's swing begins with cs > 1 -- but for a leg at cs == nsw in the call of an entry;
      after a switch the four armed slots are zero and every other word of swing_mem, and the two
        reserved record words, are the bit pattern they were filled with."""
    gaits = all_gaits()
    code, _, lib = header_library(header, gaits)
    assert code == 0 and np.array_equal(lib[:10].astype(np.int64), gr.library(gaits))
    lib = lib[:10]
    for old in range(len(gaits)):
        run = _run_pair_batch(header, old, ibm, gaits, lib)
        tick, gait, switched = run["tick"], run["gait"], run["switched"]
        T, B = tick.shape
        k = np.arange(T)[:, None]
        assert ((tick - k) % ibm == (tick[0] % ibm)[None]).all()
        assert (switched.sum(0) == 1).all()
        at = switched.argmax(0)
        t0 = int(lib[old, 9]) * ibm
        for b in range(0, B, max(1, B // 97)):              # the switch tick by a direct count, on a sample
            t = t0 + run["ask"][b]
            while not counted_seam(header, t, ibm, lib[old, :9]):
                t += 1
            assert at[b] == t - t0, (old, ibm, b)
        assert np.array_equal(tick[at, np.arange(B)], lib[run["new"], 9] * ibm)
        assert np.array_equal(gait[-1], lib[run["new"], :9])
        assert np.array_equal(run["state"][:, gr.LAST], t0 + at)
        assert (run["state"][:, gr.CUR] == run["new"]).all() and (run["state"][:, gr.SWITCHES] == 1).all()
        assert np.array_equal(run["state"][:, gr.SINCE], T - 1 - at)
        assert np.array_equal(run["state"][:, 6:8], run["state0"][:, 6:8])
        # the stream as the leg controller sees it
        flat_t, flat_g = tick.reshape(-1), gait.reshape(-1, 9)
        swing, finished, _ = swing_ref.swing_state(flat_t, ibm, flat_g)
        swing, finished = swing.reshape(T, B, 4), finished.reshape(T, B, 4)
        cs, nsw = _cs(tick, ibm, gait)
        begins = swing[1:] & ~swing[:-1]
        entry = switched[1:].astype(bool)[..., None]
        assert (cs[1:][begins & ~entry] == 1).all()
        assert ((cs[1:] == 1) | (cs[1:] == nsw[1:]))[begins & entry].all()
        active = swing & ~finished
        assert not active[switched.astype(bool)].any()      # no entry and no exit cuts into a swing
        assert ((cs[1:] == cs[:-1] + 1) | ~active[1:] | (cs[1:] == 1)).all()
        # swing_mem: armed slots zero, the rest untouched
        want_mem = run["pattern"].copy()
        want_mem[:, 0::8] = 0.0
        assert np.array_equal(run["mem"].view(np.int64), want_mem.view(np.int64))


def test_a_robot_that_does_not_switch_keeps_swing_mem_and_gait(header):
    gaits = all_gaits()
    lib = gr.library(gaits).astype(np.int32)
    B = 5
    state = np.zeros((B, 8), np.int32)
    state[:, gr.CUR] = state[:, gr.PENDING] = 2
    gait = np.tile(lib[2, :9], (B, 1)).astype(np.int32)
    tick = np.array([0, 7, 20, 99, 1234], np.int32)
    mem = np.arange(B * 32, dtype=np.float64).reshape(B, 32) + 0.5
    it, sw, st = run_header(header, lib, gr.Constants(), gr.ADVANCE, 20, np.full(B, -1, np.int32), state, gait, tick, mem)
    assert np.array_equal(tick, [1, 8, 21, 100, 1235]) and (sw == 0).all() and (st == 0).all()
    assert np.array_equal(mem, np.arange(B * 32).reshape(B, 32) + 0.5) and (gait == lib[2, :9]).all()
    assert np.array_equal(state[:, gr.SINCE], [1] * B) and np.array_equal(it, (tick // 20) % 10)
    # with every output NULL the records move the same
    s2, t2 = state.copy(), tick.copy()
    run_header(header, lib, gr.Constants(), gr.ADVANCE, 20, np.full(B, -1, np.int32), s2, gait, t2, None, outputs=False)
    assert np.array_equal(t2, tick + 1) and np.array_equal(s2[:, gr.SINCE], [2] * B)


# ---- the library

def test_library_checks_leave_the_previous_library(header):
    from mpcqp.params import GAITS
    named = list(GAITS.values())
    code, which, lib = header_library(header, named)
    assert code == 0 and (lib[:7, 9] == 0).all() and (lib[7:] == 0).all()          # e(g) == 0 for the seven named gaits
    assert all(gr.entry(gr.record(g)) == 0 for g in named)
    code, _, lib10 = header_library(header, all_gaits())
    assert code == 0 and lib10[:10, 9].tolist() == [gr.entry(g) for g in all_gaits()] and lib10[7, 9] == 2
    trot = (10, (0, 5, 5, 0), (5, 5, 5, 5))
    # the oracle's search finds no entry segment of NO_ENTRY: at every segment some leg is mid-swing
    g = gr.record(gr.NO_ENTRY)
    assert gr.entry(g) is None and gr.valid(g)
    assert all(any(gr.mid_swing(s * ibm, ibm, g, leg) for leg in range(4)) for s in range(4) for ibm in IBMS)
    bad = {"period 0": ((0, (0, 0, 0, 0), (0, 0, 0, 0)), 2), "period 2049": ((2049, (0,) * 4, (1,) * 4), 2),
           "negative duration": ((10, (0, 5, 5, 0), (5, -1, 5, 5)), 2), "duration past the period": ((10, (0,) * 4, (5, 11, 5, 5)), 2),
           "offset past 4 P": ((10, (0, 41, 5, 0), (5,) * 4), 2), "offset below -4 P": ((10, (0, -41, 5, 0), (5,) * 4), 2),
           "no entry segment": (gr.NO_ENTRY, 3)}
    for name, (rec, want) in bad.items():
        assert not gr.valid(gr.record(rec)) or gr.entry(gr.record(rec)) is None, name
        for place in (0, 1):
            gaits = [trot, trot]
            gaits[place] = rec
            lib = lib10.copy()
            recs = np.ascontiguousarray(np.stack([gr.record(x) for x in gaits]), np.int32)
            which = ctypes.c_int(-9)
            code = header.library(2, _vp(recs), _vp(lib), ctypes.byref(which))
            assert code == want and which.value == place, (name, place, code)
            assert np.array_equal(lib, lib10), name                              # the previous library stays
    ok = {"period 2048": (2048, (0, 1024, 1024, 0), (1024,) * 4), "offsets at +-4 P": (10, (40, -40, 5, 0), (5,) * 4),
          "durations 0 and P": (10, (0, 0, 0, 0), (0, 10, 10, 10))}
    for name, rec in ok.items():
        assert header_library(header, [rec])[0] == 0, name
    lib = lib10.copy()
    which = ctypes.c_int()
    recs = np.ascontiguousarray(np.tile(gr.record(trot), (17, 1)), np.int32)
    for count in (0, -1, 17):
        assert header.library(count, _vp(recs), _vp(lib), ctypes.byref(which)) == 1 and np.array_equal(lib, lib10)
    assert header.library(1, None, _vp(lib), ctypes.byref(which)) == 1 and np.array_equal(lib, lib10)
    assert header.library(16, _vp(recs), _vp(lib), ctypes.byref(which)) == 0


# ---- the automatic choice

def _auto_run(header, c, lib, cmds, state0=None):
    """One robot through the commands (vx, vy, yaw) call after call: the (pending, calm, status)
    after each, from the header, held to the restatement."""
    st = [np.zeros((1, 8), np.int32) if state0 is None else state0.copy() for _ in range(2)]
    gait = [np.tile(lib[0, :9], (1, 1)).astype(np.int32) for _ in range(2)]
    tick = [np.array([1], np.int32) for _ in range(2)]             # never aligned at ibm = 2^30: no switch
    out = []
    for vx, vy, yaw in cmds:
        vb, yr = np.array([[vx, vy, 9.9]]), np.array([yaw])
        got = run_header(header, lib, c, 0, 2 ** 30, None, st[0], gait[0], tick[0], None, vb, yr)
        ref = gr.schedule(lib, c, 0, 2 ** 30, None, st[1], gait[1], tick[1], None, vb, yr)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)) and np.array_equal(st[0], st[1])
        out.append((int(st[0][0, gr.PENDING]), int(st[0][0, gr.CALM]), int(got[2][0])))
    return out


def test_automatic_choice_thresholds_hysteresis_and_dwell(header):
    lib = gr.library(all_gaits()).astype(np.int32)
    c = gr.Constants(idle=0, move=2, v_go=0.25, v_stop=0.125, w_go=0.5, w_stop=0.25, dwell=3)
    up = np.nextafter
    # at equality nothing moves: v == v_go is not above it; one ulp above is
    assert _auto_run(header, c, lib, [(0.25, 0.0, 0.0)])[0][0] == 0
    assert _auto_run(header, c, lib, [(up(0.25, 1), 0.0, 0.0)])[0][:2] == (2, 0)
    assert _auto_run(header, c, lib, [(0.15, 0.2, 0.0)])[0][0] == 0                  # 0.15^2 + 0.2^2 == 0.25^2 exactly
    assert _auto_run(header, c, lib, [(0.0, 0.0, -0.5)])[0][0] == 0 and _auto_run(header, c, lib, [(0, 0, -up(0.5, 1))])[0][0] == 2
    assert 0.15 * 0.15 + 0.2 * 0.2 == 0.25 * 0.25
    # v_y counts, v_z does not (vel_body_des[2] is 9.9 throughout)
    assert _auto_run(header, c, lib, [(0.0, -0.3, 0.0)])[0][0] == 2
    # moving, then at the stop threshold itself (calm: at or below), dwell 3: idle on the third calm call
    moving = np.zeros((1, 8), np.int32)
    moving[0, gr.CUR] = moving[0, gr.PENDING] = 2
    run = _auto_run(header, c, lib, [(0.125, 0.0, 0.25)] * 4, moving)
    assert run == [(2, 1, 0), (2, 2, 0), (0, 3, 0), (0, 4, 0)]
    # the band between the thresholds keeps the latched request and restarts the count
    run = _auto_run(header, c, lib, [(0.1, 0, 0), (0.1, 0, 0), (0.2, 0, 0), (0.1, 0, 0), (0.1, 0, 0), (0.0, 0.0, 0.3), (0.1, 0, 0)], moving)
    assert run == [(2, 1, 0), (2, 2, 0), (2, 0, 0), (2, 1, 0), (2, 2, 0), (2, 0, 0), (2, 1, 0)]
    # just above the stop threshold is the band
    assert _auto_run(header, c, lib, [(up(0.125, 1), 0, 0)] * 5, moving)[-1] == (2, 0, 0)
    # dwell 0: idle at once; and a move command restarts it
    c0 = gr.Constants(idle=0, move=2, v_go=0.25, v_stop=0.125, w_go=0.5, w_stop=0.25, dwell=0)
    assert _auto_run(header, c0, lib, [(0.0, 0.0, 0.0), (1.0, 0, 0), (0, 0, 0)], moving) == [(0, 1, 0), (2, 0, 0), (0, 1, 0)]
    # a non-finite command: the status, and nothing but the clock changes
    for bad in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (0, 0, np.nan)):
        run = _auto_run(header, c, lib, [(0.0, 0, 0), bad, (0.0, 0, 0)], moving)
        assert run == [(2, 1, 0), (2, 1, gr.NONFINITE), (2, 2, 0)], bad


def test_a_nonfinite_command_advances_the_clock_and_blocks_the_switch(header):
    lib = gr.library(all_gaits()).astype(np.int32)
    c = gr.Constants(idle=0, move=2, v_go=0.25, v_stop=0.125, w_go=0.5, w_stop=0.25, dwell=0)
    state = np.zeros((2, 8), np.int32)
    state[:, gr.PENDING] = 2                                    # standing, a request for trot10 latched
    gait = np.tile(lib[0, :9], (2, 1)).astype(np.int32)
    tick = np.array([19, 19], np.int32)
    vb, yr = np.array([[np.nan, 0, 0], [1.0, 0, 0]]), np.zeros(2)
    for step in (lambda *a, **k: run_header(header, *a, **k), gr.schedule):
        s, g, t = state.copy(), gait.copy(), tick.copy()
        it, sw, st = step(lib, c, gr.ADVANCE, 20, None, s, g, t, None, vb, yr)
        assert st.tolist() == [gr.NONFINITE, 0] and sw.tolist() == [0, 1] and t.tolist() == [20, 0]
        assert s[0].tolist() == [0, 2, 1, 0, 0, 0, 0, 0] and s[1].tolist() == [2, 2, 0, 1, 0, 20, 0, 0]


# ---- min_hold, want, the tick's range

def test_min_hold_want_and_tick_range(header):
    lib = gr.library(all_gaits()).astype(np.int32)
    for step in (lambda *a, **k: run_header(header, *a, **k), gr.schedule):
        # min_hold 45 on a standing robot (every aligned tick a seam): asked at once, honoured at
        # the first aligned tick with since >= 45, which is 60
        c = gr.Constants(min_hold=45)
        state, gait, tick = np.zeros((1, 8), np.int32), lib[None, 0, :9].astype(np.int32).copy(), np.zeros(1, np.int32)
        want = np.array([2], np.int32)
        when = None
        for k in range(100):
            _, sw, st = step(lib, c, gr.ADVANCE if k else 0, 20, want, state, gait, tick)
            if sw[0] and when is None:
                when = k
        assert when == 60 and state[0, :6].tolist() == [2, 2, 39, 1, 0, 60] and tick[0] == 39
        # since >= min_hold exactly: 40 is honoured at 40
        c = gr.Constants(min_hold=40)
        state, gait, tick = np.zeros((1, 8), np.int32), lib[None, 0, :9].astype(np.int32).copy(), np.zeros(1, np.int32)
        for k in range(41):
            _, sw, _ = step(lib, c, gr.ADVANCE if k else 0, 20, want, state, gait, tick)
        assert sw[0] == 1 and state[0, gr.LAST] == 40
        # want: -1 keeps a latched request, the current index withdraws it, outside the library UNSUPPORTED
        c = gr.Constants()
        B = 6
        state = np.zeros((B, 8), np.int32)
        state[:, gr.PENDING] = [0, 2, 2, 0, 0, 2]
        gait = np.tile(lib[0, :9], (B, 1)).astype(np.int32)
        tick = np.full(B, 39, np.int32)
        want = np.array([-1, -1, 0, 10, -2, 16], np.int32)
        it, sw, st = step(lib, c, gr.ADVANCE, 20, want, state, gait, tick)
        assert st.tolist() == [0, 0, 0, gr.UNSUPPORTED, gr.UNSUPPORTED, gr.UNSUPPORTED]
        assert sw.tolist() == [0, 1, 0, 0, 0, 1]                       # the last: its earlier request is still honoured
        assert tick.tolist() == [40, 0, 40, 40, 40, 0] and state[:, gr.PENDING].tolist() == [0, 2, 0, 0, 0, 2]
        assert it.tolist() == [2, 0, 2, 2, 2, 0]
        # a record set by hand (current -1): left at one of its own seams
        state = np.zeros((1, 8), np.int32)
        state[0, :2] = (-1, -1)
        hand = np.array([[12, 0, 6, 6, 0, 6, 6, 6, 6]], np.int32)     # a trot of period 12
        tick = np.array([100], np.int32)
        want = np.array([1], np.int32)
        for k in range(30):
            _, sw, st = step(lib, c, gr.ADVANCE, 20, want, state, hand, tick)
            if sw[0]:
                break
        assert st[0] == 0 and state[0, gr.LAST] == 120 and gr.seam(120, 20, [12, 0, 6, 6, 0, 6, 6, 6, 6]) and not gr.seam(100, 20, [12, 0, 6, 6, 0, 6, 6, 6, 6])
        assert (hand[0] == lib[1, :9]).all() and state[0, gr.CUR] == 1
        # the tick's range: negative, and INT32_MAX under advance, are left untouched
        B = 4
        state = np.zeros((B, 8), np.int32)
        state[:, gr.PENDING] = 2
        state[:, gr.SINCE] = 5
        gait = np.tile(lib[0, :9], (B, 1)).astype(np.int32)
        tick = np.array([-1, gr.INT_MAX, gr.INT_MAX - 1, -2 ** 31], np.int32)
        s0 = state.copy()
        it, sw, st = step(lib, c, gr.ADVANCE, 20, np.full(B, 2, np.int32), state, gait, tick)
        assert st.tolist() == [gr.UNSUPPORTED, gr.UNSUPPORTED, 0, gr.UNSUPPORTED] and (sw == 0).all()
        assert tick.tolist() == [-1, gr.INT_MAX, gr.INT_MAX, -2 ** 31]
        assert np.array_equal(state[[0, 1, 3]], s0[[0, 1, 3]]) and state[2, gr.SINCE] == 6
        assert it.tolist() == [15, (gr.INT_MAX // 20) % 16, (gr.INT_MAX // 20) % 16, ((-2 ** 31) % 320) // 20]
        # without advance INT32_MAX is a tick like any other
        tick = np.array([gr.INT_MAX], np.int32)
        _, _, st = step(lib, c, 0, 20, np.array([-1], np.int32), state[:1].copy(), gait[:1].copy(), tick)
        assert st[0] == 0 and tick[0] == gr.INT_MAX
        # since saturates
        state = np.zeros((1, 8), np.int32)
        state[0, gr.SINCE] = gr.INT_MAX
        tick = np.array([5], np.int32)
        step(lib, c, gr.ADVANCE, 20, np.array([-1], np.int32), state, gait[:1].copy(), tick)
        assert state[0, gr.SINCE] == gr.INT_MAX and tick[0] == 6


def test_iteration_is_the_planner_segment(header):
    for ibm in IBMS:
        for g in all_gaits():
            P = int(g[0])
            for t in (0, 1, ibm - 1, ibm, P * ibm - 1, P * ibm, 7 * P * ibm + 3 * ibm + 1, gr.INT_MAX):
                assert header.iteration_of(t, ibm, P) == (t // ibm) % P
    assert header.iteration_of(5, 20, 0) == 0 and header.iteration_of(5, 20, -3) == 0


# ---- the closed loop on the CPU oracles, against the recorded figures

@pytest.fixture(scope="module")
def loop():
    return gr.closed_loop_scheduled(gr.PLAN, gr.PLAN_TICKS)


def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "gait_switch.npz")))


def test_the_scheduled_closed_loop_switches_where_recorded_and_stays_up(loop):
    """gait_ref.PLAN: requests made at arbitrary ticks are honoured at the next seam -- 320 / 1020,
    600, 500, 200 / 1000, and 260 / 960 for the automatic robot -- every status OK and every solve
    converged, and every robot but the pacing one stays under the hard limits of
    tests/test_gpu_plant.py, 0.05 m and 0.1 rad.  The figures are the recorded ones."""
    fx = golden()
    sw = loop["switch_ticks"]
    print(f"\nswitch ticks {sw}")
    assert tuple(tuple(s) for s in sw) == gr.PLAN_SWITCHES
    assert [s for s in sw] == [[int(x) for x in row if x >= 0] for row in fx["switch_ticks"]]
    assert loop["finite"].all() and loop["solve_ok"].all()
    err, tilt, speeds = gr.figures(loop["x"], loop["height"], loop["roll"], loop["pitch"], sw, loop["dt"])
    for b in range(len(gr.PLAN)):
        print(f"robot {b}: height error {err[b]:.4f} m, roll / pitch {tilt[b]:.4f} rad, phase speeds {np.round(speeds[b], 4).tolist()}")
    pacing = 2
    others = [b for b in range(len(gr.PLAN)) if b != pacing]
    assert (err < 0.05).all() and (tilt[others] < 0.1).all() and tilt[pacing] < 0.3
    assert np.abs(err - fx["height_error"]).max() < 5e-5 and np.abs(tilt - fx["tilt"]).max() < 5e-4
    for b, row in enumerate(speeds):
        assert np.abs(np.array(row) - fx["phase_speed"][b, :len(row)]).max() < 5e-4 and np.isnan(fx["phase_speed"][b, len(row):]).all()
    # the robots that stopped settle: within 0.02 m/s of rest over their last 200 ticks... robot 5
    # stops at 960 under the automatic choice and is still gliding to rest (0.03 m/s)
    assert abs(speeds[0][-1]) < 0.02 and abs(speeds[1][-1]) < 0.005 and abs(speeds[5][-1]) < 0.05


# ---- the kernel's resources

@pytest.fixture(scope="module")
def usage():
    return kernel_usage()


def test_gait_kernel_has_no_private_memory_no_spills_and_no_lds(usage):
    hits = [v for n, v in usage.items() if re.search(r"\d+mpcqp_gait_kernelE", n)]
    assert len(hits) == 1, sorted(usage)
    u = hits[0]
    print(f"\nmpcqp_gait_kernel: {u}")
    assert u.get("ScratchSize") == 0, u
    assert u.get("VGPRs Spill") == 0 and u.get("SGPRs Spill") == 0, u
    assert u.get("LDS Size") == GAIT_LDS, u

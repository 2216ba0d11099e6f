"""CPU: the solve's routing policy (csrc/mpcqp_solve_plan.h), compiled for the host with g++:
which capacity classes one mpcqp_solve call launches, which one takes the batch directly, and
the launches' schedule (order, priority, interior-point layout, fork).  The schedule never
changes a result, so no parity test on the GPU can see it: it is checked here, against plans
written out by hand from the rules and against the rules' invariants over a grid."""
import ctypes

import numpy as np
import pytest

from helpers import host_build

# one row of ints per plan, in this order
FIELDS = ("first", "l64", "l96", "l128", "lipm", "queues", "order", "order_mode", "order_segs", "prio",
          "ipm_size", "ipm_thru", "ipm_xr", "ipm_full", "fork")
INPUTS = ("horizon", "stance_min", "stance_hint", "order", "ncu", "batch", "full", "xr")

SHIM = r'''
#include "mpcqp_solve_plan.h"
extern "C" void plans(int n, const int* in, int* out) {
  for (int i = 0; i < n; ++i, in += 8, out += 15) {
    const SolvePlan p = solve_plan(SolveInput{in[0], in[1], in[2], in[3], in[4], in[5], in[6] != 0, in[7] != 0});
    const int row[15] = {p.first, p.launch[kClass64], p.launch[kClass96], p.launch[kClass128], p.launch[kClassIpm],
                         p.queues, p.order, p.order_mode, p.order_segs, p.prio, p.ipm_size, p.ipm_thru, p.ipm_xr,
                         p.ipm_full, p.fork};
    for (int k = 0; k < 15; ++k) out[k] = row[k];
  }
}
extern "C" void constants(int* out) {
  const int c[6] = {kCap64, kDenseN, kOrderMin, kOrderMax, kOrderSeg, kIpmPerCU};
  for (int k = 0; k < 6; ++k) out[k] = c[k];
}
'''

C64, C96, C128, IPM = 0, 1, 2, 3
NCU = 256
DENSE_N, MAX_N = 20, 32


@pytest.fixture(scope="module")
def lib():
    so_lib = host_build(SHIM, ("-std=c++17", "-O2"), "plan")
    ip = ctypes.POINTER(ctypes.c_int)
    so_lib.plans.argtypes = [ctypes.c_int, ip, ip]
    so_lib.constants.argtypes = [ip]

    def plans(rows):
        """rows: (n, 8) ints in the order of INPUTS -> (n, 15) ints in the order of FIELDS."""
        rows = np.ascontiguousarray(rows, np.int32).reshape(-1, len(INPUTS))
        out = np.zeros((len(rows), len(FIELDS)), np.int32)
        so_lib.plans(len(rows), rows.ctypes.data_as(ip), out.ctypes.data_as(ip))
        return out

    def constants():
        out = np.zeros(6, np.int32)
        so_lib.constants(out.ctypes.data_as(ip))
        return out.tolist()

    plans.constants = constants
    return plans


def _plan(lib, horizon, batch, stance=(0, 0), order=1, ncu=NCU, full=0, xr=0):
    row = lib([[horizon, stance[0], stance[1], order, ncu, batch, full, xr]])[0]
    return dict(zip(FIELDS, (int(v) for v in row)))


def _expect(got, first, launch, queues, order, prio, ipm=None, fork=False):
    """order: None, or (mode, segments).  ipm: None, or (size index, 'latency' / 'throughput' / 'xr', full);
    the order's and the interior point's fields mean nothing where neither is launched."""
    want = {"first": first, "l64": C64 in launch, "l96": C96 in launch, "l128": C128 in launch, "lipm": IPM in launch,
            "queues": queues, "order": order is not None, "prio": prio, "fork": fork}
    if order is not None:
        want.update(order_mode=order[0], order_segs=order[1])
    assert (ipm is not None) == (IPM in launch)
    if ipm is not None:
        want.update(ipm_size=ipm[0], ipm_thru=ipm[1] == "throughput", ipm_xr=ipm[1] == "xr", ipm_full=ipm[2])
    assert {k: got[k] for k in want} == {k: int(v) for k, v in want.items()}


def test_constants(lib):
    """The constants the policy reads, as DESIGN.md and the kernels' layouts state them."""
    assert lib.constants() == [64, DENSE_N, 64, 8192, 1024, 4]


# ---- literal cases, ncu = 256: a robot has n = 3 * #stance <= 12 N variables; class 64 holds
# n <= 64, class 96 n <= 96, class 128 n <= 128, the interior point the rest and every N > 20.
# Class 64 is resident up to 4 workgroups per CU (1024 robots), the other dense classes 1 (256).

def test_n10_resident_batch(lib):
    # n <= 120: classes 64 / 96 / 128; 1024 robots are resident: priority, no order
    _expect(_plan(lib, 10, 1024), C64, {C64, C96, C128}, queues=True, order=None, prio=True)


def test_n10_queued_batch_takes_the_order(lib):
    # 4096 > 1024 resident: class 64's order (mode 0, its 8 XCD ranges), and no priority
    _expect(_plan(lib, 10, 4096), C64, {C64, C96, C128}, queues=True, order=(0, 8), prio=False)


def test_n10_hint_class64_alone(lib):
    # hint 20: n <= 60, class 64 alone; queues only for the order's perm
    _expect(_plan(lib, 10, 1024, (0, 20)), C64, {C64}, queues=False, order=None, prio=True)
    _expect(_plan(lib, 10, 256, (0, 20)), C64, {C64}, queues=False, order=None, prio=True)
    _expect(_plan(lib, 10, 4096, (0, 20)), C64, {C64}, queues=True, order=(0, 8), prio=False)


@pytest.mark.parametrize("batch,order,prio", [(512, None, True), (1024, None, True), (2048, (0, 8), False)])
def test_n16_all_four_classes_fork(lib, batch, order, prio):
    # n <= 192: all four, class 64 routes, the interior point (queued: latency layout) forks
    _expect(_plan(lib, 16, batch), C64, {C64, C96, C128, IPM}, queues=True, order=order, prio=prio,
            ipm=(0, "latency", False), fork=True)


def test_n16_standing_interior_point_direct(lib):
    # range (64, 64): n = 192 for every robot; more than 3 per CU (768) take the throughput layout
    _expect(_plan(lib, 16, 1024, (64, 64)), IPM, {IPM}, queues=True, order=None, prio=False,
            ipm=(0, "throughput", False))
    _expect(_plan(lib, 16, 769, (64, 64)), IPM, {IPM}, queues=True, order=None, prio=False,
            ipm=(0, "throughput", False))
    _expect(_plan(lib, 16, 768, (64, 64)), IPM, {IPM}, queues=True, order=None, prio=False, ipm=(0, "latency", False))
    _expect(_plan(lib, 16, 768, (64, 64), full=1), IPM, {IPM}, queues=True, order=None, prio=False,
            ipm=(0, "latency", True))


def test_n16_class96_direct(lib):
    # range (22, 32): 66 <= n <= 96, class 96 alone and direct; 2048 > 256 resident: interleaved
    # segments of 1024 (mode 1)
    _expect(_plan(lib, 16, 2048, (22, 32)), C96, {C96}, queues=True, order=(1, 2), prio=False)
    _expect(_plan(lib, 16, 2049, (22, 32)), C96, {C96}, queues=True, order=(1, 3), prio=False)
    _expect(_plan(lib, 16, 256, (22, 32)), C96, {C96}, queues=True, order=None, prio=False)


@pytest.mark.parametrize("batch,order", [(64, None), (256, None), (257, (1, 1)), (4096, (1, 4))])
def test_n16_class128_direct_alone(lib, batch, order):
    # range (33, 42): 99 <= n <= 126
    _expect(_plan(lib, 16, batch, (33, 42)), C128, {C128}, queues=True, order=order, prio=False)


@pytest.mark.parametrize("batch,order,prio", [(64, None, True), (1025, (0, 8), False)])
def test_n16_class64_routes_for_the_fork(lib, batch, order, prio):
    # range (33, 64): 99 <= n <= 192 fits no class-64 robot, but the interior point may be needed
    # beside class 128: class 64 routes the batch so the fork starts at once
    _expect(_plan(lib, 16, batch, (33, 64)), C64, {C64, C96, C128, IPM}, queues=True, order=order, prio=prio,
            ipm=(0, "latency", False), fork=True)


@pytest.mark.parametrize("batch", [1, 64, 1024, 65536])
@pytest.mark.parametrize("stance", [(0, 0), (0, 4), (10, 20)])
def test_n24_interior_point_alone(lib, batch, stance):
    # N > 20: no dense layout holds it, whatever the stance counts; the kMaxN layout, never an order
    _expect(_plan(lib, 24, batch, stance), IPM, {IPM}, queues=True, order=None, prio=False, ipm=(2, "latency", False))


def test_order_off(lib):
    _expect(_plan(lib, 10, 4096, order=0), C64, {C64, C96, C128}, queues=True, order=None, prio=False)
    _expect(_plan(lib, 10, 4096, (0, 20), order=0), C64, {C64}, queues=False, order=None, prio=False)
    _expect(_plan(lib, 16, 2048, (22, 32), order=0), C96, {C96}, queues=True, order=None, prio=False)


def test_class64_order_bounds(lib):
    # below kOrderMin = 64 nothing to balance (8 CUs: 32 resident, so the batch does queue);
    # above 8 * kOrderMax the order kernel's 8 ranges do not hold the batch
    _expect(_plan(lib, 10, 63, (0, 20)), C64, {C64}, queues=False, order=None, prio=True)
    _expect(_plan(lib, 10, 63, (0, 20), ncu=8), C64, {C64}, queues=False, order=None, prio=False)
    _expect(_plan(lib, 10, 64, (0, 20), ncu=8), C64, {C64}, queues=True, order=(0, 8), prio=False)
    _expect(_plan(lib, 10, 8 * 8192, (0, 20)), C64, {C64}, queues=True, order=(0, 8), prio=False)
    _expect(_plan(lib, 10, 8 * 8192 + 1, (0, 20)), C64, {C64}, queues=False, order=None, prio=False)
    # classes 96 / 128 direct have no such cap: one more segment
    _expect(_plan(lib, 16, 8 * 8192 + 1, (22, 32)), C96, {C96}, queues=True, order=(1, 65), prio=False)


@pytest.mark.parametrize("batch", [1, 1024, 4096])
def test_xr_layout_at_n20(lib, batch):
    # a cross-leg R: the XR instantiation (always full weights) of the kDenseN layout
    _expect(_plan(lib, 20, batch, full=1, xr=1), C64, {C64, C96, C128, IPM}, queues=True,
            order=(0, 8) if batch > 1024 else None, prio=batch <= 1024, ipm=(1, "xr", True), fork=True)
    _expect(_plan(lib, 16, 1024, (64, 64), full=1, xr=1), IPM, {IPM}, queues=True, order=None, prio=False,
            ipm=(0, "xr", True))


# ---- invariants over the grid

BATCHES = (1, 63, 64, 256, 257, 1024, 1025, 65536, 65537)


def _grid(horizon):
    ranges = [(mn, 0) for mn in range(4 * horizon + 1)]
    ranges += [(mn, hint) for hint in range(1, 4 * horizon + 1) for mn in range(hint + 1)]
    ranges = np.array(ranges, np.int32)
    rest = np.array([(order, NCU, batch, full, xr) for batch in BATCHES for order in (0, 1) for full in (0, 1)
                     for xr in (0, 1)], np.int32)
    rows = np.empty((len(ranges), len(rest), len(INPUTS)), np.int32)
    rows[:, :, 0] = horizon
    rows[:, :, 1:3] = ranges[:, None, :]
    rows[:, :, 3:] = rest[None, :, :]
    return rows.reshape(-1, len(INPUTS))


@pytest.mark.parametrize("horizon", range(1, MAX_N + 1))
def test_invariants(lib, horizon):
    rows = _grid(horizon)
    p = dict(zip(FIELDS, lib(rows).T))
    i = dict(zip(INPUTS, rows.T))
    launch = np.stack([p["l64"], p["l96"], p["l128"], p["lipm"]], axis=1).astype(bool)
    first, batch = p["first"], i["batch"]
    for k in ("l64", "l96", "l128", "lipm", "queues", "order", "prio", "ipm_thru", "ipm_xr", "ipm_full", "fork"):
        assert np.isin(p[k], (0, 1)).all(), k
    assert np.isin(first, (C64, C96, C128, IPM)).all() and np.isin(p["ipm_size"], (0, 1, 2)).all()

    # every class whose band of variable counts meets [3 min, nmax] is launched (or routed to)
    nmin = 3 * i["stance_min"]
    nmax = np.where(i["stance_hint"] > 0, np.minimum(3 * i["stance_hint"], 12 * horizon), 12 * horizon)
    if horizon > DENSE_N:
        assert launch[:, IPM].all()
    else:
        for cls, lo, hi in ((C64, 0, 64), (C96, 65, 96), (C128, 97, 128), (IPM, 129, 12 * MAX_N)):
            needed = (nmin <= hi) & (nmax >= lo)
            assert launch[needed, cls].all(), cls
    # no dense class at N > 20
    if horizon > DENSE_N:
        assert not launch[:, :IPM].any()
    # the first class is launched and none before it: at most one class is direct, the first launched
    assert launch[np.arange(len(rows)), first].all()
    for cls in (C96, C128, IPM):
        assert not launch[first == cls, :cls].any(), cls
    # the order: never for the interior point, never for a resident batch, only on request
    resident = np.where(first == C64, 4, 1) * NCU
    on = p["order"] == 1
    assert (first[on] != IPM).all() and (batch[on] > resident[on]).all() and (i["order"][on] == 1).all()
    assert (p["order_mode"][on] == (first[on] != C64)).all()
    segs = np.where(first == C64, 8, (batch + 1023) // 1024)
    assert (p["order_segs"][on] == segs[on]).all()
    # priority: class 64 first, the batch resident
    pr = p["prio"] == 1
    assert (first[pr] == C64).all() and (batch[pr] <= 4 * NCU).all()
    # the interior point's layout: the size follows the horizon; throughput only at N <= 16,
    # without XR, direct; XR is the caller's and always full
    assert (p["ipm_size"] == (0 if horizon <= 16 else 1 if horizon <= DENSE_N else 2)).all()
    th = p["ipm_thru"] == 1
    assert not th.any() or horizon <= 16
    assert (p["ipm_xr"][th] == 0).all() and (first[th] == IPM).all() and (batch[th] > 3 * NCU).all()
    assert (p["ipm_xr"] == i["xr"]).all() and (p["ipm_full"] == (i["full"] | i["xr"])).all()
    # the fork: the interior point beside a first class that is not it
    assert ((p["fork"] == 1) == (launch[:, IPM] & (first != IPM))).all()
    # queues whenever a class other than class 64 launches (each takes its queue) or the order is on
    assert (p["queues"][launch[:, C96:].any(axis=1) | on] == 1).all()

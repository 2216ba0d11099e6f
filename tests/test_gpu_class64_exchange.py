"""Class 64's drops and the additions that follow them: a pass that drops a blocking slot l
leaves the pending row p pending, and p's next step either adds it -- into the freed slot or a
lower free one -- or drops again.  These are the two passes an "exchange pass" would merge
("finishing a dropped slot's pending row": built, measured, left out); the cases
hold the kernel to the oracle, to the iteration cap's rule and to launch-shape independence
exactly where such a pass acts, whichever way the loop takes them.

Every case is at N = 10 against the float64 oracle with the tail test's helpers and bound.  The
robots are picked on the CPU by the simulation of the kernel's loop with the drop and the add
merged (tools/gi_sim.py, simulate(..., kmax=2, merge=True): the same decisions, iterations and
drops as the plain loop), whose `events` list every pass as (iterations before it, kind, dropped
slot l, slot q the row went into, occupied slots before); each pick's property is asserted in
its case builder.

Two things the cases cannot show.  The row goes into the FIRST free slot, and l has just been
freed, so q <= l always: with more than 32 slots active (wave 1's R rows live) the cases are l in
wave 1's rows with q in wave 0's, l = q in wave 1's rows, and l = q in wave 0's rows; q in wave
1's rows with l in wave 0's cannot happen.  And no one-foot-step robot (n = 3) of the small-case
construction drops a slot: 60 candidates, velocity errors enlarged 8 x to 1024 x, all reach their
optimum by two or three additions (one foot-step has no pair step and at most three active
rows); the n = 3 robots here run the loop's add passes only, the n = 6 ones drop and add."""
import functools
import os
import sys

import numpy as np
import pytest

from helpers import rel_err_u0
from test_gpu_class64_tail import (N, ROW_CANDIDATES, ROW_SCALES, ROW_SEED, SMALL_SEED, TOL_ACHIEVED,
                                   _enlarge_velocity_error, _solve, _take, _with_oracle)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

# of the tail test's 60 candidates (make_batch(60, 10, seed=6400, trot / pace), velocity errors
# enlarged by ROW_SCALES[b % 5]); what each is picked for is asserted in _exchange_case
PICKS = (15, 41, 18, 42, 38, 34, 33, 52)
CAP_ROBOT = 0   # PICKS[0]: 32 iterations, a drop and its add at 21 / 22 and at 25 / 26, a single add last
# the small-case construction (12 robots, 1 + b % 2 stance foot-steps, velocity errors 8 x)
SMALL_PICKS = (6, 10, 9, 7)
STATUS_OK, STATUS_MAX_ITER = 0, 1


def _simulate(bt):
    import gi_sim
    out = []
    for b in range(len(bt["x0"])):
        qp = gi_sim.robot_qp(bt, b, N)
        r = gi_sim.simulate(*qp, kmax=2, merge=True)
        assert "x" in r, (b, r)
        out.append((qp[0].shape[0], r))
    return out


def _merged(r):
    return [e for e in r["events"] if e[1] == "merged"]


@functools.lru_cache(maxsize=None)
def _exchange_case():
    from mpcqp.synthetic import make_batch
    bt = make_batch(ROW_CANDIDATES, N, seed=ROW_SEED, gaits=("trot10", "pace10"), robots=("a1",))
    for b in range(ROW_CANDIDATES):
        _enlarge_velocity_error(bt, b, ROW_SCALES[b % len(ROW_SCALES)])
    bt = _take(bt, PICKS)
    sim = _simulate(bt)
    assert all(n == 60 for n, _ in sim)
    ev = [r["events"] for _, r in sim]
    mg = [_merged(r) for _, r in sim]
    assert all(q <= l for m in mg for _, _, l, q, _ in m)
    # the freed slot takes the row (q == l); a lower free slot does (q < l)
    assert any(q == l for _, _, l, q, _ in mg[0]), mg[0]
    assert any(q < l for _, _, l, q, _ in mg[1]), mg[1]
    assert any(q < l for _, _, l, q, _ in mg[2]) and any(q == l for _, _, l, q, _ in mg[2]), mg[2]
    # a drop, another drop, then the add (the second drop pass ends as a plain drop)
    kinds = [e[1] for e in ev[3]]
    assert any(kinds[i:i + 3] == ["drop", "drop", "merged"] for i in range(len(kinds))), kinds
    # more than 32 slots active: l in wave 1's rows and q in wave 0's; l = q in wave 1's rows; l = q
    # in wave 0's rows
    assert any(nocc > 32 and l >= 32 and q < 32 for _, _, l, q, nocc in mg[4]), mg[4]
    assert any(nocc > 32 and l >= 32 and q == l for _, _, l, q, nocc in mg[5]), mg[5]
    assert any(nocc > 32 and l < 32 for _, _, l, q, nocc in mg[5]), mg[5]
    assert any(nocc > 32 and l >= 32 for _, _, l, q, nocc in mg[6]), mg[6]
    return bt, _with_oracle(bt), tuple(r for _, r in sim)


@functools.lru_cache(maxsize=None)
def _small_case():
    from mpcqp.synthetic import make_batch
    B = 12
    bt = make_batch(B, N, seed=SMALL_SEED, gaits=("trot10", "pace10"), robots=("a1",))
    rng = np.random.default_rng(SMALL_SEED + 1)
    for b in range(B):
        c = np.zeros(4 * N, dtype=np.float32)
        c[rng.choice(4 * N, size=1 + b % 2, replace=False)] = 1.0
        bt["contact"][b] = c.reshape(N, 4)
        _enlarge_velocity_error(bt, b, 8.0)
    bt = _take(bt, SMALL_PICKS)
    sim = _simulate(bt)
    assert [n for n, _ in sim] == [3, 3, 6, 6], [n for n, _ in sim]
    assert len(_merged(sim[2][1])) >= 1, sim[2][1]["events"]   # an n = 6 robot that drops and adds
    assert all(r["drops"] == 0 and len(r["active"]) >= 1 for _, r in sim[:2])   # see the module's docstring
    return bt, _with_oracle(bt)


def _expected_under_cap(events, total, cap):
    """Status and reported count under max_iter = cap by the rule at the loop's head (a pass
    starts only while the count after it is begun stays within the cap; a cap between a drop
    and its add lets the drop through and refuses the add, merged into one pass or not).  The
    count is the steps executed (include/mpcqp.h): the refused pass is not one of them."""
    for before, kind, _, _, _ in events:
        if before + 1 > cap:
            return STATUS_MAX_ITER, before
        if kind == "merged" and before + 1 == cap:
            return STATUS_MAX_ITER, cap
    return STATUS_OK, total


def _check(bt, ref):
    from mpcqp import LinearMpc
    u0, U, status, iters = _solve(LinearMpc(horizon=N, robot="a1"), bt)
    errs = [max(rel_err_u0(u0[b], ref[b][:12]), rel_err_u0(U[b], ref[b])) for b in range(len(ref))]
    print("iterations", iters.tolist(), "worst relative error per robot:", " ".join(f"{e:.1e}" for e in errs))
    assert (status == 0).all(), status
    assert max(errs) < TOL_ACHIEVED, (int(np.argmax(errs)), max(errs))
    return iters


def test_cases_are_what_they_claim():
    """The case builders' asserts and the oracle's optimum run on the CPU; merging a drop and its add
    changes no decision of the simulated loop (iterations, drops and the optimum are those of
    the plain loop); the cap rule on the simulated passes."""
    import gi_sim
    bt, ref, sims = _exchange_case()
    assert np.isfinite(ref).all() and len(ref) == len(PICKS)
    for b, r in enumerate(sims):
        plain = gi_sim.simulate(*gi_sim.robot_qp(bt, b, N), kmax=2)
        assert plain["it"] == r["it"] and plain["drops"] == r["drops"] and plain["active"] == r["active"], b
        assert plain["passes"] - r["passes"] == r["kinds"]["merged"] > 0, b
        assert np.abs(plain["x"] - r["x"]).max() <= 1e-9 * max(1.0, np.abs(r["x"]).max()), b
    bt, ref = _small_case()
    assert np.isfinite(ref).all() and len(ref) == len(SMALL_PICKS)
    r = sims[CAP_ROBOT]
    between = [e[0] + 1 for e in _merged(r)]   # the caps that fall between a drop and its add
    assert between and r["events"][-1][1] != "pair"
    for cap in between:
        assert _expected_under_cap(r["events"], r["it"], cap) == (STATUS_MAX_ITER, cap)
    assert _expected_under_cap(r["events"], r["it"], r["it"]) == (STATUS_OK, r["it"])
    assert all(_expected_under_cap(r["events"], r["it"], cap)[0] == STATUS_MAX_ITER for cap in range(1, r["it"]))


@pytest.mark.gpu
def test_drop_then_add_against_the_oracle():
    """q == l and q < l, a drop followed by another drop and then the add, and drops with their
    adds while more than 32 slots are active, on both sides of the waves' row split."""
    bt, ref, _ = _exchange_case()
    _check(bt, ref)


@pytest.mark.gpu
def test_small_n():
    """n = 3 (add passes only) and n = 6 (a drop and its add with one register row of slots)."""
    _check(*_small_case())


@pytest.mark.gpu
def test_iteration_caps():
    """One dropping robot at B = 1 under max_iter = 1 ... its full count + 1 (per-robot caps do
    not exist: one engine per cap).  At or above the full count the result is bitwise the uncapped
    one; below it the status is MAX_ITER and the reported count follows the loop-head rule,
    including the caps that fall between a drop and its add.  The passes are the
    simulated ones: the robot is one whose count on the device is the simulation's (the f32 row
    keys send some robots down another path of equal right), which the test asserts first."""
    from mpcqp import LinearMpc
    bt, _, sims = _exchange_case()
    one = _take(bt, [CAP_ROBOT])
    r = sims[CAP_ROBOT]
    free = _solve(LinearMpc(horizon=N, robot="a1"), one)
    total = int(free[3][0])
    print("uncapped iterations", total, "simulated", r["it"], "simulated passes", [(e[0], e[1]) for e in r["events"]])
    assert free[2][0] == STATUS_OK and total == r["it"]
    for cap in range(1, total + 2):
        got = _solve(LinearMpc(horizon=N, robot="a1", max_iter=cap), one)
        status, count = _expected_under_cap(r["events"], total, cap)
        print("cap", cap, "status", int(got[2][0]), "iterations", int(got[3][0]), "expected", status, count)
        assert (int(got[2][0]), int(got[3][0])) == (status, count), cap
        assert cap < total or all(np.array_equal(x, y) for x, y in zip(got, free)), cap
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), cap


@pytest.mark.gpu
def test_launch_shape_cannot_change_a_result():
    """The dropping robots as one batch, one per launch, alone in a padded batch (the robot
    followed by seven copies of another, so it is at times its CU's heaviest and at times not)
    and on two streams: u0, U, status and iterations are bitwise equal."""
    import torch
    from mpcqp import LinearMpc
    bt, _, _ = _exchange_case()
    B = len(bt["x0"])
    eng = LinearMpc(horizon=N, robot="a1")
    ref = _solve(eng, bt)
    for b in range(B):
        got = _solve(eng, _take(bt, [b]))
        assert all(np.array_equal(x[0], y[b]) for x, y in zip(got, ref)), b
        pad = [b] + [(b + 1) % B] * 7
        got = _solve(eng, _take(bt, pad))
        assert all(np.array_equal(x, y[pad]) for x, y in zip(got, ref)), b
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    dev = {k: torch.as_tensor(v).to("cuda:0") for k, v in bt.items()}
    torch.cuda.synchronize()
    outs = [eng.solve(dev["x0"], dev["xref"], dev["contact"], dev["feet"], robot=dev["robot"], return_all=True,
                      stream=streams[k % 2]) for k in range(4)]   # no host synchronisation in between
    torch.cuda.synchronize()
    for k, res in enumerate(outs):
        got = (res.u0.cpu().numpy(), res.U.cpu().numpy().reshape(B, -1), res.status.cpu().numpy(),
               res.iterations.cpu().numpy())
        assert all(np.array_equal(x, y) for x, y in zip(got, ref)), k

"""Class 64's active-set slots and its setup priority: robots whose active sets end in each
register-row band of R's tiles (slot s is register row s & 3 of tile row s >> 2; beyond 32
slots wave 1's rows go live), robots that drop slots and add again, one-slot robots, and the
same robots solved in different launch shapes -- the heaviest robot of each CU runs its H tile
and sweep at a raised wave priority, which is a schedule and may never change a result.

Every case is at N = 10 against the float64 oracle, generated once per process from the seeds
below; the robots are picked on the CPU by a simulation of the kernel's loop
(tools/gi_sim.py) and each pick is asserted in its case builder, so a case that exists
exercises what it claims."""
import functools
import os
import sys

import numpy as np
import pytest

from helpers import oracle_solution, rel_err_u0

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

TOL_ACHIEVED = 1e-5   # test_gpu_class64_setup.TOL_ACHIEVED
N = 10

# Register-row bands of the final active count: wave 0's R tile has ceil(count / 8) live register
# rows up to 32 slots, beyond which wave 1's rows go live.
BANDS = ((1, 8), (9, 16), (17, 24), (25, 32), (33, 60))
# make_batch(ROW_CANDIDATES, 10, seed=ROW_SEED, trot / pace), robot b's xy velocity error
# enlarged by ROW_SCALES[b % 5]; ROW_PICKS: two robots per band, in band order (their simulated
# final counts 3, 8 | 11, 13 | 18, 24 | 32, 28 | 50, 53; robots 52, 41, 46, 3 and 34 drop 7, 3, 5,
# 12 and 11 slots on the way)
ROW_SEED, ROW_CANDIDATES = 6400, 60
ROW_SCALES = (1.0, 2.0, 3.0, 5.0, 8.0)
ROW_PICKS = (10, 50, 25, 55, 52, 41, 46, 15, 3, 34)
# make_batch(12, 10, seed=SMALL_SEED, trot / pace), robot b's contact table replaced by 1 + b % 2
# stance foot-steps drawn with default_rng(SMALL_SEED + 1), its xy velocity error enlarged 8 x;
# SMALL_PICKS: two n = 3 robots and two n = 6 robots with a binding friction row
SMALL_SEED = 6500
SMALL_PICKS = (6, 10, 7, 5)


def _enlarge_velocity_error(bt, b, scale):
    bt["x0"][b, 9:11] = bt["xref"][b, 0, 9:11] + np.float32(scale) * (bt["x0"][b, 9:11] - bt["xref"][b, 0, 9:11])


def _take(bt, idx):
    return {k: np.ascontiguousarray(v[list(idx)]) for k, v in bt.items()}


def _simulate(bt):
    """The kernel's loop on the CPU (pair steps): per robot the final active rows (5 per
    foot-step: 4 friction rows, then fz <= fz_max) and the number of dropped slots."""
    import gi_sim
    out = []
    for b in range(len(bt["x0"])):
        qp = gi_sim.robot_qp(bt, b, N)
        r = gi_sim.simulate(*qp, kmax=2)
        assert "x" in r, (b, r)
        out.append((qp[0].shape[0], r["active"], r["drops"]))
    return out


def _with_oracle(bt):
    return np.stack([oracle_solution(bt, b, N)[0] for b in range(len(bt["x0"]))])


@functools.lru_cache(maxsize=None)
def _row_case():
    from mpcqp.synthetic import make_batch
    bt = make_batch(ROW_CANDIDATES, N, seed=ROW_SEED, gaits=("trot10", "pace10"), robots=("a1",))
    for b in range(ROW_CANDIDATES):
        _enlarge_velocity_error(bt, b, ROW_SCALES[b % len(ROW_SCALES)])
    bt = _take(bt, ROW_PICKS)
    sim = _simulate(bt)
    assert all(n == 60 for n, _, _ in sim), sim
    counts = [len(a) for _, a, _ in sim]
    for i, (lo, hi) in enumerate(BANDS):   # two robots per register-row band
        assert lo <= counts[2 * i] <= hi and lo <= counts[2 * i + 1] <= hi, (i, counts)
    # robots that free >= 3 slots while rows beyond the first register row are live and add
    # again afterwards (every drop is followed by the pending row's addition)
    redo = [b for b, (_, a, drops) in enumerate(sim) if drops >= 3 and len(a) > 8]
    assert len(redo) >= 2, sim
    return bt, _with_oracle(bt)


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
    assert [n for n, _, _ in sim] == [3, 3, 6, 6], sim
    for _, active, _ in sim:   # a binding friction row, at most one register row of slots
        assert 1 <= len(active) <= 8 and any(r % 5 < 4 for r in active), sim
    assert any(len(a) == 1 for _, a, _ in sim), sim   # one live slot
    return bt, _with_oracle(bt)


def _solve(eng, bt, stream=None):
    import torch
    res = eng.solve(bt["x0"], bt["xref"], bt["contact"], bt["feet"], robot=bt["robot"], return_all=True,
                    stream=stream)
    torch.cuda.synchronize()
    B = len(bt["x0"])
    return (res.u0.cpu().numpy(), res.U.cpu().numpy().reshape(B, -1), res.status.cpu().numpy(),
            res.iterations.cpu().numpy())


def _check(bt, ref):
    from mpcqp import LinearMpc
    u0, U, status, iters = _solve(LinearMpc(horizon=N, robot="a1"), bt)
    errs = [max(rel_err_u0(u0[b], ref[b][:12]), rel_err_u0(U[b], ref[b])) for b in range(len(ref))]
    print("iterations", iters.tolist(), "worst relative error per robot:", " ".join(f"{e:.1e}" for e in errs))
    assert (status == 0).all(), status
    assert max(errs) < TOL_ACHIEVED, (int(np.argmax(errs)), max(errs))


def test_cases_are_what_they_claim():
    """The case builders' asserts (bands, drops, binding rows) and the oracle's optimum run on
    the CPU."""
    for bt, ref in (_row_case(), _small_case()):
        assert np.isfinite(ref).all() and len(ref) == len(bt["x0"])


@pytest.mark.gpu
def test_register_row_bands():
    """Final active counts in 1-8, 9-16, 17-24, 25-32 and > 32, two robots each; five of them drop
    3-12 slots and re-use the freed ones while higher register rows are live."""
    _check(*_row_case())


@pytest.mark.gpu
def test_small_n_one_register_row():
    """n = 3 and n = 6 (1 and 2 stance foot-steps) with a binding friction row."""
    _check(*_small_case())


@pytest.mark.gpu
def test_launch_shape_cannot_change_a_result():
    """The ten robots as one batch, one per launch, and as a batch of 40 (the ten four times in
    permuted order, so each is at times its CU's heaviest robot and at times not): u0, status
    and iterations are bitwise equal."""
    from mpcqp import LinearMpc
    bt, _ = _row_case()
    B = len(bt["x0"])
    eng = LinearMpc(horizon=N, robot="a1")
    u0, _, st, it = _solve(eng, bt)
    for b in range(B):
        u1, _, s1, i1 = _solve(eng, _take(bt, [b]))
        assert np.array_equal(u1[0], u0[b]) and s1[0] == st[b] and i1[0] == it[b], b
    order = np.concatenate([np.random.default_rng(6600 + k).permutation(B) for k in range(4)])
    u4, _, s4, i4 = _solve(eng, _take(bt, order))
    assert np.array_equal(u4, u0[order]) and np.array_equal(s4, st[order]) and np.array_equal(i4, it[order])


@pytest.mark.gpu
def test_two_engines_and_two_streams_alternate():
    """Two engines on one device, and one engine on two streams, solve the same batch
    alternately for 8 launches: every result is bitwise that of a single solve."""
    import torch
    from mpcqp import LinearMpc
    bt, _ = _row_case()
    a, b = LinearMpc(horizon=N, robot="a1"), LinearMpc(horizon=N, robot="a1")
    ref = _solve(a, bt)
    for k in range(8):
        got = _solve((a, b)[k % 2], bt)
        assert all(np.array_equal(x, y) for x, y in zip(got, ref)), k
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    dev = {k: torch.as_tensor(v).to("cuda:0") for k, v in bt.items()}
    torch.cuda.synchronize()
    outs = [a.solve(dev["x0"], dev["xref"], dev["contact"], dev["feet"], robot=dev["robot"], return_all=True,
                    stream=streams[k % 2]) for k in range(8)]   # no host synchronisation in between
    torch.cuda.synchronize()
    for k, res in enumerate(outs):
        got = (res.u0.cpu().numpy(), res.U.cpu().numpy().reshape(len(ref[0]), -1), res.status.cpu().numpy(),
               res.iterations.cpu().numpy())
        assert all(np.array_equal(x, y) for x, y in zip(got, ref)), k

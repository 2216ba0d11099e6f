"""The interior-point class (csrc/mpcqp_ipm.h, solve_robot_ipm) at its internal boundaries: every
horizon of its three LDS layouts (NM = 16 / 20 / 32), the partial MFMA tile of stage_gemm (16
stages per tile), the lane tails of the foot-step loops (one foot-step per lane in registers at
NM = 16, up to two in LDS above), the smallest problems of the class, the throughput layout below
N = 16 and with full weights, and the warm start's memory on a contact table that moves.

  A  N = 11 .. 32, six robots per horizon through the default routing (class 64 stages and routes
     at N <= 20, the interior point takes the batch at N > 20): standing; standing with stage
     N // 2, stage 0 or stage N - 1 in flight; a trot whose first stages are full stance until
     3 S > 128; a dense random table.  At N = 12, 17, 21, 31 again with full Q and leg-block R and
     with a cross-leg R.  (N = 11: a standing robot with one stage in flight has S = 40, n = 120
     -- class 128, no interior point; those three robots are held to the dense classes' guard.
     From N = 12 on every robot of the sweep is interior point.)
  B  stance counts at which a lane's second foot-step starts or stops existing, foot-steps
     cleared once from the front and once from the back of a standing table: N = 17 S = 63, 64,
     65, 68; N = 20 S = 79; N = 32 S = 127; N = 31 S = 123; N = 11 S = 43, 44; N = 16 S = 63.
  C  N = 21 and 29: one foot-step (S = 1), one leg at two consecutive stages (S = 2) and one
     full stage (S = 4), each at the first, a middle and the last stage; nothing else in stance.
  D  B = 3 CUs + 16 standing robots promised as such: N = 12, 15 diagonal weights, N = 16, 13
     full weights (mpcqp_kernel_ipm<true, 16, true>), sampled against the oracle and against the
     latency layout; the plan (solve_plan, compiled for the host) is asserted to pick them.
  E  warm start at N = 24 on tables advancing one step per tick (four trots, a pace, a standing
     robot), the memory's bytes after every tick, every robot handed the pacing table, a memory
     of three rows for six robots, and N = 13 (bytes 4 N .. 63 of a 16-stage layout's row).

Bounds are test_gpu_parity's: TOL_U0 per robot on u0 and U, TOL_ACHIEVED_IPM on the worst robot
of a case (TOL_ACHIEVED for N = 11's three class-128 robots), every status OK, iterations > 0 for
a robot the class solved.  The oracle (float64, CPU) solves every case once per process; the
builders' asserts (stance counts, classes) and those solves are the unmarked tests of this file.

Measured on the MI355X (worst relative error of a part's worst robot, largest factorisation count):
  A  diagonal weights, N = 11 .. 32: 1.5e-5 (N = 21; 1.2e-5 at N = 32, below 1e-5 elsewhere), 14
     factorisations (the three class-128 robots of N = 11: 4.5e-7, up to 86 active-set steps);
     full weights / cross-leg R at N = 12, 17, 21, 31: 1.4e-5 / 1.3e-5 (N = 21), 13
  B  3.2e-6 (N = 32, S = 127), 13 factorisations
  C  3.3e-6 (N = 21, one full stage), 15 factorisations (N = 29, S = 1)
  D  1.2e-5 (N = 16 full weights; the latency layout gives the same figures), 19 factorisations
     in a batch of 784
  E  moving schedule 1.6e-5 (tick 0), later ticks below 2e-6; factorisations per tick over the six
     robots, warm [62, 55, 67, 67, 69, 45, 63], cold [62, 64, 61, 63, 63, 61, 64]: on a trot whose
     table moves a remembered set costs up to 20 factorisations where the cold start takes 10 or
     11, the standing robot 1 or 2, the pace 2 to 4; N = 13 standing 7.4e-7, [46, 5, 5] per tick.

Before csrc/mpcqp_ipm_foot.h's inv3 became an L D L^T inverse, A's trot at N = 24, C's full stage
at the first and the last step of N = 29 and E's tick 1 ended with MPCQP_STATUS_MAX_ITER (60
iterations, up to 73 factorisations; C's S = 1 and S = 2 in mid-horizon took 38 and 63):
tools/ipm_proto.py verifies all of them in 9 to 15 iterations.  The adjugate inverse returned an
indefinite foot-step weight once one row's lambda / s passed ~1e6 on a tilted cone
(tests/test_ipm_foot.py), which a robot reaches only when its first polish does not verify."""
import functools

import numpy as np
import pytest

from helpers import _cross_leg_weights, _full_weights, oracle_solution, rel_err_u0
from test_solve_plan import _plan, lib   # noqa: F401 (lib: the module fixture that compiles solve_plan for the host)

TOL_U0 = 1e-4             # test_gpu_parity.TOL_U0: the project's contract (1e-3 floor on the denominator)
TOL_ACHIEVED = 1e-5       # test_gpu_parity.TOL_ACHIEVED: the dense classes' regression guard
TOL_ACHIEVED_IPM = 5e-5   # test_gpu_parity.TOL_ACHIEVED_IPM: the interior-point class's
WARM_BYTES = 128          # MPCQP_WARM_BYTES
PLAN_IPM = 3              # test_solve_plan.IPM: the class index of SolvePlan.first
MI355X_CUS = 256
SEED = 8100

SWEEP = tuple(range(11, 33))
WEIGHTED = (12, 17, 21, 31)   # inside NM = 16; a partial tile of 1 stage; the smallest NM = 32; a partial tile of 15
KINDS = ("full", "xleg")
GAIT_MIX = ("trot10", "pace10", "bound8")


def _copy(bt):
    return {k: v.copy() for k, v in bt.items()}


def _stance(bt):
    return (bt["contact"] > 0).reshape(len(bt["x0"]), -1).sum(1)


def _is_ipm(N, stance):
    return N > 20 or 3 * int(stance) > 128


def _weights(kind, N):
    """{} (the reference's diagonals), full Q with a leg-block R, or full Q with a cross-leg R."""
    if kind == "diag":
        return {}
    Q, R = _full_weights(N) if kind == "full" else _cross_leg_weights(N)
    return {"Q": Q, "R": R}


def _fleet(B, N, seed):
    """B seeded robots as in test_random_contact_patterns_every_class: A1 and Aliengo, normals
    tilted up to 10 degrees, per-robot mu and fz_max; the contact tables are set by the caller."""
    from mpcqp.params import R_FZMAX, R_MU
    from mpcqp.synthetic import make_batch
    bt = make_batch(B, N, seed=seed, gaits=GAIT_MIX, robots=("a1", "aliengo"), tilt_deg=10.0)
    rng = np.random.default_rng(seed + 1)
    bt["robot"][:, R_MU] = rng.uniform(0.2, 1.0, B).astype(np.float32)
    bt["robot"][:, R_FZMAX] = rng.uniform(120.0, 600.0, B).astype(np.float32)
    return bt


def _oracle(bt, robots, N, kind="diag"):
    out = {b: oracle_solution(bt, b, N, **_weights(kind, N))[0] for b in robots}
    assert all(np.isfinite(x).all() for x in out.values())
    return out


# ---- A: the horizon sweep
@functools.lru_cache(maxsize=None)
def _sweep(N):
    from mpcqp.synthetic import gait_table
    bt = _fleet(6, N, SEED + N)
    c = bt["contact"]
    c[:4] = 1.0
    c[1, N // 2] = 0.0                    # E_k = 0 in mid-horizon
    c[2, 0] = 0.0                         # the first step of the forward recursion, the last of the backward
    c[3, N - 1] = 0.0                     # and the other end
    c[4] = gait_table("trot10", N % 10, N)
    k = 0
    while 3 * int(c[4].sum()) <= 128:     # near standing: the shape c128 has one class below
        c[4, k] = 1.0
        k += 1
    for draw in range(1000):              # a dense random table, interior point at every N
        rng = np.random.default_rng(SEED + 1000 * N + draw)
        c[5] = (rng.random((N, 4)) < rng.uniform(0.75, 1.0)).astype(np.float32)
        if 0 < c[5].sum() < 4 * N and _is_ipm(N, c[5].sum()):
            break
    S = _stance(bt)
    assert S[0] == 4 * N and (S[1:4] == 4 * N - 4).all() and S[5] < 4 * N, (N, S)
    assert not c[1, N // 2].any() and not c[2, 0].any() and not c[3, N - 1].any()
    if N <= 20:
        assert 3 * S[4] > 128 and 3 * S[5] > 128, (N, S)
        # 3 (4 N - 4) > 128 from N = 12 on; at N = 11 a stage in flight leaves n = 120, class 128
        assert [not _is_ipm(N, s) for s in S] == [False, N == 11, N == 11, N == 11, False, False], (N, S)
    return bt


def _sweep_ipm(N):
    return [_is_ipm(N, s) for s in _stance(_sweep(N))]


@functools.lru_cache(maxsize=None)
def _sweep_ref(N, kind="diag"):
    return _oracle(_sweep(N), range(6), N, kind)


# ---- B: lane tails.  N -> (stance count, foot-steps cleared from the "front" / "back" / nowhere)
TAILS = {
    17: ((63, "front"), (63, "back"), (64, "front"), (64, "back"), (65, "front"), (65, "back"), (68, None)),
    20: ((79, "front"), (79, "back")),
    32: ((127, "front"), (127, "back")),
    31: ((123, "front"), (123, "back")),
    11: ((43, "front"), (43, "back"), (44, None)),
    16: ((63, "front"), (63, "back")),
}


@functools.lru_cache(maxsize=None)
def _tails(N):
    spec = TAILS[N]
    bt = _fleet(len(spec), N, SEED + 100 + N)
    bt["contact"][:] = 1.0
    for b, (S, side) in enumerate(spec):
        flat = bt["contact"][b].reshape(-1)
        drop = 4 * N - S
        assert (drop == 0) == (side is None)
        if side == "front":
            flat[:drop] = 0.0    # the foot-step that becomes the 65th moves with the side
        elif side == "back":
            flat[4 * N - drop:] = 0.0
    S = _stance(bt)
    assert tuple(S) == tuple(s for s, _ in spec), (N, S)
    assert all(_is_ipm(N, s) for s in S), (N, S)
    return bt


@functools.lru_cache(maxsize=None)
def _tails_ref(N):
    return _oracle(_tails(N), range(len(TAILS[N])), N)


# ---- C: the smallest problems of the class
SMALL_N = (21, 29)
SMALL = tuple((count, where) for count in (1, 2, 4) for where in ("first", "middle", "last"))


@functools.lru_cache(maxsize=None)
def _small(N):
    bt = _fleet(len(SMALL), N, SEED + 200 + N)
    bt["contact"][:] = 0.0
    for b, (count, where) in enumerate(SMALL):
        stages = 2 if count == 2 else 1
        k = {"first": 0, "middle": N // 2, "last": N - stages}[where]
        if count == 4:
            bt["contact"][b, k] = 1.0                 # one full stage in stance
        else:
            bt["contact"][b, k:k + stages, b % 4] = 1.0   # one leg, at one stage or at two
    S = _stance(bt)
    assert tuple(S) == tuple(count for count, _ in SMALL), (N, S)
    assert (bt["contact"][[0, 3, 6], 0] > 0).any(axis=1).all() and (bt["contact"][[2, 5, 8], N - 1] > 0).any(axis=1).all()
    return bt


@functools.lru_cache(maxsize=None)
def _small_case(N, count):
    """The three robots of ``_small(N)`` with that stance count, and their optima."""
    pick = [b for b, (c, _) in enumerate(SMALL) if c == count]
    sub = {k: v[pick] for k, v in _small(N).items()}
    assert (_stance(sub) == count).all()
    return sub, _oracle(sub, range(len(pick)), N)


# ---- D: the throughput layout
THRU = ((12, "diag"), (15, "diag"), (16, "full"), (13, "full"))


def _thru_pick(B):
    return [0, 1, B // 2, B - 2, B - 1]


@functools.lru_cache(maxsize=None)
def _thru(N, ncu):
    from mpcqp.synthetic import make_batch
    B = 3 * ncu + 16
    bt = make_batch(B, N, seed=SEED + 300 + N, gaits=("trot10",), robots=("a1", "aliengo"), tilt_deg=5.0)
    bt["contact"][:] = 1.0
    assert (_stance(bt) == 4 * N).all() and 3 * 4 * N > 128
    return bt


@functools.lru_cache(maxsize=None)
def _thru_ref(N, kind, ncu):
    bt = _thru(N, ncu)
    return _oracle(bt, _thru_pick(len(bt["x0"])), N, kind)


def _assert_plans_throughput(plans, N, kind, ncu):
    """These inputs reach the throughput kernel: the interior point first, direct, 16-stage
    layout, ipm_thru, and ipm_full exactly with full weights."""
    B = 3 * ncu + 16
    got = _plan(plans, N, B, (4 * N, 4 * N), ncu=ncu, full=int(kind == "full"))
    want = {"first": PLAN_IPM, "lipm": 1, "l64": 0, "l96": 0, "l128": 0, "ipm_size": 0, "ipm_thru": 1, "ipm_xr": 0,
            "ipm_full": int(kind == "full"), "fork": 0}
    assert {k: got[k] for k in want} == want, (N, kind, ncu, got)


# ---- E: warm start on a moving schedule
WARM_N, WARM_TICKS = 24, 6
WARM_GAITS = ("trot10", "trot10", "trot10", "trot10", None, "pace10")   # None: standing
WARM_IT0 = (0, 3, 5, 8, 0, 2)


@functools.lru_cache(maxsize=None)
def _moving():
    """[(batch, {robot: optimum})] for WARM_TICKS ticks -- every gait robot's table is
    gait_table(g, it0 + tick, N), x0 drifts by a few mm / mrad per tick as in
    test_warm_start_interior_point -- and one more entry: the next tick with every robot
    handed the pacing robot's table."""
    from mpcqp.synthetic import gait_table
    N, B = WARM_N, len(WARM_GAITS)
    bt = _fleet(B, N, SEED + 400)
    rng = np.random.default_rng(SEED + 401)
    out = []
    for tick in range(WARM_TICKS + 1):
        bt = _copy(bt)
        if tick:
            bt["x0"][:, :12] += rng.normal(0.0, 2e-3, size=(B, 12)).astype(np.float32)
        for b, (g, it0) in enumerate(zip(WARM_GAITS, WARM_IT0)):
            bt["contact"][b] = 1.0 if g is None else gait_table(g, it0 + tick, N)
        if tick == WARM_TICKS:
            bt["contact"][:] = bt["contact"][5]
        out.append((bt, _oracle(bt, range(B), N)))
    for (a, _), (b, _) in zip(out, out[1:WARM_TICKS]):   # the tables do move, the standing robot's does not
        changed = (a["contact"] != b["contact"]).reshape(B, -1).any(axis=1)
        assert changed.tolist() == [True, True, True, True, False, True]
    assert (_stance(out[0][0]) == (48, 48, 48, 48, 96, 48)).all()
    return out


WARM_SHORT_N = 13   # N < NM = 16: S = 52, n = 156, interior point, bytes 52 .. 63 of a row unused


@functools.lru_cache(maxsize=None)
def _short_standing():
    N, B = WARM_SHORT_N, 4
    bt = _fleet(B, N, SEED + 500)
    bt["contact"][:] = 1.0
    assert all(_is_ipm(N, s) for s in _stance(bt))
    rng = np.random.default_rng(SEED + 501)
    out = []
    for tick in range(3):
        bt = _copy(bt)
        if tick:
            bt["x0"][:, :12] += rng.normal(0.0, 2e-3, size=(B, 12)).astype(np.float32)
        out.append((bt, _oracle(bt, range(B), N)))
    return out


# ------------------------------------------------------------------ the unmarked tests
PARTS = ("A", "A-weights", "B", "C", "D", "E")


@pytest.mark.parametrize("part", PARTS)
def test_cases_are_what_they_claim(part):
    """The builders' asserts -- every case's stance count and capacity class -- and the oracle's
    finite solve of every case, part by part."""
    if part == "A":
        for N in SWEEP:
            _sweep_ref(N)
            assert all(_sweep_ipm(N)) or N == 11
    elif part == "A-weights":
        for N in WEIGHTED:
            for kind in KINDS:
                _sweep_ref(N, kind)
    elif part == "B":
        for N in TAILS:
            _tails_ref(N)
    elif part == "C":
        for N in SMALL_N:
            for count in (1, 2, 4):
                _small_case(N, count)
    elif part == "D":
        for N, kind in THRU:
            _thru_ref(N, kind, MI355X_CUS)
    else:
        _moving()
        _short_standing()


@pytest.mark.parametrize("ncu", (8, 104, MI355X_CUS, 304))
def test_throughput_cases_plan_the_throughput_kernel(lib, ncu):   # noqa: F811
    """D's inputs plan ipm_thru, with ipm_full set for the full weights: a routing change that
    stops them reaching mpcqp_kernel_ipm<FULL, 16, true> fails here, whatever the chip's size."""
    for N, kind in THRU:
        _assert_plans_throughput(lib, N, kind, ncu)
    # one robot fewer than "more than three per CU" is the latency layout: the cases sit past the threshold
    assert _plan(lib, 16, 3 * ncu, (64, 64), ncu=ncu, full=1)["ipm_thru"] == 0


# ------------------------------------------------------------------ device side
def _engine(N, kind="diag"):
    from mpcqp import LinearMpc
    return LinearMpc(horizon=N, robot="a1", **_weights(kind, N))


def _solve(eng, bt):
    import torch
    res = eng.solve(bt["x0"], bt["xref"], bt["contact"], bt["feet"], robot=bt["robot"], return_all=True)
    torch.cuda.synchronize()
    B = len(bt["x0"])
    return (res.u0.cpu().numpy(), res.U.cpu().numpy().reshape(B, -1), res.status.cpu().numpy(),
            res.iterations.cpu().numpy())


def _held_to_oracle(label, bt, out, xs, ipm=None):
    """Status OK; u0 and U of every robot the oracle solved within the contract; the worst
    interior-point robot within that class's guard (a dense-class robot within the dense one);
    iterations > 0 for a robot with stance, U = 0 and no iteration for one without."""
    u0, U, st, it = out
    assert (st == 0).all(), (label, st)
    stance = _stance(bt)
    worst = 0.0
    for b, x in xs.items():
        e0, eU = rel_err_u0(u0[b], x[:12]), rel_err_u0(U[b], x)
        assert e0 < TOL_U0 and eU < TOL_U0, (label, b, int(stance[b]), e0, eU)
        if ipm is not None and not ipm[b]:
            assert max(e0, eU) < TOL_ACHIEVED, (label, b, int(stance[b]), e0, eU)
        else:
            worst = max(worst, e0, eU)
    for b in range(len(st)):
        if stance[b] == 0:
            assert not U[b].any() and not u0[b].any() and it[b] == 0, (label, b)
        else:
            assert it[b] > 0, (label, b, it)
    print(f"{label}: worst relative error {worst:.2e}, factorisations {it.tolist()}")
    assert worst < TOL_ACHIEVED_IPM, (label, worst)
    return worst


# ---- A
@pytest.mark.gpu
@pytest.mark.parametrize("N", SWEEP)
def test_horizon_sweep(N):
    """Every horizon of the class, default routing.  stage_gemm's tiles hold 16 stages: N = 17
    has one live stage in the second tile, N = 31 fifteen, N = 15 is one short of a full tile;
    N < NM everywhere but at 16, 20 and 32, so a loop over NM stages, or a read of a stage row
    nobody wrote, shows here.  (One of stage_gemm's two guards alone widened to NM does not: the
    product's rows are independent, so a row past N read in only reaches an output row past N,
    which the other guard keeps from being stored or, stored as zero, from being read.)"""
    bt = _sweep(N)
    _held_to_oracle(f"A N={N}", bt, _solve(_engine(N), bt), _sweep_ref(N), _sweep_ipm(N))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", WEIGHTED)
def test_horizon_sweep_full_weights(N, kind):
    """The sweep's batch under full Q with a leg-block R (the FULL instantiations) and under a
    cross-leg R (XR: 12 x 12 stage weights), against the oracle with the same Q and R."""
    bt = _sweep(N)
    _held_to_oracle(f"A N={N} {kind}", bt, _solve(_engine(N, kind), bt), _sweep_ref(N, kind), _sweep_ipm(N))


# ---- B
@pytest.mark.gpu
@pytest.mark.parametrize("N", tuple(TAILS))
def test_foot_step_lane_tails(N):
    """``for j = lane; j < S; j += 64``: S = 63 / 64 / 65 (the last lane idle, every lane one
    foot-step, lane 0 a second one), 79, 123 and 127 (the second round's tail) in the LDS
    layouts; S = 43 / 44 / 63 in the register layout."""
    bt = _tails(N)
    _held_to_oracle(f"B N={N} S={[s for s, _ in TAILS[N]]}", bt, _solve(_engine(N), bt), _tails_ref(N))


# ---- C
@pytest.mark.gpu
@pytest.mark.parametrize("count", (1, 2, 4))
@pytest.mark.parametrize("N", SMALL_N)
def test_smallest_problems_beyond_the_dense_layouts(N, count):
    """S = 1, 2 and 4 at N > 20: m_tot = S R of 5 .. 24 rows, E_k = 0 at all stages but one or
    two, the only stance at the first, a middle or the last step of the recursions."""
    bt, xs = _small_case(N, count)
    _held_to_oracle(f"C N={N} S={count}", bt, _solve(_engine(N), bt), xs)


# ---- D
@pytest.mark.gpu
@pytest.mark.parametrize("N,kind", THRU)
def test_throughput_layout_short_horizons_and_full_weights(lib, N, kind):   # noqa: F811
    """More than three standing robots per CU, promised as such: the throughput layout at
    N < 16 and, with full weights, its FULL instantiation -- planned (asserted for this chip's
    CU count), every status OK, robots 0, 1, B // 2, B - 2, B - 1 on the oracle's optimum and
    within the guard of the latency layout's result for the same robots."""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    _assert_plans_throughput(lib, N, kind, ncu)
    bt = _thru(N, ncu)
    B = len(bt["x0"])
    eng = _engine(N, kind)
    eng.set_stance_range(4 * N, 4 * N)
    u0, U, st, it = _solve(eng, bt)
    assert (st == 0).all(), np.unique(st, return_counts=True)
    assert (it > 0).all()
    pick = _thru_pick(B)
    xs = _thru_ref(N, kind, ncu)
    sub = {k: v[pick] for k, v in bt.items()}
    _held_to_oracle(f"D N={N} {kind} B={B} (largest count of the batch {int(it.max())})", sub,
                    tuple(a[pick] for a in (u0, U, st, it)), {j: xs[b] for j, b in enumerate(pick)})
    small = _solve(_engine(N, kind), sub)   # five robots: the latency layout
    _held_to_oracle(f"D N={N} {kind} latency layout", sub, small, {j: xs[b] for j, b in enumerate(pick)})
    for j, b in enumerate(pick):
        assert rel_err_u0(U[b], small[1][j].astype(np.float64)) < TOL_ACHIEVED_IPM, (N, kind, b)


# ---- E
def _memory_matches(mem, bt, N, label):
    """A status-OK robot's row: 0x80 in bytes 0 .. 4 N - 1, row bits (the six cone rows) only at
    stance foot-steps, bytes 4 N .. 127 zero."""
    m = mem.cpu().numpy()
    assert m.shape[1] == WARM_BYTES
    stance = bt["contact"].reshape(len(bt["x0"]), -1)[:len(m)] > 0
    assert np.all(m[:, :4 * N] & 0x80), label
    assert not m[:, 4 * N:].any(), label
    assert not (m[:, :4 * N] & 0x40).any() and not (m[:, :4 * N] & 0x3F)[~stance].any(), label
    return m


@pytest.mark.gpu
def test_warm_start_on_a_moving_schedule():
    """The memory is indexed by (stage, leg); a controller's table advances every tick, so a
    foot-step's remembered rows sit under another foot-step, or under a swing entry.  Every
    tick of the warm and of a cold engine on the oracle's optimum, the memory's bytes after
    every tick, and then every robot handed the pacing robot's table.  The factorisation counts
    are printed, and no ratio asserted."""
    N, ticks = WARM_N, _moving()
    B = len(WARM_GAITS)
    warm, cold = _engine(N), _engine(N)
    mem = warm.set_warm_start(B)
    assert tuple(mem.shape) == (B, WARM_BYTES) and int(mem.sum()) == 0
    fw, fc = [], []
    for tick, (bt, xs) in enumerate(ticks):
        what = "pacing table for all" if tick == WARM_TICKS else f"tick {tick}"
        w, c = _solve(warm, bt), _solve(cold, bt)
        _held_to_oracle(f"E moving, warm, {what}", bt, w, xs)
        _held_to_oracle(f"E moving, cold, {what}", bt, c, xs)
        _memory_matches(mem, bt, N, what)
        fw.append(int(w[3].sum()))
        fc.append(int(c[3].sum()))
    print(f"E moving: factorisations per tick, warm {fw}, cold {fc}")
    warm.set_warm_start(0)


@pytest.mark.gpu
def test_warm_start_past_its_capacity():
    """set_warm_start(3) with six robots: three rows, robots 3 .. 5 solved cold -- bitwise the
    cold engine's result, its iteration counts included -- and rows 0 .. 2 bitwise those of an
    engine that remembers all six."""
    N, ticks = WARM_N, _moving()[:3]
    three, six, cold = _engine(N), _engine(N), _engine(N)
    mem3, mem6 = three.set_warm_start(3), six.set_warm_start(6)
    assert tuple(mem3.shape) == (3, WARM_BYTES)
    for tick, (bt, xs) in enumerate(ticks):
        a, s, c = _solve(three, bt), _solve(six, bt), _solve(cold, bt)
        _held_to_oracle(f"E capacity 3, tick {tick}", bt, a, xs)
        assert np.array_equal(a[3][3:], c[3][3:]), (tick, a[3], c[3])
        for x, y in zip(a, c):
            assert np.array_equal(x[3:], y[3:]), tick
        for x, y in zip(a, s):
            assert np.array_equal(x[:3], y[:3]), tick
        m3 = _memory_matches(mem3, bt, N, tick)
        assert np.array_equal(m3, _memory_matches(mem6, bt, N, tick)[:3]), tick
    three.set_warm_start(0)
    six.set_warm_start(0)


@pytest.mark.gpu
def test_warm_start_below_the_layout_size():
    """N = 13 in the 16-stage layout, standing, three ticks: bytes 4 N .. 63 -- stages the layout
    has and the horizon has not -- stay zero, like bytes 64 .. 127."""
    N = WARM_SHORT_N
    eng = _engine(N)
    mem = eng.set_warm_start(4)
    fact = []
    for tick, (bt, xs) in enumerate(_short_standing()):
        out = _solve(eng, bt)
        _held_to_oracle(f"E N={N}, tick {tick}", bt, out, xs)
        m = _memory_matches(mem, bt, N, tick)
        assert not m[:, 4 * N:64].any()
        fact.append(int(out[3].sum()))
    print(f"E N={N}: factorisations per tick {fact}")
    eng.set_warm_start(0)

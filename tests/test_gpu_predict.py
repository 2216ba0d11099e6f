"""GPU: mpcqp_predict -- the trajectory the QP believes a force sequence produces, its cost, cone
margin and swing residual, one wavefront per robot in one launch -- against the float64
restatement tests/predict_ref.py (pinned on the CPU to the reference's recorded com_traj and to
the oracle's Sx, Su, tests/test_predict.py), against that recording itself, and after a real
solve.  Every output lies between canary rows and every launch finds them untouched.

Bounds.  The float32 X against predict_ref within F32_BOUND = 2.4e-7 (max norm relative to
max(1, |X|_inf)), the project's floor for a float32 store.  The float64 costs within 10
predict_ref.D_J = 2.6e-14 relative, margin and swing residual within the same times max(1, max|U|):
the project's rule for a device build of a host-checked text (D: tests/test_predict.py).  Against
the reference's com_traj / objective and the oracle's objective: predict_ref.REF_X_BOUND =
1.72e-5 and REF_J_BOUND = 5.55e-6, 10 x what predict_ref itself measures against them on the CPU.
Status, batch tails, refusals' neighbours and graph replays have none: equal / bitwise.

Measured on the MI355X (also DESIGN.md 4.4h; printed by the tests): the float32 X bitwise
predict_ref's (0) in every case; the costs 9.4e-16 (B = 131, N = 10), 2.7e-16 (N = 32), 3.4e-16
(N = 1), 7.5e-16 and 2.4e-15 (full weights, N = 10 and 32), 4.6e-16 (0.3 rad normals); margin and swing residual 0,
6.3e-17 on the tilted normals, 3.7e-17 of (1 + mu) max|U| against oracle.formulation.cone_rows.
The reference's com_traj 1.21e-6 (N = 10) and 1.02e-6 (N = 16), its objective 4.67e-7 and
4.33e-7 -- predict_ref's own figures.  After a real solve: 65 of 65 status-OK, the smallest margin
-0.24 of the allowance, cost at most 0.09 of cost_free, the objective against the oracle's
optimum 4.6e-7.
"""
import ctypes
import os

import numpy as np
import pytest

# torch first: it brings its own HIP runtime, which must be loaded before libmpcqp.so
torch = pytest.importorskip("torch")

import predict_ref as pr  # noqa: E402
from helpers import DEV, _dev, oracle_solution  # noqa: E402
from oracle import formulation as F  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = -77.0
PAD = 2
J_BOUND = 10 * pr.D_J
INPUTS = ("x0", "xref", "contact", "feet", "robot")


def engine(N, Q=pr.Q_DIAG, R=pr.R_DIAG):
    from mpcqp import LinearMpc
    return LinearMpc(horizon=N, robot="a1", Q=Q, R=R, device=DEV)


def buffers(B, N):
    """X, report and status with one canary row ahead of their B rows and PAD behind."""
    rows = 1 + B + PAD
    return dict(X=torch.full((rows, N, 13), CANARY, dtype=torch.float32, device=DEV),
                report=torch.full((rows, 4), CANARY, dtype=torch.float64, device=DEV),
                status=torch.full((rows,), int(CANARY), dtype=torch.int32, device=DEV))


def launch(eng, N, bt, U, skip=(), inputs=None):
    """One mpcqp_predict launch on canary-framed outputs: dict(X, report, status) as NumPy, B rows;
    the outputs named in `skip` are passed as NULL and come back as canaries."""
    B = len(bt["x0"])
    inp = inputs or {k: _dev(bt[k]) for k in INPUTS}
    Ud = U if torch.is_tensor(U) else _dev(U)
    bf = buffers(B, N)
    live = {k: (None if k in skip else v[1:1 + B]) for k, v in bf.items()}
    eng.predict_raw(B, inp["x0"], inp["xref"], inp["contact"], inp["feet"], inp["robot"], Ud, live["X"],
                    live["report"], live["status"])
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in bf.items()}
    for k, v in out.items():
        assert (v[0] == CANARY).all() and (v[1 + B:] == CANARY).all(), k
    return {k: v[1:1 + B] for k, v in out.items()}


def check_against_ref(name, out, ref, U):
    ex = pr.x_err(out["X"], ref["X"])
    ej, em = pr.report_err(out["report"], ref["report"], U)
    print(f"\n{name}: X {ex:.2e} (bound {pr.F32_BOUND:.1e}), costs {ej:.2e}, margin / swing {em:.2e} (bound {J_BOUND:.1e})")
    assert np.array_equal(out["status"], ref["status"])
    assert ex <= pr.F32_BOUND and ej <= J_BOUND and em <= J_BOUND
    return ex, ej, em


# ---- the restatement

@pytest.mark.parametrize("name", ["mixed_N10", "long_N32", "short_N1"])
def test_matches_the_restatement(name):
    """B = 131 with mixed gaits and robots at N = 10, B = 3 at N = 32, B = 2 at N = 1; U random, a
    quarter of the swing entries non-zero, contact values 0.5, -inf and NaN among them."""
    case = pr.gpu_cases()[name]
    out = launch(engine(case["N"]), case["N"], case["bt"], case["U"])
    check_against_ref(name, out, case["ref"], case["U"])
    assert (case["ref"]["report"][:, pr.SWING] > 0).any()


@pytest.mark.parametrize("name", ["full_N10", "full_N32"])
def test_full_weights_match_the_restatement(name):
    """A full Q and an R coupling every pair of legs (mpcqp_set_weights), at N = 10 and at N = 32,
    the kernel's two full-weight instantiations."""
    case = pr.gpu_cases()[name]
    N = case["N"]
    assert np.abs(case["R"][0, 3:]).max() > 0 and np.abs(case["Q"] - np.diag(np.diag(case["Q"]))).max() > 0
    out = launch(engine(N, case["Q"], case["R"]), N, case["bt"], case["U"])
    check_against_ref(name, out, case["ref"], case["U"])
    diag = launch(engine(N), N, case["bt"], case["U"])
    assert np.array_equal(diag["X"], out["X"]) and not np.array_equal(diag["report"][:, :2], out["report"][:, :2])


def test_tilted_normal_matches_the_restatement_and_the_oracle_rows():
    """Every normal tilted by 0.3 rad: against predict_ref's rows, and the margin against
    oracle.formulation.cone_rows.  Both evaluate the same rows from the same float32 normal in
    float64, a handful of roundings of terms up to (1 + mu) max|U|: bound 64 eps (1 + mu) max|U|."""
    case = pr.gpu_cases()["tilted_N10"]
    bt, U, N = case["bt"], case["U"], 10
    assert np.allclose(np.arccos(bt["robot"][:, 11].astype(np.float64)), 0.3, atol=1e-6)
    out = launch(engine(N), N, bt, U)
    check_against_ref("tilted_N10", out, case["ref"], U)
    worst = 0.0
    for b in range(len(U)):
        mu, fz_max = float(bt["robot"][b, 7]), float(bt["robot"][b, 8])
        rows = F.cone_rows(mu, bt["robot"][b, 9:12].astype(np.float64)).astype(np.float64)
        f = U[b].astype(np.float64).reshape(N, 4, 3)
        ct = bt["contact"][b].astype(np.float64)
        slack = np.concatenate([f @ rows.T, (ct * fz_max - f @ rows[4])[..., None]], axis=-1)
        want = slack[bt["contact"][b] > 0].min()
        err = abs(out["report"][b, pr.MARGIN] - want) / ((1 + mu) * np.abs(U[b]).max())
        worst = max(worst, err)
    print(f"margin against oracle.formulation.cone_rows: {worst:.2e} of (1 + mu) max|U| (bound {64 * 2.0 ** -52:.1e})")
    assert worst <= 64 * 2.0 ** -52


# ---- the reference's recorded run

@pytest.mark.parametrize("N", [10, 16])
def test_matches_the_reference_com_traj_and_objective(N):
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(pr.__file__)), "golden", "predict.npz"))
    bt = {k: fx[f"N{N}_{k}"] for k in INPUTS}
    U = fx[f"N{N}_u_star"].astype(np.float32).reshape(-1, N, 12)
    out = launch(engine(N), N, bt, U)
    ex = pr.x_err(out["X"].reshape(len(U), -1), fx[f"N{N}_com_traj"])
    ej = pr.rel_err(out["report"][:, pr.COST] - out["report"][:, pr.COST_FREE], fx[f"N{N}_objective"])
    print(f"\nN={N}: com_traj {ex:.2e} (bound {pr.REF_X_BOUND:.2e}), objective {ej:.2e} (bound {pr.REF_J_BOUND:.2e})")
    assert (out["status"] == 0).all()
    assert ex <= pr.REF_X_BOUND and ej <= pr.REF_J_BOUND


# ---- after a real solve

def test_after_a_real_solve():
    """B = 65, N = 10, trot: solve, then predict on its U.  A status-OK robot has nothing on its
    swing legs, costs no more than U = 0, and sits inside its cones to the rounding of float32 U,
    2^-23 (1 + mu) max|U| per row; for 8 robots the objective is the oracle's at its optimum."""
    from mpcqp.synthetic import make_batch
    B, N = 65, 10
    bt = make_batch(B, N, seed=77, gaits=("trot10",), robots=("a1", "aliengo"))
    eng = engine(N)
    res = eng.solve(bt["x0"], bt["xref"], bt["contact"], bt["feet"], robot=bt["robot"], return_all=True)
    prd = eng.predict(bt["x0"], bt["xref"], bt["contact"], bt["feet"], res.U, robot=bt["robot"])
    torch.cuda.synchronize()
    ok = (res.status.cpu().numpy() == 0) & (prd.status.cpu().numpy() == 0)
    assert ok.sum() >= B - 2 and (prd.status.cpu().numpy() == 0).all()
    rep, U = prd.report.cpu().numpy(), res.U.cpu().numpy()
    assert np.array_equal(rep[:, pr.COST], prd.cost.cpu().numpy()) and prd.cone_margin.data_ptr() == prd.report.data_ptr() + 16
    allow = 2.0 ** -23 * (1 + bt["robot"][:, 7].astype(np.float64)) * np.abs(U).reshape(B, -1).max(axis=1)
    print(f"\nstatus-OK {ok.sum()} of {B}: smallest margin / allowance {(rep[ok, pr.MARGIN] / allow[ok]).min():.2f}, "
          f"largest cost / cost_free {(rep[ok, pr.COST] / rep[ok, pr.COST_FREE]).max():.3f}")
    assert (rep[ok, pr.SWING] == 0).all()
    assert (rep[ok, pr.COST] <= rep[ok, pr.COST_FREE]).all()
    assert (rep[ok, pr.MARGIN] >= -allow[ok]).all()
    worst = 0.0
    for b in np.flatnonzero(ok)[:8]:
        x, o, _ = oracle_solution(bt, b, N)
        worst = max(worst, pr.rel_err(rep[b, pr.COST] - rep[b, pr.COST_FREE], 0.5 * x @ o["H"] @ x + o["g"] @ x))
    print(f"objective against the oracle's optimum, 8 robots: {worst:.2e} (bound {pr.REF_J_BOUND:.2e})")
    assert worst <= pr.REF_J_BOUND


# ---- batch tails

@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_batch_tails_are_bitwise_the_large_launch(B):
    case = pr.gpu_cases()["mixed_N10"]
    eng = engine(10)
    whole = launch(eng, 10, case["bt"], case["U"])
    part = launch(eng, 10, {k: v[:B] for k, v in case["bt"].items()}, case["U"][:B])
    for k in whole:
        assert part[k].tobytes() == whole[k][:B].tobytes(), k


# ---- refusals

def test_refusals_zero_the_robot_and_leave_its_neighbours():
    case = pr.gpu_cases()["mixed_N10"]
    N, B = 10, 16
    bt = {k: v[:B].copy() for k, v in case["bt"].items()}
    U = case["U"][:B].copy()
    eng = engine(N)
    clean = launch(eng, N, bt, U)
    bt["x0"][1, 4] = np.nan
    bt["xref"][2, 9, 12] = np.nan
    bt["feet"][3, 2, 1] = np.nan
    bt["robot"][4, 0] = np.nan
    U[5, 3, 7] = np.nan
    bt["contact"][6, 4, 1] = np.inf
    bt["robot"][7, 0] = 0.0                                       # mass 0: finite inputs, 1 / m is not
    bad = np.arange(1, 8)
    keep = np.setdiff1d(np.arange(B), bad)
    out = launch(eng, N, bt, U)
    ref = pr.predict_batch(N, bt, U)
    assert (out["status"][bad] == pr.STATUS_NONFINITE).all() and (out["status"][keep] == 0).all()
    assert np.array_equal(out["status"], ref["status"])
    assert (out["X"][bad] == 0).all() and (out["report"][bad] == 0).all()
    for k in out:
        assert out[k][keep].tobytes() == clean[k][keep].tobytes(), k
    # a -inf or NaN contact is a swing foot-step, as in the solve
    sw = {k: v[:B].copy() for k, v in case["bt"].items()}
    stance = np.argwhere(sw["contact"][8] > 0)[:2]
    sw["contact"][8][tuple(stance[0])] = -np.inf
    sw["contact"][8][tuple(stance[1])] = np.nan
    zero = {k: v.copy() for k, v in sw.items()}
    zero["contact"][8][tuple(stance[0])] = 0.0
    zero["contact"][8][tuple(stance[1])] = 0.0
    a, b = launch(eng, N, sw, case["U"][:B]), launch(eng, N, zero, case["U"][:B])
    assert a["status"][8] == 0
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- pointers

def test_misaligned_inputs_give_the_aligned_result():
    """U, x0 and xref as views one float past a 16-byte boundary."""
    case = pr.gpu_cases()["mixed_N10"]
    N, B = 10, 5
    bt = {k: v[:B] for k, v in case["bt"].items()}
    eng = engine(N)
    want = launch(eng, N, bt, case["U"][:B])
    inp = {k: _dev(bt[k]) for k in INPUTS}
    Ud = _dev(case["U"][:B])

    def shifted(t):
        buf = torch.full((t.numel() + 8,), float("nan"), dtype=torch.float32, device=DEV)
        assert buf.data_ptr() % 16 == 0
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    for names in (("U",), ("x0",), ("xref",), ("U", "x0", "xref")):
        moved = dict(inp, **{k: shifted(inp[k]) for k in names if k != "U"})
        got = launch(eng, N, bt, shifted(Ud) if "U" in names else Ud, inputs=moved)
        for k in want:
            assert got[k].tobytes() == want[k].tobytes(), (names, k)


def test_each_output_null_in_turn_and_all_null():
    case = pr.gpu_cases()["long_N32"]
    N, bt, U = 32, case["bt"], case["U"]
    eng = engine(N)
    want = launch(eng, N, bt, U)
    for skip in ("X", "report", "status"):
        got = launch(eng, N, bt, U, skip=(skip,))
        for k in want:
            assert (got[k] == CANARY).all() if k == skip else got[k].tobytes() == want[k].tobytes(), (skip, k)
    got = launch(eng, N, bt, U, skip=("X", "report", "status"))      # MPCQP_OK, nothing launched
    assert all((v == CANARY).all() for v in got.values())


def test_argument_refusals():
    from mpcqp import _lib
    case = pr.gpu_cases()["short_N1"]
    eng = engine(1)
    inp = [_dev(case["bt"][k]) for k in INPUTS] + [_dev(case["U"])]
    X = torch.full((2, 1, 13), CANARY, dtype=torch.float32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    call = lambda B, flags, ins, out: eng.lib.mpcqp_predict(eng._ctx, B, flags, *[p(t) for t in ins], p(out), None, None, None)
    assert call(2, 1, inp, X) == _lib.ERR_ARG and b"flags" in eng.lib.mpcqp_last_error(eng._ctx)
    assert call(-1, 0, inp, X) == _lib.ERR_ARG
    for i in range(6):
        assert call(2, 0, inp[:i] + [None] + inp[i + 1:], X) == _lib.ERR_ARG, i
    assert call(0, 0, inp, X) == _lib.MPCQP_OK
    torch.cuda.synchronize()
    assert (X == CANARY).all()
    with pytest.raises(ValueError):
        eng.predict_raw(2, *inp[:5], inp[5].double(), X)
    with pytest.raises(ValueError):
        eng.predict_raw(3, *inp, X)


# ---- graph

def test_graph_replay_equals_the_eager_call():
    """bind_predict captured on a side stream and replayed twice over changed U."""
    case = pr.gpu_cases()["mixed_N10"]
    N, B = 10, 65
    bt = {k: v[:B] for k, v in case["bt"].items()}
    eng = engine(N)
    inp = {k: _dev(bt[k]) for k in INPUTS}
    Ud = _dev(case["U"][:B])
    bf = buffers(B, N)
    fn = eng.bind_predict(B, inp["x0"], inp["xref"], inp["contact"], inp["feet"], inp["robot"], Ud,
                          bf["X"][1:1 + B], bf["report"][1:1 + B], bf["status"][1:1 + B])
    assert any(t is Ud for t in fn.buffers)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fn(s)
    seen = []
    for r, seed in enumerate((1, 2)):
        U = pr.random_u(bt, 900 + seed)
        Ud.copy_(_dev(U))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in bf.items()}
        eager = launch(eng, N, bt, U, inputs=inp)
        for k in eager:
            assert got[k][1:1 + B].tobytes() == eager[k].tobytes(), (r, k)
            assert (got[k][0] == CANARY).all() and (got[k][1 + B:] == CANARY).all()
        seen.append(got["X"].tobytes())
    assert seen[0] != seen[1]


# ---- the drop-in

def test_shim_predicted_trajectory_is_predict_on_the_tick_buffers():
    import test_shim as ts
    m = ts._shim()
    c = m.ModelPredictiveController(ts.LinearMpcConfig, ts.AliengoConfig)
    with pytest.raises(RuntimeError):
        c.predicted_trajectory()
    rd = ts.FakeRobotData()
    c.update_robot_state(rd)
    with pytest.raises(RuntimeError):
        c.predicted_trajectory()
    table = np.tile(np.array([1, 0, 0, 1], np.float32), 10)
    c.update_mpc_if_needed(0, np.array([0.8, 0.0, 0.0]), 0.1, table)
    traj = c.predicted_trajectory()
    assert traj.shape == (10, 13) and traj.dtype == np.float32
    dv, up, eng = c._dev, c._up_views, c._engine
    res = eng.predict(dv["x0"], dv["xref"], up["contact"].reshape(1, 10, 4), up["feet"], dv["U"].reshape(1, 10, 12),
                      robot=dv["robot"])
    torch.cuda.synchronize()
    assert np.array_equal(traj, res.X.cpu().numpy()[0]) and int(res.status[0]) == 0
    # and it is the restatement's trajectory of the tick's own inputs
    ref = pr.predict_robot(10, dv["x0"].cpu().numpy()[0], dv["xref"].cpu().numpy()[0], table, up["feet"].cpu().numpy()[0],
                           dv["robot"].cpu().numpy()[0], dv["U"].cpu().numpy())
    assert ref[3] == 0 and pr.x_err(traj[None], ref[1][None]) <= pr.F32_BOUND
    assert float(res.cost[0]) <= float(res.cost_free[0]) and float(res.swing_residual[0]) == 0.0

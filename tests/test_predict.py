"""CPU: the predicted trajectory (mpcqp_predict) without a GPU -- the ABI and Python surface, the
float64 restatement tests/predict_ref.py against the reference's recorded com_traj and objective
(tests/golden/predict.npz, made by tests/golden/make_golden_predict.py from the reference's own
Sx, Su) and against the oracle's Sx, Su at N = 1, 10, 20, 32, the per-robot header
csrc/mpcqp_predict_robot.h compiled with g++ and driven through ctypes against the restatement,
and known answers that need no tolerance argument.

Measured here (printed by the tests):
  predict_ref against the fixture (12 robots, N = 10 and 16, U = float32(u*)): com_traj 1.21e-6 in
    the max norm relative to max(1, |X|_inf), the objective J - J_free 4.7e-7 relative.
  predict_ref against oracle.formulation.condensed_cost's Sx, Su (3 robots each at N = 1, 10, 20,
    32, U = float32 of the oracle's optimum): X 8.3e-8 / 4.4e-7 / 1.71e-6 / 1.02e-6, the objective
    5.5e-7 / 4.1e-7 / 4.3e-7 / 2.6e-7.  What remains is the reference's float32 powers of A_d.
    predict_ref.REF_X = 1.72e-6, REF_J = 5.55e-7 (the worst of both, rounded up); the bounds are
    10 x these.
  the host-compiled header against predict_ref over predict_ref.gpu_cases(), float64 before the
    store: X 1.02e-15, the costs 2.55e-15 (8.5e-16 but for the full weights at N = 32, whose
    quadratic form has terms of both signs; predict_ref.D_X = 1.1e-15, D_J = 2.6e-15); the margin
    and the swing residual 6.3e-17 of max(1, max|U|); the float32 X within F32_BOUND of predict_ref's,
    the status equal.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import predict_ref as pr
from helpers import host_build, oracle_solution
from oracle import formulation as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpcqp.h")
PREDICT_HEADER = os.path.join(ROOT, "include", "mpcqp_predict_abi.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "predict.npz")
KNOWN = 1e-12
SENTINEL = -77

SHIM = r'''
#include "mpcqp_predict_robot.h"
// a launch of mpcqp_predict_kernel, robot after robot; W: full Q then R, or NULL
extern "C" void launch(int N, double h, const double* q, const double* r, const double* W, int B, const float* x0,
                       const float* xref, const float* contact, const float* feet, const float* robot,
                       const float* U, float* X, double* Xd, double* report, int32_t* status) {
  for (int b = 0; b < B; ++b)
    prd_robot_host(N, h, q, r, W, x0 + 13 * b, xref + 13 * N * b, contact + 4 * N * b, feet + 12 * b, robot + 16 * b,
                   U + 12 * N * b, X ? X + 13 * N * b : nullptr, Xd ? Xd + 13 * N * b : nullptr,
                   report ? report + PRD_REPORT * b : nullptr, status ? status + b : nullptr);
}
extern "C" int report_words(void) { return PRD_REPORT; }
extern "C" int status_nonfinite(void) { return PRD_STATUS_NONFINITE; }
extern "C" int max_horizon(void) { return PRD_MAX_N; }
'''


# ---- the ABI and Python surface

def test_constants_match_binding(robot):
    from mpcqp import _lib
    src = open(HEADER).read() + open(PREDICT_HEADER).read()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", src).group(1))
    assert define("MPCQP_PREDICT_REPORT") == _lib.PREDICT_REPORT == pr.REPORT == robot.report_words() == 4
    assert pr.STATUS_NONFINITE == _lib.STATUS_NONFINITE == robot.status_nonfinite()
    assert define("MPCQP_MAX_HORIZON") == robot.max_horizon()


def test_null_ctx_is_an_error_code():
    from mpcqp import _lib
    assert _lib.load().mpcqp_predict(None, 1, 0, *([None] * 10)) == -1


def test_python_surface():
    import mpcqp
    from mpcqp.engine import LinearMpc, PredictResult, SolveResult
    assert "PredictResult" in mpcqp.__all__ and mpcqp.PredictResult is PredictResult
    for name in ("predict", "predict_raw", "bind_predict"):
        assert getattr(LinearMpc, name).__doc__
    assert PredictResult.__doc__ and SolveResult.__doc__
    rep = np.arange(8.0).reshape(2, 4)
    res = PredictResult("X", rep, "status")
    assert res.X == "X" and res.status == "status" and res.report is rep
    for k, name in enumerate(("cost", "cost_free", "cone_margin", "swing_residual")):
        assert np.shares_memory(getattr(res, name), rep) and getattr(res, name).tolist() == rep[:, k].tolist()
    import importlib.util
    spec = importlib.util.spec_from_file_location("shim_mpc", os.path.join(ROOT, "pympc-quadruped_amd", "linear_mpc",
                                                                           "mpc.py"))
    shim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shim)
    assert shim.ModelPredictiveController.predicted_trajectory.__doc__


# ---- the restatement against the reference's recorded run and the oracle's Sx, Su

def _fixture(N):
    fx = np.load(GOLDEN)
    g = lambda k: fx[f"N{N}_{k}"]
    bt = {k: g(k) for k in ("x0", "xref", "contact", "feet", "robot")}
    return bt, g("u_star"), g("com_traj"), g("objective")


def test_fixture_holds_arrays_only():
    fx = np.load(GOLDEN)     # allow_pickle is off: arrays alone load
    assert fx["horizons"].tolist() == [10, 16] and os.path.getsize(GOLDEN) < 100 * 1024
    for N in (10, 16):
        assert fx[f"N{N}_com_traj"].shape == (6, 13 * N) and fx[f"N{N}_u_star"].shape == (6, 12 * N)
        assert {4.713, 9.042} == {round(float(m), 3) for m in fx[f"N{N}_robot"][:, 0]}


def test_restatement_matches_the_reference_com_traj_and_objective():
    """Measured: com_traj 1.21e-6 (N = 10), 1.02e-6 (N = 16); objective 4.7e-7, 4.3e-7.  The gap is
    the reference's float32 powers of A_d and float32 Su (mpc.py:213-230), not the restatement."""
    for N in (10, 16):
        bt, u_star, com_traj, objective = _fixture(N)
        U = u_star.astype(np.float32).reshape(-1, N, 12)
        out = pr.predict_batch(N, bt, U)
        ex = pr.x_err(out["X64"].reshape(len(U), -1), com_traj)
        ej = pr.rel_err(out["report"][:, pr.COST] - out["report"][:, pr.COST_FREE], objective)
        print(f"\nN={N}: com_traj {ex:.2e} (bound {pr.REF_X_BOUND:.1e}), objective {ej:.2e} (bound {pr.REF_J_BOUND:.1e})")
        assert (out["status"] == 0).all()
        assert ex <= pr.REF_X_BOUND and ej <= pr.REF_J_BOUND
        assert ex <= pr.REF_X and ej <= pr.REF_J            # the recorded figures still describe it
        # u* is an optimum: J <= J_free, nothing on a swing leg beyond the solver's rounding, cones
        # feasible to the rounding of float32 U
        assert (out["report"][:, pr.COST] <= out["report"][:, pr.COST_FREE]).all()
        assert (out["report"][:, pr.SWING] < 1e-9).all()
        assert (out["report"][:, pr.MARGIN] >= -2.0 ** -23 * 1.7 * np.abs(U).reshape(len(U), -1).max(axis=1)).all()


@pytest.mark.parametrize("N", [1, 10, 20, 32])
def test_restatement_matches_the_oracle_sx_su(N):
    """Measured: X 8.3e-8 / 4.4e-7 / 1.71e-6 / 1.02e-6 and the objective 5.5e-7 / 4.1e-7 / 4.3e-7 /
    2.6e-7 at N = 1 / 10 / 20 / 32."""
    from mpcqp.synthetic import make_batch
    bt = make_batch(3, N, seed=600 + N, gaits=("trot10", "bound8"), robots=("a1", "aliengo"))
    ex = ej = 0.0
    for b in range(3):
        u, o, _ = oracle_solution(bt, b, N)
        U = u.astype(np.float32)
        H, g, Su, Sx = F.condensed_cost(o["Ad"], o["Bd"], bt["x0"][b], bt["xref"][b].reshape(-1), N)
        traj = Sx @ bt["x0"][b] + Su @ U.astype(np.float64)
        obj = 0.5 * U.astype(np.float64) @ H @ U + g @ U
        X, _, rep, status = pr.predict_robot(N, bt["x0"][b], bt["xref"][b], bt["contact"][b], bt["feet"][b],
                                             bt["robot"][b], U)
        assert status == 0
        ex = max(ex, pr.x_err(X.reshape(1, -1), traj[None]))
        ej = max(ej, pr.rel_err(rep[pr.COST] - rep[pr.COST_FREE], obj))
    print(f"\nN={N}: X {ex:.2e} (bound {pr.REF_X_BOUND:.1e}), objective {ej:.2e} (bound {pr.REF_J_BOUND:.1e})")
    assert ex <= pr.REF_X_BOUND and ej <= pr.REF_J_BOUND
    assert ex <= pr.REF_X and ej <= pr.REF_J


# ---- the host-compiled header

@pytest.fixture(scope="module")
def robot():
    lib = host_build(SHIM, name="predict")
    vp = ctypes.c_void_p
    lib.launch.argtypes = [ctypes.c_int, ctypes.c_double, vp, vp, vp, ctypes.c_int] + [vp] * 10
    lib.launch.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_launch(lib, N, bt, U, Q=pr.Q_DIAG, R=pr.R_DIAG, dt=pr.DT, pad=2, skip=()):
    """A launch on the host: the outputs come back with `pad` sentinel rows; `skip`: outputs passed
    as NULL."""
    B = len(bt["x0"])
    Q, R = np.asarray(Q, np.float64), np.asarray(R, np.float64)
    W = None
    if Q.ndim == 2 or R.ndim == 2:
        Qm = Q if Q.ndim == 2 else np.diag(Q)
        Rm = R if R.ndim == 2 else np.diag(R)
        W = np.ascontiguousarray(np.concatenate([Qm.reshape(-1), Rm.reshape(-1)]))
        Q, R = np.diag(Qm).copy(), np.diag(Rm).copy()
    c = lambda k: np.ascontiguousarray(bt[k], np.float32)
    out = dict(X=np.full((B + pad, N, 13), SENTINEL, np.float32), X64=np.full((B + pad, N, 13), float(SENTINEL)),
               report=np.full((B + pad, 4), float(SENTINEL)), status=np.full((B + pad,), SENTINEL, np.int32))
    a = {k: (None if k in skip else v) for k, v in out.items()}
    lib.launch(N, dt, _p(np.ascontiguousarray(Q)), _p(np.ascontiguousarray(R)), _p(W), B, _p(c("x0")), _p(c("xref")),
               _p(c("contact")), _p(c("feet")), _p(c("robot")), _p(np.ascontiguousarray(U, np.float32)), _p(a["X"]),
               _p(a["X64"]), _p(a["report"]), _p(a["status"]))
    for k, v in out.items():
        assert (v[B:] == SENTINEL).all(), k
    return {k: v[:B] for k, v in out.items()}


def test_header_matches_the_restatement(robot):
    """D over predict_ref.gpu_cases(), the inputs of tests/test_gpu_predict.py, recorded as
    predict_ref.D_X and D_J.  What bounds it: the two differ in the order of float64 sums alone --
    24 terms per entry of X, 13 N + 12 N terms per cost, non-negative with diagonal weights -- so a
    few eps = 2.2e-16, a few more where a full Q's cross terms cancel."""
    dx = dj = dm = 0.0
    for name, case in pr.gpu_cases().items():
        N, bt, U, ref = case["N"], case["bt"], case["U"], case["ref"]
        out = host_launch(robot, N, bt, U, case["Q"], case["R"])
        ex = pr.x_err(out["X64"], ref["X64"])
        ej, em = pr.report_err(out["report"], ref["report"], U)
        print(f"\n{name}: X {ex:.2e}, costs {ej:.2e}, margin / swing {em:.2e}")
        assert np.array_equal(out["status"], ref["status"]) and (ref["status"] == 0).all()
        assert pr.x_err(out["X"], ref["X"]) <= pr.F32_BOUND
        dx, dj, dm = max(dx, ex), max(dj, ej), max(dm, em)
    print(f"D_X = {dx:.2e} (predict_ref.D_X = {pr.D_X:.1e}), D_J = {dj:.2e} (predict_ref.D_J = {pr.D_J:.1e})")
    assert dx <= 64 * 2.0 ** -52 and dj <= 64 * 2.0 ** -52
    assert dx <= 4 * pr.D_X and dj <= 4 * pr.D_J and dm <= 4 * pr.D_J      # the recorded figures still describe it


def test_each_output_absent_in_turn(robot):
    case = pr.gpu_cases()["short_N1"]
    full = host_launch(robot, 1, case["bt"], case["U"])
    for skip in ("X", "X64", "report", "status"):
        out = host_launch(robot, 1, case["bt"], case["U"], skip=(skip,))
        for k in out:
            assert (out[k] == SENTINEL).all() if k == skip else np.array_equal(out[k], full[k], equal_nan=True), (skip, k)


# ---- known answers

def _standing(N, B=1):
    """A robot at rest on its reference: level, yaw 0.3, feet under the hips, all feet in stance."""
    from mpcqp.params import ROBOT_PRESETS, pack_robot
    x0 = np.zeros((B, 13), np.float32)
    x0[:, 2], x0[:, 3:6], x0[:, 12] = 0.3, [0.5, -0.25, 0.42], -9.81
    feet = np.tile(np.float32([[0.18, 0.13, -0.42], [0.18, -0.13, -0.42], [-0.18, 0.13, -0.42], [-0.18, -0.13, -0.42]]),
                   (B, 1, 1))
    return dict(x0=x0, xref=np.tile(x0[:, None, :], (1, N, 1)), contact=np.ones((B, N, 4), np.float32), feet=feet,
                robot=np.tile(pack_robot(ROBOT_PRESETS["a1"]), (B, 1)).astype(np.float32))


@pytest.mark.parametrize("N", [1, 10, 32])
def test_zero_force_costs_the_free_cost_and_falls_under_gravity(robot, N):
    bt = _standing(N)
    out = host_launch(robot, N, bt, np.zeros((1, N, 12), np.float32))
    ref = pr.predict_batch(N, bt, np.zeros((1, N, 12), np.float32))
    for o in (out, ref):
        rep = o["report"][0]
        assert rep[pr.COST] == rep[pr.COST_FREE] > 0 and rep[pr.MARGIN] == 0.0 and rep[pr.SWING] == 0.0
        # at rest: X == x0 but for z and vz, whose closed form is n1, n2
        k = np.arange(1, N + 1, dtype=np.float64)
        h, g = 0.05, float(bt["x0"][0, 12])
        want = np.tile(bt["x0"][0].astype(np.float64), (N, 1))
        want[:, 5] += k * (0.5 * h * h * g) + 0.5 * k * (k - 1) * (h * h * g)
        want[:, 11] += k * (h * g)
        assert np.abs(o["X64"][0] - want).max() < KNOWN
        moved = np.ones(13, bool)
        moved[[5, 11]] = False
        assert np.array_equal(o["X64"][0][:, moved], want[:, moved])                   # bitwise
        assert np.abs(o["X64"][0][:, 5] - (float(bt["x0"][0, 5]) + 0.5 * g * (k * h) ** 2)).max() < KNOWN    # z0 + g t^2 / 2
    assert np.array_equal(out["X"], ref["X"])


def test_weight_holding_force_keeps_the_robot_at_rest(robot):
    """f_z = m g / 4 on every foot of the symmetric stance: no net force, no net moment."""
    N = 10
    bt = _standing(N)
    U = np.zeros((1, N, 4, 3), np.float32)
    U[..., 2] = np.float32(bt["robot"][0, 0]) * np.float32(9.81) / 4
    out = host_launch(robot, N, bt, U.reshape(1, N, 12))
    # float32(m g / 4) and float32(1 / m) leave 1e-7 of the weight: 3e-8 m/s^2 over 0.5 s
    assert np.abs(out["X64"][0] - bt["x0"][0].astype(np.float64)).max() < 1e-6
    assert out["report"][0, pr.COST] < 1e-3 * out["report"][0, pr.COST_FREE]


def test_force_on_a_cone_edge_has_margin_zero(robot):
    N = 1
    bt = _standing(N)
    mu = np.float32(bt["robot"][0, 7])
    for fx, fy, row in ((-1.0, 0.2, 0), (1.0, 0.2, 1), (0.2, -1.0, 2), (0.2, 1.0, 3)):
        U = np.zeros((1, N, 4, 3), np.float32)
        U[..., 2] = 100.0                                         # inside: slack mu fz = 70 on every row
        U[0, 0, 1] = [np.float32(fx) * mu * 100, np.float32(fy) * mu * 100, 100.0]   # on the edge of `row`
        for o in (host_launch(robot, N, bt, U.reshape(1, N, 12)), pr.predict_batch(N, bt, U.reshape(1, N, 12))):
            m = o["report"][0, pr.MARGIN]
            assert abs(m) <= 2.0 ** -23 * (1 + mu) * 100 and o["status"][0] == 0, (row, m)
    # past the edge by 1 N: the margin is -1
    U[0, 0, 1] = [0.0, mu * 100 + 1.0, 100.0]
    m = host_launch(robot, N, bt, U.reshape(1, N, 12))["report"][0, pr.MARGIN]
    assert abs(m + 1.0) < 1e-5


def test_half_contact_halves_the_upper_bound(robot):
    N = 2
    bt = _standing(N)
    bt["contact"][0, 1, 2] = 0.5
    fz_max = float(bt["robot"][0, 8])
    U = np.zeros((1, N, 4, 3), np.float32)
    U[..., 2] = 10.0
    U[0, 1, 2, 2] = 0.5 * fz_max                                  # on the upper row of contact 0.5
    for o in (host_launch(robot, N, bt, U.reshape(1, N, 12)), pr.predict_batch(N, bt, U.reshape(1, N, 12))):
        assert o["report"][0, pr.MARGIN] == 0.0
    U[0, 1, 2, 2] = 0.5 * fz_max + 8.0
    assert host_launch(robot, N, bt, U.reshape(1, N, 12))["report"][0, pr.MARGIN] == -8.0


def test_no_stance_gives_an_infinite_margin_and_the_swing_residual(robot):
    N = 3
    bt = _standing(N)
    bt["contact"][:] = [0.0, -1.0, -np.inf, np.nan]
    U = np.zeros((1, N, 12), np.float32)
    U[0, 2, 7] = -3.5
    for o in (host_launch(robot, N, bt, U), pr.predict_batch(N, bt, U)):
        assert o["report"][0, pr.MARGIN] == np.inf and o["report"][0, pr.SWING] == 3.5 and o["status"][0] == 0


# ---- refusals

def test_refusals_zero_the_robot_and_leave_its_neighbours(robot):
    case = pr.gpu_cases()["mixed_N10"]
    N = 10
    bt = {k: v[:12].copy() for k, v in case["bt"].items()}
    U = case["U"][:12].copy()
    clean = host_launch(robot, N, bt, U)
    bt["x0"][1, 4] = np.nan
    bt["xref"][2, 9, 12] = np.inf
    bt["feet"][3, 2, 1] = -np.inf
    bt["robot"][4, 0] = np.nan
    U[5, 3, 7] = np.nan
    bt["contact"][6, 4, 1] = np.inf
    bt["robot"][7, 0] = 0.0                                       # mass 0: finite inputs, 1 / m is not
    bt["robot"][8, 1:7] = 0.0                                     # a singular inertia
    bt["robot"][9, 12:] = np.nan                                  # words 12..15 are not read
    bad = np.arange(1, 9)
    out = host_launch(robot, N, bt, U)
    ref = pr.predict_batch(N, bt, U)
    for o in (out, ref):
        assert (o["status"][bad] == pr.STATUS_NONFINITE).all()
        assert (o["X"][bad] == 0).all() and (o["report"][bad] == 0).all()
        keep = np.setdiff1d(np.arange(12), bad)
        assert (o["status"][keep] == 0).all()
    keep = np.setdiff1d(np.arange(12), bad)
    for k in ("X", "X64", "report", "status"):
        assert out[k][keep].tobytes() == clean[k][keep].tobytes(), k

"""CPU: the optimality certificate (mpcqp_certify) without a GPU -- the ABI and Python surface,
the float64 restatement tests/certify_ref.py against the dense H, g of
oracle.formulation.condensed_cost and the oracle's optimum at N = 1, 10, 20, 32, the bound
itself, a finite-difference identity, known answers, and the per-robot header
csrc/mpcqp_certify_robot.h compiled with g++ and driven through ctypes against the restatement.

Measured here (printed by the tests):
  certify_ref's G against H U + g at random U (3 robots each at N = 1, 10, 20, 32), relative to
    max |H U + g|: 1.9e-7 / 5.2e-7 / 3.2e-7 / 5.4e-7; the objective against 1/2 U^T H U + g^T U
    2.1e-7 / 4.7e-7 / 3.8e-7 / 5.2e-7 relative.  What remains is the reference's float32 powers of
    A_d.  certify_ref.REF_G = 5.4e-7; the bound is 10 x that.
  the bound on those robots: gap >= phi(U) - phi* - slack for U = 0, 0.5 u*, 0.9 u* and
    float32(u*), lower <= phi* + slack for those and for random U, without exception.  gap / |phi*|
    at float32(u*) between 3.0e-6 and 1.8e-4; gap / (phi(U) - phi*) at 0.9 u* between 240 and 2100:
    the gap is a first-order bound, tight at the optimum and loose far from it.
  the finite-difference identity G64 . d = (phi(U + d) - phi(U - d)) / 2: at most 1.1e-16 of
    sum |G64| |d| + |J| + |J_free| (FD_BOUND = 64 eps).
  the host-compiled header against certify_ref over certify_ref.gpu_cases(), float64: G 2.5e-16
    of gscale, the objective 7.5e-16 of |J| + |J_free|, gap / lower / worst 1.7e-15 of gapscale
    but for optimum_N10, 2.9e-9: there the gradient cancels to 1e-7 of its terms and gapscale with
    it, while the gap still carries eps gscale (|u| + ub (1 + 2 mu)), which the test also holds it
    to (certify_ref.D_G = 2.5e-16, D_OBJ = 7.5e-16, D_GAP = 2.9e-9); the float32 G within
    F32_BOUND of certify_ref's, the status equal.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import certify_ref as cr
import predict_ref as pr
from helpers import host_build, oracle_solution
from oracle import formulation as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpcqp.h")
CERTIFY_HEADER = os.path.join(ROOT, "include", "mpcqp_certify_abi.h")
KNOWN = 1e-12
FD_BOUND = 64 * 2.0 ** -52
SENTINEL = -77

SHIM = r'''
#include "mpcqp_certify_robot.h"
// a launch of mpcqp_certify_kernel, robot after robot; W: full Q then R, or NULL
extern "C" void launch(int N, double h, const double* q, const double* r, const double* W, int B, const float* x0,
                       const float* xref, const float* contact, const float* feet, const float* robot,
                       const float* U, float* G, double* Gd, double* report, int32_t* status) {
  for (int b = 0; b < B; ++b)
    cert_robot_host(N, h, q, r, W, x0 + 13 * b, xref + 13 * N * b, contact + 4 * N * b, feet + 12 * b, robot + 16 * b,
                    U + 12 * N * b, G ? G + 12 * N * b : nullptr, Gd ? Gd + 12 * N * b : nullptr,
                    report ? report + CERT_REPORT * b : nullptr, status ? status + b : nullptr);
}
// the predicted trajectory's report and status on the same inputs (mpcqp_predict_robot.h)
extern "C" void launch_predict(int N, double h, const double* q, const double* r, const double* W, int B,
                               const float* x0, const float* xref, const float* contact, const float* feet,
                               const float* robot, const float* U, double* report, int32_t* status) {
  for (int b = 0; b < B; ++b)
    prd_robot_host(N, h, q, r, W, x0 + 13 * b, xref + 13 * N * b, contact + 4 * N * b, feet + 12 * b, robot + 16 * b,
                   U + 12 * N * b, nullptr, nullptr, report + PRD_REPORT * b, status + b);
}
extern "C" int report_words(void) { return CERT_REPORT; }
extern "C" int report_word(int k) { return k == 0 ? CERT_OBJECTIVE : k == 1 ? CERT_GAP : k == 2 ? CERT_LOWER : CERT_WORST; }
extern "C" int status_nonfinite(void) { return PRD_STATUS_NONFINITE; }
extern "C" int max_horizon(void) { return PRD_MAX_N; }
'''


# ---- the ABI and Python surface

def test_constants_match_binding(robot):
    from mpcqp import _lib
    src = open(HEADER).read() + open(CERTIFY_HEADER).read()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", src).group(1))
    assert define("MPCQP_CERTIFY_REPORT") == _lib.CERTIFY_REPORT == cr.REPORT == robot.report_words() == 4
    assert [robot.report_word(k) for k in range(4)] == [cr.OBJECTIVE, cr.GAP, cr.LOWER, cr.WORST]
    assert cr.STATUS_NONFINITE == _lib.STATUS_NONFINITE == robot.status_nonfinite()
    assert define("MPCQP_MAX_HORIZON") == robot.max_horizon()


def test_null_ctx_is_an_error_code():
    from mpcqp import _lib
    assert _lib.load().mpcqp_certify(None, 1, 0, *([None] * 10)) == -1


def test_python_surface():
    import mpcqp
    from mpcqp.engine import CertifyResult, LinearMpc
    assert "CertifyResult" in mpcqp.__all__ and mpcqp.CertifyResult is CertifyResult
    for name in ("certify", "certify_raw", "bind_certify"):
        assert getattr(LinearMpc, name).__doc__
    assert "first-order bound" in CertifyResult.__doc__ and "first-order bound" in LinearMpc.certify.__doc__
    rep = np.arange(8.0).reshape(2, 4)
    res = CertifyResult("G", rep, "status")
    assert res.G == "G" and res.status == "status" and res.report is rep
    for k, name in enumerate(("objective", "gap", "lower", "worst")):
        assert np.shares_memory(getattr(res, name), rep) and getattr(res, name).tolist() == rep[:, k].tolist()
    import importlib.util
    spec = importlib.util.spec_from_file_location("shim_mpc", os.path.join(ROOT, "pympc-quadruped_amd", "linear_mpc",
                                                                           "mpc.py"))
    shim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shim)
    assert "first-order" in shim.ModelPredictiveController.optimality_gap.__doc__


# ---- the restatement against the dense oracle

HORIZONS = [1, 10, 20, 32]


def _oracle_robots(N):
    """Three robots at horizon N: [(inputs of certify_robot, H, g, u*, phi*)]."""
    from mpcqp.synthetic import make_batch
    bt = make_batch(3, N, seed=600 + N, gaits=("trot10", "bound8"), robots=("a1", "aliengo"))
    out = []
    for b in range(3):
        u, o, _ = oracle_solution(bt, b, N)
        H, g, _, _ = F.condensed_cost(o["Ad"], o["Bd"], bt["x0"][b], bt["xref"][b].reshape(-1), N)
        args = (bt["x0"][b], bt["xref"][b], bt["contact"][b], bt["feet"][b], bt["robot"][b])
        out.append((args, H, g, u, 0.5 * u @ H @ u + g @ u, {k: v[b:b + 1] for k, v in bt.items()}))
    return out


@pytest.fixture(scope="module")
def oracle_robots():
    return {N: _oracle_robots(N) for N in HORIZONS}


@pytest.mark.parametrize("N", HORIZONS)
def test_restatement_matches_the_dense_gradient(oracle_robots, N):
    """G against H U + g relative to max |H U + g|, the objective against 1/2 U^T H U + g^T U."""
    eg = ej = 0.0
    for b, (args, H, g, _, _, bt1) in enumerate(oracle_robots[N]):
        U = pr.random_u(bt1, 700 + 10 * N + b)[0]
        u = U.astype(np.float64).reshape(-1)
        out = cr.certify_robot(N, *args, U)
        want = H @ u + g
        assert out["status"] == 0
        eg = max(eg, float(np.abs(out["G64"].reshape(-1) - want).max() / np.abs(want).max()))
        ej = max(ej, pr.rel_err(out["report"][cr.OBJECTIVE], 0.5 * u @ H @ u + g @ u))
        assert out["report"][cr.LOWER] == out["report"][cr.OBJECTIVE] - out["report"][cr.GAP]
    print(f"\nN={N}: G {eg:.2e} (bound {cr.REF_G_BOUND:.1e}), objective {ej:.2e} (bound {cr.REF_J_BOUND:.1e})")
    assert eg <= cr.REF_G_BOUND and ej <= cr.REF_J_BOUND
    assert eg <= cr.REF_G            # the recorded figure still describes it


@pytest.mark.parametrize("N", HORIZONS)
def test_the_gap_bounds_the_suboptimality(oracle_robots, N):
    """gap >= phi(U) - phi* - slack for feasible U, lower <= phi* + slack for any U, slack =
    REF_J_BOUND |phi*| + 10 D_GAP gapscale."""
    tight, loose = [], []
    for b, (args, H, g, us, phis, bt1) in enumerate(oracle_robots[N]):
        u32 = us.astype(np.float32)
        for name, U in (("0", np.zeros_like(u32)), ("0.5", (0.5 * us).astype(np.float32)),
                        ("0.9", (0.9 * us).astype(np.float32)), ("f32", u32)):
            out = cr.certify_robot(N, *args, U)
            prd = pr.predict_robot(N, *args, U)
            assert out["status"] == 0
            assert prd[2][pr.MARGIN] >= -1e-5 and prd[2][pr.SWING] < 1e-9, (name, prd[2])      # feasible
            slack = cr.REF_J_BOUND * abs(phis) + 10 * cr.D_GAP * out["gapscale"]
            rep = out["report"]
            assert rep[cr.GAP] >= rep[cr.OBJECTIVE] - phis - slack, (N, b, name, rep, phis)
            assert rep[cr.LOWER] <= phis + slack, (N, b, name, rep, phis)
            assert rep[cr.WORST] <= rep[cr.GAP] + slack
            if name == "f32":
                tight.append(rep[cr.GAP] / abs(phis))
            if name == "0.9":
                loose.append(rep[cr.GAP] / (rep[cr.OBJECTIVE] - phis))
        for seed in range(3):
            U = pr.random_u(bt1, 800 + 10 * N + seed)[0]
            out = cr.certify_robot(N, *args, U)
            slack = cr.REF_J_BOUND * abs(phis) + 10 * cr.D_GAP * out["gapscale"]
            assert out["report"][cr.LOWER] <= phis + slack, (N, b, seed, out["report"], phis)
    print(f"\nN={N}: gap / |phi*| at float32(u*) {min(tight):.1e} .. {max(tight):.1e}; gap / (phi - phi*) at 0.9 u* "
          f"{min(loose):.0f} .. {max(loose):.0f}")
    assert max(tight) < 1e-2            # tight at the optimum


@pytest.mark.parametrize("N", HORIZONS)
def test_finite_difference_identity(oracle_robots, N):
    """G64 . d = (phi(U + d) - phi(U - d)) / 2, exact for a quadratic up to float64 rounding; phi
    from predict_ref.  U and d are multiples of 2^-10 well inside float32, so U +- d are exact."""
    worst = 0.0
    for b, (args, _, _, _, _, bt1) in enumerate(oracle_robots[N]):
        rng = np.random.default_rng(900 + 10 * N + b)
        U = np.round(pr.random_u(bt1, 910 + b)[0] * 1024) / 1024
        d = (np.round(rng.uniform(-4, 4, U.shape) * 1024) / 1024).astype(np.float32)
        U = U.astype(np.float32)
        out = cr.certify_robot(N, *args, U)
        phi = []
        scale = float((np.abs(out["G64"]) * np.abs(d)).sum())
        for Ud in (U + d, U - d):
            rep = pr.predict_robot(N, *args, Ud)[2]
            phi.append(rep[pr.COST] - rep[pr.COST_FREE])
            scale += abs(rep[pr.COST]) + abs(rep[pr.COST_FREE])
        assert np.array_equal((U + d).astype(np.float64), U.astype(np.float64) + d.astype(np.float64))
        err = abs(float((out["G64"] * d).sum()) - 0.5 * (phi[0] - phi[1])) / scale
        worst = max(worst, err)
    print(f"\nN={N}: finite-difference identity {worst:.2e} of the terms' scale (bound {FD_BOUND:.1e})")
    assert worst <= FD_BOUND


# ---- the host-compiled header

@pytest.fixture(scope="module")
def robot():
    lib = host_build(SHIM, name="certify")
    vp = ctypes.c_void_p
    lib.launch.argtypes = [ctypes.c_int, ctypes.c_double, vp, vp, vp, ctypes.c_int] + [vp] * 10
    lib.launch.restype = None
    lib.launch_predict.argtypes = [ctypes.c_int, ctypes.c_double, vp, vp, vp, ctypes.c_int] + [vp] * 8
    lib.launch_predict.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _weights(Q, R):
    """(q, r, W) as the host bodies take them: the diagonals, and the full Q then R or None."""
    Q, R = np.asarray(Q, np.float64), np.asarray(R, np.float64)
    W = None
    if Q.ndim == 2 or R.ndim == 2:
        Qm = Q if Q.ndim == 2 else np.diag(Q)
        Rm = R if R.ndim == 2 else np.diag(R)
        W = np.ascontiguousarray(np.concatenate([Qm.reshape(-1), Rm.reshape(-1)]))
        Q, R = np.diag(Qm).copy(), np.diag(Rm).copy()
    return np.ascontiguousarray(Q), np.ascontiguousarray(R), W


def host_launch(lib, N, bt, U, Q=cr.Q_DIAG, R=cr.R_DIAG, dt=cr.DT, pad=2, skip=()):
    """A launch on the host: the outputs come back with `pad` sentinel rows; `skip`: outputs passed
    as NULL."""
    B = len(bt["x0"])
    Q, R, W = _weights(Q, R)
    c = lambda k: np.ascontiguousarray(bt[k], np.float32)
    out = dict(G=np.full((B + pad, N, 12), SENTINEL, np.float32), G64=np.full((B + pad, N, 12), float(SENTINEL)),
               report=np.full((B + pad, 4), float(SENTINEL)), status=np.full((B + pad,), SENTINEL, np.int32))
    a = {k: (None if k in skip else v) for k, v in out.items()}
    lib.launch(N, dt, _p(Q), _p(R), _p(W), B, _p(c("x0")), _p(c("xref")),
               _p(c("contact")), _p(c("feet")), _p(c("robot")), _p(np.ascontiguousarray(U, np.float32)), _p(a["G"]),
               _p(a["G64"]), _p(a["report"]), _p(a["status"]))
    for k, v in out.items():
        assert (v[B:] == SENTINEL).all(), k
    return {k: v[:B] for k, v in out.items()}


def test_header_matches_the_restatement(robot):
    """D over certify_ref.gpu_cases(), the inputs of tests/test_gpu_certify.py, recorded as
    certify_ref.D_G, D_OBJ and D_GAP.  What bounds it: the two differ in the order of float64 sums
    alone, and every figure is taken relative to the sum of the absolute values of its terms, so a
    few eps = 2.2e-16 times the number of roundings along the longest chain (the two scans)."""
    dg = do = dp = 0.0
    for name, case in cr.gpu_cases().items():
        N, bt, U, ref = case["N"], case["bt"], case["U"], case["ref"]
        out = host_launch(robot, N, bt, U, case["Q"], case["R"])
        eg = cr.g_err(out["G64"], ref)
        eo, ep = cr.report_err(out["report"], ref)
        print(f"\n{name}: G {eg:.2e}, objective {eo:.2e}, gap / lower / worst {ep:.2e}")
        assert np.array_equal(out["status"], ref["status"]) and (ref["status"] == 0).all()
        assert cr.g_err(out["G"], ref) <= cr.F32_BOUND
        dg, do, dp = max(dg, eg), max(do, eo), max(dp, ep)
        # the gap inherits G's rounding, eps gscale, times what multiplies G: |u| and ub (1 + 2 mu).
        # Where the gradient cancels (optimum_N10) that exceeds eps gapscale, which D_GAP records
        fair = cr.gap_rounding_scale(bt, U, ref)
        assert (np.abs(out["report"][:, cr.GAP] - ref["report"][:, cr.GAP]) <= 64 * 2.0 ** -52 * fair).all()
    print(f"D_G = {dg:.2e} (certify_ref.D_G = {cr.D_G:.1e}), D_OBJ = {do:.2e} (certify_ref.D_OBJ = {cr.D_OBJ:.1e}), "
          f"D_GAP = {dp:.2e} (certify_ref.D_GAP = {cr.D_GAP:.1e})")
    assert dg <= 64 * 2.0 ** -52 and do <= 64 * 2.0 ** -52
    assert dg <= 4 * cr.D_G and do <= 4 * cr.D_OBJ and dp <= 4 * cr.D_GAP      # the recorded figures still describe it


def test_objective_is_predicts_cost_difference_to_the_bit(robot):
    """cert_robot_host's objective is prd_robot_host's cost - cost_free bitwise, and the statuses
    agree: both take J and J_free from prd_rollout_host, as both kernels take them from the same
    rollout_* functions (tests/test_gpu_certify.py asserts the same of the device)."""
    for name in ("short_N1", "mixed_N10", "long_N32", "full_N10", "full_N32"):
        case = cr.gpu_cases()[name]
        N, bt, U = case["N"], case["bt"], case["U"]
        B = len(U)
        out = host_launch(robot, N, bt, U, case["Q"], case["R"])
        Q, R, W = _weights(case["Q"], case["R"])
        c = lambda k: np.ascontiguousarray(bt[k], np.float32)
        report, status = np.full((B, 4), float(SENTINEL)), np.full((B,), SENTINEL, np.int32)
        robot.launch_predict(N, cr.DT, _p(Q), _p(R), _p(W), B, _p(c("x0")), _p(c("xref")), _p(c("contact")),
                             _p(c("feet")), _p(c("robot")), _p(np.ascontiguousarray(U, np.float32)), _p(report),
                             _p(status))
        assert np.array_equal(status, out["status"]) and (status == 0).all(), name
        want = report[:, pr.COST] - report[:, pr.COST_FREE]
        assert want.tobytes() == out["report"][:, cr.OBJECTIVE].tobytes(), name
        assert np.abs(want).min() > 0, name           # nothing compared is the zero of a refusal


def test_optimum_case_is_near_the_optimum():
    """optimum_N10: the gradient cancels (|G| far below gscale) and the gap is small against
    |phi*|, the regime the scales are there for."""
    case = cr.gpu_cases()["optimum_N10"]
    ref = case["ref"]
    _, _, phis = cr.optimum_batch()
    assert (ref["status"] == 0).all()
    assert (ref["report"][:, cr.GAP] <= 1e-2 * np.abs(phis)).all()
    assert (ref["report"][:, cr.GAP] >= -cr.REF_J_BOUND * np.abs(phis) - 10 * cr.D_GAP * ref["gapscale"]).all()


def test_each_output_absent_in_turn(robot):
    case = cr.gpu_cases()["short_N1"]
    full = host_launch(robot, 1, case["bt"], case["U"])
    for skip in ("G", "G64", "report", "status"):
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


def _both(robot, N, bt, U):
    ref = cr.certify_batch(N, bt, U)
    return host_launch(robot, N, bt, U), dict(G64=ref["G64"], G=ref["G"], report=ref["report"], status=ref["status"])


@pytest.mark.parametrize("N", [1, 10, 32])
def test_zero_force_has_objective_zero_and_gradient_g(robot, oracle_robots, N):
    """U = 0: phi = 0 exactly, and G is g.  g in closed form for the robot at rest: only z and vz
    fall, so g_j[c] = 2 sum_{t>=j} (X0 + (t - j) X1)[:, c] . Q e_t with e_t known."""
    bt = _standing(N)
    U = np.zeros((1, N, 12), np.float32)
    X0, X1, _, _ = pr.model(bt["x0"][0], bt["feet"][0], bt["robot"][0])
    h, g = 0.05, float(bt["x0"][0, 12])
    k = np.arange(1, N + 1, dtype=np.float64)
    e = np.zeros((N, 13))
    e[:, 5] = k * (0.5 * h * h * g) + 0.5 * k * (k - 1) * (h * h * g)
    e[:, 11] = k * (h * g)
    qe = e * pr.Q_DIAG
    want = np.array([2 * sum((X0 + (t - j) * X1).T @ qe[t] for t in range(j, N)) for j in range(N)])
    for o in _both(robot, N, bt, U):
        assert o["report"][0, cr.OBJECTIVE] == 0.0 and o["status"][0] == 0
        assert np.abs(o["G64"][0] - want).max() <= KNOWN * np.abs(want).max()
        # all stance, U = 0: the gap is -sum m_k >= 0, and lower = -gap
        assert o["report"][0, cr.GAP] >= 0 and o["report"][0, cr.LOWER] == -o["report"][0, cr.GAP]
    # and against the dense g of the oracle's formulation, at the restatement's distance from it
    for args, H, gd, _, _, _ in oracle_robots[N]:
        out = cr.certify_robot(N, *args, np.zeros((N, 12), np.float32))
        assert out["report"][cr.OBJECTIVE] == 0.0
        assert np.abs(out["G64"].reshape(-1) - gd).max() <= cr.REF_G_BOUND * np.abs(gd).max()


def test_all_swing_and_zero_force_has_gap_zero(robot):
    N = 4
    bt = _standing(N)
    bt["contact"][:] = [0.0, -1.0, -np.inf, np.nan]
    for o in _both(robot, N, bt, np.zeros((1, N, 12), np.float32)):
        assert (o["report"][0] == 0.0).all() and o["status"][0] == 0
        assert np.abs(o["G64"][0]).max() > 0


def _single_foot(robot, g_dir, mu=0.5, ub=30.0):
    """A gradient that can be set by hand: N = 1, one stance foot-step (leg 1), Q = 0 and R = I / 2,
    so phi = |u|^2 / 2 and G = u; the foot's force is g_dir.  Returns the restatement's and the
    header's outputs."""
    N = 1
    bt = _standing(N)
    bt["contact"][:] = 0.0
    bt["contact"][0, 0, 1] = 1.0
    bt["robot"][0, 7], bt["robot"][0, 8] = mu, ub
    U = np.zeros((1, N, 4, 3), np.float32)
    U[0, 0, 1] = g_dir
    Q, R = np.zeros(13), np.full(12, 0.5)
    ref = cr.certify_batch(N, bt, U.reshape(1, N, 12), Q, R)
    out = host_launch(robot, N, bt, U.reshape(1, N, 12), Q, R)
    return ref, out


def test_gradient_inside_the_polar_cone_gives_m_zero(robot):
    """g = (0.1, -0.2, 1): g.n - mu |g.t1| - mu |g.t2| = 1 - 0.15 > 0, so m = 0 and gap = g . u =
    |g|^2 (u = g here)."""
    g = np.float32([0.1, -0.2, 1.0])
    want = float((g.astype(np.float64) ** 2).sum())
    for o in _single_foot(robot, g):
        assert np.abs(o["G64"][0, 0, 3:6] - g.astype(np.float64)).max() <= KNOWN
        assert abs(o["report"][0, cr.GAP] - want) <= KNOWN and abs(o["report"][0, cr.WORST] - want) <= KNOWN
        assert abs(o["report"][0, cr.OBJECTIVE] - 0.5 * want) <= KNOWN


@pytest.mark.parametrize("sx,sy", [(1, 1), (1, -1), (-1, 1), (-1, -1)])
def test_gradient_along_a_corner_direction(robot, sx, sy):
    """g = -(sx mu, sy mu, 1) points from the corner v = ub (sx mu, sy mu, 1) of the cut pyramid to
    the apex: m = g . v = -ub (1 + 2 mu^2), by hand."""
    mu, ub = 0.5, 30.0
    g = np.float32([-sx * mu, -sy * mu, -1.0])
    m = -ub * (1.0 + 2.0 * mu * mu)
    gu = float((g.astype(np.float64) ** 2).sum())
    for o in _single_foot(robot, g, mu=mu, ub=ub):
        assert abs(o["report"][0, cr.GAP] - (gu - m)) <= KNOWN * abs(m)
        assert abs(o["report"][0, cr.LOWER] - (0.5 * gu - (gu - m))) <= KNOWN * abs(m)
    # twice the bound doubles m
    ref, _ = _single_foot(robot, g, mu=mu, ub=2 * ub)
    assert abs(ref["report"][0, cr.GAP] - (gu - 2 * m)) <= KNOWN * abs(m)


# ---- refusals

def test_refusals_zero_the_robot_and_leave_its_neighbours(robot):
    case = cr.gpu_cases()["mixed_N10"]
    N = 10
    bt = {k: v[:12].copy() for k, v in case["bt"].items()}
    U = case["U"][:12].copy()
    clean = host_launch(robot, N, bt, U)
    bt["x0"][1, 4] = np.nan
    bt["xref"][2, 9, 12] = np.inf
    bt["feet"][3, 2, 1] = -np.inf
    bt["robot"][4, 0] = np.nan
    U[5, 3, 7] = np.inf
    bt["contact"][6, 4, 1] = np.inf
    bt["robot"][7, 0] = 0.0                                       # mass 0: finite inputs, 1 / m is not
    bt["robot"][8, 1:7] = 0.0                                     # a singular inertia
    bt["robot"][9, 12:] = np.nan                                  # words 12..15 are not read
    bad = np.arange(1, 9)
    out = host_launch(robot, N, bt, U)
    ref = cr.certify_batch(N, bt, U)
    for o in (out, ref):
        assert (o["status"][bad] == cr.STATUS_NONFINITE).all()
        assert (o["G"][bad] == 0).all() and (o["report"][bad] == 0).all()
        keep = np.setdiff1d(np.arange(12), bad)
        assert (o["status"][keep] == 0).all()
    keep = np.setdiff1d(np.arange(12), bad)
    for k in ("G", "G64", "report", "status"):
        assert out[k][keep].tobytes() == clean[k][keep].tobytes(), k

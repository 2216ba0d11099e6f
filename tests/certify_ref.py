"""Float64 NumPy restatement of mpcqp_certify (include/mpcqp_certify_abi.h): the gradient
G = H U + g of the QP's objective phi(U) = J - J_free at a force sequence U, phi(U), and the
duality gap the friction pyramids give in closed form -- TEST INFRASTRUCTURE ONLY.  Built on
predict_ref.model (X0, X1, n1, n2 with the reference's float32 roundings) and cone_rows6.

  G_j  = 2 (X0^T S0_j + X1^T S1_j) + 2 (R u)_j
  S0_j = sum_{t>=j} Q e_t,   S1_j = sum_{t>=j} (t - j) Q e_t = S1_{j+1} + S0_{j+1}
  gap  = sum_k (g_k . u_k - m_k),   m_k = min(0, ub+ (g_k.n - mu |g_k.t1| - mu |g_k.t2|)) in stance, else 0

certify_robot handles one robot, certify_batch a batch; gpu_cases are the inputs of
tests/test_gpu_certify.py, which tests/test_certify.py also runs through the host-compiled
per-robot header to measure D."""
import functools

import numpy as np

import predict_ref as pr
from predict_ref import DT, F32_BOUND, NU, NX, Q_DIAG, R_DIAG, REF_J_BOUND, STATUS_NONFINITE, STATUS_OK  # noqa: F401

REPORT = 4                                    # MPCQP_CERTIFY_REPORT
OBJECTIVE, GAP, LOWER, WORST = 0, 1, 2, 3

# The host build of csrc/mpcqp_certify_robot.h (g++ -O2 -ffp-contract=off) against certify_batch
# over gpu_cases(), measured by tests/test_certify.py::test_header_matches_the_restatement in
# float64: G before the float32 store relative to gscale per robot; the objective relative to
# |J| + |J_free| (it is their difference); gap, lower and worst relative to gapscale (lower: plus
# |J| + |J_free|).  The two differ in the order of float64 sums alone.  The device build of the same
# text is held to 10 D (tests/test_gpu_certify.py).
D_G = 2.5e-16
D_OBJ = 7.5e-16
D_GAP = 2.9e-9       # optimum_N10, where the gradient cancels and gapscale with it; 1.7e-15 over the six others

# certify_robot's G against the dense H U + g of oracle.formulation.condensed_cost at N = 1, 10,
# 20, 32 and random U, relative to max |H U + g|, measured by tests/test_certify.py on the CPU:
# what remains is the reference's float32 powers of A_d, as with predict_ref.REF_X.  The bound is
# 10 x the measured worst.
REF_G = 5.4e-7
REF_G_BOUND = 10 * REF_G


def frame(robot):
    """t1, t2, n of the cone rows: cone_rows6's rows 0, 2 and 4 with mu = 0."""
    rb = np.array(robot, np.float32)
    rb[7] = 0.0
    rows = pr.cone_rows6(rb)
    return rows[0], rows[2], rows[4]


def _suffix(a):
    """(S0, S1): S0_j = sum_{t>=j} a_t, S1_j = sum_{t>j} S0_t = sum_{t>=j} (t - j) a_t."""
    S0 = np.cumsum(a[::-1], axis=0)[::-1]
    S1 = np.concatenate([np.cumsum(S0[:0:-1], axis=0)[::-1], np.zeros((1, a.shape[1]))])
    return S0, S1


def certify_robot(N, x0, xref, contact, feet, robot, U, Q=Q_DIAG, R=R_DIAG, dt=DT):
    """One robot: dict(G64 [N,12] before the float32 store, G float32, report [4], status, gscale,
    gapscale, oscale).  gscale: the largest entry of the gradient's scans, forward and backward,
    run on absolute values (e_t is itself a difference that nearly cancels at an optimum);
    gapscale: sum_k |g_k| . |u_k| + |m_k|; oscale: |J| + |J_free|.  Q / R: diagonals or full."""
    zero = dict(G64=np.zeros((N, NU)), G=np.zeros((N, NU), np.float32), report=np.zeros(REPORT),
                status=STATUS_NONFINITE, gscale=1.0, gapscale=1.0, oscale=1.0)
    x0 = np.asarray(x0, np.float32).reshape(NX)
    xref = np.asarray(xref, np.float32).reshape(N, NX)
    contact = np.asarray(contact, np.float32).reshape(N, 4)
    U = np.asarray(U, np.float32).reshape(N, NU)
    robot = np.asarray(robot, np.float32).reshape(-1)
    if pr.refused_input(x0, xref, contact, feet, robot, U):
        return zero
    Q = np.asarray(Q, np.float64)
    R = np.asarray(R, np.float64)
    Q = np.diag(Q) if Q.ndim == 1 else Q
    R = np.diag(R) if R.ndim == 1 else R
    X0, X1, n1, n2 = pr.model(x0, feet, robot, dt)
    u = U.astype(np.float64)
    P0 = np.cumsum(u, axis=0)
    P1 = np.cumsum(np.concatenate([np.zeros((1, NU)), P0[:-1]]), axis=0)
    k = np.arange(1, N + 1, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        free = (x0.astype(np.float64)[None] + k * n1[None]) + (0.5 * k * (k - 1.0)) * n2[None]
        e = (free + (P0 @ X0.T + P1 @ X1.T)) - xref.astype(np.float64)
        ef = free - xref.astype(np.float64)
        J = float(np.einsum("ti,ij,tj->", e, Q, e) + np.einsum("ti,ij,tj->", u, R, u))
        Jf = float(np.einsum("ti,ij,tj->", ef, Q, ef))
        S0, S1 = _suffix(e @ Q.T)
        G64 = 2.0 * (S0 @ X0 + S1 @ X1) + 2.0 * (u @ R.T)
        aP0 = np.cumsum(np.abs(u), axis=0)
        aP1 = np.cumsum(np.concatenate([np.zeros((1, NU)), aP0[:-1]]), axis=0)
        ae = ((np.abs(x0.astype(np.float64))[None] + k * np.abs(n1)[None]) + (0.5 * k * (k - 1.0)) * np.abs(n2)[None]
              + (aP0 @ np.abs(X0).T + aP1 @ np.abs(X1).T) + np.abs(xref.astype(np.float64)))
        A0, A1 = _suffix(ae @ np.abs(Q).T)
        gscale = float((2.0 * (A0 @ np.abs(X0) + A1 @ np.abs(X1)) + 2.0 * (np.abs(u) @ np.abs(R).T)).max())
        t1, t2, n = frame(robot)
        mu, fz_max = float(robot[7]), float(robot[8])
        stance = contact > 0
        g3, f = G64.reshape(N, 4, 3), u.reshape(N, 4, 3)
        ub = np.maximum(0.0, np.where(stance, contact.astype(np.float64) * fz_max, 0.0))
        v = ub * (g3 @ n - mu * np.abs(g3 @ t1) - mu * np.abs(g3 @ t2))
        m = np.where(stance, np.where(v < 0.0, v, np.where(np.isnan(v), v, 0.0)), 0.0)
        term = (g3 * f).sum(axis=-1) - m
        gap = float(term.sum())
        gapscale = float((np.abs(g3) * np.abs(f)).sum() + np.abs(m).sum())
        G32 = G64.astype(np.float32)
    report = np.array([J - Jf, gap, (J - Jf) - gap, float(term.max())])
    if not (np.isfinite(G32).all() and np.isfinite(report).all()):
        return zero
    return dict(G64=G64, G=G32, report=report, status=STATUS_OK, gscale=gscale, gapscale=gapscale,
                oscale=abs(J) + abs(Jf))


def certify_batch(N, bt, U, Q=Q_DIAG, R=R_DIAG, dt=DT):
    """A batch (the dict of mpcqp.synthetic.make_batch and U [B,N,12]): dict(G64, G, report, status,
    gscale [B], gapscale [B], oscale [B])."""
    B = len(bt["x0"])
    out = [certify_robot(N, bt["x0"][b], bt["xref"][b], bt["contact"][b], bt["feet"][b], bt["robot"][b], U[b], Q, R, dt)
           for b in range(B)]
    res = {k: np.stack([o[k] for o in out]) for k in ("G64", "G", "report")}
    res["status"] = np.array([o["status"] for o in out], np.int32)
    for k in ("gscale", "gapscale", "oscale"):
        res[k] = np.array([o[k] for o in out])
    return res


# ---- error measures

def g_err(G, ref):
    """max over robots of |G - ref.G|_inf / gscale."""
    B = len(ref["gscale"])
    d = np.abs(np.asarray(G, np.float64) - ref["G64" if np.asarray(G).dtype == np.float64 else "G"]).reshape(B, -1).max(axis=1)
    return float((d / ref["gscale"]).max())


def report_err(rep, ref):
    """(objective over |J| + |J_free|; the largest of gap and worst over gapscale and lower over
    gapscale + |J| + |J_free|)."""
    d = np.abs(np.asarray(rep, np.float64) - ref["report"])
    eo = float((d[:, OBJECTIVE] / ref["oscale"]).max())
    eg = max(float((d[:, GAP] / ref["gapscale"]).max()), float((d[:, WORST] / ref["gapscale"]).max()),
             float((d[:, LOWER] / (ref["gapscale"] + ref["oscale"])).max()))
    return eo, eg


def gap_rounding_scale(bt, U, ref):
    """[B]: what a rounding eps of the float64 arithmetic can move the gap by, over eps: G's own
    scale gscale times what multiplies G -- |u| in g . u and ub (1 + 2 mu) in m -- plus gapscale.
    Where the gradient cancels (optimum_N10) it exceeds gapscale by the factor D_GAP shows."""
    B = len(U)
    mu, fz = bt["robot"][:, 7].astype(np.float64), bt["robot"][:, 8].astype(np.float64)
    ub = np.where(bt["contact"] > 0, bt["contact"], 0).astype(np.float64).reshape(B, -1).sum(axis=1) * fz
    return ref["gscale"] * (np.abs(U).astype(np.float64).reshape(B, -1).sum(axis=1) + (1 + 2 * mu) * ub) + ref["gapscale"]


# ---- the GPU tests' inputs

@functools.lru_cache(maxsize=None)
def optimum_batch(B=6, N=10, seed=41):
    """(bt, u* float64 [B,12N], phi* [B]) of B robots with the oracle's optimum."""
    from helpers import oracle_solution
    from mpcqp.synthetic import make_batch
    bt = make_batch(B, N, seed=seed, gaits=pr.GAITS, robots=pr.ROBOTS)
    us, phis = [], []
    for b in range(B):
        x, o, _ = oracle_solution(bt, b, N)
        us.append(x)
        phis.append(0.5 * x @ o["H"] @ x + o["g"] @ x)
    return bt, np.stack(us), np.array(phis)


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """name -> dict(N, bt, U, Q, R, ref, pref): predict_ref.gpu_cases()'s six inputs (mixed N = 10
    B = 131, N = 32 B = 3, N = 1 B = 2, full weights N = 10 B = 9, tilted N = 10 B = 9, full
    weights N = 32 B = 3, with their contact values 0.5, -inf and NaN) and optimum_N10 (B = 6, U =
    float32 of the oracle's optimum, where the gradient cancels); ref is certify_batch of them,
    pref predict_ref.predict_batch (computed once, never modified)."""
    cases = {}
    for name, c in pr.gpu_cases().items():
        cases[name] = dict(N=c["N"], bt=c["bt"], U=c["U"], Q=c["Q"], R=c["R"], pref=c["ref"],
                           ref=certify_batch(c["N"], c["bt"], c["U"], c["Q"], c["R"]))
    bt, us, _ = optimum_batch()
    U = us.astype(np.float32).reshape(len(us), 10, NU)
    cases["optimum_N10"] = dict(N=10, bt=bt, U=U, Q=Q_DIAG, R=R_DIAG, pref=pr.predict_batch(10, bt, U),
                                ref=certify_batch(10, bt, U))
    return cases

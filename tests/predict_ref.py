"""Float64 NumPy restatement of mpcqp_predict (include/mpcqp_predict_abi.h): the trajectory the QP believes a
force sequence U produces, com_traj = Sx x0 + Su U (mpc.py:293-294), its cost, cone margin and
swing residual -- TEST INFRASTRUCTURE ONLY.  The model is form_model's (csrc/mpcqp_form.h), with
the reference's float32 roundings in the same places: cos / sin of the yaw, I_w, its inverse,
inv(I_w)[r]x and 1/m (mpc.py:178-190); everything after is float64.

  x_{t+1} = x0 + (t+1) n1 + C(t+1, 2) n2 + X0 P0_t + X1 P1_t
  P0_t = sum_{j<=t} u_j,   P1_t = sum_{j<=t} (t - j) u_j = P1_{t-1} + P0_{t-1}

predict_robot handles one robot, predict_batch a batch; gpu_cases are the inputs of
tests/test_gpu_predict.py, which tests/test_predict.py also runs through the host-compiled
per-robot header to measure D."""
import functools

import numpy as np

NX, NU, REPORT = 13, 12, 4                    # MPCQP_PREDICT_REPORT
COST, COST_FREE, MARGIN, SWING = 0, 1, 2, 3
STATUS_OK, STATUS_NONFINITE = 0, 4
DT = 0.05
Q_DIAG = np.array([5., 5., 10., 10., 10., 50., 0.01, 0.01, 0.2, 0.2, 0.2, 0.2, 0.])
R_DIAG = np.full(12, 1e-5)

# The host build of csrc/mpcqp_predict_robot.h (g++ -O2 -ffp-contract=off) against predict_batch
# over gpu_cases(), measured by tests/test_predict.py::test_header_matches_the_restatement in
# float64, before the float32 store: X in the max norm relative to max(1, |X|_inf) per robot, the
# two costs relative.  The two differ in the order of float64 sums alone.  The device build of
# the same text is held to 10 D (tests/test_gpu_predict.py).
D_X = 1.1e-15
D_J = 2.6e-15
F32_BOUND = 2.4e-7      # two float32 ulps norm-wise, the project's floor for a float32 store

# predict_batch against the reference's recorded com_traj / objective (tests/golden/predict.npz)
# and against oracle.formulation.condensed_cost's Sx, Su at N = 1, 10, 20, 32, measured by
# tests/test_predict.py on the CPU: what remains is the reference's float32 powers of A_d.  The
# bounds are 10 x the measured worst.
REF_X = 1.72e-6
REF_J = 5.55e-7
REF_X_BOUND = 10 * REF_X
REF_J_BOUND = 10 * REF_J


def f32r(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def rot_z(yaw):
    c, s = f32r(np.cos(yaw)), f32r(np.sin(yaw))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def skew(r):
    return np.array([[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]])


def cone_rows6(robot):
    """The six one-sided rows a_r . f >= b_r form_model writes to mt.rows from robot[7..11]: four
    pyramid rows, n . f >= 0, -n . f >= -contact fz_max."""
    n = np.asarray(robot[9:12], np.float64)
    nn = np.sqrt(n @ n)
    n = n / nn if nn > 0 else np.array([0.0, 0.0, 1.0])
    t1 = np.array([1.0, 0.0, 0.0]) - n[0] * n
    with np.errstate(invalid="ignore", divide="ignore"):
        t1 = t1 / np.sqrt(t1 @ t1)
    t2 = np.cross(n, t1)
    mu = float(robot[7])
    return np.array([t1 + mu * n, -t1 + mu * n, t2 + mu * n, -t2 + mu * n, n, -n])


def model(x0, feet, robot, dt=DT):
    """X0 = B_d, X1 = (A_d - I) B_d (13 x 12 each), n1 = (A_d - I) x0, n2 = (A_d - I)^2 x0."""
    x0 = np.asarray(x0, np.float32).astype(np.float64)
    feet = np.asarray(feet, np.float32).astype(np.float64).reshape(4, 3)
    rb = np.asarray(robot, np.float32).astype(np.float64)
    h = float(dt)
    Rz = rot_z(x0[2])
    Ib = np.array([[rb[1], rb[2], rb[3]], [rb[2], rb[4], rb[5]], [rb[3], rb[5], rb[6]]])
    with np.errstate(all="ignore"):
        Iw = f32r(f32r(Rz @ Ib) @ Rz.T)
        det = (Iw[0, 0] * (Iw[1, 1] * Iw[2, 2] - Iw[1, 2] * Iw[2, 1]) - Iw[0, 1] * (Iw[1, 0] * Iw[2, 2] - Iw[1, 2] * Iw[2, 0])
               + Iw[0, 2] * (Iw[1, 0] * Iw[2, 1] - Iw[1, 1] * Iw[2, 0]))
        adj = np.array([[Iw[(j + 1) % 3, (i + 1) % 3] * Iw[(j + 2) % 3, (i + 2) % 3]
                         - Iw[(j + 1) % 3, (i + 2) % 3] * Iw[(j + 2) % 3, (i + 1) % 3] for j in range(3)] for i in range(3)])
        inv = f32r(adj / det)
        K = np.concatenate([f32r(inv @ skew(feet[leg])) for leg in range(4)], axis=1)     # 3 x 12
        minv = float(f32r(1.0 / rb[0]))
        G = Rz.T @ K
        S = np.tile(np.eye(3), (1, 4))
        X0 = np.concatenate([G * (0.5 * h * h), S * (minv * (0.5 * h * h)), K * h, S * (h * minv), np.zeros((1, 12))])
        X1 = np.concatenate([G * (h * h), S * (minv * (h * h)), np.zeros((7, 12))])
    n1 = np.zeros(NX)
    n1[0:3] = h * (Rz.T @ x0[6:9])
    n1[3:6] = h * x0[9:12]
    n1[5] += 0.5 * h * h * x0[12]
    n1[11] = h * x0[12]
    n2 = np.zeros(NX)
    n2[5] = h * h * x0[12]
    return X0, X1, n1, n2


def refused_input(x0, xref, contact, feet, robot, U):
    """The inputs mpcqp_solve refuses (a non-finite x0, xref, feet or robot[0..11], a +inf
    contact), and a non-finite U entry."""
    fin = lambda a: np.isfinite(np.asarray(a, np.float64)).all()
    return not (fin(x0) and fin(xref) and fin(feet) and fin(np.asarray(robot)[:12]) and fin(U)) \
        or bool((np.asarray(contact) == np.inf).any())


def predict_robot(N, x0, xref, contact, feet, robot, U, Q=Q_DIAG, R=R_DIAG, dt=DT):
    """One robot: (X float64 [N,13] before the float32 store, X float32, report [4], status).  Q /
    R: diagonals or full matrices."""
    zero = (np.zeros((N, NX)), np.zeros((N, NX), np.float32), np.zeros(REPORT), STATUS_NONFINITE)
    x0 = np.asarray(x0, np.float32).reshape(NX)
    xref = np.asarray(xref, np.float32).reshape(N, NX)
    contact = np.asarray(contact, np.float32).reshape(N, 4)
    U = np.asarray(U, np.float32).reshape(N, NU)
    robot = np.asarray(robot, np.float32).reshape(-1)
    if refused_input(x0, xref, contact, feet, robot, U):
        return zero
    Q = np.asarray(Q, np.float64)
    R = np.asarray(R, np.float64)
    Q = np.diag(Q) if Q.ndim == 1 else Q
    R = np.diag(R) if R.ndim == 1 else R
    X0, X1, n1, n2 = model(x0, feet, robot, dt)
    u = U.astype(np.float64)
    P0 = np.cumsum(u, axis=0)
    P1 = np.cumsum(np.concatenate([np.zeros((1, NU)), P0[:-1]]), axis=0)
    k = np.arange(1, N + 1, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        free = (x0.astype(np.float64)[None] + k * n1[None]) + (0.5 * k * (k - 1.0)) * n2[None]
        X = free + (P0 @ X0.T + P1 @ X1.T)
        e, ef = X - xref.astype(np.float64), free - xref.astype(np.float64)
        J = float(np.einsum("ti,ij,tj->", e, Q, e) + np.einsum("ti,ij,tj->", u, R, u))
        Jf = float(np.einsum("ti,ij,tj->", ef, Q, ef))
        rows = cone_rows6(robot)
        stance = contact > 0
        f = u.reshape(N, 4, 3)
        slack = np.einsum("rk,tlk->tlr", rows, f)
        slack[:, :, 5] += contact.astype(np.float64) * float(robot[8])
        X32 = X.astype(np.float32)
    ok = np.isfinite(X32).all() and np.isfinite(J) and np.isfinite(Jf) and np.isfinite(slack[stance]).all()
    if not ok:
        return zero
    margin = float(slack[stance].min()) if stance.any() else np.inf
    swing = float(np.abs(f[~stance]).max()) if (~stance).any() else 0.0
    return X, X32, np.array([J, Jf, margin, swing]), STATUS_OK


def predict_batch(N, bt, U, Q=Q_DIAG, R=R_DIAG, dt=DT):
    """A batch (the dict of mpcqp.synthetic.make_batch and U [B,N,12]): dict(X64, X, report, status)."""
    B = len(bt["x0"])
    out = [predict_robot(N, bt["x0"][b], bt["xref"][b], bt["contact"][b], bt["feet"][b], bt["robot"][b], U[b], Q, R, dt)
           for b in range(B)]
    return dict(X64=np.stack([o[0] for o in out]), X=np.stack([o[1] for o in out]),
                report=np.stack([o[2] for o in out]), status=np.array([o[3] for o in out], np.int32))


# ---- error measures

def x_err(X, ref):
    """Per batch: max over robots of |X - ref|_inf / max(1, |ref|_inf)."""
    X, ref = np.asarray(X, np.float64), np.asarray(ref, np.float64)
    B = ref.shape[0]
    d = np.abs(X - ref).reshape(B, -1).max(axis=1)
    return float((d / np.maximum(1.0, np.abs(ref).reshape(B, -1).max(axis=1))).max())


def rel_err(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(a - ref) / np.abs(ref)).max())


def report_err(rep, ref, U):
    """(cost and cost_free relative, margin and swing residual absolute over max(1, max|U|) per robot)."""
    B = ref.shape[0]
    scale = np.maximum(1.0, np.abs(np.asarray(U, np.float64)).reshape(B, -1).max(axis=1))
    both_inf = np.isinf(ref[:, MARGIN]) & (rep[:, MARGIN] == ref[:, MARGIN])
    dm = np.where(both_inf, 0.0, np.abs(rep[:, MARGIN] - np.where(both_inf, 0.0, ref[:, MARGIN])))
    ds = np.abs(rep[:, SWING] - ref[:, SWING])
    return rel_err(rep[:, :2], ref[:, :2]), float((np.maximum(dm, ds) / scale).max())


# ---- the GPU tests' inputs

def random_u(bt, seed, scale=60.0):
    """A random force sequence: stance entries U(-scale, scale) with f_z >= 0 mostly, a quarter of
    the swing entries non-zero."""
    rng = np.random.default_rng(seed)
    ct = bt["contact"]
    B, N = ct.shape[:2]
    U = rng.uniform(-scale, scale, (B, N, 4, 3))
    U[..., 2] = rng.uniform(-0.2 * scale, 2 * scale, (B, N, 4))
    keep = (ct > 0) | (rng.random((B, N, 4)) < 0.25)
    return (U * keep[..., None]).reshape(B, N, NU).astype(np.float32)


def full_weights(seed=7):
    """A full symmetric Q (the diagonal scaled by a correlation matrix) and an R coupling every
    pair of legs."""
    rng = np.random.default_rng(seed)
    C = np.eye(NX)
    for _ in range(12):
        i, j = rng.choice(12, size=2, replace=False)
        C[i, j] = C[j, i] = rng.uniform(-0.3, 0.3)
    sq = np.sqrt(Q_DIAG)
    Q = np.outer(sq, sq) * C
    A = rng.standard_normal((NU, NU))
    Cr = A @ A.T / 12.0 + 0.5 * np.eye(NU)
    dr = np.sqrt(np.diag(Cr))
    R = 1e-5 * Cr / np.outer(dr, dr)
    return 0.5 * (Q + Q.T), 0.5 * (R + R.T)


GAITS = ("trot10", "pace10", "bound8", "standing")
ROBOTS = ("a1", "aliengo")


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """name -> dict(N, bt, U, Q, R, ref): the inputs of tests/test_gpu_predict.py's comparisons with
    this restatement, and predict_batch of them (computed once, never modified)."""
    from mpcqp.synthetic import make_batch
    cases = {}

    def add(name, N, B, seed, Q=Q_DIAG, R=R_DIAG, tilt=None):
        bt = make_batch(B, N, seed=seed, gaits=GAITS, robots=ROBOTS)
        rng = np.random.default_rng(seed + 1)
        if tilt is not None:                      # every normal tilted by `tilt` rad, any azimuth
            az = rng.uniform(0, 2 * np.pi, B)
            bt["robot"][:, 9:12] = np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az),
                                             np.full(B, np.cos(tilt))], axis=1).astype(np.float32)
        # contact values other than 1 scale the foot-step's bound; -inf and NaN are swing
        ct = bt["contact"]
        stance = ct > 0
        ct[stance & (rng.random(ct.shape) < 0.1)] = 0.5
        ct[~stance & (rng.random(ct.shape) < 0.05)] = -np.inf
        ct[~stance & (rng.random(ct.shape) < 0.05)] = np.nan
        U = random_u(bt, seed + 2)
        cases[name] = dict(N=N, bt=bt, U=U, Q=Q, R=R, ref=predict_batch(N, bt, U, Q, R))

    add("mixed_N10", 10, 131, 31)
    add("long_N32", 32, 3, 32)
    add("short_N1", 1, 2, 33)
    Qf, Rf = full_weights()
    add("full_N10", 10, 9, 34, Q=Qf, R=Rf)
    add("tilted_N10", 10, 9, 35, tilt=0.3)
    add("full_N32", 32, 3, 36, Q=Qf, R=Rf)       # the largest instantiation: 32 stages and full weights
    return cases

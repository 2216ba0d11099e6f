"""Float64 restatement of the base-state estimator (mpcqp_estimate), batched with NumPy:
one tick of the 18-state IMU + leg-kinematics Kalman filter of doc/state_estimation_kf.md
(second stage) for B robots, in two forms -- the batch update through numpy.linalg.solve and
the 28 scalar updates in sequence -- plus the record's packing helpers and a seeded
generator of test trajectories.  The reference raises NotImplementedError where this filter
would sit, so there is no program to record a fixture from: this restatement of the doc's
equations is the oracle, checked against known answers and against its own second form
(tests/test_est.py)."""
import numpy as np

import kin_ref

STRIDE = 352            # MPCQP_EST_STRIDE
DOF_STATES = 1          # MPCQP_EST_DOF_STATES
NX, NY = 18, 28
INIT, P_OFF = 18, 24
STATUS_NONFINITE = 4
DEFAULTS = dict(dt=0.001, gravity=9.81, sigma_p=0.001, sigma_v=0.0098, sigma_f=0.002, r_p=0.001, r_v=0.1,
                r_z=0.001, suspicion=100.0, p0=100.0, contact_height=0.0)
GEOMETRY = {"a1": (0.183, 0.047, 0.08505, 0.2, 0.2), "aliengo": (0.2399, 0.051, 0.083, 0.25, 0.25)}
CROUCH = (0.0, 0.8, -1.6)
INPUTS = ("quat", "gyro", "accel", "q", "qdot", "trust", "geom")
# the batch form against the sequential form over make_trajectory(8, 400, seed=7), norm-wise
# per robot, largest over ticks and robots, as tests/test_est.py measures and prints it: the
# problem's rounding sensitivity d, from which tests/test_gpu_est.py takes its bounds
D_X, D_P = 1.94e-11, 4.8e-15
# the same figure for the long regimes of regime_trajectory(7, 200) below, where the generator's
# d does not hold (tests/test_est.py measures and prints them): regime -> (d_x, d_P)
D_REGIME = {"swing": (7.17e-12, 1.95e-14), "stance": (5.86e-11, 1.96e-15), "noiseless": (8.56e-10, 1.96e-15)}
REGIME_SEED = 11


def measurement_matrix():
    C = np.zeros((NY, NX))
    for i in range(4):
        for k in range(3):
            C[3 * i + k, k] = 1.0
            C[3 * i + k, 6 + 3 * i + k] = -1.0
            C[12 + 3 * i + k, 3 + k] = 1.0
        C[24 + i, 8 + 3 * i] = 1.0
    return C


C = measurement_matrix()


def pack(x, P, initialised=1.0):
    """x [B,18], P [B,18,18] -> records [B,STRIDE]."""
    x, P = np.asarray(x, np.float64), np.asarray(P, np.float64)
    rec = np.zeros((x.shape[0], STRIDE))
    rec[:, :NX] = x
    rec[:, INIT] = initialised
    rec[:, P_OFF:P_OFF + NX * NX] = P.reshape(-1, NX * NX)
    return rec


def unpack(rec):
    """records [B,STRIDE] -> x [B,18], P [B,18,18], initialised [B]."""
    rec = np.asarray(rec, np.float64)
    return rec[:, :NX].copy(), rec[:, P_OFF:P_OFF + NX * NX].reshape(-1, NX, NX).copy(), rec[:, INIT].copy()


def geometry(names):
    """[B,8] geometry records (MPCQP_KIN_STRIDE) of the named robots."""
    g = np.zeros((len(names), kin_ref.STRIDE))
    g[:, :5] = [GEOMETRY[n] for n in names]
    return g


def estimate_step(state, inputs, constants=None, form="batch"):
    """One tick.  state [B,STRIDE]; inputs: dict of quat [B,4] (w, x, y, z), gyro, accel
    [B,3], q, qdot [B,12], trust [B,4] (float32 values) and geom [B,>=5] float64.  Returns
    (new state, dict(root_states [B,13], feet_world [B,4,3], status [B])), float64."""
    c = dict(DEFAULTS, **(constants or {}))
    state = np.asarray(state, np.float64)
    B = state.shape[0]
    f64 = lambda k: np.asarray(inputs[k]).astype(np.float64)
    quat, w, ab, q, qd, tr, geom = (f64(k) for k in INPUTS)
    bad = ~np.all([np.isfinite(a.reshape(B, -1)).all(1) for a in (quat, w, ab, q, qd, tr, geom[:, :5])], axis=0)
    # an initialised record (any non-zero word, NaN included) with a non-finite x, P or
    # `initialised` word is refused like a non-finite input; a fresh record is not read
    used = np.concatenate([state[:, :NX + 1], state[:, P_OFF:P_OFF + NX * NX]], axis=1)
    bad |= (state[:, INIT] != 0.0) & ~np.isfinite(used).all(1)
    with np.errstate(all="ignore"):
        Rq = kin_ref.quat2matrix_eigen(quat)
        p, _, Jb = kin_ref.chain(geom, q)
        world = lambda v: np.einsum("brc,blc->blr", Rq, v)
        r = world(p)
        rd = world(np.cross(w[:, None], p) + np.einsum("blrc,blc->blr", Jb, qd.reshape(B, 4, 3)))
        t = np.clip(tr, 0.0, 1.0)
        k = 1.0 + (1.0 - t) * c["suspicion"]
        a = np.einsum("brc,bc->br", Rq, ab)
        a[:, 2] -= c["gravity"]
        wworld = np.einsum("brc,bc->br", Rq, w)

        x0, P0, init = unpack(state)
        fresh = init == 0.0
        x0[fresh] = 0.0
        P0[fresh] = c["p0"] * np.eye(NX)
        y = np.concatenate([(-r).reshape(B, 12),
                            ((1.0 - t)[..., None] * x0[:, None, 3:6] + t[..., None] * (-rd)).reshape(B, 12),
                            t * c["contact_height"] + (1.0 - t) * (x0[:, 2:3] + r[..., 2])], axis=1)
        dt = c["dt"]
        A = np.eye(NX)
        A[0:3, 3:6] = dt * np.eye(3)
        Bm = np.zeros((NX, 3))
        Bm[0:3], Bm[3:6] = 0.5 * dt * dt * np.eye(3), dt * np.eye(3)
        kk = np.repeat(k, 3, axis=1)                                   # [B,12]
        Q = dt * np.concatenate([np.full((B, 3), c["sigma_p"]), np.full((B, 3), c["sigma_v"]), c["sigma_f"] * kk], 1)
        R = np.concatenate([np.full((B, 12), c["r_p"]), c["r_v"] * kk, c["r_z"] * k], 1)
        x = x0 @ A.T + a @ Bm.T
        P = A @ P0 @ A.T
        P[:, np.arange(NX), np.arange(NX)] += Q
        if form == "batch":
            CP = C @ P                                                  # [B,28,18]
            S = CP @ C.T
            S[:, np.arange(NY), np.arange(NY)] += R
            ok = np.isfinite(S).all((1, 2))
            S[~ok] = np.eye(NY)
            K = np.swapaxes(np.linalg.solve(S, CP), 1, 2)               # P C^T S^-1 (S symmetric)
            x = x + np.einsum("bij,bj->bi", K, y - x @ C.T)
            P = P - K @ CP
        elif form == "sequential":
            for m in range(NY):
                h = P @ C[m]                                            # [B,18]
                s = h @ C[m] + R[:, m]
                g = h / s[:, None]
                x = x + g * (y[:, m] - x @ C[m])[:, None]
                P = P - g[:, :, None] * h[:, None, :]
        else:
            raise ValueError(form)
        P = 0.5 * (P + np.swapaxes(P, 1, 2))
    new = state.copy()
    good = ~bad
    new[good] = pack(x[good], P[good])
    xo = np.where(bad[:, None], x0, x)
    root = np.concatenate([xo[:, 0:3], quat[:, 1:4], quat[:, 0:1], xo[:, 3:6], wworld], axis=1)
    return new, dict(root_states=root, feet_world=xo[:, 6:].reshape(B, 4, 3),
                     status=np.where(bad, STATUS_NONFINITE, 0).astype(np.int32))


def level_crouch(B, robot="aliengo", gravity=9.81):
    """The sensors of a robot standing level in the crouch, all feet trusted (float32)."""
    f = np.float32
    return dict(quat=np.tile(f([1, 0, 0, 0]), (B, 1)), gyro=np.zeros((B, 3), f),
                accel=np.tile(f([0, 0, gravity]), (B, 1)), q=np.tile(f(CROUCH * 4), (B, 1)),
                qdot=np.zeros((B, 12), f), trust=np.ones((B, 4), f), geom=geometry([robot] * B))


def tilted_one_foot(B, foot=2, robot="a1", gravity=9.81, seed=5):
    """A tilted base at rest with perturbed joints and only `foot` trusted; accel is the
    float32 rounding of R_q^T (0, 0, g)."""
    rng = np.random.default_rng(seed)
    f = np.float32
    quat = np.array([0.98, 0.1, -0.12, 0.05])
    quat = np.tile((quat / np.linalg.norm(quat)).astype(f), (B, 1))
    Rq = kin_ref.quat2matrix_eigen(quat)
    trust = np.zeros((B, 4), f)
    trust[:, foot] = 1.0
    q = (np.tile(CROUCH * 4, (B, 1)) + rng.uniform(-0.2, 0.2, (B, 12))).astype(f)
    return dict(quat=quat, gyro=np.zeros((B, 3), f), accel=(Rq[:, 2, :] * gravity).astype(f), q=q,
                qdot=np.zeros((B, 12), f), trust=trust, geom=geometry([robot] * B))


def make_trajectory(B, T, seed):
    """Seeded sensor streams for T ticks of B robots: a list of T input dicts (float32,
    geom float64).  Quaternions near level and near unit length, gyro, accelerometer around
    gravity, joints around the crouch, trust patterns mixing 0, 1 and fractions with
    all-swing and all-stance ticks, A1 and Aliengo geometry alternating."""
    rng = np.random.default_rng(seed)
    f = np.float32
    geom = geometry([("a1", "aliengo")[b % 2] for b in range(B)])
    t = 0.001 * np.arange(T)[:, None]
    ph = rng.uniform(0, 2 * np.pi, (B, 3))
    rpy = np.stack([0.05 * np.sin(9 * t + ph[:, 0]), 0.04 * np.sin(7 * t + ph[:, 1]),
                    rng.uniform(-1, 1, B) + 0.2 * t], -1)
    cs, sn = np.cos(rpy / 2), np.sin(rpy / 2)
    cr, cp, cy, sr, sp, sy = cs[..., 0], cs[..., 1], cs[..., 2], sn[..., 0], sn[..., 1], sn[..., 2]
    quat = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy,
                     cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], -1)
    quat = quat * (1.0 + 1e-3 * rng.standard_normal((T, B, 1)))         # unit-ish, as an IMU delivers it
    gyro = np.stack([0.45 * np.cos(9 * t + ph[:, 0]), 0.28 * np.cos(7 * t + ph[:, 1]), 0.2 + 0 * t + 0 * ph[:, 2]], -1)
    accel = np.array([0.0, 0.0, 9.81]) + 0.6 * np.sin(11 * t[..., None] + ph[None]) + 0.05 * rng.standard_normal((T, B, 3))
    lp = rng.uniform(0, 2 * np.pi, (B, 12))
    amp = np.tile([0.1, 0.3, 0.3], 4)
    q = np.tile(CROUCH, 4) + amp * np.sin(12 * t[..., None] + lp)
    qdot = 12 * amp * np.cos(12 * t[..., None] + lp)
    # trust: a trot-like ramp per leg, then overwritten on some ticks by the corner cases
    leg_ph = rng.uniform(0, 1, (B, 4))
    cyc = (t[..., None] / 0.06 + leg_ph) % 1.0
    trust = np.clip(np.minimum(cyc, 0.6 - cyc) / 0.08, 0.0, 1.0)        # 0 in swing, ramps to 1 in stance
    kind = rng.integers(0, 10, (T, B))
    trust[kind == 0] = 0.0                                              # an all-swing tick
    trust[kind == 1] = 1.0                                              # an all-stance tick
    hard = (kind == 2)[..., None] & np.ones(4, bool)
    trust[hard] = rng.integers(0, 2, int(hard.sum()))                   # a touch sensor's 0 / 1
    out = rng.uniform(-0.5, 1.5, (T, B, 4))
    trust = np.where((kind == 3)[..., None], out, trust)                # outside [0, 1]: clipped by the filter
    return [dict(quat=quat[i].astype(f), gyro=gyro[i].astype(f), accel=accel[i].astype(f), q=q[i].astype(f),
                 qdot=qdot[i].astype(f), trust=trust[i].astype(f), geom=geom) for i in range(T)]


# ---- edge inputs shared by tests/test_est.py (the kernel on host threads) and
# tests/test_gpu_est_edges.py (the device)
NONFINITE = (np.nan, np.inf, -np.inf)
WIDTH = dict(quat=4, gyro=3, accel=3, q=12, qdot=12, trust=4, geom=5)
DIRTY = (1, 5, 6)          # of B = 7: a middle slot, the second workgroup's last slot, the tail
TRUST_OUTSIDE = np.float32([-0.0, 1.0 + 2.0 ** -23, 3e38, -3e38])      # behaves as ...
TRUST_CLIPPED = np.float32([0.0, 1.0, 1.0, 0.0])
TRUST_INSIDE = np.float32([1e-45, 1.0 - 2.0 ** -24, 0.5, 0.25])        # a subnormal, one ulp under 1
# words of the record for a non-finite value: x_0, x_4, x_17, P[0][0], P[4][4], P[17][17],
# P[2][11], P[11][2], P[17][0], and the `initialised` word
RECORD_WORDS = (0, 4, 17, P_OFF, P_OFF + 4 * NX + 4, P_OFF + 17 * NX + 17, P_OFF + 2 * NX + 11, P_OFF + 11 * NX + 2,
                P_OFF + 17 * NX, INIT)
PADDING = tuple(range(19, 24)) + tuple(range(348, 352))


def nonfinite_cases():
    """One launch per (input, element) of a robot: [(key, element, value, dirty robot)], the
    value alternating NaN / +inf / -inf and the robot rotating through DIRTY.  43 cases."""
    cases = [(k, e) for k in INPUTS for e in range(WIDTH[k])]
    return [(k, e, NONFINITE[i % 3], DIRTY[i % 3]) for i, (k, e) in enumerate(cases)]


def dof_cases():
    """The same in the dof-state layout: a position and a velocity slot of each leg, as
    (key, element, value, dirty robot) on the split arrays.  8 cases."""
    cases = [(("q", "qdot")[s], 3 * leg + (leg + s) % 3) for leg in range(4) for s in range(2)]
    return [(k, e, NONFINITE[i % 3], DIRTY[i % 3]) for i, (k, e) in enumerate(cases)]


def poisoned(inp, key, element, value, robot):
    out = {k: v.copy() for k, v in inp.items()}
    out[key][robot, element] = value
    return out


def record_cases():
    """A non-finite word in an initialised record: [(word, value, dirty robot)], robots 2 (a
    workgroup's last slot) and 6 (the tail) of B = 7."""
    return [(w, np.nan if w == INIT else NONFINITE[i % 3], (2, 6)[i % 2]) for i, w in enumerate(RECORD_WORDS)]


def quat_variants(quat):
    """quat [B,4] float32 -> the same attitude given as 2 q, q / 2, 0 and -q."""
    quat = np.asarray(quat, np.float32)
    return dict(double=quat * np.float32(2), half=quat * np.float32(0.5), zero=np.zeros_like(quat), negated=-quat)


def regime_trajectory(B, T, regime):
    """The generator's trajectory held in one regime for T ticks: `swing` (every trust 0),
    `stance` (every trust 1) or `noiseless` (the generator's trust, sigma_p = sigma_v = sigma_f =
    suspicion = 0).  Returns (trajectory, constants)."""
    traj = make_trajectory(B, T, seed=REGIME_SEED)
    if regime == "noiseless":
        return traj, dict(sigma_p=0.0, sigma_v=0.0, sigma_f=0.0, suspicion=0.0)
    value = np.float32({"swing": 0.0, "stance": 1.0}[regime])
    return [dict(t, trust=np.full_like(t["trust"], value)) for t in traj], None


def same_bits(a, b):
    """Bitwise equality: NaN payloads and the sign of zero count."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_refused(start, quat, clean, dirty, robot, skip=(), tag=None):
    """What a refusal is.  `clean` and `dirty` are (records, outputs) of the same launch from
    the records `start` without and with the non-finite value, sentinel rows included; `quat`
    is the dirty launch's.  The dirty robot: status 4, its record bitwise as it was, position,
    velocity and feet the float32 of the old x, the orientation the input quaternion's bits;
    every other row, sentinels included, bitwise the clean launch's."""
    (sc, oc), (sd, od) = clean, dirty
    f = np.float32
    assert same_bits(sd[robot], start[robot]), tag
    if "status" not in skip:
        assert od["status"][robot] == STATUS_NONFINITE, (tag, od["status"])
        assert oc["status"][robot] == 0, tag
    if "root_states" not in skip:
        root = od["root_states"][robot]
        assert same_bits(root[0:3], start[robot, 0:3].astype(f)) and same_bits(root[7:10], start[robot, 3:6].astype(f)), tag
        assert same_bits(root[3:7], np.asarray(quat, f)[robot, [1, 2, 3, 0]]), tag
    if "feet_world" not in skip:
        assert same_bits(od["feet_world"][robot].ravel(), start[robot, 6:18].astype(f)), tag
    others = [b for b in range(sd.shape[0]) if b != robot]
    assert same_bits(sd[others], sc[others]), tag
    for k in oc:
        assert same_bits(od[k][others], oc[k][others]), (tag, k)


def worst_err(states, ref):
    """Largest norm-wise distance per robot over the ticks of two [T+1,B,STRIDE] runs: (x, P)."""
    dx = dP = 0.0
    for i in range(1, len(ref)):
        xa, Pa, _ = unpack(states[i])
        xr, Pr, _ = unpack(ref[i])
        for b in range(xa.shape[0]):
            dx, dP = max(dx, norm_err(xa[b], xr[b])), max(dP, norm_err(Pa[b], Pr[b]))
    return dx, dP


def run(traj, constants=None, form="batch", state=None):
    """Every tick of a trajectory: ([T+1,B,STRIDE] records with the start first, list of outputs)."""
    B = traj[0]["quat"].shape[0]
    state = np.zeros((B, STRIDE)) if state is None else state
    states, outs = [state], []
    for inp in traj:
        state, out = estimate_step(state, inp, constants, form)
        states.append(state)
        outs.append(out)
    return np.stack(states), outs


def norm_err(a, ref):
    return kin_ref.norm_err(a, ref)

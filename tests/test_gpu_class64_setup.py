"""Class 64's per-robot setup (staging, model chain, H tile, post-sweep epilogue): cases
placed where its tile and table indexing can go wrong, against the float64 oracle.

Every case is generated once per process (seeded) together with its oracle optimum; the
oracle raises on an infeasible or unsolved QP, so a case that exists has been solved on the
CPU, and no test skips any."""
import functools
import math

import numpy as np
import pytest

from helpers import oracle_solution, rel_err_u0

TOL_ACHIEVED = 1e-5   # test_gpu_parity.TOL_ACHIEVED: what the dense classes deliver (~5e-7)

# stance foot-steps S of the tile-boundary case: n = 3 S = 3, 6, 15, 21, 33, 45, 57, 60
TILE_STANCE = (1, 2, 5, 7, 11, 15, 19, 20)
# float32(pi) = 3.1415927: the -3.1415927 of the float32 state is the -pi entry
YAWS = (0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi, 3.1415927, 1e-8, 40.0)


def _random_contacts(rng, N, stance):
    """One robot's (N, 4) contact table with exactly `stance` stance foot-steps."""
    c = np.zeros(4 * N, dtype=np.float32)
    c[rng.choice(4 * N, size=stance, replace=False)] = 1.0
    return c.reshape(N, 4)


def _with_oracle(bt, N, **kw):
    ref = [oracle_solution(bt, b, N, **kw)[0] for b in range(len(bt["x0"]))]
    return bt, np.stack(ref)


@functools.lru_cache(maxsize=None)
def _stance_case(N):
    """B = 16 robots with random contact patterns: at N = 10 two robots per TILE_STANCE
    count, at a short horizon counts drawn from 1..4N with both ends present."""
    from mpcqp.synthetic import make_batch
    B = 16
    rng = np.random.default_rng(5100 + N)
    bt = make_batch(B, N, seed=5000 + N, gaits=("trot10", "pace10", "bound8"), robots=("a1", "aliengo"),
                    tilt_deg=10.0)
    if N == 10:
        stance = list(TILE_STANCE) * 2
    else:
        stance = [1, 4 * N] + [int(s) for s in rng.integers(1, 4 * N + 1, size=B - 2)]
    for b in range(B):
        bt["contact"][b] = _random_contacts(rng, N, stance[b])
    assert [int(v) for v in bt["contact"].reshape(B, -1).sum(1)] == stance
    return _with_oracle(bt, N)


@functools.lru_cache(maxsize=None)
def _yaw_case():
    """B = 8, one robot per YAWS entry (state, reference and feet turned with it), a tilted
    surface normal on the odd robots."""
    from mpcqp.params import ROBOT_PRESETS, pack_robot
    from mpcqp.synthetic import make_batch
    N, B = 10, len(YAWS)
    bt = make_batch(B, N, seed=5200, gaits=("trot10", "pace10"), robots=("a1",))
    for b, yaw in enumerate(YAWS):
        d = yaw - float(bt["x0"][b, 2])
        c, s = math.cos(d), math.sin(d)
        bt["x0"][b, 2] = yaw
        bt["xref"][b, :, 2] += np.float32(d)
        fx, fy = bt["feet"][b, :, 0].copy(), bt["feet"][b, :, 1].copy()
        bt["feet"][b, :, 0] = c * fx - s * fy
        bt["feet"][b, :, 1] = s * fx + c * fy
        if b % 2:
            th, az = math.radians(5.0 + b), 0.7 * b
            normal = (math.sin(th) * math.cos(az), math.sin(th) * math.sin(az), math.cos(th))
            bt["robot"][b] = pack_robot(ROBOT_PRESETS["a1"], normal=normal)
    assert bt["x0"][5, 2] == bt["x0"][3, 2] == np.float32(3.1415927)
    return _with_oracle(bt, N)


def _coupled_weights():
    """Q coupling state components and an R coupling the force components inside each leg
    and across two legs (the non-diagonal instantiation)."""
    from mpcqp.params import Q_DIAG, R_DIAG
    rng = np.random.default_rng(5300)
    Q = np.diag(np.asarray(Q_DIAG, np.float64))
    sq = np.sqrt(np.diag(Q))
    for i, j in ((0, 1), (3, 9), (4, 10), (6, 8)):
        Q[i, j] = Q[j, i] = 0.3 * sq[i] * sq[j]
    R = np.diag(np.asarray(R_DIAG, np.float64))
    for leg in range(4):
        S = rng.uniform(-0.3, 0.3, size=(3, 3))
        R[3 * leg:3 * leg + 3, 3 * leg:3 * leg + 3] += 1e-5 * (S @ S.T)
    R[1, 7] = R[7, 1] = 3e-6
    assert np.linalg.eigvalsh(Q).min() > -1e-12 and np.linalg.eigvalsh(R).min() > 0
    return Q, R


@functools.lru_cache(maxsize=None)
def _full_case():
    from mpcqp.synthetic import make_batch
    N, B = 10, 4
    bt = make_batch(B, N, seed=5400, gaits=("trot10", "bound8"), robots=("a1", "aliengo"), tilt_deg=10.0)
    Q, R = _coupled_weights()
    return _with_oracle(bt, N, Q=Q, R=R) + (Q, R)


def _check(bt, ref, N, **kw):
    from mpcqp import LinearMpc
    eng = LinearMpc(horizon=N, robot="a1", **kw)
    res = eng.solve(bt["x0"], bt["xref"], bt["contact"], bt["feet"], robot=bt["robot"], return_all=True)
    B = len(bt["x0"])
    u0 = res.u0.cpu().numpy()
    U = res.U.cpu().numpy().reshape(B, -1)
    status = res.status.cpu().numpy()
    errs = [max(rel_err_u0(u0[b], ref[b][:12]), rel_err_u0(U[b], ref[b])) for b in range(B)]
    print("worst relative error per robot:", " ".join(f"{e:.1e}" for e in errs))
    assert (status == 0).all(), status
    assert max(errs) < TOL_ACHIEVED, (int(np.argmax(errs)), max(errs))


def test_cases_solve_on_the_oracle():
    """Every case is built (the oracle raises on an infeasible or unsolved QP); its optimum
    is finite, zero on the swing foot-steps and not zero on the others."""
    cases = [_stance_case(N)[:2] for N in (10, 1, 2, 3)] + [_yaw_case(), _full_case()[:2]]
    for bt, ref in cases:
        B = len(ref)
        assert np.isfinite(ref).all()
        f = np.abs(ref.reshape(B, -1, 3)).max(2)
        swing = bt["contact"].reshape(B, -1) <= 0
        assert (f[swing] < 1e-9).all() and (f.max(1) > 1e-3).all()


@pytest.mark.gpu
def test_tile_boundary_stance_counts():
    """n = 3, 6, 15, 21, 33, 45, 57, 60 from random contact patterns: foot-steps straddling the
    4-row / 8-column register tiles and identity padding inside a tile (the H tile's table
    lookups, the 3 x 3 block extraction after the sweep)."""
    bt, ref = _stance_case(10)
    _check(bt, ref, 10)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 3])
def test_short_horizons(N):
    """The smallest step-pair tables: N = 1, 2, 3 with 1..4N stance foot-steps."""
    bt, ref = _stance_case(N)
    _check(bt, ref, N)


@pytest.mark.gpu
def test_yaw_values():
    """cos / sin of the yaw at 0, +-pi/2, +-pi (the float32 pi), 1e-8 and 40 rad, flat and
    tilted surface normals."""
    bt, ref = _yaw_case()
    _check(bt, ref, 10)


@pytest.mark.gpu
def test_full_weights_coupled_r():
    """Non-diagonal Q and a coupled R through one set_weights call (the full-weights
    instantiation keeps its own H build)."""
    bt, ref, Q, R = _full_case()
    _check(bt, ref, 10, Q=Q, R=R)

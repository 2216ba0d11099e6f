"""CPU: the terrain plane (mpcqp_terrain) without a GPU -- the ABI surface, the float64
restatement tests/terrain_ref.py against known answers and against the reference's recorded run
(tests/golden/terrain.npz, made by tests/golden/make_golden_terrain.py from the reference's own
update_terrain_normal), and the per-robot header csrc/mpcqp_terrain_robot.h compiled with g++
and driven through ctypes against it; the ground terms of csrc/mpcqp_swing_leg.h.

Measured here (printed by the tests):
  known answers on the host-compiled header: a level square gives n = (0, 0, 1) and d exactly;
    a plane of known tilt 1.4e-16 against eigh on the float32 feet (3.3e-8 against the plane
    itself, the float32 rounding of the feet); ter_eig against numpy.linalg.eigh over 300 random
    scatter matrices 2.3e-15; 18 of 72 raw Jacobi vectors come out with n_z < 0 and are flipped.
  the host-compiled header against terrain_ref over make_trajectory(8, 120, seed=11), both contact
    rules: history, fitted and status equal, n and d within D = 1.11e-15 (norm_err: n in the max
    norm, d relative to max(1, |mu|)); over the GPU tests' trajectory (131 robots x 24 ticks)
    1.04e-15: terrain_ref.D_N = 1.1e-15.  The float32 outputs are bitwise terrain_ref's.
  the normal against the generator's true plane after 120 ticks: 7.2e-3 (the z noise of up to
    1e-2 m over the footprint).
  the reference's recorded vector (a row of the eigenvector matrix) differs from the eigenvector
    by up to 1.4 in the fixture; our n agrees with numpy.linalg.eigh's column to 1.0e-15.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import terrain_edge_checks as edge
import terrain_ref as tr
from helpers import _declared, host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpcqp.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "terrain.npz")
NEW_SYMBOLS = {"mpcqp_terrain", "mpcqp_set_terrain", "mpcqp_set_ground"}
KNOWN = 1e-12
F32_BOUND = 2.4e-7      # two float32 ulps norm-wise, the project's floor for a float32 store
SENTINEL = -77

SHIM = r'''
#include "mpcqp_terrain_robot.h"
#include "mpcqp_swing_leg.h"
// a launch of mpcqp_terrain_kernel, robot after robot; c: contact_threshold, flat_tol,
// cos_max_tilt, blend, touchdown_z
extern "C" void launch(const double* c, int flags, int B, const float* pos_feet, const float* contact,
                       const float* quat, double* st, float* robot, float* normal, float* plane,
                       float* normal_base, int32_t* status) {
  const TerParams tp{c[0], c[1], c[2], c[3], flags, c[4]};
  for (int b = 0; b < B; ++b)
    ter_robot(tp, (size_t)b, pos_feet, contact, quat, st, robot, normal, plane, normal_base, status);
}
extern "C" void eig(const double* S, double* l, double* v) { ter_eig(S, l, v); }
extern "C" int stride(void) { return TER_STRIDE; }
extern "C" int flag_swing(void) { return TER_SWING_STATE; }
extern "C" int flag_root(void) { return TER_ROOT_STATES; }
extern "C" int flag_ground(void) { return TER_GROUND; }
// in: t_swing, t_stance, dt, finished, pos[3], vel[3], R[9], vbody[3], yaw_rate, thigh[3], foot[3],
// gravity, vel_gain, touchdown_z, swing_height (33 doubles); which: 0 swing_leg_step, 1 _ground
extern "C" void leg_step(int which, double* mem, const double* in, const double* ground, double* pb, double* vb) {
  const double *pos = in + 4, *vel = in + 7, *R = in + 10, *vbody = in + 19, *thigh = in + 23, *foot = in + 26;
  if (which == 0)
    swing_leg_step(mem, in[3] != 0.0, in[2], in[0], in[1], pos, vel, R, vbody, in[22], thigh, foot, in[29], in[30],
                   in[31], in[32], pb, vb);
  else
    swing_leg_step_ground(mem, in[3] != 0.0, in[2], in[0], in[1], pos, vel, R, vbody, in[22], thigh, foot, in[29],
                          in[30], in[31], in[32], pb, vb, ground);
}
'''


def test_header_declares_the_terrain_entry_points_and_binding_agrees():
    from mpcqp import _lib
    assert NEW_SYMBOLS <= _declared()
    assert _declared() == set(_lib.EXPORTED_SYMBOLS)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.mpcqp_abi_version() == 6     # additive: the ABI version stays


def test_constants_match_binding(robot):
    from mpcqp import _lib
    src = open(HEADER).read()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", src).group(1))
    assert define("MPCQP_TERRAIN_STRIDE") == _lib.TERRAIN_STRIDE == tr.STRIDE == robot.stride() == 20
    assert define("MPCQP_TERRAIN_SWING_STATE") == _lib.TERRAIN_SWING_STATE == tr.SWING_STATE == robot.flag_swing()
    assert define("MPCQP_TERRAIN_ROOT_STATES") == _lib.TERRAIN_ROOT_STATES == tr.ROOT_STATES == robot.flag_root()
    assert define("MPCQP_TERRAIN_GROUND") == _lib.TERRAIN_GROUND == tr.GROUND == robot.flag_ground() == 4
    assert tr.STATUS_NONFINITE == _lib.STATUS_NONFINITE


def test_null_ctx_is_an_error_code():
    from mpcqp import _lib
    lib = _lib.load()
    assert lib.mpcqp_terrain(None, 1, 0, *([None] * 10)) == -1
    assert lib.mpcqp_set_terrain(None, 0.5, 1e-3, 0.5, 1.0) == -1
    assert lib.mpcqp_set_ground(None, None, 0) == -1


def test_python_surface():
    import mpcqp
    from mpcqp.engine import LinearMpc
    assert "BatchedTerrain" in mpcqp.__all__
    for name in ("terrain", "set_terrain", "set_ground"):
        assert getattr(LinearMpc, name).__doc__


@pytest.fixture(scope="module")
def robot():
    lib = host_build(SHIM, name="terrain")
    vp = ctypes.c_void_p
    lib.launch.argtypes = [vp, ctypes.c_int, ctypes.c_int] + [vp] * 9
    lib.launch.restype = None
    lib.eig.argtypes = [vp] * 3
    lib.leg_step.argtypes = [ctypes.c_int] + [vp] * 5
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_launch(lib, state, inp, constants=None, pad=2, skip=(), ground=False, touchdown_z=tr.TOUCHDOWN_Z):
    """A launch on the host, on `state` [B + pad, STRIDE] in place; the outputs come back with
    their `pad` sentinel rows.  `skip`: outputs passed as NULL.  `ground`: MPCQP_TERRAIN_GROUND."""
    B = state.shape[0] - pad
    c = dict(tr.DEFAULTS, **(constants or {}))
    cv = np.array([c[k] for k in ("contact_threshold", "flat_tol", "cos_max_tilt", "blend")] + [touchdown_z])
    flags = tr.GROUND if ground else 0
    if "swing_state" in inp:
        flags |= tr.SWING_STATE
        contact = np.ascontiguousarray(inp["swing_state"], np.float32)
    else:
        contact = np.ascontiguousarray(inp["contact"], np.float32)
    quat = None
    if inp.get("root_states") is not None:
        flags |= tr.ROOT_STATES
        quat = np.ascontiguousarray(inp["root_states"], np.float32)
    elif inp.get("quat") is not None:
        quat = np.ascontiguousarray(inp["quat"], np.float32)
    out = dict(normal=np.full((B + pad, 3), SENTINEL, np.float32), plane=np.full((B + pad, 4), SENTINEL, np.float32),
               normal_base=np.full((B + pad, 3), SENTINEL, np.float32),
               status=np.full((B + pad,), SENTINEL, np.int32))
    if quat is None:
        skip = tuple(skip) + ("normal_base",)
    rob = None
    if inp.get("robot") is not None:
        rob = out["robot"] = np.ascontiguousarray(inp["robot"], np.float32).copy()
    feet = np.ascontiguousarray(inp["pos_feet"], np.float32)
    a = {k: (None if k in skip else v) for k, v in out.items()}
    lib.launch(_p(cv), flags, B, _p(feet), _p(contact), _p(quat), _p(state), _p(rob), _p(a["normal"]),
               _p(a["plane"]), _p(a["normal_base"]), _p(a["status"]))
    return out


def one(lib, feet, contact=(1, 1, 1, 1), state=None, constants=None, **kw):
    """One robot, one tick on the host: (record, outputs without the sentinel rows)."""
    st = np.full((3, tr.STRIDE), float(SENTINEL))
    st[0] = 0.0 if state is None else state
    out = host_launch(lib, st, dict(pos_feet=np.float32(feet).reshape(1, 4, 3), contact=np.float32([contact]), **kw),
                      constants)
    assert (st[1:] == SENTINEL).all() and all((v[1:] == SENTINEL).all() for k, v in out.items() if k != "robot")
    return st[0].copy(), {k: v[0] for k, v in out.items()}


SQUARE = np.array([[0.2, 0.13, 0], [0.2, -0.13, 0], [-0.2, 0.13, 0], [-0.2, -0.13, 0]], np.float64)


def on_plane(n, d, xy=SQUARE[:, :2]):
    n = np.asarray(n, np.float64) / np.linalg.norm(n)
    z = (d - n[0] * xy[:, 0] - n[1] * xy[:, 1]) / n[2]
    return np.concatenate([xy, z[:, None]], axis=1), n


# ---- known answers

def test_level_square(robot):
    feet = SQUARE + [3.0, -2.0, 0.75]
    st, out = one(robot, feet)
    assert st[tr.N].tolist() == [0.0, 0.0, 1.0] and st[tr.FITTED] == 1 and st[tr.INIT] == 1
    assert st[tr.D] == np.float32(0.75) and out["status"] == 0 and (st[18:] == 0).all()
    assert out["normal"].tolist() == [0, 0, 1] and out["plane"].tolist() == [0, 0, 1, 0.75]
    assert np.array_equal(st[tr.HIST], np.float32(feet).astype(np.float64).reshape(12))


def test_known_tilt(robot):
    feet, n = on_plane([0.2, -0.1, 1.0], 0.3)
    feet32 = np.float32(feet)
    st, out = one(robot, feet32)
    # the float32 rounding of the feet moves them off the plane by 3e-8: fit the rounded points
    _, _, nf = tr.fit(feet32.astype(np.float64)[None])
    err = np.abs(st[tr.N] - nf[0]).max()
    print(f"\nknown tilt: against eigh {err:.2e}, against the plane {np.abs(st[tr.N] - n).max():.2e}")
    assert err < KNOWN and np.abs(st[tr.N] - n).max() < 1e-6 and st[tr.FITTED] == 1
    assert abs(st[tr.D] - 0.3) < 1e-6 and abs(np.linalg.norm(st[tr.N]) - 1) < KNOWN


def test_collinear_and_coincident_feet_are_held(robot):
    line = np.array([[0.1 * i, 0.2 * i, 0.05 * i] for i in range(4)])
    point = np.tile([1.0, 2.0, 0.5], (4, 1))
    tilted, n = on_plane([0.2, -0.1, 1.0], 0.3)
    seeded, _ = one(robot, tilted)
    for feet in (line, point):
        st, out = one(robot, feet)                       # from a cold record: n stays (0, 0, 1)
        assert st[tr.N].tolist() == [0, 0, 1] and st[tr.FITTED] == 0 and out["status"] == 0 and st[tr.INIT] == 1
        st, out = one(robot, feet, state=seeded)         # from a fitted record: n stays what it was
        assert np.array_equal(st[tr.N], seeded[tr.N]) and st[tr.FITTED] == 0
        mu = np.float32(feet).astype(np.float64).mean(axis=0)
        assert abs(st[tr.D] - seeded[tr.N] @ mu) < KNOWN     # d follows the centroid either way


def test_tilt_past_the_limit_is_held(robot):
    feet, n = on_plane([np.tan(1.2), 0.0, 1.0], 0.0)      # 1.2 rad > acos(0.5)
    st, _ = one(robot, feet)
    assert st[tr.N].tolist() == [0, 0, 1] and st[tr.FITTED] == 0
    st, _ = one(robot, feet, constants=dict(cos_max_tilt=0.3))
    assert st[tr.FITTED] == 1 and np.abs(st[tr.N] - n).max() < 1e-6


def test_blend_follows_the_recursion(robot):
    feet, nt = on_plane([0.3, 0.2, 1.0], 0.1)
    st, _ = one(robot, feet, constants=dict(blend=0.25))
    _, _, nf = tr.fit(np.float32(feet).astype(np.float64)[None])
    n = np.array([0.0, 0.0, 1.0])
    for k in range(5):
        n = 0.75 * n + 0.25 * nf[0]
        n /= np.linalg.norm(n)
        assert np.abs(st[tr.N] - n).max() < KNOWN, k
        st, _ = one(robot, feet, state=st, constants=dict(blend=0.25))


def test_raw_vector_with_negative_z_is_flipped(robot):
    """Over planes of three slopes and many azimuths the Jacobi vector comes out with either sign: both occur,
    and the stored normal has n_z > 0 every time."""
    raw_neg = 0
    for k in range(72):
        az, slope = 2 * np.pi * (k % 24) / 24 + 0.1, (0.4, 1.1, 1.5)[k // 24]
        feet, n = on_plane([slope * np.cos(az), slope * np.sin(az), 1.0], 0.2)
        f64 = np.float32(feet).astype(np.float64)
        X = f64 - f64.mean(axis=0)
        S, l, v = np.ascontiguousarray(X.T @ X), np.zeros(3), np.zeros(3)
        robot.eig(_p(S), _p(l), _p(v))
        assert np.abs(S @ v - l[0] * v).max() < KNOWN and l[0] <= l[1] <= l[2]
        raw_neg += v[2] < 0
        st, _ = one(robot, feet)
        assert st[tr.N][2] > 0 and np.abs(st[tr.N] - n).max() < 1e-6
    print(f"\nraw vectors with n_z < 0: {raw_neg} of 72")
    assert 0 < raw_neg < 72


def test_eig_matches_eigh_on_random_scatter(robot):
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(300):
        X = rng.standard_normal((4, 3)) * rng.uniform(0.01, 3.0, 3)
        X -= X.mean(axis=0)
        S, l, v = np.ascontiguousarray(X.T @ X), np.zeros(3), np.zeros(3)
        robot.eig(_p(S), _p(l), _p(v))
        w, V = np.linalg.eigh(S)
        if (w[1] - w[0]) / w[2] < 0.05:
            continue
        ref = V[:, 0] * np.sign(V[:, 0] @ v)
        worst = max(worst, np.abs(v - ref).max(), np.abs(l - w).max() / w[2])
    print(f"\nter_eig against eigh: {worst:.2e}")
    assert worst < 2e-14


# ---- the header against terrain_ref over the trajectory

@pytest.fixture(scope="module")
def oracle():
    traj = tr.make_trajectory(8, 120, seed=11)
    return traj, *tr.run(traj)


def _follow(robot, traj, states, outs, rule):
    """The host-compiled header over a trajectory against terrain_ref's run of it: the exact
    parts asserted, (D, the float32 outputs' largest error) returned."""
    B = states.shape[1]
    st = np.vstack([np.zeros((B, tr.STRIDE)), np.full((2, tr.STRIDE), float(SENTINEL))])
    D = f32 = 0.0
    for t, step in enumerate(traj):
        out = host_launch(robot, st, {"pos_feet": step["pos_feet"], rule: step[rule], "quat": step["quat"]})
        assert np.array_equal(st[:B, tr.HIST], states[t][:, tr.HIST]), t            # bitwise
        assert np.array_equal(st[:B, [tr.INIT, tr.FITTED, 18, 19]], states[t][:, [tr.INIT, tr.FITTED, 18, 19]])
        assert np.array_equal(out["status"][:B], outs["status"][t])
        D = max(D, tr.norm_err(st[:B], states[t]))
        for k in ("normal", "plane", "normal_base"):
            scale = max(1.0, float(np.abs(outs[k][t]).max()))
            f32 = max(f32, float(np.abs(out[k][:B].astype(np.float64) - outs[k][t]).max()) / scale)
        assert (st[B:] == SENTINEL).all() and all((v[B:] == SENTINEL).all() for v in out.values())
    return D, f32


def test_header_matches_the_restatement(robot, oracle):
    """D over 8 robots x 120 ticks and over the trajectory of tests/test_gpu_terrain.py (131
    robots x 24 ticks), recorded as terrain_ref.D_N.  What bounds it: the eigenvector of l0 moves
    by eps l2 / (l1 - l0) per rounding of S, the generator keeps (l1 - l0) / l2 >= 0.05, and a
    handful of roundings reach S: 16 eps / 0.05 = 7.1e-14."""
    traj, states, outs = oracle
    worst = 0.0
    for rule in ("swing_state", "contact"):
        D, f32 = _follow(robot, traj, states, outs, rule)
        print(f"\n{rule}: record D = {D:.2e} (terrain_ref.D_N = {tr.D_N:.1e}), float32 outputs {f32:.2e}")
        worst = max(worst, D)
        assert f32 <= F32_BOUND
    gtraj = tr.make_trajectory(**tr.GPU_TRAJECTORY)
    D, f32 = _follow(robot, gtraj, *tr.run(gtraj), "swing_state")
    print(f"the GPU tests' trajectory: record D = {D:.2e}, float32 outputs {f32:.2e}")
    worst = max(worst, D)
    assert f32 <= F32_BOUND
    assert worst <= 16 * 2.0 ** -52 / 0.05
    assert worst <= 4 * tr.D_N                      # the recorded figure still describes it
    assert (states[:, :, tr.FITTED] == 1).all()
    # the fit finds the plane the feet stand on, to the z noise over the footprint
    err = np.abs(states[-1][:, tr.N] - traj[0]["n_true"]).max()
    print(f"normal against the generator's plane after 120 ticks: {err:.2e}")
    assert err < 0.1


def test_each_output_absent_in_turn(robot, oracle):
    traj, states, outs = oracle
    for skip in ("normal", "plane", "normal_base", "status"):
        st = np.vstack([np.zeros((8, tr.STRIDE)), np.full((2, tr.STRIDE), float(SENTINEL))])
        out = host_launch(robot, st, dict(pos_feet=traj[0]["pos_feet"], contact=traj[0]["contact"],
                                          quat=traj[0]["quat"]), skip=(skip,))
        assert (out[skip] == SENTINEL).all() and np.array_equal(st[:8, tr.HIST], states[0][:, tr.HIST])


def test_root_state_layout_and_robot_record(robot, oracle):
    traj, states, outs = oracle
    step = traj[0]
    rs = np.zeros((8, 13), np.float32)
    rs[:, [6, 3, 4, 5]] = step["quat"]
    rob = np.arange(10 * 16, dtype=np.float32).reshape(10, 16)
    a = host_launch(robot, np.zeros((10, tr.STRIDE)), dict(pos_feet=step["pos_feet"], contact=step["contact"],
                                                           quat=step["quat"]))
    b = host_launch(robot, np.zeros((10, tr.STRIDE)), dict(pos_feet=step["pos_feet"], contact=step["contact"],
                                                           root_states=rs, robot=rob))
    assert np.array_equal(a["normal_base"], b["normal_base"])
    assert np.array_equal(b["robot"][:8, 9:12], b["normal"][:8])
    keep = np.ones(16, bool)
    keep[9:12] = False
    assert np.array_equal(b["robot"][:, keep], rob[:, keep]) and np.array_equal(b["robot"][8:], rob[8:])


# ---- refusal

def _seeded(robot):
    feet, _ = on_plane([0.2, -0.1, 1.0], 0.3)
    return one(robot, feet)[0], np.float32(feet)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_refusals_leave_the_record_bytes_untouched(robot, bad):
    seeded, feet = _seeded(robot)
    cases = []
    f = feet.copy()
    f[2, 1] = bad
    cases.append(("cold record, bad foot (no contact: latched all the same)", np.zeros(tr.STRIDE), f, (0, 0, 0, 0)))
    cases.append(("fitted record, bad foot in contact", seeded, f, (0, 0, 1, 0)))
    for w in (0, 11, 13, 16, 17, 18, 19):
        rec = seeded.copy()
        rec[w] = bad
        cases.append((f"bad word {w}", rec, feet, (1, 1, 1, 1)))
    rec = np.zeros(tr.STRIDE)
    rec[tr.INIT] = bad
    cases.append(("bad initialised word", rec, feet, (1, 1, 1, 1)))
    for name, rec, ft, c in cases:
        st, out = one(robot, ft, contact=c, state=rec)
        assert st.tobytes() == np.asarray(rec, np.float64).tobytes(), name
        assert out["status"] == tr.STATUS_NONFINITE, name
        want = tr.as_was(np.asarray(rec, np.float64)[None])[0]
        assert np.array_equal(out["normal"], want[tr.N].astype(np.float32), equal_nan=True), name
        assert np.array_equal(out["plane"][3], np.float32(want[tr.D]), equal_nan=True), name
        ref, o = tr.terrain_step(np.asarray(rec, np.float64)[None], dict(pos_feet=ft[None], contact=np.float32([c])))
        assert ref.tobytes() == np.asarray(rec, np.float64).tobytes() and o["status"][0] == tr.STATUS_NONFINITE, name
    # a non-finite foot that is not latched is ignored
    st, out = one(robot, f, contact=(1, 1, 0, 1), state=seeded)
    assert out["status"] == 0 and np.array_equal(st[tr.HIST].reshape(4, 3)[2], seeded[tr.HIST].reshape(4, 3)[2])
    # a cold record full of garbage but for a zero `initialised` word is a cold record
    rec = np.full(tr.STRIDE, bad)
    rec[tr.INIT] = 0.0
    st, out = one(robot, feet, state=rec)
    assert out["status"] == 0 and np.array_equal(st, seeded)


def test_a_refused_robot_does_not_touch_its_neighbours(robot, oracle):
    traj, states, outs = oracle
    step = dict(pos_feet=traj[1]["pos_feet"].copy(), contact=traj[1]["contact"])
    clean_st = np.vstack([states[0], np.zeros((2, tr.STRIDE))])
    clean = host_launch(robot, clean_st, step)
    step["pos_feet"][3] = np.nan
    st = np.vstack([states[0], np.zeros((2, tr.STRIDE))])
    out = host_launch(robot, st, step)
    others = np.arange(8) != 3
    assert out["status"][3] == tr.STATUS_NONFINITE and np.array_equal(st[3], states[0][3])
    assert np.array_equal(st[:8][others], clean_st[:8][others])
    for k in ("normal", "plane", "status"):
        assert np.array_equal(out[k][:8][others], clean[k][:8][others])


# ---- the contact rules

def test_both_contact_rules(robot):
    seeded, feet = _seeded(robot)
    moved = feet + np.float32([0.5, 0.25, 0.125])
    f32 = np.float32
    below, above = np.nextafter(f32(0.5), f32(0)), np.nextafter(f32(0.5), f32(1))
    # value, in contact under `contact` (threshold 0.5), in contact under `swing_state`
    table = [(np.nan, False, True), (-0.0, False, True), (0.0, False, True), (0.5, False, False),
             (below, False, False), (above, True, False), (1.0, True, False), (-1.0, False, True),
             (np.inf, True, False), (-np.inf, False, True), (1e-45, False, False)]
    for v, by_contact, by_swing in table:
        for rule, want in (("contact", by_contact), ("swing_state", by_swing)):
            st = np.vstack([seeded, np.full((2, tr.STRIDE), float(SENTINEL))])
            host_launch(robot, st, {"pos_feet": moved[None], rule: np.float32([[v, v, v, v]])})
            latched = np.array_equal(st[0, tr.HIST], moved.astype(np.float64).reshape(12))
            kept = np.array_equal(st[0, tr.HIST], seeded[tr.HIST])
            assert latched == want and kept == (not want), (v, rule)
            assert bool(tr.contact_decision(np.float32([[v]]), None, rule == "swing_state")[0, 0]) == want
    # a threshold of its own: exactly at it is no contact
    st = np.vstack([seeded, np.full((2, tr.STRIDE), float(SENTINEL))])
    host_launch(robot, st, dict(pos_feet=moved[None], contact=np.float32([[2.0, 2.5, 1.0, 3.0]])),
                dict(contact_threshold=2.0))
    h, h0, m = st[0, tr.HIST].reshape(4, 3), seeded[tr.HIST].reshape(4, 3), moved.astype(np.float64)
    assert np.array_equal(h[[0, 2]], h0[[0, 2]]) and np.array_equal(h[[1, 3]], m[[1, 3]])


# ---- the reference's recorded run

def test_reference_recorded_run(robot):
    """tests/golden/terrain.npz: 30 ticks of 4 robots through the reference's own
    update_terrain_normal.  From the first tick by which every foot has been latched once (before
    it the reference still holds its zeros) our history is the reference's bitwise.  The
    deviation, both ways: our normal is numpy.linalg.eigh's column on that history; the
    reference's recorded vector, a row of its eigenvector matrix, is not."""
    fx = np.load(GOLDEN)
    feet, contact, ref_hist, ref_n = fx["pos_feet"], fx["contact"], fx["history"], fx["terrain_normal_est"]
    T, B = contact.shape[:2]
    assert (T, B) == (30, 4)
    seen = np.cumsum(contact == 1, axis=0) > 0                 # [T,B,4]
    start = int(np.argmax(seen.all(axis=(1, 2))))
    assert seen.all(axis=(1, 2)).any() and 0 < start < T - 5
    st = np.vstack([np.zeros((B, tr.STRIDE)), np.full((2, tr.STRIDE), float(SENTINEL))])
    ours, differs = 0.0, 0.0
    for t in range(T):
        host_launch(robot, st, dict(pos_feet=feet[t], contact=contact[t]))
        if t < start:
            continue
        assert np.array_equal(st[:B, tr.HIST].reshape(B, 4, 3), ref_hist[t].astype(np.float64)), t
        _, _, col = tr.fit(ref_hist[t].astype(np.float64))
        ours = max(ours, np.abs(st[:B, tr.N] - col).max())
        differs = max(differs, np.abs(ref_n[t] - col).max())
        assert (st[:B, tr.FITTED] == 1).all()
    print(f"\nours against eigh's column {ours:.2e}; the reference's row against it {differs:.2e}")
    assert ours < 1e-12 and differs > 1e-3


# ---- the edges, shared with tests/test_gpu_terrain_edges.py (tests/terrain_edge_checks.py)

@pytest.fixture(scope="module")
def launch(robot):
    def run(state, inp, constants=None, ground=False):
        B = len(state)
        st = np.vstack([np.asarray(state, np.float64), np.full((2, tr.STRIDE), float(SENTINEL))])
        out = host_launch(robot, st, inp, constants, ground=ground)
        assert (st[B:] == SENTINEL).all() and all((v[B:] == SENTINEL).all() for k, v in out.items() if k != "robot")
        return st[:B].copy(), {k: v[:B] for k, v in out.items()}
    return run


@pytest.fixture(scope="module")
def gpu_traj():
    return tr.make_trajectory(**tr.GPU_TRAJECTORY)


def test_cases_are_what_they_claim(gpu_traj):
    """Every edge case on terrain_ref alone: the decision it is meant to take, and its distance
    from the threshold -- a factor 2 and more for a spread and for the length of a blend, 0.02 rad
    for a tilt (n_z 1.7e-2 off cos_max_tilt, 1e5 float32 roundings), or an exact zero."""
    flat, cmt = tr.DEFAULTS["flat_tol"], tr.DEFAULTS["cos_max_tilt"]
    rows = {name: (fitted, spread, nz, l2) for name, fitted, spread, nz, l2 in edge.describe_held()}
    for name in edge.HELD:
        assert not rows[name][0], name
    for name in edge.ACCEPTED:
        assert rows[name][0], name
    assert rows["coincident"][3] == 0.0 and rows["collinear"][1] < 1e-12 and rows["collinear"][3] > 0.1
    assert abs(rows["spread flat_tol / 2"][1] / (flat / 2) - 1) < 1e-3 and abs(rows["spread 2 flat_tol"][1] / (2 * flat) - 1) < 1e-3
    for name in ("spread flat_tol / 2", "spread 2 flat_tol"):
        assert rows[name][2] > cmt + 0.1                       # the tilt does not decide these
    assert abs(rows["tilt 0.02 rad past the limit"][2] - np.cos(edge.ACOS_HALF + 0.02)) < 1e-6
    assert abs(rows["tilt 0.02 rad inside the limit"][2] - np.cos(edge.ACOS_HALF - 0.02)) < 1e-6
    for name in ("tilt 0.02 rad past the limit", "tilt 0.02 rad inside the limit"):
        assert abs(rows[name][2] - cmt) > 1.7e-2 and rows[name][1] > 0.1
    assert abs(rows["vertical plane"][2]) < 1e-12 and rows["vertical plane"][1] > 0.1
    # the seeded normals at blend = 0.5: the blend's length is exactly 0, and 1.5 / 1.45
    recs, feet = edge.seeded_n_records()
    _, _, nf = tr.fit(feet.astype(np.float64)[None])
    assert nf[0].tolist() == [0.0, 0.0, 1.0]
    ln = np.linalg.norm(0.5 * recs[:, tr.N] + 0.5 * nf, axis=1)
    assert ln[0] == 0.0 and ln[1] == 1.5 and 1.4 < ln[2] < 1.5
    # the thin footprints: accepted, spread a factor 2 and more over flat_tol
    thin = edge.thin_feet()
    sp = tr.spread(thin.astype(np.float64))
    st, ok = tr.tick_step(np.zeros((len(thin), tr.STRIDE)), thin, np.ones((len(thin), 4), bool))
    assert ok.all() and (st[:, tr.FITTED] == 1).all() and sp.min() >= 2 * flat * (1 - 1e-4) and sp.max() <= 0.05 * (1 + 1e-4)
    # the bad records: refused but for the cold one
    rows_, rec = edge.bad_records()
    moved = np.tile(edge.rectangle(0.2, 0.13, 0.25, -1.0, (1.5, -1.75, 0.525)), (len(rows_), 1, 1))
    with np.errstate(invalid="ignore"):
        _, ok = tr.tick_step(rows_, moved, np.ones((len(rows_), 4), bool))
    assert ok.tolist() == [False] * 18 + [True] and len(rows_) == 19
    # far from the origin: the larger coordinate is 7e3 .. 1e4 and 7e4 .. 1e5 m, where float32
    # positions are 2^-11 or 2^-10 (5e-4, 1e-3 m) and 2^-7 (8e-3 m) apart
    far = edge.far_feet()
    gap = np.round(np.log2(np.spacing(np.abs(far).max(axis=(1, 2))))).astype(int)
    assert set(gap[0::2]) <= {-11, -10} and set(gap[1::2]) == {-7}
    # the blend trajectory: spread 0.05 and more, asserted by the generator itself
    assert len(gpu_traj) >= 10 and gpu_traj[0]["pos_feet"].shape[0] >= edge.B_EDGE


def test_edge_held_fits(launch):
    print(f"\nheld fits: d and accepted n against the restatement {edge.check_held_fits(launch):.2e} of the bound")


def test_edge_blend_and_seeded_normals(launch, gpu_traj):
    print(f"\nblend 0.25 / 0.5 over 10 ticks: {edge.check_blend(launch, gpu_traj):.2e} (bound {edge.N_BOUND:.1e})")
    edge.check_seeded_normals(launch)


def test_edge_exact_structure_and_scaling(launch):
    w = edge.check_exact_structure(launch)
    rows = edge.check_scaling(launch)
    print(f"\nexact structure {w:.2e} of the bound; {rows} scaled rows bitwise")


def test_edge_thin_footprints(launch):
    err = edge.check_thin_footprints(launch)
    print("\nthin footprints, spread: error (bound)  " + "  ".join(
        f"{s}: {e:.2e} ({edge.N_BOUND * max(1, 0.05 / s):.1e})" for s, e in err.items()))


def test_edge_odd_inputs_and_bad_records(launch):
    edge.check_odd_inputs(launch)
    print(f"\nrefused records: {edge.check_bad_records(launch)}")


def test_edge_far_from_the_origin(launch):
    worst, fitted = edge.check_far_from_the_origin(launch)
    print(f"\n1e4 / 1e5 m from the origin: {worst:.2e} (bound {edge.N_BOUND:.1e}); share fitted per tick {fitted}")


def test_edge_ground_flag(launch, gpu_traj):
    print(f"\nground flag: plane word against d - n_z touchdown_z {edge.check_ground_flag(launch, gpu_traj):.2e}")


# ---- the swing leg on the plane

def _leg_inputs(seed):
    rng = np.random.default_rng(seed)
    R = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    v = np.concatenate([[0.1, 0.1, 0.001, 0.0], rng.uniform(-1, 1, 3) + [0, 0, 0.4], rng.uniform(-1, 1, 3),
                        R.reshape(9), rng.uniform(-0.5, 0.5, 3), [0.3], rng.uniform(-0.2, 0.2, 3),
                        rng.uniform(-0.3, 0.3, 3), [9.81, 0.03, -0.0255, 0.1]])
    assert v.size == 33
    return v


def _leg_run(lib, which, ground, ticks=6, seed=0):
    mem = np.zeros(8)
    out = []
    g = None if ground is None else np.ascontiguousarray(ground, np.float64)
    for t in range(ticks):
        inp = _leg_inputs(seed)
        inp[3] = float(t == ticks - 1)
        pb, vb = np.zeros(3), np.zeros(3)
        lib.leg_step(which, _p(mem), _p(inp), _p(g), _p(pb), _p(vb))
        out.append(np.concatenate([mem, pb, vb]))
    return np.stack(out)


def test_swing_leg_step_ground_without_a_plane_is_swing_leg_step(robot):
    flat = _leg_run(robot, 0, None)
    assert np.isfinite(flat).all() and (flat[:-1, 0] == 1).all() and flat[-1, 0] == 0
    assert _leg_run(robot, 1, None).tobytes() == flat.tobytes()
    assert _leg_run(robot, 1, [0.0, 0.0, 1.0, 0.0]).tobytes() == flat.tobytes()
    for none in ([np.nan, 0, 1, 0], [0, 0, 1, np.inf], [0, 0, 0, 0], [0.1, 0, -1, 0]):
        assert _leg_run(robot, 1, none).tobytes() == flat.tobytes(), none


def test_swing_leg_step_ground_on_a_plane(robot):
    g = np.array([0.19, -0.1, 0.97, 0.4])
    got = _leg_run(robot, 1, g)
    flat = _leg_run(robot, 0, None)
    ground = lambda p: (g[3] - g[0] * p[0] - g[1] * p[1]) / g[2]
    for t in range(6):
        init, fin = got[t, 2:5], got[t, 5:8]
        assert np.array_equal(fin[:2], flat[t, 5:7]) and np.array_equal(init, flat[t, 2:5])
        assert abs(fin[2] - (-0.0255 + ground(fin))) < KNOWN
        # the curve through the apex: GroundSwingRef's, evaluated for this leg
        ref = tr.GroundSwingRef(1, ground=g[None])
        apex = 0.1 + (ground(init) + ground(fin)) / 2
        p, v = tr.swing_ref.curve(np.array([0.1]), np.array([0.1 - got[t, 1]]), init[None], fin[None], apex)
        inp = _leg_inputs(0)
        Rm, pos, vel = inp[10:19].reshape(3, 3), inp[4:7], inp[7:10]
        assert np.abs(Rm.T @ (p[0] - pos) - got[t, 8:11]).max() < KNOWN
        assert np.abs(Rm.T @ (v[0] - vel) - got[t, 11:14]).max() < 1e-10
        assert ref.on.all()
    assert not np.array_equal(got[:, 8:11], flat[:, 8:11])

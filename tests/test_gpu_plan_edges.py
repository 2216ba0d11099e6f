"""GPU: mpcqp_plan / mpcqp_plan_root_states and mpcqp_stance_torques at the edges -- batch tails
around the 64 robots a workgroup owns, sentinel rows behind every buffer, the caller's R_base,
a command with vz != 0, the planner constants, the clamp and compensation thresholds, large
attitudes, the shortest and the longest horizon, malformed gait records, outputs that must stay
unwritten, non-finite input and every MPCQP_ERR_ARG branch -- against oracle/planner.py robot by
robot, hand-written expectations, and the reference's own recording at the same edges
(tests/golden/planner_edges.npz, which tests/test_oracle.py holds the oracle to).

Bounds: those tests/test_gpu_plan.py holds against the oracle -- x0 rtol 2.4e-7 (two float32
ulps), X_ref 2e-6 absolute, the gait table exact, the planner record 1e-7 absolute -- with
|position| <= 2 m, |velocity| <= 2 m/s and |yaw| <= 4 rad as there.  Against the recording:
X_ref 1e-6 and the record 3e-7, as test_plan_matches_reference_sequence.  The Euler angles of
test_euler_edges_known_answers are held to 2 float32 ulps of the reference's own formula
(kinematics.py:46-48) evaluated on the float32 quaternion.  Stance torques: rtol 1e-5, atol 1e-3
against the oracle (tests/test_gpu_plan.py), bitwise against mpcqp_leg_torques.

Measured on the MI355X (worst over all cases of each test): test_parity (B = 1 .. 131, three
layouts) and test_horizon_edges (N = 1, 2, 32) x0 0, xref 0, record 4.4e-16;
planner_edges.npz x0 0, xref 6.0e-08, record 2.4e-08 (the oracle's own distance from the
recording); test_planner_constants 0 / 0 / 0, and 7.0e-02 from the default-constant oracle;
clamp, thresholds and saturation 0 / 0 / 0 against the oracle and against the hand-written
expectations; Euler edges 0.40 float32 ulps from the reference's formula (3.6e-05 rad from
the angles the quaternions were built from, the float32 rounding of asin's argument at
pitch = pi/2 - 1e-3); stance torques 3.1e-05 absolute from the oracle,
bitwise mpcqp_leg_torques.  Before the pitch clamp was written with comparisons a NaN
quaternion packed (nan, -1.5707964, nan); before mpcqp_set_planner checked, it accepted
dt_control = inf.
"""
import ctypes
import math
import os

import numpy as np
import pytest

# torch first: it brings its own HIP runtime, which must be loaded before libmpcqp.so
# pulls in the system's (a CPU test file collected ahead of this one loads the library)
torch = pytest.importorskip("torch")

from oracle.planner import GAITS, PlannerOracle, gait_table, quat2matrix, quat2zyx, world_velocity  # noqa: E402
from oracle.planner import stance_torques as oracle_stance_torques  # noqa: E402
from helpers import DEV, _dev  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SENTINEL = -77.0
PAD = 3
X0_RTOL, XREF_ATOL, STATE_ATOL = 2.4e-7, 2e-6, 1e-7
W = 64                     # kPlanRobots: robots per workgroup (csrc/mpcqp_plan.h)
BMAX = 2 * W + 3
T_PARITY, IBM = 41, 20
X, Y, YAW, ROLL, PITCH, STARTED = range(6)     # the planner record (include/mpcqp.h)
f32, f64 = np.float32, np.float64


def new_engine(N=10):
    from mpcqp import LinearMpc
    return LinearMpc(horizon=N, robot="aliengo", device=DEV)


@pytest.fixture(scope="module")
def eng():
    return new_engine()


def flags(reference=False, no_integrate=False):
    from mpcqp._lib import PLAN_NO_INTEGRATE, PLAN_REFERENCE
    return (PLAN_REFERENCE if reference else 0) | (PLAN_NO_INTEGRATE if no_integrate else 0)


def euler_quat(r, p, y):
    """(w, x, y, z) of the ZYX Euler angles, float64."""
    r, p, y = np.broadcast_arrays(np.asarray(r, f64), np.asarray(p, f64), np.asarray(y, f64))
    cr, sr, cp, sp, cy, sy = np.cos(r / 2), np.sin(r / 2), np.cos(p / 2), np.sin(p / 2), np.cos(y / 2), np.sin(y / 2)
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy,
                     cr * cp * sy - sr * sp * cy], -1)


def root_rows(quat, pos, omega, vel):
    """Isaac Gym actor root states [..., 13]: pos, quat (x, y, z, w), lin_vel, ang_vel."""
    return np.concatenate([pos, quat[..., 1:4], quat[..., 0:1], vel, omega], -1).astype(f32)


class Device:
    """The caller's buffers for B robots of one engine, each with `pad` extra rows of SENTINEL;
    the output rows start as SENTINEL too, so an unwritten output shows.  run() is one plan call."""

    def __init__(self, eng, B, N, gait=None, height=0.38, state=None, pad=PAD):
        self.eng, self.B, self.N = eng, B, N
        f = dict(dtype=torch.float32, device=DEV)
        self.state = torch.full((B + pad, 8), SENTINEL, dtype=torch.float64, device=DEV)
        self.state[:B] = 0.0 if state is None else _dev(state)
        self.x0 = torch.full((B + pad, 13), SENTINEL, **f)
        self.xref = torch.full((B + pad, N, 13), SENTINEL, **f)
        self.contact = torch.full((B + pad, N, 4), SENTINEL, **f)
        self.height = _dev(np.array(np.broadcast_to(np.asarray(height, f32), (B,))))
        self.gait = _dev(np.asarray(gait, np.int32)) if gait is not None else None
        self.iteration = torch.zeros((B,), dtype=torch.int32, device=DEV)

    def run(self, fl, vb, yr, iteration=None, use_gait=True, **inputs):
        """inputs: quat, pos, omega, vel[, rot] or root_states (device tensors or arrays)."""
        B = self.B
        if iteration is not None:
            self.iteration.copy_(torch.as_tensor(np.asarray(iteration, np.int32)))
        inputs = {k: (v if torch.is_tensor(v) else _dev(np.asarray(v, f32))) for k, v in inputs.items()}
        vb = vb if torch.is_tensor(vb) else _dev(np.asarray(vb, f64))
        yr = yr if torch.is_tensor(yr) else _dev(np.asarray(yr, f64))
        g = self.gait if use_gait else None
        self.eng.plan(fl, self.state[:B], self.x0[:B], vb, yr, gait=g, iteration=self.iteration if g is not None else None,
                      height_des=self.height, xref=self.xref[:B], contact=self.contact[:B], **inputs)

    def read(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in ("state", "x0", "xref", "contact")}

    def padding_untouched(self):
        return all((v[self.B:] == SENTINEL).all() for v in self.read().values())


def layout_inputs(layout, quat, pos, omega, vel, rot=None):
    if layout == "root":
        return dict(root_states=root_rows(quat, pos, omega, vel))
    kw = dict(quat=quat, pos=pos, omega=omega, vel=vel)
    if layout == "rot":
        kw["rot"] = rot
    return kw


def make_inputs(B, T, seed):
    """T ticks of B robots at the planner's edges: |roll|, |pitch| up to 1.2 rad, every other
    robot's quaternion negated (w < 0), a yaw sweeping past +-pi, a drifting base that drives
    the clamp, a command per robot with vz != 0, a height per robot, every gait, and a second
    R_base unrelated to the quaternion (not even a rotation)."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None]
    amp = rng.uniform(-1.2, 1.2, (B, 2))
    amp[0] = [1.2, -1.2]
    yaw0, yawd = rng.uniform(-3.1, 3.1, B), rng.choice([-0.02, 0.02], B)
    yaw0[0], yawd[0] = 3.1, 0.02                                  # robot 0 crosses +pi at once
    q = euler_quat(amp[:, 0] * (0.9 + 0.1 * np.cos(0.3 * t)), amp[:, 1] * (0.9 + 0.1 * np.cos(0.2 * t)), yaw0 + yawd * t)
    q[:, 1::2] *= -1.0
    p0 = np.concatenate([rng.uniform(-1, 1, (B, 2)), rng.uniform(0.25, 0.45, (B, 1))], 1)
    pos = p0[None] + rng.uniform(-0.01, 0.01, (B, 3))[None] * t[..., None]
    sign = rng.choice([-1.0, 1.0], B)
    names = list(GAITS)
    gsel = [names[b % len(names)] for b in range(B)]
    return dict(quat=q.astype(f32), pos=pos.astype(f32), omega=rng.uniform(-1, 1, (T, B, 3)).astype(f32),
                vel=rng.uniform(-1.5, 1.5, (T, B, 3)).astype(f32),
                vb=np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.5, 0.5, B), sign * rng.uniform(0.2, 0.5, B)], 1),
                yr=rng.uniform(-1, 1, B), height=rng.uniform(0.25, 0.45, B).astype(f32),
                rot=rng.uniform(-1, 1, (B, 3, 3)).astype(f32), names=gsel,
                gait=np.array([[GAITS[n][0], *GAITS[n][1], *GAITS[n][2]] for n in gsel], np.int32))


def oracle_trace(inp, B, T, N, ibm, rot=None, **constants):
    """oracle/planner.py robot by robot over T ticks: x0 [T,B,13], state [T,B,8], and per MPC
    tick xref [K,B,N,13] and contact [K,B,N,4].  rot [B,3,3] replaces quat2matrix(quat)."""
    x0, st = np.zeros((T, B, 13), f32), np.zeros((T, B, 8))
    K = (T + ibm - 1) // ibm
    xref, contact = np.zeros((K, B, N, 13), f32), np.zeros((K, B, N, 4), f32)
    for b in range(B):
        o = PlannerOracle(N, inp["height"][b], **constants)
        period, off, dur = (int(inp["gait"][b, 0]), inp["gait"][b, 1:5], inp["gait"][b, 5:9])
        for t in range(T):
            x0[t, b] = o.update_robot_state(inp["quat"][t, b], inp["pos"][t, b], inp["omega"][t, b], inp["vel"][t, b])
            v = world_velocity(rot[b] if rot is not None else quat2matrix(inp["quat"][t, b]), inp["vb"][b])
            o.integrate(v, inp["yr"][b])
            if t % ibm == 0:
                xref[t // ibm, b] = o.reference_trajectory(v, inp["yr"][b])
                contact[t // ibm, b] = gait_table(period, off, dur, (t // ibm) % period, N)
            st[t, b] = o.state_record()
    return dict(x0=x0, state=st, xref=xref, contact=contact)


def rel_x0(got, want):
    """The worst |got - want| / |want| of assert_allclose(rtol, atol=0); a zero is met exactly."""
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    nz = want != 0
    assert np.array_equal(got[~nz], want[~nz])
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0


def follow(eng, inp, ora, B, T, N, ibm, layout="split", rot=None):
    """T ticks on the device against the oracle's trace after every one; the worst figures."""
    d = Device(eng, B, N, gait=inp["gait"][:B], height=inp["height"][:B])
    up = {k: _dev(inp[k][:, :B]) for k in ("quat", "pos", "omega", "vel")}
    rs = _dev(root_rows(inp["quat"][:, :B], inp["pos"][:, :B], inp["omega"][:, :B], inp["vel"][:, :B]))
    vb, yr = _dev(inp["vb"][:B]), _dev(inp["yr"][:B])
    rot_d = _dev(rot[:B]) if rot is not None else None
    worst = dict(x0=0.0, xref=0.0, state=0.0)
    for t in range(T):
        tick = t % ibm == 0
        kw = dict(root_states=rs[t]) if layout == "root" else {k: v[t] for k, v in up.items()}
        if layout == "rot":
            kw["rot"] = rot_d
        d.run(flags(reference=tick), vb, yr, iteration=(t // ibm) % inp["gait"][:B, 0], **kw)
        o = d.read()
        worst["x0"] = max(worst["x0"], rel_x0(o["x0"][:B], ora["x0"][t, :B]))
        worst["state"] = max(worst["state"], float(np.abs(o["state"][:B, :5] - ora["state"][t, :B, :5]).max()))
        assert np.array_equal(o["state"][:B, 5:], ora["state"][t, :B, 5:]), t
        if tick:
            k = t // ibm
            worst["xref"] = max(worst["xref"], float(np.abs(o["xref"][:B].astype(f64) - ora["xref"][k, :B]).max()))
            assert np.array_equal(o["contact"][:B], ora["contact"][k, :B]), t
        assert d.padding_untouched(), t
    return worst


def check(worst, tag):
    print(f"\n{tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["x0"] <= X0_RTOL and worst["xref"] <= XREF_ATOL and worst["state"] <= STATE_ATOL, (tag, worst)


@pytest.fixture(scope="module")
def parity():
    """The inputs of test_parity for BMAX robots and the oracle's trace of them, once with
    quat2matrix(quat) and once with the unrelated R_base: robots are independent, so the first
    B robots are the oracle of a batch of B."""
    inp = make_inputs(BMAX, T_PARITY, seed=11)
    rpy = np.array([[quat2zyx(inp["quat"][t, b]) for b in range(BMAX)] for t in range(T_PARITY)])
    assert np.abs(rpy[..., :2]).max() > 1.19 and (inp["quat"][..., 0] < 0).any() and (inp["vb"][:, 2] != 0).all()
    assert (np.abs(np.diff(rpy[:, 0, 2])) > 6.0).any()            # robot 0's yaw wraps (B = 1 too)
    assert np.abs(inp["pos"]).max() <= 2 and np.abs(inp["vel"]).max() <= 2
    return inp, oracle_trace(inp, BMAX, T_PARITY, 10, IBM), oracle_trace(inp, BMAX, T_PARITY, 10, IBM, rot=inp["rot"])


@pytest.mark.parametrize("layout", ["split", "root", "rot"])
@pytest.mark.parametrize("B", [1, W - 1, W, W + 1, BMAX])
def test_parity(eng, parity, B, layout):
    """B = 63, 64, 65 around one workgroup, 131 a third workgroup with a tail of three; both
    input layouts, and the split one with a caller's R_base that is not quat2matrix(quat): it
    turns the command (vz != 0, so its third column too), the Euler angles stay the
    quaternion's.  41 control iterations, three MPC ticks, N = 10."""
    inp, ora, ora_rot = parity
    rot = inp["rot"] if layout == "rot" else None
    check(follow(eng, inp, ora_rot if layout == "rot" else ora, B, T_PARITY, 10, IBM, layout, rot), f"B={B} {layout}")
    if layout == "rot":
        assert np.abs(ora_rot["xref"][:, :B, :, 9:11] - ora["xref"][:, :B, :, 9:11]).max() > 1e4 * XREF_ATOL


@pytest.mark.parametrize("N", [1, 2, 32])
def test_horizon_edges(N):
    """The shortest horizons and MPCQP_MAX_HORIZON (the length of the kernel's per-robot LDS
    sequence), B = 65, two MPC ticks; at N = 32 the gait tables of every member also equal the
    reference's own (gait_N32.npz)."""
    from mpcqp.params import GAIT_MEMBERS
    B, T = W + 1, IBM + 1
    inp = make_inputs(B, T, seed=100 + N)
    ora = oracle_trace(inp, B, T, N, IBM)
    check(follow(new_engine(N), inp, ora, B, T, N, IBM, "root"), f"N={N}")
    if N == 32:
        z = np.load(os.path.join(GOLDEN, "gait_N32.npz"), allow_pickle=False)
        for member in z.files:
            b = inp["names"].index(GAIT_MEMBERS[member])
            for k in range(2):
                assert np.array_equal(ora["contact"][k, b].reshape(-1), z[member][k]), member
        assert len(z.files) == 6


def test_device_matches_reference_at_the_edges(eng):
    """The reference's own recording at large attitudes, w < 0, vz != 0 and every clamp branch
    (planner_edges.npz, B = 8, N = 10) on the device, to the bounds test_gpu_plan.py holds
    against planner.npz."""
    z = np.load(os.path.join(GOLDEN, "planner_edges.npz"), allow_pickle=False)
    B, T = z["quat"].shape[:2]
    N, ibm = int(z["horizon"]), int(z["iterations_between_mpc"])
    worst = dict(x0=0.0, xref=0.0, state=0.0)
    for layout in ("split", "root"):
        d = Device(eng, B, N, gait=z["gait"], height=float(z["height"]))
        for t in range(T):
            tick = t % ibm == 0
            d.run(flags(reference=tick), z["v_body"], z["yaw_rate"], iteration=(t // ibm) % z["gait"][:, 0],
                  **layout_inputs(layout, z["quat"][:, t], z["pos"][:, t], z["omega"][:, t], z["vel"][:, t]))
            o = d.read()
            worst["x0"] = max(worst["x0"], rel_x0(o["x0"][:B], z["x0"][:, t]))
            if tick:
                k = t // ibm
                worst["xref"] = max(worst["xref"], float(np.abs(o["xref"][:B].reshape(B, -1).astype(f64) - z["xref"][:, k]).max()))
                worst["state"] = max(worst["state"], float(np.abs(o["state"][:B, :5] - z["plan_state"][:, k]).max()))
                assert np.array_equal(o["contact"][:B].reshape(B, -1), z["table"][:, k]), t
        assert d.padding_untouched()
    print("\nplanner_edges.npz: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["x0"] <= X0_RTOL and worst["xref"] <= 1e-6 and worst["state"] <= 3e-7, worst


def test_planner_constants():
    """set_planner(dt_control, gravity, max_pos_error) with none at its default, B = 3: parity
    with an oracle built with the same three numbers, far from the default-constant oracle, the
    gravity entry exact, the clamp engaging at 0.03; a refused call (non-finite or negative)
    names the planner and leaves the three as they were."""
    from mpcqp import _lib
    mine = dict(dt_control=0.002, gravity=9.0, max_pos_error=0.03)
    eng = new_engine()
    eng.set_planner(**mine)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(dt_control=inf), dict(dt_control=nan), dict(gravity=nan), dict(gravity=inf), dict(gravity=-inf),
                dict(max_pos_error=nan), dict(max_pos_error=inf), dict(dt_control=-0.001), dict(max_pos_error=-0.1)):
        a = dict(mine, **bad)
        assert eng.lib.mpcqp_set_planner(eng._ctx, a["dt_control"], a["gravity"], a["max_pos_error"]) == _lib.ERR_ARG, bad
        assert "planner" in eng.lib.mpcqp_last_error(eng._ctx).decode(), bad
        with pytest.raises(_lib.MpcqpError, match="planner"):
            eng.set_planner(**a)
    other = new_engine()                                          # accepted: zeros and a negative gravity
    assert other.lib.mpcqp_set_planner(other._ctx, 0.0, -3.5, 0.0) == 0

    B, N, T = 3, 10, IBM + 1
    inp = make_inputs(B, T, seed=5)
    # robot 0 stays within 0.03 of its desired track, robot 1 sits 0.05 off in x (clamped at 0.03
    # but not at 0.1), robot 2 0.2 off in y (clamped either way)
    # a level base, so the command is the world velocity: robot 1 moves further off in x and
    # robot 2 in y, and both clamp again on the second MPC tick
    inp["quat"][:] = f32([1, 0, 0, 0])
    inp["pos"][:, :, :2] = 0.0
    inp["pos"][:, 1, 0], inp["pos"][:, 2, 1] = 0.05, -0.2
    inp["vb"][:, :2] = [[0.5, 0.2], [-0.4, -0.3], [-0.6, 0.1]]
    ora, dflt = oracle_trace(inp, B, T, N, IBM, **mine), oracle_trace(inp, B, T, N, IBM)
    d = Device(eng, B, N, gait=inp["gait"], height=inp["height"])
    worst = dict(x0=0.0, xref=0.0, state=0.0)
    apart = dict(xref=0.0, state=0.0)
    for t in range(T):
        tick = t % IBM == 0
        d.run(flags(reference=tick), inp["vb"], inp["yr"], iteration=(t // IBM) % inp["gait"][:, 0],
              **layout_inputs("split", *(inp[k][t] for k in ("quat", "pos", "omega", "vel"))))
        o = d.read()
        worst["x0"] = max(worst["x0"], rel_x0(o["x0"][:B], ora["x0"][t]))
        worst["state"] = max(worst["state"], float(np.abs(o["state"][:B, :5] - ora["state"][t, :, :5]).max()))
        apart["state"] = max(apart["state"], float(np.abs(o["state"][:B, :5] - dflt["state"][t, :, :5]).max()))
        assert (o["x0"][:B, 12] == f32(-9.0)).all()
        if tick:
            k = t // IBM
            worst["xref"] = max(worst["xref"], float(np.abs(o["xref"][:B].astype(f64) - ora["xref"][k]).max()))
            apart["xref"] = max(apart["xref"], float(np.abs(o["xref"][:B, :, :12].astype(f64) - dflt["xref"][k][:, :, :12]).max()))
            assert (o["xref"][:B, :, 12] == f32(-9.0)).all()
            # the clamp at 0.03, by hand: robot 1's x_des is px - 0.03, robot 2's y_des py + 0.03
            px, py = f64(inp["pos"][t, 1, 0]), f64(inp["pos"][t, 2, 1])
            assert o["state"][1, X] == px - 0.03 and o["state"][2, Y] == py + 0.03
            assert abs(o["state"][0, X] - f64(inp["pos"][t, 0, 0])) < 0.03
    check(worst, f"set_planner {mine}")
    print(f"against the default constants: xref {apart['xref']:.2e}, state {apart['state']:.2e}")
    # dt_control doubles robot 0's integrated track (about 0.02 m after 20 ticks at 0.5 m/s), the
    # clamp moves robot 1's x_des by 0.05: the constants do matter here
    assert apart["xref"] > 1e3 * XREF_ATOL and apart["state"] > 1e4 * STATE_ATOL
    assert abs(o["state"][0, X] - 2 * dflt["state"][T - 1, 0, X]) < 1e-3 and abs(dflt["state"][T - 1, 0, X]) > 5e-3
    assert d.padding_untouched()


def _seeded_oracle(N, height, rec, quat, pos, omega, vel):
    """A PlannerOracle standing where the record `rec` stands."""
    o = PlannerOracle(N, height)
    o.first = rec[STARTED] == 0
    o.xpos_des, o.ypos_des, o.yaw_des, o.roll_init, o.pitch_init = (float(v) for v in rec[:5])
    o.update_robot_state(quat, pos, omega, vel)
    return o


def test_clamp_and_compensation_edges(eng):
    """B = 8, REFERENCE | NO_INTEGRATE on prepared records, each row against a hand-written
    expectation and against the oracle.  The four clamp branches (mpc.py:129-137) and robots
    exactly at the boundary, x_des - px == e in float64, which must not clamp (the record is
    one float64 ulp away from px + e, so a clamp would show).  vel = float32(0.2) is 0.2000000030
    in float64, above the 0.2 threshold (mpc.py:143, NumPy 1.24 promotion): it compensates, the
    next float32 below does not; the same at float32(0.1) for vy, and for negative velocities."""
    B, N, e = 8, 10, 0.1
    below = lambda v: np.nextafter(f32(v), f32(0))
    edge = float(np.nextafter(0.1 - 0.0625, 1.0))
    assert edge - (-0.0625) == e and edge != -0.0625 + e and 0.0625 - (-edge) == e and -edge != 0.0625 - e
    px = f32([0.5, -0.5, 0.3, 0.3, -0.0625, 0.2, 0.0625, 1.0])
    py = f32([0.1, 0.1, 0.7, -0.7, 0.0, -0.0625, 0.0, -1.0])
    xd = np.array([0.65, -0.65, 0.32, 0.28, edge, 0.25, -edge, 0.0])
    yd = np.array([0.12, 0.12, 0.85, -0.85, 0.0, edge, 0.0, 0.0])
    want_x = np.array([f64(px[0]) + e, f64(px[1]) - e, 0.32, 0.28, edge, 0.25, -edge, f64(px[7]) - e])
    want_y = np.array([0.12, 0.12, f64(py[2]) + e, f64(py[3]) - e, 0.0, edge, 0.0, f64(py[7]) + e])
    vx = f32([f32(0.2), below(0.2), -f32(0.2), -below(0.2), 0.05, 0.05, 0.5, -0.5])
    vy = f32([0.05, 0.05, 0.05, 0.05, f32(0.1), below(0.1), -f32(0.1), -below(0.1)])
    comp_pitch = np.array([1, 0, 1, 0, 0, 0, 1, 1], bool)
    comp_roll = np.array([0, 0, 0, 0, 1, 0, 1, 0], bool)
    assert f64(f32(0.2)) > 0.2 > f64(below(0.2)) and f64(f32(0.1)) > 0.1 > f64(below(0.1))
    q = np.tile(euler_quat(0.1, 0.1, 0.3).astype(f32), (B, 1))
    roll, pitch = (f64(f32(v)) for v in quat2zyx(q[0])[:2])
    rec = np.zeros((B, 8))
    rec[:, X], rec[:, Y], rec[:, YAW], rec[:, ROLL], rec[:, PITCH], rec[:, STARTED] = xd, yd, 0.3, 0.01, -0.02, 1.0
    want_pitch = np.where(comp_pitch, -0.02 + 0.05 * (0.0 - pitch) / f64(vx), -0.02)
    want_roll = np.where(comp_roll, 0.01 + 0.05 * (0.0 - roll) / f64(vy), 0.01)
    assert np.abs(want_pitch).max() < 0.25 and np.abs(want_roll).max() < 0.25
    pos = np.stack([px, py, np.full(B, 0.3, f32)], 1)
    vel = np.stack([vx, vy, np.zeros(B, f32)], 1)
    omega = np.zeros((B, 3), f32)
    vb, yr = np.tile([0.3, 0.1, 0.2], (B, 1)), np.full(B, 0.2)
    d = Device(eng, B, N, state=rec)
    d.run(flags(True, True), vb, yr, quat=q, pos=pos, omega=omega, vel=vel)
    o = d.read()
    st, xr = o["state"][:B], o["xref"][:B].astype(f64)
    hand = np.stack([want_x, want_y, np.full(B, 0.3), want_roll, want_pitch], 1)
    err = float(np.abs(st[:, :5] - hand).max())
    assert err <= STATE_ATOL, (st[:, :5], hand)
    for b in (4, 5, 6):                                           # at the boundary: not one ulp moved
        assert st[b, X] == want_x[b] and st[b, Y] == want_y[b], b
    assert (st[:, STARTED] == 1).all()
    exr = max(float(np.abs(xr[:, 0, 3] - f64(f32(want_x))).max()), float(np.abs(xr[:, 0, 4] - f64(f32(want_y))).max()),
              float(np.abs(xr[:, :, 0] - f64(f32(f64(vy) * want_roll))[:, None]).max()),
              float(np.abs(xr[:, :, 1] - f64(f32(f64(vx) * want_pitch))[:, None]).max()))
    assert exr <= XREF_ATOL
    worst = dict(x0=0.0, xref=0.0, state=0.0)
    for b in range(B):
        orc = _seeded_oracle(N, 0.38, rec[b], q[b], pos[b], omega[b], vel[b])
        Xo = orc.reference_trajectory(world_velocity(quat2matrix(q[b]), vb[b]), yr[b])
        worst["x0"] = max(worst["x0"], rel_x0(o["x0"][b], orc.current_state))
        worst["xref"] = max(worst["xref"], float(np.abs(xr[b] - Xo).max()))
        worst["state"] = max(worst["state"], float(np.abs(st[b, :5] - orc.state_record()[:5]).max()))
    check(worst, "clamp and thresholds vs oracle")
    print(f"clamp and thresholds by hand: record {err:.2e}, xref {exr:.2e}")
    assert d.padding_untouched()

    # ---- the +-0.25 saturation (mpc.py:149-150): a constant 0.3 rad at 0.25 m/s adds -+0.06 a tick
    ang = 0.3
    rp = [(0, ang), (0, -ang), (0, ang), (-ang, 0), (ang, 0), (ang, 0), (0.01, 0.01), (0, 0)]
    q = euler_quat([a for a, _ in rp], [a for _, a in rp], 0.0).astype(f32)
    vx = f32([0.25, 0.25, -0.25, 0.05, 0.05, 0.05, 0.25, 0.25])
    vy = f32([0.05, 0.05, 0.05, 0.25, 0.25, -0.25, 0.25, 0.25])
    sat_pitch, sat_roll = {0: -0.25, 1: 0.25, 2: 0.25}, {3: 0.25, 4: -0.25, 5: 0.25}
    ang32 = np.array([[f64(f32(v)) for v in quat2zyx(q[b])[:2]] for b in range(B)])
    pos, vel = np.zeros((B, 3), f32), np.stack([vx, vy, np.zeros(B, f32)], 1)
    d = Device(eng, B, N)
    inputs = dict(quat=_dev(q), pos=_dev(pos), omega=_dev(omega), vel=_dev(vel))
    d.run(flags(), vb, yr, **inputs)                              # the first integration: started
    oracles = [PlannerOracle(N, 0.38) for _ in range(B)]
    vw = [world_velocity(quat2matrix(q[b]), vb[b]) for b in range(B)]
    for b in range(B):
        oracles[b].update_robot_state(q[b], pos[b], omega[b], vel[b])
        oracles[b].integrate(vw[b], yr[b])
    acc_r, acc_p = np.zeros(B), np.zeros(B)
    worst = dict(x0=0.0, xref=0.0, state=0.0)
    err = 0.0
    for k in range(12):
        d.run(flags(True, True), vb, yr, **inputs)
        o = d.read()
        acc_p = np.clip(acc_p + np.where(np.abs(f64(vx)) > 0.2, 0.05 * (0.0 - ang32[:, 1]) / f64(vx), 0.0), -0.25, 0.25)
        acc_r = np.clip(acc_r + np.where(np.abs(f64(vy)) > 0.1, 0.05 * (0.0 - ang32[:, 0]) / f64(vy), 0.0), -0.25, 0.25)
        err = max(err, float(np.abs(o["state"][:B, ROLL] - acc_r).max()), float(np.abs(o["state"][:B, PITCH] - acc_p).max()))
        for b in range(B):
            Xo = oracles[b].reference_trajectory(vw[b], yr[b])
            worst["xref"] = max(worst["xref"], float(np.abs(o["xref"][b].astype(f64) - Xo).max()))
            worst["state"] = max(worst["state"], float(np.abs(o["state"][b, :5] - oracles[b].state_record()[:5]).max()))
        if k >= 4:                                                # 5 x 0.06 = 0.30: saturated from the fifth tick on
            for b, s in sat_pitch.items():
                assert o["state"][b, PITCH] == s and (o["xref"][b, :, 1] == f32(f64(vx[b]) * s)).all(), (k, b)
            for b, s in sat_roll.items():
                assert o["state"][b, ROLL] == s and (o["xref"][b, :, 0] == f32(f64(vy[b]) * s)).all(), (k, b)
        else:
            assert all(abs(o["state"][b, PITCH]) < 0.25 for b in sat_pitch), k
    assert err <= STATE_ATOL and 0 < abs(o["state"][6, PITCH]) < 0.05 and o["state"][7, PITCH] == 0
    check(worst, "saturation vs oracle")
    print(f"saturation by hand: record {err:.2e}")
    assert d.padding_untouched()


def _reference_euler(q):
    """quat2ZYXangle as the reference writes it (kinematics.py:46-48), on the float32
    quaternion it is handed: NumPy float32 scalar arithmetic inside, math.atan2 / asin in
    float64 outside.  asin's argument is returned too (the reference raises past +-1)."""
    q = np.asarray(q, f32)
    phi = math.atan2(2 * (q[0] * q[1] + q[2] * q[3]), 1 - 2 * (q[1] ** 2 + q[2] ** 2))
    s = float(2 * (q[0] * q[2] - q[3] * q[1]))
    psi = math.atan2(2 * (q[0] * q[3] + q[1] * q[2]), 1 - 2 * (q[2] ** 2 + q[3] ** 2))
    return phi, (math.asin(s) if abs(s) <= 1 else None), psi, s


def test_euler_edges_known_answers(eng):
    """B = 8 quaternions built in float64 from known Euler angles and rounded to float32:
    identity, yaw-only at +-3.1 and +-pi/2, pitch-only at +-(pi/2 - 1e-3), and the last of them
    scaled by 1 + 1e-3 so that asin's argument passes 1: the clamp gives float32(pi/2) exactly.
    The whole batch negated gives the same angles bitwise.

    The allowance is 2 float32 ulps of the angle the reference's own formula gives on the same
    float32 quaternion (its products and sums are NumPy float32 scalars, as on the device; its
    atan2 / asin float64) -- not of the angle the quaternion was built from: at pitch = pi/2 -
    1e-3 one float32 rounding of asin's argument alone moves the angle by 6e-8 / cos(pitch) =
    6e-5 rad, in the reference as on the device.  The distance to the known angle is printed."""
    h = math.pi / 2
    known = np.array([[0, 0, 0], [0, 0, 3.1], [0, 0, -3.1], [0, 0, h], [0, 0, -h], [0, h - 1e-3, 0], [0, -(h - 1e-3), 0],
                      [0, h - 1e-3, 0]])
    q64 = euler_quat(known[:, 0], known[:, 1], known[:, 2])
    q64[7] *= 1 + 1e-3
    q = q64.astype(f32)
    B = len(q)
    z3, vb, yr = np.zeros((B, 3), f32), np.zeros((B, 3)), np.zeros(B)
    got = []
    for sign in (1.0, -1.0):
        d = Device(eng, B, 10)
        d.run(flags(), vb, yr, quat=f32(sign) * q, pos=z3, omega=z3, vel=z3)
        got.append(d.read()["x0"][:B, :3])
        assert d.padding_untouched()
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))
    worst, off = 0.0, 0.0
    for b in range(B):
        phi, theta, psi, s = _reference_euler(q[b])
        if b == 7:
            assert s > 1 and theta is None and got[0][b, 1] == f32(h)
            theta = h
        for k, want in enumerate((phi, theta, psi)):
            ulps = abs(f64(got[0][b, k]) - want) / float(np.spacing(f32(abs(want)))) if want != 0 else (
                0.0 if got[0][b, k] == 0 else np.inf)
            worst = max(worst, ulps)
            assert ulps <= 2, (b, k, got[0][b, k], want)
        if b != 7:                                                # past the clamp the roll is pi, not the 0 it was built from
            off = max(off, float(np.abs(f64(got[0][b]) - known[b]).max()))
    assert got[0][0].tolist() == [0, 0, 0]
    print(f"\nEuler edges: {worst:.2f} float32 ulps from the reference's formula; {off:.2e} rad from the angles the "
          "quaternions were built from")


def test_gait_record_edges(eng):
    """B = 6, N = 10.  period = 0 and period = -3 schedule no stance; iteration = -1 and -23
    give the table of the non-negative residue; an offset past the period and a duration of 0
    follow oracle.planner.gait_table (one += period, gait.py:92-93); iteration = period - 1
    wraps."""
    B, N = 6, 10
    odd = (10, (0, 20, 5, 0), (5, 5, 0, 5))
    recs = [(0, (0, 5, 5, 0), (5, 5, 5, 5)), (-3, (0, 5, 5, 0), (5, 5, 5, 5)), GAITS["trot10"], GAITS["pace16"], odd,
            GAITS["trot10"]]
    its = [3, 3, -1, -23, 3, 9]
    want = [np.zeros((N, 4), f32), np.zeros((N, 4), f32), gait_table(*GAITS["trot10"], 9, N),
            gait_table(*GAITS["pace16"], (-23) % 16, N), gait_table(*odd, 3, N), gait_table(*GAITS["trot10"], 9, N)]
    # by hand: trot10 one step after iteration 9 is segment 0, FL and RR in stance for 5 steps
    assert want[2][:5].tolist() == [[1, 0, 0, 1]] * 5 and want[2][5:].tolist() == [[0, 1, 1, 0]] * 5
    # pace16 one step after iteration 9 is segment 10: FR and RR (offset 0) are past their 8 steps
    assert (-23) % 16 == 9 and want[3][0].tolist() == [1, 0, 1, 0] and not want[3].all()
    # leg 1's offset 20 stays negative after one += period (stance throughout), leg 2 never stands
    assert (want[4][:, 1] == 1).all() and (want[4][:, 2] == 0).all()
    gait = np.array([[p, *o, *dd] for p, o, dd in recs], np.int32)
    d = Device(eng, B, N, gait=gait)
    z3 = np.zeros((B, 3), f32)
    d.run(flags(True), np.zeros((B, 3)), np.zeros(B), iteration=its, quat=np.tile(f32([1, 0, 0, 0]), (B, 1)), pos=z3,
          omega=z3, vel=z3)
    c = d.read()["contact"]
    for b in range(B):
        assert np.array_equal(c[b], want[b]), (b, c[b], want[b])
    assert d.padding_untouched()


def test_outputs_written_only_when_documented(eng):
    """B = 5.  A tick without REFERENCE writes neither xref nor contact; an MPC tick without a
    gait writes xref and leaves contact alone.  REFERENCE | NO_INTEGRATE on an all-zero record:
    the reference has no answer (generate_reference_trajectory before the first
    update_mpc_if_needed reads xpos_base_desired and yaw_desired before mpc.py:85-87 assign
    them, an AttributeError), so this is the engine's own definition, pinned as it stands --
    xref[0, 2] is the present yaw, x_des = y_des = 0, and `started` stays 0."""
    B, N = 5, 10
    inp = make_inputs(B, 1, seed=3)
    inp["pos"][0, :, :2] *= 0.05                                  # within the clamp of the origin
    inp["vel"][0] *= 0.05                                         # below the compensation thresholds
    kw = layout_inputs("split", *(inp[k][0] for k in ("quat", "pos", "omega", "vel")))
    d = Device(eng, B, N, gait=inp["gait"], height=inp["height"])
    d.run(flags(), inp["vb"], inp["yr"], iteration=np.zeros(B), **kw)
    o = d.read()
    assert (o["xref"] == SENTINEL).all() and (o["contact"] == SENTINEL).all()
    assert (o["x0"][:B] != SENTINEL).all() and (o["state"][:B, STARTED] == 1).all()

    d = Device(eng, B, N, gait=inp["gait"], height=inp["height"])
    d.run(flags(True), inp["vb"], inp["yr"], use_gait=False, **kw)
    o = d.read()
    assert (o["contact"] == SENTINEL).all() and (o["xref"][:B] != SENTINEL).all() and d.padding_untouched()

    d = Device(eng, B, N, height=inp["height"])
    d.run(flags(True, True), inp["vb"], inp["yr"], **kw)
    o = d.read()
    yaw = np.array([quat2zyx(inp["quat"][0, b])[2] for b in range(B)])
    assert (o["state"][:B, [X, Y, ROLL, PITCH, STARTED, 6, 7]] == 0).all()
    assert np.abs(o["state"][:B, YAW] - yaw).max() <= STATE_ATOL
    assert np.array_equal(o["xref"][:B, 0, 2], o["x0"][:B, 2]) and (o["xref"][:B, 0, 3:5] == 0).all()
    assert rel_x0(o["x0"][:B, 2], f32(yaw)) <= X0_RTOL and d.padding_untouched()


@pytest.mark.parametrize("layout", ["split", "root"])
def test_non_finite_input_stays_with_its_robot(eng, layout):
    """B = 5, a NaN or an inf in robot 1's quat, pos, vel, vel_body_des and record in turn on an
    MPC tick: the other four robots are bitwise those of a clean run, outputs and records, and
    the padding is untouched.  A NaN quaternion leaves none of robot 1's Euler angles finite
    (fmin / fmax once turned its pitch into -pi/2); an inf one follows the oracle (atan2(+-inf,
    finite) and the clamped asin are +-pi/2 there too).  The kernel has no status output: where
    the input reaches the record it stays poisoned on the next, clean tick, and a zeroed record
    plans finite values again."""
    B, N = 5, 10
    inp = make_inputs(B, 3, seed=17)
    inp["quat"][:, 1] = euler_quat(0.3, -0.4, 1.0).astype(f32)    # every component of robot 1's is non-zero
    tick_inputs = lambda t: {k: inp[k][t].copy() for k in ("quat", "pos", "omega", "vel")}
    run = lambda d, fl, a, vb=inp["vb"]: d.run(fl, vb, inp["yr"], iteration=np.ones(B), **layout_inputs(layout, **a))
    first = Device(eng, B, N, gait=inp["gait"], height=inp["height"])
    run(first, flags(), tick_inputs(0))
    start = first.read()["state"][:B]
    clean = Device(eng, B, N, gait=inp["gait"], height=inp["height"], state=start)
    run(clean, flags(True), tick_inputs(1))
    oc = clean.read()
    assert all(np.isfinite(v[:B]).all() for v in oc.values())
    keep = [0, 2, 3, 4]
    cases = (("quat", 0, np.nan, True), ("quat", 2, np.inf, True), ("pos", 0, np.inf, True), ("vel", 1, np.nan, False),
             ("vel_body_des", 2, np.nan, True), ("plan_state", X, np.nan, True))
    for key, col, bad, reaches_record in cases:
        a, vb, st = tick_inputs(1), inp["vb"].copy(), start.copy()
        if key == "vel_body_des":
            vb[1, col] = bad
        elif key == "plan_state":
            st[1, col] = bad
        else:
            a[key][1, col] = bad
        dirty = Device(eng, B, N, gait=inp["gait"], height=inp["height"], state=st)
        run(dirty, flags(True), a, vb)
        od = dirty.read()
        for k in od:
            assert np.array_equal(od[k][keep].view(np.uint8), oc[k][keep].view(np.uint8)), (key, k)
            assert (od[k][B:] == SENTINEL).all(), (key, k)
        assert not np.isfinite(od["x0"][1]).all() or not np.isfinite(od["xref"][1]).all(), key
        if key == "quat" and np.isnan(bad):
            assert not np.isfinite(od["x0"][1, :3]).any(), od["x0"][1, :3]
        elif key == "quat":
            with np.errstate(all="ignore"):
                assert np.array_equal(od["x0"][1, :3], f32(quat2zyx(a["quat"][1])), equal_nan=True), od["x0"][1, :3]
        run(dirty, flags(), tick_inputs(2))                       # the next tick is clean
        assert np.isfinite(dirty.read()["state"][1]).all() != reaches_record, key
        dirty.state[1] = 0.0
        run(dirty, flags(True), tick_inputs(2))
        on = dirty.read()
        assert all(np.isfinite(v[:B]).all() for v in on.values()) and dirty.padding_untouched(), key


def test_argument_errors():
    """Every MPCQP_ERR_ARG branch of the plan launch, through the C ABI, each with its word in
    mpcqp_last_error; batch = 0 is a successful no-op; and a refused call runs nothing (only
    NULL or valid pointers are passed)."""
    from mpcqp import _lib
    eng = new_engine()
    B, N = 3, 10
    inp = make_inputs(B, 1, seed=23)
    t = {k: _dev(inp[k][0]) for k in ("quat", "pos", "omega", "vel")}
    t.update(rot=None, vb=_dev(inp["vb"]), yr=_dev(inp["yr"]), gait=_dev(inp["gait"]), height=_dev(inp["height"]),
             iteration=torch.zeros((B,), dtype=torch.int32, device=DEV),
             rs=_dev(root_rows(*(inp[k][0] for k in ("quat", "pos", "omega", "vel")))))
    ptr = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    REF = flags(True)

    def call(d, root=False, batch=B, fl=REF, **kw):
        a = dict(t, state=d.state, x0=d.x0, xref=d.xref, contact=d.contact)
        a.update(kw)
        tail = [ptr(a[k]) for k in ("vb", "yr", "gait", "iteration", "height", "state", "x0", "xref", "contact")]
        if root:
            return eng.lib.mpcqp_plan_root_states(eng._ctx, batch, fl, ptr(a["rs"]), *tail, None)
        return eng.lib.mpcqp_plan(eng._ctx, batch, fl, *(ptr(a[k]) for k in ("quat", "pos", "omega", "vel", "rot")), *tail,
                                  None)

    refused = [(dict(batch=-1), "batch"), (dict(batch=-1, root=True), "batch"), (dict(quat=None), "null"),
               (dict(pos=None), "null"), (dict(omega=None), "null"), (dict(vel=None), "null"), (dict(vb=None), "null"),
               (dict(yr=None), "null"), (dict(state=None), "null"), (dict(x0=None), "null"),
               (dict(rs=None, root=True), "null"), (dict(vb=None, root=True), "null"), (dict(yr=None, root=True), "null"),
               (dict(state=None, root=True), "null"), (dict(x0=None, root=True), "null"), (dict(fl=4), "flags"),
               (dict(fl=8), "flags"), (dict(fl=REF | 4), "flags"), (dict(fl=8, root=True), "flags"),
               (dict(height=None), "height"), (dict(xref=None), "xref"), (dict(height=None, root=True), "height"),
               (dict(xref=None, root=True), "xref"), (dict(iteration=None), "iteration"), (dict(contact=None), "contact"),
               (dict(iteration=None, root=True), "iteration"), (dict(contact=None, root=True), "contact")]
    d = Device(eng, B, N)
    d.state.fill_(SENTINEL)
    for kw, word in refused:
        assert call(d, **kw) == _lib.ERR_ARG, kw
        assert word in eng.lib.mpcqp_last_error(eng._ctx).decode(), (kw, eng.lib.mpcqp_last_error(eng._ctx))
    assert call(d, batch=0) == 0 and call(d, batch=0, root=True) == 0
    assert call(d, batch=0, quat=None, state=None) == 0           # nothing is looked at for an empty batch
    assert all((v == SENTINEL).all() for v in d.read().values())  # none of them ran anything
    with pytest.raises(_lib.MpcqpError, match="flags"):
        eng.plan(4, d.state[:B], d.x0[:B], t["vb"], t["yr"], root_states=t["rs"])
    # what is optional may be absent: no REFERENCE needs no height / xref, no gait no iteration / contact
    d.state[:B] = 0.0
    assert call(d, fl=0, height=None, xref=None, gait=None, iteration=None, contact=None) == 0
    assert call(d, root=True, gait=None, iteration=None, contact=None) == 0
    assert call(d) == 0 and call(d, root=True) == 0
    o = d.read()
    assert all((v[:B] != SENTINEL).any() for v in o.values()) and d.padding_untouched()


# ---- mpcqp_stance_torques -----------------------------------------------------------------------

def _leg_torque_run(B, seed):
    """One mpcqp_leg_torques tick for B robots of every gait (tests/test_gpu_swing.py's helper):
    its inputs, tau and which legs it holds in stance."""
    import swing_ref
    from test_gpu_swing import _engine, run_device
    from mpcqp.params import gait_record
    names = list(GAITS)
    gait = np.stack([gait_record(names[b % len(names)]) for b in range(B)])
    inp = swing_ref.make_inputs(B, 1, seed=seed)
    eng = _engine()
    out = run_device(eng, inp, gait, np.full((1, B), 120), 20)
    return eng, inp, out["tau"][0], out["swing_state"][0] == 0


@pytest.mark.parametrize("B", [1, 21, 22, 65])
def test_stance_torques_stride_and_masks(B):
    """The stance mask read as the controller reads it: row 0 of the [B][N][4] contact table,
    stance_stride = 4 N.  256 threads are 21 1/3 robots, so B = 21, 22 and 65 sit around the
    block boundaries.  Row 0 holds 1 or 0.5 for the legs mpcqp_leg_torques holds in stance and
    0, -0.0, -1 or NaN for the others (rows 1.. hold the opposite, a wrong stride would show):
    only entries > 0 are written, to the oracle's value within rtol 1e-5, atol 1e-3 and bitwise
    to what mpcqp_leg_torques writes for the same legs; the rest and the padding keep SENTINEL."""
    N = 10
    eng, inp, tau_leg, stance = _leg_torque_run(B, seed=40 + B)
    if B > 1:
        assert stance.any() and (~stance).any()
    pos_vals, neg_vals = f32([1.0, 0.5]), f32([0.0, -0.0, -1.0, np.nan])
    idx = np.arange(B * 4).reshape(B, 4)
    row0 = np.where(stance, pos_vals[idx % 2], neg_vals[idx % 4]).astype(f32)
    table = np.zeros((B, N, 4), f32)
    table[:, 0] = row0
    table[:, 1:] = np.where(stance, f32(0), f32(1))[:, None, :]
    tau = torch.full((B + PAD, 12), SENTINEL, dtype=torch.float32, device=DEV)
    eng.stance_torques(_dev(inp["jac"]), _dev(table), _dev(inp["u0"]), tau[:B], stance_stride=4 * N)
    torch.cuda.synchronize()
    got = tau.cpu().numpy()
    m = np.repeat(stance, 3, axis=1)
    assert (got[B:] == SENTINEL).all() and (got[:B][~m] == SENTINEL).all()
    with np.errstate(invalid="ignore"):
        ref = oracle_stance_torques(inp["jac"], row0, inp["u0"], np.full((B, 12), SENTINEL, f32))
    np.testing.assert_allclose(got[:B], ref, rtol=1e-5, atol=1e-3)
    assert (ref[~m] == SENTINEL).all()
    assert np.array_equal(got[:B][m].view(np.uint32), tau_leg[m].view(np.uint32))
    err = float(np.abs(got[:B][m] - ref[m]).max()) if m.any() else 0.0
    print(f"\nstance torques B={B}: {int(stance.sum())} stance legs, |tau - oracle| {err:.2e}, bitwise mpcqp_leg_torques")


def test_stance_torques_argument_errors():
    from mpcqp import _lib
    eng = new_engine()
    B = 3
    rng = np.random.default_rng(2)
    t = dict(jac=_dev(rng.standard_normal((B, 4, 3, 3)).astype(f32)), stance=torch.ones((B, 4), device=DEV),
             u0=_dev(rng.uniform(-40, 120, (B, 12)).astype(f32)),
             tau=torch.full((B + PAD, 12), SENTINEL, dtype=torch.float32, device=DEV))
    ptr = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())

    def call(batch=B, stride=4, **kw):
        a = dict(t, **kw)
        return eng.lib.mpcqp_stance_torques(eng._ctx, batch, ptr(a["jac"]), ptr(a["stance"]), stride, ptr(a["u0"]),
                                            ptr(a["tau"]), None)

    for kw, word in ((dict(stride=3), "stride"), (dict(stride=0), "stride"), (dict(stride=-4), "stride"),
                     (dict(batch=-1), "batch"), (dict(jac=None), "null"), (dict(stance=None), "null"),
                     (dict(u0=None), "null"), (dict(tau=None), "null")):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert word in eng.lib.mpcqp_last_error(eng._ctx).decode(), (kw, eng.lib.mpcqp_last_error(eng._ctx))
    assert call(batch=0) == 0 and call(batch=0, jac=None, tau=None) == 0
    torch.cuda.synchronize()
    assert (t["tau"] == SENTINEL).all()                           # a refused call and an empty batch write nothing
    assert call() == 0
    torch.cuda.synchronize()
    assert (t["tau"][:B] != SENTINEL).all() and (t["tau"][B:] == SENTINEL).all()

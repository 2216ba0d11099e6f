"""GPU: mpcqp_kinematics -- foot and thigh positions, foot Jacobians and foot velocities of
every robot in one launch -- against the reference's own product-of-exponentials chain
(tests/golden/kin.npz) and the float64 restatement tests/kin_ref.py; BatchedController.step
and the drop-in RobotData on top of it.

Tolerance (norm-wise per robot, max|a - a_ref| / max|a_ref|).  Measured on the CPU against
kin.npz (tests/test_kin.py prints them):
    tests/kin_ref.py                         3.895e-10  (jac; foot_vel_base 2.7e-10, positions 9e-16)
    csrc/mpcqp_kin_leg.h compiled with g++   3.895e-10  (the same figures)
Both are the error of the fixture's central-difference Jacobians (h = 1e-6).  Four times the
larger is 1.6e-9 -- room for float64 rounding differences between the host's and the
device's sincos -- which is below what a float32 store can hold, so the device bound is the
two-ulp float32 floor, BOUND = 2.4e-07 (under the project's 1e-5 regression guard): each
output is computed in float64 and rounded to float32 once, half an ulp (6.0e-08) of the
entry, at most that norm-wise.  The same bound holds against kin_ref.
Measured on the MI355X, against kin.npz and against kin_ref alike (max over B = 1, 3, 64,
65, the three input variants and all robots): feet 5.83e-08, thighs 5.72e-08, pos_feet
5.65e-08, foot_pos_base 5.12e-08, foot_vel_base 5.31e-08, jac 5.40e-08 -- the float32 store,
under half an ulp norm-wise.  The drop-in RobotData on the robot_data.py:234-246 state:
3.2e-08 at most (Jv_feet 1.3e-08).  BatchedController.step against a tick + leg_torques fed
kin_ref's float32 outputs: u0 and tau bitwise equal for all five robots.
"""
import importlib.util
import os

import numpy as np
import pytest

# torch first: it brings its own HIP runtime, which must be loaded before libmpcqp.so
# pulls in the system's (a CPU test file collected ahead of this one loads the library)
torch = pytest.importorskip("torch")

import kin_ref  # noqa: E402
from kin_ref import OUTPUTS, norm_err  # noqa: E402
from helpers import DEV, _dev  # noqa: E402

pytestmark = pytest.mark.gpu

BOUND = 2.4e-7
SENTINEL = -77.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    from mpcqp import LinearMpc
    return LinearMpc(horizon=10, robot="aliengo", device=DEV)


@pytest.fixture(scope="module")
def fx():
    return kin_ref.load_fixture()


def batch(fx, B):
    """The first B robots of the fixture (it has 64; past that they repeat), A1 and Aliengo
    geometry mixed: (rows into the fixture, geom [B,5], inputs dict)."""
    rows = np.arange(B) % len(fx["quat"])
    return rows, fx["geom"][rows], {k: fx[k][rows] for k in ("quat", "pos", "vel", "omega", "q", "qdot")}


def run_device(eng, geom, inp, layout="split", rot=None, skip=(), pad=3):
    """One launch; every output buffer has `pad` extra rows filled with SENTINEL, returned too.
    Outputs named in `skip` are passed as NULL (and come back as None)."""
    from mpcqp.params import pack_leg_geometry
    B = len(geom)
    g = _dev(pack_leg_geometry(geom), torch.float64)
    full = {k: torch.full((B + pad, 4, 3, 3) if k == "jac" else (B + pad, 4, 3), SENTINEL, dtype=torch.float32,
                          device=DEV) for k in OUTPUTS}
    outs = {k: (None if k in skip else full[k][:B]) for k in OUTPUTS}
    if layout == "root":
        eng.kinematics(g, root_states=_dev(kin_ref.root_states(inp["quat"], inp["pos"], inp["vel"], inp["omega"])),
                       dof_states=_dev(kin_ref.dof_states(inp["q"], inp["qdot"])), **outs)
    else:
        eng.kinematics(g, q=_dev(inp["q"]), qdot=_dev(inp["qdot"]), quat=_dev(inp["quat"]), pos=_dev(inp["pos"]),
                       vel=_dev(inp["vel"]), omega=_dev(inp["omega"]),
                       rot=_dev(rot, torch.float32) if rot is not None else None, **outs)
    torch.cuda.synchronize()
    return {k: (None if k in skip else full[k].cpu().numpy()) for k in OUTPUTS}


def assert_close(out, ref, B, tag, rows=None):
    errs = kin_ref.robot_errors({k: out[k][:B] for k in OUTPUTS}, ref, rows)
    print(f"\n{tag}: " + ", ".join(f"{k} {float(v.max()):.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert (v <= BOUND).all(), (tag, k, v.max())
    for k in OUTPUTS:
        assert (out[k][B:] == SENTINEL).all(), (tag, k, "padding written")


@pytest.mark.parametrize("B", [1, 3, 64, 65])
@pytest.mark.parametrize("layout", ["split", "root", "rot"])
def test_parity(eng, fx, B, layout):
    """Against kin.npz and against kin_ref, both layouts and the split layout with R_base
    supplied; B = 64 fills the workgroup's last lanes, 65 starts a second workgroup.  With
    `rot` the caller's matrix is used: the fixture's own R_base first (every output still
    matches kin.npz), then another robot's (against kin_ref, which takes the same matrix)."""
    rows, geom, inp = batch(fx, B)
    rot = fx["R_base"][rows] if layout == "rot" else None
    out = run_device(eng, geom, inp, layout=layout, rot=rot)
    assert_close(out, fx, B, f"B={B} {layout} vs kin.npz", rows)
    assert_close(out, kin_ref.kinematics(geom, rot=rot, **inp), B, f"B={B} {layout} vs kin_ref")
    if layout == "rot":
        other = fx["R_base"][(rows + 7) % len(fx["quat"])]
        out2 = run_device(eng, geom, inp, layout="rot", rot=other)
        assert_close(out2, kin_ref.kinematics(geom, rot=other, **inp), B, f"B={B} other rot vs kin_ref")
        for k in ("feet", "pos_feet", "jac"):                   # R_base does not enter these
            assert np.array_equal(out2[k], out[k]), k
        for k in ("thighs", "foot_pos_base", "foot_vel_base"):
            assert not np.array_equal(out2[k], out[k]), k


@pytest.mark.parametrize("layout", ["split", "root"])
def test_null_outputs_and_padding(eng, fx, layout):
    """Each output NULL in turn: the others are bitwise what the full launch writes, and the
    padded rows past B keep their sentinel."""
    B = 65
    _, geom, inp = batch(fx, B)
    want = run_device(eng, geom, inp, layout=layout)
    for k in OUTPUTS:
        assert (want[k][B:] == SENTINEL).all() and np.isfinite(want[k][:B]).all() and (want[k][:B] != SENTINEL).all()
    for skip in OUTPUTS:
        got = run_device(eng, geom, inp, layout=layout, skip=(skip,))
        assert got[skip] is None
        for k in OUTPUTS:
            if k != skip:
                assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (skip, k)
    none = run_device(eng, geom, inp, layout=layout, skip=OUTPUTS)         # nothing to write: still a launch
    assert all(v is None for v in none.values())


def test_argument_errors(eng, fx):
    """batch == 0 is a no-op, a missing input and an unknown flag are MPCQP_ERR_ARG, as for
    mpcqp_leg_torques."""
    import ctypes
    from mpcqp import _lib
    lib, ctx = eng.lib, eng._ctx
    null = ctypes.c_void_p(0)
    assert lib.mpcqp_kinematics(ctx, 0, 0, *([null] * 15)) == 0
    assert lib.mpcqp_kinematics_root_states(ctx, 0, 0, *([null] * 10)) == 0
    assert lib.mpcqp_kinematics(ctx, -1, 0, *([null] * 15)) == _lib.ERR_ARG
    _, geom, inp = batch(fx, 2)
    with pytest.raises(_lib.MpcqpError):
        eng.kinematics(_dev(np.zeros((2, 8))), q=_dev(inp["q"]), qdot=None, quat=_dev(inp["quat"]),
                       pos=_dev(inp["pos"]), vel=_dev(inp["vel"]), omega=_dev(inp["omega"]))
    g = _dev(np.zeros((2, 8)))
    rs = _dev(kin_ref.root_states(inp["quat"], inp["pos"], inp["vel"], inp["omega"]))
    ds = _dev(kin_ref.dof_states(inp["q"], inp["qdot"]))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.mpcqp_kinematics_root_states(ctx, 2, 1, p(rs), p(ds), p(g), *([null] * 7)) == _lib.ERR_ARG
    assert lib.mpcqp_kinematics_root_states(ctx, 2, 0, p(rs), null, p(g), *([null] * 7)) == _lib.ERR_ARG
    torch.cuda.synchronize()


@pytest.mark.parametrize("layout", ["split", "root"])
def test_non_finite_input_stays_with_its_robot(eng, fx, layout):
    """A NaN in one hip angle of robot 63, the last of the first workgroup (the hip's, as the
    thigh-joint position depends on no other angle): that robot's outputs for the leg are
    non-finite, every other robot -- 62 beside it, 64 in the next
    workgroup -- is bitwise what it is without the NaN."""
    B, bad, leg = 65, 63, 2
    _, geom, inp = batch(fx, B)
    want = run_device(eng, geom, inp, layout=layout)
    inp = dict(inp, q=inp["q"].copy())
    inp["q"][bad, 3 * leg] = np.nan
    got = run_device(eng, geom, inp, layout=layout)
    others = np.arange(B + 3) != bad
    for k in OUTPUTS:
        assert not np.isfinite(got[k][bad, leg]).any(), k
        assert np.array_equal(got[k][others].view(np.uint32), want[k][others].view(np.uint32)), k
        assert np.isfinite(got[k][:B][others[:B]]).all(), k


def _controllers(n, B, **kw):
    from mpcqp.controller import BatchedController
    return [BatchedController(B, horizon=10, robot="a1", gait="TROTTING10", **kw) for _ in range(n)]


def test_batched_controller_step():
    """45 control iterations (80..124) of B = 5 robots in TROTTING10 at the reference's
    iterations_between_mpc = 20: MPC ticks at 80, 100 and 120, legs 1 and 2 touch down at
    100 and legs 0 and 3 lift off at 101.  step() is bitwise the three calls made by hand on
    the same buffers, at every iteration; and on the first iteration's inputs u0 and tau
    match a tick + leg_torques fed kin_ref's outputs rounded to float32 (the swing decision
    is an integer one on the tick, so no leg sits on a swing / stance boundary)."""
    from test_gpu_swing import BOUND as SWING_BOUND
    B, T, start = 5, 45, 80
    rs_all, ds_all = kin_ref.make_states(B, T, seed=5)
    vb, yr = np.array([0.5, 0.1, 0.0]), 0.1
    a, h, c = _controllers(3, B)
    assert torch.equal(a.geometry[:, :5].cpu(), torch.tensor([[0.183, 0.047, 0.08505, 0.2, 0.2]] * B,
                                                             dtype=torch.float64))
    first = None
    masks = []
    for t in range(T):
        it = start + t
        rs, ds = _dev(rs_all[t]), _dev(ds_all[t])
        tau = a.step(it, vb, yr, rs, ds)
        h.engine.kinematics(h.geometry, root_states=rs, dof_states=ds, feet=h.feet, thighs=h.thighs,
                            pos_feet=h.pos_feet, foot_pos_base=h.foot_pos_base, foot_vel_base=h.foot_vel_base,
                            jac=h.jac)
        h.tick(it, vb, yr, h.feet, root_states=rs)
        tau_h = h.leg_torques(it, vb, yr, h.thighs, h.pos_feet, h.foot_pos_base, h.foot_vel_base, h.jac,
                              root_states=rs)
        torch.cuda.synchronize()
        assert tau is a.tau and tuple(tau.shape) == (B, 12)
        for k in ("tau", "u0", "x0", "swing_state", "pos_target", "vel_target", "swing_mem", "feet", "jac"):
            assert torch.equal(getattr(a, k), getattr(h, k)), (it, k)
        assert torch.isfinite(tau).all() and (a.status == 0).all(), it
        masks.append((a.swing_state > 0).cpu().numpy())
        if t == 0:
            first = dict(u0=a.u0.cpu().numpy(), tau=a.tau.cpu().numpy())
    masks = np.stack(masks)                                   # [T,B,4]
    assert masks[20, :, 1:3].all() and not masks[21, :, 1:3].any()        # touchdown after iteration 100
    assert not masks[20, :, [0, 3]].any() and masks[21, :, [0, 3]].all()  # lift-off at 101
    # the first iteration again, from the restatement's kinematics
    rs0, ds0 = rs_all[0], ds_all[0]
    quat = np.concatenate([rs0[:, 6:7], rs0[:, 3:6]], 1)
    ref = kin_ref.kinematics(np.tile(a.geometry[:1, :5].cpu().numpy(), (B, 1)), quat, rs0[:, 0:3], rs0[:, 7:10],
                             rs0[:, 10:13], ds0[..., 0], ds0[..., 1])
    r = {k: _dev(v.astype(np.float32)) for k, v in ref.items()}
    c.tick(start, vb, yr, r["feet"], root_states=_dev(rs0))
    c.leg_torques(start, vb, yr, r["thighs"], r["pos_feet"], r["foot_pos_base"], r["foot_vel_base"], r["jac"],
                  root_states=_dev(rs0))
    torch.cuda.synchronize()
    u0, tau = c.u0.cpu().numpy(), c.tau.cpu().numpy()
    # not a comparison of zeros: every robot carries weight and commands torque on that iteration
    assert (np.abs(u0).max(axis=1) > 1.0).all() and (np.abs(tau).max(axis=1) > 1e-2).all()
    for b in range(B):
        eu, et = norm_err(first["u0"][b], u0[b]), norm_err(first["tau"][b], tau[b])
        print(f"robot {b}: u0 {eu:.2e} tau {et:.2e}")
        assert eu <= SWING_BOUND and et <= SWING_BOUND, (b, eu, et)


def test_controller_geometry_argument(fx):
    """geometry= takes a preset name, five numbers or a [B,5] array; the default is the robot
    preset's; a packed robot record has none and step() says so."""
    from mpcqp.controller import BatchedController
    from mpcqp.params import LEG_GEOMETRY, ROBOT_PRESETS, pack_robot
    B = 4
    mixed = fx["geom"][:B]
    ctl = BatchedController(B, horizon=10, robot="aliengo", geometry=mixed)
    assert np.array_equal(ctl.geometry.cpu().numpy()[:, :5], mixed)
    ctl = BatchedController(B, horizon=10, robot="aliengo")
    assert np.array_equal(ctl.geometry.cpu().numpy()[:, :5], np.tile(LEG_GEOMETRY["aliengo"], (B, 1)))
    rec = np.tile(pack_robot(ROBOT_PRESETS["a1"]), (B, 1))
    ctl = BatchedController(B, horizon=10, robot=rec, height=0.3)
    rs, ds = kin_ref.make_states(B, 1, seed=2)
    with pytest.raises(ValueError, match="geometry"):
        ctl.step(0, [0.0, 0.0, 0.0], 0.0, _dev(rs[0]), _dev(ds[0]))
    # a mixed fleet through the controller: its buffers against kin_ref
    ctl = BatchedController(B, horizon=10, robot=rec, height=0.3, geometry=mixed)
    ctl.kinematics(_dev(rs[0]), _dev(ds[0].reshape(B * 12, 2)))        # Isaac Gym's flat dof tensor
    torch.cuda.synchronize()
    quat = np.concatenate([rs[0][:, 6:7], rs[0][:, 3:6]], 1)
    ref = kin_ref.kinematics(mixed, quat, rs[0][:, 0:3], rs[0][:, 7:10], rs[0][:, 10:13], ds[0][..., 0], ds[0][..., 1])
    errs = kin_ref.robot_errors({k: getattr(ctl, k).cpu().numpy() for k in OUTPUTS}, ref)
    assert max(float(v.max()) for v in errs.values()) <= BOUND


def test_drop_in_robot_data(fx, tmp_path):
    """The drop-in RobotData on the state printed in robot_data.py:234-246, its geometry read
    from a URDF text written here: every attribute the reference's consumers read against
    the fixture."""
    spec = importlib.util.spec_from_file_location(
        "robot_data_drop_in", os.path.join(ROOT, "pympc-quadruped_amd", "utils", "robot_data.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "import pinocchio" not in open(mod.__file__).read()
    urdf = tmp_path / "aliengo_like.urdf"
    urdf.write_text(kin_ref.urdf_text(geom=(0.2399, 0.051, 0.083, 0.25, 0.25)))
    rd = mod.RobotData(robot_model=str(urdf))
    assert rd.leg_geometry == tuple(fx["geom_aliengo"])
    d = lambda k: fx["demo_" + k]
    # lists of Python floats, as robot_data.py:234-246 passes them
    rd.update(pos_base=[float(x) for x in d("pos")], lin_vel_base=[float(x) for x in d("vel")],
              quat_base=[float(x) for x in d("quat")], ang_vel_base=[float(x) for x in d("omega")],
              q=[float(x) for x in d("q")], qdot=[float(x) for x in d("qdot")])
    for attr, key in (("pos_base", "pos"), ("lin_vel_base", "vel"), ("quat_base", "quat"), ("ang_vel_base", "omega"),
                      ("q", "q"), ("qdot", "qdot"), ("R_base", "R_base")):
        assert np.array_equal(getattr(rd, attr), d(key)), attr
    assert rd.R_base.dtype == np.float32 and rd.R_base.shape == (3, 3)
    assert np.allclose(rd.rpy_base, d("rpy"), rtol=0, atol=1e-15)
    for attr, key in (("pos_feet", "pos_feet"), ("pos_base_feet", "feet"), ("base_pos_base_feet", "foot_pos_base"),
                      ("base_vel_base_feet", "foot_vel_base"), ("base_pos_base_thighs", "thighs"), ("Jv_feet", "Jv")):
        got = getattr(rd, attr)
        assert isinstance(got, list) and len(got) == 4, attr
        assert np.asarray(got).shape == d(key).shape, attr
        e = norm_err(np.asarray(got), d(key))
        print(f"{attr} {e:.2e}")
        assert e <= BOUND, (attr, e)
    for leg in range(4):                                   # the zero columns are exactly zero
        rest = np.delete(rd.Jv_feet[leg], np.r_[0:6, 6 + 3 * leg:9 + 3 * leg], axis=1)
        assert (rest == 0).all()
    # a second update reuses the bound buffers
    rd.update(d("pos"), d("vel"), d("quat"), d("omega"), np.zeros(12, np.float32), np.zeros(12, np.float32))
    want = kin_ref.kinematics(fx["geom_aliengo"][None], d("quat")[None], d("pos")[None], d("vel")[None],
                              d("omega")[None], np.zeros((1, 12)), np.zeros((1, 12)))
    assert norm_err(np.asarray(rd.base_pos_base_feet), want["foot_pos_base"][0]) <= BOUND
    for name in ("base_Jv_feet", "pos_thighs", "X_base"):
        with pytest.raises(NotImplementedError):
            getattr(rd, name)
    with pytest.raises(NotImplementedError):
        rd.update_terrain_normal([1, 1, 1, 1])
    with pytest.raises(NotImplementedError):
        mod.RobotData(robot_model=str(urdf), state_estimation=True).update(*([[0.0] * 3] * 2), [1.0, 0, 0, 0],
                                                                           [0.0] * 3, [0.0] * 12, [0.0] * 12)

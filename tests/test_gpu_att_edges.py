"""GPU: mpcqp_attitude at its edges -- the contact trust on the leg controller's decision
table (ticks at the ends of int32, spans up to 2^31, ramps over 2^30 iterations), the
first-tick special cases, the corners of the accelerometer gate and the small-angle switch,
large rotations per tick through the device's own sin / cos, seeded records of any length,
refusal across a workgroup boundary, and BatchedEstimator.update_from_imu's argument checks.
The checks are tests/att_edge_checks.py, which tests/test_att.py runs on the host build of
csrc/mpcqp_attitude_robot.h with the same inputs (att_ref's edge tables), so each assertion is
known to hold for correct code.  W = 64 robots per workgroup, one lane per robot; every
launch keeps two sentinel rows past B and finds them untouched.

Bounds.  The record against att_ref at Q_BOUND = 10 att_ref.D_Q = 5.6e-15 (the quaternion up
to sign); the trust bitwise the float32 of att_ref.gait_trust and within 2^-24 relative of an
exact rational restatement (att_edge_checks.trust_exact); | |q| - 1 | <= 4e-16.
The header on the host (tests/test_att.py): trust bitwise on every row and window; first tick
0 (bitwise att_ref), after 5 ticks 1.1e-16; gate corners 1.4e-17, small-angle switch 0; large
rotation 1.1e-16, at 1e6 and 3e38 rad/s 1.1e-16 and 5.6e-17 (both sides glibc, so this says
nothing about the device); seeded quaternions of norm 2, 1e-3, 1e-160 1.1e-16.
Measured on the MI355X: first tick 0, after 5 ticks 1.11e-16; gate corners 1.39e-17,
small-angle switch 0; large rotation (up to 23 rad per tick) 5.55e-17; seeded quaternions
1.11e-16; trust bitwise on all 127 rows x 4 windows.  The two unasserted distances to att_ref
at 1e6 and 3e38 rad/s, the device's argument reduction against glibc's: 1.11e-16 and 5.55e-17.
"""
import numpy as np
import pytest

# torch first: it brings its own HIP runtime, which must be loaded before libmpcqp.so
torch = pytest.importorskip("torch")

import att_edge_checks  # noqa: E402
import att_ref  # noqa: E402
import est_ref  # noqa: E402
import kin_ref  # noqa: E402
from test_gpu_att import ALL, DEV, Device, _dev, new_engine  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def launch():
    eng = new_engine()                                       # its own: the constants are changed here

    def run(state, inp, constants):
        eng.set_attitude(**dict(att_ref.DEFAULTS, **(constants or {})))
        d = Device(eng, state.shape[0], state=state)
        d.tick(att_ref.select(inp, ALL))
        no_trust = "gait" not in inp and "touch" not in inp
        assert d.padding_untouched(("trust",) if no_trust else ())
        return d.read()
    return run


@pytest.mark.parametrize("ibm", [1, 20, 2 ** 20])
def test_trust_on_the_decision_table(launch, ibm):
    """a.  One launch per window with B = the table's rows (42, 42, 43), each robot on its own
    tick: bitwise att_ref, 0 exactly where the leg controller swings, within 2^-24 of the
    exact rational; 0, 1 and a ramp all occur for w = 0.2 and 0.5, only 0 and 1 for 0 and
    1e-300."""
    assert len(att_ref.trust_edges(ibm)[0]) == (43 if ibm == 2 ** 20 else 42)
    for window in att_ref.TRUST_WINDOWS:
        att_edge_checks.check_trust_table(launch, ibm, window)


def test_touch_at_the_threshold(launch):
    """a.  At the threshold and one float32 below it the trust is 0; one above, the gait's."""
    att_edge_checks.check_touch_threshold(launch)


def test_first_tick(launch):
    """b."""
    first, later = att_edge_checks.check_first_tick(launch)
    print(f"\nfirst tick on the device: {first:.2e}, after 5 ticks {later:.2e}")


def test_gate_and_small_angle_switch(launch):
    """c."""
    gate, switch = att_edge_checks.check_gate_and_switch(launch)
    print(f"\ngate corners on the device: {gate:.2e}, small-angle switch {switch:.2e}")


def test_large_rotation_per_tick(launch):
    """d.  The two distances at 1e6 and 3e38 rad/s are printed, not asserted: they measure
    the device's argument reduction against glibc's."""
    large, huge = att_edge_checks.check_large_rotation(launch)
    print(f"\nlarge rotation on the device: {large:.2e}; distance to att_ref at 1e6 and 3e38 rad/s "
          + ", ".join(f"{v:.2e}" for v in huge))


def test_seeded_records(launch):
    """e."""
    seeded = att_edge_checks.check_seeded_records(launch)
    print(f"\nseeded quaternions of norm 2, 1e-3, 1e-160 on the device: {seeded:.2e}")


def test_refusal_across_a_workgroup_boundary(launch):
    """e.  B = 65, robots 63 and 64."""
    att_edge_checks.check_refusal_across_a_workgroup(launch)


def test_update_from_imu_arguments_and_a_bad_touch():
    """f.  ValueError for a controller of another batch size, a tick tensor of the wrong
    length and a touch of the wrong shape; an int64 tick tensor and a non-contiguous gyro view
    give the bits of their int32 / contiguous copies; a robot whose touch is NaN for one tick
    has attitude_status 4 and trusts 0, its filter record is still one the estimator accepts,
    and the next clean tick recovers."""
    from mpcqp.controller import BatchedController
    from mpcqp.estimator import BatchedEstimator
    B = 4
    ctl = BatchedController(B, robot="a1", gait="TROTTING10")
    with pytest.raises(ValueError, match="robots"):
        BatchedEstimator(B + 1, robot="a1", controller=ctl)
    inp = est_ref.level_crouch(B, "a1")
    dofs = _dev(kin_ref.dof_states(inp["q"], inp["qdot"]))
    rng = np.random.default_rng(4)
    wide = _dev(rng.uniform(-0.3, 0.3, (B, 6)).astype(np.float32))
    gyro_view, accel = wide[:, ::2], _dev(inp["accel"])
    assert not gyro_view.is_contiguous()
    ticks = np.array([3, 59, 120, 199])
    touch = torch.ones((B, 4), device=DEV)

    def fresh():
        return BatchedEstimator(B, robot="a1", controller=ctl)

    est = fresh()
    with pytest.raises(ValueError, match="expected"):
        est.update_from_imu(gyro_view, accel, dofs, tick=torch.zeros((B + 1,), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="expected"):
        est.update_from_imu(gyro_view, accel, dofs, tick=3, touch=torch.ones((B, 3), device=DEV))
    torch.cuda.synchronize()
    assert (est.att_state == 0).all() and (est.est_state == 0).all()         # nothing ran

    def run(est, gyro, tick):
        for _ in range(3):
            est.update_from_imu(gyro, accel, dofs, tick=tick, touch=touch)
        torch.cuda.synchronize()
        return [t.cpu().numpy().tobytes() for t in (est.att_state, est.est_state, est.root_states, est.trust, est.quat)]

    a = run(fresh(), gyro_view, _dev(ticks.astype(np.int64)))
    b = run(fresh(), gyro_view.contiguous(), _dev(ticks.astype(np.int32)))
    assert a == b

    est, clean = fresh(), fresh()
    for e in (est, clean):
        for i in range(5):
            e.update_from_imu(gyro_view, accel, dofs, tick=20 + i, touch=touch)
    bad = touch.clone()
    bad[2, 1] = float("nan")
    torch.cuda.synchronize()
    before = est.att_state.clone()
    est.update_from_imu(gyro_view, accel, dofs, tick=25, touch=bad)
    clean.update_from_imu(gyro_view, accel, dofs, tick=25, touch=touch)
    torch.cuda.synchronize()
    assert est.attitude_status.tolist() == [0, 0, 4, 0] and (est.trust[2] == 0).all() and (est.status == 0).all()
    assert torch.equal(est.att_state[2], before[2]) and torch.isfinite(est.est_state).all()
    keep = [0, 1, 3]
    assert torch.equal(est.att_state[keep], clean.att_state[keep]) and torch.equal(est.trust[keep], clean.trust[keep])
    assert torch.equal(est.root_states[keep], clean.root_states[keep])
    est.update_from_imu(gyro_view, accel, dofs, tick=26, touch=touch)
    clean.update_from_imu(gyro_view, accel, dofs, tick=26, touch=touch)
    torch.cuda.synchronize()
    assert (est.attitude_status == 0).all() and (est.status == 0).all()
    assert torch.equal(est.trust, clean.trust) and float(est.trust[2].max()) > 0
    assert torch.equal(est.att_state[keep], clean.att_state[keep]) and torch.isfinite(est.root_states).all()

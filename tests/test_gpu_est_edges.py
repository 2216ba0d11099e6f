"""GPU: mpcqp_estimate at its edges -- a non-finite value that one lane alone sees, in every
input element and in every kind of word of the record, trust values at the clip, the
quaternion used as given, the record's other words, long single-regime runs, batch shapes
with an idle robot slot, and every argument the host refuses.  The inputs are est_ref's edge
tables; tests/test_est.py runs the same ones through the kernel on host threads with the
same assertions (est_ref.assert_refused), so each is known to hold for correct code.

kEstRobots = 3; B = 7 is workgroup slots 0, 1, 2, a second workgroup and a tail of one.
Aliengo engine, A1 / Aliengo geometry alternating.  Every launch keeps two sentinel rows past
B, and they and every NULL output's buffer are asserted untouched.

Bounds.  Ordinary inputs: X_BOUND = 10 D_X = 1.94e-10, P_BOUND = 10 D_P = 4.8e-14, F32_BOUND =
2.4e-7 (tests/test_gpu_est.py).  The long regimes have a rounding sensitivity of their own:
est_ref's batch and sequential forms differ on those very inputs by d (est_ref.D_REGIME,
measured and asserted by tests/test_est.py at B = 7, 200 ticks, seed 11)
  all trust 0             d_x 7.17e-12   d_P 1.95e-14
  all trust 1             d_x 5.86e-11   d_P 1.96e-15
  zero noise, suspicion   d_x 8.56e-10   d_P 1.96e-15
and the device is held to 10 d, its float32 outputs to max(2.4e-7, 10 d_x).
The kernel on host threads (tests/test_est.py): trust inside (0, 1) x 3.1e-14, P 3.6e-16;
quaternion 2 q / q / 2 / 0: x 1.2e-11 / 6.3e-12 / 8.2e-12, P 1.2e-15; regimes x 8.4e-12 /
6.0e-11 / 7.2e-10, P 2.2e-14 / 2.1e-15 / 2.7e-15, float32 outputs 5.9e-08; B = 2, 5, 6: x
9.3e-13, P 2.2e-15.
Measured on the MI355X (printed by the tests; the host-thread figures to the digit): trust
inside (0, 1) x 3.14e-14, P 3.55e-16; quaternion 2 q / q / 2 / 0 x 1.20e-11 / 6.25e-12 /
8.24e-12, P 1.24e-15; regimes (swing, stance, noiseless) x 8.38e-12 / 6.02e-11 / 7.17e-10, P
2.17e-14 / 2.13e-15 / 2.69e-15, float32 outputs 5.62e-08 / 5.93e-08 / 5.84e-08; B = 2, 5, 6
x 9.28e-13, P 2.19e-15, float32 outputs 5.80e-08.
"""
import ctypes

import numpy as np
import pytest

# torch first: it brings its own HIP runtime, which must be loaded before libmpcqp.so
torch = pytest.importorskip("torch")

import est_ref  # noqa: E402
import kin_ref  # noqa: E402
from est_ref import assert_refused, same_bits  # noqa: E402
from test_gpu_est import DEV, F32_BOUND, OUTS, P_BOUND, SENTINEL, X_BOUND, Device, _dev, first  # noqa: E402

pytestmark = pytest.mark.gpu

B = 7
ZERO = np.zeros((B, est_ref.STRIDE))


@pytest.fixture(scope="module")
def eng():
    from mpcqp import LinearMpc
    return LinearMpc(horizon=10, robot="aliengo", device=DEV)


@pytest.fixture(scope="module")
def start():
    """The generator's trajectory for B robots and est_ref's records after 5 ticks."""
    traj = est_ref.make_trajectory(B, 12, seed=7)
    return traj, est_ref.run(traj[:5])[0][-1]


def tick(eng, state, inp, layout="split", skip=()):
    """One launch from the records `state`: (records, outputs) with their sentinel rows; the
    sentinel rows and every NULL output's buffer are untouched."""
    d = Device(eng, state.shape[0], state=state)
    d.tick(inp, layout, skip)
    assert d.padding_untouched(skip)
    return d.read()


def same(a, b):
    return same_bits(a[0], b[0]) and all(same_bits(a[1][k], b[1][k]) for k in OUTS)


def follow(eng, traj, state, constants=None):
    """Every tick of `traj` on the device from `state`: ([T+1,B,STRIDE] records, the outputs of
    each tick).  Status 0, P bitwise symmetric, everything finite, sentinels untouched."""
    n = state.shape[0]
    d = Device(eng, n, state=state)
    states, outs = [state], []
    for inp in traj:
        d.tick(inp)
        st, o = d.read()
        P = est_ref.unpack(st[:n])[1]
        assert (o["status"][:n] == 0).all() and np.array_equal(P, np.swapaxes(P, 1, 2)) and np.isfinite(st[:n]).all()
        states.append(st[:n])
        outs.append(o)
    assert d.padding_untouched()
    return np.stack(states), outs


def f32_err(outs, ref_outs, n):
    return max(est_ref.norm_err(o[k][b], r[k][b]) for o, r in zip(outs, ref_outs)
               for k in ("root_states", "feet_world") for b in range(n))


def test_a_value_one_lane_sees_refuses_that_robot(eng, start):
    """a.  One launch per (input, element): the joints and the trust of legs 1..3 reach one
    leg lane only.  In the dof-state layout (qdot NULL) a position and a velocity slot of each
    leg.  geom words 5..7 are read by nobody.  Each output is NULL in turn over the cases."""
    traj, st0 = start
    clean = {(layout, skip): tick(eng, st0, traj[5], layout, skip)
             for layout in ("split", "dof") for skip in ((), ("root_states",), ("feet_world",))}
    skips = ((), (), ("root_states",), ("feet_world",))
    for i, (key, e, v, robot) in enumerate(est_ref.nonfinite_cases()):
        inp = est_ref.poisoned(traj[5], key, e, v, robot)
        skip = skips[i % 4]
        assert_refused(st0, inp["quat"], clean["split", skip], tick(eng, st0, inp, "split", skip), robot, skip,
                       tag=(key, e, v, robot))
    for i, (key, e, v, robot) in enumerate(est_ref.dof_cases()):
        inp = est_ref.poisoned(traj[5], key, e, v, robot)
        skip = skips[i % 4]
        assert_refused(st0, inp["quat"], clean["dof", skip], tick(eng, st0, inp, "dof", skip), robot, skip,
                       tag=("dof", key, e, v, robot))
    for word in (5, 6, 7):
        assert same(tick(eng, st0, est_ref.poisoned(traj[5], "geom", word, np.nan, 1)), clean["split", ()])


def test_refusal_on_a_fresh_record(eng, start):
    """b.  An all-zero record and a NaN joint: the record stays all-zero, position, velocity
    and feet are exactly 0, and the next clean tick is a first tick."""
    traj, _ = start
    clean = tick(eng, ZERO, traj[0])
    inp = est_ref.poisoned(traj[0], "q", 7, np.nan, 4)
    sd, od = tick(eng, ZERO, inp)
    assert_refused(ZERO, inp["quat"], clean, (sd, od), 4)
    assert (sd[4] == 0).all() and (od["root_states"][4, [0, 1, 2, 7, 8, 9]] == 0).all() and (od["feet_world"][4] == 0).all()
    s2, o2 = tick(eng, sd[:B], traj[0])
    assert same_bits(s2[4], clean[0][4]) and all(same_bits(o2[k][4], clean[1][k][4]) for k in OUTS)


def test_trust_values(eng, start):
    """c.  -0.0, one ulp over 1 and +-3e38 are 0, 1, 1, 0 to the bit; a subnormal, one ulp under
    1, 0.5 and 0.25 follow est_ref (reading leg 0's trust for every leg: over 100 bounds off,
    tests/test_est.py)."""
    traj, st0 = start
    tile = lambda t: np.tile(t, (B, 1))
    assert same(tick(eng, st0, dict(traj[5], trust=tile(est_ref.TRUST_OUTSIDE))),
                tick(eng, st0, dict(traj[5], trust=tile(est_ref.TRUST_CLIPPED))))
    inp = dict(traj[5], trust=tile(est_ref.TRUST_INSIDE))
    st, out = tick(eng, st0, inp)
    ref, ref_out = est_ref.estimate_step(st0, inp)
    dx, dP = est_ref.worst_err([None, st[:B]], [None, ref])
    f32 = f32_err([out], [ref_out], B)
    print(f"\ntrust inside (0, 1) on the device: x {dx:.2e}, P {dP:.2e}, float32 outputs {f32:.2e}")
    assert dx <= X_BOUND and dP <= P_BOUND and f32 <= F32_BOUND and (out["status"][:B] == 0).all()


def test_a_nonfinite_record_is_refused(eng, start):
    """d.  NaN / inf in x_0, x_4, x_17, in P on and off the diagonal, NaN in the `initialised`
    word, for robots 2 (slot 2) and 6 (the tail): status 4, the record as it was, the others
    bitwise clean, and the same again on the next tick.  The same words in a record whose
    `initialised` word is 0 are not read: a first tick, status 0."""
    traj, st0 = start
    clean = tick(eng, st0, traj[5])
    for word, v, robot in est_ref.record_cases():
        seeded = st0.copy()
        seeded[robot, word] = v
        dirty = tick(eng, seeded, traj[5])
        ref = (np.vstack([clean[0][:robot], seeded[robot:robot + 1], clean[0][robot + 1:]]), clean[1])
        assert_refused(seeded, traj[5]["quat"], ref, dirty, robot, tag=(word, v, robot))
        again = tick(eng, dirty[0][:B], traj[6])
        assert again[1]["status"][robot] == 4 and same_bits(again[0][robot], seeded[robot])
    fresh = ZERO.copy()
    fresh[2, [0, 4, 17]] = np.nan
    fresh[6, [est_ref.P_OFF, est_ref.P_OFF + 29]] = np.nan, np.inf
    got = tick(eng, fresh, traj[5])
    assert same(got, tick(eng, ZERO, traj[5])) and (got[1]["status"][:B] == 0).all()


def test_other_words_of_the_record(eng, start):
    """e.  `initialised` = 2.0 and -3.0 behave as 1 and are rewritten to 1.0; padding words
    set to 5.0 / 6.0 keep their bits and change nothing else."""
    traj, st0 = start
    clean = tick(eng, st0, traj[5])
    seeded = st0.copy()
    seeded[1, est_ref.INIT], seeded[3, est_ref.INIT] = 2.0, -3.0
    seeded[:, est_ref.PADDING[:5]], seeded[:, est_ref.PADDING[5:]] = 5.0, 6.0
    sd, od = tick(eng, seeded, traj[5])
    pad = list(est_ref.PADDING)
    assert (sd[:B, est_ref.INIT] == 1.0).all() and same_bits(sd[:B, pad], seeded[:, pad])
    sd[:B, pad] = 0.0
    assert same((sd, od), clean)


def test_quaternion_as_given(eng, start):
    """f.  2 q, q / 2 and 0 over 10 ticks follow est_ref fed the same quaternion (0 gives
    R = I by the documented formula; a kernel that normalised q would be over 100 bounds off
    for 2 q, tests/test_est.py); -q gives q's record to the bit and root_states carries -q."""
    traj, st0 = start
    given = traj[:10]
    variants = {name: [dict(t, quat=est_ref.quat_variants(t["quat"])[name]) for t in given]
                for name in ("double", "half", "zero", "negated")}
    for name in ("double", "half", "zero"):
        states, outs = follow(eng, variants[name], st0)
        ref, ref_outs = est_ref.run(variants[name], state=st0)
        dx, dP = est_ref.worst_err(states, ref)
        f32 = f32_err(outs, ref_outs, B)
        print(f"\nquaternion {name} on the device: x {dx:.2e}, P {dP:.2e}, float32 outputs {f32:.2e}")
        assert dx <= X_BOUND and dP <= P_BOUND and f32 <= F32_BOUND
    assert np.array_equal(kin_ref.quat2matrix_eigen(np.zeros((1, 4)))[0], np.eye(3))
    (sg, og), (sn, on) = follow(eng, given, st0), follow(eng, variants["negated"], st0)
    assert same_bits(sn, sg)
    for a, b, inp in zip(on, og, variants["negated"]):
        assert same_bits(a["root_states"][:B, 3:7], inp["quat"][:, [1, 2, 3, 0]])
        assert same_bits(a["root_states"][:B, 3:7], -b["root_states"][:B, 3:7])
        assert same_bits(np.delete(a["root_states"], [3, 4, 5, 6], 1), np.delete(b["root_states"], [3, 4, 5, 6], 1))
        assert same_bits(a["feet_world"], b["feet_world"])


@pytest.mark.parametrize("name", list(est_ref.D_REGIME))
def test_long_regimes(name):
    """g.  200 ticks of all trust 0, all trust 1, and zero process noise and suspicion: within
    10 d of est_ref's batch form with that regime's own d, P bitwise symmetric and finite,
    status 0 (follow)."""
    from mpcqp import LinearMpc
    eng = LinearMpc(horizon=10, robot="aliengo", device=DEV)      # its own: the constants are changed here
    traj, c = est_ref.regime_trajectory(B, 200, name)
    if c:
        eng.set_estimator(**dict(est_ref.DEFAULTS, **c))
    ref, ref_outs = est_ref.run(traj, c)
    states, outs = follow(eng, traj, ZERO)
    dx, dP = est_ref.worst_err(states, ref)
    f32 = f32_err(outs, ref_outs, B)
    print(f"\n{name} on the device: x {dx:.2e}, P {dP:.2e}, float32 outputs {f32:.2e}")
    bx, bP = (10 * d for d in est_ref.D_REGIME[name])
    assert dx <= bx and dP <= bP and f32 <= max(2.4e-7, bx)


@pytest.mark.parametrize("n", [2, 5, 6])
def test_batch_shapes(eng, start, n):
    """h.  B = 2 and 5 leave a robot slot of a workgroup idle, 6 fills two workgroups exactly."""
    traj = [first(t, n) for t in start[0][:10]]
    ref, ref_outs = est_ref.run(traj)
    states, outs = follow(eng, traj, np.zeros((n, est_ref.STRIDE)))
    dx, dP = est_ref.worst_err(states, ref)
    f32 = f32_err(outs, ref_outs, n)
    print(f"\nB = {n} on the device: x {dx:.2e}, P {dP:.2e}, float32 outputs {f32:.2e}")
    assert dx <= X_BOUND and dP <= P_BOUND and f32 <= F32_BOUND


def test_arguments(eng, start):
    """i.  Each required pointer NULL in turn, qdot NULL without the dof flag, est_state off
    16-byte alignment and a negative batch: MPCQP_ERR_ARG with a matching word in
    mpcqp_last_error, refused on the host -- the zeroed record they all point at stays zero.
    qdot NULL with the dof flag is accepted."""
    from mpcqp import _lib
    traj, _ = start
    d = Device(eng, B)
    t = {k: _dev(v, torch.float64 if k == "geom" else None) for k, v in traj[0].items()}
    dofs = _dev(kin_ref.dof_states(traj[0]["q"], traj[0]["qdot"]))
    ptr = lambda x: None if x is None else ctypes.c_void_p(x if isinstance(x, int) else x.data_ptr())

    def call(batch=B, flags=0, state=d.state, **kw):
        a = dict(t, **kw)
        return eng.lib.mpcqp_estimate(eng._ctx, batch, flags, ptr(a["quat"]), ptr(a["gyro"]), ptr(a["accel"]),
                                      ptr(a["q"]), ptr(a["qdot"]), ptr(a["trust"]), ptr(a["geom"]), ptr(state),
                                      ptr(d.full["root_states"]), ptr(d.full["feet_world"]), ptr(d.full["status"]), None)

    assert d.state.data_ptr() % 16 == 0
    refused = [(dict(**{k: None}), "null") for k in ("quat", "gyro", "accel", "q", "qdot", "trust", "geom")]
    refused += [(dict(state=d.state.data_ptr() + 8), "aligned"), (dict(batch=-4), "batch")]
    for kw, word in refused:
        assert call(**kw) == _lib.ERR_ARG, kw
        assert word in eng.lib.mpcqp_last_error(eng._ctx).decode(), kw
    torch.cuda.synchronize()
    assert (d.state[:B] == 0).all() and d.padding_untouched() and (d.full["status"] == int(SENTINEL)).all()
    assert call(flags=_lib.EST_DOF_STATES, q=dofs, qdot=None) == 0
    st, out = d.read()
    assert same((st, out), tick(eng, ZERO, traj[0], "dof"))

"""GPU: mpcqp_attitude -- one tick of every robot's orientation filter and the contact trust of
its feet in one launch -- against the float64 restatement tests/att_ref.py, the known answers
of tests/test_att.py on the device, independence of the robots, argument checks, the trust
against mpcqp_leg_torques' swing state, graph replay and BatchedEstimator.update_from_imu
feeding BatchedController.

Bounds (norm-wise per robot, max|a - a_ref| / max|a_ref|, the quaternion up to sign).  The
host build of csrc/mpcqp_attitude_robot.h differs from att_ref by d = 5.6e-16 in the record
(att_ref.D_Q; tests/test_att.py measures it): the problem's rounding sensitivity.  The device
runs the same text with its own sqrt, sin and cos, so the float64 record is held to 10 d --
Q_BOUND = 5.6e-15 -- and the float32 outputs to F32_BOUND = 2.4e-7, the two-ulp float32 floor of
tests/test_gpu_kin.py; the trust is bitwise att_ref's.  The known answers are held to the 1e-12
(1e-9 for the bias) of tests/test_att.py.
Measured on the MI355X (max over B = 1, 63, 64, 65, 131, with and without gait and touch,
each output absent in turn, 40 ticks, all robots): record 3.05e-16, quat 3.02e-08, gyro_out
bitwise the gyro (no bias estimate); with the bias estimate on (BIAS_ON) record 2.22e-16, quat
3.01e-08, gyro_out 5.74e-08.  Known answers: (a) tilt 2.78e-16, (b) closed-form exponential
1.01e-15, (d) bias 3.43e-16 and tilt 1.72e-17.  Closing the loop from raw sensors: root_states
against est_ref fed att_ref's quaternion and trust after 200 ticks 7.11e-09; the position
against update() on the true quaternion differs by 0 (a level robot's filtered quaternion is
the identity exactly).
"""
import numpy as np
import pytest

# torch first: it brings its own HIP runtime, which must be loaded before libmpcqp.so
# pulls in the system's (a CPU test file collected ahead of this one loads the library)
torch = pytest.importorskip("torch")

import att_ref  # noqa: E402
import est_ref  # noqa: E402
import kin_ref  # noqa: E402
from helpers import DEV, _dev  # noqa: E402

pytestmark = pytest.mark.gpu

Q_BOUND = 10 * att_ref.D_Q
F32_BOUND = 2.4e-7
KNOWN = 1e-12
SENTINEL = -77.0
W = 64                     # kAttThreads: robots per workgroup (csrc/mpcqp_attitude.h)
TICKS, BMAX = 40, 2 * W + 3
OUTS = ("quat", "gyro_out", "trust", "status")
ALL = ("tick", "gait", "ibm", "touch")
BIAS_ON = dict(kappa_ref=2.0, bias_gain=0.5)


def new_engine():
    from mpcqp import LinearMpc
    return LinearMpc(horizon=10, robot="a1", device=DEV)


@pytest.fixture(scope="module")
def eng():
    return new_engine()


@pytest.fixture(scope="module")
def traj():
    return att_ref.make_trajectory(BMAX, TICKS, seed=7)


@pytest.fixture(scope="module")
def oracles(traj):
    """att_ref over the generator's trajectory for BMAX robots, once per set of optional inputs
    (and once with the bias estimate on): robots are independent, so the first B robots are
    the oracle of a batch of B."""
    cache = {}

    def get(keys=ALL, constants=None):
        k = (tuple(keys), tuple(sorted((constants or {}).items())))
        if k not in cache:
            cache[k] = att_ref.run(traj, constants, keys=keys)
        return cache[k]
    return get


def first(inp, B):
    return {k: (v[:B] if isinstance(v, np.ndarray) else v) for k, v in inp.items()}


class Device:
    """The caller's buffers for B robots, each with `pad` extra rows of SENTINEL."""

    def __init__(self, eng, B, state=None, pad=2):
        self.eng, self.B = eng, B
        self.state = torch.full((B + pad, att_ref.STRIDE), SENTINEL, dtype=torch.float64, device=DEV)
        self.state[:B] = 0.0 if state is None else _dev(state)
        f = dict(dtype=torch.float32, device=DEV)
        self.full = dict(quat=torch.full((B + pad, 4), SENTINEL, **f), gyro_out=torch.full((B + pad, 3), SENTINEL, **f),
                         trust=torch.full((B + pad, 4), SENTINEL, **f),
                         status=torch.full((B + pad,), int(SENTINEL), dtype=torch.int32, device=DEV))

    def tick(self, inp, skip=(), stream=None):
        B = self.B
        outs = {k: (None if k in skip else v[:B]) for k, v in self.full.items()}
        if "gait" not in inp and "touch" not in inp:
            outs["trust"] = None
        kw = {k: _dev(inp[k]) for k in ("tick", "gait", "touch") if k in inp}
        self.eng.attitude(self.state[:B], _dev(inp["gyro"]), _dev(inp["accel"]), iterations_between_mpc=inp.get("ibm", 0),
                          stream=stream, **kw, **outs)

    def read(self):
        torch.cuda.synchronize()
        return self.state.cpu().numpy(), {k: v.cpu().numpy() for k, v in self.full.items()}

    def padding_untouched(self, skip=()):
        st, outs = self.read()
        ok = (st[self.B:] == SENTINEL).all() and all((v[self.B:] == int(SENTINEL)).all() for v in outs.values())
        return ok and all((outs[k] == int(SENTINEL)).all() for k in skip)


def follow(eng, traj, oracle, B, keys=ALL, skip=()):
    """TICKS ticks on the device, compared with the oracle after every one; the worst figures."""
    states, outs = oracle
    d = Device(eng, B)
    worst = dict(record=0.0, quat=0.0, gyro_out=0.0)
    no_trust = "gait" not in keys and "touch" not in keys
    for i in range(TICKS):
        d.tick(att_ref.select(first(traj[i], B), keys), skip)
        st, o = d.read()
        assert (st[:B, att_ref.INIT] == 1).all()
        for b in range(B):
            worst["record"] = max(worst["record"], att_ref.record_err(st[b], states[i + 1][b]))
            if "quat" not in skip:
                worst["quat"] = max(worst["quat"], att_ref.quat_err(o["quat"][b], outs[i]["quat"][b]))
            if "gyro_out" not in skip:
                worst["gyro_out"] = max(worst["gyro_out"], att_ref.norm_err(o["gyro_out"][b], outs[i]["gyro_out"][b]))
        if "trust" not in skip and not no_trust:
            assert np.array_equal(o["trust"][:B], outs[i]["trust"][:B].astype(np.float32)), i      # bitwise
        if "status" not in skip:
            assert (o["status"][:B] == 0).all()
    assert d.padding_untouched(tuple(skip) + (("trust",) if no_trust else ()))
    return worst


def check(worst, tag):
    print(f"\n{tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["record"] <= Q_BOUND, (tag, worst)
    assert worst["quat"] <= F32_BOUND and worst["gyro_out"] <= F32_BOUND, (tag, worst)


@pytest.mark.parametrize("B", [1, W - 1, W, W + 1, BMAX])
def test_parity(eng, traj, oracles, B):
    """B = 63, 64, 65 around one workgroup, 131 a third workgroup with a tail of three."""
    check(follow(eng, traj, oracles(), B), f"B={B}")


@pytest.mark.parametrize("keys", [("tick", "gait", "ibm"), ("touch",), ()])
def test_parity_with_optional_inputs_absent(eng, traj, oracles, keys):
    """Without the touch sensor, without the gait, and without both (then no trust is asked for
    and its buffer is not written)."""
    check(follow(eng, traj, oracles(keys), W + 1, keys), f"B={W + 1} inputs {keys}")


@pytest.mark.parametrize("skip", OUTS)
def test_parity_with_an_output_absent(eng, traj, oracles, skip):
    """Each nullable output NULL in turn: the record and the other outputs hold the same
    bounds, and the absent output's buffer is not written."""
    check(follow(eng, traj, oracles(), W + 1, skip=(skip,)), f"B={W + 1} without {skip}")


def test_parity_with_a_bias_estimate(traj, oracles):
    """The bias estimate on and a stronger correction: the record's bias words and
    gyro_out = w_b - b take part."""
    eng = new_engine()
    eng.set_attitude(**BIAS_ON)
    check(follow(eng, traj, oracles(constants=BIAS_ON), W + 1), f"B={W + 1} {BIAS_ON}")


def _known(k, B=3):
    eng = new_engine()
    eng.set_attitude(**k["constants"])
    d = Device(eng, B, state=k["state"])
    gyro, accel = _dev(k["gyro"]), _dev(k["accel"])
    for _ in range(k["ticks"]):
        eng.attitude(d.state[:B], gyro, accel, quat=d.full["quat"][:B], status=d.full["status"][:B])
    st, o = d.read()
    assert (o["status"][:B] == 0).all()
    return st[:B], o


def test_known_answer_tilt_convergence():
    """tests/test_att.py (a) on the device, B = 3."""
    k = att_ref.known_tilt(3)
    st, o = _known(k)
    a = k["accel"][0].astype(np.float64)
    err = np.abs(att_ref.up(st[:, att_ref.Q]) - a / np.linalg.norm(a)).max()
    print(f"\n(a) tilt convergence on the device: {err:.2e}")
    assert err < KNOWN
    assert max(att_ref.norm_err(o["quat"][b], st[b, att_ref.Q]) for b in range(3)) <= F32_BOUND


def test_known_answer_gyro_only():
    """tests/test_att.py (b) on the device, B = 3: the closed-form exponential, and bitwise the
    same record with kappa_ref = 0."""
    k = att_ref.known_gyro_only(3)
    st, _ = _known(k)
    err = max(att_ref.quat_err(st[b, att_ref.Q], k["answer"]) for b in range(3))
    print(f"\n(b) gyro only on the device: {err:.2e}")
    assert err < KNOWN
    off, _ = _known(dict(k, constants=dict(k["constants"], kappa_ref=0.0)))
    assert np.array_equal(st, off)


def test_known_answer_bias():
    """tests/test_att.py (d) on the device, B = 3, 20 000 launches."""
    k = att_ref.known_bias(3)
    st, _ = _known(k)
    eb = np.abs(st[:, att_ref.BIAS] - k["answer"]).max()
    tilt = np.abs(att_ref.up(st[:, att_ref.Q]) - [0, 0, 1]).max()
    print(f"\n(d) bias on the device: {eb:.2e}, tilt {tilt:.2e}")
    assert eb < 1e-9 and tilt < 1e-9


def test_robots_are_independent(eng, traj):
    """A permuted batch gives the permuted records and outputs, bitwise; a NaN in robot 1's
    gyro, accel, touch or record gives it status 4, leaves its record as it was and forms its
    outputs from it, a bad touch zeroes its trusts, and no other robot notices."""
    B, n = 5, 6
    rng = np.random.default_rng(0)
    perm = rng.permutation(B)
    a, b = Device(eng, B), Device(eng, B)
    for i in range(n):
        inp = first(traj[i], B)
        a.tick(inp)
        b.tick({k: (v[perm] if isinstance(v, np.ndarray) else v) for k, v in inp.items()})
    (sa, oa), (sb, ob) = a.read(), b.read()
    assert np.array_equal(sa[:B][perm], sb[:B])
    assert all(np.array_equal(oa[k][:B][perm], ob[k][:B]) for k in OUTS)

    clean = Device(eng, B, state=sa[:B])
    clean.tick(first(traj[n], B))
    sc, oc = clean.read()
    keep = [0, 2, 3, 4]
    for key in ("gyro", "accel", "touch", "record"):
        inp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in first(traj[n], B).items()}
        start = sa[:B].copy()
        if key == "record":
            start[1, 2] = np.inf
        else:
            inp[key][1, 0] = np.nan
        dirty = Device(eng, B, state=start)
        dirty.tick(inp)
        sd, od = dirty.read()
        ref_state, ref = att_ref.attitude_step(start, inp)
        assert od["status"][:B].tolist() == [0, 4, 0, 0, 0] and oc["status"][:B].tolist() == [0] * B, key
        assert np.array_equal(sd[1], start[1], equal_nan=True) and not np.array_equal(sc[1], sa[1])
        assert np.array_equal(sd[keep], sc[keep])
        assert all(np.array_equal(od[k][keep], oc[k][keep]) for k in OUTS), key
        assert np.array_equal(od["quat"][1], start[1, :4].astype(np.float32), equal_nan=True)      # the record as it was
        assert np.array_equal(od["gyro_out"][1], ref["gyro_out"][1].astype(np.float32), equal_nan=True)
        assert np.array_equal(od["trust"][1], ref["trust"][1].astype(np.float32))
        if key == "touch":
            assert (od["trust"][1] == 0).all()
        assert dirty.padding_untouched()
    # an all-zero record with a bad reading: identity out, still not initialised
    inp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in first(traj[0], B).items()}
    inp["accel"][1, 1] = np.inf
    fresh = Device(eng, B)
    fresh.tick(inp)
    sf, of = fresh.read()
    assert (sf[1] == 0).all() and of["quat"][1].tolist() == [1, 0, 0, 0] and of["status"][1] == 4
    assert np.array_equal(of["gyro_out"][1], inp["gyro"][1])


def test_argument_errors(traj):
    import ctypes

    from mpcqp import _lib
    eng = new_engine()                                       # its own: the constants are changed here
    B = 3
    d = Device(eng, B)
    inp = first(traj[0], B)
    t = {k: _dev(inp[k]) for k in ("gyro", "accel", "tick", "gait", "touch")}
    out = {k: v[:B] for k, v in d.full.items()}
    odd = torch.zeros((B * 8 + 1,), dtype=torch.float64, device=DEV)[1:]
    ptr = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())

    def call(batch=B, flags=0, ibm=20, state=d.state, **kw):
        a = dict(t, **out)
        a.update(kw)
        return eng.lib.mpcqp_attitude(eng._ctx, batch, flags, ptr(a["gyro"]), ptr(a["accel"]), ptr(a["tick"]), ibm,
                                      ptr(a["gait"]), ptr(a["touch"]), ptr(state), ptr(a["quat"]), ptr(a["gyro_out"]),
                                      ptr(a["trust"]), ptr(a["status"]), None)

    for kw, word in ((dict(flags=1), "flags"), (dict(flags=2), "flags"), (dict(batch=0), "batch"), (dict(batch=-4), "batch"),
                     (dict(gyro=None), "null"), (dict(accel=None), "null"), (dict(state=None), "null"),
                     (dict(state=odd), "aligned"), (dict(gait=None, tick=None, touch=None), "trust"),
                     (dict(tick=None), "tick"), (dict(ibm=0), "iterations_between_mpc")):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert word in eng.lib.mpcqp_last_error(eng._ctx).decode(), (kw, eng.lib.mpcqp_last_error(eng._ctx))
    assert call(gait=None, tick=None, ibm=0) == 0            # touch alone serves the trust; ibm is not looked at
    with pytest.raises(_lib.MpcqpError, match="batch"):
        eng.attitude(d.state[:0], t["gyro"], t["accel"])
    torch.cuda.synchronize()
    st, o = d.read()
    assert (st[:B, :4] != 0).any() and (o["status"][:B] == 0).all()      # the one good call ran ...
    d2 = Device(eng, B)
    for kw in (dict(flags=1), dict(batch=0), dict(state=None), dict(ibm=0)):
        call(**dict(dict(state=d2.state), **kw))
    assert (d2.read()[0][:B] == 0).all()                     # ... and a refused one runs nothing

    mine = dict(dt=0.002, gravity=9.0, kappa_ref=3.0, bias_gain=2.0, trust_window=0.35, touch_threshold=0.5)
    eng.set_attitude(**mine)
    for bad in (dict(dt=0.0), dict(dt=-1.0), dict(gravity=0.0), dict(kappa_ref=-0.1), dict(bias_gain=-1.0),
                dict(trust_window=-0.1), dict(trust_window=0.6), dict(touch_threshold=float("nan")),
                dict(kappa_ref=float("inf")), dict(dt=float("nan"))):
        with pytest.raises(_lib.MpcqpError, match="attitude"):
            eng.set_attitude(**dict(mine, **bad))
    assert eng.attitude_constants == mine
    start = att_ref.run(traj[:2])[0][-1][:B]
    inp = dict(first(traj[2], B), touch=np.tile(np.float32([0.3, 1.0, 1.0, 0.3]), (B, 1)))
    d = Device(eng, B, state=start)
    d.tick(inp)
    st, o = d.read()
    ref, ro = att_ref.attitude_step(start, inp, mine)
    dflt, do = att_ref.attitude_step(start, inp)
    assert max(att_ref.record_err(st[b], ref[b]) for b in range(B)) <= Q_BOUND
    assert np.array_equal(o["trust"][:B], ro["trust"].astype(np.float32))
    assert max(att_ref.record_err(st[b], dflt[b]) for b in range(B)) > 1e6 * Q_BOUND     # the constants do matter here
    assert not np.array_equal(ro["trust"], do["trust"])


def test_trust_against_the_leg_controller():
    """trust == 0 exactly where mpcqp_leg_torques reports swing_state > 0, for the same ticks
    and gait: B = 4, one TROTTING10 period at iterations_between_mpc = 20 (200 ticks)."""
    from mpcqp.controller import BatchedController
    B = 4
    ctl = BatchedController(B, horizon=10, robot="a1", gait="TROTTING10")
    inp = est_ref.level_crouch(B, "a1")
    dofs = _dev(kin_ref.dof_states(inp["q"], inp["qdot"]))
    rs = torch.zeros((B, 13), device=DEV)
    rs[:, 2], rs[:, 6] = 0.28, 1.0
    ctl.kinematics(rs, dofs)
    state = torch.zeros((B, att_ref.STRIDE), dtype=torch.float64, device=DEV)
    gyro, accel = _dev(inp["gyro"]), _dev(inp["accel"])
    trust = torch.zeros((B, 4), device=DEV)
    swing, trusts = [], []
    for it in range(200):
        ctl.leg_torques(it, [0.5, 0.0, 0.0], 0.0, ctl.thighs, ctl.pos_feet, ctl.foot_pos_base, ctl.foot_vel_base,
                        ctl.jac, root_states=rs)
        ctl.engine.attitude(state, gyro, accel, tick=ctl.tick_count, iterations_between_mpc=ctl.iterations_between_mpc,
                            gait=ctl.gait, trust=trust)
        swing.append(ctl.swing_state.clone())
        trusts.append(trust.clone())
    torch.cuda.synchronize()
    swing, trusts = torch.stack(swing).cpu().numpy(), torch.stack(trusts).cpu().numpy()
    assert np.array_equal(trusts == 0, swing > 0)
    assert (swing > 0).any() and (trusts == 1).any() and ((trusts > 0) & (trusts < 1)).any()
    want = att_ref.gait_trust(np.arange(200), 20, att_ref.gait_records([att_ref.TROTTING10] * 200), 0.2)
    assert np.array_equal(trusts[:, 0], want.astype(np.float32))


def test_graph_replay_advances_the_filter(eng):
    """One launch for B = 64 captured on a side stream after one eager call; three replays
    with the inputs rewritten in place equal three eager ticks bitwise."""
    B, reps = 64, 3
    traj = att_ref.make_trajectory(B, reps + 1, seed=21)
    keys = ("gyro", "accel", "touch", "tick")
    gait = _dev(traj[0]["gait"])
    names = ("state", "quat", "gyro_out", "trust", "status")

    def buffers():
        f = dict(dtype=torch.float32, device=DEV)
        return dict(state=torch.zeros((B, att_ref.STRIDE), dtype=torch.float64, device=DEV),
                    quat=torch.zeros((B, 4), **f), gyro_out=torch.zeros((B, 3), **f), trust=torch.zeros((B, 4), **f),
                    status=torch.zeros((B,), dtype=torch.int32, device=DEV), **{k: _dev(traj[0][k]) for k in keys})

    def launch(bf, stream=None):
        eng.attitude(bf["state"], bf["gyro"], bf["accel"], tick=bf["tick"], iterations_between_mpc=1, gait=gait,
                     touch=bf["touch"], quat=bf["quat"], gyro_out=bf["gyro_out"], trust=bf["trust"],
                     status=bf["status"], stream=stream)

    def load(bf, i):
        for k in keys:
            bf[k].copy_(_dev(traj[i][k]))

    eager, seen = buffers(), []
    launch(eager)                                             # tick 0, eager in both runs
    for i in range(1, reps + 1):
        load(eager, i)
        launch(eager)
        seen.append({k: eager[k].clone() for k in names})
    torch.cuda.synchronize()
    bf = buffers()
    launch(bf)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch(bf, stream=s)
    for i in range(1, reps + 1):
        load(bf, i)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(bf[k], seen[i - 1][k]) for k in names), i
    assert (bf["status"] == 0).all()
    assert len({x["state"].cpu().numpy().tobytes() for x in seen}) == reps      # the ticks did advance the filter
    assert len({x["trust"].cpu().numpy().tobytes() for x in seen}) > 1


def test_update_from_imu_closes_the_loop():
    """BatchedEstimator.update_from_imu on the controller's engine and gait: 200 ticks of the
    level-crouch sensors with the quaternion and the trust withheld, against est_ref fed
    att_ref's quaternion and trust; then ctl.step on the estimated root state; and a second
    estimator given the true quaternion through update() lands on the same position."""
    from mpcqp.controller import BatchedController
    from mpcqp.estimator import BatchedEstimator
    B, T = 4, 200
    ctl = BatchedController(B, robot="a1", gait="TROTTING10")
    est = BatchedEstimator(B, robot="a1", controller=ctl)
    told = BatchedEstimator(B, robot="a1", engine=ctl.engine)
    assert est.engine is ctl.engine and est.gait is ctl.gait and est.iterations_between_mpc == 20
    assert ctl.engine.attitude_constants == att_ref.DEFAULTS
    inp = est_ref.level_crouch(B, "a1")
    dofs = _dev(kin_ref.dof_states(inp["q"], inp["qdot"]))
    gyro, accel, quat_true = (_dev(inp[k]) for k in ("gyro", "accel", "quat"))
    for i in range(T):
        root = est.update_from_imu(gyro, accel, dofs, tick=i)
        told.update(quat_true, gyro, accel, dofs, est.trust)
    assert root is est.root_states
    one = {k: v[:1] for k, v in inp.items()}
    gait = att_ref.gait_records([att_ref.TROTTING10])
    att_state, ref_state = np.zeros((1, att_ref.STRIDE)), np.zeros((1, est_ref.STRIDE))
    for i in range(T):
        att_state, ao = att_ref.attitude_step(att_state, dict(gyro=one["gyro"], accel=one["accel"], tick=np.array([i]),
                                                              gait=gait, ibm=20))
        fed = dict(one, quat=ao["quat"].astype(np.float32), gyro=ao["gyro_out"].astype(np.float32),
                   trust=ao["trust"].astype(np.float32))
        ref_state, ref_out = est_ref.estimate_step(ref_state, fed)
    torch.cuda.synchronize()
    got = root.cpu().numpy()
    err = max(est_ref.norm_err(got[b], ref_out["root_states"][0]) for b in range(B))
    apart = float((est.position - told.position).abs().max())
    print(f"\nclosing the loop from raw sensors: root_states vs est_ref {err:.2e}, z {got[0, 2]:.6f}, "
          f"position against update(quat_true) {apart:.2e} m")
    assert err <= max(2.4e-7, 10 * est_ref.D_X) and (est.status == 0).all() and (est.attitude_status == 0).all()
    assert np.array_equal(est.trust.cpu().numpy()[0], ao["trust"][0].astype(np.float32))
    assert apart < 1e-5
    tau = ctl.step(T, [0.5, 0.0, 0.0], 0.0, root, dofs)
    torch.cuda.synchronize()
    assert torch.isfinite(tau).all() and (ctl.status == 0).all()

    # an explicit trust bypasses the computed one; touch alone serves too; reset zeroes and seeds
    ones = torch.ones((B, 4), device=DEV)
    est.trust.fill_(SENTINEL)
    est.update_from_imu(gyro, accel, dofs, tick=3, trust=ones)
    assert (est.trust == SENTINEL).all()
    est.update_from_imu(gyro, accel, dofs, touch=ones)
    assert (est.trust == 1).all()
    with pytest.raises(ValueError, match="trust"):
        told.update_from_imu(gyro, accel, dofs)
    # the tick as a device tensor, and gait / iterations_between_mpc given to the call, serve alike
    est.update_from_imu(gyro, accel, dofs, tick=59)
    by_int = est.trust.clone()
    est.update_from_imu(gyro, accel, dofs, tick=torch.full((B,), 59, dtype=torch.int32, device=DEV))
    told.update_from_imu(gyro, accel, dofs, tick=59, gait="TROTTING10", iterations_between_mpc=20)
    assert torch.equal(est.trust, by_int) and torch.equal(told.trust, by_int)
    assert by_int[0].tolist() == [1.0, 0.0, 0.0, 1.0]
    with pytest.raises(ValueError, match="iterations_between_mpc"):
        told.update_from_imu(gyro, accel, dofs, tick=59, gait="TROTTING10")
    est.reset()
    assert (est.att_state == 0).all() and (est.est_state == 0).all()
    est.reset(robots=[1], quat=[2.0, 0.0, 0.0, 2.0])
    torch.cuda.synchronize()
    rec = est.att_state.cpu().numpy()
    assert np.allclose(rec[1], [np.sqrt(0.5), 0, 0, np.sqrt(0.5), 1, 0, 0, 0]) and (rec[[0, 2, 3]] == 0).all()
    est.update_from_imu(gyro, accel, dofs, tick=0)
    torch.cuda.synchronize()
    q = est.quat.cpu().numpy()
    assert abs(q[1, 3] - np.sqrt(0.5)) < 1e-3 and q[0].tolist() == [1, 0, 0, 0]      # the seeded yaw is kept

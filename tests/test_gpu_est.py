"""GPU: mpcqp_estimate -- one tick of every robot's IMU + leg-kinematics Kalman filter in
one launch -- against the float64 restatement tests/est_ref.py (batch form through
numpy.linalg.solve), the known answers of tests/test_est.py on the device, independence of
the robots, argument checks, graph replay and BatchedEstimator feeding BatchedController.

Bounds (norm-wise per robot, max|a - a_ref| / max|a_ref|, as kin_ref.norm_err).  est_ref's two
forms differ by d = 1.94e-11 in x and 4.8e-15 in P (est_ref.D_X, D_P; tests/test_est.py
measures them): the problem's rounding sensitivity.  The device runs the sequential form in
another summation order, so the float64 record is held to 10 d -- X_BOUND = 1.94e-10,
P_BOUND = 4.8e-14 -- and the float32 outputs to max(2.4e-7, 10 d) = F32_BOUND = 2.4e-7, the
two-ulp float32 floor of tests/test_gpu_kin.py.  The known answers are held to 1e-5 m.
Measured on the MI355X (max over B = 1, 3, 4, 7, both joint layouts, each output absent in
turn, 40 ticks, all robots): x 2.09e-12, P 1.78e-15 -- to the digit what the kernel gives on
host threads in tests/test_est.py -- root_states 3.58e-08, feet_world 5.51e-08 (the float32
store, under half an ulp norm-wise).  Known answers: level crouch z 3.99e-09, xy 6.5e-17,
v 2.08e-08, foot z 6.5e-11; tilted on one foot z 7.86e-10, foot z 2.61e-10, v 2.60e-08, feet
5.26e-10.  Closing the loop: root_states against est_ref after 200 ticks 1.60e-09.
"""
import numpy as np
import pytest

# torch first: it brings its own HIP runtime, which must be loaded before libmpcqp.so
# pulls in the system's (a CPU test file collected ahead of this one loads the library)
torch = pytest.importorskip("torch")

import est_ref  # noqa: E402
import kin_ref  # noqa: E402
from est_ref import norm_err  # noqa: E402
from helpers import DEV, _dev  # noqa: E402

pytestmark = pytest.mark.gpu

X_BOUND, P_BOUND = 10 * est_ref.D_X, 10 * est_ref.D_P
F32_BOUND = max(2.4e-7, 10 * est_ref.D_X)
KNOWN = 1e-5
SENTINEL = -77.0
G = 3                      # kEstRobots: robots per workgroup (csrc/mpcqp_estimator.h)
TICKS, BMAX = 40, 2 * G + 1
OUTS = ("root_states", "feet_world", "status")


@pytest.fixture(scope="module")
def eng():
    from mpcqp import LinearMpc
    return LinearMpc(horizon=10, robot="aliengo", device=DEV)


@pytest.fixture(scope="module")
def oracle():
    """The generator's trajectory for BMAX robots and est_ref's batch form over it, once:
    robots are independent, so the first B robots are the oracle of a batch of B."""
    traj = est_ref.make_trajectory(BMAX, TICKS, seed=7)
    states, outs = est_ref.run(traj, form="batch")
    return traj, states, outs


def first(inp, B):
    return {k: v[:B] for k, v in inp.items()}


class Device:
    """The caller's buffers for B robots, each with `pad` extra rows of SENTINEL."""

    def __init__(self, eng, B, state=None, pad=2):
        self.eng, self.B = eng, B
        self.state = torch.full((B + pad, est_ref.STRIDE), SENTINEL, dtype=torch.float64, device=DEV)
        self.state[:B] = 0.0 if state is None else _dev(state)
        self.full = dict(root_states=torch.full((B + pad, 13), SENTINEL, dtype=torch.float32, device=DEV),
                         feet_world=torch.full((B + pad, 4, 3), SENTINEL, dtype=torch.float32, device=DEV),
                         status=torch.full((B + pad,), int(SENTINEL), dtype=torch.int32, device=DEV))

    def tick(self, inp, layout="split", skip=(), stream=None):
        B = self.B
        outs = {k: (None if k in skip else v[:B]) for k, v in self.full.items()}
        joints = dict(dof_states=_dev(kin_ref.dof_states(inp["q"], inp["qdot"]))) if layout == "dof" else \
            dict(q=_dev(inp["q"]), qdot=_dev(inp["qdot"]))
        self.eng.estimate(self.state[:B], _dev(inp["quat"]), _dev(inp["gyro"]), _dev(inp["accel"]), _dev(inp["trust"]),
                          _dev(inp["geom"], torch.float64), stream=stream, **joints, **outs)

    def read(self):
        torch.cuda.synchronize()
        return self.state.cpu().numpy(), {k: v.cpu().numpy() for k, v in self.full.items()}

    def padding_untouched(self, skip=()):
        st, outs = self.read()
        ok = (st[self.B:] == SENTINEL).all() and all((v[self.B:] == int(SENTINEL)).all() for v in outs.values())
        return ok and all((outs[k] == int(SENTINEL)).all() for k in skip)


def follow(eng, oracle, B, layout, skip=()):
    """TICKS ticks on the device, compared with the oracle after every one; the worst figures."""
    traj, states, outs = oracle
    d = Device(eng, B)
    worst = dict(x=0.0, P=0.0, root_states=0.0, feet_world=0.0)
    for i in range(TICKS):
        d.tick(first(traj[i], B), layout, skip)
        st, o = d.read()
        x, P, init = est_ref.unpack(st[:B])
        xr, Pr, _ = est_ref.unpack(states[i + 1][:B])
        assert (init == 1).all() and (st[:B, 19:24] == 0).all() and (st[:B, 348:] == 0).all()
        for b in range(B):
            worst["x"] = max(worst["x"], norm_err(x[b], xr[b]))
            worst["P"] = max(worst["P"], norm_err(P[b], Pr[b]))
            for k in ("root_states", "feet_world"):
                if k not in skip:
                    worst[k] = max(worst[k], norm_err(o[k][b], outs[i][k][b]))
        if "status" not in skip:
            assert (o["status"][:B] == 0).all()
    assert d.padding_untouched(skip)
    return worst


def check(worst, tag):
    print(f"\n{tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["x"] <= X_BOUND and worst["P"] <= P_BOUND, (tag, worst)
    assert worst["root_states"] <= F32_BOUND and worst["feet_world"] <= F32_BOUND, (tag, worst)


@pytest.mark.parametrize("B", [1, 3, G + 1, BMAX])
@pytest.mark.parametrize("layout", ["split", "dof"])
def test_parity(eng, oracle, B, layout):
    """B = 3 fills a workgroup's robot slots, 4 starts a second workgroup, 7 a third with a
    tail; both joint layouts."""
    check(follow(eng, oracle, B, layout), f"B={B} {layout}")


@pytest.mark.parametrize("skip", OUTS)
@pytest.mark.parametrize("layout", ["split", "dof"])
def test_parity_with_an_output_absent(eng, oracle, layout, skip):
    """Each nullable output NULL in turn: the record and the other outputs hold the same
    bounds, and the absent output's buffer is not written."""
    check(follow(eng, oracle, G + 1, layout, skip=(skip,)), f"B={G + 1} {layout} without {skip}")


def test_known_answer_level_crouch(eng):
    """tests/test_est.py (a) on the device, B = 3 (Aliengo, l = 0.25)."""
    d = Device(eng, 3)
    inp = est_ref.level_crouch(3, "aliengo")
    dev_inp = {k: _dev(v, torch.float64 if k == "geom" else None) for k, v in inp.items()}
    for _ in range(2000):
        eng.estimate(d.state[:3], dev_inp["quat"], dev_inp["gyro"], dev_inp["accel"], dev_inp["trust"],
                     dev_inp["geom"], q=dev_inp["q"], qdot=dev_inp["qdot"], **{k: v[:3] for k, v in d.full.items()})
    st, o = d.read()
    x = est_ref.unpack(st[:3])[0]
    errs = dict(z=np.abs(x[:, 2] - 2 * 0.25 * np.cos(0.8)).max(), xy=np.abs(x[:, 0:2]).max(),
                v=np.abs(x[:, 3:6]).max(), foot_z=np.abs(x[:, 8::3]).max())
    print("\nlevel crouch on the device: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < KNOWN
    assert np.abs(o["root_states"][:3, 2] - 2 * 0.25 * np.cos(0.8)).max() < KNOWN and (o["status"][:3] == 0).all()


def test_known_answer_tilted_one_foot(eng):
    """tests/test_est.py (b) on the device, B = 3."""
    foot = 2
    d = Device(eng, 3)
    inp = est_ref.tilted_one_foot(3, foot=foot, robot="a1")
    dev_inp = {k: _dev(v, torch.float64 if k == "geom" else None) for k, v in inp.items()}
    for _ in range(3000):
        eng.estimate(d.state[:3], dev_inp["quat"], dev_inp["gyro"], dev_inp["accel"], dev_inp["trust"],
                     dev_inp["geom"], q=dev_inp["q"], qdot=dev_inp["qdot"], **{k: v[:3] for k, v in d.full.items()})
    st, _ = d.read()
    x = est_ref.unpack(st[:3])[0]
    r = np.einsum("brc,blc->blr", kin_ref.quat2matrix_eigen(inp["quat"]), kin_ref.chain(inp["geom"], inp["q"])[0])
    errs = dict(z=np.abs(x[:, 2] + r[:, foot, 2]).max(), foot_z=np.abs(x[:, 8 + 3 * foot]).max(),
                v=np.abs(x[:, 3:6]).max(), feet=np.abs(x[:, 6:].reshape(3, 4, 3) - x[:, None, 0:3] - r).max())
    print("\ntilted, one foot on the device: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < KNOWN


def test_robots_are_independent(eng, oracle):
    """A permuted batch gives the permuted records and outputs, bitwise; a NaN in robot 1's
    accel gives it status 4 and leaves its record as it was, and no other robot notices."""
    traj = oracle[0]
    B, n = G + 1, 6
    perm = np.array([2, 0, 3, 1])
    a, b = Device(eng, B), Device(eng, B)
    for i in range(n):
        inp = first(traj[i], B)
        a.tick(inp)
        b.tick({k: v[perm] for k, v in inp.items()})
    (sa, oa), (sb, ob) = a.read(), b.read()
    assert np.array_equal(sa[:B][perm], sb[:B])
    assert all(np.array_equal(oa[k][:B][perm], ob[k][:B]) for k in OUTS)

    inp = {k: v.copy() for k, v in first(traj[n], B).items()}
    clean = Device(eng, B, state=sa[:B])
    clean.tick(inp)
    inp["accel"][1, 2] = np.nan
    dirty = Device(eng, B, state=sa[:B])
    dirty.tick(inp)
    (sc, oc), (sd, od) = clean.read(), dirty.read()
    assert od["status"][:B].tolist() == [0, 4, 0, 0] and oc["status"][:B].tolist() == [0, 0, 0, 0]
    assert np.array_equal(sd[1], sa[1]) and not np.array_equal(sc[1], sa[1])
    keep = [0, 2, 3]
    assert np.array_equal(sd[keep], sc[keep])
    assert all(np.array_equal(od[k][keep], oc[k][keep]) for k in OUTS)
    assert np.array_equal(od["root_states"][1, 0:3], sa[1, 0:3].astype(np.float32))     # the state as it was
    assert np.array_equal(od["feet_world"][1].ravel(), sa[1, 6:18].astype(np.float32))
    assert dirty.padding_untouched()


def test_argument_errors(oracle):
    import ctypes

    from mpcqp import LinearMpc, _lib
    eng = LinearMpc(horizon=10, robot="a1", device=DEV)      # its own: the constants are changed here
    traj = oracle[0]
    B = 3
    d = Device(eng, B)
    inp = first(traj[0], B)
    t = {k: _dev(v, torch.float64 if k == "geom" else None) for k, v in inp.items()}
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())

    def call(batch=B, flags=0, state=d.state):
        return eng.lib.mpcqp_estimate(eng._ctx, batch, flags, ptr(t["quat"]), ptr(t["gyro"]), ptr(t["accel"]),
                                      ptr(t["q"]), ptr(t["qdot"]), ptr(t["trust"]), ptr(t["geom"]),
                                      ptr(state) if state is not None else None, None, None, None, None)

    for kw, word in ((dict(flags=2), "flags"), (dict(flags=5), "flags"), (dict(batch=0), "batch"),
                     (dict(state=None), "null")):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert word in eng.lib.mpcqp_last_error(eng._ctx).decode(), kw
    with pytest.raises(_lib.MpcqpError, match="batch"):
        eng.estimate(d.state[:0], t["quat"], t["gyro"], t["accel"], t["trust"], t["geom"], q=t["q"], qdot=t["qdot"])
    torch.cuda.synchronize()
    assert (d.state[:B] == 0).all()                          # nothing ran

    mine = dict(r_p=0.002, suspicion=50.0, sigma_f=0.004, contact_height=0.01)
    eng.set_estimator(**mine)
    for bad in (dict(r_z=0.0), dict(r_v=float("nan")), dict(dt=0.0), dict(p0=-1.0), dict(sigma_v=-1e-3),
                dict(suspicion=-1.0), dict(gravity=float("inf"))):
        with pytest.raises(_lib.MpcqpError, match="estimator"):
            eng.set_estimator(**dict(mine, **bad))
    assert eng.estimator_constants == dict(est_ref.DEFAULTS, **mine)
    d.tick(inp)
    st, o = d.read()
    ref, _ = est_ref.estimate_step(np.zeros((B, est_ref.STRIDE)), inp, mine)
    dflt, _ = est_ref.estimate_step(np.zeros((B, est_ref.STRIDE)), inp)
    for b in range(B):
        x, P, _ = est_ref.unpack(st[b:b + 1])
        xr, Pr, _ = est_ref.unpack(ref[b:b + 1])
        assert norm_err(x, xr) <= X_BOUND and norm_err(P, Pr) <= P_BOUND
        assert norm_err(est_ref.unpack(dflt[b:b + 1])[1], Pr) > 1e6 * P_BOUND      # the constants do matter here


def test_graph_replay_advances_the_filter(eng, oracle):
    """One estimate for B = 64 captured on a side stream after one eager call; three
    replays with the inputs rewritten in place leave the record bitwise equal to three
    eager ticks."""
    B, reps = 64, 3
    traj = est_ref.make_trajectory(B, reps + 1, seed=21)
    keys = ("quat", "gyro", "accel", "q", "qdot", "trust")
    geom = _dev(traj[0]["geom"], torch.float64)

    def buffers():
        return dict(state=torch.zeros((B, est_ref.STRIDE), dtype=torch.float64, device=DEV),
                    root=torch.zeros((B, 13), device=DEV), feet=torch.zeros((B, 4, 3), device=DEV),
                    status=torch.zeros((B,), dtype=torch.int32, device=DEV),
                    **{k: _dev(traj[0][k]) for k in keys})

    def launch(bf, stream=None):
        eng.estimate(bf["state"], bf["quat"], bf["gyro"], bf["accel"], bf["trust"], geom, q=bf["q"], qdot=bf["qdot"],
                     root_states=bf["root"], feet_world=bf["feet"], status=bf["status"], stream=stream)

    def load(bf, i):
        for k in keys:
            bf[k].copy_(_dev(traj[i][k]))

    eager, roots = buffers(), []
    launch(eager)                                             # tick 0, eager in both runs
    for i in range(1, reps + 1):
        load(eager, i)
        launch(eager)
        roots.append(eager["root"].clone())
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
        assert torch.equal(bf["root"], roots[i - 1]), i
    assert torch.equal(bf["state"], eager["state"]) and torch.equal(bf["feet"], eager["feet"])
    assert (bf["status"] == 0).all()
    assert len({r.cpu().numpy().tobytes() for r in roots}) == reps      # the ticks did advance the filter


def test_estimator_closes_the_loop():
    """BatchedEstimator on the controller's engine: 200 ticks of the level-crouch sensors,
    then ctl.step on the estimated root state."""
    from mpcqp.controller import BatchedController
    from mpcqp.estimator import BatchedEstimator
    B = 4
    ctl = BatchedController(B, robot="a1", gait="TROTTING10")
    est = BatchedEstimator(B, robot="a1", engine=ctl.engine)
    assert est.engine is ctl.engine
    inp = est_ref.level_crouch(B, "a1")
    dofs = _dev(kin_ref.dof_states(inp["q"], inp["qdot"]))
    quat, gyro, accel, trust = (_dev(inp[k]) for k in ("quat", "gyro", "accel", "trust"))
    for _ in range(200):
        root = est.update(quat, gyro, accel, dofs, trust)
    assert root is est.root_states
    ref_state = np.zeros((1, est_ref.STRIDE))
    one = first(inp, 1)
    for _ in range(200):
        ref_state, ref_out = est_ref.estimate_step(ref_state, one)
    torch.cuda.synchronize()
    got = root.cpu().numpy()
    err = max(norm_err(got[b], ref_out["root_states"][0]) for b in range(B))
    hx, hy, dd, l1, l2 = est_ref.GEOMETRY["a1"]
    height = l1 * np.cos(np.float32(0.8)) + l2 * np.cos(np.float32(0.8))
    print(f"\nclosing the loop: root_states vs est_ref {err:.2e}, z {got[0, 2]:.6f} (crouch {height:.6f})")
    assert err <= F32_BOUND and (est.status == 0).all()
    assert norm_err(est.position.cpu().numpy()[0], ref_state[0, 0:3]) <= X_BOUND
    assert est.covariance.shape == (B, 18, 18) and est.velocity.shape == (B, 3)

    tau = ctl.step(20, [0.5, 0.0, 0.0], 0.0, est.root_states, dofs)
    torch.cuda.synchronize()
    assert torch.isfinite(tau).all() and (ctl.status == 0).all()
    truth = torch.zeros((B, 13), device=DEV)
    truth[:, 2], truth[:, 6] = float(height), 1.0
    ctl2 = BatchedController(B, robot="a1", gait="TROTTING10")
    tau2 = ctl2.step(20, [0.5, 0.0, 0.0], 0.0, truth, dofs)
    torch.cuda.synchronize()
    feet, feet2 = ctl.feet.cpu().numpy(), ctl2.feet.cpu().numpy()
    assert max(norm_err(feet[b], feet2[b]) for b in range(B)) <= F32_BOUND
    pf, pf2 = ctl.pos_feet.cpu().numpy(), ctl2.pos_feet.cpu().numpy()
    assert np.abs(pf - pf2).max() < KNOWN                    # the feet stand where the truth has them
    assert torch.isfinite(tau2).all() and float((tau - tau2).abs().max()) < 1e-2 * float(tau2.abs().max())

    est.reset(robots=[1], pos=[0.3, -0.2, float(height)])
    est.update(quat, gyro, accel, dofs, trust)
    torch.cuda.synchronize()
    p = est.position.cpu().numpy()
    assert np.abs(p[1] - [0.3, -0.2, height]).max() < 1e-3 and np.abs(p[0, 0:2]).max() < KNOWN

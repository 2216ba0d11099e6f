"""GPU: mpcqp_sensors / BatchedSensors and mpcqp_push / BatchedPlant.push against the restatement
tests/disturb_ref.py, their determinism, their edges and misuse, and the loop
plant -> sensors -> estimator -> step_fused -> plant closed on the device.

Bounds.  The generator and the touch path are integers: histories, count, touch_m and status are
compared bit by bit.  The float32 outputs must be equal, except that at most 1 word in 10^4 may
differ by exactly one float32 ulp (one q_lsb for a quantised q); the bias words are held to
BIAS_BOUND, relative to the robot's own s walk sqrt(dt T), which must lie below 1e-12 -- above
that a difference is a wrong draw, not rounding.  The push is held to the plant's record bound,
7.3e-15.

Measured on the MI355X.  With the device library's log, sin and cos (the first build) every
integer and every float32 word agreed, but one turn-on bias in a few hundred was one ulp off:
5.6e-17 at worst, 6.2e-13 of s walk sqrt(dt T), which times four is above 1e-12.  With log, sin
and cos spelled out in IEEE operations (csrc/mpcqp_sensors_robot.h sense_log, sense_sincos_turn;
the restatement does the same operations) the worst bias difference is 0 at every size and in
both configurations and no float32 word differs (0 of 780 000 at B = 130): BIAS_BOUND = 4 x 0.
The push: 4.6e-17 at B = 5, 4.4e-16 at B = 130.  The closed loop's figures stand with its test.
"""
import ctypes

import numpy as np
import pytest

# torch first: it brings its own HIP runtime, which must be loaded before libmpcqp.so
torch = pytest.importorskip("torch")

import disturb_ref as dr  # noqa: E402
import kin_ref  # noqa: E402
import plant_ref as pr  # noqa: E402
from helpers import DEV, _dev  # noqa: E402

pytestmark = pytest.mark.gpu

N = 10
T = 200
SIZES = (1, 3, 4, 5, 63, 64, 65, 130)
# |device - restatement| of a bias word over s walk sqrt(dt T): four times the worst seen on the
# MI355X, which is 0 (the module docstring); it must lie below BIAS_LIMIT
BIAS_BOUND = 0.0
BIAS_LIMIT = 1e-12
PUSH_BOUND = 7.3e-15
CONFIGS = (dict(dr.MEMS, sigma_q=1e-3, touch_lag=2, p_drop=0.25),
           dict(dr.MEMS, sigma_q=1e-3, q_lsb=0.0, touch_lag=0, p_drop=0.0))


P_LSB = np.float32(CONFIGS[0]["q_lsb"] * 1.0001)


def _bits(t):
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def inputs(B, ticks, seed):
    """[ticks] plant-like inputs: gyro, accel [B,3], dofs [B,12,2], touch [B,4] (0 / 1), float32."""
    rng = np.random.default_rng(seed)
    f4 = np.float32
    touch = (rng.random((ticks, B, 4)) < 0.6).astype(f4)
    return dict(gyro=rng.normal(0, 0.3, (ticks, B, 3)).astype(f4),
                accel=(rng.normal(0, 1.0, (ticks, B, 3)) + [0, 0, 9.81]).astype(f4),
                dofs=rng.normal(0, 1.0, (ticks, B, 12, 2)).astype(f4), touch=touch)


def sensors(B, seed=7, scale=None, **constants):
    from mpcqp.sensors import BatchedSensors
    return BatchedSensors(B, seed=seed, scale=scale, **dict(dr.Params().constants(), **constants))


def run_device(sens, ins, ticks, groups=("gyro", "accel", "dofs", "touch"), alias=False):
    """`ticks` updates on the device with nothing read back in between: the outputs per tick and
    the record after each, as NumPy."""
    dev = {k: _dev(ins[k]) for k in groups}
    outs = {k: [] for k in groups}
    states, status = [], []
    for t in range(ticks):
        if alias:
            for k in groups:
                getattr(sens, k).copy_(dev[k][t])
            sens.update(**{k: getattr(sens, k) for k in groups})
        else:
            sens.update(**{k: dev[k][t] for k in groups})
        for k in groups:
            outs[k].append(getattr(sens, k).clone())
        states.append(sens.state.clone())
        status.append(sens.status.clone())
    torch.cuda.synchronize()
    res = {k: torch.stack(v).cpu().numpy() for k, v in outs.items()}
    res["state"], res["status"] = torch.stack(states).cpu().numpy(), torch.stack(status).cpu().numpy()
    return res


def run_ref(P, B, ins, ticks, scale=None, state=None):
    st = dr.new_state(B) if state is None else state
    outs = {k: [] for k in ("gyro", "accel", "dofs", "touch", "status", "state")}
    for t in range(ticks):
        o = dr.tick(st, P, scale=scale, **{k: ins[k][t] for k in ("gyro", "accel", "dofs", "touch")})
        for k in o:
            outs[k].append(o[k])
        outs["state"].append(st.copy())
    return {k: np.stack(v) for k, v in outs.items()}


@pytest.mark.parametrize("B", SIZES)
def test_device_against_restatement(B):
    """T = 200 ticks of the preset (with joint noise) at per-robot scales 0..4, once with q_lsb on,
    lag 2 and p_drop 0.25 and once with q_lsb off, lag 0 and no dropout.  Histories, count,
    touch_m and status bitwise; float32 outputs equal but for at most 1 word in 10^4 one ulp
    (one q_lsb) off; bias words within BIAS_BOUND of the robot's s walk sqrt(dt T).

    Measured on the MI355X: no float32 word off, worst bias difference 0 (the module docstring)."""
    scale = (np.arange(B) % 5).astype(np.float32)
    ins = inputs(B, T, seed=B)
    for n, c in enumerate(CONFIGS):
        P = dr.Params(seed=0xC0FFEE0000000001 + n, **c)
        sens = sensors(B, seed=P.seed, scale=scale, **c)
        got, want = run_device(sens, ins, T), run_ref(P, B, ins, T, scale=scale)
        assert np.array_equal(got["state"][:, :, dr.INIT:dr.WORDS], want["state"][:, :, dr.INIT:dr.WORDS])
        assert np.array_equal(got["touch"], want["touch"]) and np.array_equal(got["status"], want["status"])
        assert (got["status"] == 0).all() and (got["state"][-1, :, dr.COUNT] == T).all()
        words = off = 0
        for k in ("gyro", "accel", "dofs"):
            d = got[k] != want[k]
            words += d.size
            off += int(d.sum())
            lim = np.spacing(np.maximum(np.abs(got[k]), np.abs(want[k])))
            if k == "dofs" and P.q_lsb > 0:
                lim[..., 0] = np.float32(P.q_lsb * 1.0001)
            assert (np.abs(got[k].astype(np.float64) - want[k]) <= lim)[d].all(), k
        unit = scale.astype(np.float64)[:, None] * np.repeat([P.walk_gyro, P.walk_accel], 3) * np.sqrt(P.dt * T)
        err = np.abs(got["state"][:, :, :6] - want["state"][:, :, :6]).max(0)
        assert (err[scale == 0] == 0).all()
        rel = (err[scale > 0] / unit[scale > 0]).max() if (scale > 0).any() else 0.0
        print(f"\nB = {B}, config {n}: {off} of {words} float32 words one ulp off; worst bias error "
              f"{err.max():.3e}, {rel:.3e} of s walk sqrt(dt T)")
        assert off <= words * 1e-4
        assert rel <= BIAS_BOUND < BIAS_LIMIT


def test_determinism_seeds_offsets_and_aliasing():
    """The same seed twice is bitwise; another seed differs in every channel; rows [0, 37) plus
    [37, 130) through offset pointers are bitwise the whole batch; outputs aliased to the inputs
    are bitwise the separate buffers."""
    B, ticks = 130, 5
    c = CONFIGS[0]
    ins = inputs(B, ticks, seed=1)
    a = run_device(sensors(B, seed=7, **c), ins, ticks)
    b = run_device(sensors(B, seed=7, **c), ins, ticks)
    for k in a:
        assert np.array_equal(_bits(torch.as_tensor(a[k])), _bits(torch.as_tensor(b[k]))), k
    other = run_device(sensors(B, seed=8, **c), ins, ticks)
    for k in ("gyro", "accel"):
        assert (other[k] != a[k]).all(), k
    assert (other["dofs"][..., 1] != a["dofs"][..., 1]).all()
    assert (other["dofs"][..., 0] != a["dofs"][..., 0]).mean() > 0.5           # quantised: some land on the same step
    assert (other["state"][:, :, :6] != a["state"][:, :, :6]).all() and (other["touch"] != a["touch"]).any()
    al = run_device(sensors(B, seed=7, **c), ins, ticks, alias=True)
    for k in a:
        assert np.array_equal(_bits(torch.as_tensor(a[k])), _bits(torch.as_tensor(al[k]))), k
    # two launches on offset pointers
    sens = sensors(B, seed=7, **c)
    dev = {k: _dev(v) for k, v in ins.items()}
    s = torch.cuda.current_stream()
    for t in range(ticks):
        for first, count in ((0, 37), (37, 93)):
            sens.bind_update(**{k: v[t] for k, v in dev.items()}, first=first, count=count)(s)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(sens.state), _bits(torch.as_tensor(a["state"][-1])))
    for k in ("gyro", "accel", "dofs", "touch"):
        assert np.array_equal(_bits(getattr(sens, k)), _bits(torch.as_tensor(a[k][-1]))), k


def test_graph_replay_equals_eager_calls():
    """update captured once and replayed 19 times leaves bitwise what 19 eager calls leave: the
    record lives in caller memory, so a replay advances it."""
    B = 65
    ins = {k: _dev(v[0]) for k, v in inputs(B, 1, seed=2).items()}
    runs = []
    for graphed in (False, True):
        sens = sensors(B, seed=3, **CONFIGS[0])
        sens.update(**ins)                                   # the turn-on call, eager in both
        if graphed:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                sens.update(**ins)
            for _ in range(19):
                g.replay()
        else:
            for _ in range(19):
                sens.update(**ins)
        torch.cuda.synchronize()
        assert (sens.count == 20).all()
        runs.append([_bits(t) for t in (sens.state, sens.gyro, sens.accel, sens.dofs, sens.touch, sens.status)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_canaries_and_nullable_pairs():
    """Rows past the batch are untouched; every nullable pair left out leaves the remaining
    outputs and the record's draws bitwise."""
    B, extra = 67, 3
    c = CONFIGS[0]
    ins = {k: _dev(v[0]) for k, v in inputs(B + extra, 1, seed=3).items()}
    P = dr.Params(seed=5, **c)
    full = sensors(B + extra, seed=5, **c)
    for _ in range(3):
        full.update(**ins)
    sens = sensors(B + extra, seed=5, **c)
    for t in (sens.gyro, sens.accel, sens.dofs, sens.touch):
        t.fill_(-77.0)
    sens._status.fill_(-3)
    sens.state[B:] = -5.0
    for _ in range(3):
        sens.bind_update(**ins, first=0, count=B)(torch.cuda.current_stream())
    torch.cuda.synchronize()
    for k in ("gyro", "accel", "dofs", "touch"):
        assert (getattr(sens, k)[B:] == -77.0).all() and np.array_equal(_bits(getattr(sens, k)[:B]), _bits(getattr(full, k)[:B])), k
    assert (sens.status[B:] == -3).all() and (sens.state[B:] == -5.0).all() and (sens.status[:B] == 0).all()
    assert np.array_equal(_bits(sens.state[:B]), _bits(full.state[:B]))
    for left_out in ("gyro", "accel", "dofs", "touch"):
        part = sensors(B + extra, seed=5, **c)
        getattr(part, left_out).fill_(-77.0)
        for _ in range(3):
            part.update(**{k: v for k, v in ins.items() if k != left_out})
        torch.cuda.synchronize()
        assert (getattr(part, left_out) == -77.0).all()
        for k in ins:
            if k != left_out:
                assert np.array_equal(_bits(getattr(part, k)), _bits(getattr(full, k))), (left_out, k)
        words = slice(0, dr.HIST) if left_out == "touch" else slice(0, dr.WORDS)
        assert np.array_equal(_bits(part.state[:, words]), _bits(full.state[:, words]))
    assert P.seed == 5


def test_one_robot_per_refusal_cause():
    """A non-finite gyro, dof, touch, scale or record word and a negative scale each refuse one
    robot: status 4, its record untouched, its outputs its inputs; its neighbours draw what they
    draw without it."""
    B = 70
    c = CONFIGS[0]
    ins = {k: v[0] for k, v in inputs(B, 1, seed=4).items()}
    scale = np.ones(B, np.float32)
    clean = sensors(B, seed=9, scale=_dev(scale), **c)
    clean.update(**{k: _dev(v) for k, v in ins.items()})
    start = clean.state.clone()
    clean.update(**{k: _dev(v) for k, v in ins.items()})
    bad_rows = [2, 17, 33, 48, 63, 69, 5, 40]
    ins = {k: v.copy() for k, v in ins.items()}
    ins["gyro"][2, 0] = np.nan
    ins["dofs"][17, 11, 0] = np.inf
    ins["touch"][33, 1] = np.nan
    scale[48], scale[63] = np.nan, -0.5
    sens = sensors(B, seed=9, scale=_dev(scale), **c)
    sens.state.copy_(start)
    sens.state[69, dr.BIAS_A + 1] = float("inf")
    sens.state[5, dr.COUNT], sens.state[40, dr.HIST] = -1.0, 2.0 ** 32       # outside the integers they are read as
    before = sens.state.clone()
    dev = {k: _dev(v) for k, v in ins.items()}
    sens.update(**dev)
    torch.cuda.synchronize()
    status = sens.status.cpu().numpy()
    others = np.ones(B, bool)
    others[bad_rows] = False
    assert (status[bad_rows] == 4).all() and (status[others] == 0).all()
    assert np.array_equal(_bits(sens.state[bad_rows]), _bits(before[bad_rows]))
    assert np.array_equal(_bits(sens.state)[others], _bits(clean.state)[others])
    for k in dev:
        assert np.array_equal(_bits(getattr(sens, k))[bad_rows], _bits(dev[k])[bad_rows]), k
        assert np.array_equal(_bits(getattr(sens, k))[others], _bits(getattr(clean, k))[others]), k


def test_entry_refusals_and_setter():
    """Non-zero flags, batch < 0, a NULL or misaligned record, an input without its output:
    MPCQP_ERR_ARG with a message and nothing written; batch == 0 is MPCQP_OK.  A refused constant
    raises and the previous constants stay in force."""
    from mpcqp import _lib
    B = 5
    c = CONFIGS[0]
    sens = sensors(B, seed=2, **c)
    ins = {k: _dev(v[0]) for k, v in inputs(B, 1, seed=5).items()}
    lib, ctx = sens.lib, sens._ctx
    for t in (sens.gyro, sens.accel, sens.dofs, sens.touch):
        t.fill_(-77.0)
    big = torch.zeros((B * dr.STRIDE + 2,), dtype=torch.float64, device=DEV)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(batch=B, flags=0, state=sens.state, **over):
        b = dict(gyro=ins["gyro"], accel=ins["accel"], dofs=ins["dofs"], touch=ins["touch"], gyro_m=sens.gyro,
                 accel_m=sens.accel, dofs_m=sens.dofs, touch_m=sens.touch)
        b.update(over)
        return lib.mpcqp_sensors(ctx, batch, flags, p(b["gyro"]), p(b["accel"]), p(b["dofs"]), p(b["touch"]), None,
                                 p(state) if isinstance(state, torch.Tensor) else state, p(b["gyro_m"]), p(b["accel_m"]),
                                 p(b["dofs_m"]), p(b["touch_m"]), p(sens._status), stream)
    before = _bits(sens.state)
    assert call(flags=1) == -1 and b"flags" in lib.mpcqp_last_error(ctx)
    assert call(batch=-1) == -1
    assert call(state=None) == -1
    assert call(state=ctypes.c_void_p(big.data_ptr() + 8)) == -1 and b"aligned" in lib.mpcqp_last_error(ctx)
    assert call(gyro=None) == -1 and call(gyro_m=None) == -1 and call(touch_m=None) == -1 and call(dofs=None) == -1
    assert call(batch=0) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(sens.state), before)
    assert all((t == -77.0).all() for t in (sens.gyro, sens.accel, sens.dofs, sens.touch))
    # the setter
    kept = sens.constants
    for bad in (dict(sigma_gyro=-1.0), dict(walk_accel=float("nan")), dict(q_lsb=float("inf")), dict(touch_lag=32),
                dict(touch_lag=-1), dict(p_drop=1.0), dict(p_drop=-0.1), dict(bias0_gyro=-1e-9)):
        with pytest.raises(_lib.MpcqpError):
            sens.set_constants(**bad)
        assert sens.constants == kept
    with pytest.raises(TypeError):
        sens.set_constants(sigma=1.0)
    with pytest.raises(ValueError, match="contiguous float32"):
        sens.bind_update(gyro=ins["gyro"].double())
    assert call() == 0                                       # the constants in force are still the accepted ones
    torch.cuda.synchronize()
    st = dr.new_state(B)
    want = dr.tick(st, dr.Params(seed=2, **c), **{k: v.cpu().numpy() for k, v in ins.items()})
    assert np.array_equal(sens.touch.cpu().numpy(), want["touch"]) and np.array_equal(sens.state.cpu().numpy()[:, dr.INIT:], st[:, dr.INIT:])
    # the push's entry refusals
    from mpcqp.plant import BatchedPlant
    plant = BatchedPlant(B, engine=sens.engine)
    plant.reset()
    J = _dev(np.ones((B, 3), np.float32))
    rec = _bits(plant.state)
    status = torch.zeros(B, dtype=torch.int32, device=DEV)
    assert lib.mpcqp_push(ctx, -1, p(J), None, p(plant.robot), p(plant.state), p(status), stream) == -1
    assert lib.mpcqp_push(ctx, B, None, None, p(plant.robot), p(plant.state), p(status), stream) == -1
    assert lib.mpcqp_push(ctx, B, p(J), None, None, p(plant.state), p(status), stream) == -1
    assert lib.mpcqp_push(ctx, B, p(J), None, p(plant.robot), None, p(status), stream) == -1
    assert lib.mpcqp_push(ctx, B, p(J), None, p(plant.robot), ctypes.c_void_p(big.data_ptr() + 8), p(status), stream) == -1
    assert lib.mpcqp_push(ctx, 0, p(J), None, p(plant.robot), p(plant.state), p(status), stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(plant.state), rec)
    with pytest.raises(ValueError, match="contiguous float32"):
        plant.bind_push(J.double())


def test_count_crossing_2_to_32():
    B = 6
    c = CONFIGS[0]
    ins = inputs(B, 4, seed=6)
    st = dr.new_state(B)
    st[:, dr.COUNT], st[:, dr.INIT] = 2.0 ** 32 - 2, 1.0
    sens = sensors(B, seed=12, **c)
    sens.state.copy_(_dev(st))
    got, want = run_device(sens, ins, 4), run_ref(dr.Params(seed=12, **c), B, ins, 4, state=st)
    assert np.array_equal(got["state"][:, :, dr.INIT:dr.WORDS], want["state"][:, :, dr.INIT:dr.WORDS])
    assert (got["state"][-1, :, dr.COUNT] == 2.0 ** 32 + 2).all()
    assert np.array_equal(got["touch"], want["touch"])
    assert np.array_equal(got["state"][:, :, :6], want["state"][:, :, :6])      # the main comparison's bias bound, 0
    for k in ("gyro", "accel", "dofs"):
        assert (np.abs(got[k].astype(np.float64) - want[k]) <= np.maximum(np.spacing(np.abs(want[k])), P_LSB if k == "dofs" else 0)).all()
        assert (got[k] != want[k]).mean() <= 1e-4


# ---- the push on the device

@pytest.mark.parametrize("B", (5, 130))
def test_push_matches_the_restatement_on_a_mixed_fleet(B):
    """A1 and Aliengo records alternate; with and without a point: the record within PUSH_BOUND
    of the restatement, nothing but velocity and rate written; J = 0 bitwise; refusals."""
    from mpcqp.plant import BatchedPlant
    par = pr.Params()
    st = pr.make_mixed_states(B, seed=B, par=par)
    rng = np.random.default_rng(B)
    J = rng.normal(0, 3.0, (B, 3)).astype(np.float32)
    r = rng.normal(0, 0.2, (B, 3)).astype(np.float32)
    plant = BatchedPlant(B)
    plant.robot = _dev(st["robot"], torch.float32)
    worst = 0.0
    for point in (None, r):
        want = st["rec"].copy()
        assert (dr.push(want, J, st["robot"], point) == 0).all()
        plant.state.copy_(_dev(st["rec"]))
        plant.push(_dev(J), None if point is None else _dev(point))
        torch.cuda.synchronize()
        got = plant.state.cpu().numpy()
        assert (plant.push_status == 0).all()
        keep = np.ones(pr.STRIDE, bool)
        keep[pr.VEL:pr.OMEGA + 3] = False
        assert np.array_equal(got[:, keep].view(np.uint64), st["rec"][:, keep].view(np.uint64))
        if point is None:
            assert np.array_equal(got[:, pr.OMEGA:pr.OMEGA + 3].view(np.uint64), st["rec"][:, pr.OMEGA:pr.OMEGA + 3].view(np.uint64))
        worst = max(worst, pr.record_error(got, want).max())
        plant.state.copy_(_dev(st["rec"]))
        plant.push(np.zeros(3, np.float32), None if point is None else _dev(point))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(plant.state), st["rec"].view(np.uint64))
    print(f"\npush, B = {B}: worst record error {worst:.2e}")
    assert worst <= PUSH_BOUND
    # refusals: one robot per cause, the others pushed
    k = min(B, 5)
    Jb, rb, rec0, robot = J.copy(), r.copy(), st["rec"].copy(), st["robot"].copy()
    Jb[0, 2] = np.nan
    if k > 1:
        rb[1, 0] = np.inf
        rec0[2, pr.FVEL + 1] = np.nan
        robot[3, 0] = -1.0
        rec0[4, pr.QUAT:pr.QUAT + 4] = 0.0
    want = rec0.copy()
    status = dr.push(want, Jb, robot, rb)
    assert status[:k].tolist() == [4] * k and (status[k:] == 0).all()
    plant.robot = _dev(robot, torch.float32)
    plant.state.copy_(_dev(rec0))
    plant.push(_dev(Jb), _dev(rb))
    torch.cuda.synchronize()
    got = plant.state.cpu().numpy()
    assert np.array_equal(plant.push_status.cpu().numpy(), status)
    assert np.array_equal(got[:k].view(np.uint64), rec0[:k].view(np.uint64))
    assert B == k or pr.record_error(got[k:], want[k:]).max() <= PUSH_BOUND


# ---- the closed loop on the device

def _closed_loop(scales, pushes, ticks=600, push_tick=400, with_stage=True, preset="mems"):
    """The sensing chain's loop of tests/test_gpu_plant.py (Aliengo, TROTTING10, 0.5 m/s, N = 10,
    50 ticks of settling) with the sensor stage between the plant and the estimator and a
    lateral impulse at the centre of mass at `push_tick`.  Returns per tick the plant's body
    words, the torques and the estimate, and the worst status."""
    from mpcqp.controller import BatchedController
    from mpcqp.estimator import BatchedEstimator
    from mpcqp.plant import BatchedPlant
    from mpcqp.sensors import BatchedSensors
    B = len(scales)
    ctl = BatchedController(B, horizon=N, robot="aliengo", gait="TROTTING10")
    plant = BatchedPlant(B, controller=ctl, foot_mass=0.15, substeps=1, ground_z=-0.0255, contact_tol=1e-4)
    par = pr.Params()
    geom = plant.geometry.cpu().numpy()
    root0, _ = pr.stand_pose(B, geom, par)
    plant.reset(height=float(root0[0, 2]))
    est = BatchedEstimator(B, robot="aliengo", controller=ctl, contact_height=par.ground_z)
    sens = BatchedSensors(B, plant=plant, seed=7, preset=preset, scale=_dev(np.asarray(scales, np.float32)))
    src = sens if with_stage else plant
    _, _, Jb = kin_ref.chain(geom, plant.dofs[:, :, 0].cpu().numpy())
    m = float(plant.robot[0, 0])
    stand = _dev(np.einsum("blcr,c->blr", Jb, -np.array([0, 0, m * par.gravity / 4])).reshape(B, 12), torch.float32)

    def sense(it):
        if with_stage:
            sens.update()
        return est.update_from_imu(src.gyro, src.accel, src.dofs, tick=it, touch=src.touch)
    for it in range(50):
        plant.step(stand)
        sense(it)
    vb = torch.zeros((B, 3), dtype=torch.float64, device=DEV)
    vb[:, 0] = 0.5
    ctl.set_command(vb, 0.0)
    J = torch.zeros((B, 3), dtype=torch.float32, device=DEV)
    J[:, 1] = torch.as_tensor(np.asarray(pushes, np.float32))
    hist = torch.zeros((ticks, B, 13), dtype=torch.float64, device=DEV)
    taus = torch.zeros((ticks, B, 12), dtype=torch.float32, device=DEV)
    ests = torch.zeros((ticks, B, 13), dtype=torch.float32, device=DEV)
    sig = torch.zeros((ticks, B, 3), dtype=torch.float64, device=DEV)
    bad = torch.zeros((B,), dtype=torch.int32, device=DEV)
    for it in range(ticks):
        r = sense(it)
        ests[it] = r
        sig[it] = torch.diagonal(est.covariance, dim1=1, dim2=2)[:, 0:3]
        ctl.step_fused(it, None, None, r, src.dofs)
        if it == push_tick and with_stage:
            plant.push(J)
        plant.step(ctl.tau)
        hist[it], taus[it] = plant.state[:, :13], ctl.tau
        bad |= ctl.status | plant.status | est.status | (sens.status if with_stage else 0)
    torch.cuda.synchronize()
    return dict(hist=hist.cpu().numpy(), tau=taus.cpu().numpy(), est=ests.cpu().numpy(), bad=bad.cpu().numpy(),
                sigma3=3 * np.sqrt(np.abs(sig.cpu().numpy())))


def cpu_loop():
    """The CPU oracle loop's recorded figures (tests/golden/disturb_loop.npz, compared with a
    fresh run by tests/test_disturb.py)."""
    import os
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disturb_loop.npz")))


def test_closed_loop_with_the_stage():
    """Eight robots in the CPU loop's configuration (disturb_ref.closed_loop_sensed).  Four at
    scales 0, 1, 2, 4 of the preset: those that stayed within bounds on the CPU loop stay finite,
    keep every status OK and stay within twice the CPU loop's recorded figures (height error,
    roll, pitch, estimate error; the speed within 0.05 m/s, the measure tests/test_gpu_plant.py
    uses for it).  The others are noise-free and shoved sideways at tick 400 by the CPU loop's
    impulses up to half the largest that recovered there (2 N s: so 0 and 1 N s), and stay within
    twice the CPU figures likewise.  A robot's scale does not reach the encoder step or the touch
    lag, so a scale-0 robot is not the loop without the stage: that comparison is
    test_identity_stage_is_bitwise_the_loop_without_it's.  Printed: every robot's figures, and
    the estimate's error beside the 3 sigma of the filter's own covariance.

    Measured on the MI355X: the CPU loop's figures to four digits for every robot -- at scales 0,
    1, 2, 4 height error 0.0235 m, roll 0.0317 / 0.0365 / 0.0288 / 0.0425 rad, pitch 0.0343 / 0.0257 /
    0.0295 / 0.0477 rad, speed 0.5498 / 0.5417 / 0.5424 / 0.5797 m/s, estimate error 5.53 / 5.54 / 5.53 /
    13.78 mm; shoved by 1 N s: roll 0.0317 rad, speed 0.5494 m/s."""
    fx = cpu_loop()
    recovered = fx["pushes"][fx["recovered"] & (fx["scales"] == 0)]
    allowed = sorted(set(p for p in fx["pushes"][fx["scales"] == 0] if p <= recovered.max() / 2))
    assert recovered.max() == 2.0 and allowed == [0.0, 1.0]
    noisy = [int(np.flatnonzero((fx["scales"] == s) & (fx["pushes"] == 0))[0]) for s in (0, 1, 2, 4)]
    pushed = [int(np.flatnonzero((fx["scales"] == 0) & (fx["pushes"] == p))[-1]) for p in allowed]
    rows = (noisy + pushed + pushed)[:8]                    # the CPU loop's robot each device robot repeats
    scales, pushes = fx["scales"][rows], fx["pushes"][rows]
    run = _closed_loop(tuple(scales), tuple(pushes))
    fig = dr.loop_figures(run["hist"], run["est"].astype(np.float64), (run["bad"] == 0)[None, :])
    print(f"\nclosed loop with the sensor stage, scales {scales}, pushes {pushes} N s:")
    for k in dr.FIGURES:
        print(f"  {k}: {fig[k]}\n    CPU loop: {fx[k][rows]}")
    print(f"  3 sigma of the filter's position covariance {run['sigma3'].max((0, 2))}")
    held = fx["within"][rows]
    assert held.all()                                        # every robot chosen stayed within bounds on the CPU loop
    assert np.isfinite(run["hist"]).all() and np.isfinite(run["tau"]).all() and (run["bad"] == 0).all()
    for k in ("height", "roll", "pitch", "est_error"):
        assert (fig[k] <= 2 * fx[k][rows]).all(), (k, fig[k], fx[k][rows])
    assert (np.abs(fig["speed"] - fx["speed"][rows]) <= 0.05).all()
    assert fig["within"].all() and fig["recovered"].all()
    # the repeated robots agree bitwise: nothing of a robot's draws reaches its neighbour
    for a in range(len(rows)):
        for b in range(a + 1, len(rows)):
            if rows[a] == rows[b]:
                assert np.array_equal(_bits(torch.as_tensor(run["hist"][:, a])), _bits(torch.as_tensor(run["hist"][:, b])))


def test_identity_stage_is_bitwise_the_loop_without_it():
    """With every constant zero the stage in the loop leaves every recorded buffer of every tick
    bitwise what the loop without the stage leaves: the no-regression proof."""
    with_stage = _closed_loop((1, 1, 1, 1), (0, 0, 0, 0), ticks=300, preset=None)
    without = _closed_loop((1, 1, 1, 1), (0, 0, 0, 0), ticks=300, with_stage=False)
    for k in ("hist", "tau", "est"):
        assert np.array_equal(_bits(torch.as_tensor(with_stage[k])), _bits(torch.as_tensor(without[k]))), k
    assert (with_stage["bad"] == 0).all() and np.isfinite(with_stage["hist"]).all()

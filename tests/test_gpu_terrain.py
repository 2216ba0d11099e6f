"""GPU: mpcqp_terrain -- each robot's ground plane fitted to the feet last in contact, in one
launch -- against the float64 restatement tests/terrain_ref.py (pinned on the CPU to known
answers and to the reference's recorded run, tests/test_terrain.py), and the two consumers:
the cone rows of the solve through the robot record, the swing leg through mpcqp_set_ground.

W = 64 robots per workgroup, one lane per robot; B = 1, W - 1, W, W + 1, 2 W + 3, 24 ticks of
TROTTING10 at iterations_between_mpc = 2 (terrain_ref.GPU_TRAJECTORY, more than one gait
period).  Every output and the record lie between canaries -- one row ahead of the first robot,
two past the last -- and every launch finds them untouched.

Bounds.  The history, `fitted` and `status` have none: bitwise / equal.  The record's n and d
against terrain_ref within N_BOUND = 10 terrain_ref.D_N = 1.1e-14 (norm_err: n in the max norm,
d relative to max(1, |mu|)), the project's rule for a device build of a host-checked text.  The
float32 outputs within F32_BOUND = 2.4e-7 of tests/test_gpu_kin.py.  The swing leg on a plane
against terrain_ref.GroundSwingRef within tests/test_gpu_swing.py's BOUND = 4.61e-7.

Measured on the MI355X (also DESIGN.md 4.4g): the record against terrain_ref 1.3e-16 at B = 1,
1.0e-15 at B = 63, 64, 65 and 131; the float32 outputs bitwise terrain_ref's (0) at every B;
history, fitted and status equal.  The swing leg on tilted planes against GroundSwingRef, both
input layouts alike: tau 1.7e-8, pos_target 5.6e-8, vel_target 5.3e-8.  BatchedTerrain after 40
ticks on a 0.2 rad plane: 2.0e-8 against the plane itself, 2.2e-8 against the fit of the
controller's float32 pos_feet (footprint 0.264 m), both under F32_BOUND; normal_base 2.2e-8
against R_base^T n of the restatement (1.1e-8 against the body's own z, not asserted: R_base is
the float32 quat2matrix, whose own rounding that figure would be held to).
"""
import ctypes
import functools

import numpy as np
import pytest

# torch first: it brings its own HIP runtime, which must be loaded before libmpcqp.so
torch = pytest.importorskip("torch")

import swing_ref  # noqa: E402
import terrain_ref as tr  # noqa: E402
from helpers import DEV, _dev  # noqa: E402

pytestmark = pytest.mark.gpu

W = 64
BATCHES = (1, W - 1, W, W + 1, 2 * W + 3)
N_BOUND = 10 * tr.D_N
F32_BOUND = 2.4e-7
SWING_BOUND = 4.61e-7          # tests/test_gpu_swing.py BOUND
CANARY = -77.0
OUTPUTS = ("normal", "plane", "normal_base", "status")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def oracle():
    """The trajectory and terrain_ref's run of it, computed once and sliced per batch size
    (the robots are independent)."""
    traj = tr.make_trajectory(**tr.GPU_TRAJECTORY)
    states, outs = tr.run(traj)
    stack = {k: np.stack([t[k] for t in traj]) for k in ("pos_feet", "swing_state", "contact", "quat")}
    rs = np.zeros(stack["quat"].shape[:2] + (13,), np.float32)
    rs[..., [6, 3, 4, 5]] = stack["quat"]
    stack["root_states"] = rs
    return stack, states, outs


def engine(**constants):
    from mpcqp import LinearMpc
    eng = LinearMpc(horizon=10, robot="a1", device=DEV)
    eng.set_terrain(**constants)
    return eng


FRONT = 1        # canary rows ahead of the first robot (a 160-byte record row keeps the 16-byte alignment)


def buffers(B, pad=2):
    """The record and the outputs, each with FRONT canary rows ahead of its B rows and `pad`
    behind them; the record's B rows start at zero."""
    rows = FRONT + B + pad
    bf = dict(state=torch.full((rows, tr.STRIDE), CANARY, dtype=torch.float64, device=DEV),
              normal=torch.full((rows, 3), CANARY, device=DEV), plane=torch.full((rows, 4), CANARY, device=DEV),
              normal_base=torch.full((rows, 3), CANARY, device=DEV),
              status=torch.full((rows,), int(CANARY), dtype=torch.int32, device=DEV))
    bf["state"][FRONT:FRONT + B] = 0.0
    return bf


def live(bf, k, B):
    """The B rows of buffer k that a launch is handed."""
    return bf[k][FRONT:FRONT + B]


def read(bf):
    """The buffers on the host without their front canaries, which are checked here: rows
    [:B] the robots', rows [B:] the canaries behind them."""
    out = {}
    for k, v in bf.items():
        a = v.cpu().numpy().copy()
        assert (a[:FRONT] == CANARY).all(), (k, "front canary")
        out[k] = a[FRONT:]
    return out


def run_device(eng, B, rule="swing_state", layout="quat", skip=(), robot=None, ticks=None, feet=None):
    """The trajectory's first B robots through eng.terrain: per tick the record and the
    outputs, canary rows included."""
    stack, _, _ = oracle()
    dv = {k: _dev(v[:, :B]) for k, v in stack.items()}
    if feet is not None:
        dv["pos_feet"] = _dev(feet)
    bf = buffers(B)
    out = []
    for t in range(stack["quat"].shape[0] if ticks is None else ticks):
        kw = {rule: dv[rule][t], ("root_states" if layout == "root" else "quat"): dv["root_states" if layout == "root" else "quat"][t]}
        kw.update({k: live(bf, k, B) for k in OUTPUTS if k not in skip})
        eng.terrain(live(bf, "state", B), dv["pos_feet"][t], robot=robot, **kw)
        torch.cuda.synchronize()
        out.append(read(bf))
    return out


def check_against_ref(out, B, skip=(), tag=""):
    """The exact parts asserted; returns (record error, float32 error)."""
    _, states, outs = oracle()
    D = f32 = 0.0
    for t, o in enumerate(out):
        st, ref = o["state"][:B], states[t][:B]
        assert same(st[:, tr.HIST], ref[:, tr.HIST]), (tag, t, "history")
        assert np.array_equal(st[:, [tr.INIT, tr.FITTED, 18, 19]], ref[:, [tr.INIT, tr.FITTED, 18, 19]]), (tag, t)
        D = max(D, tr.norm_err(st, ref))
        for k in OUTPUTS:
            if k in skip:
                assert (o[k] == CANARY).all(), (tag, t, k)
                continue
            assert (o[k][B:] == CANARY).all(), (tag, t, k, "canary")
            if k == "status":
                assert np.array_equal(o[k][:B], outs[k][t][:B]), (tag, t)
            else:
                want = outs[k][t][:B].astype(np.float64)
                f32 = max(f32, float(np.abs(o[k][:B] - want).max()) / max(1.0, float(np.abs(want).max())))
        assert (o["state"][B:] == CANARY).all(), (tag, t, "state canary")
    return D, f32


@pytest.mark.parametrize("B", BATCHES)
def test_against_the_restatement(B):
    out = run_device(engine(), B)
    D, f32 = check_against_ref(out, B, tag=B)
    print(f"\nB = {B}: record {D:.2e} (bound {N_BOUND:.1e}), float32 outputs {f32:.2e} (bound {F32_BOUND:.1e})")
    assert D <= N_BOUND and f32 <= F32_BOUND
    _, states, _ = oracle()
    assert (states[:, :B, tr.FITTED] == 1).all()


@pytest.mark.parametrize("skip", OUTPUTS)
def test_each_output_absent_in_turn(skip):
    B = W + 1
    D, f32 = check_against_ref(run_device(engine(), B, skip=(skip,), ticks=6), B, skip=(skip,), tag=skip)
    assert D <= N_BOUND and f32 <= F32_BOUND


@pytest.mark.parametrize("rule,layout", [("contact", "quat"), ("swing_state", "root"), ("contact", "root")])
def test_contact_rules_and_quaternion_layouts(rule, layout):
    B = W + 1
    base = run_device(engine(), B)
    out = run_device(engine(), B, rule=rule, layout=layout)
    for t, (a, b) in enumerate(zip(out, base)):
        for k in a:
            assert same(a[k], b[k]), (rule, layout, t, k)


def test_robot_record_words():
    B = W + 1
    full0 = np.arange((B + 3) * 16, dtype=np.float32).reshape(B + 3, 16)
    full = _dev(full0)
    out = run_device(engine(), B, robot=full[1:B + 1], ticks=3)       # a row ahead, two behind
    assert same(full.cpu().numpy()[0], full0[0])
    got, rob0 = full.cpu().numpy()[1:], full0[1:]
    assert same(got[:B, 9:12], out[-1]["normal"][:B]) and not same(got[:B, 9:12], rob0[:B, 9:12])
    keep = np.ones(16, bool)
    keep[9:12] = False
    assert same(got[:, keep], rob0[:, keep]) and same(got[B:], rob0[B:])


@pytest.mark.parametrize("bad", [0, 31, W - 1, W, W + 2])
def test_a_refused_robot_leaves_its_neighbours_alone(bad):
    """A NaN foot on one robot at each position of a workgroup, the tail included (B = W + 3):
    it is refused from that tick on and keeps its record; every other robot is bitwise the run
    without it."""
    B, at = W + 3, 4
    stack, _, _ = oracle()
    clean = run_device(engine(), B, ticks=8)
    feet = stack["pos_feet"][:8, :B].copy()
    feet[at:, bad, :, 2] = np.nan
    out = run_device(engine(), B, ticks=8, feet=feet)
    others = np.arange(B) != bad
    for t in range(8):
        for k in ("state",) + OUTPUTS:
            assert same(out[t][k][:B][others], clean[t][k][:B][others]), (bad, t, k)
            assert (out[t][k][B:] == CANARY).all()
        want = tr.STATUS_NONFINITE if t >= at else tr.STATUS_OK
        assert out[t]["status"][bad] == want
        if t >= at:
            assert same(out[t]["state"][bad], clean[at - 1]["state"][bad])
            assert same(out[t]["normal"][bad], clean[at - 1]["normal"][bad])


def test_argument_errors():
    from mpcqp import _lib
    eng = engine()
    lib, ctx = eng.lib, eng._ctx
    B = 5
    bf = buffers(B)
    stack, _, _ = oracle()
    a = dict(pos_feet=_dev(stack["pos_feet"][0, :B]), contact=_dev(stack["contact"][0, :B]),
             quat=_dev(stack["quat"][0, :B]), state=live(bf, "state", B), robot=None, normal=live(bf, "normal", B),
             plane=live(bf, "plane", B), normal_base=live(bf, "normal_base", B), status=live(bf, "status", B))
    odd = torch.zeros((B * tr.STRIDE + 1,), dtype=torch.float64, device=DEV)[1:]
    assert odd.data_ptr() % 16 == 8
    ptr = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())

    def call(batch=B, flags=0, **kw):
        v = dict(a, **kw)
        return lib.mpcqp_terrain(ctx, batch, flags, *(ptr(v[k]) for k in (
            "pos_feet", "contact", "quat", "state", "robot", "normal", "plane", "normal_base", "status")), None)

    err = lambda: lib.mpcqp_last_error(ctx).decode()
    refused = [(dict(flags=8), "flags"), (dict(flags=-1), "flags"), (dict(batch=-1), "batch"),
               (dict(pos_feet=None), "null"), (dict(contact=None), "null"), (dict(state=None), "null"),
               (dict(state=odd), "aligned"), (dict(quat=None), "normal_base")]
    for kw, word in refused:
        assert call(**kw) == _lib.ERR_ARG, kw
        assert word in err(), (kw, err())
    assert call(batch=0) == 0 and call(batch=0, quat=None, normal_base=None) == 0
    torch.cuda.synchronize()
    assert (bf["normal"] == CANARY).all() and (live(bf, "state", B) == 0).all()      # a refused call runs nothing
    assert call(quat=None, normal_base=None) == 0 and call(flags=3, quat=_dev(stack["root_states"][0, :B])) == 0
    # the constants: each refusal keeps the previous set
    good = (0.5, 1e-3, 0.5, 1.0)
    nan, inf = float("nan"), float("inf")
    for bad, word in [((nan,) + good[1:], "non-finite"), ((0.5, inf, 0.5, 1.0), "non-finite"), ((0.5, -1e-9, 0.5, 1.0), "flat_tol"),
                      ((0.5, 1.0, 0.5, 1.0), "flat_tol"), ((0.5, 1e-3, 0.0, 1.0), "cos_max_tilt"),
                      ((0.5, 1e-3, 1.5, 1.0), "cos_max_tilt"), ((0.5, 1e-3, 0.5, 0.0), "blend"),
                      ((0.5, 1e-3, 0.5, 1.5), "blend"), ((0.5, 1e-3, nan, 1.0), "non-finite")]:
        assert lib.mpcqp_set_terrain(ctx, *bad) == _lib.ERR_ARG and word in err(), bad
    assert lib.mpcqp_set_terrain(ctx, 0.5, 0.0, 1.0, 1.0) == 0 and lib.mpcqp_set_terrain(ctx, *good) == 0
    D, f32 = check_against_ref(run_device(eng, 3, ticks=3), 3)                  # the defaults are still in force
    assert D <= N_BOUND
    assert lib.mpcqp_set_ground(ctx, None, 1) == _lib.ERR_ARG and "ground" in err()
    assert lib.mpcqp_set_ground(ctx, ptr(bf["plane"]), -1) == _lib.ERR_ARG
    assert lib.mpcqp_set_ground(ctx, None, 0) == 0 and lib.mpcqp_set_ground(ctx, ptr(bf["plane"]), 0) == 0


def test_python_call_refuses_wrong_tensors():
    """LinearMpc.terrain takes B from terrain_state and checks every other tensor against it
    before the launch: a short, non-contiguous, wrongly typed or host tensor raises and nothing
    runs."""
    B = 5
    eng = engine()
    stack, _, _ = oracle()
    bf = buffers(B)
    good = dict(pos_feet=_dev(stack["pos_feet"][0, :B]), swing_state=_dev(stack["swing_state"][0, :B]),
                quat=_dev(stack["quat"][0, :B]), robot=torch.zeros((B, 16), device=DEV),
                **{k: live(bf, k, B) for k in OUTPUTS})
    short = lambda t: t[:B - 1]
    bad = [dict(pos_feet=short(good["pos_feet"])), dict(swing_state=short(good["swing_state"])),
           dict(quat=short(good["quat"])), dict(robot=short(good["robot"])), dict(normal=short(good["normal"])),
           dict(plane=short(good["plane"])), dict(normal_base=short(good["normal_base"])),
           dict(status=short(good["status"])), dict(status=good["status"].to(torch.int64)),
           dict(pos_feet=good["pos_feet"].double()), dict(pos_feet=good["pos_feet"].cpu()),
           dict(plane=torch.zeros((B, 8), device=DEV)[:, :4]), dict(pos_feet=None)]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.terrain(live(bf, "state", B), **dict(good, **kw))
    with pytest.raises(ValueError):
        eng.terrain(torch.zeros((B, tr.STRIDE + 1), dtype=torch.float64, device=DEV), **good)
    torch.cuda.synchronize()
    o = read(bf)
    assert (o["state"][:B] == 0).all() and all((o[k] == CANARY).all() for k in OUTPUTS)
    eng.terrain(live(bf, "state", B), **good)
    torch.cuda.synchronize()
    assert (read(bf)["status"][:B] == 0).all()


def test_graph_capture_advances_the_record():
    """A captured launch, replayed, advances the record as eager calls do (blend = 0.25, so the
    normal moves on every tick of constant inputs)."""
    B, reps = W + 1, 5
    stack, _, _ = oracle()
    feet, sw, q = _dev(stack["pos_feet"][3, :B]), _dev(stack["swing_state"][3, :B]), _dev(stack["quat"][3, :B])
    eng = engine(blend=0.25)

    def launch(bf, stream=None):
        eng.terrain(live(bf, "state", B), feet, swing_state=sw, quat=q, normal=live(bf, "normal", B),
                    plane=live(bf, "plane", B), normal_base=live(bf, "normal_base", B), status=live(bf, "status", B),
                    stream=stream)

    eager, seen = buffers(B), []
    for _ in range(reps):
        launch(eager)
        seen.append({k: v.clone() for k, v in eager.items()})
    torch.cuda.synchronize()
    bf = buffers(B)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch(bf, stream=s)
    for r in range(reps):
        g.replay()
        torch.cuda.synchronize()
        for k in bf:
            assert torch.equal(bf[k], seen[r][k]), (r, k)
    assert len({x["normal"].cpu().numpy().tobytes() for x in seen}) == reps


def test_cones_read_the_fitted_normal():
    """After ter.update() a solve on the attached record is bitwise a solve whose record had
    the same normal written by hand, and differs from the flat-cone solve.  N = 10, B = 8."""
    from mpcqp import BatchedTerrain
    from mpcqp.controller import BatchedController
    from mpcqp.synthetic import make_batch
    B, N = 8, 10
    bt = make_batch(B, N, seed=4)
    ctl = BatchedController(B, horizon=N, robot="a1", gait="trot10", iterations_between_mpc=2, warm_start=False)
    eng = ctl.engine
    flat = ctl.robot.clone()
    ter = BatchedTerrain(B, controller=ctl)
    stack, _, outs = oracle()
    n = ter.update(pos_feet=_dev(stack["pos_feet"][0, :B]), swing_state=_dev(stack["swing_state"][0, :B]))
    torch.cuda.synchronize()
    assert np.abs(n.cpu().numpy() - outs["normal"][0][:B]).max() <= F32_BOUND
    assert same(ctl.robot[:, 9:12].cpu().numpy(), n.cpu().numpy())
    hand = flat.clone()
    hand[:, 9:12] = n
    args = [_dev(bt[k]) for k in ("x0", "xref", "contact", "feet")]
    u_att = eng.solve(*args, robot=ctl.robot).clone()
    u_hand = eng.solve(*args, robot=hand).clone()
    u_flat = eng.solve(*args, robot=flat).clone()
    torch.cuda.synchronize()
    assert same(u_att.cpu().numpy(), u_hand.cpu().numpy())
    stance = bt["contact"][:, 0].any(axis=1)
    assert stance.any()
    assert all(not same(u_att.cpu().numpy()[b], u_flat.cpu().numpy()[b]) for b in np.flatnonzero(stance))


# ---- the swing leg

def _planes(B, seed=9):
    """Tilted planes [B,4] float32 near the robots' feet."""
    rng = np.random.default_rng(seed)
    tilt, az = rng.uniform(0.05, 0.5, B), rng.uniform(-np.pi, np.pi, B)
    n = np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], axis=1)
    return np.concatenate([n, rng.uniform(-0.2, 0.2, (B, 1))], axis=1).astype(np.float32)


@pytest.mark.parametrize("B", [1, 65, 130])
def test_step_without_a_ground_is_unchanged_and_level_planes_change_nothing(B):
    """Three controllers in one process: test_gpu_step's reference run never calls set_ground;
    one registers a ground and disables it again; one registers the planes (0, 0, 1, 0).  Every
    buffer of ``step`` and of ``step_fused`` is bitwise the first's."""
    import test_gpu_step as S
    seq, ref = S.sequence(B), S.reference(B)
    vb, yr = _dev(seq["vb"]), _dev(seq["yr"])
    level = torch.zeros((B, 4), device=DEV)
    level[:, 2] = 1.0
    for mode in ("disabled", "level"):
        for fused in (False, True):
            ctl = S.controller(B)
            ctl.engine.set_ground(_dev(_planes(B)))
            ctl.engine.set_ground(None if mode == "disabled" else level)
            for it in range(S.T):
                rs, ds = _dev(seq["rs"][it]), _dev(seq["ds"][it])
                if fused:
                    ctl.step_fused(it, vb, yr, rs, ds, outputs=True)
                else:
                    ctl.step(it, vb, yr, rs, ds)
                torch.cuda.synchronize()
                names = S.names_at(it) if fused else S.STATE + S.OPTIONAL + S.MPC_OUT
                S.assert_same(S.snapshot(ctl, names), ref[it], names, (mode, fused, B, it))


def test_leg_torques_without_a_ground_is_unchanged():
    import test_gpu_swing as GS
    from mpcqp.params import gait_record
    B, T = 65, 24
    gait = np.tile(gait_record("trot10"), (B, 1))
    ticks = np.tile(np.arange(T)[:, None], (1, B))
    inp = swing_ref.make_inputs(B, T, seed=77)
    base = GS.run_device(GS._engine(), inp, gait, ticks, 2, layout="root")
    level = np.tile(np.float32([0, 0, 1, 0]), (B, 1))
    for planes in (None, level):
        eng = GS._engine()
        eng.set_ground(_dev(_planes(B)))
        eng.set_ground(None if planes is None else _dev(planes))
        out = GS.run_device(eng, inp, gait, ticks, 2, layout="root")
        for k in base:
            assert same(out[k], base[k]), (planes is None, k)


def test_leg_torques_on_tilted_planes():
    """tau, the targets and swing_mem against GroundSwingRef within test_gpu_swing's bound; a
    robot past the capacity and a robot with a NaN plane walk as on the flat."""
    import test_gpu_swing as GS
    from mpcqp.params import gait_record
    B, T, cap, nanrow = 67, 24, 60, 7
    gait = np.tile(gait_record("trot10"), (B, 1))
    ticks = np.tile(np.arange(T)[:, None], (1, B))
    inp = swing_ref.make_inputs(B, T, seed=78)
    planes = _planes(B)
    planes[nanrow, 1] = np.nan
    eng = GS._engine()
    eng.set_ground(_dev(planes[:cap]))
    seen = np.full((B, 4), np.nan, np.float32)
    seen[:cap] = planes[:cap]
    ref = tr.GroundSwingRef(B, ground=seen)
    assert ref.on.sum() == cap - 1
    outs = []
    for t in range(T):
        outs.append(ref.step(ticks[t], 2, gait, inp["pos"][t], inp["vel"][t], inp["rot"][t], inp["v_body"],
                             inp["yaw_rate"], inp["thighs"], inp["pos_feet"][t], inp["foot_pos_base"][t],
                             inp["foot_vel_base"][t], inp["jac"], inp["u0"]))
    r = {k: np.stack([x[k] for x in outs]) for k in outs[0]}
    r["mem"] = ref.mem.reshape(B, swing_ref.STRIDE).copy()
    for layout in ("root", "split"):
        out = GS.run_device(eng, inp, gait, ticks, 2, layout=layout)
        GS.assert_matches_ref(out, r, B, tag=layout)
        worst = {k: max(swing_ref.norm_err(out[k][:, b], r[k][:, b]) for b in range(B))
                 for k in ("tau", "pos_target", "vel_target")}
        print(f"\n{layout}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f" (bound {SWING_BOUND:.2e})")
    assert GS.BOUND == SWING_BOUND
    flat = GS.run_device(GS._engine(), inp, gait, ticks, 2, layout="root")
    out = GS.run_device(eng, inp, gait, ticks, 2, layout="root")
    walks_flat = np.r_[nanrow, np.arange(cap, B)]
    on = np.setdiff1d(np.arange(B), walks_flat)
    for k in ("tau", "pos_target", "vel_target", "swing_state"):
        assert same(out[k][:, walks_flat], flat[k][:, walks_flat]), k
        if k != "swing_state":
            assert all(not same(out[k][:, b], flat[k][:, b]) for b in on), k
    assert same(out["mem"][walks_flat], flat["mem"][walks_flat])


@pytest.mark.parametrize("B", [1, 65, 130])
def test_step_and_step_fused_agree_on_tilted_planes(B):
    import test_gpu_step as S
    seq, ref = S.sequence(B), S.reference(B)
    vb, yr = _dev(seq["vb"]), _dev(seq["yr"])
    planes = _dev(_planes(B))
    a, b = S.controller(B), S.controller(B)
    a.engine.set_ground(planes)
    b.engine.set_ground(planes)
    differs = False
    for it in range(S.T):
        rs, ds = _dev(seq["rs"][it]), _dev(seq["ds"][it])
        a.step(it, vb, yr, rs, ds)
        b.step_fused(it, vb, yr, rs, ds, outputs=True)
        torch.cuda.synchronize()
        names = S.names_at(it)
        got = S.snapshot(a, names)
        S.assert_same(S.snapshot(b, names), got, names, ("planes", B, it))
        differs |= not same(got["tau"], ref[it]["tau"])
    assert differs or all(g == "STANDING" for g in S.gait_names(B))      # the planes did change the torques


def test_batched_terrain_with_a_controller():
    """40 ticks of ctl.step followed by ter.update(): every leg is fed the same joint angles and
    the base is pitched and rolled by a rotation of 0.2 rad, so the feet stand on a plane 0.2 rad
    off level.  ter.normal agrees with that plane's normal R e_z within F32_BOUND, and with the
    fit of the controller's own float32 pos_feet too; normal_base is R_base^T n of the
    restatement (R_base the float32 quat2matrix) within F32_BOUND."""
    import kin_ref
    from mpcqp import BatchedTerrain
    from mpcqp.controller import BatchedController
    B, T = 5, 40
    ctl = BatchedController(B, horizon=10, robot="a1", gait="trot10", iterations_between_mpc=2)
    ter = BatchedTerrain(B, controller=ctl)
    assert ter.robot is ctl.robot
    ang = 0.2
    az = np.linspace(0.0, 2.0, B)
    axis = np.stack([np.cos(az), np.sin(az), np.zeros(B)], axis=1)
    quat = np.concatenate([np.full((B, 1), np.cos(ang / 2)), np.sin(ang / 2) * axis], axis=1).astype(np.float32)
    pos = np.tile(np.float32([0.0, 0.0, 0.3]), (B, 1))
    zero = np.zeros((B, 3), np.float32)
    rs = _dev(kin_ref.root_states(quat, pos, zero, zero))
    q = np.tile(np.float32([0.0, 0.8, -1.6]), (B, 4))
    ds = _dev(kin_ref.dof_states(q, np.zeros_like(q)))
    for it in range(T):
        ctl.step(it, [0.3, 0.0, 0.0], 0.0, rs, ds)
        n = ter.update(root_states=rs)
    torch.cuda.synchronize()
    assert n is ter.normal and (ter.status == 0).all() and ter.fitted.all()
    feet = ctl.pos_feet.cpu().numpy()
    assert same(ter.history.cpu().numpy(), feet.astype(np.float64))
    mu, l, nf = tr.fit(feet.astype(np.float64))
    got = ter.normal.cpu().numpy().astype(np.float64)
    q64 = quat.astype(np.float64)
    q64 /= np.linalg.norm(q64, axis=1, keepdims=True)
    w, x, y, z = q64.T
    true = np.stack([2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)], axis=1)
    e_fit, e_true = np.abs(got - nf).max(), np.abs(got - true).max()
    width = np.sqrt(l[:, 1] / 4).min() * 2
    print(f"\nagainst the fit of pos_feet {e_fit:.2e}, against the plane {e_true:.2e}; footprint {width:.3f} m")
    assert width >= 0.24 and abs(np.arccos(true[:, 2]) - ang).max() < 1e-6
    assert e_fit <= F32_BOUND and e_true <= F32_BOUND
    assert same(ctl.robot[:, 9:12].cpu().numpy(), ter.normal.cpu().numpy())
    assert same(ter.plane[:, :3].cpu().numpy(), ter.normal.cpu().numpy())
    nb = ter.normal_base.cpu().numpy().astype(np.float64)
    R32 = swing_ref.quat2matrix_f32(quat).astype(np.float64)
    want = np.einsum("bcr,bc->br", R32, ter.terrain_state[:, tr.N].cpu().numpy())
    e_base = np.abs(nb - want).max()
    print(f"normal_base against R_base^T n {e_base:.2e}, against the body's own z {np.abs(nb - [0.0, 0.0, 1.0]).max():.2e}")
    assert e_base <= F32_BOUND
    ter.reset([1])
    assert (ter.terrain_state[1] == 0).all() and ter.normal[1].tolist() == [0.0, 0.0, 1.0]
    assert ctl.robot[1, 9:12].tolist() == [0.0, 0.0, 1.0]

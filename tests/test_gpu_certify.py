"""GPU: mpcqp_certify -- the gradient G = H U + g of the QP's objective at a force sequence, the
objective and the closed-form duality gap, one wavefront per robot in one launch -- against the
float64 restatement tests/certify_ref.py (pinned on the CPU to the oracle's dense H, g and to its
optimum, tests/test_certify.py), against mpcqp_predict, and after a real solve.  Every output
lies between canary rows and every launch finds them untouched.

Bounds.  The float32 G against certify_ref within F32_BOUND = 2.4e-7 of gscale, the project's
floor for a float32 store.  The float64 report within 10 x the CPU-measured D (tests/test_certify.py):
the objective 10 D_OBJ = 7.5e-15 of |J| + |J_free|, gap / lower / worst 10 D_GAP of gapscale (plus
|J| + |J_free| for lower), and the gap also within 64 eps of certify_ref.gap_rounding_scale, which
stays tight where D_GAP, set by the case at the optimum, is not.  Against mpcqp_predict: 10 (D_J +
D_OBJ) of |cost| + |cost_free|.  After a solve: slack = REF_J_BOUND |phi*| + 10 D_GAP gapscale.
Status, batch tails, refusals' neighbours and graph replays have none: equal / bitwise.

Measured on the MI355X (also DESIGN.md 4.4j; printed by the tests): the float32 G bitwise
certify_ref's in the six cases with random U, 30 of 720 entries apart by at most 2.7e-15 of gscale
at the optimum; the objective 9.2e-16, 2.2e-16, 3.2e-16, 3.6e-16, 2.7e-16, 7.4e-16 and 4.3e-16 of
|J| + |J_free| (mixed, N = 32, N = 1, tilted, optimum, full N = 10 and 32); gap / lower / worst at
most 1.5e-15 of gapscale, 3.0e-9 at the optimum; the gap at most 1.8e-17 of its rounding scale.
The objective is bitwise mpcqp_predict's cost - cost_free (0).  After a real solve: 64 of 64 and
8 of 8 status-OK, the largest gap 1.6e-4 and 2.6e-5 of |objective|; against the restatement's gap
at float32(u*_oracle) the solver's gap is 0.01 .. 0.84 (N = 10, dense classes) and 0.02 .. 0.23
(N = 16, interior point) -- the solver's own float32 U sits on its active rows, the rounded
oracle's does not; lower - phi* between -5.2e-3 and 8.3e-5 under a slack of 1.2e-3 and more.
"""
import ctypes

import numpy as np
import pytest

# torch first: it brings its own HIP runtime, which must be loaded before libmpcqp.so
torch = pytest.importorskip("torch")

import certify_ref as cr  # noqa: E402
import predict_ref as pr  # noqa: E402
from helpers import DEV, _dev, oracle_solution  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = -77.0
PAD = 2
INPUTS = ("x0", "xref", "contact", "feet", "robot")
OUTPUTS = ("G", "report", "status")


def engine(N, Q=cr.Q_DIAG, R=cr.R_DIAG):
    from mpcqp import LinearMpc
    return LinearMpc(horizon=N, robot="a1", Q=Q, R=R, device=DEV)


def buffers(B, N):
    """G, report and status with one canary row ahead of their B rows and PAD behind."""
    rows = 1 + B + PAD
    return dict(G=torch.full((rows, N, 12), CANARY, dtype=torch.float32, device=DEV),
                report=torch.full((rows, 4), CANARY, dtype=torch.float64, device=DEV),
                status=torch.full((rows,), int(CANARY), dtype=torch.int32, device=DEV))


def launch(eng, N, bt, U, skip=(), inputs=None):
    """One mpcqp_certify launch on canary-framed outputs: dict(G, report, status) as NumPy, B rows;
    the outputs named in `skip` are passed as NULL and come back as canaries."""
    B = len(bt["x0"])
    inp = inputs or {k: _dev(bt[k]) for k in INPUTS}
    Ud = U if torch.is_tensor(U) else _dev(U)
    bf = buffers(B, N)
    live = {k: (None if k in skip else v[1:1 + B]) for k, v in bf.items()}
    eng.certify_raw(B, inp["x0"], inp["xref"], inp["contact"], inp["feet"], inp["robot"], Ud, live["G"],
                    live["report"], live["status"])
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in bf.items()}
    for k, v in out.items():
        assert (v[0] == CANARY).all() and (v[1 + B:] == CANARY).all(), k
    return {k: v[1:1 + B] for k, v in out.items()}


def check_against_ref(name, out, case, bitwise=True):
    """`bitwise`: the float32 G is certify_ref's to the bit, as observed wherever U is away from
    the optimum.  At the optimum the gradient cancels to 1e-7 of its terms and a float64 rounding
    moves a float32 store now and then (30 of 720 entries, by 2.7e-15 of gscale)."""
    ref, bt, U = case["ref"], case["bt"], case["U"]
    eg = cr.g_err(out["G"], ref)
    eo, ep = cr.report_err(out["report"], ref)
    fair = float((np.abs(out["report"][:, cr.GAP] - ref["report"][:, cr.GAP]) / cr.gap_rounding_scale(bt, U, ref)).max())
    differ = int((out["G"] != ref["G"]).sum())
    print(f"\n{name}: G {eg:.2e} (bound {cr.F32_BOUND:.1e}; {differ} of {ref['G'].size} entries differ), objective "
          f"{eo:.2e} (bound {10 * cr.D_OBJ:.1e}), gap / lower / worst {ep:.2e} (bound {10 * cr.D_GAP:.1e}), gap over "
          f"its rounding scale {fair:.2e} (bound {64 * 2.0 ** -52:.1e})")
    assert np.array_equal(out["status"], ref["status"])
    assert eg <= cr.F32_BOUND and eo <= 10 * cr.D_OBJ and ep <= 10 * cr.D_GAP and fair <= 64 * 2.0 ** -52
    assert np.array_equal(out["report"][:, cr.LOWER], out["report"][:, cr.OBJECTIVE] - out["report"][:, cr.GAP])
    assert differ == 0 or not bitwise


# ---- the restatement

@pytest.mark.parametrize("name", ["mixed_N10", "long_N32", "short_N1", "tilted_N10", "optimum_N10"])
def test_matches_the_restatement(name):
    """B = 131 with mixed gaits and robots at N = 10, B = 3 at N = 32, B = 2 at N = 1, normals tilted
    by 0.3 rad, and U = float32 of the oracle's optimum; U random otherwise, a quarter of the
    swing entries non-zero, contact values 0.5, -inf and NaN among them."""
    case = cr.gpu_cases()[name]
    out = launch(engine(case["N"]), case["N"], case["bt"], case["U"])
    check_against_ref(name, out, case, bitwise=name != "optimum_N10")
    assert (out["status"] == 0).all() and np.abs(out["G"]).max() > 0


@pytest.mark.parametrize("name", ["full_N10", "full_N32"])
def test_full_weights_match_the_restatement(name):
    """A full Q and an R coupling every pair of legs (mpcqp_set_weights), at N = 10 and at N = 32,
    the kernel's two full-weight instantiations."""
    case = cr.gpu_cases()[name]
    N = case["N"]
    out = launch(engine(N, case["Q"], case["R"]), N, case["bt"], case["U"])
    check_against_ref(name, out, case)
    diag = launch(engine(N), N, case["bt"], case["U"])
    assert not np.array_equal(diag["G"], out["G"]) and not np.array_equal(diag["report"], out["report"])


# ---- the tail of a batch, misaligned, with NaN around the slice

def test_misaligned_slice_of_a_larger_allocation():
    """mixed_N10's 131 robots as the slice that starts one robot into an allocation of 133: x0 (13
    floats a robot), robot (16, moved by one float more) and U start off a 16-byte boundary,
    and everything outside the slice is NaN."""
    case = cr.gpu_cases()["mixed_N10"]
    N, bt, U = 10, case["bt"], case["U"]
    B = len(U)
    eng = engine(N)
    want = launch(eng, N, bt, U)

    def inside(a, shift=0):
        a = np.ascontiguousarray(a, np.float32)
        per = a[0].size
        buf = torch.full(((B + 2) * per + 4,), float("nan"), dtype=torch.float32, device=DEV)
        v = buf[per + shift:per + shift + B * per].view(a.shape)
        v.copy_(torch.as_tensor(a))
        assert v.is_contiguous()
        return v

    inp = {k: inside(bt[k], shift=1 if k == "robot" else 0) for k in INPUTS}
    Ud = inside(U, shift=1)
    for t in (inp["x0"], inp["robot"], Ud):
        assert t.data_ptr() % 16 != 0
    got = launch(eng, N, bt, Ud, inputs=inp)
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k


# ---- pointers

def test_each_output_null_in_turn_and_all_null():
    case = cr.gpu_cases()["long_N32"]
    N, bt, U = 32, case["bt"], case["U"]
    eng = engine(N)
    want = launch(eng, N, bt, U)
    for skip in OUTPUTS:
        got = launch(eng, N, bt, U, skip=(skip,))
        for k in want:
            assert (got[k] == CANARY).all() if k == skip else got[k].tobytes() == want[k].tobytes(), (skip, k)
    got = launch(eng, N, bt, U, skip=OUTPUTS)      # MPCQP_OK, nothing launched
    assert all((v == CANARY).all() for v in got.values())


def test_argument_refusals():
    from mpcqp import _lib
    case = cr.gpu_cases()["short_N1"]
    eng = engine(1)
    inp = [_dev(case["bt"][k]) for k in INPUTS] + [_dev(case["U"])]
    bf = buffers(2, 1)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    outs = [bf[k][1:3] for k in OUTPUTS]
    call = lambda B, flags, ins: eng.lib.mpcqp_certify(eng._ctx, B, flags, *[p(t) for t in ins], *[p(t) for t in outs], None)
    assert call(2, 1, inp) == _lib.ERR_ARG and b"flags" in eng.lib.mpcqp_last_error(eng._ctx)
    assert call(-1, 0, inp) == _lib.ERR_ARG
    for i in range(6):
        assert call(2, 0, inp[:i] + [None] + inp[i + 1:]) == _lib.ERR_ARG, i
    assert call(0, 0, inp) == _lib.MPCQP_OK
    torch.cuda.synchronize()
    for k in OUTPUTS:
        assert (bf[k] == CANARY).all(), k
    with pytest.raises(ValueError):
        eng.certify_raw(2, *inp[:5], inp[5].double(), outs[0])
    with pytest.raises(ValueError):
        eng.certify_raw(3, *inp, outs[0])


# ---- non-finite inputs

@pytest.mark.parametrize("what", ["x0", "U", "mass"])
def test_one_bad_robot_in_nine(what):
    """Robot 4 of 9 gets a NaN x0, a +inf U entry or mass 0 (finite inputs, 1 / m is not): its
    status is NONFINITE and its outputs zeros; the eight others are bitwise as without it."""
    case = cr.gpu_cases()["tilted_N10"]
    N, B, bad = 10, 9, 4
    bt = {k: v.copy() for k, v in case["bt"].items()}
    U = case["U"].copy()
    eng = engine(N)
    clean = launch(eng, N, bt, U)
    if what == "x0":
        bt["x0"][bad, 7] = np.nan
    elif what == "U":
        U[bad, 6, 5] = np.inf
    else:
        bt["robot"][bad, 0] = 0.0
    out = launch(eng, N, bt, U)
    ref = cr.certify_batch(N, bt, U)
    keep = np.setdiff1d(np.arange(B), [bad])
    assert out["status"][bad] == cr.STATUS_NONFINITE and (out["status"][keep] == 0).all()
    assert np.array_equal(out["status"], ref["status"])
    assert (out["G"][bad] == 0).all() and (out["report"][bad] == 0).all()
    for k in out:
        assert out[k][keep].tobytes() == clean[k][keep].tobytes(), k


# ---- mpcqp_predict

@pytest.mark.parametrize("name", ["mixed_N10", "full_N32", "optimum_N10"])
def test_objective_is_predicts_cost_minus_cost_free(name):
    """Measured: 0 in all three cases (the kernel sums J and J_free as mpcqp_predict does)."""
    case = cr.gpu_cases()[name]
    N, bt, U = case["N"], case["bt"], case["U"]
    B = len(U)
    eng = engine(N, case["Q"], case["R"])
    out = launch(eng, N, bt, U)
    prd = eng.predict(bt["x0"], bt["xref"], bt["contact"], bt["feet"], U, robot=bt["robot"])
    torch.cuda.synchronize()
    rep = prd.report.cpu().numpy()
    assert (prd.status.cpu().numpy() == 0).all() and (out["status"] == 0).all() and len(rep) == B
    err = np.abs(out["report"][:, cr.OBJECTIVE] - (rep[:, pr.COST] - rep[:, pr.COST_FREE])) \
        / (np.abs(rep[:, pr.COST]) + np.abs(rep[:, pr.COST_FREE]))
    print(f"\n{name}: objective against cost - cost_free {err.max():.2e} (bound {10 * (pr.D_J + cr.D_OBJ):.1e})")
    assert err.max() <= 10 * (pr.D_J + cr.D_OBJ)


# ---- after a real solve: the check ADVICE asks for

@pytest.mark.parametrize("B,N,gaits", [(64, 10, ("trot10", "pace10", "bound8", "standing")), (8, 16, ("standing",))])
def test_after_a_real_solve(B, N, gaits):
    """solve, then predict and certify on its U: B = 64, N = 10, mixed gaits (the dense classes) and
    B = 8, N = 16, all standing (64 stance foot-steps: the interior-point class).  For a status-OK
    robot inside its cones to 1e-4, lower <= phi*_oracle + slack, and the gap is at most 10 x the
    restatement's gap at float32(u*_oracle) plus 10 D_GAP gapscale: the solver's U differs from
    the oracle's by up to 1e-5 relative.  The oracle is solved for three robots of each batch."""
    from mpcqp.synthetic import make_batch
    bt = make_batch(B, N, seed=170 + N, gaits=gaits, robots=("a1", "aliengo"))
    eng = engine(N)
    res = eng.solve(bt["x0"], bt["xref"], bt["contact"], bt["feet"], robot=bt["robot"], return_all=True)
    prd = eng.predict(bt["x0"], bt["xref"], bt["contact"], bt["feet"], res.U, robot=bt["robot"])
    crt = eng.certify(bt["x0"], bt["xref"], bt["contact"], bt["feet"], res.U, robot=bt["robot"])
    torch.cuda.synchronize()
    prep, rep = prd.report.cpu().numpy(), crt.report.cpu().numpy()
    assert np.array_equal(rep[:, cr.GAP], crt.gap.cpu().numpy()) and crt.lower.data_ptr() == crt.report.data_ptr() + 16
    assert (crt.status.cpu().numpy() == 0).all()
    ok = (res.status.cpu().numpy() == 0) & (prep[:, pr.MARGIN] >= -1e-4)
    assert ok.sum() >= B - 2
    print(f"\nB={B} N={N}: status-OK {ok.sum()}, largest gap / |objective| {(rep[ok, cr.GAP] / np.abs(rep[ok, cr.OBJECTIVE])).max():.2e}")
    U = res.U.cpu().numpy()
    ratios = []
    for b in np.flatnonzero(ok)[:3]:
        x, o, _ = oracle_solution(bt, b, N)
        phis = 0.5 * x @ o["H"] @ x + o["g"] @ x
        args = (bt["x0"][b], bt["xref"][b], bt["contact"][b], bt["feet"][b], bt["robot"][b])
        at_opt = cr.certify_robot(N, *args, x.astype(np.float32))
        mine = cr.certify_robot(N, *args, U[b])
        slack = cr.REF_J_BOUND * abs(phis) + 10 * cr.D_GAP * mine["gapscale"]
        ratios.append(rep[b, cr.GAP] / at_opt["report"][cr.GAP])
        print(f"robot {b}: gap {rep[b, cr.GAP]:.3e}, at float32(u*) {at_opt['report'][cr.GAP]:.3e} (ratio {ratios[-1]:.2f}), "
              f"lower - phi* {rep[b, cr.LOWER] - phis:.3e}, slack {slack:.3e}, phi* {phis:.3e}")
        assert rep[b, cr.LOWER] <= phis + slack
        assert rep[b, cr.GAP] <= 10 * at_opt["report"][cr.GAP] + 10 * cr.D_GAP * mine["gapscale"]
    print(f"gap of the solver's U over the gap at float32(u*_oracle): {min(ratios):.2f} .. {max(ratios):.2f}")


# ---- graph

def test_graph_replay_equals_the_eager_call():
    """bind_certify captured on a side stream and replayed three times over U changed in place."""
    case = cr.gpu_cases()["mixed_N10"]
    N, B = 10, 65
    bt = {k: v[:B] for k, v in case["bt"].items()}
    eng = engine(N)
    inp = {k: _dev(bt[k]) for k in INPUTS}
    Ud = _dev(case["U"][:B])
    bf = buffers(B, N)
    fn = eng.bind_certify(B, inp["x0"], inp["xref"], inp["contact"], inp["feet"], inp["robot"], Ud,
                          bf["G"][1:1 + B], bf["report"][1:1 + B], bf["status"][1:1 + B])
    assert any(t is Ud for t in fn.buffers)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fn(s)
    seen = set()
    for r, seed in enumerate((1, 2, 3)):
        U = pr.random_u(bt, 900 + seed)
        Ud.copy_(_dev(U))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in bf.items()}
        eager = launch(eng, N, bt, U, inputs=inp)
        for k in eager:
            assert got[k][1:1 + B].tobytes() == eager[k].tobytes(), (r, k)
            assert (got[k][0] == CANARY).all() and (got[k][1 + B:] == CANARY).all()
        seen.add(got["G"].tobytes())
    assert len(seen) == 3


# ---- the drop-in

def test_shim_optimality_gap_is_certify_on_the_tick_buffers():
    import test_shim as ts
    m = ts._shim()
    c = m.ModelPredictiveController(ts.LinearMpcConfig, ts.AliengoConfig)
    with pytest.raises(RuntimeError):
        c.optimality_gap()
    rd = ts.FakeRobotData()
    c.update_robot_state(rd)
    with pytest.raises(RuntimeError):
        c.optimality_gap()
    table = np.tile(np.array([1, 0, 0, 1], np.float32), 10)
    c.update_mpc_if_needed(0, np.array([0.8, 0.0, 0.0]), 0.1, table)
    objective, gap = c.optimality_gap()
    assert type(objective) is float and type(gap) is float
    dv, up, eng = c._dev, c._up_views, c._engine
    res = eng.certify(dv["x0"], dv["xref"], up["contact"].reshape(1, 10, 4), up["feet"], dv["U"].reshape(1, 10, 12),
                      robot=dv["robot"])
    torch.cuda.synchronize()
    assert int(res.status[0]) == 0 and objective == float(res.objective[0]) and gap == float(res.gap[0])
    assert c.optimality_gap() == (objective, gap)             # the bound launch, a second time
    # an optimum: below U = 0, and the gap small against it
    print(f"\noptimality_gap(): objective {objective:.4e}, gap {gap:.3e}")
    assert objective < 0 and abs(gap) <= 1e-2 * abs(objective)

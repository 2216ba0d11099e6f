"""mpcqp_solve at its input boundary, in every capacity class: input slices at every 16-byte
alignment among NaN words, output views inside canaries, nullable outputs, non-finite values
at the first and last element of every checked slice, finite records whose result is not
finite, contact values other than 0 and 1, degenerate cones and bounds, and the iteration cap
beyond class 64.

Each class is taken directly through ``set_stance_range`` (its own ``form_stage`` stages the
inputs), at the smallest shape that reaches its kernel, four robots per call:

  c64    N = 10 trot, n = 60, no range            class 64
  c96    N = 16 trot, n = 96, range (32, 32)      class 96
  c128   N = 16 trot with its first 5 steps full stance, n = 126, range (33, 42)   class 128
  ipm16  N = 16 standing, n = 192, range (43, 64)  interior point, 16-stage layout
  ipm20  N = 20 standing, n = 240, range (80, 80)  interior point, 20-stage layout
  ipm32  N = 24 trot, n = 144, no range            interior point, 32-stage layout (N > 20)
  mixed  N = 16, n = 60 / 96 / 126 / 192 / 114, no range: class 64 stages and routes every
         robot, the queued classes stage their own again

The oracle (float64, CPU) solves every parity case once per process; the builders' asserts
(stance counts, binding bound rows) and those solves are the unmarked test of this file."""
import functools
import math

import numpy as np
import pytest

from helpers import oracle_solution, rel_err_u0

TOL_U0 = 1e-4             # test_gpu_parity.TOL_U0: the project's contract (1e-3 floor on the denominator)
TOL_ACHIEVED = 1e-5       # test_gpu_parity.TOL_ACHIEVED: the dense classes' regression guard
TOL_ACHIEVED_IPM = 5e-5   # test_gpu_parity.TOL_ACHIEVED_IPM: the interior-point class's
NONFINITE = 4             # MPCQP_STATUS_NONFINITE

# name -> (N, stance range, what is done to a trot batch's contact table, stance foot-steps)
SPECS = {
    "c64": (10, (0, 0), None, 20),
    "c96": (16, (32, 32), None, 32),
    "c128": (16, (33, 42), "full5", 42),
    "ipm16": (16, (43, 64), "standing", 64),
    "ipm20": (20, (80, 80), "standing", 80),
    "ipm32": (24, (0, 0), None, 48),
}
DENSE = ("c64", "c96", "c128")
IPM = ("ipm16", "ipm20", "ipm32")
CLASSES = DENSE + IPM
MIXED_STANCE = (20, 32, 42, 64, 38)
# E's standing robot of the dense classes: N = 10 standing is n = 120, class 128 directly
STAND10 = (10, (33, 40), "standing", 40)
SEED = 7100


def _guard(name):
    return TOL_ACHIEVED_IPM if name in IPM else TOL_ACHIEVED


def _copy(bt):
    return {k: v.copy() for k, v in bt.items()}


def _stance(bt):
    return (bt["contact"] > 0).reshape(len(bt["x0"]), -1).sum(1)


def _shape(bt, how):
    if how == "full5":
        bt["contact"][:, :5, :] = 1.0
    elif how == "standing":
        bt["contact"][:] = 1.0
    return bt


@functools.lru_cache(maxsize=None)
def _base(name):
    """The class's four robots (``mixed``: five, one per class and an n = 114 one)."""
    from mpcqp.synthetic import make_batch
    if name == "mixed":
        bt = make_batch(5, 16, seed=SEED + 50, gaits=("trot10",), robots=("a1",))
        bt["contact"][0, 10:, :] = 0.0    # n = 60: class 64
        bt["contact"][2, :5, :] = 1.0     # n = 126: class 128
        bt["contact"][3] = 1.0            # n = 192: interior point
        bt["contact"][4, :3, :] = 1.0     # n = 114: class 128
        assert tuple(_stance(bt)) == MIXED_STANCE
        return bt
    N, _, how, stance = STAND10 if name == "stand10" else SPECS[name]
    seed = SEED + 10 * (list(SPECS).index(name) if name in SPECS else 9)
    bt = _shape(make_batch(4, N, seed=seed, gaits=("trot10",), robots=("a1",)), how)
    assert (_stance(bt) == stance).all(), (name, _stance(bt))
    return bt


def _horizon(name):
    return 16 if name == "mixed" else (STAND10 if name == "stand10" else SPECS[name])[0]


def _oracle(bt, robots, N):
    return {b: oracle_solution(bt, b, N)[0] for b in robots}


@functools.lru_cache(maxsize=None)
def _base_ref(name):
    bt = _base(name)
    return _oracle(bt, range(len(bt["x0"])), _horizon(name))


# ---- D: contact as a number.  Case -> the table's change; the oracle solves all four robots.
def _contact_cases(name):
    out = {}
    for key in ("x0.08", "x2", "mixed"):
        bt = _copy(_base(name))
        if key == "x0.08":
            bt["contact"] *= np.float32(0.08)          # ub = 40 N: the fz <= ub row binds
        elif key == "x2":
            bt["contact"] *= np.float32(2.0)
        else:
            bt["contact"][:, ::2] *= np.float32(0.05)
            bt["contact"][:, 1::3] *= np.float32(0.5)
        assert (_stance(bt) == _stance(_base(name))).all()
        out[key] = bt
    return out


@functools.lru_cache(maxsize=None)
def _contact_refs(name):
    N = _horizon(name)
    out = {}
    for key, bt in _contact_cases(name).items():
        xs, binding = {}, 0
        for b in range(4):
            x, o, _ = oracle_solution(bt, b, N)
            ub = o["ub"][4::5].astype(np.float64)      # the oracle's own contact * fz_max
            binding += int(np.sum((ub > 0) & (np.abs(x.reshape(-1, 3)[:, 2] - ub) < 1e-6)))
            xs[b] = x
        if key == "x0.08":
            assert binding >= 1, (name, binding)       # the case really exercises the bound rows
        out[key] = (bt, xs)
    return out


# ---- E: degenerate cones and bounds
# mu0lift: mu = 0 with the base moving up at 1 m/s, so that the n.f >= 0 row -- a real row only
# when mu = 0 -- binds in every class (with mu = 0 alone it binds in some: the robots mostly push)
E_CASES = ("mu0", "mu1e-3", "fzmax0", "contact1e-30", "mu0lift")


def _e_cases(name):
    return ("mu0", "mu0lift") if name == "stand10" else E_CASES


def _degenerate(bt, key):
    bt = _copy(bt)
    if key in ("mu0", "mu0lift"):
        bt["robot"][:, 7] = 0.0
        if key == "mu0lift":
            bt["x0"][:, 11] = 1.0
    elif key == "mu1e-3":
        bt["robot"][:, 7] = 1e-3
    elif key == "fzmax0":
        bt["robot"][:, 8] = 0.0
    else:
        bt["contact"] *= np.float32(1e-30)
    return bt


@functools.lru_cache(maxsize=None)
def _degenerate_refs(name):
    """case -> (batch, {robot: optimum}), two robots per case.  ``stand10``: standing with mu = 0
    only (the standing interior-point classes' mu0 cases are standing with mu = 0 already)."""
    N = _horizon(name)
    out = {}
    for i, key in enumerate(_e_cases(name)):
        bt = _degenerate(_base(name), key)
        b0 = (i + (CLASSES.index(name) if name in CLASSES else 0)) % 2
        xs = _oracle(bt, (b0, b0 + 2), N)
        for x in xs.values():
            assert np.isfinite(x).all()
            if key in ("mu0", "mu0lift"):
                assert np.abs(x.reshape(-1, 3)[:, :2]).max() < 1e-9    # no tangential force at all
            if key in ("fzmax0", "contact1e-30"):
                assert np.abs(x).max() < 1e-9                          # every bound active at f = 0
        if key == "mu0lift":   # the n.f >= 0 row binds on a stance foot-step of each robot
            for b, x in xs.items():
                stance = bt["contact"][b].reshape(-1) > 0
                assert np.sum(stance & (np.abs(x.reshape(-1, 3)[:, 2]) < 1e-9)) >= 1, (name, b)
        out[key] = (bt, xs)
    return out


def test_cases_are_what_they_claim():
    """The builders' asserts (stance counts per class, a binding fz <= ub row in every 40 N
    case, the degenerate optima's shape) and the oracle's solve of every A / D / E case."""
    for name in CLASSES + ("mixed",):
        ref = _base_ref(name)
        assert all(np.isfinite(x).all() for x in ref.values()), name
    for name in CLASSES:
        assert all(np.isfinite(x).all() for _, xs in _contact_refs(name).values() for x in xs.values()), name
    for name in CLASSES + ("stand10",):
        _degenerate_refs(name)


def test_oracle_refuses_the_records_without_a_finite_result():
    """mass 0, an all-zero inertia and a normal along world x have no parity value: the oracle
    raises or returns a non-finite optimum, so the device tests hold only the status contract."""
    bt = _base("c64")
    for key in C_RECORDS:
        bad = _nonfinite_result_record(bt, 1, key)
        try:
            with np.errstate(all="ignore"):
                x = oracle_solution(bad, 1, 10)[0]
        except Exception:
            continue
        assert not np.isfinite(x).all(), key


# ------------------------------------------------------------------ device side
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _same(a, b):
    """Bitwise equality of two results (u0, U, status, iters) or arrays."""
    if isinstance(a, tuple):
        return all(_same(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _engine(name, max_iter=0):
    from mpcqp import LinearMpc
    spec = STAND10 if name == "stand10" else SPECS.get(name)
    eng = LinearMpc(horizon=_horizon(name), robot="a1", max_iter=max_iter)
    if spec is not None and spec[1] != (0, 0):
        eng.set_stance_range(*spec[1])
    return eng


def _solve(eng, bt):
    import torch
    res = eng.solve(bt["x0"], bt["xref"], bt["contact"], bt["feet"], robot=bt["robot"], return_all=True)
    torch.cuda.synchronize()
    B = len(bt["x0"])
    return (res.u0.cpu().numpy(), res.U.cpu().numpy().reshape(B, -1), res.status.cpu().numpy(),
            res.iterations.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _clean(name):
    """The class's base batch solved the ordinary way -- fresh, aligned, finite tensors -- and
    held to the oracle, so that "bitwise the clean call" below means "right"."""
    out = _solve(_engine(name), _base(name))
    assert (out[2] == 0).all(), (name, out[2])
    err = _worst(out[0], out[1], _base_ref(name))
    print(f"{name}: clean batch, worst relative error {err:.2e}, iterations {out[3].tolist()}")
    assert err < (TOL_ACHIEVED_IPM if name == "mixed" else _guard(name)), (name, err)
    return out


INPUTS = ("x0", "xref", "contact", "feet", "robot")
F_CANARY, I_CANARY = -12345.5, 0x5A5A5A5A


def _raw(eng, bt, in_off=(0, 0, 0, 0, 0), out_off=None, null=()):
    """solve_raw on views: input i starts 4 + in_off[i] floats into a NaN-filled tensor (so
    there are NaN words on both sides of the batch at every alignment), robot fields 12..15
    are NaN, and with ``out_off`` each output starts that many elements into a canary-filled
    tensor.  Returns (u0, U, status, iters) -- None for the outputs in ``null`` -- and the
    canary words around the outputs."""
    import torch
    B, N = len(bt["x0"]), bt["xref"].shape[1]
    views = []
    for key, k in zip(INPUTS, in_off):
        a = np.ascontiguousarray(bt[key], dtype=np.float32).copy()
        if key == "robot":
            a[:, 12:16] = np.nan
        flat = torch.from_numpy(a.reshape(-1))
        buf = torch.full((flat.numel() + 16,), float("nan"), dtype=torch.float32, device="cuda:0")
        assert buf.data_ptr() % 16 == 0
        buf[4 + k:4 + k + flat.numel()] = flat.to("cuda:0")
        views.append((buf, buf[4 + k:4 + k + flat.numel()]))
    outs, guards = [], []
    for key, numel, dt, canary in (("u0", B * 12, torch.float32, F_CANARY), ("U", B * N * 12, torch.float32, F_CANARY),
                                   ("status", B, torch.int32, I_CANARY), ("iters", B, torch.int32, I_CANARY)):
        if key in null:
            outs.append(None)
            continue
        k = 0 if out_off is None else out_off
        buf = torch.full((numel + 8,), canary, dtype=dt, device="cuda:0")
        outs.append(buf[k:k + numel])
        guards.append((buf, k, numel, canary))
    eng.solve_raw(B, *(v for _, v in views), *outs)
    torch.cuda.synchronize()
    for buf, k, numel, canary in guards:
        host = buf.cpu().numpy()
        rest = np.concatenate([host[:k], host[k + numel:]])
        assert len(rest) == 8 and (rest == np.asarray(canary, dtype=host.dtype)).all(), "a word outside an output was written"
    u0, U, st, it = (None if t is None else t.cpu().numpy() for t in outs)
    return (None if u0 is None else u0.reshape(B, 12), None if U is None else U.reshape(B, -1), st, it)


# ---- A: slices at every alignment, poisoned surroundings
@pytest.mark.gpu
@pytest.mark.parametrize("name", CLASSES + ("mixed",))
def test_input_slices_at_every_alignment_among_nan(name):
    """Every input at 0..3 floats past a 16-byte boundary (the same offset for all five, then
    five different ones), NaN before the first and after the last robot's slice and in robot
    fields 12..15: bitwise the aligned, finite-padded call, status 0.  An off-by-one in the
    staging's chunk count, first index or slice length reads one of those NaN words."""
    eng, bt, ref = _engine(name), _base(name), _clean(name)
    for off in ((0,) * 5, (1,) * 5, (2,) * 5, (3,) * 5, (1, 3, 0, 2, 3), (3, 2, 1, 0, 1)):
        got = _raw(eng, bt, in_off=off)
        assert (got[2] == 0).all(), (name, off, got[2])
        assert _same(got, ref), (name, off)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLASSES + ("mixed",))
def test_output_views_inside_canaries(name):
    """u0, U, status and iters at 1..3 elements into canary-filled tensors: the words around
    them are untouched (checked in _raw) and the results bitwise the reference call's."""
    eng, bt, ref = _engine(name), _base(name), _clean(name)
    for off in (1, 2, 3):
        assert _same(_raw(eng, bt, in_off=(off,) * 5, out_off=off), ref), (name, off)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLASSES + ("mixed",))
def test_nullable_outputs(name):
    """U, status and iters each NULL, then all three: u0 and the outputs still given are
    bitwise unchanged."""
    eng, bt, ref = _engine(name), _base(name), _clean(name)
    for null in (("U",), ("status",), ("iters",), ("U", "status", "iters")):
        got = _raw(eng, bt, null=null)
        for g, r in zip(got, ref):
            assert g is None or _same(g, r), (name, null)
        assert got[0] is not None and [g is None for g in got[1:]] == [k in null for k in ("U", "status", "iters")]


def _check_refused(name, bad, robots, what):
    """``robots`` of the batch ``bad`` report NONFINITE with u0 / U = 0 and iters 0; every other
    robot is bitwise what it is in the clean batch; nothing non-finite leaves the solve."""
    u0, U, st, it = _solve(_engine(name), bad)
    ref = _clean(name)
    assert np.isfinite(u0).all() and np.isfinite(U).all(), (name, what)
    for b in range(len(st)):
        if b in robots:
            assert st[b] == NONFINITE, (name, what, b, st)
            assert not u0[b].any() and not U[b].any() and it[b] == 0, (name, what, b, it[b])
        else:
            assert _same(tuple(x[b] for x in (u0, U, st, it)), tuple(x[b] for x in ref)), (name, what, b)


# ---- B: non-finite inputs at the slice edges
@pytest.mark.gpu
@pytest.mark.parametrize("name", CLASSES + ("mixed",))
def test_nonfinite_at_the_first_and_last_element_of_every_checked_slice(name):
    """NaN, +inf and -inf at the first and the last element of robot 1's x0, feet, xref and
    robot[0:12] -- the positions the chunk logic can lose: status 4, zero outputs, the
    neighbours bitwise untouched.  One engine per class.  (``mixed``: robot 1 is the class-96
    robot, refused by class 64's routing pass; then the interior-point robot, 3.)"""
    base = _base(name)
    for b in (1, 3) if name == "mixed" else (1,):
        for key, last in (("x0", 12), ("feet", 11), ("xref", 13 * _horizon(name) - 1), ("robot", 11)):
            for pos in (0, last):
                for val in (np.nan, np.inf, -np.inf):
                    bad = _copy(base)
                    bad[key][b].reshape(-1)[pos] = val
                    _check_refused(name, bad, (b,), (key, pos, val))


# ---- C: finite inputs, non-finite result
C_RECORDS = ("mass0", "inertia0", "normal+x", "normal-x")


def _nonfinite_result_record(bt, b, key):
    bad = _copy(bt)
    if key == "mass0":
        bad["robot"][b, 0] = 0.0
    elif key == "inertia0":
        bad["robot"][b, 1:7] = 0.0
    else:
        bad["robot"][b, 9:12] = (1.0 if key == "normal+x" else -1.0, 0.0, 0.0)
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLASSES + ("mixed",))
def test_finite_record_without_a_finite_result_is_refused(name):
    """mass = 0 (1 / m = inf), an all-zero inertia (det = 0) and a surface normal along world
    +-x (its tangent frame is 0 / 0): MPCQP_STATUS_NONFINITE with u0 / U = 0, never a NaN under
    a status that promises a usable iterate; the neighbours bitwise untouched.  The loops are
    bounded (the active set by max_iter, the interior point by its 60 iterations and fixed
    correction counts), so these solves terminate."""
    base = _base(name)
    for b in range(len(base["x0"])) if name == "mixed" else (1,):
        for key in C_RECORDS:
            _check_refused(name, _nonfinite_result_record(base, b, key), (b,), (key, b))


def _tilted(bt, deg=15.0, az=0.7):
    bt = _copy(bt)
    th = math.radians(deg)
    bt["robot"][:, 9:12] = (math.sin(th) * math.cos(az), math.sin(th) * math.sin(az), math.cos(th))
    return bt


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLASSES)
def test_normal_is_normalised(name):
    """normal = (0, 0, 0) is bitwise normal = (0, 0, 1) (the guard in form_model); twice the
    normal is bitwise the normal, flat and tilted by 15 degrees (a power-of-two scale is exact
    through the normalisation); three times the tilted normal -- float32 rounds each entry, a
    6e-8 change of direction -- stays within the class's achieved tolerance of the oracle."""
    eng, base, ref = _engine(name), _base(name), _clean(name)
    assert (base["robot"][:, 9:12] == (0.0, 0.0, 1.0)).all()
    zero = _copy(base)
    zero["robot"][:, 9:12] = 0.0
    assert _same(_solve(eng, zero), ref), name
    tilt = _tilted(base)
    tref = _solve(eng, tilt)
    assert (tref[2] == 0).all(), tref[2]
    for bt, r in ((base, ref), (tilt, tref)):
        two = _copy(bt)
        two["robot"][:, 9:12] *= np.float32(2.0)
        assert _same(_solve(eng, two), r), name
    three = _copy(tilt)
    three["robot"][:, 9:12] *= np.float32(3.0)
    u0, U, st, _ = _solve(eng, three)
    b = CLASSES.index(name) % 4
    x = oracle_solution(three, b, _horizon(name))[0]
    err = max(rel_err_u0(u0[b], x[:12]), rel_err_u0(U[b], x))
    print(f"{name}: 3 x tilted normal, robot {b}: {err:.2e}")
    assert (st == 0).all() and err < _guard(name), (name, err)


def _worst(u0, U, xs):
    """Worst rel_err_u0 of u0 and of U over the robots the oracle solved."""
    return max(max(rel_err_u0(u0[b], x[:12]), rel_err_u0(U[b], x)) for b, x in xs.items())


# ---- D: contact as a number
def _cone_ok(bt, U):
    """fz >= -tol, |f_t| <= mu fz + tol and fz <= ub + tol in the robot's (t1, t2, n) frame, swing
    GRFs exactly 0 (tolerances as in test_gpu_parity.test_full_size_properties)."""
    B, N = len(bt["x0"]), bt["xref"].shape[1]
    f = U.reshape(B, N, 4, 3).astype(np.float64)
    c = bt["contact"]
    assert np.all(f[~(c > 0)] == 0)
    nrm = bt["robot"][:, 9:12].astype(np.float64)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    t1 = np.array([1.0, 0.0, 0.0])[None, :] - nrm[:, :1] * nrm
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(nrm, t1)
    fn, f1, f2 = (np.einsum("bnlk,bk->bnl", f, v) for v in (nrm, t1, t2))
    mu = bt["robot"][:, 7].astype(np.float64)[:, None, None]
    ub = np.where(c > 0, c.astype(np.float64) * bt["robot"][:, 8].astype(np.float64)[:, None, None], 0.0)
    tol = 1e-4 * (1.0 + np.abs(f).max(axis=(1, 2, 3)))[:, None, None]
    assert np.all(fn >= -tol) and np.all(fn <= ub + tol)
    assert np.all(np.abs(f1) <= mu * fn + tol) and np.all(np.abs(f2) <= mu * fn + tol)


# The achieved-precision guards are relative to ||u*||_inf of full 500 N bounds.  A table scaled
# by s caps the forces, and with them the metric's denominator, at s x 500 N, while the
# rounding error comes from H and g, which the table does not change: the guard of a scaled
# case is the class's guard / s (s: the scale of the first step's bound, u0's denominator),
# capped at the contract.  That is the contract itself for x 0.08 and the mixed table (measured
# there: up to 1.7e-5 relative, 3e-5 to 7e-4 N absolute -- the x 2 cases' absolute error is 3e-5
# to 3e-4 N), and the class's guard for x 2, which caps nothing.
D_BOUND_SCALE = {"x0.08": 0.08, "x2": 1.0, "mixed": 0.05}


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLASSES)
def test_contact_scales_the_bound(name):
    """contact x 0.08 (ub = 40 N, at least one fz <= ub row binding), x 2 and a mixed table
    (every second step x 0.05, every third x 0.5) against the oracle, whose ub is
    contact * fz_max as well."""
    eng = _engine(name)
    for key, (bt, xs) in _contact_refs(name).items():
        u0, U, st, _ = _solve(eng, bt)
        assert (st == 0).all(), (name, key, st)
        _cone_ok(bt, U)
        err = _worst(u0, U, xs)
        absolute = max(float(np.abs(U[b] - x).max()) for b, x in xs.items())
        print(f"{name} contact {key}: worst relative error {err:.2e}, absolute {absolute:.2e} N")
        assert err < min(TOL_U0, _guard(name) / D_BOUND_SCALE[key]), (name, key, err)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLASSES + ("mixed",))
def test_contact_that_is_not_positive_is_swing(name):
    """NaN, -1 and -inf contact entries are swing foot-steps: bitwise the same table with 0
    there, status 0.  A +inf entry would be an infinite bound: that robot is refused (status
    4, zero outputs), its neighbours bitwise untouched."""
    eng, base = _engine(name), _base(name)
    N = _horizon(name)
    where = [(0, 0, 0), (1, N - 1, 3), (2, N // 2, 1), (3, 1, 2)]   # (robot, step, leg), each in stance
    zero = _copy(base)
    for b, t, leg in where:
        stance_legs = np.flatnonzero(base["contact"][b, t] > 0)
        leg = int(stance_legs[leg % len(stance_legs)])
        zero["contact"][b, t, leg] = 0.0
    ref = _solve(eng, zero)
    assert (ref[2] == 0).all(), ref[2]
    for val in (np.nan, -1.0, -np.inf):
        bad = _copy(base)
        bad["contact"][zero["contact"] != base["contact"]] = val
        assert _same(_solve(eng, bad), ref), (name, val)
    for b, pos in ((1, 0), (2, 4 * N - 1)) + (((3, 5),) if name == "mixed" else ()):
        bad = _copy(base)
        bad["contact"][b].reshape(-1)[pos] = np.inf   # first / last element of the slice, stance or not
        _check_refused(name, bad, (b,), ("contact +inf", pos))


# ---- E: degenerate cones and bounds
# Worst relative error measured on the MI355X per class and case (_e_cases' order), robots and
# metric as below (max of u0's and U's rel_err_u0; with every force 0
# the metric's 1e-3 floor makes it the absolute error in mN); the guard is 10 x that, capped at
# TOL_U0.  Every case ended with status 0: no degenerate active set cycled (the dense classes
# take 82-336 steps for fz_max = 0, every bound row entering the set).
E_MEASURED = {
    "c64": (4.42e-07, 5.73e-07, 1.30e-08, 6.88e-09, 5.79e-07),
    "c96": (6.12e-07, 7.85e-07, 1.28e-07, 1.81e-07, 1.99e-06),
    "c128": (1.58e-06, 1.14e-06, 3.65e-07, 1.86e-07, 1.27e-06),
    "ipm16": (1.32e-06, 2.14e-06, 4.13e-09, 2.50e-09, 1.05e-06),
    "ipm20": (1.01e-06, 2.14e-06, 1.46e-08, 9.23e-09, 1.90e-06),
    "ipm32": (1.02e-06, 1.17e-06, 5.75e-09, 8.70e-09, 1.24e-06),
    "stand10": (4.32e-07, 5.58e-07),
}


def _e_guard(name, key):
    return min(TOL_U0, 10.0 * E_MEASURED[name][_e_cases(name).index(key)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLASSES + ("stand10",))
def test_degenerate_cones_and_bounds(name):
    """mu = 0 (the n.f >= 0 row is a real row, not implied by rows 0 and 1; ``stand10`` and the
    standing interior-point classes: standing with mu = 0), the same with that row binding
    (mu0lift), mu = 1e-3, fz_max = 0 and contact x 1e-30 (every bound active at f = 0): status 0,
    the oracle's optimum to the contract, cone and bounds feasible."""
    eng = _engine(name)
    for key, (bt, xs) in _degenerate_refs(name).items():
        u0, U, st, it = _solve(eng, bt)
        err = _worst(u0, U, xs)
        print(f"E_MEASURED {name} {key}: status {st.tolist()} iterations {it.tolist()} worst relative error {err:.2e}")
        assert (st == 0).all(), (name, key, st)
        _cone_ok(bt, U)
        assert err < TOL_U0, (name, key, err)
        assert err < _e_guard(name, key), (name, key, err)


# ---- F: the iteration cap beyond class 64
@pytest.mark.gpu
@pytest.mark.parametrize("name", ("c96", "c128"))
def test_iteration_cap_dense_classes(name):
    """One robot, uncapped count T: max_iter = T and T + 1 are bitwise the uncapped result;
    T - 1, T // 2 and 1 report MAX_ITER within cap + 1 steps executed (a pair step begun at the
    cap counts 2; class 96's robot has one across T // 2 = 15: 16 steps) with a finite iterate."""
    one = {k: v[2:3].copy() for k, v in _base(name).items()}
    ref = _solve(_engine(name), one)
    T = int(ref[3][0])
    assert ref[2][0] == 0 and T >= 4, (name, T)
    for cap in (T, T + 1):
        assert _same(_solve(_engine(name, max_iter=cap), one), ref), (name, cap)
    for cap in (T - 1, T // 2, 1):
        u0, U, st, it = _solve(_engine(name, max_iter=cap), one)
        assert st[0] == 1 and it[0] <= cap + 1, (name, cap, st, it)
        assert np.isfinite(u0).all() and np.isfinite(U).all(), (name, cap)


@pytest.mark.gpu
@pytest.mark.parametrize("name", IPM)
def test_interior_point_does_not_read_max_iter(name):
    """max_iter = 1 is bitwise the default engine's result, status 0."""
    assert _same(_solve(_engine(name, max_iter=1), _base(name)), _clean(name)), name

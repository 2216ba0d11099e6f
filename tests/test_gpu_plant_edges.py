"""GPU: mpcqp_plant and mpcqp_plant_reset where tests/test_gpu_plant.py cannot see a mistake --
per-robot ground planes, a mixed fleet (A1 and Aliengo in turn, each robot its own mass, mu and
inertia), legs at every clamp of the inverse kinematics, 16 substeps, the small branch of
plant_quat_step, the refusals after the substeps and after the output pass, the entry refusals
not yet tried, rows past the batch, each nullable output, reset from seeded poses on slopes and
200 ticks of standing on a slope.  The lane mapping of csrc/mpcqp_plant.h (quad broadcasts, the
per-leg selects, the per-robot indices, the re-load of a refused robot, lane 3's short store) is
device-only code: the CPU suite checks the algebra through plant_robot_step and cannot see it.

Everything is compared with tests/plant_ref.py on the same inputs; tests/test_plant.py runs the
same seeded sets through the host-compiled header, so a mismatch here that the header does not
share points at the lane mapping.

Bounds, by the rule of tests/test_gpu_plant.py: the record norm-wise per robot under ten times
the worst error of the first green run, capped at 1e-9; the float32 outputs under F32_BOUND, one
ulp of the row's largest value; contact words, flag word, tick count, touch, status and a refused
robot's record exactly.  A robot that the restatement alone places within 1e-9 of a switching
threshold is left out of the contact comparison, at most 2 % of a set.  A clamped leg's hip and
thigh angles and its joint rates hang on rounding noise (J_b^-1 near 1e14) and are not compared;
its knee angle, its foot and the rest of its robot are.

A foot that stays pinned is held to |n . p - d| <= 1e-12 with its robot's own float32 plane.  A
foot that lands in the tick is projected by p - s n with the float32 n as it is, whose length
differs from 1 by up to 2e-7: it ends |s| |1 - n . n| off the plane, 4e-11 m at worst in the
restatement itself, so a landed foot is held to the restatement's own n . p - d within 1e-12.

Measured on the MI355X on the first green run (printed by the tests), the record norm-wise per
robot against the restatement:
    mixed fleet on slopes, substeps 1:   B = 1 1.67e-16, 16 3.87e-16, 67 5.09e-16, 130 5.55e-16
    mixed fleet on slopes, substeps 16:  B = 1 3.33e-16, 16 1.74e-15, 67 1.74e-15, 130 2.63e-15
    one plane for all 5.17e-16; clamped legs 4.44e-16, their second call 6.28e-16
    slow rotation 3.33e-16 (substeps 1), 4.44e-16 (substeps 16)
    a record quaternion of norm 2 / 0.5: the body 2.37e-16 / 1.73e-16
    reset on slopes 2.22e-16 (absolute, B = 67 and 130)
    standing on a slope, 200 ticks: 9.34e-17 per tick at worst; the body moves 3.6e-17 m in the
      restatement under the float64 torques, 3.19e-9 m on both sides under their float32 roundings
Every float32 output equals the restatement's rounding, but a gyro word of the slow set (2.2e-16
of its row).  The worst of these, 2.63e-15, is under the single ticks' DEVICE_BOUND = 7.3e-15
(tests/test_gpu_plant.py: ten times 7.29e-16), so every comparison here reuses that bound; ten
times 2.63e-15 would be 2.7e-14.  Nothing was found wrong in the kernel: all of this passed on
its first run on the device.

Each of these, inverted in a scratch copy of csrc/mpcqp_plant.h, fails here (and nothing else
of this file does):
    the plane index bs * 4 -> 0          test_mixed_fleet_on_per_robot_slopes (B = 16, 67, 130),
                                         test_entry_refusals_not_yet_tried (the NaN plane row)
    the same in mpcqp_plant_reset        test_reset_from_seeded_poses_on_slopes,
                                         test_rows_past_the_batch_are_untouched (B = 15, 17, 67)
    the robot-record index -> 0          test_mixed_fleet_on_per_robot_slopes (B = 16, 67, 130),
                                         test_a_plane_broadcast..., test_clamp_flags...,
                                         test_entry_refusals..., test_standing_on_a_slope...
    the geometry index -> 0              the same, and test_late_refusals...
    1 << leg -> 1                        test_clamp_flags_per_robot_and_rebuilt_by_every_call,
                                         test_a_record_quaternion_off_unit_length
    the re-load of a refused robot       test_late_refusals_leave_the_neighbours_alone (1 and 4)
"""
import ctypes
import functools

import numpy as np
import pytest

# torch first: see tests/test_gpu_plant.py
torch = pytest.importorskip("torch")

import kin_ref  # noqa: E402
import plant_ref as pr  # noqa: E402
from test_gpu_plant import DEV, DEVICE_BOUND, F32_BOUND, SENTINEL, _bits, _dev, pair, run_device  # noqa: E402
from test_plant import SETS, check_set  # noqa: E402

pytestmark = pytest.mark.gpu

# the single ticks' 7.3e-15 holds for every set here (worst 2.63e-15, the mixed fleet at B = 130
# and 16 substeps; the figures stand in the docstring) and is reused
MIXED_BOUND = CLAMPED_BOUND = SLOW_BOUND = DEVICE_BOUND
STAND_BOUND = DEVICE_BOUND          # per tick, as the replay's; measured 9.34e-17
ORDER = ("tau", "robot", "geom", "plane", "state", "root", "dofs", "gyro", "accel", "touch", "status")
OUTS = ("root", "dofs", "gyro", "accel", "touch")
SHAPES = dict(root=(13,), dofs=(12, 2), gyro=(3,), accel=(3,), touch=(4,))


@functools.lru_cache(maxsize=None)
def edge_set(name, substeps):
    """A seeded set of 512 (tests/test_plant.py's, which runs it through the host header), what
    the restatement makes of it and which robots it places near a threshold; computed once."""
    make, seed = SETS[name]
    par = pr.Params(substeps=substeps)
    st = make(512, seed, par)
    args = (st["tau"], st["robot"], st["geom"], par, st.get("plane"))
    near = pr.near_threshold(st["rec"], *args)
    ref = st["rec"].copy()
    want = pr.plant_step(ref, *args)
    check_set(st, par, pr.trace_step(st["rec"], *args), ref)
    assert near.mean() <= 0.02 and (want["status"] == 0).all()
    return st, near, ref, want


def batch(name, substeps, B):
    """B robots of a set, the two rows that hold every case among them (as states())."""
    st, near, ref, want = edge_set(name, substeps)
    idx = np.r_[np.arange(B - 1), 511]
    sub = {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    return sub, near[idx], ref[idx], {k: v[idx] for k, v in want.items()}


def on_device(B, st, substeps=1, plane="own", **kw):
    """A plant of B robots with the set's own plane (through BatchedPlant(plane=...)), robots and
    geometry, stepped once."""
    if isinstance(plane, str):
        plane = st.get("plane")
    _, plant = pair(B, substeps=substeps, **({} if plane is None else dict(plane=plane)), **kw)
    rec, out = run_device(plant, st["rec"], st["tau"], st["robot"], st["geom"])
    return plant, rec, out


def compare(got_rec, got, ref, want, near, bound, clamped=None, still=None):
    """The device against the restatement; returns the worst record error and the worst float32
    error."""
    B = len(ref)
    keep = ~near
    err = pr.record_error(got_rec, ref)[keep].max()
    assert (got["status"] == 0).all()
    assert np.array_equal(got_rec[keep, pr.CONTACT:pr.WORDS], ref[keep, pr.CONTACT:pr.WORDS])   # contact, flag word, count
    assert np.array_equal(got_rec[:, pr.FLAGS:pr.WORDS], ref[:, pr.FLAGS:pr.WORDS])
    assert np.array_equal(got_rec[:, pr.WORDS:], ref[:, pr.WORDS:])                             # the padding is kept
    assert np.array_equal(got["touch"][keep], want["touch"][keep])
    assert np.isfinite(got_rec).all() and all(np.isfinite(got[k]).all() for k in OUTS)
    cl = np.zeros((B, 4), bool) if clamped is None else clamped
    moving = np.ones(B, bool) if still is None else ~still
    assert np.abs(got["gyro"][~moving]).max(initial=0.0) <= 1e-15        # at rest: rounding noise, 1e-19
    worst = 0.0
    for k in ("root", "gyro", "accel"):
        rows = np.flatnonzero(keep & (moving | (k != "gyro")))
        worst = max(worst, max(kin_ref.norm_err(got[k][b], want[k][b]) for b in rows))
    gd, wd = got["dofs"].reshape(B, 4, 6), want["dofs"].reshape(B, 4, 6)
    worst = max(worst, max(kin_ref.norm_err(gd[b][~cl[b]], wd[b][~cl[b]]) for b in np.flatnonzero(keep & ~cl.all(1))))
    assert err <= bound, (err, bound)
    assert worst <= F32_BOUND, worst
    return err, worst


def plane_residual(rec, plane):
    """n . p - d of the four feet with the robot's own float32 plane, [B,4]."""
    pl = np.asarray(plane, np.float32).astype(np.float64)
    feet = rec[:, pr.FEET:pr.FEET + 12].reshape(-1, 4, 3)
    return np.sum(pl[:, None, :3] * feet, -1) - pl[:, None, 3]


# ---- a mixed fleet on per-robot slopes

@pytest.mark.parametrize("substeps", [1, 16])
@pytest.mark.parametrize("B", [1, 16, 67, 130])
def test_mixed_fleet_on_per_robot_slopes(B, substeps):
    """A1 and Aliengo in turn, each robot its own mass, mu, inertia and ground plane; 130 is
    eight whole wavefronts and a quad of two robots, 16 substeps the ABI's maximum.  A plane, a
    robot record or a geometry read from another robot of the wavefront moves the record far
    beyond the bound: every robot's neighbour differs in all of them."""
    st, near, ref, want = batch("mixed", substeps, B)
    plant, rec, out = on_device(B, st, substeps)
    assert plant.plane.shape == (B, 4) and np.array_equal(_bits(plant.plane), st["plane"].view(np.uint32))
    err, f32 = compare(rec, out, ref, want, near, MIXED_BOUND)
    print(f"\nmixed fleet, B = {B}, substeps {substeps}: record {err:.2e} (bound {MIXED_BOUND:g}), float32 outputs {f32:.2e}")
    before, after = st["rec"][:, pr.CONTACT:pr.CONTACT + 4] != 0, rec[:, pr.CONTACT:pr.CONTACT + 4] != 0
    s, s_ref = plane_residual(rec, st["plane"]), plane_residual(ref, st["plane"])
    keep = ~near[:, None]
    assert np.abs(s[before & after & keep]).max(initial=0.0) <= 1e-12
    assert np.abs(s - s_ref)[after & keep].max(initial=0.0) <= 1e-12
    assert np.abs(s_ref[after]).max(initial=0.0) <= 1e-10


def test_a_plane_broadcast_and_a_plane_at_an_odd_offset():
    """plane given as [4] is every robot's; a [B,4] plane that is a slice of a larger allocation
    at an odd 4-byte offset gives bitwise the aligned result."""
    B = 67
    st, near, ref, want = batch("mixed", 1, B)
    one = st["plane"][5]
    plant, rec, out = on_device(B, st, plane=one)
    assert plant.plane.shape == (B, 4) and plant.plane.is_contiguous()
    ref1 = st["rec"].copy()
    want1 = pr.plant_step(ref1, st["tau"], st["robot"], st["geom"], pr.Params(), np.tile(one, (B, 1)))
    near1 = pr.near_threshold(st["rec"], st["tau"], st["robot"], st["geom"], pr.Params(), np.tile(one, (B, 1)))
    assert (want1["status"] == 0).all() and near1.mean() <= 0.02
    err = pr.record_error(rec, ref1)[~near1].max()
    print(f"\none plane for all: record {err:.2e}")
    assert err <= MIXED_BOUND and np.array_equal(rec[~near1, pr.CONTACT:pr.WORDS], ref1[~near1, pr.CONTACT:pr.WORDS])
    assert not np.array_equal(ref1[:, pr.CONTACT:pr.CONTACT + 4], ref[:, pr.CONTACT:pr.CONTACT + 4])   # the plane matters
    # the slice at an odd offset, through the class
    _, aligned_rec, aligned = on_device(B, st)
    big = torch.full((4 * B + 8,), SENTINEL, dtype=torch.float32, device=DEV)
    big[3:3 + 4 * B] = _dev(st["plane"]).reshape(-1)
    _, plant = pair(B, plane=big[3:3 + 4 * B].view(B, 4))
    assert plant.plane.data_ptr() == big.data_ptr() + 12           # the view itself: no copy on the way
    assert plant.plane.data_ptr() % 8 == 4
    odd_rec, odd = run_device(plant, st["rec"], st["tau"], st["robot"], st["geom"])
    assert np.array_equal(odd_rec.view(np.uint64), aligned_rec.view(np.uint64))
    for k in OUTS + ("status",):
        assert np.array_equal(odd[k].view(np.uint32), aligned[k].view(np.uint32)), k
    assert (big[:3] == SENTINEL).all() and (big[3 + 4 * B:] == SENTINEL).all()


# ---- the raw binding: rows past the batch, each nullable output

def _raw_buffers(B, st, rows):
    """Device buffers of `rows` robots for the raw call, the state and the outputs filled with
    the sentinel past what the inputs fill."""
    f32 = dict(dtype=torch.float32, device=DEV)
    bufs = dict(tau=_dev(st["tau"], torch.float32), robot=_dev(st["robot"], torch.float32),
                geom=_dev(st["geom"], torch.float64), plane=None if st.get("plane") is None else _dev(st["plane"], torch.float32))
    bufs["state"] = torch.full((rows, pr.STRIDE), SENTINEL, dtype=torch.float64, device=DEV)
    bufs["state"][:B] = _dev(st["rec"])
    for k in OUTS:
        bufs[k] = torch.full((rows,) + SHAPES[k], SENTINEL, **f32)
    bufs["status"] = torch.full((rows,), int(SENTINEL), dtype=torch.int32, device=DEV)
    return bufs


def _raw_plant(plant, B, bufs, **override):
    from mpcqp import _lib
    p = dict(bufs, **override)
    code = plant.lib.mpcqp_plant(plant._ctx, B, 0, *[None if p[k] is None else ctypes.c_void_p(p[k].data_ptr()) for k in ORDER], None)
    torch.cuda.synchronize()
    assert code == _lib.MPCQP_OK, plant.lib.mpcqp_last_error(plant._ctx)


@pytest.mark.parametrize("B", [1, 15, 17, 67])
def test_rows_past_the_batch_are_untouched(B):
    """The state and every output carry two more robots' rows than the batch, filled with a
    sentinel: bitwise untouched after mpcqp_plant and after mpcqp_plant_reset, and the rows of
    the batch are the class's."""
    from mpcqp import _lib
    st, near, ref, want = batch("mixed", 1, B)
    _, class_rec, class_out = on_device(B, st)
    _, plant = pair(B)
    bufs = _raw_buffers(B, st, B + 2)
    _raw_plant(plant, B, bufs)
    assert np.array_equal(_bits(bufs["state"][:B]), class_rec.view(np.uint64))
    for k in OUTS + ("status",):
        assert np.array_equal(_bits(bufs[k][:B]), class_out[k].view(np.uint32)), k
        assert (bufs[k][B:] == SENTINEL).all(), k
    assert (bufs["state"][B:] == SENTINEL).all()
    # reset from the outputs it has just written
    code = plant.lib.mpcqp_plant_reset(plant._ctx, B, *[ctypes.c_void_p(bufs[k].data_ptr())
                                                        for k in ("root", "dofs", "geom", "plane", "state")], None)
    torch.cuda.synchronize()
    assert code == _lib.MPCQP_OK
    got = bufs["state"][:B].cpu().numpy()
    want_rec = pr.reset(class_out["root"], class_out["dofs"], st["geom"], pr.Params(), st["plane"])
    assert np.abs(got - want_rec)[:, :pr.CONTACT].max() <= 1e-12 and not got[:, pr.FLAGS:].any()
    sure = np.abs(plane_residual(want_rec, st["plane"]) - pr.Params().contact_tol) > 1e-9
    assert np.array_equal(got[:, pr.CONTACT:pr.CONTACT + 4][sure], want_rec[:, pr.CONTACT:pr.CONTACT + 4][sure])
    assert (bufs["state"][B:] == SENTINEL).all()
    for k in OUTS:
        assert (bufs[k][B:] == SENTINEL).all(), k


@pytest.mark.parametrize("skipped", ["gyro", "accel", "touch", "status"])
def test_each_nullable_output_null_in_turn(skipped):
    B = 67
    st, _, _, _ = batch("mixed", 1, B)
    _, plant = pair(B)
    full = _raw_buffers(B, st, B)
    _raw_plant(plant, B, full)
    bufs = _raw_buffers(B, st, B)
    _raw_plant(plant, B, bufs, **{skipped: None})
    assert (bufs[skipped] == SENTINEL).all()
    assert not (full[skipped] == SENTINEL).any()
    for k in ("state",) + OUTS + ("status",):
        if k != skipped:
            assert np.array_equal(_bits(bufs[k]), _bits(full[k])), k


# ---- the clamp bits

def test_clamp_flags_per_robot_and_rebuilt_by_every_call():
    """Every single leg at each kind of clamp, the side pairs, the diagonal pairs and all four:
    the flag words 1, 2, 4, 8, 5, 10, 6, 9 and 15, each on its own robot.  The second call runs
    on the first one's records with the clamped feet of every other robot moved within reach:
    their flag word is 0 again, rebuilt from that call alone."""
    B = 67
    st, near, ref, want = batch("clamped", 1, B)
    assert set(st["word"]) == {1, 2, 4, 8, 5, 10, 6, 9, 15}
    plant, rec, out = on_device(B, st)
    assert np.array_equal(rec[:, pr.FLAGS], st["word"].astype(np.float64))
    err, f32 = compare(rec, out, ref, want, near, CLAMPED_BOUND, clamped=st["clamped"])
    print(f"\nclamped legs, B = {B}: record {err:.2e} (bound {CLAMPED_BOUND:g}), float32 outputs {f32:.2e}")
    for o in (out, want):
        calf = o["dofs"].reshape(B, 4, 3, 2)[:, :, 2, 0].astype(np.float64)
        knee = -calf[st["clamped"] & (st["kind"] == 0)]
        assert (knee > 0).all() and (knee <= np.sqrt(2 * pr.IK_EPS) * (1 + 1e-6)).all()
        assert (np.abs(np.pi + calf[st["clamped"] & (st["kind"] == 1)]) <= 2.0 ** -22).all()
    # the second call
    again = rec.copy()
    even = (np.arange(B) % 2 == 0)[:, None] & st["clamped"]
    feet = again[:, pr.FEET:pr.FEET + 12].reshape(B, 4, 3)
    feet[even] = st["feet_ok"][even]
    par = pr.Params()
    near2 = pr.near_threshold(again, st["tau"], st["robot"], st["geom"], par)
    ref2 = again.copy()
    want2 = pr.plant_step(ref2, st["tau"], st["robot"], st["geom"], par)
    word2 = np.where(np.arange(B) % 2 == 0, 0, st["word"]).astype(np.float64)
    assert np.array_equal(ref2[:, pr.FLAGS], word2) and (want2["status"] == 0).all() and near2.mean() <= 0.02
    rec2, out2 = run_device(plant, again, st["tau"])
    assert np.array_equal(rec2[:, pr.FLAGS], word2)
    err, f32 = compare(rec2, out2, ref2, want2, near2, CLAMPED_BOUND, clamped=st["clamped"] & ~even)
    print(f"the second call: record {err:.2e}, float32 outputs {f32:.2e}")
    assert np.array_equal(rec2[:, pr.TICK], st["rec"][:, pr.TICK] + 2)


# ---- slow rotation

@pytest.mark.parametrize("substeps", [1, 16])
def test_slow_rotation_takes_the_small_branch(substeps):
    """|h w*| below 1e-6 on three quarters of the robots (asserted on the restatement by
    check_set): exactly 0 where nothing pushes -- those keep their quaternion bitwise -- near
    1e-19 on the loaded symmetric stand, whose quaternion moves by less than an ulp of 1, and near
    1e-7 in the air."""
    B = 67
    st, near, ref, want = batch("slow", substeps, B)
    plant, rec, out = on_device(B, st, substeps)
    err, f32 = compare(rec, out, ref, want, near, SLOW_BOUND, still=st["still"])
    print(f"\nslow rotation, B = {B}, substeps {substeps}: record {err:.2e} (bound {SLOW_BOUND:g}), float32 outputs {f32:.2e}")
    q0, q1 = st["rec"][:, pr.QUAT:pr.QUAT + 4], rec[:, pr.QUAT:pr.QUAT + 4]
    assert st["zero"].sum() >= 8 and np.array_equal(q1[st["zero"]].view(np.uint64), q0[st["zero"]].view(np.uint64))
    assert np.abs(q1 - q0)[st["still"]].max() <= 2.0 ** -53
    assert np.array_equal(rec[st["zero"], pr.OMEGA:pr.OMEGA + 3], np.zeros((st["zero"].sum(), 3)))


# ---- refusals

def _classify(st, b, par):
    """What the restatement makes of robot b alone: refused at entry, finite after the substeps,
    the status, and its outputs."""
    one = {k: st[k][b:b + 1] for k in ("rec", "tau", "robot", "geom")}
    plane = None if st.get("plane") is None else st["plane"][b:b + 1]
    pl = pr.planes(1, par, plane)
    with np.errstate(all="ignore"):
        entry = bool(pr.refused(one["rec"], one["tau"], one["robot"])[0]) or not np.isfinite(one["geom"][:, :5]).all() \
            or not np.isfinite(pl).all()
        work = one["rec"].copy()
        for _ in range(par.substeps):
            pr.substep(work, one["tau"], one["robot"], one["geom"], pl, par, par.dt_control / par.substeps)
    rec = one["rec"].copy()
    out = pr.plant_step(rec, one["tau"], one["robot"], one["geom"], par, plane)
    assert np.array_equal(rec, one["rec"], equal_nan=True) or out["status"][0] == 0
    return entry, bool(np.isfinite(work[:, :pr.FLAGS]).all()), int(out["status"][0]), out


def _refused_alone(plant, st, bad, b, clean_rec, clean, want, rewrite=True):
    """Robot b of `bad` (the set st with one robot spoilt) is refused and nothing else changes:
    status 4, its record bitwise untouched, every other robot's record and outputs bitwise the
    clean run's, its own outputs the restatement's rewrite from the untouched record (rewrite
    False: root and touch alone, the roundings of the record's own words -- what libm and the
    device make of an inf or a NaN inside the inverse kinematics is not pinned)."""
    B = len(bad["rec"])
    if bad.get("plane") is not None:
        plant.plane = _dev(bad["plane"], torch.float32)
    rec, out = run_device(plant, bad["rec"], bad["tau"], bad["robot"], bad["geom"])
    others = np.arange(B) != b
    assert out["status"][b] == 4 and (out["status"][others] == 0).all()
    assert np.array_equal(rec[b].view(np.uint64), bad["rec"][b].view(np.uint64))          # the tick count with it
    assert np.array_equal(rec[others].view(np.uint64), clean_rec[others].view(np.uint64))
    for k in OUTS:
        assert np.array_equal(out[k][others].view(np.uint32), clean[k][others].view(np.uint32)), k
    # the rewrite: a word that is not finite in the restatement is not finite here (payloads and
    # inf against NaN are not compared); the finite words that are roundings of the record's own
    # words (root, touch) and accel = Rq^T (0, 0, g) bitwise, the angles and rates of the inverse
    # kinematics, and the gyro, under F32_BOUND
    for k in OUTS if rewrite else ("root", "touch"):
        g, w = out[k][b].ravel().astype(np.float64), want[k][0].ravel().astype(np.float64)
        fin = np.isfinite(w)
        assert not np.isfinite(g[~fin]).any(), k
        if k in ("root", "touch"):
            assert np.array_equal(g[fin], w[fin]), k
        elif fin.any():
            assert np.abs(g[fin] - w[fin]).max() <= F32_BOUND * max(np.abs(w[fin]).max(), 1e-30), k
    return out


def _spoilt(st, b, **words):
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    for k, (col, val) in words.items():
        bad[k][b, col] = val
    return bad


@pytest.mark.parametrize("substeps", [1, 4])
def test_late_refusals_leave_the_neighbours_alone(substeps):
    """The two refusals that only the kernel's loop has (the host build is straight-line code):
    a non-finite state after the substeps and a non-finite float32 output after the output pass.
    Both re-load the robot's chunk and re-run the output pass over the untouched record.  One
    robot among 67 on per-robot slopes, in a full wavefront and in the tail of three."""
    B = 67
    par = pr.Params(substeps=substeps)
    st, _, _, _ = batch("mixed", substeps, B)
    plant, clean_rec, clean = on_device(B, st, substeps)
    assert (clean["status"] == 0).all()
    first = next(b for b in range(16, 32) if (st["case"][b] == 0).any())
    for b in (first, B - 1):
        leg = int(np.flatnonzero(st["case"][b] == 0)[0])
        kinds = {
            # after the output pass, the rewritten outputs finite: the velocity leaves float32
            "torque 3e38": (_spoilt(st, b, tau=(3 * leg, np.float32(3e38))), True, True),
            # after the substeps; the untouched record's own omega is beyond float32
            "omega 1e200": (_spoilt(st, b, rec=(pr.OMEGA + 1, 1e200)), False, False),
            # after the output pass, the record beyond float32
            "velocity 1e39": (_spoilt(st, b, rec=(pr.VEL, 1e39)), True, False),
        }
        for name, (bad, state_finite, rewrite_finite) in kinds.items():
            entry, finite, status, want = _classify(bad, b, par)
            assert (entry, finite, status) == (False, state_finite, 4), (name, entry, finite, status)
            assert all(np.isfinite(want[k]).all() for k in OUTS) == rewrite_finite, name
            out = _refused_alone(plant, st, bad, b, clean_rec, clean, want)
            if rewrite_finite:
                Rq = kin_ref.quat2matrix_eigen(st["rec"][b:b + 1, pr.QUAT:pr.QUAT + 4])[0]
                assert np.array_equal(out["accel"][b], (Rq.T @ np.array([0.0, 0.0, par.gravity])).astype(np.float32))
                assert np.array_equal(out["touch"][b], (st["rec"][b, pr.CONTACT:pr.CONTACT + 4] != 0).astype(np.float32))
                assert np.isfinite(out["dofs"][b]).all() and np.isfinite(out["root"][b]).all()


def test_entry_refusals_not_yet_tried():
    """mass 0 and negative, a singular inertia, a zero quaternion, an inf in each geometry word,
    a NaN in the robot's plane row, a NaN flag word: each refuses its robot alone."""
    B = 67
    par = pr.Params()
    st, _, _, _ = batch("mixed", 1, B)
    plant, clean_rec, clean = on_device(B, st)
    kinds = [("mass 0", dict(robot=(0, 0.0))), ("mass negative", dict(robot=(0, -4.0))),
             ("singular inertia", dict(robot=(slice(1, 7), 0.0))), ("zero quaternion", dict(rec=(slice(pr.QUAT, pr.QUAT + 4), 0.0))),
             ("NaN flag word", dict(rec=(pr.FLAGS, np.nan))), ("NaN in the plane", dict(plane=(2, np.nan))),
             ("NaN plane offset", dict(plane=(3, np.nan)))]
    kinds += [(f"inf in geom[{k}]", dict(geom=(k, np.inf))) for k in range(5)]
    for i, (name, words) in enumerate(kinds):
        b = (21, 66, 35)[i % 3]
        bad = _spoilt(st, b, **words)
        entry, _, status, want = _classify(bad, b, par)
        assert entry and status == 4, name
        _refused_alone(plant, st, bad, b, clean_rec, clean, want, rewrite=False)
    plant.plane = _dev(st["plane"], torch.float32)
    rec, out = run_device(plant, st["rec"], st["tau"], st["robot"], st["geom"])       # and the context works afterwards
    assert np.array_equal(rec.view(np.uint64), clean_rec.view(np.uint64)) and (out["status"] == 0).all()


@pytest.mark.parametrize("scale", [2.0, 0.5])
def test_a_record_quaternion_off_unit_length(scale):
    """The quaternion is applied as given, as the host header and the restatement do
    (tests/test_plant.py); the one written back is of unit length."""
    B = 16
    par = pr.Params()
    st = pr.make_states(B, seed=9, par=par)
    rec0 = st["rec"].copy()
    rec0[:, pr.QUAT:pr.QUAT + 4] *= scale
    rec0[:, pr.CONTACT:pr.CONTACT + 4] = 0.0
    tau = np.zeros_like(st["tau"])
    ref = rec0.copy()
    want = pr.plant_step(ref, tau, st["robot"], st["geom"], par)
    _, plant = pair(B)
    rec, out = run_device(plant, rec0, tau, st["robot"], st["geom"])
    assert (out["status"] == 0).all() and (want["status"] == 0).all()
    body = slice(0, pr.FEET)
    err = np.abs(rec[:, body] - ref[:, body]).max() / np.abs(ref[:, body]).max()
    print(f"\nquaternion of norm {scale}: the body {err:.2e}")
    assert err <= DEVICE_BOUND and np.array_equal(rec[:, pr.CONTACT:pr.WORDS], ref[:, pr.CONTACT:pr.WORDS])
    assert np.abs(np.linalg.norm(rec[:, pr.QUAT:pr.QUAT + 4], axis=1) - 1.0).max() <= 1e-15
    for k in ("root", "gyro", "accel"):
        assert max(kin_ref.norm_err(out[k][b], want[k][b]) for b in range(B)) <= F32_BOUND, k


# ---- reset on slopes

def slope_poses(B, seed, tol):
    """Seeded root poses (non-level, moving), a mixed fleet's geometry, varied joint angles and
    per-robot planes placed so that one foot is 0.5 tol inside the contact tolerance (n . p - d =
    0.5 tol) and another 2 tol outside it (n . p - d = 2 tol)."""
    rng = np.random.default_rng(seed)
    geom, _ = pr.fleet(B)
    rpy = rng.uniform([-0.3, -0.3, -3.0], [0.3, 0.3, 3.0], (B, 3))
    c, s = np.cos(rpy / 2), np.sin(rpy / 2)
    quat = np.stack([c[:, 0] * c[:, 1] * c[:, 2] + s[:, 0] * s[:, 1] * s[:, 2], s[:, 0] * c[:, 1] * c[:, 2] - c[:, 0] * s[:, 1] * s[:, 2],
                     c[:, 0] * s[:, 1] * c[:, 2] + s[:, 0] * c[:, 1] * s[:, 2], c[:, 0] * c[:, 1] * s[:, 2] - s[:, 0] * s[:, 1] * c[:, 2]], -1)
    pos = rng.uniform([-1, -1, 0.2], [1, 1, 0.4], (B, 3))
    root = kin_ref.root_states(quat, pos, rng.uniform(-0.5, 0.5, (B, 3)), rng.uniform(-1, 1, (B, 3)))
    q = np.tile([0.0, 0.75, -1.5], (B, 4)) + rng.uniform(-0.25, 0.25, (B, 12))
    dofs = kin_ref.dof_states(q, rng.uniform(-1, 1, (B, 12)))
    feet = pr.reset(root, dofs, geom, pr.Params())[:, pr.FEET:pr.FEET + 12].reshape(B, 4, 3)
    i, j = np.arange(B) % 4, (np.arange(B) % 4 + 1 + np.arange(B) % 3) % 4
    pi, pj = feet[np.arange(B), i], feet[np.arange(B), j]
    delta = pj - pi
    n = np.tile([0.0, 0.0, 1.0], (B, 1))
    for _ in range(30):
        n = n - ((np.sum(n * delta, -1) - 1.5 * tol) / np.sum(delta * delta, -1))[:, None] * delta
        n /= np.linalg.norm(n, axis=1)[:, None]
    d = np.sum(n * pi, -1) - 0.5 * tol
    return root, dofs, geom, np.concatenate([n, d[:, None]], 1).astype(np.float32), i, j


@pytest.mark.parametrize("B", [67, 130])
def test_reset_from_seeded_poses_on_slopes(B):
    par = pr.Params()
    root, dofs, geom, plane, i, j = slope_poses(B, 17, par.contact_tol)
    want = pr.reset(root, dofs, geom, par, plane)
    s = plane_residual(want, plane)
    sure = np.abs(s - par.contact_tol) > 1e-9
    rows = np.arange(B)
    assert np.abs(s[rows, i] - 0.5 * par.contact_tol).max() < 1e-6 and np.abs(s[rows, j] - 2 * par.contact_tol).max() < 1e-6
    assert want[rows, pr.CONTACT + i].all() and not want[rows, pr.CONTACT + j].any() and sure.mean() > 0.98
    assert np.arccos(plane[:, 2].astype(np.float64)).max() > 0.1                      # slopes
    _, plant = pair(B, plane=plane)
    plant.geometry = _dev(geom, torch.float64)
    plant.state.fill_(SENTINEL)
    plant.reset(root_states=root, dof_states=dofs)
    torch.cuda.synchronize()
    got = plant.state.cpu().numpy()
    print(f"\nreset on slopes, B = {B}: worst {np.abs(got - want).max():.2e}")
    assert np.abs(got - want).max() <= 1e-12
    assert np.array_equal(got[:, pr.CONTACT:pr.CONTACT + 4][sure], want[:, pr.CONTACT:pr.CONTACT + 4][sure])
    assert not got[:, pr.FVEL:pr.FVEL + 12].any() and not got[:, pr.FLAGS:].any()
    assert np.array_equal(plant.touch.cpu().numpy(), got[:, pr.CONTACT:pr.CONTACT + 4].astype(np.float32))


# ---- standing on a slope

def slope_stand(B, par):
    """B level bodies (A1 and Aliengo in turn, mu 0.7) standing on planes tilted 0.05 .. 0.25 rad:
    the feet at symmetric xy on the robot's float32 plane, joint angles from plant_ref.ik,
    constant torques J^T (-(0, 0, m g / 4)) per leg.  The forces sum to the weight and their
    moments to zero: an equilibrium while tan(tilt) < mu.  Returns the records, the float64
    torques, robot, geom, plane."""
    geom, robot = pr.fleet(B)
    robot[:, 7] = 0.7
    tilt, az = np.linspace(0.05, 0.25, B), 0.9 * np.arange(B)
    n = np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], -1)
    reach = geom[:, 3] + geom[:, 4]
    plane = np.concatenate([n, (-0.7 * reach * n[:, 2])[:, None]], 1).astype(np.float32)
    pl = plane.astype(np.float64)
    xy = np.stack([kin_ref.SX * geom[:, 0:1], kin_ref.SY * (geom[:, 1:2] + geom[:, 2:3])], -1)       # under the hips
    z = (pl[:, None, 3] - np.sum(pl[:, None, :2] * xy, -1)) / pl[:, None, 2]
    feet = np.concatenate([xy, z[..., None]], -1)
    for _ in range(2):                                          # n . p = d to rounding, along z
        feet[..., 2] -= (np.sum(pl[:, None, :3] * feet, -1) - pl[:, None, 3]) / pl[:, None, 2]
    q, clamped = pr.ik(geom, feet)
    assert not clamped.any()
    _, _, Jb = kin_ref.chain(geom, q.reshape(B, 12))
    f = np.array([0.0, 0.0, 1.0]) * (robot[:, 0].astype(np.float64) * par.gravity / 4)[:, None, None]
    tau = np.einsum("blcr,blc->blr", Jb, -np.broadcast_to(f, (B, 4, 3))).reshape(B, 12)
    rec = np.zeros((B, pr.STRIDE))
    rec[:, pr.QUAT] = 1.0
    rec[:, pr.FEET:pr.FEET + 12] = feet.reshape(B, 12)
    rec[:, pr.CONTACT:pr.CONTACT + 4] = 1.0
    return rec, tau, robot, geom, plane


def test_standing_on_a_slope_for_200_ticks():
    """Per tick the device's record against the restatement's under STAND_BOUND x the tick count,
    every contact word 1 throughout.  The construction is checked on the restatement alone: under
    the float64 torques the body moves by less than 1e-9 m in 200 ticks.  The device is given the
    torques in float32, whose rounding (2^-24 of each) unbalances the weight by a few parts in
    1e8: g t^2 / 2 of that over 0.2 s is below 1e-7 m, on the restatement and on the device."""
    B, T = 8, 200
    par = pr.Params()
    rec, tau, robot, geom, plane = slope_stand(B, par)
    exact = rec.copy()
    for _ in range(T):
        out = pr.plant_step(exact, tau, robot, geom, par, plane)
    moved = np.abs(exact[:, :3] - rec[:, :3]).max()
    print(f"\nstanding on slopes of 0.05 .. 0.25 rad: the restatement's body moves {moved:.2e} m in {T} ticks")
    assert moved < 1e-9 and (out["status"] == 0).all() and exact[:, pr.CONTACT:pr.CONTACT + 4].all()
    tau32 = tau.astype(np.float32)
    _, plant = pair(B, plane=plane)
    plant.robot, plant.geometry = _dev(robot, torch.float32), _dev(geom, torch.float64)
    plant.state.copy_(_dev(rec))
    tau_dev = _dev(tau32)
    worst = 0.0
    for t in range(T):
        assert not pr.near_threshold(rec, tau32, robot, geom, par, plane).any()
        pr.plant_step(rec, tau32, robot, geom, par, plane)
        plant.step(tau_dev)
        got = plant.state.cpu().numpy()
        assert (got[:, pr.CONTACT:pr.CONTACT + 4] == 1.0).all() and np.array_equal(got[:, pr.FLAGS:pr.WORDS], rec[:, pr.FLAGS:pr.WORDS]), t
        err = pr.record_error(got, rec).max()
        worst = max(worst, err / (t + 1))
        assert err <= STAND_BOUND * (t + 1), (t, err)
    print(f"the device against the restatement: worst record error per tick {worst:.2e}; the body moved "
          f"{np.abs(got[:, :3]).max():.2e} m under the float32 torques")
    assert (plant.status == 0).all() and np.abs(got[:, :3]).max() < 1e-7 and np.abs(rec[:, :3]).max() < 1e-7

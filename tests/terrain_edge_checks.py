"""The edge checks of mpcqp_terrain, written once and run twice: by tests/test_terrain.py on the
host build of csrc/mpcqp_terrain_robot.h and by tests/test_gpu_terrain_edges.py on the device.
Each check takes ``launch(state [B,STRIDE], inputs, constants=None, ground=False) -> (records
[B,STRIDE], outputs)``: one launch on a copy of ``state``; the launcher keeps canary rows around
every buffer and has found them untouched.  A check returns the figures it measured.

One robot per case, the cases cycled to B = W + 3 = 67 robots, so that every case also sits in
the tail workgroup of three.  ``describe_*`` give, from terrain_ref alone, the decision each
case is meant to take and how far it sits from the threshold
(tests/test_terrain.py::test_cases_are_what_they_claim).
"""
import numpy as np

import terrain_ref as tr

W = 64
B_EDGE = W + 3
N_BOUND = 10 * tr.D_N      # the device build of a host-checked text (tests/test_gpu_terrain.py)
F32_BOUND = 2.4e-7
SQUARE = np.array([[0.2, 0.13, 0.0], [0.2, -0.13, 0.0], [-0.2, 0.13, 0.0], [-0.2, -0.13, 0.0]])
ACOS_HALF = np.arccos(0.5)
BAD = (np.nan, np.inf, -np.inf)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def cycle(rows, B=B_EDGE):
    """rows [K,...] -> ([B,...], case index [B]): robot b is case b mod K."""
    idx = np.arange(B) % len(rows)
    return np.asarray(rows)[idx], idx


def rotation(tilt, az):
    """The rotation that takes e_z to (sin tilt cos az, sin tilt sin az, cos tilt) about the
    level axis at right angles to az."""
    k = np.array([-np.sin(az), np.cos(az), 0.0])
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(tilt) * K + (1 - np.cos(tilt)) * K @ K


def rectangle(a, b, tilt=0.0, az=0.0, centre=(0.0, 0.0, 0.0)):
    """Feet at (+-a, +-b, 0), turned onto the plane of (tilt, az) and moved to ``centre``:
    [4,3] float32.  Level, its scatter is diag(4 a^2, 4 b^2, 0): spread (l1 - l0) / l2 =
    (b / a)^2 for b <= a."""
    p = np.array([[a, b, 0.0], [a, -b, 0.0], [-a, b, 0.0], [-a, -b, 0.0]])
    return (p @ rotation(tilt, az).T + np.asarray(centre)).astype(np.float32)


def seeded_record(feet=None):
    """An initialised record: a tick from zero on ``feet`` (default: the footprint on a plane
    0.3 rad off level at azimuth 0.7), all four in contact."""
    f = rectangle(0.2, 0.13, 0.3, 0.7, (1.0, -2.0, 0.4)) if feet is None else feet
    st, ok = tr.tick_step(np.zeros((1, tr.STRIDE)), f[None], np.ones((1, 4), bool))
    assert ok.all() and st[0, tr.FITTED] == 1
    return st[0]


def against_ref(launch, state, inp, constants=None, ground=False, bound=N_BOUND):
    """One launch against terrain_ref.terrain_step on the same records: the history, the words
    initialised / fitted / pad and the status equal, n and d within ``bound`` (a number or [B]),
    the float32 outputs within F32_BOUND (NaN where the restatement has NaN).  A robot that the
    restatement refuses keeps its bytes.  Returns (records, outputs, the restatement's records
    and outputs, the worst error over bound)."""
    state = np.asarray(state, np.float64)
    B = state.shape[0]
    ref, want = tr.terrain_step(state, inp, constants, ground=ground)
    st, out = launch(state, inp, constants, ground)
    assert np.array_equal(out["status"], want["status"]), np.flatnonzero(out["status"] != want["status"])
    refused = want["status"] != tr.STATUS_OK
    assert same_bits(st[refused], state[refused])
    ok = ~refused
    assert same_bits(st[ok][:, tr.HIST], ref[ok][:, tr.HIST])
    assert np.array_equal(st[ok][:, [tr.INIT, tr.FITTED, 18, 19]], ref[ok][:, [tr.INIT, tr.FITTED, 18, 19]]), \
        (st[ok][:, tr.FITTED], ref[ok][:, tr.FITTED])
    bound = np.broadcast_to(np.asarray(bound, np.float64), (B,))
    worst = 0.0
    for b in np.flatnonzero(ok):
        e = tr.norm_err(st[b], ref[b])
        worst = max(worst, e / bound[b])
        assert e <= bound[b], (b, e, bound[b])
    for k in ("normal", "plane", "normal_base", "robot"):
        if k in want:
            a, r = out[k].astype(np.float64), want[k].astype(np.float64)
            assert np.array_equal(np.isnan(a), np.isnan(r)), k
            fin = np.isfinite(r)
            assert np.array_equal(a[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)]), k
            scale = max(1.0, float(np.abs(r[fin]).max())) if fin.any() else 1.0
            assert np.abs(a[fin] - r[fin]).max() <= F32_BOUND * scale * max(1.0, float(bound.max() / N_BOUND)), k
    return st, out, ref, want, worst


# ---- held fits

HELD = ("collinear", "coincident", "spread flat_tol / 2", "tilt 0.02 rad past the limit", "vertical plane")
ACCEPTED = ("spread 2 flat_tol", "tilt 0.02 rad inside the limit")


def held_feet():
    """[7,4,3] float32 in the order HELD + ACCEPTED, and the names."""
    flat = tr.DEFAULTS["flat_tol"]
    line = np.array([[0.125 * i + 1.0, 0.25 * i - 2.0, 0.0625 * i + 0.5] for i in range(4)], np.float32)
    point = np.tile(np.float32([1.0, 2.0, 0.5]), (4, 1))
    centre = (0.5, 0.25, 0.125)
    thin = rectangle(0.2, 0.2 * np.sqrt(flat / 2), 0.2, 0.4, centre)
    wide = rectangle(0.2, 0.2 * np.sqrt(2 * flat), 0.2, 0.4, centre)
    past = rectangle(0.2, 0.13, ACOS_HALF + 0.02, 2.0, centre)
    inside = rectangle(0.2, 0.13, ACOS_HALF - 0.02, 2.0, centre)
    wall = np.array([[0.2, 1.0, 0.3], [0.2, 1.0, -0.1], [-0.2, 1.0, 0.3], [-0.2, 1.0, -0.1]], np.float32)
    return np.stack([line, point, thin, past, wall, wide, inside]), HELD + ACCEPTED


def describe_held():
    """Per case: (name, fitted by terrain_ref, spread, n_fit_z)."""
    feet, names = held_feet()
    mu, l, nf = tr.fit(feet.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        spread = np.where(l[:, 2] > 0, (l[:, 1] - l[:, 0]) / l[:, 2], 0.0)
    st, ok = tr.tick_step(np.zeros((len(feet), tr.STRIDE)), feet, np.ones((len(feet), 4), bool))
    assert ok.all()
    return [(names[k], bool(st[k, tr.FITTED]), float(spread[k]), float(nf[k, 2]), float(l[k, 2])) for k in range(len(feet))]


def check_held_fits(launch):
    """Each case from a fresh record (contact whatever: the seed tick takes all four) and from
    a record that holds a tilted n, with the robot record handed in: a held tick leaves n
    bitwise, d = n . mu follows the centroid, the history is latched, the status OK, and words
    9..11 of the robot record are rewritten with the old normal, no other word touched."""
    feet, names = held_feet()
    f, idx = cycle(feet)
    held = idx < len(HELD)
    rob0 = np.arange(B_EDGE * 16, dtype=np.float32).reshape(B_EDGE, 16)
    worst = 0.0
    for start in ("fresh", "seeded"):
        state = np.zeros((B_EDGE, tr.STRIDE)) if start == "fresh" else np.tile(seeded_record(), (B_EDGE, 1))
        old = tr.as_was(state)[:, tr.N]
        inp = dict(pos_feet=f, contact=np.ones((B_EDGE, 4), np.float32), robot=rob0)
        st, out, ref, want, w = against_ref(launch, state, inp)
        worst = max(worst, w)
        assert (out["status"] == 0).all() and (st[:, tr.INIT] == 1).all()
        assert np.array_equal(st[:, tr.FITTED] == 0, held), (start, st[:, tr.FITTED])
        assert same_bits(st[held][:, tr.N], old[held]), start
        assert not any(same_bits(st[b, tr.N], old[b]) for b in np.flatnonzero(~held)), start
        assert same_bits(st[:, tr.HIST], f.astype(np.float64).reshape(B_EDGE, 12))
        mu = f.astype(np.float64).mean(axis=1)
        assert np.abs(st[:, tr.D] - np.einsum("bk,bk->b", st[:, tr.N], mu)).max() <= N_BOUND * 4
        assert same_bits(out["robot"][:, 9:12], st[:, tr.N].astype(np.float32))
        assert same_bits(out["robot"][held][:, 9:12], old[held].astype(np.float32))
        keep = np.ones(16, bool)
        keep[9:12] = False
        assert same_bits(out["robot"][:, keep], rob0[:, keep])
        assert same_bits(out["plane"][:, :3], out["normal"])
    return worst


# ---- blend

def check_blend(launch, traj):
    """blend = 0.25 and 0.5 over 10 ticks of the trajectory's first B_EDGE robots against
    terrain_ref, record after record."""
    worst = 0.0
    for blend in (0.25, 0.5):
        c = dict(blend=blend)
        st = np.zeros((B_EDGE, tr.STRIDE))
        ref = st.copy()
        for t in range(10):
            inp = dict(pos_feet=traj[t]["pos_feet"][:B_EDGE], swing_state=traj[t]["swing_state"][:B_EDGE],
                       quat=traj[t]["quat"][:B_EDGE])
            ref, want = tr.terrain_step(ref, inp, c)
            st, out = launch(st, inp, c, False)
            assert same_bits(st[:, tr.HIST], ref[:, tr.HIST]) and np.array_equal(st[:, tr.FITTED], ref[:, tr.FITTED])
            e = tr.norm_err(st, ref)
            worst = max(worst, e)
            assert e <= N_BOUND, (blend, t, e)
            for k in ("normal", "plane", "normal_base"):
                assert np.abs(out[k].astype(np.float64) - want[k]).max() <= F32_BOUND * max(1.0, float(np.abs(want[k]).max()))
        assert (ref[:, tr.FITTED] == 1).all()
        n_full = tr.run(traj[:10])[0][-1][:B_EDGE, tr.N]
        assert np.abs(ref[:, tr.N] - n_full).max() > 1e-3              # the filter did lag
    return worst


SEEDED_N = ("opposite", "length 2 along the fit", "length 2, tilted")


def seeded_n_records():
    """Caller-seeded records on the level rectangle (whose fit is (0, 0, 1) exactly) at blend =
    0.5: n exactly opposite to the fit (the blend has length 0: hold), n of length 2."""
    feet = rectangle(0.2, 0.13, centre=(1.0, 2.0, 0.5))
    base = seeded_record(feet)
    assert base[tr.N].tolist() == [0.0, 0.0, 1.0]
    recs = np.tile(base, (3, 1))
    recs[0, tr.N] = [0.0, 0.0, -1.0]
    recs[1, tr.N] = [0.0, 0.0, 2.0]
    recs[2, tr.N] = 2.0 * np.array([np.sin(0.3), 0.0, np.cos(0.3)])
    return recs, feet


def check_seeded_normals(launch):
    recs, feet = seeded_n_records()
    state, idx = cycle(recs)
    inp = dict(pos_feet=np.tile(feet, (B_EDGE, 1, 1)), contact=np.ones((B_EDGE, 4), np.float32))
    st, out, ref, want, w = against_ref(launch, state, inp, dict(blend=0.5))
    assert np.array_equal(st[:, tr.FITTED], (idx != 0).astype(np.float64))
    assert all(st[b, tr.N].tolist() == [0.0, 0.0, -1.0] for b in np.flatnonzero(idx == 0))      # held, as seeded
    assert all(st[b, tr.N].tolist() == [0.0, 0.0, 1.0] for b in np.flatnonzero(idx == 1))
    tilted = st[idx == 2][:, tr.N]
    assert np.abs(np.linalg.norm(tilted, axis=1) - 1.0).max() <= 4e-16 and (np.abs(tilted[:, 0] - 0.199) < 1e-4).all()
    return w


# ---- exact structure

def check_exact_structure(launch):
    """The level rectangle (S diagonal: every rotation skipped) and the level square (l1 == l2):
    n = (0, 0, 1) and d exactly.  The tilted square, and planes whose normal is near x, near y
    and near z at cos_max_tilt = 0.05, against the restatement."""
    centre = (3.0, -2.0, 0.75)
    near = np.arccos(0.1)
    cases = [rectangle(0.2, 0.13, centre=centre), rectangle(0.25, 0.25, centre=centre),
             rectangle(0.25, 0.25, 0.3, 1.1, centre), rectangle(0.2, 0.13, near, 0.0, centre),
             rectangle(0.2, 0.13, near, np.pi / 2, centre), rectangle(0.2, 0.13, 0.01, 2.5, centre),
             rectangle(0.2, 0.13, near, np.pi, centre), rectangle(0.2, 0.13, near, -np.pi / 2, centre)]
    f, idx = cycle(np.stack(cases))
    inp = dict(pos_feet=f, contact=np.ones((B_EDGE, 4), np.float32))
    st, out, ref, want, w = against_ref(launch, np.zeros((B_EDGE, tr.STRIDE)), inp, dict(cos_max_tilt=0.05))
    assert (st[:, tr.FITTED] == 1).all()
    for b in np.flatnonzero(idx <= 1):
        assert st[b, tr.N].tolist() == [0.0, 0.0, 1.0] and st[b, tr.D] == 0.75, b
        assert out["plane"][b].tolist() == [0.0, 0.0, 1.0, 0.75]
    n = st[:, tr.N]
    assert (np.abs(n[idx == 3][:, 0]) > 0.99).all() and (np.abs(n[idx == 4][:, 1]) > 0.99).all() and (n[idx == 5][:, 2] > 0.9999).all()
    assert (n[:, 2] > 0).all()
    # at the default limit the four steep ones are held
    st2, _, _, _, _ = against_ref(launch, np.zeros((B_EDGE, tr.STRIDE)), inp)
    assert np.array_equal(st2[:, tr.FITTED] == 0, np.isin(idx, (3, 4, 6, 7)))
    return w


SCALES = (0, -40, -10, 10, 40)


def check_scaling(launch):
    """The same feet multiplied by 2^k: every product, sum, quotient and square root of the tick
    scales by a power of two without rounding differently, so n and fitted are bitwise the
    unscaled ones and d is scaled exactly.  No tolerance: a divide or square root that is not
    correctly rounded shows here."""
    base = [rectangle(0.2, 0.13, 0.3, 0.7, (1.0, -2.0, 0.4)), rectangle(0.21, 0.12, 0.8, -2.0, (0.3, 0.2, -0.1)),
            rectangle(0.2, 0.2 * np.sqrt(0.004), 0.1, 0.3, (0.5, 0.5, 0.5)), rectangle(0.2, 0.13, ACOS_HALF + 0.02, 2.0)]
    rows = np.stack([f * np.float32(2.0 ** k) for f in base for k in SCALES])
    assert np.isfinite(rows).all() and (np.abs(rows[rows != 0]) > 1e-30).all()
    f, idx = cycle(rows)
    inp = dict(pos_feet=f, contact=np.ones((B_EDGE, 4), np.float32))
    st, out = launch(np.zeros((B_EDGE, tr.STRIDE)), inp, None, False)
    ref, _ = tr.terrain_step(np.zeros((B_EDGE, tr.STRIDE)), inp)
    assert np.array_equal(st[:, tr.FITTED], ref[:, tr.FITTED]) and (out["status"] == 0).all()
    for b in range(B_EDGE):
        k = SCALES[idx[b] % len(SCALES)]
        unit = (idx[b] // len(SCALES)) * len(SCALES)         # the k = 0 row of the same feet
        assert same_bits(st[b, tr.N], st[unit, tr.N]), (b, k)
        assert st[b, tr.FITTED] == st[unit, tr.FITTED] and st[b, tr.D] == st[unit, tr.D] * 2.0 ** k, (b, k)
    assert set(st[:, tr.FITTED]) == {0.0, 1.0}
    return int(len(rows))


# ---- ill-conditioned but accepted

SPREADS = (0.002, 0.005, 0.01, 0.02, 0.05)


def thin_feet():
    """Rectangles of spread (b / a)^2 in SPREADS on planes 0.3 rad off level, 13 azimuths each."""
    rows = [rectangle(0.2, 0.2 * np.sqrt(s), 0.3, 0.5 * j, (1.0 + 0.1 * j, -0.5, 0.3)) for j in range(13) for s in SPREADS]
    return np.stack(rows)


def check_thin_footprints(launch):
    """The eigenvector of l0 moves by eps l2 / (l1 - l0) per rounding of S, and N_BOUND was
    measured at a spread of 0.05 and more: the bound is N_BOUND max(1, 0.05 / spread).  Returns
    the worst error per spread."""
    f, idx = cycle(thin_feet())
    inp = dict(pos_feet=f, contact=np.ones((B_EDGE, 4), np.float32))
    spread = tr.spread(f.astype(np.float64))
    assert np.abs(spread / np.array(SPREADS)[idx % len(SPREADS)] - 1.0).max() < 1e-4
    bound = N_BOUND * np.maximum(1.0, 0.05 / spread)
    st, out, ref, want, _ = against_ref(launch, np.zeros((B_EDGE, tr.STRIDE)), inp, None, False, bound)
    assert (st[:, tr.FITTED] == 1).all()
    err = {}
    for j, s in enumerate(SPREADS):
        rows = np.flatnonzero(idx % len(SPREADS) == j)
        err[s] = max(tr.norm_err(st[b], ref[b]) for b in rows)
    return err


# ---- decisions on odd inputs

ODD = (("contact", 0.5, False), ("contact", np.nan, False), ("swing_state", np.nan, True), ("swing_state", -0.0, True),
       ("swing_state", 1e-45, False), ("contact", np.nextafter(np.float32(0.5), np.float32(1)), True))


def check_odd_inputs(launch):
    """A value per rule on all four feet of a seeded record with the feet moved: latched or
    not, as terrain_ref.contact_decision says and as the table says.  Then a non-finite foot:
    ignored on a leg that is not latched, refused on the seed tick, whose outputs are the level
    plane through the origin (under MPCQP_TERRAIN_GROUND: its ground, -touchdown_z)."""
    rec = seeded_record()
    moved = rectangle(0.2, 0.13, 0.25, -1.0, (1.5, -1.75, 0.525))
    for rule in ("contact", "swing_state"):
        rows = [(v, want) for r, v, want in ODD if r == rule]
        vals, idx = cycle(np.float32([v for v, _ in rows]))
        want = np.array([w for _, w in rows])[idx]
        inp = {"pos_feet": np.tile(moved, (B_EDGE, 1, 1)), rule: np.tile(vals[:, None], (1, 4))}
        assert np.array_equal(tr.contact_decision(inp[rule], None, rule == "swing_state")[:, 0], want)
        st, out, ref, _, _ = against_ref(launch, np.tile(rec, (B_EDGE, 1)), inp)
        latched = np.array([same_bits(st[b, tr.HIST], moved.astype(np.float64).reshape(12)) for b in range(B_EDGE)])
        kept = np.array([same_bits(st[b, tr.HIST], rec[tr.HIST]) for b in range(B_EDGE)])
        assert np.array_equal(latched, want) and np.array_equal(kept, ~want), rule
        assert (out["status"] == 0).all()
    # a non-finite foot
    feet, idx = cycle(np.stack([moved] * 3))
    feet = feet.copy()
    for k, bad in enumerate(BAD):
        feet[idx == k, 2, 1] = bad
    contact = np.tile(np.float32([1, 1, 0, 1]), (B_EDGE, 1))
    st, out, _, _, _ = against_ref(launch, np.tile(rec, (B_EDGE, 1)), dict(pos_feet=feet, contact=contact))
    assert (out["status"] == 0).all() and same_bits(st[:, tr.HIST].reshape(-1, 4, 3)[:, 2], np.tile(rec[tr.HIST].reshape(4, 3)[2], (B_EDGE, 1)))
    for ground in (False, True):
        st, out, _, _, _ = against_ref(launch, np.zeros((B_EDGE, tr.STRIDE)), dict(pos_feet=feet, contact=contact), None, ground)
        assert (out["status"] == tr.STATUS_NONFINITE).all() and (st == 0).all()
        level = [0.0, 0.0, 1.0, float(np.float32(-tr.TOUCHDOWN_Z)) if ground else 0.0]
        assert all(out["plane"][b].tolist() == level for b in range(B_EDGE))
        assert all(out["normal"][b].tolist() == [0.0, 0.0, 1.0] for b in range(B_EDGE))


# ---- refusals by the record

RECORD_WORDS = (("history", 4), ("n", tr.N.start + 1), ("d", tr.D), ("fitted", tr.FITTED), ("pad", 19), ("initialised", tr.INIT))


def bad_records():
    """[19,STRIDE]: the seeded record with NaN, +inf, -inf in turn in a history word, n, d,
    fitted, a pad word and `initialised` itself (6 x 3), and a record full of NaN whose
    `initialised` is 0, which is not refused: it is reseeded."""
    rec = seeded_record()
    rows = []
    for _, w in RECORD_WORDS:
        for bad in BAD:
            r = rec.copy()
            r[w] = bad
            rows.append(r)
    cold = np.full(tr.STRIDE, np.nan)
    cold[tr.INIT] = 0.0
    return np.stack(rows + [cold]), rec


def check_bad_records(launch):
    """A bad record between clean neighbours (every third robot carries one): refused with
    MPCQP_STATUS_NONFINITE, its bytes untouched, its outputs formed from the record as it was;
    the neighbours bitwise the run in which every record is clean."""
    rows, rec = bad_records()
    moved = rectangle(0.2, 0.13, 0.25, -1.0, (1.5, -1.75, 0.525))
    B = B_EDGE
    state = np.tile(rec, (B, 1))
    carrier = np.arange(B) % 3 == 1
    which = (np.arange(B) // 3) % len(rows)
    state[carrier] = rows[which[carrier]]
    assert set(which[carrier]) == set(range(len(rows)))
    rob0 = np.arange(B * 16, dtype=np.float32).reshape(B, 16)
    inp = dict(pos_feet=np.tile(moved, (B, 1, 1)), contact=np.ones((B, 4), np.float32), robot=rob0)
    clean_st, clean_out = launch(np.tile(rec, (B, 1)), inp, None, True)
    st, out, ref, want, _ = against_ref(launch, state, inp, None, True)
    reseeded = carrier & (which == len(rows) - 1)
    refused = carrier & ~reseeded
    assert np.array_equal(out["status"] != 0, refused) and (out["status"][refused] == tr.STATUS_NONFINITE).all()
    assert same_bits(st[refused], state[refused])
    for k in ("normal", "plane", "status", "robot"):
        assert same_bits(out[k][~carrier], clean_out[k][~carrier]), k
    assert same_bits(st[~carrier], clean_st[~carrier])
    src = tr.as_was(state)
    for b in np.flatnonzero(refused):
        assert np.array_equal(out["normal"][b], src[b, tr.N].astype(np.float32), equal_nan=True), b
        assert np.array_equal(out["robot"][b, 9:12], out["normal"][b], equal_nan=True)
    fresh, _ = tr.tick_step(np.zeros((1, tr.STRIDE)), moved[None], np.ones((1, 4), bool))
    for b in np.flatnonzero(reseeded):
        assert tr.norm_err(st[b], fresh[0]) <= N_BOUND and same_bits(st[b, tr.HIST], fresh[0, tr.HIST]), b
    return int(refused.sum())


# ---- far from the origin

def far_feet():
    """The footprint on a plane 0.3 rad off level with the base 1e4 and 1e5 m out, where float32
    positions are 1e-3 and 8e-3 m apart: [B_EDGE,4,3] float32, a different azimuth per robot."""
    rows = []
    for b in range(B_EDGE):
        r, az = (1e4, 1e5)[b % 2], 0.37 * b
        c = np.array([r * np.cos(1.0 + b), r * np.sin(1.0 + b), 0.0])
        n = rotation(0.3, az)[:, 2]
        c[2] = -(n[0] * c[0] + n[1] * c[1]) / n[2]            # the plane goes through the origin
        rows.append(rectangle(0.2, 0.13, 0.3, az, c))
    return np.stack(rows)


def check_far_from_the_origin(launch):
    """Device against restatement within N_BOUND (d relative to |mu|), the decision the
    restatement's: at this spacing of the float32 positions the fit may be held."""
    f = far_feet()
    worst = 0.0
    st = np.zeros((B_EDGE, tr.STRIDE))
    fitted = []
    for c in (np.ones((B_EDGE, 4), np.float32), np.tile(np.float32([1, 0, 0, 1]), (B_EDGE, 1))):
        st, out, ref, want, w = against_ref(launch, st, dict(pos_feet=f, contact=c, quat=np.tile(np.float32([1, 0, 0, 0]), (B_EDGE, 1))))
        worst = max(worst, w * N_BOUND)
        fitted.append(ref[:, tr.FITTED].mean())
        f = f + np.float32([0.125, 0.0, 0.0])
    return worst, fitted


# ---- the ground flag

def check_ground_flag(launch, traj):
    """MPCQP_TERRAIN_GROUND over six ticks of the trajectory: the fourth word of `plane` is
    d - n_z touchdown_z of the restatement; the record and every other output are bitwise the
    launch without the flag."""
    st = np.zeros((B_EDGE, tr.STRIDE))
    worst = 0.0
    for t in range(6):
        inp = dict(pos_feet=traj[t]["pos_feet"][:B_EDGE], swing_state=traj[t]["swing_state"][:B_EDGE],
                   quat=traj[t]["quat"][:B_EDGE], robot=np.zeros((B_EDGE, 16), np.float32))
        plain_st, plain = launch(st, inp, None, False)
        st, out, ref, want, _ = against_ref(launch, st, inp, None, True)
        assert same_bits(st, plain_st)
        for k in ("normal", "normal_base", "status", "robot"):
            assert same_bits(out[k], plain[k]), k
        assert same_bits(out["plane"][:, :3], plain["plane"][:, :3])
        lift = out["plane"][:, 3].astype(np.float64) - (st[:, tr.D] - st[:, tr.N.start + 2] * tr.TOUCHDOWN_Z)
        worst = max(worst, float(np.abs(lift / np.maximum(1.0, np.abs(st[:, tr.D]))).max()))
        assert not same_bits(out["plane"][:, 3], plain["plane"][:, 3])
    assert worst <= 2.0 ** -23                                # one float32 rounding of the float64 value, |value| < 2 max(1, |d|)
    return worst

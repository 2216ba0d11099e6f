"""The edge checks of mpcqp_attitude, written once and run twice: by tests/test_att.py on the
host build of csrc/mpcqp_attitude_robot.h and by tests/test_gpu_att_edges.py on the device.
Each check takes ``launch(state [B,STRIDE], inputs, constants) -> (records, outputs)``, both
with two sentinel rows past B that the launcher has already found untouched, and returns the
figures it measured.  The inputs are att_ref's edge tables."""
from fractions import Fraction

import numpy as np

import att_ref
import swing_ref

Q_BOUND = 10 * att_ref.D_Q
UNIT = 4e-16            # | |q| - 1 | after the tick's normalisation: sqrt and four divisions, under 2 ulps


def unit_bound(norm):
    """| |q| - 1 | after a tick from a seeded quaternion of length `norm`.  The tick normalises
    by s = sqrt(sum of four squares); below |q| = 1e-146 or so the squares are subnormal and
    each is rounded to a multiple of 2^-1074, an absolute error of 2^-1075 apiece (their sums
    are exact), so s is off by 4 * 2^-1075 / (2 |q|^2) relative: 4.9e-4 at 1e-160."""
    return max(UNIT, 2.0 ** -1074 / norm ** 2)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def trust_exact(tick, ibm, rec, leg, window):
    """One leg's trust as an exact rational (a Fraction; `window` is taken as the float64 it
    is), from swing_ref.decide_exact's unbounded integers -- nothing shared with att_ref."""
    swing, _, cs, nsw = swing_ref.decide_exact(tick, ibm, rec, leg)
    period, dur = int(rec[0]), int(rec[5 + leg])
    if swing:
        return Fraction(0)
    nst = dur * int(ibm)
    if period <= 0 or nsw <= 0 or nst <= 0 or not window > 0:
        return Fraction(1)
    k = nst if cs == 0 else cs - nsw
    phi = Fraction(2 * k - 1, 2 * nst)
    w = Fraction(window)
    return min(Fraction(1), phi / w, (1 - phi) / w)


def worst_record(st, ref):
    return max(att_ref.record_err(a, r) for a, r in zip(st, ref))


def check_trust_table(launch, ibm, window):
    """3a.  A robot per row of the leg controller's decision table, each on its own tick:
    the trust is the float32 of att_ref.gait_trust bitwise, 0 exactly where
    swing_ref.decide_exact says swing, and within 2^-24 (one float32 rounding) of the exact
    rational.  Returns the set of kinds of value seen."""
    tick, gait = att_ref.trust_edges(ibm)
    B = len(tick)
    inp = dict(att_ref.level(B), tick=tick, gait=gait, ibm=ibm)
    st, out = launch(np.zeros((B, att_ref.STRIDE)), inp, dict(trust_window=window))
    trust = out["trust"][:B]
    assert trust.dtype == np.float32 and (out["status"][:B] == 0).all()
    assert same_bits(trust, att_ref.gait_trust(tick, ibm, gait, window).astype(np.float32)), (ibm, window)
    kinds = set()
    for b in range(B):
        for leg in range(4):
            exact = trust_exact(tick[b], ibm, gait[b], leg, window)
            got = Fraction(float(trust[b, leg]))
            assert (got == 0) == swing_ref.decide_exact(tick[b], ibm, gait[b], leg)[0], (ibm, window, b, leg)
            assert abs(got - exact) <= Fraction(1, 2 ** 24) * exact, (ibm, window, b, leg, float(got), float(exact))
            kinds.add("zero" if got == 0 else "one" if got == 1 else "ramp")
    assert kinds == ({"zero", "one", "ramp"} if window in (0.2, 0.5) else {"zero", "one"}), (ibm, window, kinds)
    return kinds


def check_touch_threshold(launch):
    """3a, the touch sensor: at the threshold exactly and one float32 below it the trust is
    0; one float32 above it is the gait's."""
    tick, gait = att_ref.trust_edges(20)
    B = len(tick)
    gait_only = att_ref.gait_trust(tick, 20, gait, 0.2).astype(np.float32)
    assert (gait_only > 0).any()
    c = dict(trust_window=0.2, touch_threshold=0.25)
    for row, want in zip(att_ref.touch_at_threshold(0.25), (0 * gait_only, 0 * gait_only, gait_only)):
        inp = dict(att_ref.level(B), tick=tick, gait=gait, ibm=20, touch=np.tile(row, (B, 1)))
        _, out = launch(np.zeros((B, att_ref.STRIDE)), inp, c)
        assert same_bits(out["trust"][:B], want), row


def check_first_tick(launch):
    """3b.  The first-tick special cases, then 5 ticks at 0.3 rad/s on every axis."""
    a = att_ref.FIRST_ACCEL
    B = len(a)
    inp = dict(gyro=np.zeros((B, 3), np.float32), accel=a)
    ref, _ = att_ref.attitude_step(np.zeros((B, att_ref.STRIDE)), inp)
    st, out = launch(np.zeros((B, att_ref.STRIDE)), inp, None)
    st = st[:B]
    first = worst_record(st, ref)
    assert first <= Q_BOUND and (out["status"][:B] == 0).all()
    assert st[:3, :4].tolist() == [[1, 0, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0]]
    assert (st[:, 3] == 0).all() and (st[:, att_ref.BIAS] == 0).all() and (st[:, att_ref.INIT] == 1).all()
    assert np.abs(np.linalg.norm(st[:, :4], axis=1) - 1).max() <= UNIT
    inp = dict(gyro=np.full((B, 3), 0.3, np.float32), accel=a)
    later = 0.0
    for _ in range(5):
        ref, _ = att_ref.attitude_step(ref, inp)
        st, out = launch(st, inp, None)
        st = st[:B]
        later = max(later, worst_record(st, ref))
        assert (out["status"][:B] == 0).all()
    assert later <= Q_BOUND
    return first, later


def check_gate_and_switch(launch):
    """3c.  The gate's corners on a tilted record with kappa_ref = 2 (past 2 g the tick is
    bitwise the tick with kappa_ref = 0; reading gamma as 1 there would move q by
    kappa_ref dt |e| = 7e-4, over 1e11 bounds), and the |theta| < 1e-8 switch."""
    a = att_ref.GATE_ACCEL
    B = len(a)
    start = att_ref.seeded(np.tile(att_ref.TILT, (B, 1)))
    inp = dict(gyro=np.full((B, 3), 0.05, np.float32), accel=a)
    ref, _ = att_ref.attitude_step(start, inp, att_ref.GATE_CONSTANTS)
    open_ref, _ = att_ref.attitude_step(start, dict(inp, accel=np.tile(a[:1], (B, 1))), att_ref.GATE_CONSTANTS)
    st, out = launch(start, inp, att_ref.GATE_CONSTANTS)
    off, _ = launch(start, inp, dict(kappa_ref=0.0))
    gate = worst_record(st[:B], ref)
    closed = list(att_ref.GATE_CLOSED)
    assert gate <= Q_BOUND and (out["status"][:B] == 0).all()
    assert same_bits(st[closed], off[closed]) and not same_bits(st[0], off[0])
    assert min(att_ref.record_err(open_ref[b], ref[b]) for b in closed) >= 100 * Q_BOUND
    g = att_ref.SWITCH_GYRO
    n = len(g)
    start = att_ref.seeded(np.tile([1.0, 0, 0, 0], (n, 1)))
    inp = dict(att_ref.level(n), gyro=g)
    ref, _ = att_ref.attitude_step(start, inp, dict(dt=1e-3))
    st, out = launch(start, inp, dict(dt=1e-3))
    theta = np.abs(g[:, 0].astype(np.float64)) * 1e-3
    assert (theta[0] < 1e-8 < theta[1]) and (out["status"][:n] == 0).all()
    switch = worst_record(st[:n], ref)
    assert switch <= Q_BOUND and st[2, :4].tolist() == [1, 0, 0, 0]
    assert st[0, 1] == 0.5 * theta[0] and st[0, 0] == 1.0      # (1, theta / 2), normalised: 1 + 2e-17 rounds to 1
    return gate, switch


def check_large_rotation(launch):
    """3d.  Up to 23 rad per tick against att_ref at Q_BOUND; at 1e6 and 3e38 rad/s only
    status 0, a finite unit record -- and the distance to att_ref, returned, not asserted: it
    is the argument reduction of this side's sin / cos against the oracle's."""
    g = att_ref.rate_rows(att_ref.LARGE_RATES)
    B = len(g)
    start = att_ref.seeded(np.tile(att_ref.TILT, (B, 1)))
    inp = dict(att_ref.level(B), gyro=g)
    ref, _ = att_ref.attitude_step(start, inp)
    st, out = launch(start, inp, None)
    large = worst_record(st[:B], ref)
    assert large <= Q_BOUND and (out["status"][:B] == 0).all()
    assert 20 < np.linalg.norm(g[-1].astype(np.float64)) * 1e-3 < 25
    g = att_ref.rate_rows(att_ref.HUGE_RATES)
    n = len(g)
    start = att_ref.seeded(np.tile(att_ref.TILT, (n, 1)))
    inp = dict(att_ref.level(n), gyro=g)
    ref, _ = att_ref.attitude_step(start, inp)
    st, out = launch(start, inp, None)
    assert (out["status"][:n] == 0).all() and np.isfinite(st[:n]).all()
    assert np.abs(np.linalg.norm(st[:n, :4], axis=1) - 1).max() <= UNIT
    return large, [att_ref.record_err(st[b], ref[b]) for b in range(n)]


def check_seeded_records(launch):
    """3e.  A seeded quaternion of norm 2, 1e-3 and 1e-160 comes out unit and follows att_ref;
    a zero one, or one of norm 1e150, is misuse: no other robot notices, and from the second
    tick on that robot has status 4 and its record stays as it is."""
    norms = att_ref.SEED_NORMS + att_ref.MISUSE_NORMS
    B, good = len(norms), len(att_ref.SEED_NORMS)
    start = att_ref.seeded(np.array(norms)[:, None] * att_ref.TILT[None])
    # level and at rest but for a small rate: gamma = 1 and e != 0 on the tilted records, so a
    # quaternion of norm 1e150 overflows |theta|; the zero one normalises 0 / 0
    cut = lambda d: {k: v[:good] for k, v in d.items()}
    inp = dict(att_ref.level(B), gyro=np.full((B, 3), 0.05, np.float32))
    inp2 = dict(att_ref.level(B), gyro=np.full((B, 3), -0.02, np.float32))
    ref, _ = att_ref.attitude_step(start, inp)
    st, out = launch(start, inp, None)
    seeded = worst_record(st[:good], ref[:good])
    assert seeded <= Q_BOUND and (out["status"][:good] == 0).all()
    off_unit = np.abs(np.linalg.norm(st[:good, :4], axis=1) - 1)
    assert all(off_unit[b] <= unit_bound(norms[b]) for b in range(good)), off_unit
    alone, _ = launch(start[:good], cut(inp), None)
    assert same_bits(st[:good], alone[:good])
    st2, out2 = launch(st[:B], inp2, None)
    alone2, _ = launch(alone[:good], cut(inp2), None)
    assert (out2["status"][good:B] == 4).all() and same_bits(st2[good:B], st[good:B]) and same_bits(st2[:good], alone2[:good])
    st3, out3 = launch(st2[:B], inp, None)
    assert (out3["status"][good:B] == 4).all() and same_bits(st3[good:B], st[good:B]) and (out3["status"][:good] == 0).all()
    return seeded


def check_refusal_across_a_workgroup(launch):
    """3e.  B = 65: a non-finite record word (q, `initialised`, bias) at robots 63 and 64, the
    last lane of one workgroup and the first of the next: status 4, the record as it was,
    robot 62 and every other row bitwise the clean launch's."""
    B = 65
    traj = att_ref.make_trajectory(B, 4, seed=13)
    start = att_ref.run(traj[:3])[0][-1]
    clean = launch(start, traj[3], None)
    for word, value in ((2, np.nan), (att_ref.INIT, np.inf), (6, -np.inf)):
        dirty_start = start.copy()
        dirty_start[[63, 64], word] = value
        st, out = launch(dirty_start, traj[3], None)
        assert out["status"][:B].tolist() == [0] * 63 + [4, 4], word
        assert same_bits(st[[63, 64]], dirty_start[[63, 64]])
        assert same_bits(out["quat"][[63, 64]], dirty_start[[63, 64], :4].astype(np.float32))
        keep = [b for b in range(B + 2) if b not in (63, 64)]
        assert same_bits(st[keep], clean[0][keep]) and all(same_bits(out[k][keep], clean[1][k][keep]) for k in out), word

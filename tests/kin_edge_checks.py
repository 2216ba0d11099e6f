"""The edge checks of mpcqp_kinematics, written once and run twice: by tests/test_kin.py on
the host build of csrc/mpcqp_kin_leg.h and by tests/test_gpu_kin_edges.py on the device.  Each
takes ``run(geom [B,5], inputs, layout, rot) -> {output: float32 [B + pad, ...]}`` (layout
"split", "root" or "rot"; the rows past B are sentinels the runner has found untouched).  The
inputs are kin_ref's edge tables."""
import numpy as np

import kin_ref
from kin_ref import OUTPUTS

BOUND = 2.4e-7
DIRTY = (63, 64)        # of B = 65: the last robot of one workgroup and the first of the next


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_edge_poses(run, layout):
    """4a.  B = 12 in one launch against kin_ref at BOUND, norm-wise per robot; where the
    reference output of a robot is all zero (zero geometry) the output is exactly 0.  Returns
    {output: worst error}."""
    geom, inp, rot = kin_ref.edge_poses()
    rot = rot if layout == "rot" else None
    B = len(geom)
    out = run(geom, inp, layout, rot)
    with np.errstate(all="ignore"):
        ref = kin_ref.kinematics(geom, rot=rot, **inp)
    worst = {}
    zero_rows = 0
    for k in OUTPUTS:
        worst[k] = 0.0
        for b in range(B):
            assert np.isfinite(ref[k][b]).all() and np.isfinite(out[k][b]).all(), (k, b)
            if np.abs(ref[k][b]).max() == 0.0:
                assert (out[k][b] == 0).all(), (layout, k, kin_ref.EDGE_ROWS[b])
                zero_rows += 1
            else:
                e = kin_ref.norm_err(out[k][b], ref[k][b])
                assert e <= BOUND, (layout, k, kin_ref.EDGE_ROWS[b], e)
                worst[k] = max(worst[k], e)
    assert zero_rows >= 3           # zero geometry: feet, thighs, foot_pos_base at least
    return worst


def wrong_reading_moves_the_result():
    """The edges matter: with the quaternion normalised (rows 2 quat, quat / 2), or the calf
    angle read for the thigh's (row calf = 0), kin_ref's feet move by over 100 BOUND."""
    geom, inp, _ = kin_ref.edge_poses()
    ref = kin_ref.kinematics(geom, **inp)
    q = inp["quat"].astype(np.float64)
    n = np.linalg.norm(q, axis=1, keepdims=True)
    unit = kin_ref.kinematics(geom, **dict(inp, quat=(q / np.where(n > 0, n, 1)).astype(np.float32)))
    swapped = inp["q"].copy()
    swapped[:, 1::3] = inp["q"][:, 2::3]
    swap = kin_ref.kinematics(geom, **dict(inp, q=swapped))
    return min(kin_ref.norm_err(unit["feet"][b], ref["feet"][b]) for b in (6, 7)), kin_ref.norm_err(swap["feet"][2], ref["feet"][2])


def check_nan_stays_put(run, layout):
    """4b.  B = 65, one launch per input with a NaN for robots 63 and 64: the (output, leg)
    pairs kin_ref makes non-finite are non-finite, every other one of the dirty robots is
    bitwise the clean launch's -- its other legs included -- and so is every other robot and
    the sentinel rows."""
    B = 65
    geom, inp, rot = kin_ref.ordinary(B, seed=23)
    seen = {}
    for key, idx in kin_ref.NAN_CASES:
        if key == "rot" and layout != "split":
            continue
        use_rot = rot if key == "rot" else None
        lay = "rot" if key == "rot" else layout
        clean = run(geom, inp, lay, use_rot)
        g2, i2, r2 = geom.copy(), {k: v.copy() for k, v in inp.items()}, None if use_rot is None else use_rot.copy()
        for b in DIRTY:
            if key == "geom":
                g2[b, idx] = np.nan
            elif key == "rot":
                r2[b].reshape(-1)[idx] = np.nan
            else:
                i2[key][b, idx] = np.nan
        dirty = run(g2, i2, lay, r2)
        with np.errstate(all="ignore"):
            ref = kin_ref.kinematics(g2, rot=r2, **i2)
        pattern = set()
        for k in OUTPUTS:
            rows = np.ones(len(clean[k]), bool)
            rows[list(DIRTY)] = False
            assert same_bits(dirty[k][rows], clean[k][rows]), (key, idx, k)
            for b in DIRTY:
                for leg in range(4):
                    if np.isfinite(ref[k][b, leg]).all():
                        assert same_bits(dirty[k][b, leg], clean[k][b, leg]), (key, idx, k, b, leg)
                    else:
                        assert same_bits(np.isfinite(dirty[k][b, leg]), np.isfinite(ref[k][b, leg])), (key, idx, k, b, leg)
                        pattern.add((k, leg))
        seen[key, idx] = pattern
    legs = lambda p, k: {l for kk, l in p if kk == k}
    every = {(k, l) for k in OUTPUTS for l in range(4)}
    assert seen["quat", 2] == every
    assert seen["pos", 1] == {("pos_feet", l) for l in range(4)}
    assert seen["vel", 0] == seen["omega", 2] == {("foot_vel_base", l) for l in range(4)}
    assert seen["q", 4] == {(k, 1) for k in OUTPUTS if k != "thighs"} and seen["q", 11] == {(k, 3) for k in OUTPUTS if k != "thighs"}
    assert seen["q", 6] == {(k, 2) for k in OUTPUTS}
    assert seen["qdot", 1] == {("foot_vel_base", 0)}
    if layout == "split":
        assert seen["rot", 5] == {(k, l) for k in ("thighs", "foot_pos_base", "foot_vel_base") for l in range(4)}
    return seen

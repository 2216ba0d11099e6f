"""CPU: the rigid-body plant (mpcqp_plant) without a GPU -- the ABI and Python surface, the
per-robot header csrc/mpcqp_plant_robot.h compiled with g++ and driven through ctypes against the
float64 restatement tests/plant_ref.py, the inverse kinematics against kin_ref.chain, physics with
known answers, and the closed loop on the CPU oracles of the controller: it walks.

Measured here (printed by the tests):
  the host-compiled header against plant_ref on 512 seeded single ticks per setting (substeps 1
    and 3, level ground and a tilted plane; stance, friction clamp, release, swing, touchdown on
    every leg): the record 1.3e-15 norm-wise per robot, the float32 outputs equal, contact flags,
    flag word and call count equal; no state within 1e-9 of a switching threshold.
  kin_ref.chain(ik(p)) against p: 6.7e-16 over 1000 seeded poses, 3.1e-16 at worst over
    kin_ref.edge_poses(), its stretched legs (q = 0, calf = 0) and its legs folded onto the thigh
    joint (q = (pi, -pi, pi), q = (pi/2, pi/2, -pi)) included: the clamp is applied to 1 - cos(calf)
    and 1 + cos(calf), where eps = 2^-90 is representable.
  free fall over 1000 ticks, tumbling at 2.9 rad/s: position against the discrete parabola
    2.2e-14, I_w w conserved to 1.7e-13, |quat| - 1 below 2.3e-16.
  the stand over 1000 ticks: the record moves by 1.8e-15.
  the closed loop (Aliengo, TROTTING10, N = 10, 1000 ticks, commands 0 / 0.5 / 1.0 m/s):
    worst |height - 0.38|  0.01086  0.01094  0.01109 m
    worst |roll|, |pitch|  3.3e-8   0.0336   0.0854 rad  (the first 250 ticks, the start from
                                                          rest; 0.005 / 0.010 rad from tick 1500 on)
    mean speed, last 500   0.0000   0.5210   1.0442 m/s
    every solve converged; all four feet are off the ground for about 2 ticks per half period.
    These are plant_ref.CLOSED_LOOP, the yardstick of tests/test_gpu_plant.py.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import kin_ref
import plant_ref as pr
from helpers import _vp, host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANT_HEADER = os.path.join(ROOT, "include", "mpcqp_plant_abi.h")
CPU_BOUND = 1e-12      # both sides are float64 with libm: the gap is rounding
IK_BOUND = 1e-13

SHIM = r'''
#include "mpcqp_plant_robot.h"
// a launch of mpcqp_plant_kernel, robot after robot; par: dt_control, gravity, foot_mass,
// ground_z, contact_tol, substeps
extern "C" void plant_step(int B, const double* par, double* rec, const float* tau, const float* robot,
                           const double* geom, const float* plane, float* root, float* dofs, float* gyro, float* accel,
                           float* touch, int* status) {
  PlantParams P{par[0], par[1], par[2], par[3], par[4], (int)par[5]};
  for (int b = 0; b < B; ++b)
    status[b] = plant_robot_step(P, rec + PLANT_STRIDE * b, tau + 12 * b, robot + 16 * b, geom + KIN_STRIDE * b,
                                 plane ? plane + 4 * b : nullptr, root + 13 * b, dofs + 24 * b, gyro + 3 * b,
                                 accel + 3 * b, touch + 4 * b);
}
extern "C" void plant_reset(int B, const double* par, const float* root, const float* dofs, const double* geom,
                            const float* plane, double* rec) {
  PlantParams P{par[0], par[1], par[2], par[3], par[4], (int)par[5]};
  for (int b = 0; b < B; ++b)
    plant_robot_reset(P, root + 13 * b, dofs + 24 * b, geom + KIN_STRIDE * b, plane ? plane + 4 * b : nullptr,
                      rec + PLANT_STRIDE * b);
}
extern "C" int leg_ik(const double* geom, int leg, const double* p, double* q) { return plant_leg_ik(geom, leg, p, q); }
extern "C" int stride(void) { return PLANT_STRIDE; }
extern "C" int words(void) { return PLANT_WORDS; }
extern "C" int status_nonfinite(void) { return PLANT_STATUS_NONFINITE; }
extern "C" double ik_eps(void) { return PLANT_IK_EPS; }
'''


@pytest.fixture(scope="module")
def header():
    lib = host_build(SHIM, name="plant")
    lib.ik_eps.restype = ctypes.c_double
    return lib


def _par(par):
    return np.array([par.dt_control, par.gravity, par.foot_mass, par.ground_z, par.contact_tol, par.substeps], float)


def run_header(lib, rec, tau, robot, geom, par, plane=None):
    """plant_ref.plant_step's dict from the host-compiled header; rec is advanced in place."""
    B = len(rec)
    out = dict(root=np.zeros((B, 13), np.float32), dofs=np.zeros((B, 12, 2), np.float32), gyro=np.zeros((B, 3), np.float32),
               accel=np.zeros((B, 3), np.float32), touch=np.zeros((B, 4), np.float32))
    status = np.zeros(B, np.int32)
    assert rec.flags.c_contiguous and rec.dtype == np.float64
    pl = None if plane is None else np.ascontiguousarray(plane, np.float32)
    lib.plant_step(B, _vp(_par(par)), _vp(rec), _vp(np.ascontiguousarray(tau, np.float32)),
                   _vp(np.ascontiguousarray(robot, np.float32)), _vp(np.ascontiguousarray(geom, np.float64)), _vp(pl),
                   *[_vp(out[k]) for k in ("root", "dofs", "gyro", "accel", "touch")], _vp(status))
    out["status"] = status
    return out


# ---- the ABI and Python surface

def test_strides_agree(header):
    from mpcqp import _lib, params
    src = open(PLANT_HEADER).read()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", src).group(1))
    assert define("MPCQP_PLANT_STRIDE") == _lib.PLANT_STRIDE == params.PLANT_STRIDE == pr.STRIDE == header.stride() == 48
    assert define("MPCQP_PLANT_MAX_SUBSTEPS") == _lib.PLANT_MAX_SUBSTEPS == 16
    assert header.words() == pr.WORDS == 43 and header.status_nonfinite() == pr.STATUS_NONFINITE == _lib.STATUS_NONFINITE
    assert header.ik_eps() == pr.IK_EPS == 2.0 ** -90


def test_null_ctx_is_an_error_code():
    """Every call refuses a NULL context with -1.  The other misuse rules need a context, which
    needs a device: tests/test_gpu_plant.py checks them."""
    from mpcqp import _lib
    lib = _lib.load()
    assert lib.mpcqp_plant(None, 1, 0, *([None] * 12)) == -1
    assert lib.mpcqp_plant_reset(None, 1, *([None] * 6)) == -1
    assert lib.mpcqp_set_plant(None, 0.15, 1, 0.0, 1e-4) == -1


def test_python_surface():
    import mpcqp
    from mpcqp.plant import BatchedPlant
    assert "BatchedPlant" in mpcqp.__all__ and mpcqp.BatchedPlant is BatchedPlant
    for name in ("reset", "step", "bind_step", "set_constants"):
        assert getattr(BatchedPlant, name).__doc__
    for name in ("contact", "feet_world", "flags"):
        assert isinstance(getattr(BatchedPlant, name), property)


# ---- the header against the restatement

@pytest.mark.parametrize("substeps, tilted", [(1, False), (3, False), (1, True)])
def test_header_matches_the_restatement_on_single_ticks(header, substeps, tilted):
    B = 512
    par = pr.Params(substeps=substeps)
    st = pr.make_states(B, seed=5 + substeps, par=par)
    plane = None
    if tilted:   # a slope through the level ground's height under the origin: contact feet hover or dig a little
        n = np.array([0.05, -0.03, 1.0])
        n /= np.linalg.norm(n)
        plane = np.tile(np.r_[n, n[2] * par.ground_z].astype(np.float32), (B, 1))
    near = pr.near_threshold(st["rec"], st["tau"], st["robot"], st["geom"], par, plane)
    print(f"\nsubsteps {substeps} tilted {tilted}: {near.mean():.4f} of the states within {pr.BAND:g} of a threshold")
    assert near.mean() <= 0.02
    ref = st["rec"].copy()
    want = pr.plant_step(ref, st["tau"], st["robot"], st["geom"], par, plane)
    got_rec = st["rec"].copy()
    got = run_header(header, got_rec, st["tau"], st["robot"], st["geom"], par, plane)
    keep = ~near
    err = pr.record_error(got_rec, ref)[keep]
    print(f"record, norm-wise per robot: worst {err.max():.2e} (bound {CPU_BOUND:g})")
    assert err.max() <= CPU_BOUND
    assert np.array_equal(got_rec[keep, pr.CONTACT:pr.WORDS], ref[keep, pr.CONTACT:pr.WORDS])    # contact, flag word, count
    assert np.array_equal(got["status"], want["status"]) and (want["status"] == 0).all()
    for k in ("root", "dofs", "gyro", "accel"):
        e = np.array([kin_ref.norm_err(got[k][b], want[k][b]) for b in np.flatnonzero(keep)])
        print(f"{k}: worst {e.max():.2e}")
        assert e.max() <= 2.0 ** -23, k              # float32 roundings of values 1e-15 apart: one ulp at the most
    assert np.array_equal(got["touch"][keep], want["touch"][keep])
    if tilted:        # on the slope a foot may start under the plane: the cases are level ground's
        return
    # every case took place: contacts kept, released and made
    before, after = st["rec"][:, pr.CONTACT:pr.CONTACT + 4] != 0, ref[:, pr.CONTACT:pr.CONTACT + 4] != 0
    case = st["case"]
    assert after[case <= 1].all() and not after[case == 3].any() and not before[case >= 3].any()
    assert (~after[case == 2]).mean() > 0.9 and after[case == 4].mean() > (0.9 if substeps == 1 else 0.3)
    assert (got_rec[:, pr.FLAGS] == 0).all() and np.array_equal(got_rec[:, pr.TICK], st["rec"][:, pr.TICK] + 1)


def check_set(st, par, trace, ref):
    """What a seeded set promises, from the restatement alone (shared with
    tests/test_gpu_plant_edges.py): every case occurs and does what its name says in at least
    90 % of its legs, the flag words are the set's, the slow set turns slowly."""
    case = st["case"]
    after = ref[:, pr.CONTACT:pr.CONTACT + 4] != 0
    land = np.any([t["land"] for t in trace], 0)
    share = {"stance": after[case == 0].mean(), "friction clamp": (trace[0]["over"] & after)[case == 1].mean(),
             "release": trace[0]["release"][case == 2].mean(), "swing": (~trace[0]["pinned"])[case == 3].mean(),
             "touchdown": land[case == 4].mean()}
    if "still" not in st:                            # the slow set leaves most robots one case
        assert all((case == k).sum() >= 4 for k in range(len(pr.CASES)))
        assert min(share.values()) >= 0.9, share
        assert not trace[0]["over"][case == 0].any()
    assert np.array_equal(ref[:, pr.FLAGS], st["word"] if "word" in st else np.zeros(len(ref)))
    if "still" in st:
        t = np.stack([x["t"] for x in trace])
        assert (t < 1e-6).all(0).mean() > 0.5 and (t[:, st["zero"]] == 0.0).all() and st["zero"].any()
        assert (t[:, st["still"]] < 1e-15).all()
        assert ((t > 0.0) & (t < 1e-6)).all(0).mean() > 0.25           # the small branch with a turn that is not zero
        assert (t >= 1e-6).all(0).mean() > 0.1                          # and the large one
        assert np.abs(t / 1e-6 - 1.0).min() > 1e-6                     # no robot on the branch point itself
        kept = ref[:, pr.QUAT:pr.QUAT + 4].view(np.uint64) == st["rec"][:, pr.QUAT:pr.QUAT + 4].view(np.uint64)
        assert kept[st["zero"]].all()
    return share


SETS = {"mixed": (pr.make_mixed_states, 22), "clamped": (pr.make_clamped_states, 31), "slow": (pr.make_slow_states, 40)}


@pytest.mark.parametrize("substeps", [1, 16])
@pytest.mark.parametrize("name", sorted(SETS))
def test_header_matches_the_restatement_on_the_edge_sets(header, name, substeps):
    """The sets of tests/test_gpu_plant_edges.py through the host-compiled header: a mixed fleet
    (A1 and Aliengo in turn, own mass, mu, inertia) on per-robot slopes, legs at every clamp of
    the inverse kinematics, rotations in the small branch of plant_quat_step; substeps 1 and 16,
    the ABI's maximum.  Measured here, the record norm-wise per robot at substeps 1 / 16: mixed
    8.5e-16 / 3.1e-15, clamped 6.6e-16 / 3.3e-15, slow 7.5e-16 / 6.8e-16; every float32 output
    within one ulp, flag words equal, no robot within 1e-9 of a threshold."""
    B = 512
    make, seed = SETS[name]
    par = pr.Params(substeps=substeps)
    st = make(B, seed, par)
    plane = st.get("plane")
    args = (st["tau"], st["robot"], st["geom"], par, plane)
    near = pr.near_threshold(st["rec"], *args)
    assert near.mean() <= 0.02
    ref = st["rec"].copy()
    want = pr.plant_step(ref, *args)
    share = check_set(st, par, pr.trace_step(st["rec"], *args), ref)
    got_rec = st["rec"].copy()
    got = run_header(header, got_rec, *args)
    keep = ~near
    cl = st.get("clamped", np.zeros((B, 4), bool))
    # a clamped leg's foot falls freely and is compared; its hip and thigh angles and its joint
    # rates hang on rounding noise (J_b^-1 near 1e14) and are not
    err = pr.record_error(got_rec, ref)[keep]
    print(f"\n{name}, substeps {substeps}: {near.mean():.4f} near a threshold, cases {share}\n"
          f"record, norm-wise per robot: worst {err.max():.2e} (bound {CPU_BOUND:g})")
    assert err.max() <= CPU_BOUND
    assert np.array_equal(got_rec[keep, pr.CONTACT:pr.WORDS], ref[keep, pr.CONTACT:pr.WORDS])    # contact, flag word, count
    assert np.array_equal(got_rec[:, pr.FLAGS], ref[:, pr.FLAGS])
    assert np.array_equal(got["status"], want["status"]) and (want["status"] == 0).all()
    for out in (got, want):
        assert all(np.isfinite(out[k]).all() for k in ("root", "dofs", "gyro", "accel")) and np.isfinite(got_rec).all()
        knee = -out["dofs"].reshape(B, 4, 3, 2)[:, :, 2, 0].astype(np.float64)[cl & (st.get("kind") == 0)]
        assert (knee > 0).all() and (knee <= np.sqrt(2 * pr.IK_EPS) * (1 + 1e-6)).all()       # stretched: at its clamp
        fold = np.pi + out["dofs"].reshape(B, 4, 3, 2)[:, :, 2, 0].astype(np.float64)[cl & (st.get("kind") == 1)]
        assert (np.abs(fold) <= 2.0 ** -22).all()                                             # folded: -pi, in float32
    moving = ~st.get("still", np.zeros(B, bool))          # a robot at rest: its gyro is rounding noise, 1e-19
    assert np.abs(got["gyro"][~moving]).max(initial=0.0) <= 1e-15 and np.abs(want["gyro"][~moving]).max(initial=0.0) <= 1e-15
    for k in ("root", "gyro", "accel"):
        e = np.array([kin_ref.norm_err(got[k][b], want[k][b]) for b in np.flatnonzero(keep & (moving | (k != "gyro")))])
        assert e.max() <= 2.0 ** -23, k
    gd, wd = got["dofs"].reshape(B, 4, 6), want["dofs"].reshape(B, 4, 6)
    e = max(kin_ref.norm_err(gd[b][~cl[b]], wd[b][~cl[b]]) for b in np.flatnonzero(keep & ~cl.all(1)))
    assert e <= 2.0 ** -23
    assert np.array_equal(got["touch"][keep], want["touch"][keep])
    assert np.array_equal(got_rec[:, pr.TICK], st["rec"][:, pr.TICK] + 1)


def test_make_states_gives_what_it_gave():
    """The new builders leave make_states alone: its records replay the golden fixture's
    (tests/test_gpu_plant.py), and A1 drawn by it stands beyond its reach, which is why the mixed
    fleet draws the base height from each robot's own legs."""
    st = pr.make_states(512, seed=21, robot="a1")
    ref = st["rec"].copy()
    pr.plant_step(ref, st["tau"], st["robot"], st["geom"], pr.Params())
    assert (ref[:, pr.FLAGS] != 0).any()
    # weighted sums of what it returned before the new builders came (the cases, the records, the
    # torques): a draw added, dropped or moved in its sequence changes them in the first digit
    for (B, kw), (cases, rec, tau) in ((((512, dict(seed=6))), (159479, 4737.5668883353665, 226.85155916317117)),
                                       ((8, dict(seed=0)), (2452, -896.8553727690638, 77.48438029981122)),
                                       ((512, dict(seed=21, robot="a1")), (154924, 3117.150495678319, 735.7598306831137))):
        st = pr.make_states(B, **kw)
        w = np.cos(np.arange(st["rec"].size)).reshape(st["rec"].shape)
        assert int(st["case"].astype(np.int64).dot(5 ** np.arange(4)).sum()) == cases
        assert abs((st["rec"] * w).sum() - rec) <= 1e-9 and abs((st["tau"].astype(np.float64) * w[:, :12]).sum() - tau) <= 1e-9
        assert (st["robot"] == st["robot"][0]).all() and (st["geom"] == st["geom"][0]).all()


@pytest.mark.parametrize("scale", [2.0, 0.5])
def test_a_record_quaternion_off_unit_length_is_applied_as_given(header, scale):
    """kin_quat2matrix and kin_ref.quat2matrix_eigen apply the quaternion as given (the ABI asks
    for no unit length, only a non-zero one): the header and the restatement agree on a record
    whose quaternion has norm 2 or 0.5, status OK, and the quaternion they leave is of unit
    length (plant_quat_step normalises)."""
    par = pr.Params()
    st = pr.make_states(16, seed=9, par=par)
    rec = st["rec"].copy()
    rec[:, pr.QUAT:pr.QUAT + 4] *= scale
    rec[:, pr.CONTACT:pr.CONTACT + 4] = 0.0               # the feet of the unit pose are far from the scaled one's legs
    ref, got_rec = rec.copy(), rec.copy()
    tau = np.zeros_like(st["tau"])                        # and some are at a clamp: no torque through J_b^-1
    want = pr.plant_step(ref, tau, st["robot"], st["geom"], par)
    got = run_header(header, got_rec, tau, st["robot"], st["geom"], par)
    assert (want["status"] == 0).all() and (got["status"] == 0).all()
    body = slice(0, pr.FEET)
    assert np.abs(got_rec[:, body] - ref[:, body]).max() <= CPU_BOUND * np.abs(ref[:, body]).max()
    assert np.array_equal(got_rec[:, pr.CONTACT:pr.WORDS], ref[:, pr.CONTACT:pr.WORDS])
    assert np.abs(np.linalg.norm(ref[:, pr.QUAT:pr.QUAT + 4], axis=1) - 1.0).max() <= 1e-15
    for k in ("root", "gyro", "accel"):
        assert max(kin_ref.norm_err(got[k][b], want[k][b]) for b in range(16)) <= 2.0 ** -23, k


def test_reset_matches_the_restatement(header):
    B = 64
    par = pr.Params(contact_tol=2e-3)
    geom, inp, _ = kin_ref.ordinary(B, seed=3)
    geom = np.concatenate([geom, np.zeros((B, 3))], 1)
    root = kin_ref.root_states(inp["quat"], inp["pos"], inp["vel"], inp["omega"])
    dofs = kin_ref.dof_states(inp["q"], inp["qdot"])
    ref = pr.reset(root, dofs, geom, par)
    lowest = ref[:, pr.FEET:pr.FEET + 12].reshape(B, 4, 3)[:, :, 2].min(1)
    plane = np.tile(np.float32([0, 0, 1, 0]), (B, 1))
    plane[:, 3] = lowest - 1e-3                       # the lowest foot within the tolerance, the others as it falls
    ref = pr.reset(root, dofs, geom, par, plane)
    got = np.full((B, pr.STRIDE), 7.0)
    header.plant_reset(B, _vp(_par(par)), _vp(root), _vp(dofs), _vp(np.ascontiguousarray(geom)), _vp(plane), _vp(got))
    assert np.abs(got - ref).max() <= 1e-14 and np.array_equal(got[:, pr.CONTACT:], ref[:, pr.CONTACT:])
    assert 0 < ref[:, pr.CONTACT:pr.CONTACT + 4].sum() < 4 * B


# ---- the inverse kinematics

def _round_trip(geom, q, ik=pr.ik):
    p, _, _ = kin_ref.chain(geom, q)
    q2, clamped = ik(geom, p)
    p2, _, _ = kin_ref.chain(geom, q2.reshape(len(q2), 12))
    return p, p2, q2, clamped


@pytest.mark.parametrize("row", range(len(kin_ref.EDGE_ROWS)), ids=[r.replace(" ", "") for r in kin_ref.EDGE_ROWS])
def test_ik_round_trip_over_the_edge_poses(header, row):
    """kin_ref.chain(ik(p)) returns p to 1e-13, norm-wise, for p = chain(q) of every edge pose:
    stretched legs, legs folded onto the thigh joint, angles of 1e4 rad, a zero geometry."""
    geom, inp, _ = kin_ref.edge_poses()
    p, p2, q2, clamped = _round_trip(geom[row:row + 1], inp["q"][row:row + 1])
    e = kin_ref.norm_err(p2, p)
    print(f"\n{kin_ref.EDGE_ROWS[row]}: round trip {e:.2e}, clamped {clamped[0].tolist()}")
    # the header's plant_leg_ik on the same feet: its own round trip, its clamp bits and its angles
    g8 = np.ascontiguousarray(np.r_[geom[row], np.zeros(3)])
    qh, bits = np.zeros((1, 4, 3)), []
    for leg in range(4):
        q = np.zeros(3)
        bits.append(bool(header.leg_ik(_vp(g8), leg, _vp(np.ascontiguousarray(p[0, leg])), _vp(q))))
        qh[0, leg] = q
    ph, _, _ = kin_ref.chain(geom[row:row + 1], qh.reshape(1, 12))
    eh = kin_ref.norm_err(ph, p)
    print(f"  the header: round trip {eh:.2e}, clamped {bits}")
    assert np.isfinite(qh).all() and bits == clamped[0].tolist() and eh <= IK_BOUND
    # a clamped leg's hip and thigh angles hang on rounding noise (atan2 of two values near zero):
    # the angles are compared where nothing was clamped
    free = ~clamped[0]
    assert np.abs(qh[0][free] - q2[0][free]).max(initial=0.0) <= 1e-12
    assert np.isfinite(q2).all()
    assert e <= IK_BOUND


def test_ik_round_trip_over_seeded_poses(header):
    rng = np.random.default_rng(11)
    B = 250                                           # x 4 legs = 1000 poses
    geom = np.array([kin_ref.A1, kin_ref.ALIENGO])[np.arange(B) % 2]
    q = np.stack([rng.uniform(-1.0, 1.0, (B, 4)), rng.uniform(-1.5, 2.5, (B, 4)), rng.uniform(-2.6, -0.2, (B, 4))], -1)
    p, p2, q2, clamped = _round_trip(geom, q.reshape(B, 12))
    e = max(kin_ref.norm_err(p2[b], p[b]) for b in range(B))
    same = np.abs(np.angle(np.exp(1j * (q2 - q)))).max(-1) < 1e-9     # a thigh past the vertical has a twin pose
    print(f"\n1000 seeded poses: chain(ik(p)) against p {e:.2e}; {same.mean():.2f} of them are the pose itself")
    assert same.mean() > 0.5
    assert e <= IK_BOUND and not clamped.any()
    # the header's IK: the same angles
    g8 = np.concatenate([geom, np.zeros((B, 3))], 1)
    qh = np.zeros(3)
    worst = 0.0
    for b in range(0, B, 7):
        for leg in range(4):
            assert header.leg_ik(_vp(np.ascontiguousarray(g8[b])), leg, _vp(np.ascontiguousarray(p[b, leg])), _vp(qh)) == 0
            worst = max(worst, np.abs(qh - q2[b, leg]).max())
    assert worst <= 1e-14


def test_ik_beyond_reach_sets_the_flag_and_stays_finite(header):
    """A foot 0.2 m beyond a stretched leg: the flag bit of that leg alone, the clamped (stretched)
    pose pointing at the target, and a finite qdot."""
    par = pr.Params()
    st = pr.make_states(4, seed=2, par=par)
    rec = st["rec"].copy()
    rec[:, pr.CONTACT:pr.CONTACT + 4] = 0.0
    feet = rec[:, pr.FEET:pr.FEET + 12].reshape(4, 4, 3)
    feet[:, 2, 2] -= 0.4                              # leg RL: 0.33 .. 0.38 + 0.4 below the hip, reach 0.5
    rec[:, pr.FVEL:pr.FVEL + 12] = 0.3
    for step in (pr.plant_step, lambda *a: run_header(header, *a)):
        r = rec.copy()
        out = step(r, np.zeros((4, 12), np.float32), st["robot"], st["geom"], par)
        assert (out["status"] == 0).all() and (r[:, pr.FLAGS] == 4.0).all()
        assert np.isfinite(out["dofs"]).all() and np.isfinite(r).all()
        knee = -out["dofs"][:, 8, 0].astype(np.float64)                 # at its clamp: within sqrt(2 eps) of straight
        assert (knee > 0).all() and (knee <= np.sqrt(2 * pr.IK_EPS) * (1 + 1e-6)).all()


# ---- physics with known answers (on the restatement; the header is held to the restatement on the
# seeded single ticks above, which take every one of these branches)

def _aliengo(B, par):
    st = pr.make_states(B, seed=1, par=par)
    return st["robot"], st["geom"]


def test_free_fall_is_a_parabola_and_keeps_its_angular_momentum():
    par = pr.Params()
    robot, geom = _aliengo(1, par)
    root, dofs = pr.stand_pose(1, geom, par, height=5.0)
    root[0, 7:10], root[0, 10:13] = (0.3, -0.2, 1.0), (1.5, -2.0, 1.5)
    rec = pr.reset(root, dofs, geom, par)
    assert not rec[:, pr.CONTACT:pr.CONTACT + 4].any()
    p0, v0 = rec[0, :3].copy(), rec[0, pr.VEL:pr.VEL + 3].copy()
    I = pr.inertia(robot)[0]

    def momentum(r):
        R = kin_ref.quat2matrix_eigen(r[None, pr.QUAT:pr.QUAT + 4])[0]
        return R @ I @ R.T @ r[pr.OMEGA:pr.OMEGA + 3]
    L0 = momentum(rec[0])
    worst_p = worst_L = worst_q = 0.0
    g, h = np.array([0, 0, -par.gravity]), par.dt_control
    for k in range(1, 1001):
        out = pr.plant_step(rec, np.zeros((1, 12)), robot, geom, par)
        want = p0 + k * h * v0 + g * h * h * (k * (k + 1) / 2)
        worst_p = max(worst_p, kin_ref.norm_err(rec[0, :3], want))
        worst_L = max(worst_L, kin_ref.norm_err(momentum(rec[0]), L0))
        worst_q = max(worst_q, abs(np.linalg.norm(rec[0, pr.QUAT:pr.QUAT + 4]) - 1.0))
    print(f"\nfree fall: position {worst_p:.2e}, I_w w {worst_L:.2e}, |quat| - 1 {worst_q:.2e}; "
          f"turned to {rec[0, pr.QUAT:pr.QUAT + 4]}")
    assert out["status"][0] == 0 and worst_p <= 1e-12 and worst_L <= 1e-12 and worst_q <= 1e-15
    assert abs(rec[0, pr.QUAT]) < 0.9                 # it tumbled
    assert np.abs(out["accel"]).max() < 1e-6          # an accelerometer in free fall reads nothing


def _stand(par, B=1):
    robot, geom = _aliengo(B, par)
    root, dofs = pr.stand_pose(B, geom, par)
    rec = pr.reset(root, dofs, geom, par)
    assert rec[:, pr.CONTACT:pr.CONTACT + 4].all()
    _, _, Jb = kin_ref.chain(geom, dofs[:, :, 0])
    return robot, geom, rec, Jb


def test_stand_stays_where_it_is():
    par = pr.Params()
    robot, geom, rec, Jb = _stand(par)
    m = float(robot[0, 0])
    f = np.array([0.0, 0.0, m * par.gravity / 4])
    tau = np.einsum("blcr,c->blr", Jb, -f).reshape(1, 12)            # J^T (-f), float64
    start = rec.copy()
    for _ in range(1000):
        out = pr.plant_step(rec, tau, robot, geom, par)
    moved = np.abs(rec[:, :pr.FLAGS] - start[:, :pr.FLAGS]).max()
    print(f"\nstand, 1000 ticks: the record moved by {moved:.2e}")
    assert moved <= 1e-12 and rec[0, pr.TICK] == 1000 and rec[0, pr.FLAGS] == 0
    assert np.abs(out["accel"][0] - np.float32([0, 0, par.gravity])).max() <= 1e-6 and (out["touch"] == 1).all()
    assert np.abs(out["gyro"]).max() <= 1e-12


def test_a_reaction_outside_the_cone_moves_the_body_by_the_clamped_force():
    par = pr.Params()
    robot, geom, rec, Jb = _stand(par)
    m, mu = float(robot[0, 0]), float(robot[0, 7])
    fz = m * par.gravity / 4
    f = np.array([2.0 * mu * fz, 0.0, fz])                           # twice the cone's tangential limit
    tau = np.einsum("blcr,c->blr", Jb, -f).reshape(1, 12)
    pr.plant_step(rec, tau, robot, geom, par)
    want = par.dt_control * np.array([4 * mu * fz / m, 0.0, 0.0])    # the clamped force, gravity held
    assert np.abs(rec[0, pr.VEL:pr.VEL + 3] - want).max() <= 1e-12 * np.abs(want).max() + 1e-15
    assert rec[:, pr.CONTACT:pr.CONTACT + 4].all()                   # pinned: no sliding
    inside = np.array([0.5 * mu * fz, 0.0, fz])
    robot, geom, rec, Jb = _stand(par)
    pr.plant_step(rec, np.einsum("blcr,c->blr", Jb, -inside).reshape(1, 12), robot, geom, par)
    assert abs(rec[0, pr.VEL] - par.dt_control * 4 * 0.5 * mu * fz / m) <= 1e-15


def test_a_stance_leg_that_pulls_is_released_in_that_substep():
    par = pr.Params()
    robot, geom, rec, Jb = _stand(par)
    fz = float(robot[0, 0]) * par.gravity / 4
    f = np.tile([0.0, 0.0, fz], (4, 1))
    f[1] = (0.0, 0.0, -3.0)                                          # FR pulls on the ground
    tau = np.einsum("blcr,lc->blr", Jb, -f).reshape(1, 12)
    z0 = rec[0, pr.FEET + 5]
    out = pr.plant_step(rec, tau, robot, geom, par)
    assert rec[0, pr.CONTACT:pr.CONTACT + 4].tolist() == [1, 0, 1, 1] and out["touch"][0].tolist() == [1, 0, 1, 1]
    # from rest under g = -f = +3 N and gravity: v = h (3 / foot_mass - gravity), z += h v
    v = par.dt_control * (3.0 / par.foot_mass - par.gravity)
    assert abs(rec[0, pr.FVEL + 5] - v) <= 1e-12 and abs(rec[0, pr.FEET + 5] - (z0 + par.dt_control * v)) <= 1e-15
    # the body lost that leg's support and got the foot's reaction: 3 legs up, 3 N down
    az = (3 * fz - 3.0) / float(robot[0, 0]) - par.gravity
    assert abs(rec[0, pr.VEL + 2] - par.dt_control * az) <= 1e-13


def test_a_bad_robot_is_refused_alone(header):
    par = pr.Params()
    st = pr.make_states(9, seed=4, par=par)
    tau, robot, rec = st["tau"].copy(), st["robot"].copy(), st["rec"].copy()
    tau[1, 5] = np.nan
    robot[2, 0] = 0.0                                  # mass
    robot[3, 1:7] = 0.0                                # inertia
    rec[4, pr.QUAT:pr.QUAT + 4] = 0.0
    rec[5, pr.FEET + 2] = np.inf
    robot[6, 7] = np.nan                               # mu
    rec[7, pr.CONTACT + 2] = np.nan                    # a contact word
    clean = st["rec"].copy()
    pr.plant_step(clean, st["tau"], st["robot"], st["geom"], par)
    for step in (pr.plant_step, lambda *a: run_header(header, *a)):
        r = rec.copy()
        out = step(r, tau, robot, st["geom"], par)
        assert out["status"].tolist() == [0, 4, 4, 4, 4, 4, 4, 4, 0]
        assert np.array_equal(r[1:8], rec[1:8], equal_nan=True)                 # untouched
        assert np.abs(r[[0, 8]] - clean[[0, 8]]).max() <= 1e-14                # the others as without them
        assert np.array_equal(out["root"][1, :3], rec[1, :3].astype(np.float32))  # rewritten from the record


# ---- the closed loop on the CPU oracles

@pytest.fixture(scope="module")
def loop():
    return pr.closed_loop(pr.COMMANDS, 1000)


def test_the_closed_loop_walks(loop):
    """Aliengo, TROTTING10, N = 10, 1000 ticks at 0, 0.5 and 1.0 m/s forward: on every tick
    finite, every solve converged, the base within 0.05 m of 0.38, |roll| and |pitch| below 0.1.
    Recorded (plant_ref.CLOSED_LOOP): worst height error 0.01086 / 0.01094 / 0.01109 m, worst
    roll / pitch 3.3e-8 / 0.0336 / 0.0854 rad, mean speed over the last 500 ticks 0.0000 /
    0.5210 / 1.0442 m/s."""
    height, tilt, speed = pr.summary(loop)
    print(f"\nclosed loop at {pr.COMMANDS}: height error {height}, roll / pitch {tilt}, speed {speed}")
    assert loop["finite"].all() and loop["solve_ok"].all()
    assert (np.abs(loop["height"] - 0.38) < 0.05).all()
    assert (np.abs(loop["roll"]) < 0.1).all() and (np.abs(loop["pitch"]) < 0.1).all()
    # the recorded yardstick of the GPU test is what this run gives
    assert np.abs(height - pr.CLOSED_LOOP["height"]).max() < 5e-5
    assert np.abs(tilt - pr.CLOSED_LOOP["tilt"]).max() < 5e-4
    assert np.abs(speed - pr.CLOSED_LOOP["speed"]).max() < 5e-4
    assert abs(loop["x"][-1, 0]) < 1e-6                # commanded 0: it steps in place


def test_the_closed_loop_trots(loop):
    """The gait is there: diagonal pairs alternate, and between them all four feet are in the
    air for a few ticks per half period (the reference's gait table starts one segment ahead, so
    the stance legs get no force over the last segment before a switch)."""
    touch = loop["touch"]
    flight = (touch.sum(-1) == 0).sum(0)
    print(f"\nticks with no foot on the ground: {flight} of {len(touch)}")
    assert (flight > 0).all() and (flight < 50).all()
    pair_a, pair_b = touch[:, :, [0, 3]].all(-1), touch[:, :, [1, 2]].all(-1)
    assert (pair_a.sum(0) > 300).all() and (pair_b.sum(0) > 300).all() and (pair_a & pair_b).mean() < 0.1

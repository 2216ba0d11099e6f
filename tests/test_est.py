"""CPU: the base-state estimator (mpcqp_estimate) without a GPU -- its ABI surface and the
float64 restatement tests/est_ref.py, which is the oracle of tests/test_gpu_est.py: the
reference raises NotImplementedError where the filter would sit, so est_ref is checked
against known answers and against its own second form.

Measured here (printed by the tests):
  known answer (a), level crouch, 2000 ticks: |p_b,z - 2 l cos 0.8| 4.0e-09 (the float32
    rounding of 0.8), |p_b,xy| 7e-17, |v_b| 2.1e-08 (accel z = float32(9.81) - 9.81 = 4.2e-07
    m/s^2 against the velocity rows), |foot z| 6.5e-11;
  known answer (b), tilted, one foot trusted, 3000 ticks: |p_b,z + r_z| 7.9e-10, |foot z|
    2.6e-10, |v_b| 2.6e-08, |p_j - p_b - R_q p_j| 5.3e-10 (the float32-rounded accel);
  both inside the 1e-5 m the checks assert.
  batch against sequential form, B = 8, 400 ticks: d = 1.94e-11 for x and 4.8e-15 for P,
    norm-wise per robot, largest over ticks and robots (est_ref.D_X, est_ref.D_P; the first
    ticks, where P0 / r_p = 1e5 conditions S, give the x figure).  It is the problem's
    rounding sensitivity and sets the device bounds of tests/test_gpu_est.py.
  smallest eigenvalue of P over that run: 1.5e-05.

The kernel spreads a robot over 18 lanes with P's columns in registers, so there is no
lane-independent per-robot header to compile for the host as test_kin.py does.  Instead
csrc/mpcqp_estimator.h itself is compiled with g++ and a workgroup is run as 64 host threads
meeting at a std::barrier where the kernel has its barriers (KERNEL_SHIM): the kernel's own
text, lane indexing and LDS traffic included, against est_ref over the generator's
trajectory.  Measured: x 2.1e-12, P 1.8e-15 against the batch form (inside d), float32
outputs 5.5e-08."""
import ctypes
import os
import re

import numpy as np
import pytest

import est_ref
import kin_ref
from helpers import _declared, host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpcqp.h")
NEW_SYMBOLS = {"mpcqp_estimate", "mpcqp_set_estimator"}
KNOWN = 1e-5      # metres (and m/s): the known answers' bound

KERNEL_SHIM = r'''
#include <barrier>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <thread>
#include <vector>
#define __host__
#define __device__
#define __global__
#define __shared__ static
#define __launch_bounds__(x)
#define MPCQP_STATUS_OK 0
#define MPCQP_STATUS_NONFINITE 4
struct Idx { int x; };
thread_local Idx threadIdx, blockIdx;
static std::barrier<>* g_bar;
static inline void __syncthreads() { g_bar->arrive_and_wait(); }
using std::isfinite;
#include "mpcqp_estimator.h"
// the launch of mpcqp_estimate: workgroup after workgroup, a host thread per lane
extern "C" void launch(const double* c, int dof, int B, const float* quat, const float* gyro, const float* accel,
                       const float* q, const float* qdot, const float* trust, const double* geom, double* st,
                       float* root, float* feet, int32_t* status) {
  EstParams ep{dof, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], c[10]};
  for (int blk = 0; blk < (B + kEstRobots - 1) / kEstRobots; ++blk) {
    std::barrier<> bar(kEstThreads);
    g_bar = &bar;
    std::vector<std::thread> lanes;
    for (int t = 0; t < kEstThreads; ++t)
      lanes.emplace_back([=] {
        threadIdx.x = t, blockIdx.x = blk;
        mpcqp_estimate_kernel(ep, B, quat, gyro, accel, q, qdot, trust, geom, st, root, feet, status);
      });
    for (auto& l : lanes) l.join();
  }
}
extern "C" int robots_per_workgroup(void) { return kEstRobots; }
extern "C" int stride(void) { return EST_STRIDE; }
'''


def test_header_declares_the_estimator_entry_points_and_binding_agrees():
    from mpcqp import _lib
    assert NEW_SYMBOLS <= _declared()
    assert _declared() == set(_lib.EXPORTED_SYMBOLS)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.mpcqp_abi_version() == 6     # additive: the ABI version stays


def test_record_constants_match_binding():
    from mpcqp import _lib, params
    src = open(HEADER).read()
    assert int(re.search(r"#define MPCQP_EST_STRIDE (\d+)", src).group(1)) == _lib.EST_STRIDE == est_ref.STRIDE == 352
    assert int(re.search(r"#define MPCQP_EST_DOF_STATES (\d+)", src).group(1)) == _lib.EST_DOF_STATES \
        == est_ref.DOF_STATES == 1
    assert est_ref.GEOMETRY == {k: params.LEG_GEOMETRY[k] for k in est_ref.GEOMETRY}
    assert est_ref.STATUS_NONFINITE == _lib.STATUS_NONFINITE


def test_null_ctx_is_an_error_code():
    from mpcqp import _lib
    lib = _lib.load()
    assert lib.mpcqp_estimate(None, 1, 0, *([None] * 12)) == -1
    assert lib.mpcqp_set_estimator(None, *([1.0] * 11)) == -1


def test_pack_unpack_round_trip():
    rng = np.random.default_rng(0)
    x, P = rng.standard_normal((3, 18)), rng.standard_normal((3, 18, 18))
    rec = est_ref.pack(x, P)
    assert rec.shape == (3, 352) and (rec[:, 19:24] == 0).all() and (rec[:, 348:] == 0).all()
    assert (rec[:, 18] == 1).all() and rec[1, 24 + 18 * 2 + 5] == P[1, 2, 5]
    x2, P2, init = est_ref.unpack(rec)
    assert np.array_equal(x2, x) and np.array_equal(P2, P) and (init == 1).all()


@pytest.mark.parametrize("form", ["batch", "sequential"])
def test_known_answer_level_crouch(form):
    """(a): level, crouch, all feet trusted, accel (0, 0, g), from an all-zero record."""
    inp = est_ref.level_crouch(1, "aliengo")
    st = np.zeros((1, est_ref.STRIDE))
    for _ in range(2000):
        st, out = est_ref.estimate_step(st, inp, None, form)
    x = est_ref.unpack(st)[0][0]
    errs = dict(z=abs(x[2] - 2 * 0.25 * np.cos(0.8)), xy=np.abs(x[0:2]).max(), v=np.abs(x[3:6]).max(),
                foot_z=np.abs(x[8::3]).max())
    print(f"\nlevel crouch ({form}): " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < KNOWN
    assert np.abs(out["root_states"][0, 0:3] - x[0:3]).max() == 0 and (out["status"] == 0).all()


@pytest.mark.parametrize("form", ["batch", "sequential"])
def test_known_answer_tilted_one_foot(form):
    """(b): a tilted base at rest, perturbed joints, accel = R_q^T (0, 0, g), foot RL alone
    trusted: the base sits at -(R_q p_i)_z above that foot's z = 0, and every foot, trusted
    or not, at p_b + R_q p_j."""
    foot = 2
    inp = est_ref.tilted_one_foot(1, foot=foot, robot="a1")
    st = np.zeros((1, est_ref.STRIDE))
    for _ in range(3000):
        st, _ = est_ref.estimate_step(st, inp, None, form)
    x = est_ref.unpack(st)[0][0]
    r = np.einsum("rc,lc->lr", kin_ref.quat2matrix_eigen(inp["quat"])[0], kin_ref.chain(inp["geom"], inp["q"])[0][0])
    errs = dict(z=abs(x[2] + r[foot, 2]), foot_z=abs(x[8 + 3 * foot]), v=np.abs(x[3:6]).max(),
                feet=np.abs(x[6:].reshape(4, 3) - x[0:3] - r).max())
    print(f"\ntilted, one foot ({form}): " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < KNOWN


@pytest.fixture(scope="module")
def both_forms():
    traj = est_ref.make_trajectory(8, 400, seed=7)
    return traj, est_ref.run(traj, form="batch")[0], est_ref.run(traj, form="sequential")[0]


def test_batch_and_sequential_forms_agree(both_forms):
    """R is diagonal: the 28 scalar updates in sequence are the batch update.  Measured
    d = 1.94e-11 (x) and 4.8e-15 (P); est_ref.D_X and D_P record it for the device bounds.
    The assertion is the order of magnitude rounding explains: S is conditioned like
    P0 / r_p = 1e5 on the first ticks, times 1e-16, times the 28-row solve."""
    _, sb, ss = both_forms
    dx = dP = 0.0
    for i in range(1, len(sb)):
        xb, Pb, _ = est_ref.unpack(sb[i])
        xs, Ps, _ = est_ref.unpack(ss[i])
        for b in range(xb.shape[0]):
            dx, dP = max(dx, est_ref.norm_err(xs[b], xb[b])), max(dP, est_ref.norm_err(Ps[b], Pb[b]))
    print(f"\nbatch vs sequential over 8 robots x 400 ticks: d_x {dx:.3e}, d_P {dP:.3e}")
    assert dx < 1e-9 and dP < 1e-13
    assert dx <= 4 * est_ref.D_X and dP <= 4 * est_ref.D_P      # the recorded figures still describe it


def test_covariance_stays_symmetric_positive_definite(both_forms):
    _, sb, ss = both_forms
    low = np.inf
    for states in (sb, ss):
        for i in range(1, len(states)):
            P = est_ref.unpack(states[i])[1]
            assert np.array_equal(P, np.swapaxes(P, 1, 2))
            low = min(low, float(np.linalg.eigvalsh(P).min()))
    print(f"\nsmallest eigenvalue of P over both runs: {low:.3e}")
    assert low > 0.0


def test_trajectory_covers_the_trust_patterns(both_forms):
    traj = both_forms[0]
    tr = np.stack([t["trust"] for t in traj])
    assert (tr < 0).any() and (tr > 1).any() and ((tr > 0) & (tr < 1)).any()
    assert (tr == 0).all(-1).any() and (tr == 1).all(-1).any()
    assert all(t[k].dtype == np.float32 for t in traj[:2] for k in est_ref.INPUTS[:-1])
    assert len({tuple(g) for g in traj[0]["geom"]}) == 2


def test_trust_is_clipped():
    traj = est_ref.make_trajectory(4, 3, seed=1)
    a = dict(traj[0], trust=np.float32([[-0.5, 1.5, 0.25, 2.0]] * 4))
    b = dict(traj[0], trust=np.float32([[0.0, 1.0, 0.25, 1.0]] * 4))
    for form in ("batch", "sequential"):
        sa, sb_ = (est_ref.estimate_step(np.zeros((4, 352)), i, None, form)[0] for i in (a, b))
        assert np.array_equal(sa, sb_)


def test_zero_record_is_the_seeded_start():
    traj = est_ref.make_trajectory(4, 1, seed=2)
    seeded = est_ref.pack(np.zeros((4, 18)), np.tile(100.0 * np.eye(18), (4, 1, 1)))
    for form in ("batch", "sequential"):
        s0, o0 = est_ref.estimate_step(np.zeros((4, 352)), traj[0], None, form)
        s1, o1 = est_ref.estimate_step(seeded, traj[0], None, form)
        assert np.array_equal(s0, s1) and all(np.array_equal(o0[k], o1[k]) for k in o0)
    other = est_ref.estimate_step(np.zeros((4, 352)), traj[0], dict(p0=10.0))[0]
    assert not np.array_equal(other, s0)


def test_nan_leaves_that_robot_alone():
    traj = est_ref.make_trajectory(4, 6, seed=3)
    start = est_ref.run(traj[:5])[0][-1]
    for key in est_ref.INPUTS[:-1]:
        inp = {k: v.copy() for k, v in traj[5].items()}
        inp[key][1, 0] = np.nan
        for form in ("batch", "sequential"):
            clean, oc = est_ref.estimate_step(start, traj[5], None, form)
            new, out = est_ref.estimate_step(start, inp, None, form)
            assert np.array_equal(new[1], start[1]) and out["status"].tolist() == [0, 4, 0, 0], key
            keep = [0, 2, 3]
            assert np.array_equal(new[keep], clean[keep])
            assert all(np.array_equal(out[k][keep], oc[k][keep]) for k in oc)
            assert np.array_equal(out["root_states"][1, 0:3], start[1, 0:3])      # formed from the state as it was
            assert np.array_equal(out["feet_world"][1].ravel(), start[1, 6:18])


@pytest.fixture(scope="module")
def kernel():
    return host_build(KERNEL_SHIM, ("-std=c++20", "-O2", "-ffp-contract=off", "-pthread"), "est")


def host_launch(kernel, state, inp, layout="split", constants=None, pad=2):
    """The kernel on host threads, on `state` [B + pad, STRIDE] in place; the outputs come
    back with their `pad` sentinel rows."""
    B = state.shape[0] - pad
    c = dict(est_ref.DEFAULTS, **(constants or {}))
    cv = np.array([c[k] for k in ("dt", "gravity", "sigma_p", "sigma_v", "sigma_f", "r_p", "r_v", "r_z", "suspicion",
                                  "p0", "contact_height")])
    out = dict(root_states=np.full((B + pad, 13), -77, np.float32), feet_world=np.full((B + pad, 4, 3), -77, np.float32),
               status=np.full(B + pad, -77, np.int32))
    if layout == "dof":
        q, qd = kin_ref.dof_states(inp["q"], inp["qdot"]), None
    else:
        q, qd = np.ascontiguousarray(inp["q"]), np.ascontiguousarray(inp["qdot"])
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    keep = [np.ascontiguousarray(inp[k]) for k in ("quat", "gyro", "accel")] + [q, qd] + \
        [np.ascontiguousarray(inp[k]) for k in ("trust", "geom")]
    kernel.launch(ptr(cv), int(layout == "dof"), B, *(ptr(a) for a in keep), ptr(state), *(ptr(out[k]) for k in out))
    return out


@pytest.mark.parametrize("layout", ["split", "dof"])
def test_host_run_of_the_kernel_follows_the_restatement(kernel, layout):
    """B = 7 is three workgroups, the last with one robot; 40 ticks.  The record within d of
    the batch form (the kernel is the sequential form), the float32 outputs within the
    two-ulp floor, the padding rows untouched, P bitwise symmetric."""
    assert kernel.stride() == est_ref.STRIDE
    B, T = 2 * kernel.robots_per_workgroup() + 1, 40
    traj = est_ref.make_trajectory(B, T, seed=7)
    states, outs = est_ref.run(traj)
    st = np.full((B + 2, est_ref.STRIDE), -77.0)
    st[:B] = 0.0
    worst = dict(x=0.0, P=0.0, root_states=0.0, feet_world=0.0)
    for i in range(T):
        o = host_launch(kernel, st, traj[i], layout)
        x, P, init = est_ref.unpack(st[:B])
        xr, Pr, _ = est_ref.unpack(states[i + 1])
        assert (init == 1).all() and np.array_equal(P, np.swapaxes(P, 1, 2)) and (o["status"][:B] == 0).all()
        assert (st[B:] == -77).all() and all((v[B:] == -77).all() for v in o.values())
        for b in range(B):
            worst["x"], worst["P"] = max(worst["x"], est_ref.norm_err(x[b], xr[b])), max(worst["P"], est_ref.norm_err(P[b], Pr[b]))
            for k in ("root_states", "feet_world"):
                worst[k] = max(worst[k], est_ref.norm_err(o[k][b], outs[i][k][b]))
    print(f"\nkernel on host threads ({layout}): " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["x"] <= est_ref.D_X and worst["P"] <= est_ref.D_P
    assert worst["root_states"] <= 2.4e-7 and worst["feet_world"] <= 2.4e-7


def test_host_run_of_the_kernel_nan_and_constants(kernel):
    traj = est_ref.make_trajectory(4, 6, seed=3)
    start = est_ref.run(traj[:5])[0][-1]
    inp = {k: v.copy() for k, v in traj[5].items()}
    inp["gyro"][1, 1] = np.inf
    clean, dirty = np.vstack([start, np.zeros((2, 352))]), np.vstack([start, np.zeros((2, 352))])
    oc, od = host_launch(kernel, clean, traj[5]), host_launch(kernel, dirty, inp)
    assert od["status"][:4].tolist() == [0, 4, 0, 0] and np.array_equal(dirty[1], start[1])
    keep = [0, 2, 3]
    assert np.array_equal(dirty[keep], clean[keep]) and all(np.array_equal(od[k][keep], oc[k][keep]) for k in oc)
    assert np.array_equal(od["root_states"][1, 0:3], start[1, 0:3].astype(np.float32))
    mine = dict(r_p=0.002, suspicion=50.0, sigma_f=0.004, contact_height=0.01, dt=0.002, p0=10.0)
    st = np.zeros((6, 352))
    host_launch(kernel, st, traj[0], constants=mine)
    ref = est_ref.estimate_step(np.zeros((4, 352)), traj[0], mine)[0]
    for b in range(4):
        assert est_ref.norm_err(st[b, :18], ref[b, :18]) <= est_ref.D_X
        assert est_ref.norm_err(st[b, 24:348], ref[b, 24:348]) <= est_ref.D_P


# ---- the CPU twins of tests/test_gpu_est_edges.py: est_ref's edge inputs through the
# kernel on host threads, so that every assertion made on the device is shown to hold for
# correct code without one.  B = 7: slots 0, 1, 2, a second workgroup, a tail of one.
EB = 7
X_BOUND, P_BOUND, F32_BOUND = 10 * est_ref.D_X, 10 * est_ref.D_P, 2.4e-7


def host_tick(kernel, start, inp, layout="split", constants=None):
    """One host launch from the records `start` [B]: (records, outputs), each with two sentinel rows."""
    st = np.vstack([start, np.full((2, est_ref.STRIDE), -77.0)])
    out = host_launch(kernel, st, inp, layout, constants)
    assert (st[-2:] == -77).all() and all((v[-2:] == -77).all() for v in out.values())
    return st, out


@pytest.fixture(scope="module")
def edge_start():
    """The generator's trajectory for EB robots (Aliengo / A1 alternating), the records after
    5 ticks and the inputs of the sixth."""
    traj = est_ref.make_trajectory(EB, 12, seed=7)
    return traj, est_ref.run(traj[:5])[0][-1]


def test_edge_case_tables():
    cases = est_ref.nonfinite_cases()
    assert len(cases) == 43 and len(est_ref.dof_cases()) == 8
    assert {(k, e) for k, e, _, _ in cases} == {(k, e) for k in est_ref.INPUTS for e in range(est_ref.WIDTH[k])}
    assert {r for *_, r in cases} == {1, 5, 6} and {repr(v) for _, _, v, _ in cases} == {"nan", "inf", "-inf"}
    assert {(k, e // 3) for k, e, _, _ in est_ref.dof_cases()} == {(k, leg) for k in ("q", "qdot") for leg in range(4)}
    assert {r for _, _, r in est_ref.record_cases()} == {2, 6} and len(est_ref.record_cases()) == 10


def test_host_kernel_refuses_a_value_one_lane_sees(kernel, edge_start):
    """2a.  Every (input, element) in turn; the joints, the trust and so the verdict of legs
    1..3 reach one leg lane only, so a kernel that read sh.bad[0] alone would fail 24 cases."""
    traj, start = edge_start
    clean = host_tick(kernel, start, traj[5])
    for key, e, v, robot in est_ref.nonfinite_cases():
        inp = est_ref.poisoned(traj[5], key, e, v, robot)
        est_ref.assert_refused(start, inp["quat"], clean, host_tick(kernel, start, inp), robot, tag=(key, e, v, robot))
    clean = host_tick(kernel, start, traj[5], "dof")
    for key, e, v, robot in est_ref.dof_cases():
        inp = est_ref.poisoned(traj[5], key, e, v, robot)
        est_ref.assert_refused(start, inp["quat"], clean, host_tick(kernel, start, inp, "dof"), robot, tag=(key, e, v))
    for word in (5, 6, 7):                                   # nobody reads the geometry record's tail
        inp = est_ref.poisoned(traj[5], "geom", word, np.nan, 1)
        sd, od = host_tick(kernel, start, inp, "dof")
        assert est_ref.same_bits(sd, clean[0]) and all(est_ref.same_bits(od[k], clean[1][k]) for k in od)


def test_host_kernel_refusal_on_a_fresh_record(kernel, edge_start):
    """2b."""
    traj, _ = edge_start
    zero = np.zeros((EB, est_ref.STRIDE))
    clean = host_tick(kernel, zero, traj[0])
    inp = est_ref.poisoned(traj[0], "q", 7, np.nan, 4)
    sd, od = host_tick(kernel, zero, inp)
    est_ref.assert_refused(zero, inp["quat"], clean, (sd, od), 4)
    assert (sd[4] == 0).all() and (od["root_states"][4, [0, 1, 2, 7, 8, 9]] == 0).all() and (od["feet_world"][4] == 0).all()
    s2, o2 = host_tick(kernel, sd[:EB], traj[0])
    assert est_ref.same_bits(s2[4], clean[0][4]) and all(est_ref.same_bits(o2[k][4], clean[1][k][4]) for k in o2)


def test_host_kernel_trust_values(kernel, edge_start):
    """2c.  The clip is on the float32: -0.0, one ulp over 1 and +-3e38 are 0, 1, 1, 0 to the
    bit.  A subnormal, one ulp under 1 and two fractions follow est_ref; a kernel that read
    leg 0's trust for every leg would be out by more than 100 bounds."""
    traj, start = edge_start
    tile = lambda t: np.tile(t, (EB, 1))
    a = host_tick(kernel, start, dict(traj[5], trust=tile(est_ref.TRUST_OUTSIDE)))
    b = host_tick(kernel, start, dict(traj[5], trust=tile(est_ref.TRUST_CLIPPED)))
    assert est_ref.same_bits(a[0], b[0]) and all(est_ref.same_bits(a[1][k], b[1][k]) for k in a[1])
    inp = dict(traj[5], trust=tile(est_ref.TRUST_INSIDE))
    st, out = host_tick(kernel, start, inp)
    ref, _ = est_ref.estimate_step(start, inp)
    wrong, _ = est_ref.estimate_step(start, dict(inp, trust=tile(est_ref.TRUST_INSIDE[[0, 0, 0, 0]])))
    dx, dP = est_ref.worst_err([None, st[:EB]], [None, ref])
    print(f"\ntrust inside (0, 1) on host threads: x {dx:.2e}, P {dP:.2e}")
    assert dx <= X_BOUND and dP <= P_BOUND and (out["status"][:EB] == 0).all()
    assert min(est_ref.worst_err([None, wrong[b:b + 1]], [None, ref[b:b + 1]])[0] for b in range(EB)) >= 100 * X_BOUND


def test_host_kernel_refuses_a_nonfinite_record(kernel, edge_start):
    """2d.  A non-finite x_j, P entry (on and off the diagonal) or `initialised` word of an
    initialised record: that robot is refused and the others do not notice.  The same words
    in a record whose `initialised` word is 0 are not read."""
    traj, start = edge_start
    clean = host_tick(kernel, start, traj[5])
    for word, v, robot in est_ref.record_cases():
        seeded = start.copy()
        seeded[robot, word] = v
        dirty = host_tick(kernel, seeded, traj[5])
        # the clean launch's other robots; the dirty robot is compared with its own seed
        ref = (np.vstack([clean[0][:robot], seeded[robot:robot + 1], clean[0][robot + 1:]]), clean[1])
        est_ref.assert_refused(seeded, traj[5]["quat"], ref, dirty, robot, tag=(word, v, robot))
        again = host_tick(kernel, dirty[0][:EB], traj[6])
        assert again[1]["status"][robot] == 4 and est_ref.same_bits(again[0][robot], seeded[robot])
    first = host_tick(kernel, np.zeros((EB, est_ref.STRIDE)), traj[5])
    fresh = np.zeros((EB, est_ref.STRIDE))
    fresh[2, [0, 4, 17]] = np.nan
    fresh[6, [est_ref.P_OFF, est_ref.P_OFF + 29]] = np.nan, np.inf
    sd, od = host_tick(kernel, fresh, traj[5])
    assert est_ref.same_bits(sd, first[0]) and all(est_ref.same_bits(od[k], first[1][k]) for k in od)
    assert (od["status"][:EB] == 0).all()


def test_restatement_refuses_a_nonfinite_record(edge_start):
    traj, start = edge_start
    clean, oc = est_ref.estimate_step(start, traj[5])
    for word, v, robot in est_ref.record_cases():
        seeded = start.copy()
        seeded[robot, word] = v
        for form in ("batch", "sequential"):
            new, out = est_ref.estimate_step(seeded, traj[5], None, form)
            assert out["status"][robot] == 4 and est_ref.same_bits(new[robot], seeded[robot]), (word, form)
            keep = [b for b in range(EB) if b != robot]
            assert (out["status"][keep] == 0).all()
            if form == "batch":
                assert est_ref.same_bits(new[keep], clean[keep])
    fresh = np.zeros((EB, est_ref.STRIDE))
    fresh[2, 4] = fresh[6, est_ref.P_OFF + 29] = np.nan
    new, out = est_ref.estimate_step(fresh, traj[5])
    assert est_ref.same_bits(new, est_ref.estimate_step(np.zeros((EB, est_ref.STRIDE)), traj[5])[0]) and (out["status"] == 0).all()


def test_host_kernel_other_words_of_the_record(kernel, edge_start):
    """2e.  Any non-zero `initialised` word is 1 and is rewritten to 1.0; the padding words
    keep their bits and change nothing."""
    traj, start = edge_start
    clean = host_tick(kernel, start, traj[5])
    seeded = start.copy()
    seeded[1, est_ref.INIT], seeded[3, est_ref.INIT] = 2.0, -3.0
    seeded[:, est_ref.PADDING[:5]], seeded[:, est_ref.PADDING[5:]] = 5.0, 6.0
    sd, od = host_tick(kernel, seeded, traj[5])
    pad = list(est_ref.PADDING)
    assert (sd[:EB, est_ref.INIT] == 1.0).all() and est_ref.same_bits(sd[:EB, pad], seeded[:, pad])
    sd[:EB, pad] = 0.0
    assert est_ref.same_bits(sd, clean[0]) and all(est_ref.same_bits(od[k], clean[1][k]) for k in od)


def test_host_kernel_quaternion_as_given(kernel, edge_start):
    """2f.  R_q is the documented polynomial in q, used as given: 2 q, q / 2 and 0 follow
    est_ref fed the same quaternion (a kernel that normalised q would be out by more than
    100 bounds for 2 q), 0 gives R = I, and -q gives q's record to the bit."""
    traj, start = edge_start
    runs = {}
    for name in ("given", "double", "half", "zero", "negated"):
        tr = [dict(t, quat=t["quat"] if name == "given" else est_ref.quat_variants(t["quat"])[name]) for t in traj[:10]]
        st = start
        states = [st]
        for inp in tr:
            full, out = host_tick(kernel, st, inp)
            st = full[:EB]
            states.append(st)
            assert (out["status"][:EB] == 0).all()
        runs[name] = (tr, states, out)
    for name in ("double", "half", "zero"):
        tr, states, out = runs[name]
        ref = est_ref.run(tr, state=start)[0]
        dx, dP = est_ref.worst_err(states, ref)
        print(f"\nquaternion {name} on host threads: x {dx:.2e}, P {dP:.2e}")
        assert dx <= X_BOUND and dP <= P_BOUND
    normalised = est_ref.run(runs["given"][0], state=start)[0]
    assert est_ref.worst_err(est_ref.run(runs["double"][0], state=start)[0], normalised)[0] >= 100 * X_BOUND
    assert np.array_equal(kin_ref.quat2matrix_eigen(np.zeros((1, 4)))[0], np.eye(3))
    assert est_ref.same_bits(runs["negated"][1][-1], runs["given"][1][-1])
    assert est_ref.same_bits(runs["negated"][2]["root_states"][:EB, 3:7], -runs["given"][2]["root_states"][:EB, 3:7])


@pytest.fixture(scope="module")
def regimes():
    """regime -> (trajectory, constants, batch-form records, d_x, d_P): the long regimes and
    est_ref's own two forms on them."""
    out = {}
    for name in est_ref.D_REGIME:
        traj, c = est_ref.regime_trajectory(EB, 200, name)
        sb = est_ref.run(traj, c, "batch")[0]
        out[name] = (traj, c, sb) + est_ref.worst_err(est_ref.run(traj, c, "sequential")[0], sb)
    return out


@pytest.mark.parametrize("name", list(est_ref.D_REGIME))
def test_long_regimes_have_their_own_d(regimes, name):
    """2g.  200 ticks of all-swing, all-stance and zero process noise: est_ref's two forms
    differ by more than D_X / D_P there, so each regime records its own d (est_ref.D_REGIME),
    measured here and printed."""
    *_, dx, dP = regimes[name]
    print(f"\nbatch vs sequential, {name}, {EB} robots x 200 ticks: d_x {dx:.3e}, d_P {dP:.3e}")
    rx, rP = est_ref.D_REGIME[name]
    assert dx <= rx <= 4 * dx and dP <= rP <= 4 * dP            # the recorded figures describe it


@pytest.mark.parametrize("name", list(est_ref.D_REGIME))
def test_host_kernel_long_regimes(kernel, regimes, name):
    """2g on host threads: within 10 d of the batch form, P bitwise symmetric and finite,
    status 0.  The regime matters: the generator's own trust and noise give records more
    than 100 bounds away."""
    traj, c, sb, *_ = regimes[name]
    bx, bP = (10 * d for d in est_ref.D_REGIME[name])
    st = np.zeros((EB, est_ref.STRIDE))
    states, f32 = [st], 0.0
    ref_out = est_ref.run(traj[:200], c)[1]
    for i, inp in enumerate(traj):
        full, out = host_tick(kernel, st, inp, constants=c)
        st = full[:EB]
        states.append(st)
        P = est_ref.unpack(st)[1]
        assert np.array_equal(P, np.swapaxes(P, 1, 2)) and np.isfinite(st).all() and (out["status"][:EB] == 0).all()
        f32 = max([f32] + [est_ref.norm_err(out[k][b], ref_out[i][k][b]) for k in ("root_states", "feet_world") for b in range(EB)])
    dx, dP = est_ref.worst_err(states, sb)
    print(f"\n{name} on host threads: x {dx:.2e}, P {dP:.2e}, float32 outputs {f32:.2e}")
    assert dx <= bx and dP <= bP and f32 <= max(F32_BOUND, bx)
    plain = est_ref.run(est_ref.make_trajectory(EB, 200, seed=est_ref.REGIME_SEED))[0]
    assert min(est_ref.worst_err(plain[:, b:b + 1], sb[:, b:b + 1])[1] for b in range(EB)) >= 100 * bP


@pytest.mark.parametrize("B", [2, 5, 6])
def test_host_kernel_batch_shapes(kernel, edge_start, B):
    """2h.  An idle robot slot inside a workgroup (2, 5) and exactly full workgroups (6).  A
    kernel that gave robot b the inputs of robot b - 1 would be out by more than 100 bounds."""
    traj = [{k: v[:B] for k, v in t.items()} for t in edge_start[0][:10]]
    ref = est_ref.run(traj)[0]
    st = np.zeros((B, est_ref.STRIDE))
    states = [st]
    for inp in traj:
        full, out = host_tick(kernel, st, inp)
        st = full[:B]
        states.append(st)
        assert (out["status"][:B] == 0).all()
    dx, dP = est_ref.worst_err(states, ref)
    print(f"\nB = {B} on host threads: x {dx:.2e}, P {dP:.2e}")
    assert dx <= X_BOUND and dP <= P_BOUND
    assert est_ref.worst_err(ref[:, :B - 1], ref[:, 1:B])[0] >= 100 * X_BOUND

"""CPU: the leg kinematics (mpcqp_kinematics) without a GPU -- its ABI surface, the float64
restatement tests/kin_ref.py and the host-compiled per-leg header csrc/mpcqp_kin_leg.h,
both against the reference's own product-of-exponentials chain (tests/golden/kin.npz),
known answers, the Jacobian against central differences, and the URDF reader.

Measured here against kin.npz (norm-wise per robot, max over robots; printed by the two
fixture tests): positions 9e-16, jac 3.9e-10 and foot_vel_base 2.7e-10 for both -- the
fixture's Jacobians are central differences with h = 1e-6, whose truncation and rounding
error is what remains.  See CPU_BOUND below and the docstring of tests/test_gpu_kin.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import _declared, host_build
import kin_edge_checks
import kin_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpcqp.h")

# Against kin.npz the restatements carry only float64 rounding (1e-15) and, in jac and
# foot_vel_base, the error of the fixture's central differences: h^2 / 6 times a third
# derivative of order the leg length (1e-13) plus rounding 1e-16 / h = 1e-10, norm-wise a
# few 1e-10.  Anything above this bound wants an explanation, not a wider bound.
CPU_BOUND = 2e-9

SHIM = r'''
#include "mpcqp_kin_leg.h"
// one robot, as mpcqp_kinematics_kernel strings the header together: quat (w, x, y, z) and
// the base state float32, Rb the float32 R_base, geom [KIN_STRIDE]; outputs [4][3] / [4][9]
extern "C" void robot(const double* geom, const float* quat, const float* Rb32, const float* pos, const float* vel,
                      const float* omega, const float* q, const float* qdot, double* feet, double* thighs,
                      double* pos_feet, double* foot_pos_base, double* foot_vel_base, double* jac) {
  double Rq[9], Rb[9], p3[3], v3[3], w3[3];
  kin_quat2matrix((double)quat[0], (double)quat[1], (double)quat[2], (double)quat[3], Rq);
  for (int k = 0; k < 9; ++k) Rb[k] = (double)Rb32[k];
  for (int k = 0; k < 3; ++k) p3[k] = pos[k], v3[k] = vel[k], w3[k] = omega[k];
  for (int leg = 0; leg < 4; ++leg) {
    double ql[3], qd[3];
    for (int k = 0; k < 3; ++k) ql[k] = q[3 * leg + k], qd[k] = qdot[3 * leg + k];
    kin_leg(geom, leg, ql, qd, Rq, Rb, p3, v3, w3, feet + 3 * leg, thighs + 3 * leg, pos_feet + 3 * leg,
            foot_pos_base + 3 * leg, foot_vel_base + 3 * leg, jac + 9 * leg);
  }
}
extern "C" int stride(void) { return KIN_STRIDE; }
'''

NEW_SYMBOLS = {"mpcqp_kinematics", "mpcqp_kinematics_root_states"}


def test_header_declares_the_kinematics_entry_points_and_binding_agrees():
    from mpcqp import _lib
    assert NEW_SYMBOLS <= _declared()
    assert _declared() == set(_lib.EXPORTED_SYMBOLS)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.mpcqp_abi_version() == 6     # additive: the ABI version stays


def test_kin_stride_matches_binding(leg):
    from mpcqp import _lib, params
    src = open(HEADER).read()
    assert int(re.search(r"#define MPCQP_KIN_STRIDE (\d+)", src).group(1)) == _lib.KIN_STRIDE == 8
    assert kin_ref.STRIDE == params.KIN_STRIDE == _lib.KIN_STRIDE == leg.stride()


def test_null_ctx_is_an_error_code():
    from mpcqp import _lib
    lib = _lib.load()
    assert lib.mpcqp_kinematics(None, 1, 0, *([None] * 15)) == -1
    assert lib.mpcqp_kinematics_root_states(None, 1, 0, *([None] * 10)) == -1


@pytest.fixture(scope="module")
def fx():
    return kin_ref.load_fixture()


@pytest.fixture(scope="module")
def leg():
    lib = host_build(SHIM, name="kin")
    dp, fp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)
    lib.robot.argtypes = [dp] + [fp] * 7 + [dp] * 6
    lib.robot.restype = None
    lib.dp, lib.fp = dp, fp
    return lib


def run_header(leg, geom, quat, pos, vel, omega, q, qdot, rot=None):
    """csrc/mpcqp_kin_leg.h over a batch, robot by robot: the dict kin_ref.kinematics returns."""
    B = len(quat)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    g = np.zeros((B, kin_ref.STRIDE))
    g[:, :5] = np.asarray(geom)[:, :5]
    Rb = f(kin_ref.quat2matrix_f32(quat) if rot is None else rot).reshape(B, 9)
    quat, pos, vel, omega, q, qdot = (f(a) for a in (quat, pos, vel, omega, q, qdot))
    out = {k: np.zeros((B, 4, 3, 3) if k == "jac" else (B, 4, 3)) for k in kin_ref.OUTPUTS}
    for b in range(B):
        leg.robot(g[b].ctypes.data_as(leg.dp), *(a[b].ctypes.data_as(leg.fp) for a in (quat, Rb, pos, vel, omega, q,
                                                                                      qdot)),
                  *(out[k][b].ctypes.data_as(leg.dp) for k in kin_ref.OUTPUTS))
    return out


def _report(tag, errs):
    worst = max(float(v.max()) for v in errs.values())
    print(f"\n{tag}: " + ", ".join(f"{k} {float(v.max()):.2e}" for k, v in errs.items()) + f" -> worst {worst:.3e}")
    return worst


def _inputs(fx, prefix=""):
    return tuple(fx[prefix + k] for k in ("quat", "pos", "vel", "omega", "q", "qdot"))


def test_restatement_reproduces_the_reference_chain(fx):
    """kin_ref against kin.npz, the 64 seeded robots and the robot_data.py:234-246 state."""
    worst = _report("kin_ref vs kin.npz", kin_ref.robot_errors(kin_ref.kinematics(fx["geom"], *_inputs(fx)), fx))
    assert worst < CPU_BOUND
    demo = kin_ref.kinematics(fx["geom_aliengo"][None], *(a[None] for a in _inputs(fx, "demo_")))
    for k in kin_ref.OUTPUTS:
        assert kin_ref.norm_err(demo[k][0], fx["demo_" + k]) < CPU_BOUND, k


def test_host_compiled_header_reproduces_the_reference_chain(fx, leg):
    """csrc/mpcqp_kin_leg.h compiled with g++: the same checks."""
    worst = _report("mpcqp_kin_leg.h (g++) vs kin.npz",
                    kin_ref.robot_errors(run_header(leg, fx["geom"], *_inputs(fx)), fx))
    assert worst < CPU_BOUND
    demo = run_header(leg, fx["geom_aliengo"][None], *(a[None] for a in _inputs(fx, "demo_")))
    for k in kin_ref.OUTPUTS:
        assert kin_ref.norm_err(demo[k][0], fx["demo_" + k]) < CPU_BOUND, k


def test_fixture_jv_layout(fx):
    """The fixture's 3 x 18 Jv_feet is laid out as Pinocchio's: Rq, -Rq [p]x, the leg's block
    (which is the kernel's jac) at 6 + 3 leg, zeros elsewhere."""
    Jv, Rq = fx["Jv"], kin_ref.quat2matrix_eigen(fx["quat"])
    for leg in range(4):
        assert np.array_equal(Jv[:, leg, :, 0:3], Rq)
        assert np.array_equal(Jv[:, leg, :, 6 + 3 * leg:9 + 3 * leg], fx["jac"][:, leg])
        rest = np.delete(Jv[:, leg], np.r_[0:6, 6 + 3 * leg:9 + 3 * leg], axis=2)
        assert rest.shape[-1] == 9 and (rest == 0).all()


def test_known_answers_at_zero_pose(leg):
    """q = 0, identity orientation: foot = (+-hx, +-(hy + d), -(l1 + l2)), the thigh joint
    above it, and with qdot = 0 foot_vel_base = 0 for any v -- in the header and in the
    restatement alike.  With omega != 0 it is omega x p, not 0: the reference's expression
    (robot_data.py:158-167) subtracts lin_vel_base from Jv [v, omega, qdot] and keeps the
    free-flyer's angular columns, so R_base^T (Rq (v + omega x p + J_b qdot) - v) leaves
    omega x p at identity orientation.  Both are checked."""
    from mpcqp.params import LEG_GEOMETRY
    rng = np.random.default_rng(3)
    geom = np.array([LEG_GEOMETRY["a1"], LEG_GEOMETRY["aliengo"]])
    B = len(geom)
    quat = np.tile(np.array([1, 0, 0, 0], np.float32), (B, 1))
    pos = rng.uniform(-1, 1, (B, 3)).astype(np.float32)
    vel, omega = rng.uniform(-2, 2, (2, B, 3)).astype(np.float32)
    z = np.zeros((B, 12), np.float32)
    hx, hy, d, l1, l2 = geom.T
    want = np.stack([np.stack([sx * hx, sy * (hy + d), -(l1 + l2)], -1)
                     for sx, sy in zip(kin_ref.SX, kin_ref.SY)], 1)
    wth = want.copy()
    wth[..., 2] = 0.0
    for o in (kin_ref.kinematics(geom, quat, pos, vel, omega, z, z), run_header(leg, geom, quat, pos, vel, omega, z, z)):
        assert np.array_equal(o["feet"], want) and np.array_equal(o["foot_pos_base"], want)
        assert np.array_equal(o["thighs"], wth)
        assert np.array_equal(o["pos_feet"], pos[:, None].astype(np.float64) + want)
        # R = I: v + omega x p - v, and (v + x) - v is x up to a rounding of v + x
        wxp = np.cross(omega[:, None].astype(np.float64), want)
        assert np.abs(o["foot_vel_base"] - wxp).max() < 1e-15 * 4
    zero3 = np.zeros((B, 3), np.float32)
    for o in (kin_ref.kinematics(geom, quat, pos, vel, zero3, z, z), run_header(leg, geom, quat, pos, vel, zero3, z, z)):
        assert (o["foot_vel_base"] == 0).all()      # any v, omega = 0: (v + 0) - v, exactly
    # with v = omega = 0 it is exactly 0 for any orientation and any q
    tilt = np.tile(np.array([0.9, 0.3, -0.2, 0.1], np.float32), (B, 1))
    q = rng.uniform(-1, 1, (B, 12)).astype(np.float32)
    for o in (kin_ref.kinematics(geom, tilt, pos, zero3, zero3, q, z), run_header(leg, geom, tilt, pos, zero3, zero3, q, z)):
        assert (o["foot_vel_base"] == 0).all()


def test_jacobian_against_its_own_central_differences():
    """jac of kin_ref = d feet / d q by central differences of kin_ref's own feet, and the
    base-frame Jb likewise: h = 1e-6 leaves 1e-16 / h rounding, a few 1e-10."""
    rng = np.random.default_rng(11)
    from mpcqp.params import LEG_GEOMETRY
    B, h = 16, 1e-6
    geom = np.array([LEG_GEOMETRY["a1"], LEG_GEOMETRY["aliengo"]])[np.arange(B) % 2]
    quat = rng.standard_normal((B, 4))
    quat = (quat / np.linalg.norm(quat, axis=1, keepdims=True)).astype(np.float32)
    q = rng.uniform(-2.5, 2.5, (B, 12))          # float64 here: the differences step by h
    p, _, Jb = kin_ref.chain(geom, q)
    Rq = kin_ref.quat2matrix_eigen(quat)
    jac = np.einsum("brk,blkc->blrc", Rq, Jb)
    for leg in range(4):
        for j in range(3):
            e = np.zeros((B, 12))
            e[:, 3 * leg + j] = h
            dp = (kin_ref.chain(geom, q + e)[0] - kin_ref.chain(geom, q - e)[0]) / (2 * h)
            assert np.abs(dp[:, leg] - Jb[:, leg, :, j]).max() < 2e-9
            others = [l for l in range(4) if l != leg]
            assert (dp[:, others] == 0).all()     # a leg's joints move that leg alone
            assert np.abs(np.einsum("brc,bc->br", Rq, dp[:, leg]) - jac[:, leg, :, j]).max() < 2e-9


def test_leg_geometry_presets_equal_the_urdf_geometry(fx):
    from mpcqp.params import LEG_GEOMETRY, pack_leg_geometry
    assert np.array_equal(np.array(LEG_GEOMETRY["a1"]), fx["geom_a1"])
    assert np.array_equal(np.array(LEG_GEOMETRY["aliengo"]), fx["geom_aliengo"])
    rec = pack_leg_geometry("a1")
    assert rec.shape == (8,) and rec.dtype == np.float64 and np.array_equal(rec[:5], fx["geom_a1"]) and (rec[5:] == 0).all()
    assert pack_leg_geometry("aliengo", 3).shape == (3, 8)
    mixed = pack_leg_geometry(fx["geom"])
    assert mixed.shape == (len(fx["geom"]), 8) and np.array_equal(mixed[:, :5], fx["geom"])
    with pytest.raises(ValueError):
        pack_leg_geometry((0.1, 0.2, 0.3))
    with pytest.raises(ValueError):
        pack_leg_geometry(fx["geom"], 3)


def test_leg_geometry_from_urdf(tmp_path):
    from mpcqp.params import leg_geometry_from_urdf

    def read(**kw):
        path = tmp_path / "toy.urdf"
        path.write_text(kin_ref.urdf_text(**kw))
        return leg_geometry_from_urdf(str(path))

    assert read() == (0.2, 0.05, 0.08, 0.21, 0.22)
    assert read(geom=(0.183, 0.047, 0.08505, 0.2, 0.2)) == (0.183, 0.047, 0.08505, 0.2, 0.2)
    with pytest.raises(ValueError, match="RL_thigh_joint.*about"):
        read(axis={"RL_thigh_joint": "1 0 0"})                  # a wrong axis
    with pytest.raises(ValueError, match="FR_calf_joint.*rpy"):
        read(rpy={"FR_calf_joint": "0 0.1 0"})                   # a non-zero rpy
    with pytest.raises(ValueError, match="RR.*mirror"):
        read(offset={"RR_hip_joint": "-0.2 0.05 0"})             # not the mirror image of FL
    with pytest.raises(ValueError, match="no joint"):
        path = tmp_path / "short.urdf"
        path.write_text(kin_ref.urdf_text().replace("RL_foot_fixed", "RL_toe_fixed"))
        leg_geometry_from_urdf(str(path))


# ---- the CPU twins of tests/test_gpu_kin_edges.py: the checks of tests/kin_edge_checks.py
# on the host build of the header, its float64 outputs rounded to float32 as the kernel's
# stores round them

@pytest.fixture(scope="module")
def edge_run(leg):
    def run(geom, inp, layout, rot):
        with np.errstate(all="ignore"):
            out = run_header(leg, geom, rot=rot, **inp)
            out = {k: np.concatenate([v.astype(np.float32), np.full((3,) + v.shape[1:], -77, np.float32)]) for k, v in out.items()}
        return out
    return run


@pytest.mark.parametrize("layout", ["split", "rot"])
def test_edge_poses(edge_run, leg, layout):
    """4a on the host (the root layout is the split one to the header).  The header itself,
    before the float32 store, is within 2.2e-16 of kin_ref."""
    worst = kin_edge_checks.check_edge_poses(edge_run, layout)
    print(f"\nedge poses on the host ({layout}), after the float32 store: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    geom, inp, rot = kin_ref.edge_poses()
    rot = rot if layout == "rot" else None
    errs = kin_ref.robot_errors(run_header(leg, geom, rot=rot, **inp), kin_ref.kinematics(geom, rot=rot, **inp))
    rows = np.arange(len(geom)) != 9                     # zero geometry: exact zeros, no norm to divide by
    f64 = max(float(np.nanmax(v[rows])) for v in errs.values())
    print(f"header vs kin_ref in float64: {f64:.2e}")
    assert f64 <= 1e-14
    normalised, swapped = kin_edge_checks.wrong_reading_moves_the_result()
    assert normalised >= 100 * kin_edge_checks.BOUND and swapped >= 100 * kin_edge_checks.BOUND


def test_edge_nan_stays_where_the_algebra_puts_it(edge_run):
    """4b on the host."""
    seen = kin_edge_checks.check_nan_stays_put(edge_run, "split")
    assert len(seen) == len(kin_ref.NAN_CASES)
    for (key, idx), pattern in seen.items():
        if key == "geom":
            print(f"\nNaN in geom[{idx}]: " + ", ".join(sorted({k for k, _ in pattern})))

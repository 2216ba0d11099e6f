"""ctypes binding of libmpcqp.so (include/mpcqp.h and its companion headers).

The shared library is built in-tree (``__graft_entry__.build()`` or
``python -m mpcqp.build``) next to this file.  There is deliberately no
fallback: if the library is missing or fails to load, every entry point raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MPCQP_LIB: diagnostic override (A/B builds); the default is the in-tree build
LIB_PATH = os.environ.get("MPCQP_LIB") or os.path.join(_HERE, "libmpcqp.so")

MPCQP_OK = 0
ERR_ARG = -1
ERR_HIP = -2
ERR_ALLOC = -3
STATUS_OK = 0
STATUS_MAX_ITER = 1
STATUS_INFEASIBLE = 2
STATUS_TOO_LARGE = 3
STATUS_NONFINITE = 4
STATUS_UNSUPPORTED = 5
ROBOT_STRIDE = 16
MAX_HORIZON = 32    # MPCQP_MAX_HORIZON: mpcqp_create rejects a longer horizon

ABI_VERSION = 6
WARM_BYTES = 128     # MPCQP_WARM_BYTES: warm-start memory per robot
PLAN_STRIDE = 8     # MPCQP_PLAN_STRIDE: float64 planner state per robot
GAIT_STRIDE = 9     # MPCQP_GAIT_STRIDE: period, offsets[4], durations[4]
PLAN_REFERENCE = 1      # MPCQP_PLAN_REFERENCE: build X_ref (+ gait table) this tick
PLAN_NO_INTEGRATE = 2   # MPCQP_PLAN_NO_INTEGRATE: skip the desired-pose integrators
SWING_STRIDE = 32   # MPCQP_SWING_STRIDE: float64 swing-generator state per robot (8 per leg)
KIN_STRIDE = 8      # MPCQP_KIN_STRIDE: float64 leg geometry per robot (5 used)
STEP_MPC = 1        # MPCQP_STEP_MPC: this tick solves (plan with the reference, solve, leg torques)
EST_STRIDE = 352    # MPCQP_EST_STRIDE: float64 estimator record per robot (x[18], initialised, P at 24)
EST_DOF_STATES = 1  # MPCQP_EST_DOF_STATES: q is a dof-state tensor [B,12,2], qdot ignored
ATT_STRIDE = 8      # MPCQP_ATT_STRIDE: float64 orientation record per robot (q[4], initialised, gyro bias[3])
TERRAIN_STRIDE = 20        # MPCQP_TERRAIN_STRIDE: float64 terrain record per robot (history[4][3], initialised, n[3], d, fitted)
TERRAIN_SWING_STATE = 1    # MPCQP_TERRAIN_SWING_STATE: contact is a swing_state, stance where !(value > 0)
TERRAIN_ROOT_STATES = 2    # MPCQP_TERRAIN_ROOT_STATES: quat is a root-state tensor [B,13]
TERRAIN_GROUND = 4         # MPCQP_TERRAIN_GROUND: plane is the swing leg's ground, (n, d - n_z touchdown_z)
PLANT_STRIDE = 48          # MPCQP_PLANT_STRIDE (mpcqp_plant_abi.h): float64 plant record per robot (pos, quat, vel, omega, feet, foot velocities, contact, flag word, call count)
PLANT_MAX_SUBSTEPS = 16    # MPCQP_PLANT_MAX_SUBSTEPS (mpcqp_plant_abi.h)
PREDICT_REPORT = 4         # MPCQP_PREDICT_REPORT (mpcqp_predict_abi.h): float64 report per robot (cost, cost_free, cone margin, swing residual)

GAIT_MAX = 16              # MPCQP_GAIT_MAX (mpcqp_gait_abi.h): entries of the gait library
SCHED_STRIDE = 8           # MPCQP_SCHED_STRIDE (mpcqp_gait_abi.h): int32 scheduler record per robot (current, pending, since, switches, calm, last tick)
GAIT_ADVANCE = 1           # MPCQP_GAIT_ADVANCE (mpcqp_gait_abi.h): advance tick and since before deciding
SENSE_STRIDE = 16          # MPCQP_SENSE_STRIDE (mpcqp_disturb_abi.h): float64 sensor record per robot (gyro bias, accel bias, initialised, count, id, touch histories)
CERTIFY_REPORT = 4         # MPCQP_CERTIFY_REPORT (mpcqp_certify_abi.h): float64 report per robot (objective, gap, lower bound, worst foot-step term)


class MpcqpParams(ctypes.Structure):
    """struct mpcqp_params (include/mpcqp.h)."""
    _fields_ = [
        ("horizon", ctypes.c_int32),
        ("max_iter", ctypes.c_int32),
        ("dt", ctypes.c_double),
        ("q_diag", ctypes.c_double * 13),
        ("r_diag", ctypes.c_double * 12),
    ]


_vp, _i32, _int, _f64, _u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int, ctypes.c_double, ctypes.c_uint64
_params_p = ctypes.POINTER(MpcqpParams)

# The ABI, one row per function the headers under include/ declare: header -> symbol ->
# (restype, argtypes).  The context, the stream and every device or host array travel as void
# pointers (tests/test_abi.py holds each row to its declaration, position by position, and
# each symbol to one header).  A new stage is a new header and its rows here.
ABI = {
    "mpcqp.h": {
        "mpcqp_abi_version": (_i32, []),
        "mpcqp_default_params": (None, [_params_p, _i32]),
        "mpcqp_create": (_int, [_params_p, _i32, ctypes.POINTER(_vp)]),
        "mpcqp_solve": (_int, [_vp, _i32] + [_vp] * 10),
        "mpcqp_set_stance_hint": (_int, [_vp, _i32]),
        "mpcqp_set_stance_range": (_int, [_vp, _i32, _i32]),
        "mpcqp_set_order": (_int, [_vp, _i32]),
        "mpcqp_set_weights": (_int, [_vp, _vp, _vp]),
        "mpcqp_set_warm_start": (_int, [_vp, _vp, _i32]),
        "mpcqp_destroy": (_int, [_vp]),
        "mpcqp_last_error": (ctypes.c_char_p, [_vp]),
        "mpcqp_plan": (_int, [_vp, _i32, _i32] + [_vp] * 15),
        "mpcqp_plan_root_states": (_int, [_vp, _i32, _i32] + [_vp] * 11),
        "mpcqp_set_planner": (_int, [_vp, _f64, _f64, _f64]),
        "mpcqp_stance_torques": (_int, [_vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
        "mpcqp_leg_torques": (_int, [_vp, _i32, _i32, _vp, _i32] + [_vp] * 19),
        "mpcqp_leg_torques_root_states": (_int, [_vp, _i32, _i32, _vp, _i32] + [_vp] * 16),
        "mpcqp_set_swing": (_int, [_vp, _f64, _vp, _vp, _f64, _f64]),
        "mpcqp_kinematics": (_int, [_vp, _i32, _i32] + [_vp] * 15),
        "mpcqp_kinematics_root_states": (_int, [_vp, _i32, _i32] + [_vp] * 10),
        "mpcqp_step": (_int, [_vp, _i32, _i32, _i32, _vp, _i32] + [_vp] * 27),
        "mpcqp_estimate": (_int, [_vp, _i32, _i32] + [_vp] * 12),
        "mpcqp_set_estimator": (_int, [_vp] + [_f64] * 11),
        "mpcqp_attitude": (_int, [_vp, _i32, _i32, _vp, _vp, _vp, _i32] + [_vp] * 8),
        "mpcqp_set_attitude": (_int, [_vp] + [_f64] * 6),
        "mpcqp_terrain": (_int, [_vp, _i32, _i32] + [_vp] * 10),
        "mpcqp_set_terrain": (_int, [_vp] + [_f64] * 4),
        "mpcqp_set_ground": (_int, [_vp, _vp, _i32]),
    },
    "mpcqp_predict_abi.h": {
        "mpcqp_predict": (_int, [_vp, _i32, _i32] + [_vp] * 10),
    },
    "mpcqp_plant_abi.h": {
        "mpcqp_plant": (_int, [_vp, _i32, _i32] + [_vp] * 12),
        "mpcqp_plant_reset": (_int, [_vp, _i32] + [_vp] * 6),
        "mpcqp_set_plant": (_int, [_vp, _f64, _i32, _f64, _f64]),
    },
    "mpcqp_certify_abi.h": {
        "mpcqp_certify": (_int, [_vp, _i32, _i32] + [_vp] * 10),
    },
    "mpcqp_gait_abi.h": {
        "mpcqp_set_gaits": (_int, [_vp, _i32, _vp]),
        "mpcqp_set_gait_schedule": (_int, [_vp, _i32, _i32, _i32, _f64, _f64, _f64, _f64, _i32]),
        "mpcqp_gait_schedule": (_int, [_vp, _i32, _i32, _i32] + [_vp] * 11),
    },
    "mpcqp_disturb_abi.h": {
        "mpcqp_sensors": (_int, [_vp, _i32, _i32] + [_vp] * 12),
        "mpcqp_set_sensors": (_int, [_vp, _u64] + [_f64] * 9 + [_i32, _f64]),
        "mpcqp_push": (_int, [_vp, _i32] + [_vp] * 6),
    },
}
# every row, flat: what load() applies
SIGNATURES = {name: row for rows in ABI.values() for name, row in rows.items()}
EXPORTED_SYMBOLS = tuple(ABI["mpcqp.h"])   # every symbol declared in include/mpcqp.h


class MpcqpError(RuntimeError):
    pass


_lib = None


def load():
    """Load libmpcqp.so once; raise MpcqpError if it is absent (no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MpcqpError(f"{LIB_PATH} not built: run __graft_entry__.build() "
                         "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.mpcqp_abi_version() != ABI_VERSION:
        raise MpcqpError("libmpcqp ABI version mismatch")
    _lib = lib
    return lib


def default_params(horizon):
    p = MpcqpParams()
    load().mpcqp_default_params(ctypes.byref(p), int(horizon))
    return p


def lib_sha256(path=None):
    """SHA-256 of the engine library file (ties a profile's counters to the build that made them)."""
    import hashlib
    with open(path or LIB_PATH, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()


def check(ctx, code, what):
    if code != MPCQP_OK:
        msg = load().mpcqp_last_error(ctx) if ctx else b""
        raise MpcqpError(f"{what} failed ({code}): {msg.decode() if msg else ''}")

"""ctypes binding of libmpcqp.so (include/mpcqp.h).

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

# every symbol declared in include/mpcqp.h
EXPORTED_SYMBOLS = (
    "mpcqp_abi_version",
    "mpcqp_default_params",
    "mpcqp_create",
    "mpcqp_solve",
    "mpcqp_set_stance_hint",
    "mpcqp_set_stance_range",
    "mpcqp_set_order",
    "mpcqp_set_weights",
    "mpcqp_set_warm_start",
    "mpcqp_destroy",
    "mpcqp_last_error",
    "mpcqp_plan",
    "mpcqp_plan_root_states",
    "mpcqp_set_planner",
    "mpcqp_stance_torques",
    "mpcqp_leg_torques",
    "mpcqp_leg_torques_root_states",
    "mpcqp_set_swing",
    "mpcqp_kinematics",
    "mpcqp_kinematics_root_states",
    "mpcqp_step",
    "mpcqp_estimate",
    "mpcqp_set_estimator",
    "mpcqp_attitude",
    "mpcqp_set_attitude",
    "mpcqp_terrain",
    "mpcqp_set_terrain",
    "mpcqp_set_ground",
)
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


class MpcqpParams(ctypes.Structure):
    """struct mpcqp_params (include/mpcqp.h)."""
    _fields_ = [
        ("horizon", ctypes.c_int32),
        ("max_iter", ctypes.c_int32),
        ("dt", ctypes.c_double),
        ("q_diag", ctypes.c_double * 13),
        ("r_diag", ctypes.c_double * 12),
    ]


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
    vp, i32, f32p, i32p = ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p
    lib.mpcqp_abi_version.restype = i32
    lib.mpcqp_abi_version.argtypes = []
    lib.mpcqp_default_params.restype = None
    lib.mpcqp_default_params.argtypes = [ctypes.POINTER(MpcqpParams), i32]
    lib.mpcqp_create.restype = ctypes.c_int
    lib.mpcqp_create.argtypes = [ctypes.POINTER(MpcqpParams), i32, ctypes.POINTER(vp)]
    lib.mpcqp_solve.restype = ctypes.c_int
    lib.mpcqp_solve.argtypes = [vp, i32, f32p, f32p, f32p, f32p, f32p, f32p, f32p, i32p, i32p, vp]
    lib.mpcqp_set_stance_hint.restype = ctypes.c_int
    lib.mpcqp_set_stance_hint.argtypes = [vp, i32]
    lib.mpcqp_set_stance_range.restype = ctypes.c_int
    lib.mpcqp_set_stance_range.argtypes = [vp, i32, i32]
    lib.mpcqp_set_order.restype = ctypes.c_int
    lib.mpcqp_set_order.argtypes = [vp, i32]
    lib.mpcqp_set_weights.restype = ctypes.c_int
    lib.mpcqp_set_weights.argtypes = [vp, vp, vp]
    lib.mpcqp_set_warm_start.restype = ctypes.c_int
    lib.mpcqp_set_warm_start.argtypes = [vp, vp, i32]
    lib.mpcqp_destroy.restype = ctypes.c_int
    lib.mpcqp_destroy.argtypes = [vp]
    lib.mpcqp_last_error.restype = ctypes.c_char_p
    lib.mpcqp_last_error.argtypes = [vp]
    lib.mpcqp_plan.restype = ctypes.c_int
    lib.mpcqp_plan.argtypes = [vp, i32, i32] + [vp] * 14 + [vp]
    lib.mpcqp_plan_root_states.restype = ctypes.c_int
    lib.mpcqp_plan_root_states.argtypes = [vp, i32, i32] + [vp] * 10 + [vp]
    lib.mpcqp_set_planner.restype = ctypes.c_int
    lib.mpcqp_set_planner.argtypes = [vp, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    lib.mpcqp_stance_torques.restype = ctypes.c_int
    lib.mpcqp_stance_torques.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp]
    lib.mpcqp_leg_torques.restype = ctypes.c_int
    lib.mpcqp_leg_torques.argtypes = [vp, i32, i32, vp, i32] + [vp] * 18 + [vp]
    lib.mpcqp_leg_torques_root_states.restype = ctypes.c_int
    lib.mpcqp_leg_torques_root_states.argtypes = [vp, i32, i32, vp, i32] + [vp] * 15 + [vp]
    lib.mpcqp_set_swing.restype = ctypes.c_int
    lib.mpcqp_set_swing.argtypes = [vp, ctypes.c_double, vp, vp, ctypes.c_double, ctypes.c_double]
    lib.mpcqp_kinematics.restype = ctypes.c_int
    lib.mpcqp_kinematics.argtypes = [vp, i32, i32] + [vp] * 14 + [vp]
    lib.mpcqp_kinematics_root_states.restype = ctypes.c_int
    lib.mpcqp_kinematics_root_states.argtypes = [vp, i32, i32] + [vp] * 9 + [vp]
    lib.mpcqp_step.restype = ctypes.c_int
    lib.mpcqp_step.argtypes = [vp, i32, i32, i32, vp, i32] + [vp] * 26 + [vp]
    lib.mpcqp_estimate.restype = ctypes.c_int
    lib.mpcqp_estimate.argtypes = [vp, i32, i32] + [vp] * 11 + [vp]
    lib.mpcqp_set_estimator.restype = ctypes.c_int
    lib.mpcqp_set_estimator.argtypes = [vp] + [ctypes.c_double] * 11
    lib.mpcqp_attitude.restype = ctypes.c_int
    lib.mpcqp_attitude.argtypes = [vp, i32, i32, vp, vp, vp, i32] + [vp] * 7 + [vp]
    lib.mpcqp_set_attitude.restype = ctypes.c_int
    lib.mpcqp_set_attitude.argtypes = [vp] + [ctypes.c_double] * 6
    lib.mpcqp_terrain.restype = ctypes.c_int
    lib.mpcqp_terrain.argtypes = [vp, i32, i32] + [vp] * 9 + [vp]
    lib.mpcqp_set_terrain.restype = ctypes.c_int
    lib.mpcqp_set_terrain.argtypes = [vp] + [ctypes.c_double] * 4
    lib.mpcqp_set_ground.restype = ctypes.c_int
    lib.mpcqp_set_ground.argtypes = [vp, vp, i32]
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

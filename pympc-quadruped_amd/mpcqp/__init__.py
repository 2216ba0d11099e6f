"""mpcqp -- MI355X-native batched convex-MPC QP engine.

Drop-in for the formulate-and-solve hot path of yinghansun/pympc-quadruped
(``ModelPredictiveController._solve_mpc``, linear_mpc/mpc.py:262-290).
"""
from .params import (DT_MPC, GAITS, GRAVITY, LEG_GEOMETRY, MU, Q_DIAG, R_DIAG, ROBOT_PRESETS, ROBOT_STRIDE,
                     leg_geometry_from_urdf, pack_leg_geometry, pack_robot, robot_from_config)

__all__ = ["LinearMpc", "SolveResult", "PredictResult", "CertifyResult", "BatchedTerrain", "BatchedPlant", "BatchedGaitScheduler", "BatchedSensors", "SENSOR_PRESETS", "DT_MPC", "GAITS", "GRAVITY", "LEG_GEOMETRY", "MU", "Q_DIAG", "R_DIAG",
           "ROBOT_PRESETS", "ROBOT_STRIDE", "leg_geometry_from_urdf", "pack_leg_geometry", "pack_robot",
           "robot_from_config"]


def __getattr__(name):
    # torch is imported lazily so that the host-only helpers stay importable without it
    if name in ("LinearMpc", "SolveResult", "PredictResult", "CertifyResult"):
        from . import engine
        return getattr(engine, name)
    if name == "BatchedTerrain":
        from .terrain import BatchedTerrain
        return BatchedTerrain
    if name == "BatchedPlant":
        from .plant import BatchedPlant
        return BatchedPlant
    if name == "BatchedGaitScheduler":
        from .gait import BatchedGaitScheduler
        return BatchedGaitScheduler
    if name in ("BatchedSensors", "SENSOR_PRESETS"):
        from . import sensors
        return getattr(sensors, name)
    raise AttributeError(name)

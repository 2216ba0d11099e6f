"""Generate tests/golden/terrain.npz FROM THE REFERENCE ITSELF (see make_golden.py: runs only
where the reference tree is present).

RobotData.update_terrain_normal (utils/robot_data.py:186-228) is defined and never called, and
RobotData's constructor needs Pinocchio and a URDF.  So `pinocchio` is stubbed in sys.modules,
the object is created with RobotData.__new__, and the three attributes the method reads are set
on it by hand: the private _RobotData__contact_history (four zero points, float32, as the
constructor leaves it -- init_contact_history is a no-op comparison), pos_feet and R_base.  The
reference's own method is then called over 30 ticks of 4 robots, on the feet and the trot
contact states of tests/terrain_ref.make_trajectory(4, 30, seed=3).

Recorded: the inputs (pos_feet float32, contact as bytes), the contact history after every call
(float32, as the reference holds it) and the reference's terrain_normal_est (float32, the
precision its float32 scatter matrix gives it).

Usage:  python tests/golden/make_golden_terrain.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from make_golden import stub_reference  # noqa: E402

T, B, SEED = 30, 4, 3


def main():
    import swing_ref
    import terrain_ref
    stub_reference(16)
    import robot_data
    traj = terrain_ref.make_trajectory(B, T, SEED)
    robots = []
    for b in range(B):
        rd = robot_data.RobotData.__new__(robot_data.RobotData)
        rd._RobotData__contact_history = np.zeros((4, 3), dtype=np.float32)
        robots.append(rd)
    hist = np.zeros((T, B, 4, 3), np.float32)
    normal = np.zeros((T, B, 3), np.float64)
    for t, step in enumerate(traj):
        R = swing_ref.quat2matrix_f32(step["quat"])
        for b, rd in enumerate(robots):
            rd.pos_feet = [step["pos_feet"][b, i] for i in range(4)]
            rd.R_base = R[b]
            rd.update_terrain_normal([int(c) for c in step["contact"][b]])
            hist[t, b] = rd._RobotData__contact_history
            normal[t, b] = np.real(rd.terrain_normal_est)
    out = os.path.join(HERE, "terrain.npz")
    np.savez_compressed(out, pos_feet=np.stack([s["pos_feet"] for s in traj]),
                        contact=np.stack([s["contact"] for s in traj]).astype(np.uint8),
                        history=hist, terrain_normal_est=normal.astype(np.float32))
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

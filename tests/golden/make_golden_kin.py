"""Generate tests/golden/kin.npz FROM THE REFERENCE ITSELF (see make_golden.py: runs only
where the reference tree is present).

Pinocchio is not importable here, so RobotData.update (utils/robot_data.py:59-108) is
rebuilt from the reference's own pieces:

  geometry    the xyz / rpy / axis of the hip, thigh, calf and foot joints of all four legs,
              read from robot/a1/urdf/a1.urdf and robot/aliengo/urdf/aliengo.urdf
  positions   kinematics.fk_open_chain on screw axes from kinematics.compute_screw_axis and
              a home configuration from kinematics.Rp2T, per leg, with that leg's own URDF
              offsets (no mirroring assumed): the foot through hip, thigh and calf, the
              thigh joint through the hip alone
  Jacobians   central differences of that chain in the joint angles, h = 1e-6
  free flyer  Rq = Eigen's quaternion-to-matrix formula in float64 on the float32
              quaternion as given, which is what pinocchio.forwardKinematics applies to
              generalized_q (robot_data.py:85-92); oMf.translation = pos + Rq p
  Jv_feet     3 x 18 as Pinocchio lays out LOCAL_WORLD_ALIGNED (robot_data.py:117-133):
              columns 0:3 = Rq, 3:6 = -Rq [p]x, the leg's block at 6 + 3 leg, zeros elsewhere
  the rest    robot_data.py:144-184 evaluated as written, on float32 inputs (the dtype
              scripts/isaacgym_a1.py:121-132 hands over), R_base by the reference's own
              kinematics.quat2matrix on the float32 quaternion

Recorded: the parsed geometry of both robots; B = 64 seeded robots with alternating
blocks of A1 and Aliengo geometry, random unit quaternions (tilt up to +-0.5 rad, any yaw)
rounded to float32, joint angles around a crouch (hip +-0.8, thigh 0.7 +- 1.5, calf -1.5 +-
1.2, different for every leg) and joint rates of order 1 rad/s; and the Aliengo state
printed in robot_data.py:234-246 (keys demo_*), its inputs rounded to float32.

Usage:  python tests/golden/make_golden_kin.py
"""
import os
import sys
import xml.etree.ElementTree as ET

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402

sys.path.insert(0, f"{REF}/utils")
import kinematics as K  # noqa: E402  (the reference's utils/kinematics.py)

LEGS = ("FL", "FR", "RL", "RR")
URDF = {"a1": f"{REF}/robot/a1/urdf/a1.urdf", "aliengo": f"{REF}/robot/aliengo/urdf/aliengo.urdf"}
H = 1e-6
B = 64


def parse(path):
    """{leg: (hip xyz, thigh xyz, calf xyz, foot xyz)}, asserting axes x, y, y and zero rpy."""
    joints = {j.get("name"): j for j in ET.parse(path).getroot().iter("joint") if j.get("type")}
    out = {}
    for leg in LEGS:
        xyz = []
        for part, axis in (("hip_joint", "1 0 0"), ("thigh_joint", "0 1 0"), ("calf_joint", "0 1 0"),
                           ("foot_fixed", None)):
            j = joints[f"{leg}_{part}"]
            o = j.find("origin")
            assert [float(x) for x in o.get("rpy").split()] == [0.0, 0.0, 0.0], (leg, part)
            if axis is not None:
                assert [float(x) for x in j.find("axis").get("xyz").split()] == [float(x) for x in axis.split()]
            xyz.append(np.array([float(x) for x in o.get("xyz").split()]))
        out[leg] = tuple(xyz)
    return out


def leg_chain(offsets):
    """Screw axes and home configurations of one leg in the base frame at q = 0."""
    hip, thigh, calf, foot = offsets
    a_hip, a_thigh, a_calf = hip, hip + thigh, hip + thigh + calf
    S = [K.compute_screw_axis([1, 0, 0], list(a_hip)), K.compute_screw_axis([0, 1, 0], list(a_thigh)),
         K.compute_screw_axis([0, 1, 0], list(a_calf))]
    return S, K.Rp2T(np.identity(3), a_calf + foot), K.Rp2T(np.identity(3), a_thigh)


def foot_fk(chain, q):
    S, M_foot, _ = chain
    return K.fk_open_chain(M_foot, S, list(q))[0:3, 3]


def thigh_fk(chain, q):
    S, _, M_thigh = chain
    return K.fk_open_chain(M_thigh, S[:1], [q[0]])[0:3, 3]


def quat_eigen(q):
    """Eigen's Quaternion::toRotationMatrix on (w, x, y, z), float64."""
    w, x, y, z = (float(v) for v in q)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def robot_update(chains, pos_base, lin_vel_base, quat_base, ang_vel_base, q, qdot):
    """RobotData.update for one robot; every input a float32 array."""
    R_base = K.quat2matrix(quat_base)                       # robot_data.py:75 (float32 arithmetic)
    rpy_base = np.array(K.quat2ZYXangle(quat_base))         # :76
    gq = np.array(list(pos_base) + [quat_base[1], quat_base[2], quat_base[3], quat_base[0]] + list(q),
                  dtype=np.float32).astype(np.float64)      # :85-90, widened by the binding
    Rq = quat_eigen([gq[6], gq[3], gq[4], gq[5]])
    pos_feet, pos_thighs, Jv_feet, p_base = [], [], [], []
    for leg in range(4):
        ql = gq[7 + 3 * leg:10 + 3 * leg]
        p = foot_fk(chains[leg], ql)
        Jb = np.zeros((3, 3))
        for j in range(3):
            e = np.zeros(3)
            e[j] = H
            Jb[:, j] = (foot_fk(chains[leg], ql + e) - foot_fk(chains[leg], ql - e)) / (2 * H)
        Jv = np.zeros((3, 18))
        Jv[:, 0:3] = Rq
        Jv[:, 3:6] = -Rq @ K.vec2so3(list(p))
        Jv[:, 6 + 3 * leg:9 + 3 * leg] = Rq @ Jb
        Jv_feet.append(Jv)
        p_base.append(p)
        pos_feet.append(gq[0:3] + Rq @ p)                                   # oMf[foot].translation
        pos_thighs.append(gq[0:3] + Rq @ thigh_fk(chains[leg], ql))         # oMf[thigh].translation
    # robot_data.py:144-184
    pos_base_feet = [pos_feet[i] - pos_base for i in range(4)]
    base_pos_base_feet = [R_base.T @ pos_base_feet[i] for i in range(4)]
    base_vel_base_feet = []
    for i in range(4):
        generalized_qdot = np.array(list(lin_vel_base) + list(ang_vel_base) + list(qdot), dtype=np.float32)
        vel_footi = Jv_feet[i] @ generalized_qdot
        base_vel_base_feet.append(R_base.T @ (vel_footi - lin_vel_base))
    base_pos_base_thighs = [R_base.T @ (pos_thighs[i] - pos_base) for i in range(4)]
    f8 = lambda a: np.asarray(a, np.float64)
    return dict(R_base=np.asarray(R_base, np.float32), rpy=f8(rpy_base), Jv=f8(Jv_feet), pos_feet=f8(pos_feet),
                feet=f8(pos_base_feet), foot_pos_base=f8(base_pos_base_feet), foot_vel_base=f8(base_vel_base_feet),
                thighs=f8(base_pos_base_thighs), p_base=f8(p_base),
                jac=f8([Jv_feet[i][:, 6 + 3 * i:9 + 3 * i] for i in range(4)]))


def main():
    parsed = {k: parse(v) for k, v in URDF.items()}
    chains = {k: [leg_chain(parsed[k][leg]) for leg in LEGS] for k in parsed}
    geom = {}
    for k, legs in parsed.items():
        hip, thigh, calf, foot = legs["FL"]
        geom[k] = np.array([hip[0], hip[1], thigh[1], -calf[2], -foot[2]])
    names = ("a1", "aliengo")
    rng = np.random.default_rng(20261019)
    f4 = np.float32
    robot = (np.arange(B) // 3) % 2                         # blocks of three: A1, Aliengo, ...
    rpy = rng.uniform([-0.5, -0.5, -np.pi], [0.5, 0.5, np.pi], (B, 3))
    c, s = np.cos(rpy / 2), np.sin(rpy / 2)
    cr, cp, cy, sr, sp, sy = c[:, 0], c[:, 1], c[:, 2], s[:, 0], s[:, 1], s[:, 2]
    quat = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy,
                     cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], -1).astype(f4)
    pos = rng.uniform([-2.0, -2.0, 0.2], [2.0, 2.0, 0.45], (B, 3)).astype(f4)
    vel = rng.uniform(-1.0, 1.0, (B, 3)).astype(f4)
    omega = rng.uniform(-1.5, 1.5, (B, 3)).astype(f4)
    q = (np.array([0.0, 0.7, -1.5]) + rng.uniform(-1.0, 1.0, (B, 4, 3)) * np.array([0.8, 1.5, 1.2])).reshape(B, 12)
    q = q.astype(f4)
    qdot = rng.standard_normal((B, 12)).astype(f4)
    rows = [robot_update(chains[names[robot[b]]], pos[b], vel[b], quat[b], omega[b], q[b], qdot[b]) for b in range(B)]
    out = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
    out.update(geom_a1=geom["a1"], geom_aliengo=geom["aliengo"], robot=robot.astype(np.int32),
               geom=np.stack([geom[names[r]] for r in robot]), quat=quat, pos=pos, vel=vel, omega=omega, q=q,
               qdot=qdot, h=np.float64(H))
    # the state printed in robot_data.py:234-246 (aliengo.urdf), rounded to float32
    demo = dict(pos=[0.00727408, 0.00061764, 0.43571295], vel=[0.0189759, 0.00054278, 0.02322867],
                quat=[9.99951619e-01, -9.13191258e-03, 3.57360542e-03, 7.72221709e-04],
                omega=[-0.06964452, -0.01762341, -0.00088601],
                q=[0.00687206, 0.52588717, -1.22975589, 0.02480081, 0.51914926, -1.21463939,
                   0.00892169, 0.51229961, -1.20195572, 0.02621839, 0.50635251, -1.18849609],
                qdot=[0.06341452, -0.02158136, 0.16191205, 0.07448259, -0.04855474, 0.21399941,
                      0.06280346, 0.00562435, 0.10597827, 0.07388069, -0.02180622, 0.15909948])
    demo = {k: np.array(v, dtype=f4) for k, v in demo.items()}
    d = robot_update(chains["aliengo"], demo["pos"], demo["vel"], demo["quat"], demo["omega"], demo["q"],
                     demo["qdot"])
    out.update({"demo_" + k: v for k, v in {**demo, **d}.items()})
    path = os.path.join(HERE, "kin.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {B} robots; demo base_pos_base_feet =\n"
          f"{out['demo_foot_pos_base']}")


if __name__ == "__main__":
    main()

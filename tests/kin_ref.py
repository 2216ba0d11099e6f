"""Float64 restatement of the leg kinematics (mpcqp_kinematics), batched with NumPy: the
same inputs and outputs as the kernel, for B robots x 4 legs.  It restates
RobotData.update (utils/robot_data.py:59-108) for the hip-x / thigh-y / calf-y leg in
closed form; tests/golden/kin.npz records the same quantities from the reference's own
product-of-exponentials chain."""
import os

import numpy as np

from swing_ref import norm_err, quat2matrix_f32  # noqa: F401  (re-exported for the tests)

STRIDE = 8                                           # MPCQP_KIN_STRIDE
SX = np.array([1.0, 1.0, -1.0, -1.0])                # FL, FR, RL, RR
SY = np.array([1.0, -1.0, 1.0, -1.0])
OUTPUTS = ("feet", "thighs", "pos_feet", "foot_pos_base", "foot_vel_base", "jac")


def quat2matrix_eigen(quat):
    """[B,4] (w, x, y, z) -> [B,3,3] float64: Eigen's Quaternion::toRotationMatrix, which
    Pinocchio's free-flyer joint applies to the quaternion as given (no normalisation)."""
    q = np.asarray(quat).astype(np.float64)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.stack([1.0 - (tyy + tzz), txy - twz, txz + twy,
                  txy + twz, 1.0 - (txx + tzz), tyz - twx,
                  txz - twy, tyz + twx, 1.0 - (txx + tyy)], axis=1)
    return R.reshape(-1, 3, 3)


def chain(geom, q):
    """geom [B,>=5] (hip_x, hip_y, thigh_y, l_thigh, l_calf), q [B,12] -> foot p [B,4,3],
    thigh joint pth [B,4,3] and Jb = dp/dq [B,4,3,3], all in the base frame."""
    g = np.asarray(geom, np.float64)
    q = np.asarray(q).astype(np.float64).reshape(-1, 4, 3)
    hx, hy, d = SX * g[:, 0:1], SY * g[:, 1:2], SY * g[:, 2:3]
    l1, l2 = g[:, 3:4], g[:, 4:5]
    s1, c1 = np.sin(q[..., 0]), np.cos(q[..., 0])
    s2, c2 = np.sin(q[..., 1]), np.cos(q[..., 1])
    s23, c23 = np.sin(q[..., 1] + q[..., 2]), np.cos(q[..., 1] + q[..., 2])
    ux = -l1 * s2 - l2 * s23
    uz = -l1 * c2 - l2 * c23
    p = np.stack([hx + ux, hy + d * c1 - uz * s1, d * s1 + uz * c1], -1)
    pth = np.stack([hx + 0 * s1, hy + d * c1, d * s1], -1)
    zero = np.zeros_like(ux)
    Jb = np.stack([np.stack([zero, uz, -l2 * c23], -1),
                   np.stack([-d * s1 - uz * c1, ux * s1, -l2 * s23 * s1], -1),
                   np.stack([d * c1 - uz * s1, -ux * c1, l2 * s23 * c1], -1)], -2)
    return p, pth, Jb


def kinematics(geom, quat, pos, vel, omega, q, qdot, rot=None):
    """The kernel's outputs in float64 (dict of OUTPUTS).  quat [B,4] (w, x, y, z), pos /
    vel / omega [B,3], q / qdot [B,12]: float32 values; rot [B,3,3]: R_base, default the
    float32-arithmetic quat2matrix (robot_data.py:75)."""
    Rq = quat2matrix_eigen(quat)
    Rb = (quat2matrix_f32(quat) if rot is None else np.asarray(rot)).astype(np.float64).reshape(-1, 3, 3)
    pos, v, w = (np.asarray(a).astype(np.float64) for a in (pos, vel, omega))
    qd = np.asarray(qdot).astype(np.float64).reshape(-1, 4, 3)
    p, pth, Jb = chain(geom, q)
    world = lambda x: np.einsum("brc,blc->blr", Rq, x)          # Rq x
    to_base = lambda x: np.einsum("bcr,blc->blr", Rb, x)        # R_base^T x
    feet = world(p)
    u = v[:, None] + np.cross(w[:, None], p) + np.einsum("blrc,blc->blr", Jb, qd)
    return dict(feet=feet, thighs=to_base(world(pth)), pos_feet=pos[:, None] + feet, foot_pos_base=to_base(feet),
                foot_vel_base=to_base(world(u) - v[:, None]), jac=np.einsum("brk,blkc->blrc", Rq, Jb))


def root_states(quat, pos, vel, omega):
    """Isaac Gym actor root states [B,13]: pos, quat (x, y, z, w), lin_vel, ang_vel."""
    return np.concatenate([pos, quat[..., 1:4], quat[..., 0:1], vel, omega], -1).astype(np.float32)


def dof_states(q, qdot):
    """Isaac Gym dof states [B,12,2]: (pos, vel) per DOF."""
    return np.ascontiguousarray(np.stack([q, qdot], -1).astype(np.float32))


def robot_errors(out, ref, rows=None):
    """Norm-wise error per robot, max|a - ref| / max|ref|: {output: [B]}."""
    errs = {}
    for k in OUTPUTS:
        a, r = np.asarray(out[k], np.float64), np.asarray(ref[k], np.float64)
        if rows is not None:
            r = r[rows]
        errs[k] = np.array([norm_err(a[b], r[b]) for b in range(a.shape[0])])
    return errs


def make_states(B, T, seed):
    """Seeded Isaac Gym tensors for T control iterations of B robots: actor root states
    [T,B,13] and dof states [T,B,12,2] (float32) -- a base that drifts, wobbles and yaws a
    little above a crouch whose joints swing smoothly, every leg on its own phase."""
    rng = np.random.default_rng(seed)
    t = 0.001 * np.arange(T)[:, None]
    ph = rng.uniform(0, 2 * np.pi, (B, 3))
    rpy = np.stack([0.05 * np.sin(9 * t + ph[:, 0]), 0.04 * np.sin(7 * t + ph[:, 1]),
                    rng.uniform(-1, 1, B) + 0.2 * t], -1)
    c, s = np.cos(rpy / 2), np.sin(rpy / 2)
    cr, cp, cy, sr, sp, sy = c[..., 0], c[..., 1], c[..., 2], s[..., 0], s[..., 1], s[..., 2]
    quat = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy,
                     cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], -1)
    vel = rng.uniform(-0.3, 0.3, (B, 3)) * np.ones((T, 1, 1))
    pos = rng.uniform([-1, -1, 0.27], [1, 1, 0.31], (B, 3)) + vel * t[..., None]
    omega = np.stack([0.45 * np.cos(9 * t + ph[:, 0]), 0.28 * np.cos(7 * t + ph[:, 1]), 0.2 + 0 * t + 0 * ph[:, 2]], -1)
    lp = rng.uniform(0, 2 * np.pi, (B, 12))
    amp = np.tile([0.1, 0.3, 0.3], 4)
    q = np.tile([0.0, 0.8, -1.6], 4) + amp * np.sin(12 * t[..., None] + lp)
    qdot = 12 * amp * np.cos(12 * t[..., None] + lp)
    return root_states(quat, pos, vel, omega), dof_states(q, qdot)


def urdf_text(geom=(0.2, 0.05, 0.08, 0.21, 0.22), axis=None, rpy=None, offset=None):
    """A minimal quadruped URDF with the shipped robots' joint names.  axis / rpy / offset:
    {joint name: text} overrides."""
    hx, hy, d, l1, l2 = geom
    axis, rpy, offset = axis or {}, rpy or {}, offset or {}
    out = ['<?xml version="1.0"?>', '<robot name="toy">', '<link name="trunk"/>']
    for leg, sx, sy in (("FR", 1, -1), ("FL", 1, 1), ("RR", -1, -1), ("RL", -1, 1)):
        chain = [("hip_joint", "revolute", f"{sx * hx} {sy * hy} 0", "1 0 0", "trunk", "hip"),
                 ("thigh_joint", "revolute", f"0 {sy * d} 0", "0 1 0", "hip", "thigh"),
                 ("calf_joint", "revolute", f"0 0 {-l1}", "0 1 0", "thigh", "calf"),
                 ("foot_fixed", "fixed", f"0 0 {-l2}", None, "calf", "foot")]
        for part, kind, xyz, ax, parent, child in chain:
            name = f"{leg}_{part}"
            out.append(f'<joint name="{name}" type="{kind}">')
            out.append(f'<origin rpy="{rpy.get(name, "0 0 0")}" xyz="{offset.get(name, xyz)}"/>')
            out.append(f'<parent link="{parent if parent == "trunk" else leg + "_" + parent}"/>')
            out.append(f'<child link="{leg}_{child}"/>')
            if ax is not None:
                out.append(f'<axis xyz="{axis.get(name, ax)}"/>')
            out.append("</joint>")
            out.append(f'<link name="{leg}_{child}"/>')
        # a transmission names the joint again, without a type (aliengo.urdf:379-382)
        out.append(f'<transmission name="{leg}_tran"><joint name="{leg}_hip_joint"/></transmission>')
    out.append("</robot>")
    return "\n".join(out)


def load_fixture():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kin.npz")
    return {k: v for k, v in np.load(path).items()}


# ---- edge inputs shared by tests/test_kin.py (the header on the host) and
# tests/test_gpu_kin_edges.py (the device)
A1, ALIENGO = (0.183, 0.047, 0.08505, 0.2, 0.2), (0.2399, 0.051, 0.083, 0.25, 0.25)
EDGE_ROWS = ("q = 0", "q = (pi, -pi, pi)", "calf = 0", "q = (1e4, -1e4, 3e3)", "q = (pi/2, pi/2, -pi)", "quat = 0",
             "2 quat", "quat / 2", "-quat", "geom = 0", "pos = (1e6, -1e6, 1e3)", "large vel, omega, qdot")


def ordinary(B, seed):
    """B seeded robots away from every edge: (geom [B,5], inputs dict, rot [B,3,3] float32 --
    another orientation's matrix, for the layout that takes R_base from the caller)."""
    rng = np.random.default_rng(seed)
    f = np.float32
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)
    geom = np.array([A1, ALIENGO])[np.arange(B) % 2]
    inp = dict(quat=unit(rng.standard_normal((B, 4))).astype(f), pos=rng.uniform(-1, 1, (B, 3)).astype(f),
               vel=rng.uniform(-2, 2, (B, 3)).astype(f), omega=rng.uniform(-2, 2, (B, 3)).astype(f),
               q=(np.tile([0.0, 0.8, -1.6], 4) + rng.uniform(-0.5, 0.5, (B, 12))).astype(f),
               qdot=rng.uniform(-3, 3, (B, 12)).astype(f))
    rot = quat2matrix_eigen(unit(rng.standard_normal((B, 4)))).astype(f)
    return geom, inp, rot


def edge_poses():
    """The EDGE_ROWS, one robot each, everything else ordinary: (geom, inputs, rot)."""
    geom, inp, rot = ordinary(len(EDGE_ROWS), seed=17)
    f, pi = np.float32, np.pi
    inp["q"][0] = 0.0
    inp["q"][1] = np.tile(f([pi, -pi, pi]), 4)
    inp["q"][2, 2::3] = 0.0
    inp["q"][3] = np.tile(f([1e4, -1e4, 3e3]), 4)
    inp["q"][4] = np.tile(f([pi / 2, pi / 2, -pi]), 4)
    inp["quat"][5] = 0.0
    inp["quat"][6] *= f(2)
    inp["quat"][7] *= f(0.5)
    inp["quat"][8] *= f(-1)
    geom[9] = 0.0
    inp["pos"][10] = f([1e6, -1e6, 1e3])
    inp["vel"][11], inp["omega"][11], inp["qdot"][11] = f([1e3, -1e3, 50]), f([200, -300, 100]), f(1e3)
    return geom, inp, rot


# a NaN in: (input, index within the robot's row); `q` at a thigh, a calf and a hip joint
NAN_CASES = (("quat", 2), ("pos", 1), ("vel", 0), ("omega", 2), ("q", 4), ("q", 11), ("q", 6), ("qdot", 1),
             ("geom", 0), ("geom", 1), ("geom", 2), ("geom", 3), ("geom", 4), ("rot", 5))

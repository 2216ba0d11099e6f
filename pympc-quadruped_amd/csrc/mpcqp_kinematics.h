// mpcqp_kinematics.h -- the leg kinematics on the device: foot and thigh positions, foot
// Jacobians and foot velocities of every robot in one launch (included by mpcqp.hip inside
// its anonymous namespace, after mpcqp_plan.h).  For B robots x 4 legs it is
// RobotData.update (utils/robot_data.py:59-108), Pinocchio's forward kinematics and frame
// Jacobians of the hip-x / thigh-y / calf-y leg in closed form, and produces every array
// mpcqp_solve (`feet`) and mpcqp_leg_torques (the other five) take from the kinematics.
//
// The per-leg algebra is mpcqp_kin_leg.h (float64, FP contraction off; also compiled for
// the host by tests/test_kin.py).  Each output is rounded to float32 once, at its store.
#include "mpcqp_kin_leg.h"

struct KinParams {
  int root_layout;   // 1: `quat` points at Isaac Gym actor root states [B][13] and `q` at
                     // its dof-state tensor [B][12][2] (pos, vel per DOF)
};

// A workgroup owns kKinRobots consecutive robots, one thread per (robot, leg) with a
// robot's four legs in adjacent lanes: q, qdot and the [B][4][3], [B][4][3][3] outputs are
// contiguous across the lanes.  What the four legs share (base state, both rotations,
// geometry) is read once per robot -- two of the robot's lanes each fetch a part -- and
// handed over in LDS.
constexpr int kKinRobots = 64;
constexpr int kKinThreads = 256;

struct KinBase {
  double Rq[9], geom[5];
  float pos[3], vel[3], omega[3], R[9];
};

__global__ __launch_bounds__(kKinThreads) void mpcqp_kinematics_kernel(
    KinParams kp, int B, const float* __restrict__ quat, const float* __restrict__ pos,
    const float* __restrict__ vel, const float* __restrict__ omega, const float* __restrict__ rot,
    const float* __restrict__ q, const float* __restrict__ qdot, const double* __restrict__ geom,
    float* __restrict__ feet, float* __restrict__ thighs, float* __restrict__ pos_feet,
    float* __restrict__ foot_pos_base, float* __restrict__ foot_vel_base, float* __restrict__ jac) {
#pragma clang fp contract(off)
  __shared__ KinBase base[kKinRobots];
  const int t = threadIdx.x;
  const int r = t >> 2, leg = t & 3;
  const int b = blockIdx.x * kKinRobots + r;
  const bool live = b < B;   // the tail workgroup: lanes past the batch touch no memory

  // ---- per-leg inputs (issued before the barrier so they overlap the shared reads)
  const size_t bl = (size_t)b * 4 + leg;
  double ql[3] = {0.0, 0.0, 0.0}, qd[3] = {0.0, 0.0, 0.0};
  if (live) {
    if (kp.root_layout) {   // (pos, vel) per DOF (isaacgym_a1.py:116,131-132)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        ql[k] = (double)q[(bl * 3 + k) * 2];
        qd[k] = (double)q[(bl * 3 + k) * 2 + 1];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        ql[k] = (double)q[bl * 3 + k];
        qd[k] = (double)qdot[bl * 3 + k];
      }
    }
  }

  // ---- per-robot inputs, once per robot
  if (live) {
    KinBase& kb = base[r];
    if (leg == 0) {
      float qw, qx, qy, qz;
      if (kp.root_layout) {   // [pos(3), quat(x, y, z, w), lin_vel(3), ang_vel(3)] (isaacgym_a1.py:119-130)
        const float* rs = quat + (size_t)b * 13;
        qx = rs[3], qy = rs[4], qz = rs[5], qw = rs[6];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          kb.pos[k] = rs[k];
          kb.vel[k] = rs[7 + k];
          kb.omega[k] = rs[10 + k];
        }
      } else {
        qw = quat[4 * (size_t)b], qx = quat[4 * (size_t)b + 1], qy = quat[4 * (size_t)b + 2],
        qz = quat[4 * (size_t)b + 3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          kb.pos[k] = pos[3 * (size_t)b + k];
          kb.vel[k] = vel[3 * (size_t)b + k];
          kb.omega[k] = omega[3 * (size_t)b + k];
        }
      }
      double Rq[9];
      kin_quat2matrix((double)qw, (double)qx, (double)qy, (double)qz, Rq);   // robot_data.py:85-92
      float R[9];
      if (rot != nullptr) {
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = rot[9 * (size_t)b + k];
      } else {
        plan_quat2matrix(qw, qx, qy, qz, R);   // robot_data.py:75
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        kb.Rq[k] = Rq[k];
        kb.R[k] = R[k];
      }
    } else if (leg == 1) {
#pragma unroll
      for (int k = 0; k < 5; ++k) kb.geom[k] = geom[KIN_STRIDE * (size_t)b + k];
    }
  }
  __syncthreads();
  if (!live) return;

  const KinBase& kb = base[r];
  double Rq[9], Rb[9], g[5], p3[3], v3[3], w3[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    Rq[k] = kb.Rq[k];
    Rb[k] = (double)kb.R[k];
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) g[k] = kb.geom[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    p3[k] = (double)kb.pos[k];
    v3[k] = (double)kb.vel[k];
    w3[k] = (double)kb.omega[k];
  }
  double ft[3], th[3], pf[3], fp[3], fv[3], J[9];
  kin_leg(g, leg, ql, qd, Rq, Rb, p3, v3, w3, ft, th, pf, fp, fv, J);
  if (feet != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) feet[bl * 3 + k] = (float)ft[k];
  }
  if (thighs != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) thighs[bl * 3 + k] = (float)th[k];
  }
  if (pos_feet != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) pos_feet[bl * 3 + k] = (float)pf[k];
  }
  if (foot_pos_base != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) foot_pos_base[bl * 3 + k] = (float)fp[k];
  }
  if (foot_vel_base != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) foot_vel_base[bl * 3 + k] = (float)fv[k];
  }
  if (jac != nullptr) {
#pragma unroll
    for (int k = 0; k < 9; ++k) jac[bl * 9 + k] = (float)J[k];
  }
}

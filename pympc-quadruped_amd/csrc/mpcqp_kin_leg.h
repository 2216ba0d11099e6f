// mpcqp_kin_leg.h -- per-leg algebra of the leg kinematics (mpcqp_kinematics.h), host- and
// device-callable so tests/ can check it on the CPU.
//
//   kin_quat2matrix   the free-flyer rotation of pinocchio.forwardKinematics    robot_data.py:85-92
//   kin_leg_chain     foot / thigh-joint position and foot Jacobian, base frame :91-92,124-126
//   kin_leg           pos_feet, pos_base_feet, base_pos_base_feet,
//                     base_pos_base_thighs, the leg's block of Jv_feet,
//                     base_vel_base_feet                                         :97-108,117-184
//
// Both shipped robots have the leg hip (revolute x) -> thigh (revolute y) -> calf
// (revolute y) -> foot (fixed) with zero joint rpy (a1.urdf:211-310, aliengo.urdf:253-358),
// so the chain is a closed form in three sine / cosine pairs.  Everything is float64 on the
// caller's float32 inputs; FP contraction is off so the host build and the device build
// round alike.
#pragma once
#include <math.h>

#include "mpcqp_swing_leg.h"   // swing_mat3, swing_mat3t

// per-robot geometry record (doubles): hip joint at (+-hip_x, +-hip_y, 0) in the trunk,
// thigh joint at (0, +-thigh_y, 0) in the hip, calf joint at (0, 0, -l_thigh) in the thigh,
// foot at (0, 0, -l_calf) in the calf
constexpr int KIN_HIP_X = 0, KIN_HIP_Y = 1, KIN_THIGH_Y = 2, KIN_L_THIGH = 3, KIN_L_CALF = 4, KIN_STRIDE = 8;

// Rotation of a quaternion (w, x, y, z) as Pinocchio's free-flyer joint forms it: Eigen's
// Quaternion::toRotationMatrix, on the quaternion as given (no normalisation).  R row-major.
__host__ __device__ inline void kin_quat2matrix(double w, double x, double y, double z, double* R) {
#pragma clang fp contract(off)
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0 - (tyy + tzz);
  R[1] = txy - twz;
  R[2] = txz + twy;
  R[3] = txy + twz;
  R[4] = 1.0 - (txx + tzz);
  R[5] = tyz - twx;
  R[6] = txz - twy;
  R[7] = tyz + twx;
  R[8] = 1.0 - (txx + tyy);
}

// One leg's chain in the base frame.  leg: FL, FR, RL, RR (x sign + + - -, y sign + - + -);
// q: hip, thigh, calf angle.  p = foot, pth = thigh joint, Jb = d p / d q row-major 3x3.
__host__ __device__ inline void kin_leg_chain(const double* geom, int leg, const double* q, double* p, double* pth,
                                              double* Jb) {
#pragma clang fp contract(off)
  const double sx = leg < 2 ? 1.0 : -1.0, sy = (leg & 1) ? -1.0 : 1.0;
  const double hx = sx * geom[KIN_HIP_X], hy = sy * geom[KIN_HIP_Y], d = sy * geom[KIN_THIGH_Y];
  const double l1 = geom[KIN_L_THIGH], l2 = geom[KIN_L_CALF];
  const double s1 = sin(q[0]), c1 = cos(q[0]);
  const double s2 = sin(q[1]), c2 = cos(q[1]);
  const double q23 = q[1] + q[2];
  const double s23 = sin(q23), c23 = cos(q23);
  // the foot in the thigh joint's frame before the hip rotation: (ux, 0, uz)
  const double ux = -(l1 * s2) - l2 * s23;
  const double uz = -(l1 * c2) - l2 * c23;
  p[0] = hx + ux;
  p[1] = (hy + d * c1) - uz * s1;
  p[2] = d * s1 + uz * c1;
  pth[0] = hx;
  pth[1] = hy + d * c1;
  pth[2] = d * s1;
  // d ux / d q2 = uz, d uz / d q2 = -ux; d ux / d q3 = -l2 c23, d uz / d q3 = l2 s23
  const double a3 = -(l2 * c23), b3 = l2 * s23;
  Jb[0] = 0.0;
  Jb[1] = uz;
  Jb[2] = a3;
  Jb[3] = -(d * s1) - uz * c1;
  Jb[4] = ux * s1;
  Jb[5] = -(b3 * s1);
  Jb[6] = d * c1 - uz * s1;
  Jb[7] = -(ux * c1);
  Jb[8] = b3 * c1;
}

// Every per-leg quantity RobotData.update leaves behind (robot_data.py:97-108).  Rq is
// kin_quat2matrix of the base quaternion, Rb the float32 R_base (quat2matrix, :75) widened.
//   pos_feet       pos + Rq p                                   :99,135-142  (world)
//   feet           Rq p                                         :101,144-149 (pos_base_feet)
//   foot_pos_base  Rb^T (Rq p)                                  :103,151-156
//   thigh          Rb^T (Rq pth)                                :108,178-184
//   jac            Rq Jb                                        :117-133, columns 6+3 leg .. of Jv_feet
//   foot_vel_base  Rb^T (Rq (v + w x p + Jb qd) - v)            :158-167
// The free-flyer columns of Pinocchio's LOCAL_WORLD_ALIGNED Jacobian are Rq and -Rq [p]x:
// they expect the base twist in the base frame, and the reference multiplies them by the
// world-frame lin_vel_base / ang_vel_base.  That is reproduced as it stands (DESIGN.md,
// deviations).
__host__ __device__ inline void kin_leg(const double* geom, int leg, const double* q, const double* qd,
                                        const double* Rq, const double* Rb, const double* pos, const double* v,
                                        const double* w, double* feet, double* thigh, double* pos_feet,
                                        double* foot_pos_base, double* foot_vel_base, double* jac) {
#pragma clang fp contract(off)
  double p[3], pth[3], Jb[9], wth[3], u[3], Ru[3];
  kin_leg_chain(geom, leg, q, p, pth, Jb);
  swing_mat3(Rq, p, feet);
  for (int k = 0; k < 3; ++k) pos_feet[k] = pos[k] + feet[k];
  swing_mat3t(Rb, feet, foot_pos_base);
  swing_mat3(Rq, pth, wth);
  swing_mat3t(Rb, wth, thigh);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) jac[3 * r + c] = Rq[3 * r] * Jb[c] + Rq[3 * r + 1] * Jb[3 + c] + Rq[3 * r + 2] * Jb[6 + c];
  swing_mat3(Jb, qd, u);
  u[0] = (v[0] + (w[1] * p[2] - w[2] * p[1])) + u[0];
  u[1] = (v[1] + (w[2] * p[0] - w[0] * p[2])) + u[1];
  u[2] = (v[2] + (w[0] * p[1] - w[1] * p[0])) + u[2];
  swing_mat3(Rq, u, Ru);
  for (int k = 0; k < 3; ++k) Ru[k] -= v[k];
  swing_mat3t(Rb, Ru, foot_vel_base);
}

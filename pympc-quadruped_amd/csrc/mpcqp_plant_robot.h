// mpcqp_plant_robot.h -- per-robot algebra of the rigid-body plant (mpcqp_plant.h), host- and
// device-callable so tests/ can check it on the CPU against tests/plant_ref.py.
//
// The model is the one the MPC assumes, with the nonlinear rotation kept and the contact decided
// by the ground: a single rigid body (mass, body-frame inertia) on four massless legs with point
// feet of mass foot_mass.  The reference has no such component: its scripts hand the torques to
// a simulator (gym.simulate, sim.step()).
//
//   plant_leg_ik       foot in the base frame -> (hip, thigh, calf), the inverse of kin_leg_chain
//   plant_leg_substep  one leg over one substep: the force its torques put on the foot, the
//                      contact decision, the foot's motion, the force and moment on the body
//   plant_body_substep the body over one substep from the four legs' force and moment
//   plant_leg_output   joint angles and rates of one leg from the record
//   plant_robot_step   the four legs and the body strung together for one robot (the host
//                      build; mpcqp_plant_kernel strings the same functions together with one
//                      lane per leg)
//   plant_robot_reset  a record from a pose (the host build and mpcqp_plant_reset's kernel)
//
// What it leaves out: leg mass and joint limits, sliding (a foot in contact is pinned; a
// reaction outside the friction cone is scaled back onto it and the foot stays where it is),
// restitution (a landing foot stops dead), steps and stairs (one plane per robot).
// Everything is float64; FP contraction is off so the host build and the device build round
// alike.
#pragma once
#include <math.h>

#include "mpcqp_kin_leg.h"

// the record: PLANT_STRIDE float64 words per robot
constexpr int PLANT_POS = 0, PLANT_QUAT = 3, PLANT_VEL = 7, PLANT_OMEGA = 10, PLANT_FEET = 13, PLANT_FVEL = 25,
              PLANT_CONTACT = 37, PLANT_FLAGS = 41, PLANT_TICK = 42, PLANT_WORDS = 43, PLANT_STRIDE = 48;
constexpr int PLANT_STATUS_OK = 0, PLANT_STATUS_NONFINITE = 4;
// The knee clamp: cos(calf) is held in [-1 + eps, 1 - eps], applied to 1 - cos and 1 + cos as the
// law of cosines gives them without cancellation (plant_leg_ik), so that eps can be far below a
// double's spacing at 1.  2^-90: sin(calf) >= sqrt(2 eps) = 4e-14 keeps J_b invertible (its
// inverse stays below 1e14), and a leg folded onto its thigh joint or fully stretched still
// returns its foot within sqrt(2 l1 l2 eps) = 8e-15 m of the target, under the 1e-13 of the round trip.
constexpr double PLANT_IK_EPS = 8.077935669463161e-28;   // 2^-90
constexpr double PLANT_IK_TINY = 1e-30;                  // floor of y^2 + z^2 - d^2

struct PlantParams {
  double dt_control, gravity, foot_mass, ground_z, contact_tol;
  int substeps;
};

// What a robot's four legs share and no substep changes: mass, friction, the body-frame inertia
// and its inverse, the ground plane n . p = d.
struct PlantConst {
  double m, mu, I[9], Ii[9], n[3], d;
};

// Cofactor inverse of a row-major 3x3; returns the determinant (inv is M^-1 only where it is
// finite and non-zero).
__host__ __device__ inline double plant_inv3(const double* M, double* inv) {
#pragma clang fp contract(off)
  const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7], i = M[8];
  const double c00 = e * i - f * h, c01 = c * h - b * i, c02 = b * f - c * e;
  const double c10 = f * g - d * i, c11 = a * i - c * g, c12 = c * d - a * f;
  const double c20 = d * h - e * g, c21 = b * g - a * h, c22 = a * e - b * d;
  const double det = (a * c00 + b * c10) + c * c20;
  const double r = 1.0 / det;
  inv[0] = c00 * r;
  inv[1] = c01 * r;
  inv[2] = c02 * r;
  inv[3] = c10 * r;
  inv[4] = c11 * r;
  inv[5] = c12 * r;
  inv[6] = c20 * r;
  inv[7] = c21 * r;
  inv[8] = c22 * r;
  return det;
}

__host__ __device__ inline void plant_cross(const double* a, const double* b, double* c) {
#pragma clang fp contract(off)
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

__host__ __device__ inline double plant_dot(const double* a, const double* b) {
#pragma clang fp contract(off)
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// The robot's constants from its float32 record (mass, ixx, ixy, ixz, iyy, iyz, izz, mu; the
// normal of the record is not read).  Returns whether the robot can be advanced: finite values,
// mass > 0, an invertible inertia.
__host__ __device__ inline bool plant_const_load(const float* rec, PlantConst* C) {
#pragma clang fp contract(off)
  bool ok = true;
  for (int k = 0; k < 8; ++k) ok = ok && isfinite(rec[k]);
  C->m = (double)rec[0];
  C->mu = (double)rec[7];
  const double xx = (double)rec[1], xy = (double)rec[2], xz = (double)rec[3], yy = (double)rec[4], yz = (double)rec[5],
               zz = (double)rec[6];
  C->I[0] = xx;
  C->I[1] = xy;
  C->I[2] = xz;
  C->I[3] = xy;
  C->I[4] = yy;
  C->I[5] = yz;
  C->I[6] = xz;
  C->I[7] = yz;
  C->I[8] = zz;
  const double det = plant_inv3(C->I, C->Ii);
  return ok && C->m > 0.0 && fabs(det) > 0.0;
}

// The robot's ground n . p = d from its plane (n, d), NULL for level ground at ground_z.
// Returns whether it is finite.
__host__ __device__ inline bool plant_const_plane(const float* plane, double ground_z, PlantConst* C) {
  if (plane == nullptr) {
    C->n[0] = 0.0;
    C->n[1] = 0.0;
    C->n[2] = 1.0;
    C->d = ground_z;
    return true;
  }
  bool ok = true;
  for (int k = 0; k < 4; ++k) ok = ok && isfinite(plane[k]);
  for (int k = 0; k < 3; ++k) C->n[k] = (double)plane[k];
  C->d = (double)plane[3];
  return ok;
}

// Foot p in the base frame -> q = (hip, thigh, calf) with the knee bent back (calf < 0, the
// branch of the reference's 0.8 / -1.6 crouch).  Returns whether a clamp bit: the foot inside
// the hip's cylinder (y^2 + z^2 < d^2) or the knee at its clamp (beyond reach, or folded onto
// the thigh joint).
__host__ __device__ inline bool plant_leg_ik(const double* geom, int leg, const double* p, double* q) {
#pragma clang fp contract(off)
  const double sx = leg < 2 ? 1.0 : -1.0, sy = (leg & 1) ? -1.0 : 1.0;
  const double hx = sx * geom[KIN_HIP_X], hy = sy * geom[KIN_HIP_Y], d = sy * geom[KIN_THIGH_Y];
  const double l1 = geom[KIN_L_THIGH], l2 = geom[KIN_L_CALF];
  const double x = p[0] - hx, y = p[1] - hy, z = p[2];
  const double r2 = (y * y + z * z) - d * d;
  const bool low = !(r2 >= PLANT_IK_TINY);
  const double uz = -sqrt(low ? PLANT_IK_TINY : r2);
  q[0] = atan2(z, y) - atan2(uz, d);
  // a = 2 l1 l2 (1 - c3) and b = 2 l1 l2 (1 + c3) for c3 = (x^2 + uz^2 - l1^2 - l2^2) / (2 l1 l2):
  // q3 = -acos(c3) = -2 atan2(sqrt(a), sqrt(b)), exact to rounding at both ends of the range
  const double L2 = x * x + uz * uz;
  const double k2 = (2.0 * l1) * l2, lim = k2 * PLANT_IK_EPS;
  double a = (l1 + l2) * (l1 + l2) - L2, b = L2 - (l1 - l2) * (l1 - l2);
  // a + b = 4 l1 l2: a clamped end takes the other with it, as the clamp of c3 does
  const bool hi = !(a >= lim), lo = !hi && !(b >= lim);
  a = hi ? lim : lo ? 2.0 * k2 - lim : a;
  b = hi ? 2.0 * k2 - lim : lo ? lim : b;
  const double sa = sqrt(a), sb = sqrt(b), sum = a + b;
  const double inv = sum > 0.0 ? 1.0 / sum : 0.0;
  const double s3 = -(((2.0 * sa) * sb) * inv), c3 = (b - a) * inv;   // sin, cos of q3
  q[2] = -(2.0 * atan2(sa, sb));
  q[1] = atan2(-x, -uz) - atan2(l2 * s3, l1 + l2 * c3);
  return low || hi || lo;
}

// r = p_f - pos, q = ik(Rq^T r) and J_b(q)^-1.  Returns the clamp bit.
__host__ __device__ inline bool plant_leg_state(const double* geom, int leg, const double* Rq, const double* pos,
                                                const double* pf, double* r, double* q, double* Ji) {
#pragma clang fp contract(off)
  double pb[3], p[3], pth[3], Jb[9];
  for (int k = 0; k < 3; ++k) r[k] = pf[k] - pos[k];
  swing_mat3t(Rq, r, pb);
  const bool cl = plant_leg_ik(geom, leg, pb, q);
  kin_leg_chain(geom, leg, q, p, pth, Jb);
  plant_inv3(Jb, Ji);
  return cl;
}

// One leg over one substep of length h.  g = J^-T tau with J = Rq J_b, that is Rq J_b^-T tau
// (Rq is orthogonal), is the force the leg puts on its foot.
//   a foot in contact: the ground reaction is f = -g.  n . f <= 0 releases it: it goes on as a
//     free foot in this substep, from rest (it was pinned in the world; started at the velocity
//     of its body point it would re-land every substep under a descending hip).  Otherwise
//     the tangential part is scaled back onto the cone |f_t| <= mu n . f and the foot stays
//     pinned (no sliding); the body receives f at the foot.
//   a free foot: a point mass foot_mass under g plus gravity, semi-implicit Euler; the body
//     receives -g at the foot.  Below the plane and moving into it afterwards, it is projected
//     onto the plane, stopped and marked in contact.
// pf, vf, *contact are the leg's record entries (in/out); F, M the force on the body and its
// moment about the centre of mass; r and Ji are plant_leg_state's.
__host__ __device__ inline void plant_leg_force(const PlantParams& P, const PlantConst& C, const double* Rq,
                                                const double* r, const double* Ji, const double* tau, double h,
                                                double* pf, double* vf, bool* contact, double* F, double* M) {
#pragma clang fp contract(off)
  double gb[3], g[3];
  swing_mat3t(Ji, tau, gb);
  swing_mat3(Rq, gb, g);
  const double f[3] = {-g[0], -g[1], -g[2]};
  const double fn = plant_dot(C.n, f);
  const bool pinned = *contact && fn > 0.0;
  if (pinned) {
    double ft[3];
    for (int k = 0; k < 3; ++k) ft[k] = f[k] - fn * C.n[k];
    const double ftn = sqrt(plant_dot(ft, ft));
    const double cap = C.mu * fn;
    const double scale = ftn > cap ? cap / ftn : 1.0;
    for (int k = 0; k < 3; ++k) {
      F[k] = fn * C.n[k] + scale * ft[k];
      vf[k] = 0.0;
    }
  } else {
    double v0[3], pn[3], vn[3];
    for (int k = 0; k < 3; ++k) v0[k] = *contact ? 0.0 : vf[k];
    const double gz[3] = {0.0, 0.0, -P.gravity};
    for (int k = 0; k < 3; ++k) {
      const double a = g[k] / P.foot_mass + gz[k];
      vn[k] = v0[k] + h * a;
      pn[k] = pf[k] + h * vn[k];
    }
    const double s = plant_dot(C.n, pn) - C.d;
    const double vnn = plant_dot(C.n, vn);
    const bool land = s <= 0.0 && vnn < 0.0;
    for (int k = 0; k < 3; ++k) {
      pf[k] = land ? pn[k] - s * C.n[k] : pn[k];
      vf[k] = land ? 0.0 : vn[k];
      F[k] = -g[k];
    }
    *contact = land;
  }
  plant_cross(r, F, M);
}

// plant_leg_state and plant_leg_force of one leg; returns the IK's clamp bit.
__host__ __device__ inline bool plant_leg_substep(const PlantParams& P, const PlantConst& C, int leg, const double* geom,
                                                  const double* Rq, const double* pos, const double* tau, double h,
                                                  double* pf, double* vf, bool* contact, double* F, double* M) {
  double r[3], q[3], Ji[9];
  const bool cl = plant_leg_state(geom, leg, Rq, pos, pf, r, q, Ji);
  plant_leg_force(P, C, Rq, r, Ji, tau, h, pf, vf, contact, F, M);
  return cl;
}

// exp(th) (x) quat, normalised; quat (w, x, y, z), th a world-frame rotation vector.
__host__ __device__ inline void plant_quat_step(const double* th, double* quat) {
#pragma clang fp contract(off)
  const double t2 = plant_dot(th, th);
  const double t = sqrt(t2);
  const bool small = t < 1e-6;
  const double s = small ? 0.5 - t2 / 48.0 : sin(0.5 * t) / t;
  const double c = small ? 1.0 - t2 / 8.0 : cos(0.5 * t);
  const double ax = s * th[0], ay = s * th[1], az = s * th[2];
  const double w = quat[0], x = quat[1], y = quat[2], z = quat[3];
  const double nw = ((c * w - ax * x) - ay * y) - az * z;
  const double nx = ((c * x + ax * w) + ay * z) - az * y;
  const double ny = ((c * y - ax * z) + ay * w) + az * x;
  const double nz = ((c * z + ax * y) - ay * x) + az * w;
  const double nn = sqrt(((nw * nw + nx * nx) + ny * ny) + nz * nz);
  quat[0] = nw / nn;
  quat[1] = nx / nn;
  quat[2] = ny / nn;
  quat[3] = nz / nn;
}

// y = Rq A Rq^T x for a body-frame matrix A
__host__ __device__ inline void plant_world_apply(const double* Rq, const double* A, const double* x, double* y) {
#pragma clang fp contract(off)
  double xb[3], yb[3];
  swing_mat3t(Rq, x, xb);
  swing_mat3(A, xb, yb);
  swing_mat3(Rq, yb, y);
}

// The body over one substep from SF = sum F and SM = sum r x F:
//   v += h (SF / m + gravity),  pos += h v
//   L = I_w w,  w* = w + h I_w^-1 (SM - w x L),  quat <- exp(h w*) (x) quat, normalised,
//   w <- I_w'^-1 (L + h SM) on the new attitude
// with I_w = Rq I Rq^T: the attitude turns by the explicit Euler rate, and the angular momentum,
// not the rate, is what is carried through the turn, so that free flight conserves I_w w to
// rounding.  Rq is replaced by the new attitude's matrix; spec = SF / m, the accelerometer's
// specific force in the world frame.
__host__ __device__ inline void plant_body_substep(const PlantParams& P, const PlantConst& C, double h, const double* SF,
                                                   const double* SM, double* pos, double* quat, double* v, double* w,
                                                   double* Rq, double* spec) {
#pragma clang fp contract(off)
  const double gz[3] = {0.0, 0.0, -P.gravity};
  for (int k = 0; k < 3; ++k) {
    spec[k] = SF[k] / C.m;
    v[k] = v[k] + h * (spec[k] + gz[k]);
  }
  double L[3], wxL[3], e[3], de[3], th[3], Ln[3];
  plant_world_apply(Rq, C.I, w, L);
  plant_cross(w, L, wxL);
  for (int k = 0; k < 3; ++k) e[k] = SM[k] - wxL[k];
  plant_world_apply(Rq, C.Ii, e, de);
  for (int k = 0; k < 3; ++k) {
    th[k] = h * (w[k] + h * de[k]);
    pos[k] = pos[k] + h * v[k];
    Ln[k] = L[k] + h * SM[k];
  }
  plant_quat_step(th, quat);
  kin_quat2matrix(quat[0], quat[1], quat[2], quat[3], Rq);
  plant_world_apply(Rq, C.Ii, Ln, w);
}

// qdot = J_b^-1 Rq^T (v_f - v - w x r) of one leg; r and Ji are plant_leg_state's.
__host__ __device__ inline void plant_leg_rate(const double* Rq, const double* r, const double* Ji, const double* v,
                                               const double* w, const double* vf, double* qd) {
#pragma clang fp contract(off)
  double wxr[3], rel[3], rb[3];
  plant_cross(w, r, wxr);
  for (int k = 0; k < 3; ++k) rel[k] = (vf[k] - v[k]) - wxr[k];
  swing_mat3t(Rq, rel, rb);
  swing_mat3(Ji, rb, qd);
}

// q = ik(Rq^T (p_f - pos)) and qdot of one leg.  Returns the IK's clamp bit.
__host__ __device__ inline bool plant_leg_output(const double* geom, int leg, const double* Rq, const double* pos,
                                                 const double* v, const double* w, const double* pf, const double* vf,
                                                 double* q, double* qd) {
  double r[3], Ji[9];
  const bool cl = plant_leg_state(geom, leg, Rq, pos, pf, r, q, Ji);
  plant_leg_rate(Rq, r, Ji, v, w, vf, qd);
  return cl;
}

// Whether every value of a[0..n) is finite.
__host__ __device__ inline bool plant_all_finite(const double* a, int n) {
  bool ok = true;
  for (int k = 0; k < n; ++k) ok = ok && isfinite(a[k]);
  return ok;
}

// The outputs of one robot from its record and the specific force: root_states [13] (pos, quat
// x y z w, lin_vel, ang_vel), dof_states [12][2], gyro = Rq^T w, accel = Rq^T spec (at rest on
// level ground (0, 0, +g)), touch [4]; each nullable.  Returns the clamp bits of the four legs;
// *finite is cleared where a float32 output is not finite.
__host__ __device__ inline int plant_robot_outputs(const double* rec, const double* geom, const double* spec, float* root,
                                                   float* dofs, float* gyro, float* accel, float* touch, bool* finite) {
#pragma clang fp contract(off)
  double Rq[9], q[3], qd[3], gb[3], ab[3];
  const double* quat = rec + PLANT_QUAT;
  kin_quat2matrix(quat[0], quat[1], quat[2], quat[3], Rq);
  int bits = 0;
  bool ok = true;
  for (int leg = 0; leg < 4; ++leg) {
    if (plant_leg_output(geom, leg, Rq, rec + PLANT_POS, rec + PLANT_VEL, rec + PLANT_OMEGA, rec + PLANT_FEET + 3 * leg,
                         rec + PLANT_FVEL + 3 * leg, q, qd))
      bits |= 1 << leg;
    for (int k = 0; k < 3; ++k) {
      const float a = (float)q[k], b = (float)qd[k];
      ok = ok && isfinite(a) && isfinite(b);
      if (dofs != nullptr) {
        dofs[2 * (3 * leg + k)] = a;
        dofs[2 * (3 * leg + k) + 1] = b;
      }
    }
    if (touch != nullptr) touch[leg] = rec[PLANT_CONTACT + leg] != 0.0 ? 1.f : 0.f;
  }
  swing_mat3t(Rq, rec + PLANT_OMEGA, gb);
  swing_mat3t(Rq, spec, ab);
  for (int k = 0; k < 3; ++k) {
    ok = ok && isfinite((float)gb[k]) && isfinite((float)ab[k]);
    if (gyro != nullptr) gyro[k] = (float)gb[k];
    if (accel != nullptr) accel[k] = (float)ab[k];
  }
  if (root != nullptr) {
    for (int k = 0; k < 3; ++k) {
      root[k] = (float)rec[PLANT_POS + k];
      root[3 + k] = (float)quat[1 + k];
      root[7 + k] = (float)rec[PLANT_VEL + k];
      root[10 + k] = (float)rec[PLANT_OMEGA + k];
    }
    root[6] = (float)quat[0];
  }
  for (int k = 0; k < 13; ++k) ok = ok && isfinite((float)rec[k]);
  if (!ok) *finite = false;
  return bits;
}

// One control iteration of one robot: P.substeps substeps of dt_control / substeps on rec
// [PLANT_STRIDE] (in/out), then the outputs.  A robot with a non-finite torque, a non-finite or
// non-invertible record (mass <= 0, a singular inertia, a zero quaternion) or a non-finite result
// is refused: PLANT_STATUS_NONFINITE, its record untouched and its outputs rewritten from the
// untouched record (with the specific force of a robot at rest).  The four legs' forces meet as
// (F0 + F1) + (F2 + F3), the order of the kernel's two quad exchanges.
__host__ __device__ inline int plant_robot_step(const PlantParams& P, double* rec, const float* tau, const float* robot,
                                                const double* geom, const float* plane, float* root, float* dofs,
                                                float* gyro, float* accel, float* touch) {
#pragma clang fp contract(off)
  PlantConst C;
  bool ok = plant_const_load(robot, &C);
  ok = plant_const_plane(plane, P.ground_z, &C) && ok;
  double w[PLANT_STRIDE], tq[12], spec[3] = {0.0, 0.0, P.gravity};
  for (int k = 0; k < PLANT_STRIDE; ++k) w[k] = rec[k];
  ok = ok && plant_all_finite(rec, PLANT_WORDS) && plant_all_finite(geom, 5);
  for (int k = 0; k < 12; ++k) {
    tq[k] = (double)tau[k];
    ok = ok && isfinite(tau[k]);
  }
  const double* qt = rec + PLANT_QUAT;
  ok = ok && ((qt[0] * qt[0] + qt[1] * qt[1]) + qt[2] * qt[2]) + qt[3] * qt[3] > 0.0;
  if (ok) {
    const double h = P.dt_control / (double)P.substeps;
    double Rq[9];
    kin_quat2matrix(w[PLANT_QUAT], w[PLANT_QUAT + 1], w[PLANT_QUAT + 2], w[PLANT_QUAT + 3], Rq);
    int bits = 0;
    for (int s = 0; s < P.substeps; ++s) {
      double F[4][3], M[4][3], SF[3], SM[3];
      for (int leg = 0; leg < 4; ++leg) {
        bool ct = w[PLANT_CONTACT + leg] != 0.0;
        if (plant_leg_substep(P, C, leg, geom, Rq, w + PLANT_POS, tq + 3 * leg, h, w + PLANT_FEET + 3 * leg,
                              w + PLANT_FVEL + 3 * leg, &ct, F[leg], M[leg]))
          bits |= 1 << leg;
        w[PLANT_CONTACT + leg] = ct ? 1.0 : 0.0;
      }
      for (int k = 0; k < 3; ++k) {
        SF[k] = (F[0][k] + F[1][k]) + (F[2][k] + F[3][k]);
        SM[k] = (M[0][k] + M[1][k]) + (M[2][k] + M[3][k]);
      }
      plant_body_substep(P, C, h, SF, SM, w + PLANT_POS, w + PLANT_QUAT, w + PLANT_VEL, w + PLANT_OMEGA, Rq, spec);
    }
    bits |= plant_robot_outputs(w, geom, spec, root, dofs, gyro, accel, touch, &ok);
    w[PLANT_FLAGS] = (double)bits;
    w[PLANT_TICK] = rec[PLANT_TICK] + 1.0;
    ok = ok && plant_all_finite(w, PLANT_WORDS);
  }
  if (!ok) {
    const double rest[3] = {0.0, 0.0, P.gravity};
    bool unused = true;
    plant_robot_outputs(rec, geom, rest, root, dofs, gyro, accel, touch, &unused);
    return PLANT_STATUS_NONFINITE;
  }
  for (int k = 0; k < PLANT_WORDS; ++k) rec[k] = w[k];
  return PLANT_STATUS_OK;
}

// A record from a pose in the loop's own tensors: feet by forward kinematics, foot velocities
// zero, contact where n . p_f - d <= contact_tol; flag word and tick count zero.
__host__ __device__ inline void plant_robot_reset(const PlantParams& P, const float* root, const float* dofs,
                                                  const double* geom, const float* plane, double* rec) {
#pragma clang fp contract(off)
  double n[3] = {0.0, 0.0, 1.0}, d = P.ground_z, Rq[9];
  if (plane != nullptr) {
    for (int k = 0; k < 3; ++k) n[k] = (double)plane[k];
    d = (double)plane[3];
  }
  for (int k = 0; k < PLANT_STRIDE; ++k) rec[k] = 0.0;
  for (int k = 0; k < 3; ++k) {
    rec[PLANT_POS + k] = (double)root[k];
    rec[PLANT_QUAT + 1 + k] = (double)root[3 + k];
    rec[PLANT_VEL + k] = (double)root[7 + k];
    rec[PLANT_OMEGA + k] = (double)root[10 + k];
  }
  rec[PLANT_QUAT] = (double)root[6];
  kin_quat2matrix(rec[PLANT_QUAT], rec[PLANT_QUAT + 1], rec[PLANT_QUAT + 2], rec[PLANT_QUAT + 3], Rq);
  for (int leg = 0; leg < 4; ++leg) {
    double q[3], p[3], pth[3], Jb[9], pw[3];
    for (int k = 0; k < 3; ++k) q[k] = (double)dofs[2 * (3 * leg + k)];
    kin_leg_chain(geom, leg, q, p, pth, Jb);
    swing_mat3(Rq, p, pw);
    for (int k = 0; k < 3; ++k) {
      pw[k] = rec[PLANT_POS + k] + pw[k];
      rec[PLANT_FEET + 3 * leg + k] = pw[k];
    }
    rec[PLANT_CONTACT + leg] = plant_dot(n, pw) - d <= P.contact_tol ? 1.0 : 0.0;
  }
}

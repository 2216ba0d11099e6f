// mpcqp_swing_leg.h -- per-leg algebra of the swing half of the leg controller
// (mpcqp_swing.h), host- and device-callable so tests/ can check it on the CPU.
//
//   swing_decide    Gait.set_iteration / get_swing_state       gait.py:76-79,102-121
//   swing_times     Gait.swing_time / stance_time              gait.py:40-41,68-74
//   swing_foothold  set_foot_placement                         swing_foot_trajectory_generator.py:84-129
//   swing_curve     generate_swing_foot_trajectory             swing_foot_trajectory_generator.py:38-67
//   swing_to_base   compute_traj_swingfoot (frame change)      swing_foot_trajectory_generator.py:69-82
//   swing_pd        LegController.update, swing branch         leg_controller.py:78-86
//
// Everything is float64 on the caller's float32 inputs; FP contraction is off so the
// host build and the device build round alike.
#pragma once
#include <math.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

// per-leg slots of swing_mem (doubles): armed = 1 while a swing is under way (the
// generator's is_first_swing == False), the remaining swing time, the latched lift-off
// position and the foothold, both in the world frame
constexpr int SW_ARMED = 0, SW_REMAIN = 1, SW_INIT = 2, SW_FINAL = 5, SW_LEG_STRIDE = 8;

constexpr int SWING_STANCE = 0, SWING_ACTIVE = 1, SWING_FINISHED = 2;

// The integers swing_decide decides on: *nsw control iterations per swing, *c = tick mod the
// gait's span and *cs = c shifted by the leg's swing offset; the leg swings for
// 1 <= cs <= nsw.  False for a leg that never swings (nsw <= 0) or a malformed record.
// Shared with the contact trust of mpcqp_attitude_robot.h, so the two cannot disagree.
__host__ __device__ inline bool swing_counts(int tick, int ibm, int period, int off, int dur, long long* cs,
                                             long long* nsw, long long* c = nullptr) {
  if (period <= 0 || ibm <= 0) return false;
  const long long span = (long long)ibm * period;
  *nsw = (long long)(period - dur) * ibm;
  if (*nsw <= 0) return false;
  long long cc = (long long)tick % span;
  if (cc < 0) cc += span;
  long long s = (cc - (long long)(off + dur) * ibm) % span;
  if (s < 0) s += span;
  *cs = s;
  if (c != nullptr) *c = cc;
  return true;
}

// The leg's swing state at control iteration `tick` (gait.py:76-79,102-121).  The
// decisions -- stance / swing (swing_state > 0) and swing finished (swing_state >= 1) --
// are taken on integers: with c = tick mod (ibm * period) and cs = c shifted by the leg's
// swing offset (off + dur) * ibm, the leg swings for 1 <= cs <= (period - dur) * ibm and
// finishes at the last of them (the reference's float32 phase hits those boundaries
// exactly for every Gait member).  A swing offset past the period wraps per leg
// (gait.py:104-106 subtracts 1 from all four legs: DESIGN.md, deviations).  A leg whose
// stance fills the period never swings (the reference's 0 / 0 there: DESIGN.md), nor does
// a malformed record (period <= 0, ibm <= 0).  *value = swing_state, the reference's
// float division on its float32 phase; it is cs / nsw to the rounding of that phase for
// every offset, negative ones and ones past the period included.
__host__ __device__ inline int swing_decide(int tick, int ibm, int period, int off, int dur, double* value) {
#pragma clang fp contract(off)
  *value = 0.0;
  long long c, cs, nsw;   // nsw: control iterations per swing
  if (!swing_counts(tick, ibm, period, off, dur, &cs, &nsw, &c)) return SWING_STANCE;
  if (cs == 0 || cs > nsw) return SWING_STANCE;
  const long long span = (long long)ibm * period;
  const float phase = (float)((double)c / (double)span);   // phase_state is a float32 array
  // the swing offset as a fraction of the period, brought into [0, 1] as the integers above bring
  // cs into [0, span): (1, 2] loses 1 as in the reference (an offset of exactly 1 stays), anything
  // further out -- a negative stance offset, one past twice the period -- its whole periods
  double so = (double)off / (double)period + (double)dur / (double)period;
  if (so > 1.0) so -= ceil(so) - 1.0;
  if (so < 0.0) so -= floor(so);
  const double sd = 1.0 - (double)dur / (double)period;
  double s = (double)phase - so;
  if (s < 0.0) s += 1.0;
  double v = s / sd;
  if (!(v > 0.0)) v = (double)cs / (double)nsw;   // a custom gait whose boundary is no float32 value
  *value = v;
  return cs == nsw ? SWING_FINISHED : SWING_ACTIVE;
}

// total swing / stance time of every leg: the first leg's duration (gait.py:40-41)
__host__ __device__ inline void swing_times(double dt_control, int ibm, int period, int dur0, double* t_swing,
                                            double* t_stance) {
#pragma clang fp contract(off)
  const double dt_mpc = dt_control * (double)ibm;
  *t_swing = dt_mpc * (double)(period - dur0);
  *t_stance = dt_mpc * (double)dur0;
}

// y = R x, R row-major 3x3
__host__ __device__ inline void swing_mat3(const double* R, const double* x, double* y) {
#pragma clang fp contract(off)
  for (int r = 0; r < 3; ++r) y[r] = R[3 * r] * x[0] + R[3 * r + 1] * x[1] + R[3 * r + 2] * x[2];
}

// y = R^T x
__host__ __device__ inline void swing_mat3t(const double* R, const double* x, double* y) {
#pragma clang fp contract(off)
  for (int r = 0; r < 3; ++r) y[r] = R[r] * x[0] + R[3 + r] * x[1] + R[6 + r] * x[2];
}

// The foothold of the current swing, world frame (swing_foot_trajectory_generator.py:
// 108-120): the yaw-corrected thigh position plus the commanded travel over the remaining
// swing, half a stance of base travel, the velocity-error term (`vel_gain`, 0.03 in the
// reference) and the two centrifugal terms; z = touchdown_z (-0.0255 in the reference).
__host__ __device__ inline void swing_foothold(const double* pos, const double* vel, const double* R,
                                               const double* vbody, double yaw_rate, const double* thigh,
                                               double remaining, double t_stance, double gravity, double vel_gain,
                                               double touchdown_z, double* fin) {
#pragma clang fp contract(off)
  const double theta = yaw_rate * 0.5 * t_stance;
  const double ct = cos(theta), st = sin(theta);
  double a[3], Ra[3], vdes[3];
  a[0] = (ct * thigh[0] - st * thigh[1]) + vbody[0] * remaining;
  a[1] = (st * thigh[0] + ct * thigh[1]) + vbody[1] * remaining;
  a[2] = thigh[2] + vbody[2] * remaining;
  swing_mat3(R, a, Ra);
  swing_mat3(R, vbody, vdes);
  for (int k = 0; k < 3; ++k)
    fin[k] = ((pos[k] + Ra[k]) + 0.5 * t_stance * vel[k]) + vel_gain * (vel[k] - vdes[k]);
  const double kc = 0.5 * pos[2] / gravity;
  fin[0] += kc * (vel[1] * yaw_rate);
  fin[1] += kc * (-vel[0] * yaw_rate);
  fin[2] = touchdown_z;
}

// The cubic Hermite through init, mid and final with zero velocity at the breaks
// [0, T / 2, T] (:38-67), mid = (init + final) / 2 with mid.z = swing_height (a world z).
// The reference stores the breaks as float32; `cur` is clamped to them as Drake's
// value() clamps, and the velocity is the derivative at the clamped time.
__host__ __device__ inline void swing_curve(double t_swing, double cur, const double* init, const double* fin,
                                            double swing_height, double* p, double* v) {
#pragma clang fp contract(off)
  const double t1 = (double)(float)(t_swing / 2.0), t2 = (double)(float)t_swing;
  double t = cur;
  if (t < 0.0) t = 0.0;
  if (t > t2) t = t2;
  const bool second = t >= t1;
  const double h = second ? t2 - t1 : t1;
  const double x = second ? t - t1 : t;
  const double u = h > 0.0 ? x / h : 0.0;
  const double blend = (3.0 - 2.0 * u) * u * u;          // 3 u^2 - 2 u^3
  const double rate = h > 0.0 ? 6.0 * u * (1.0 - u) / h : 0.0;
  for (int k = 0; k < 3; ++k) {
    const double mid = k == 2 ? swing_height : (init[k] + fin[k]) / 2.0;
    const double a = second ? mid : init[k];
    const double d = second ? fin[k] - mid : mid - init[k];
    p[k] = a + d * blend;
    v[k] = d * rate;
  }
}

// world -> base frame: R^T (p - pos_base), R^T (v - vel_base) (:78-80)
__host__ __device__ inline void swing_to_base(const double* R, const double* pos, const double* vel, const double* p,
                                              const double* v, double* pb, double* vb) {
#pragma clang fp contract(off)
  double dp[3], dv[3];
  for (int k = 0; k < 3; ++k) {
    dp[k] = p[k] - pos[k];
    dv[k] = v[k] - vel[k];
  }
  swing_mat3t(R, dp, pb);
  swing_mat3t(R, dv, vb);
}

// tau_leg = Jv^T [Kp (R p_des - R p_foot) + Kd (R v_des - R v_foot)] (leg_controller.py:
// 78-86), J the leg's row-major 3x3 block of its foot Jacobian
__host__ __device__ inline void swing_pd(const double* R, const double* Kp, const double* Kd, const double* J,
                                         const double* p_des, const double* v_des, const double* p_foot,
                                         const double* v_foot, double* tau) {
#pragma clang fp contract(off)
  double a[3], b[3], ep[3], ev[3], kp[3], kd[3], e[3];
  swing_mat3(R, p_des, a);
  swing_mat3(R, p_foot, b);
  for (int k = 0; k < 3; ++k) ep[k] = a[k] - b[k];
  swing_mat3(R, v_des, a);
  swing_mat3(R, v_foot, b);
  for (int k = 0; k < 3; ++k) ev[k] = a[k] - b[k];
  swing_mat3(Kp, ep, kp);
  swing_mat3(Kd, ev, kd);
  for (int k = 0; k < 3; ++k) e[k] = kp[k] + kd[k];
  swing_mat3t(J, e, tau);
}

// The ground's height at (x, y): z on the plane n . p = d, g = (n_x, n_y, n_z, d), n_z > 0
__host__ __device__ inline double swing_ground(const double* g, double x, double y) {
#pragma clang fp contract(off)
  return ((g[3] - g[0] * x) - g[1] * y) / g[2];
}

// One tick of one leg's generator for a leg in swing (isaacgym_a1.py:150-160): advance
// the foot-placement state machine in `mem` (SW_LEG_STRIDE doubles), then evaluate the
// curve and change frame.  `foot_world` = pos_feet[leg], latched on the first swing tick.
// `ground`: the robot's ground plane (n_x, n_y, n_z, d; mpcqp_set_ground), or NULL.  On a plane
// the foothold's z is touchdown_z above the ground at the foothold, and the apex swing_height
// above the mean of the ground at lift-off and at the foothold; a plane that is non-finite or
// has n_z <= 0 counts as none, and without one both are the world z the reference uses.
__host__ __device__ inline void swing_leg_step_ground(double* mem, bool finished, double dt_control, double t_swing,
                                                      double t_stance, const double* pos, const double* vel,
                                                      const double* R, const double* vbody, double yaw_rate,
                                                      const double* thigh, const double* foot_world, double gravity,
                                                      double vel_gain, double touchdown_z, double swing_height,
                                                      double* p_base, double* v_base, const double* ground) {
#pragma clang fp contract(off)
  const bool first = mem[SW_ARMED] == 0.0;
  const double remaining = first ? t_swing : mem[SW_REMAIN] - dt_control;
  mem[SW_REMAIN] = remaining;
  swing_foothold(pos, vel, R, vbody, yaw_rate, thigh, remaining, t_stance, gravity, vel_gain, touchdown_z,
                 mem + SW_FINAL);
  if (first)
    for (int k = 0; k < 3; ++k) mem[SW_INIT + k] = foot_world[k];
  mem[SW_ARMED] = finished ? 0.0 : 1.0;   // swing_state >= 1 re-arms the first-swing flag
  double apex = swing_height;
  if (ground != nullptr && isfinite(ground[0]) && isfinite(ground[1]) && isfinite(ground[2]) &&
      isfinite(ground[3]) && ground[2] > 0.0) {
    const double gf = swing_ground(ground, mem[SW_FINAL], mem[SW_FINAL + 1]);
    const double gi = swing_ground(ground, mem[SW_INIT], mem[SW_INIT + 1]);
    mem[SW_FINAL + 2] = touchdown_z + gf;
    apex = swing_height + (gi + gf) / 2.0;
  }
  double p[3], v[3];
  swing_curve(t_swing, t_swing - remaining, mem + SW_INIT, mem + SW_FINAL, apex, p, v);
  swing_to_base(R, pos, vel, p, v, p_base, v_base);
}

// the same on the flat ground of the reference
__host__ __device__ inline void swing_leg_step(double* mem, bool finished, double dt_control, double t_swing,
                                               double t_stance, const double* pos, const double* vel, const double* R,
                                               const double* vbody, double yaw_rate, const double* thigh,
                                               const double* foot_world, double gravity, double vel_gain,
                                               double touchdown_z, double swing_height, double* p_base,
                                               double* v_base) {
  swing_leg_step_ground(mem, finished, dt_control, t_swing, t_stance, pos, vel, R, vbody, yaw_rate, thigh,
                        foot_world, gravity, vel_gain, touchdown_z, swing_height, p_base, v_base, nullptr);
}

// mpcqp_swing.h -- the leg controller on the device: swing state, foot placement,
// swing trajectory and all 12 joint torques of every robot in one launch (included by
// mpcqp.hip inside its anonymous namespace, after mpcqp_plan.h).  For B robots x 4 legs
// it is the loop body of scripts/isaacgym_a1.py:137-162:
//
//   swing state     Gait.set_iteration / get_swing_state          gait.py:76-79,102-121
//   foot placement  SwingFootTrajectoryGenerator.set_foot_placement
//                                                     swing_foot_trajectory_generator.py:84-129
//   trajectory      generate_swing_foot_trajectory / compute_traj_swingfoot      :38-82
//   torques         LegController.update, both branches           leg_controller.py:75-90
//
// The per-leg algebra is mpcqp_swing_leg.h (float64, FP contraction off; also compiled
// for the host by tests/test_swing.py).  The stance branch is the float32 expression of
// mpcqp_stance_torque_kernel, so a stance entry is bitwise what mpcqp_stance_torques writes.
#include "mpcqp_swing_leg.h"

struct SwingParams {
  int ibm;               // iterations_between_mpc (linear_mpc_configs.py:7)
  int root_layout;       // 1: `quat` points at Isaac Gym actor root states [B][13]
  double dt_control;     // mpcqp_set_planner
  double gravity;
  double swing_height;   // mpcqp_set_swing
  double touchdown_z;
  double vel_gain;
  double Kp[9], Kd[9];
  const float* ground;   // mpcqp_set_ground: [ground_cap][4] planes (n, d), or NULL
  int ground_cap;
};

// A workgroup owns kSwingRobots consecutive robots, one thread per (robot, leg) with a
// robot's four legs in adjacent lanes: the [B][4][3], [B][4][3][3] arrays and the
// per-leg state are contiguous across the lanes.  What the four legs share (base
// state, R_base, command, gait record, tick) is read once per robot -- three of the
// robot's lanes each fetch a part -- and handed over in LDS.
constexpr int kSwingRobots = 64;
constexpr int kSwingThreads = 256;

struct SwingBase {
  double vb[3], yr;
  float pos[3], vel[3], R[9];
  float ground[4];   // swing_load_ground
  int period, off[4], dur[4], tick;
};

// Robot b's ground plane into its LDS record, read once per robot (on the lane of leg 3, which
// fetches nothing else); zeros -- no plane -- with none registered or for a robot past the capacity
__device__ inline void swing_load_ground(const SwingParams& sp, int b, float* g) {
  const bool on = sp.ground != nullptr && b < sp.ground_cap;
#pragma unroll
  for (int k = 0; k < 4; ++k) g[k] = on ? sp.ground[4 * (size_t)b + k] : 0.f;
}

// One leg's control law on a lane (one text for mpcqp_leg_torque_kernel and mpcqp_step_kernel):
// the swing decision on the robot's tick, then the stance expression or the swing generator and
// PD law.  The robot's shared values (R_base, pos, vel, the ground plane g32 as float32; the command) come from LDS,
// the leg's kinematics J, th, pf, fp, fv as the float32 values mpcqp_kinematics stores, f its
// force of u0; Kp, Kd the gains (sp's, or a copy of them).  m2 is the leg's generator state as loaded, mp where a leg in swing stores it
// back.  Returns the torques tq, the targets pt / vt (zero in stance) and the swing state *sv.
__device__ inline void swing_leg_control(const SwingParams& sp, const double* Kp, const double* Kd, int tick, int period, int off, int dur, int dur0,
                                         const float* R32, const float* pos, const float* vel, const float* g32,
                                         const double* vbody, double yaw_rate, const float (&J)[9], const float (&f)[3],
                                         const float (&th)[3], const float (&pf)[3], const float (&fp)[3],
                                         const float (&fv)[3], const double2 (&m2)[SW_LEG_STRIDE / 2], double2* mp,
                                         float (&tq)[3], float (&pt)[3], float (&vt)[3], double* sv) {
#pragma clang fp contract(off)
  const int st = swing_decide(tick, sp.ibm, period, off, dur, sv);
#pragma unroll
  for (int k = 0; k < 3; ++k) pt[k] = vt[k] = 0.f;
  if (st == SWING_STANCE) {
    // tau_leg = Jv^T (-f_leg) (leg_controller.py:86-89), as mpcqp_stance_torque_kernel
#pragma unroll
    for (int j = 0; j < 3; ++j) tq[j] = -(J[j] * f[0] + J[3 + j] * f[1] + J[6 + j] * f[2]);
  } else {
    double R[9], p3[3], v3[3], vb[3], thd[3], pfd[3], fpd[3], fvd[3], Jd[9], mem[SW_LEG_STRIDE];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      R[k] = (double)R32[k];
      Jd[k] = (double)J[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      p3[k] = (double)pos[k];
      v3[k] = (double)vel[k];
      vb[k] = vbody[k];
      thd[k] = (double)th[k];
      pfd[k] = (double)pf[k];
      fpd[k] = (double)fp[k];
      fvd[k] = (double)fv[k];
    }
#pragma unroll
    for (int k = 0; k < SW_LEG_STRIDE / 2; ++k) {
      mem[2 * k] = m2[k].x;
      mem[2 * k + 1] = m2[k].y;
    }
    double t_swing, t_stance, pb[3], vbase[3], tqd[3];
    const double gd[4] = {(double)g32[0], (double)g32[1], (double)g32[2], (double)g32[3]};
    swing_times(sp.dt_control, sp.ibm, period, dur0, &t_swing, &t_stance);
    swing_leg_step_ground(mem, st == SWING_FINISHED, sp.dt_control, t_swing, t_stance, p3, v3, R, vb, yaw_rate, thd,
                          pfd, sp.gravity, sp.vel_gain, sp.touchdown_z, sp.swing_height, pb, vbase, gd);
#pragma unroll
    for (int k = 0; k < SW_LEG_STRIDE / 2; ++k) mp[k] = make_double2(mem[2 * k], mem[2 * k + 1]);
    swing_pd(R, Kp, Kd, Jd, pb, vbase, fpd, fvd, tqd);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      tq[k] = (float)tqd[k];
      pt[k] = (float)pb[k];
      vt[k] = (float)vbase[k];
    }
  }
}

__global__ __launch_bounds__(kSwingThreads) void mpcqp_leg_torque_kernel(
    SwingParams sp, int B, const int* __restrict__ tick, const float* __restrict__ quat,
    const float* __restrict__ pos, const float* __restrict__ vel, const float* __restrict__ rot,
    const double* __restrict__ vbody, const double* __restrict__ yaw_rate, const int* __restrict__ gait,
    const float* __restrict__ thighs, const float* __restrict__ pos_feet, const float* __restrict__ foot_pos_base,
    const float* __restrict__ foot_vel_base, const float* __restrict__ jac, const float* __restrict__ u0,
    double* __restrict__ swing_mem, float* __restrict__ tau, float* __restrict__ swing_state,
    float* __restrict__ pos_target, float* __restrict__ vel_target) {
#pragma clang fp contract(off)
  __shared__ SwingBase base[kSwingRobots];
  const int t = threadIdx.x;
  const int r = t >> 2, leg = t & 3;
  const int b = blockIdx.x * kSwingRobots + r;
  const bool live = b < B;   // the tail workgroup: lanes past the batch touch no memory

  // ---- per-leg inputs (issued before the barrier so they overlap the shared reads)
  const size_t bl = (size_t)b * 4 + leg;
  float J[9], f[3], th[3], pf[3], fp[3], fv[3];
  // the leg's generator state: 64 bytes, four 16-byte loads (and stores, for a leg in swing)
  double2* mp = reinterpret_cast<double2*>(swing_mem + bl * SW_LEG_STRIDE);
  double2 m2[SW_LEG_STRIDE / 2];
  if (live) {
#pragma unroll
    for (int k = 0; k < SW_LEG_STRIDE / 2; ++k) m2[k] = mp[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) J[k] = jac[bl * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      f[k] = u0[bl * 3 + k];
      th[k] = thighs[bl * 3 + k];
      pf[k] = pos_feet[bl * 3 + k];
      fp[k] = foot_pos_base[bl * 3 + k];
      fv[k] = foot_vel_base[bl * 3 + k];
    }
  }

  // ---- per-robot inputs, once per robot
  if (live) {
    SwingBase& sb = base[r];
    if (leg == 0) {
      float qw, qx, qy, qz;
      if (sp.root_layout) {   // [pos(3), quat(x, y, z, w), lin_vel(3), ang_vel(3)] (isaacgym_a1.py:119-128)
        const float* rs = quat + (size_t)b * 13;
        qx = rs[3], qy = rs[4], qz = rs[5], qw = rs[6];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          sb.pos[k] = rs[k];
          sb.vel[k] = rs[7 + k];
        }
      } else {
        qw = quat[4 * (size_t)b], qx = quat[4 * (size_t)b + 1], qy = quat[4 * (size_t)b + 2],
        qz = quat[4 * (size_t)b + 3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          sb.pos[k] = pos[3 * (size_t)b + k];
          sb.vel[k] = vel[3 * (size_t)b + k];
        }
      }
      float R[9];
      if (rot != nullptr) {
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = rot[9 * (size_t)b + k];
      } else {
        plan_quat2matrix(qw, qx, qy, qz, R);   // robot_data.py:75
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) sb.R[k] = R[k];
    } else if (leg == 1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) sb.vb[k] = vbody[3 * (size_t)b + k];
      sb.yr = yaw_rate[b];
    } else if (leg == 2) {
      const int* gs = gait + 9 * (size_t)b;   // period, offsets[4], durations[4] (gait.py:16-22)
      sb.period = gs[0];
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        sb.off[l] = gs[1 + l];
        sb.dur[l] = gs[5 + l];
      }
      sb.tick = tick[b];
    } else {
      swing_load_ground(sp, b, sb.ground);
    }
  }
  __syncthreads();
  if (!live) return;

  const SwingBase& sb = base[r];
  double sv;
  float tq[3], pt[3], vt[3];
  swing_leg_control(sp, sp.Kp, sp.Kd, sb.tick, sb.period, sb.off[leg], sb.dur[leg], sb.dur[0], sb.R, sb.pos, sb.vel, sb.ground,
                    sb.vb, sb.yr, J, f, th, pf, fp, fv, m2, mp, tq, pt, vt, &sv);
#pragma unroll
  for (int k = 0; k < 3; ++k) tau[bl * 3 + k] = tq[k];
  if (swing_state != nullptr) swing_state[bl] = (float)sv;
  if (pos_target != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) pos_target[bl * 3 + k] = pt[k];
  }
  if (vel_target != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) vel_target[bl * 3 + k] = vt[k];
  }
}

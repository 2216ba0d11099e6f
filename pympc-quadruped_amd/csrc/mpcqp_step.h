// mpcqp_step.h -- the control tick in one launch: leg kinematics, the plan's sequential part
// and all 12 joint torques of every robot fused (included by mpcqp.hip inside its anonymous
// namespace, after mpcqp_plan.h, mpcqp_swing.h and mpcqp_kinematics.h, whose stages it
// composes).  For B robots it is the loop body of scripts/isaacgym_a1.py:117-162 on the
// simulator's two state tensors:
//
//   kinematics     RobotData.update                              robot_data.py:59-108
//   pack           ModelPredictiveController.update_robot_state  mpc.py:55-79
//   integrate      update_mpc_if_needed (pose integrators)       mpc.py:81-92
//   reference      generate_reference_trajectory (MPC ticks)     mpc.py:110-170
//   gait table     Gait.set_iteration / get_gait_table           gait.py:76-100
//   leg control    Gait.get_swing_state, the swing generator,
//                  LegController.update                          leg_controller.py:75-90
//
// Three instantiations of one kernel: STEP_WHOLE is a non-MPC tick; STEP_FRONT and STEP_BACK
// are the parts of an MPC tick ahead of and after the solve.  The algebra is the headers' of
// the three kernels it replaces (kin_leg, plan_robot / plan_rows, swing_leg_control), FP
// contraction off, and each kinematic value is rounded to float32 once -- where
// mpcqp_kinematics_kernel's store rounds it -- and widened again for the leg controller, so
// every output is bitwise what mpcqp_kinematics + mpcqp_plan + mpcqp_leg_torques write.

constexpr int STEP_WHOLE = 0, STEP_FRONT = 1, STEP_BACK = 2;

struct StepParams {
  int N;                  // the plan's constants beyond sw's dt_control and gravity (PlanParams)
  double dt;
  double max_pos_error;
  SwingParams sw;
};

// The geometry of the three kernels: a workgroup owns kStepRobots consecutive robots, one
// thread per (robot, leg) with a robot's four legs in adjacent lanes.
constexpr int kStepRobots = 64;
constexpr int kStepThreads = 256;
static_assert(kStepRobots == kPlanRobots && kStepThreads == kPlanThreads, "plan_rows runs on this geometry");

// What a robot's four lanes share, read once per robot and handed over in LDS (KinBase,
// SwingBase and PlanSeed in one record; the gait record and the command are held once)
struct StepBase {
  double Rq[9], geom[5], vb[3], yr;
  PlanSeed seed;   // STEP_FRONT: the row seeds of plan_rows
  float pos[3], vel[3], omega[3], R[9];
  float ground[4];   // swing_load_ground
  int period, off[4], dur[4], tick;
};
static_assert(sizeof(StepBase) * kStepRobots + sizeof(float) * kStepRobots * 3 * kMaxN < 64 * 1024,
              "static LDS of STEP_FRONT");

// floor(tick / ibm) mod period, non-negative; 0 for period <= 0 (gait.py:76-78; ibm >= 1)
__device__ inline int step_gait_segment(int tick, int ibm, int period) {
  if (period <= 0) return 0;
  int q = tick / ibm;
  if (tick % ibm != 0 && tick < 0) --q;
  int m = q % period;
  return m < 0 ? m + period : m;
}

// mpcqp_plan's parameters as mpcqp_step runs it: the root layout, the integrators on, the
// reference in STEP_FRONT alone (a compile-time constant, so STEP_WHOLE carries none of it)
template <int MODE>
__device__ inline PlanParams step_plan_params(const StepParams& sp) {
  PlanParams pp;
  pp.N = sp.N;
  pp.mpc_tick = MODE == STEP_FRONT ? 1 : 0;
  pp.root_layout = 1;
  pp.integrate = 1;
  pp.dt = sp.dt;
  pp.dt_control = sp.sw.dt_control;
  pp.gravity = sp.sw.gravity;
  pp.max_pos_error = sp.max_pos_error;
  return pp;
}

// Stage 1, before the barrier: the robot's shared inputs into its LDS record -- three of its
// lanes each fetch a part -- and but for STEP_BACK the plan's sequential part on the lane of leg 0,
// which holds the root state in registers: x0, plan_state and (STEP_FRONT) the row seeds.
template <int MODE>
__device__ inline void step_load(const StepParams& sp, int b, int leg, StepBase& sb, int iter_counter,
                                 const int* __restrict__ tick, const float* __restrict__ root_states,
                                 const double* __restrict__ geom, const double* __restrict__ vbody,
                                 const double* __restrict__ yaw_rate, const int* __restrict__ gait,
                                 const float* __restrict__ height, double* __restrict__ plan_state,
                                 float* __restrict__ x0) {
#pragma clang fp contract(off)
  if (leg == 0) {
    // [pos(3), quat(x, y, z, w), lin_vel(3), ang_vel(3)] (isaacgym_a1.py:119-130)
    const float* rs = root_states + (size_t)b * 13;
    const float qx = rs[3], qy = rs[4], qz = rs[5], qw = rs[6];
    float p3[3], v3[3], w3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      p3[k] = rs[k];
      v3[k] = rs[7 + k];
      w3[k] = rs[10 + k];
      sb.pos[k] = p3[k];
      sb.vel[k] = v3[k];
      sb.omega[k] = w3[k];
    }
    double Rq[9];
    kin_quat2matrix((double)qw, (double)qx, (double)qy, (double)qz, Rq);   // robot_data.py:85-92
    float R[9];
    plan_quat2matrix(qw, qx, qy, qz, R);                                   // robot_data.py:75
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      sb.Rq[k] = Rq[k];
      sb.R[k] = R[k];
    }
    if (MODE != STEP_BACK) {
      int ih0 = 0;
      if (MODE == STEP_FRONT)
        ih0 = step_gait_segment(tick != nullptr ? tick[b] : iter_counter, sp.sw.ibm, gait[9 * (size_t)b]);
      plan_robot(step_plan_params<MODE>(sp), b, qw, qx, qy, qz, p3, w3, v3, nullptr, vbody, yaw_rate, gait, nullptr, ih0, height,
                 plan_state, x0, sb.seed);
    }
  } else if (leg == 1) {
#pragma unroll
    for (int k = 0; k < 5; ++k) sb.geom[k] = geom[KIN_STRIDE * (size_t)b + k];
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
    sb.tick = tick != nullptr ? tick[b] : iter_counter;
  } else if (MODE != STEP_FRONT) {
    swing_load_ground(sp.sw, b, sb.ground);
  }
}

// Stage 2, after the barrier: the leg's kinematics from its joint pair and the robot's record,
// each value rounded to float32 once (the store of mpcqp_kinematics_kernel).
__device__ inline void step_kin(const StepBase& sb, int leg, const double (&ql)[3], const double (&qd)[3],
                                float (&ft)[3], float (&th)[3], float (&pf)[3], float (&fp)[3], float (&fv)[3],
                                float (&J)[9]) {
#pragma clang fp contract(off)
  double Rq[9], Rb[9], g[5], p3[3], v3[3], w3[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    Rq[k] = sb.Rq[k];
    Rb[k] = (double)sb.R[k];
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) g[k] = sb.geom[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    p3[k] = (double)sb.pos[k];
    v3[k] = (double)sb.vel[k];
    w3[k] = (double)sb.omega[k];
  }
  double ftd[3], thd[3], pfd[3], fpd[3], fvd[3], Jd[9];
  kin_leg(g, leg, ql, qd, Rq, Rb, p3, v3, w3, ftd, thd, pfd, fpd, fvd, Jd);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ft[k] = (float)ftd[k];
    th[k] = (float)thd[k];
    pf[k] = (float)pfd[k];
    fp[k] = (float)fpd[k];
    fv[k] = (float)fvd[k];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) J[k] = (float)Jd[k];
}

__device__ inline void step_store3(float* __restrict__ out, size_t bl, const float (&v)[3]) {
  if (out == nullptr) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) out[bl * 3 + k] = v[k];
}

template <int MODE>
__global__ __launch_bounds__(kStepThreads) void mpcqp_step_kernel(
    StepParams sp, int B, int iter_counter, const int* __restrict__ tick, const float* __restrict__ root_states,
    const float* __restrict__ dof_states, const double* __restrict__ geom, const double* __restrict__ vbody,
    const double* __restrict__ yaw_rate, const int* __restrict__ gait, const float* __restrict__ height,
    double* __restrict__ plan_state, double* __restrict__ swing_mem, float* __restrict__ x0,
    float* __restrict__ xref, float* __restrict__ contact, float* __restrict__ feet, const float* __restrict__ u0,
    float* __restrict__ tau, float* __restrict__ thighs, float* __restrict__ pos_feet,
    float* __restrict__ foot_pos_base, float* __restrict__ foot_vel_base, float* __restrict__ jac,
    float* __restrict__ swing_state, float* __restrict__ pos_target, float* __restrict__ vel_target) {
#pragma clang fp contract(off)
  constexpr bool kLegs = MODE != STEP_FRONT;
  __shared__ StepBase base[kStepRobots];
  // the swing gains Kp, Kd through LDS: held as kernel arguments they would stay in 36 scalar
  // registers from the entry to swing_pd, beside 24 pointers, more than a wave has
  __shared__ double gains[kLegs ? 18 : 1];
  const int t = threadIdx.x;
  if (kLegs && t < 18) gains[t] = t < 9 ? sp.sw.Kp[t] : sp.sw.Kd[t - 9];
  const int r = t >> 2, leg = t & 3;
  const int b0 = blockIdx.x * kStepRobots;
  const int b = b0 + r;
  const bool live = b < B;   // the tail workgroup: lanes past the batch touch no memory

  // ---- per-leg inputs (issued before the barrier so they overlap the shared reads)
  const size_t bl = (size_t)b * 4 + leg;
  double ql[3] = {0.0, 0.0, 0.0}, qd[3] = {0.0, 0.0, 0.0};
  float f[3] = {0.f, 0.f, 0.f};
  // the leg's generator state: 64 bytes, four 16-byte loads (and stores, for a leg in swing)
  double2* mp = reinterpret_cast<double2*>(swing_mem + bl * SW_LEG_STRIDE);
  double2 m2[SW_LEG_STRIDE / 2];
  if (live) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {   // (pos, vel) per DOF (isaacgym_a1.py:116,131-132)
      ql[k] = (double)dof_states[(bl * 3 + k) * 2];
      qd[k] = (double)dof_states[(bl * 3 + k) * 2 + 1];
    }
    if (kLegs) {
#pragma unroll
      for (int k = 0; k < SW_LEG_STRIDE / 2; ++k) m2[k] = mp[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) f[k] = u0[bl * 3 + k];
    }
    step_load<MODE>(sp, b, leg, base[r], iter_counter, tick, root_states, geom, vbody, yaw_rate, gait, height,
                     plan_state, x0);
  }
  __syncthreads();

  float ft[3], th[3], pf[3], fp[3], fv[3], J[9];
  if (live) {
    step_kin(base[r], leg, ql, qd, ft, th, pf, fp, fv, J);
    if (MODE != STEP_BACK) step_store3(feet, bl, ft);   // STEP_BACK: the solve has read STEP_FRONT's
    if (kLegs) {
      step_store3(thighs, bl, th);
      step_store3(pos_feet, bl, pf);
      step_store3(foot_pos_base, bl, fp);
      step_store3(foot_vel_base, bl, fv);
      if (jac != nullptr) {
#pragma unroll
        for (int k = 0; k < 9; ++k) jac[bl * 9 + k] = J[k];
      }
    }
  }

  if constexpr (MODE == STEP_FRONT) {   // every thread: plan_rows holds the workgroup's barriers
    __shared__ float seq[kStepRobots][3][kMaxN];   // yaw / x / y along the horizon
    plan_rows(step_plan_params<MODE>(sp), b0, min(kStepRobots, B - b0), t, [&](int i) -> const PlanSeed& { return base[i].seed; }, seq,
              gait, xref, contact);
  }

  if (kLegs && live) {
    const StepBase& sb = base[r];
    double sv;
    float tq[3], pt[3], vt[3];
    swing_leg_control(sp.sw, gains, gains + 9, sb.tick, sb.period, sb.off[leg], sb.dur[leg], sb.dur[0], sb.R, sb.pos, sb.vel, sb.ground,
                      sb.vb, sb.yr, J, f, th, pf, fp, fv, m2, mp, tq, pt, vt, &sv);
    step_store3(tau, bl, tq);
    if (swing_state != nullptr) swing_state[bl] = (float)sv;
    step_store3(pos_target, bl, pt);
    step_store3(vel_target, bl, vt);
  }
}

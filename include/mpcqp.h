/*
 * mpcqp.h -- C ABI of the MI355X batched convex-MPC QP engine (libmpcqp.so).
 *
 * Replaces, for a batch of B independent robots, the per-tick
 * formulate-and-solve of the reference's ModelPredictiveController:
 *
 *   _generate_state_space_model   /root/reference/linear_mpc/mpc.py:173-192
 *   _discretize_continuous_model  /root/reference/linear_mpc/mpc.py:194-208
 *   _generate_QP_cost             /root/reference/linear_mpc/mpc.py:211-235
 *   _generate_QP_constraints      /root/reference/linear_mpc/mpc.py:237-260
 *   _solve_mpc (Drake branch)     /root/reference/linear_mpc/mpc.py:262-286
 *
 * i.e.  min_U 1/2 U^T H U + g^T U  s.t.  lb <= C U <= ub  (Drake
 * AddQuadraticCost semantics, mpc.py:281-282), returning the first-step
 * ground-reaction forces U[0:12] (mpc.py:99).  The reference binds that path
 * through pydrake (mpc.py:13, :278-286); the ctypes binding that replaces it
 * is shown in INTEGRATION.md.
 *
 * All array arguments are DEVICE pointers owned by the caller (e.g. torch
 * tensors on the context's device).  Calls are asynchronous on `stream`.
 * No exception crosses the ABI: every entry point returns MPCQP_OK (0) or a
 * negative error code; mpcqp_last_error() describes the last failure.
 * Per-robot solver outcome is reported in status[] (MPCQP_STATUS_*).
 * A context keeps per-stream device queues for up to 8 streams; a solve on a 9th
 * distinct stream takes over the least recently used stream's queues once that stream's
 * last solve on this context has finished (the host waits on an event recorded after
 * it -- not on the device or the other streams).  Round-robin over at most 8 streams per
 * context to stay fully asynchronous.
 *
 * Layouts (float32, row-major, robot-major):
 *   x0      [B][13]   [roll, pitch, yaw, px, py, pz, wx, wy, wz, vx, vy, vz, -g]
 *                     (mpc.py:65-77; x0[2] is also the model yaw, mpc.py:77)
 *   xref    [B][N][13] reference of x_{1..N} (mpc.py:154-168)
 *   contact [B][N][4]  legs FL, FR, RL, RR; > 0 = stance (gait.py:87-98);
 *                      ub of the normal-force row is contact * fz_max (mpc.py:257), so a
 *                      value other than 1 scales the foot-step's bound.  Anything that is
 *                      not > 0 is swing: 0, a negative value, -inf and NaN alike (the
 *                      values are not otherwise checked).  +inf would be an infinite
 *                      bound: the robot is refused (MPCQP_STATUS_NONFINITE)
 *   feet    [B][4][3]  foot position relative to the CoM, world frame
 *                      (RobotData.pos_base_feet, robot_data.py:101,144-149)
 *   robot   [B][16]    per-robot record: mass, ixx, ixy, ixz, iyy, iyz, izz,
 *                      mu, fz_max, nx, ny, nz, 0, 0, 0, 0
 *                      (robot_configs.py:44-79; normal (0,0,1) = reference cone)
 *   u0      [B][12]    out: first-step GRFs, world frame (mpc.py:99)
 *   U       [B][N][12] out (nullable): the whole optimal input sequence
 *   status  [B]        out (nullable): MPCQP_STATUS_*
 *   iters   [B]        out (nullable): active-set steps executed (a pair step counts 2, so
 *                      under MPCQP_STATUS_MAX_ITER at most max_iter + 1: a pass refused at
 *                      the cap is not counted);
 *                      for a robot with more than 128 stance variables (the interior-point
 *                      class: standing schedules at N >= 11) the Newton factorisations
 *
 * Input reads: a robot's x0 / xref / contact / feet / robot slices are staged with
 * 16-byte loads of the 16-byte-aligned chunks that cover them, so up to 12 bytes
 * before and after each slice (never across a 4 KiB page) are read and ignored.
 * The buffers must be device allocations (hipMalloc / torch: page-granular, no
 * guard pages); the values read outside a slice never reach any result.
 */
#ifndef MPCQP_H
#define MPCQP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPCQP_ABI_VERSION 6
#define MPCQP_ROBOT_STRIDE 16
#define MPCQP_ROBOT_NORMAL 9   /* first of the three words of the surface normal in a robot record */
#define MPCQP_MAX_HORIZON 32   /* mpcqp_create rejects horizon > 32 (MPCQP_ERR_ARG).  Horizons
                                  up to 20 use every capacity class; longer ones are solved by
                                  the interior-point class alone (its per-robot LDS scratch is
                                  sized for 32 stages, the dense classes' for 20) */

/* error codes (return values) */
#define MPCQP_OK 0
#define MPCQP_ERR_ARG -1
#define MPCQP_ERR_HIP -2
#define MPCQP_ERR_ALLOC -3

/* per-robot status */
#define MPCQP_STATUS_OK 0          /* the optimum: every cone row feasible, every active
                                      multiplier >= 0 (checked); stationarity holds by
                                      construction of the dual active-set updates (dense
                                      classes) or is checked on the active set's null
                                      space (interior-point class, n > 128) */
#define MPCQP_STATUS_MAX_ITER 1    /* iteration cap hit: best iterate returned */
#define MPCQP_STATUS_INFEASIBLE 2  /* cannot happen for this QP (U = 0 is feasible) */
#define MPCQP_STATUS_TOO_LARGE 3   /* stance variables exceed the engine's capacity */
#define MPCQP_STATUS_NONFINITE 4   /* non-finite input (x0, xref, feet, robot[0..11]; a +inf
                                      contact) or result (finite inputs reach it: mass 0, a
                                      singular inertia, a surface normal along world x, whose
                                      tangent frame is 0 / 0); u0 / U are 0, iters 0 */
#define MPCQP_STATUS_UNSUPPORTED 5 /* weights the robot's capacity class cannot apply; no
                                      weights reach it since ABI 6's cross-leg stage weights
                                      (kept as a guard); u0 / U are 0 */

typedef struct mpcqp_params {
  int32_t horizon;       /* N (LinearMpcConfig.horizon, linear_mpc_configs.py:11) */
  int32_t max_iter;      /* active-set iteration cap per robot of the dense classes (n <= 126),
                            0 = default; the interior-point class (n > 128) stops after its own
                            60 Newton iterations and does not read it */
  double dt;             /* model step, 0.05 in the reference (mpc.py:38) */
  double q_diag[13];     /* state weights (linear_mpc_configs.py:19) */
  double r_diag[12];     /* input weights (linear_mpc_configs.py:20) */
} mpcqp_params;

typedef struct mpcqp_ctx mpcqp_ctx;

/* Fill `p` with the reference's LinearMpcConfig values for horizon N. */
void mpcqp_default_params(mpcqp_params* p, int32_t horizon);

/* Create a context on HIP device `device`; the context owns scratch memory. */
int mpcqp_create(const mpcqp_params* p, int32_t device, mpcqp_ctx** out);

/* Formulate and solve B QPs (see header comment for layouts). */
int mpcqp_solve(mpcqp_ctx* ctx, int32_t batch, const float* x0, const float* xref,
                const float* contact, const float* feet, const float* robot, float* u0,
                float* U, int32_t* status, int32_t* iters, void* stream /* hipStream_t */);

/* Full state / input weights (mpc.py:49-52 builds kron(I_N, Q), kron(I_N, R) from any
 * LinearMpcConfig.Q / R): Q [13][13] and R [12][12] row-major HOST arrays, symmetric and
 * finite (else MPCQP_ERR_ARG); NULL keeps the current matrix (as last set, off-diagonal
 * entries included).  Diagonal matrices select the diagonal fast path (equivalent to
 * setting q_diag / r_diag).  The weights are copied before the call returns; solves issued
 * before it are unaffected.  A failed call (error code) leaves the previous weights in
 * force.  The previous full-weight buffer is kept until mpcqp_destroy (solves in flight
 * may still read it); only every 64th change synchronises the whole device
 * (hipDeviceSynchronize) to release the kept buffers -- not while a stream of this
 * device is being captured into a graph.
 * Every capacity class takes any symmetric Q and R; an R coupling different legs
 * (R[i][j] != 0 for i / 3 != j / 3) runs the interior-point class (robots with more than 128
 * stance variables) with whole 12 x 12 stage weights instead of per-leg blocks. */
int mpcqp_set_weights(mpcqp_ctx* ctx, const double* Q, const double* R);

/* Largest number of stance foot-steps the caller promises per robot
 * (0 = unknown: the engine dispatches every capacity class). */
int mpcqp_set_stance_hint(mpcqp_ctx* ctx, int32_t max_stance);

/* Both bounds on the stance foot-steps per robot (min 0 and max 0 = no promise):
 * classes no robot can need are not launched, and when the range rules out the
 * smaller classes the first possible one takes the batch directly (the drop-in
 * controller passes its gait table's exact count).  A robot outside the range is
 * still solved if a launched class covers it, else reports MPCQP_STATUS_TOO_LARGE.
 * MPCQP_ERR_ARG when min_stance > 4 * horizon (no schedule has that many) or
 * min_stance > max_stance > 0. */
int mpcqp_set_stance_range(mpcqp_ctx* ctx, int32_t min_stance, int32_t max_stance);

/* Dispatch order (ABI 6; the reference solves one robot at a time and has no batch order).
 * mode 1 (the default): when a batch queues on the CUs (more robots than its first capacity
 * class holds on the device at once: 4 per CU for class 64, 1 for classes 96 / 128), its
 * robots are dealt to workgroups largest predicted solve time first -- the key is the robot's
 * horizontal velocity error |v0 - vref_0|, which tracks its active-set size -- so the longest
 * robots start first and the launch ends near its mean load.  Costs one small sort launch per
 * such solve; the results are bitwise those of mode 0 (batch order: robot b on workgroup b).
 * The order needs the stream's queue set even for a batch class 64 solves alone: the first
 * such call on a stream allocates it (hipMalloc + an asynchronous clear), and a later, larger
 * batch reallocates it after a synchronisation of that stream.  To capture solves into a HIP
 * graph, make one call of at least the captured batch size on the capture stream first, or
 * set mode 0 (a class-64-only solve in batch order allocates nothing).
 * MPCQP_ERR_ARG for any other mode. */
int mpcqp_set_order(mpcqp_ctx* ctx, int32_t mode);

/* Warm start (ABI 5; no counterpart in the reference, whose Drake solve starts cold every
 * MPC tick, mpc.py:277-286): per-robot memory of the last verified active set, for
 * callers that solve the same robots tick after tick (the drop-in controller, a fleet in
 * a simulation loop).  The interior-point class (robots with more than 128 stance
 * variables, e.g. Gait.STANDING at N >= 11) then first tries the remembered rows -- one
 * equality-constrained solve and the KKT check its polish always runs, corrected up to 8
 * times -- and runs the interior point only when that fails.  The result does not depend
 * on the memory: a status-OK solution is the checked optimum either way.
 *   memory    DEVICE buffer of capacity * MPCQP_WARM_BYTES bytes, zero-filled by the
 *             caller before first use (zero = nothing remembered).  Robot b of every later
 *             mpcqp_solve on this context reads and rewrites memory + b * MPCQP_WARM_BYTES
 *             (byte 4 k + leg: 0x80 | the foot-step's active cone rows; b >= capacity: no
 *             memory).  Solves running concurrently on different streams must not share it.
 *   NULL / capacity 0 disables (the default).  The dense classes (n <= 128) do not use it.
 * MPCQP_ERR_ARG for capacity < 0, or memory NULL with capacity > 0. */
#define MPCQP_WARM_BYTES 128   /* 4 * MPCQP_MAX_HORIZON */
int mpcqp_set_warm_start(mpcqp_ctx* ctx, void* memory, int32_t capacity);

/* ---- the hot path's callers on the device -------------
 *
 * mpcqp_plan replaces, per control iteration and batched over robots:
 *   ModelPredictiveController.update_robot_state  (state packing)  mpc.py:55-79
 *     quat2ZYXangle                                                kinematics.py:40-49
 *   update_mpc_if_needed (desired-pose integrators)                mpc.py:81-92
 *   generate_reference_trajectory          (MPCQP_PLAN_REFERENCE)  mpc.py:110-170
 *   Gait.set_iteration / get_gait_table    (MPCQP_PLAN_REFERENCE)  gait.py:76-100
 * Its x0 / xref / contact outputs feed mpcqp_solve directly (no host round trip).
 * Call it every control iteration (the integrators run at 1/dt_control) with
 * flags = MPCQP_PLAN_REFERENCE when iter % iterations_between_mpc == 0 (mpc.py:95),
 * else 0.  MPCQP_PLAN_NO_INTEGRATE skips the integrators: REFERENCE | NO_INTEGRATE
 * is generate_reference_trajectory alone (mpc.py:110-170).
 *
 *   quat         [B][4]  base orientation (w, x, y, z)            robot_data.quat_base
 *   pos, omega, vel [B][3]  base position, angular / linear velocity (world)
 *   rot          [B][3][3]  R_base, row-major (mpc.py:83); NULL = quat2matrix(quat)
 *                        computed on the device (robot_data.py:75)
 *   vel_body_des [B][3]  float64 desired base velocity, body frame (mpc.py:83)
 *   yaw_rate_des [B]     float64 desired yaw rate
 *   gait         [B][9]  int32: period, stance offsets[4], stance durations[4]
 *                        (gait.py:16-22; e.g. TROTTING10 = 10, 0 5 5 0, 5 5 5 5);
 *                        NULL = the caller supplies its own contact schedule
 *   iteration    [B]     int32 gait segment: floor(iter / iterations_between_mpc) % period
 *                        (gait.py:76-78)
 *   height_des   [B]     desired CoM height (robot_configs.py:50,69)
 *   plan_state   [B][MPCQP_PLAN_STRIDE] float64 in/out: x_des, y_des, yaw_des,
 *                        roll_init, pitch_init, started, 0, 0; all-zero = first run
 *   x0 [B][13], xref [B][N][13], contact [B][N][4]: out (xref / contact only written
 *                        with MPCQP_PLAN_REFERENCE; contact only with a gait)
 */
#define MPCQP_PLAN_STRIDE 8
#define MPCQP_GAIT_STRIDE 9
#define MPCQP_PLAN_REFERENCE 1
#define MPCQP_PLAN_NO_INTEGRATE 2
int mpcqp_plan(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* quat, const float* pos,
               const float* omega, const float* vel, const float* rot, const double* vel_body_des,
               const double* yaw_rate_des, const int32_t* gait, const int32_t* iteration,
               const float* height_des, double* plan_state, float* x0, float* xref, float* contact,
               void* stream);

/* The same, reading Isaac Gym's actor root-state tensor in place:
 * root_states [B][13] = pos(3), quat(x, y, z, w), lin_vel(3), ang_vel(3) -- the
 * layout isaacgym_a1.py:119-128 slices and reorders per robot on the host.  R_base
 * is quat2matrix of that quaternion. */
int mpcqp_plan_root_states(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* root_states,
                           const double* vel_body_des, const double* yaw_rate_des, const int32_t* gait,
                           const int32_t* iteration, const float* height_des, double* plan_state, float* x0,
                           float* xref, float* contact, void* stream);

/* Planner constants: dt_control (linear_mpc_configs.py:6, default 0.001), gravity
 * (:13, 9.81) and the reference-position clamp (mpc.py:121, 0.1).  MPCQP_ERR_ARG for a
 * non-finite constant or a negative dt_control / max_pos_error; the constants then stay
 * as they were. */
int mpcqp_set_planner(mpcqp_ctx* ctx, double dt_control, double gravity, double max_pos_error);

/* Stance-leg joint torques tau = Jv_leg^T (-f_leg) (leg_controller.py:86-89,
 * SURVEY §8 f4) for the legs with stance[b * stance_stride + leg] > 0 -- the
 * controller's `not swing_states[leg]` (leg_controller.py:77); swing-leg entries of
 * tau are not written.  jac [B][4][3][3]: each leg's 3x3 block of its foot Jacobian (rows = world
 * x, y, z; columns = the leg's 3 joints), row-major.  u0 [B][12], tau [B][12]. */
int mpcqp_stance_torques(mpcqp_ctx* ctx, int32_t batch, const float* jac, const float* stance,
                         int32_t stance_stride, const float* u0, float* tau, void* stream);

/* ---- the leg controller on the device: all 12 joint torques per control iteration ----
 *
 * mpcqp_leg_torques replaces, batched over robots x legs, the rest of the loop body of
 * scripts/isaacgym_a1.py:137-162:
 *   Gait.set_iteration / get_swing_state                            gait.py:76-79,102-121
 *   SwingFootTrajectoryGenerator.set_foot_placement  swing_foot_trajectory_generator.py:84-129
 *   generate_swing_foot_trajectory / compute_traj_swingfoot         :38-82
 *   LegController.update, swing and stance branch                   leg_controller.py:75-90
 * Call it every control iteration.  One launch, no allocation, synchronisation or host
 * read: it can be captured into a HIP graph (tick lives on the device, so a replay sees
 * fresh counters).  A leg swings while its swing state is > 0 and is in stance otherwise;
 * the decision is taken in integer arithmetic on tick % (iterations_between_mpc * period).
 * A swing offset past the period wraps per leg -- a negative stance offset wraps the same
 * way, and swing_state is (ticks into the swing) / (ticks per swing) for either -- and a leg
 * whose stance fills the period never swings, nor does any leg of a record with period <= 0:
 * such a leg is in stance and its swing_mem is not written (deviations).
 *
 *   flags        0 (reserved)
 *   tick         [B]     int32: each robot's control-iteration counter (iter_counter,
 *                        isaacgym_a1.py:137)
 *   iterations_between_mpc   linear_mpc_configs.py:7 (20); >= 1
 *   quat, pos, vel, rot, vel_body_des, yaw_rate_des, gait   as for mpcqp_plan (gait required)
 *   thighs       [B][4][3]  hip positions, base frame (robot_data.base_pos_base_thighs)
 *   pos_feet     [B][4][3]  foot positions, world frame (robot_data.pos_feet)
 *   foot_pos_base, foot_vel_base [B][4][3]  foot position / velocity relative to the base,
 *                        base frame (robot_data.base_pos_base_feet, base_vel_base_feet)
 *   jac          [B][4][3][3]  as for mpcqp_stance_torques
 *   u0           [B][12]  contact forces (mpc.py:99)
 *   swing_mem    [B][MPCQP_SWING_STRIDE] float64 in/out, 16-byte aligned: per leg
 *                        armed (1 while a swing is under way), remaining swing time,
 *                        footpos_init[3], footpos_final[3] (world); all-zero = first swing
 *                        (swing_foot_trajectory_generator.py:19-24).  Written only for legs
 *                        in swing.
 *   tau          [B][12]  out: every entry -- swing legs Jv^T [Kp (R p_des - R p_foot) +
 *                        Kd (R v_des - R v_foot)], stance legs Jv^T (-f) (bitwise what
 *                        mpcqp_stance_torques writes)
 *   swing_state  [B][4]   out (nullable): gait.py:102-121, 0 = stance
 *   pos_target, vel_target [B][4][3]  out (nullable): swing-foot targets relative to the
 *                        base, base frame (isaacgym_a1.py:147-160); 0 for stance legs
 * dt_control and gravity are mpcqp_set_planner's. */
#define MPCQP_SWING_STRIDE 32
int mpcqp_leg_torques(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const int32_t* tick,
                      int32_t iterations_between_mpc, const float* quat, const float* pos, const float* vel,
                      const float* rot, const double* vel_body_des, const double* yaw_rate_des,
                      const int32_t* gait, const float* thighs, const float* pos_feet,
                      const float* foot_pos_base, const float* foot_vel_base, const float* jac, const float* u0,
                      double* swing_mem, float* tau, float* swing_state, float* pos_target, float* vel_target,
                      void* stream);

/* The same, reading Isaac Gym's actor root-state tensor in place (see
 * mpcqp_plan_root_states; isaacgym_a1.py:119-128). */
int mpcqp_leg_torques_root_states(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const int32_t* tick,
                                  int32_t iterations_between_mpc, const float* root_states,
                                  const double* vel_body_des, const double* yaw_rate_des, const int32_t* gait,
                                  const float* thighs, const float* pos_feet, const float* foot_pos_base,
                                  const float* foot_vel_base, const float* jac, const float* u0,
                                  double* swing_mem, float* tau, float* swing_state, float* pos_target,
                                  float* vel_target, void* stream);

/* Swing constants: the apex height of the swing curve, an absolute world z
 * (RobotConfig.swing_height, robot_configs.py:54, 0.1), the PD gains Kp / Kd [3][3]
 * row-major HOST doubles (robot_configs.py:55-56, A1Config: 700 I and 20 I; NULL keeps the
 * current matrix), the foothold's world z (swing_foot_trajectory_generator.py:120, -0.0255)
 * and the gain of its velocity-error term (:116, 0.03).  A non-finite value returns
 * MPCQP_ERR_ARG and leaves the previous constants in force. */
int mpcqp_set_swing(mpcqp_ctx* ctx, double swing_height, const double* Kp, const double* Kd,
                    double touchdown_z, double vel_gain);

/* ---- the leg kinematics on the device: every array the entry points above consume ----
 *
 * mpcqp_kinematics replaces, batched over robots x legs, RobotData.update
 * (utils/robot_data.py:59-108) -- pinocchio.forwardKinematics / framesForwardKinematics
 * (:91-92), computeFrameJacobian (:117-133) and the frame changes (:135-184) -- for the leg
 * both shipped robots have: hip revolute about x, thigh and calf revolute about y, zero
 * joint rpy (a1.urdf:211-310, aliengo.urdf:253-358).  Leg order FL, FR, RL, RR.  One launch,
 * no allocation, synchronisation or host read.  Float64 arithmetic on the float32 inputs,
 * each output rounded to float32 once.
 *
 *   flags        0 (reserved)
 *   quat, pos, vel, omega, rot   as for mpcqp_plan: the free-flyer rotation Rq is Eigen's
 *                        quaternion-to-matrix formula in float64 on quat as given (not
 *                        normalised, robot_data.py:85-92); R_base is rot, or quat2matrix in
 *                        float32 arithmetic when rot is NULL (:75)
 *   q, qdot      [B][12]  joint angles / rates, three per leg (hip, thigh, calf)
 *   geom         [B][MPCQP_KIN_STRIDE] float64: hip_x, hip_y, thigh_y, l_thigh, l_calf, 0, 0, 0
 *                        (magnitudes; the leg's signs are applied here)
 * Outputs, each nullable (a NULL output is not written):
 *   feet         [B][4][3]  Rq p: feet relative to the base, world frame
 *                        (robot_data.pos_base_feet, :101) -- the `feet` of mpcqp_solve
 *   thighs       [B][4][3]  R_base^T Rq p_thigh (base_pos_base_thighs, :108)
 *   pos_feet     [B][4][3]  pos + Rq p (pos_feet, :99)
 *   foot_pos_base [B][4][3] R_base^T Rq p (base_pos_base_feet, :103)
 *   foot_vel_base [B][4][3] R_base^T (Rq (vel + omega x p + J_b qdot) - vel)
 *                        (base_vel_base_feet, :158-167: the reference multiplies Pinocchio's
 *                        body-frame free-flyer columns by the world-frame vel / omega, and so
 *                        does this; DESIGN.md, deviations)
 *   jac          [B][4][3][3]  Rq J_b, the block Jv_feet[leg][:, 6 + 3 leg : 9 + 3 leg]
 *                        (:117-133, LOCAL_WORLD_ALIGNED); as for mpcqp_stance_torques
 * with p, p_thigh the foot and thigh-joint position in the base frame and J_b = dp/dq. */
#define MPCQP_KIN_STRIDE 8
int mpcqp_kinematics(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* quat, const float* pos,
                     const float* vel, const float* omega, const float* rot, const float* q, const float* qdot,
                     const double* geom, float* feet, float* thighs, float* pos_feet, float* foot_pos_base,
                     float* foot_vel_base, float* jac, void* stream);

/* The same, reading Isaac Gym's tensors in place: root_states [B][13] (see
 * mpcqp_plan_root_states) and the dof-state tensor dof_states [B][12][2], (pos, vel) per
 * DOF -- what isaacgym_a1.py:116,119-132 slices and copies to the host per robot. */
int mpcqp_kinematics_root_states(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* root_states,
                                 const float* dof_states, const double* geom, float* feet, float* thighs,
                                 float* pos_feet, float* foot_pos_base, float* foot_vel_base, float* jac,
                                 void* stream);

/* ---- the control tick in one call: kinematics, plan and leg torques fused ----
 *
 * mpcqp_step is the whole loop body of scripts/isaacgym_a1.py:117-162 for B robots on the
 * simulator's two state tensors: what mpcqp_kinematics_root_states, mpcqp_plan_root_states,
 * (on an MPC tick) mpcqp_solve and mpcqp_leg_torques_root_states do when issued in that order
 * on the same buffers, and bitwise their results.  Isaac Gym layout only; a caller with
 * split arrays keeps those entry points.  No allocation beyond what mpcqp_solve makes on its
 * first use, no synchronisation or host read.
 *
 *   flags        0: a tick between two solves (mpc.py:95-106 holds u0) -- ONE launch; the
 *                        kinematic arrays stay in registers unless asked for.
 *                MPCQP_STEP_MPC when iter % iterations_between_mpc == 0 (mpc.py:95; the caller
 *                        decides, as with MPCQP_PLAN_REFERENCE): one call that enqueues, on
 *                        `stream`, the kinematics and the plan with the reference, exactly what
 *                        mpcqp_solve enqueues (warm start, order, stance range and weights
 *                        apply), and the leg controller on the fresh u0.
 *   iter_counter, tick   the control-iteration counter (isaacgym_a1.py:137): tick [B] int32 is
 *                        each robot's, as for mpcqp_leg_torques; with tick == NULL every robot
 *                        uses iter_counter.  On an MPC tick the gait table starts at segment
 *                        floor(tick / iterations_between_mpc) mod period (gait.py:76-78).
 *   iterations_between_mpc   linear_mpc_configs.py:7 (20); >= 1
 *   root_states  [B][13], dof_states [B][12][2]   as for mpcqp_kinematics_root_states
 *   geom         as for mpcqp_kinematics
 *   vel_body_des, yaw_rate_des, gait (required), height_des   as for mpcqp_plan
 *   robot        as for mpcqp_solve
 *   plan_state, x0, xref, contact   in/out and out, as for mpcqp_plan
 *   swing_mem    in/out, 16-byte aligned, as for mpcqp_leg_torques
 *   feet         [B][4][3]  out: the `feet` the solve reads (nullable with flags == 0)
 *   u0           [B][12]  in with flags == 0 (the forces of the last solve), out and in with
 *                        MPCQP_STEP_MPC
 *   tau          [B][12]  out, as for mpcqp_leg_torques
 *   status, iters   out (nullable), as for mpcqp_solve; written on an MPC tick only
 *   thighs, pos_feet, foot_pos_base, foot_vel_base, jac   out (nullable), as for mpcqp_kinematics
 *   swing_state, pos_target, vel_target   out (nullable), as for mpcqp_leg_torques
 * With flags == 0, xref, contact, feet, robot, height_des, status and iters may be NULL (none is
 * touched).  MPCQP_ERR_ARG, with nothing written, for unknown flags, batch < 0,
 * iterations_between_mpc < 1, a NULL required pointer (xref, contact, feet, robot and
 * height_des among them with MPCQP_STEP_MPC) and a swing_mem that is not 16-byte aligned;
 * batch == 0 is MPCQP_OK.  The constants are those of mpcqp_set_planner and mpcqp_set_swing. */
#define MPCQP_STEP_MPC 1
int mpcqp_step(mpcqp_ctx* ctx, int32_t batch, int32_t flags, int32_t iter_counter, const int32_t* tick,
               int32_t iterations_between_mpc, const float* root_states, const float* dof_states,
               const double* geom, const double* vel_body_des, const double* yaw_rate_des, const int32_t* gait,
               const float* height_des, const float* robot, double* plan_state, double* swing_mem, float* x0,
               float* xref, float* contact, float* feet, float* u0, float* tau, int32_t* status, int32_t* iters,
               float* thighs, float* pos_feet, float* foot_pos_base, float* foot_vel_base, float* jac,
               float* swing_state, float* pos_target, float* vel_target, void* stream);

/* ---- the base-state estimator on the device: IMU + leg-kinematics Kalman filter ----
 *
 * mpcqp_estimate is one tick, for B robots in one launch, of the linear Kalman filter the
 * reference derives in doc/state_estimation_kf.md (its second stage, after MIT Cheetah 3)
 * and never builds: RobotData.update raises NotImplementedError for state_estimation=True.
 * It fuses the accelerometer with the leg kinematics of the feet in contact, from the
 * sensor set scripts/mujoco_aliengo.py:101-118 collects (IMU quaternion, gyro,
 * accelerometer, joint positions and rates, touch state), and writes a root-state tensor in
 * the layout the *_root_states entry points read, so the estimate feeds them in place.  One
 * launch, no allocation, synchronisation or host read: it can be captured into a HIP graph
 * (the filter's state lives in caller memory, so a replay advances it).  One filter per
 * robot, nothing shared between robots.  Float64 arithmetic on the float32 inputs, each
 * float32 output rounded once.  The orientation (the doc's first stage) and the trust are
 * inputs: mpcqp_attitude computes both from the raw sensors.
 *
 *   state x = [p_b, v_b, p_1, p_2, p_3, p_4] in R^18: base position and velocity and the
 *   four feet (FL, FR, RL, RR), world frame; covariance P 18 x 18.
 *
 *   flags        0 or MPCQP_EST_DOF_STATES
 *   quat         [B][4]  (w, x, y, z), used as given (not normalised); R_q as in mpcqp_kinematics
 *   gyro, accel  [B][3]  angular rate w_b and the accelerometer's specific force a_b, body frame
 *   q, qdot      [B][12] joint angles / rates; with MPCQP_EST_DOF_STATES q is a dof-state
 *                        tensor [B][12][2] and qdot is ignored (may be NULL)
 *   trust        [B][4]  clipped to [0, 1]: 1 = the foot is in contact, 0 = it swings; a
 *                        ramp is allowed (the touch sensor, or swing_state == 0)
 *   geom         [B][MPCQP_KIN_STRIDE]  as for mpcqp_kinematics
 *   est_state    [B][MPCQP_EST_STRIDE] float64 in/out, 16-byte aligned: x[18], initialised
 *                        (0 / 1), 5 x 0, P[18][18] row-major (symmetric) at 24, 4 x 0.  An
 *                        all-zero record is "not initialised": x = 0, P = p0 I.  A caller may
 *                        seed x, P and initialised = 1 itself.  Any non-zero initialised word
 *                        (a NaN included) marks the record initialised; a tick rewrites it to
 *                        1.  The padding words are neither read nor written.
 * Outputs, each nullable:
 *   root_states  [B][13]  pos = p_b, quat (x, y, z, w) copied from the input, lin_vel = v_b,
 *                        ang_vel = R_q w_b (world frame)
 *   feet_world   [B][4][3]  p_1 .. p_4
 *   status       [B]     MPCQP_STATUS_OK, or MPCQP_STATUS_NONFINITE for a robot with a
 *                        non-finite input (quat, gyro, accel, q, qdot, trust, geom[0..4]) or
 *                        an initialised record whose x, P or initialised word is not
 *                        finite: its record is not written and its outputs are formed from
 *                        the record as it was (so a non-finite x is handed on, under this
 *                        status, until the caller reseeds the record); no other robot is
 *                        affected.  A record that is not initialised is not read beyond
 *                        that word
 * The tick, with (p_i, J_i) the foot and its Jacobian in the base frame, t_i the clipped
 * trust, k_i = 1 + (1 - t_i) suspicion and x^-, P^- the record:
 *   r_i = R_q p_i,  rd_i = R_q (w_b x p_i + J_i qdot_i),  a = R_q a_b - (0, 0, g)
 *   y = [-r_i (4 x 3);  (1 - t_i) v_b^- - t_i rd_i (4 x 3);  t_i h + (1 - t_i)(p_b,z^- + r_i,z) (4)]
 *   predict  x = A x^- + B a, P = A P^- A^T + Q;  A = I + dt [p <- v], B = [dt^2/2 I; dt I; 0],
 *            Q = dt diag(sigma_p 1_3, sigma_v 1_3, sigma_f k_i 1_3 ...)
 *   C        rows [I, 0, -I at foot i], [0, I, 0], z of foot i;
 *            R = diag(r_p 1_12, r_v k_i 1_3 ..., r_z k_i ...)
 *   update   K = P C^T (C P C^T + R)^-1, x += K (y - C x), P -= K C P, P <- (P + P^T) / 2
 * carried out as 28 scalar updates (R is diagonal).  The Cheetah software's shrinking of
 * P's xy block is not part of it (deviations).
 *
 * An unknown flag bit, batch <= 0, a NULL required pointer or a misaligned est_state
 * return MPCQP_ERR_ARG. */
#define MPCQP_EST_STRIDE 352      /* doubles per robot: x[18], initialised, 5 x 0, P[18][18] row-major at 24, 4 x 0 */
#define MPCQP_EST_DOF_STATES 1    /* flags: q points at a dof-state tensor [B][12][2] (pos, vel); qdot is ignored */
int mpcqp_estimate(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* quat, const float* gyro,
                   const float* accel, const float* q, const float* qdot, const float* trust,
                   const double* geom, double* est_state, float* root_states, float* feet_world,
                   int32_t* status, void* stream);

/* Estimator constants (doc/state_estimation_kf.md; the noise defaults are the Cheetah 3
 * software's published values folded into rates): the time step dt (0.001) and gravity
 * (9.81), the process rates sigma_p (0.001), sigma_v (0.0098), sigma_f (0.002), the
 * measurement variances r_p (0.001), r_v (0.1), r_z (0.001), the suspicion factor (100)
 * that inflates the noise of a foot that is not trusted, the initial variance p0 (100) and
 * the contact height (0), the world z of a foot in contact.  A non-finite value, dt <= 0,
 * any of r_p, r_v, r_z, p0 <= 0, a sigma < 0 or suspicion < 0 returns MPCQP_ERR_ARG and
 * leaves the previous constants in force. */
int mpcqp_set_estimator(mpcqp_ctx* ctx, double dt, double gravity, double sigma_p, double sigma_v,
                        double sigma_f, double r_p, double r_v, double r_z, double suspicion,
                        double p0, double contact_height);

/* ---- the orientation filter and the contact trust on the device, ahead of the estimator ----
 *
 * mpcqp_attitude produces, for B robots in one launch, the two inputs of mpcqp_estimate a
 * robot's sensors do not deliver: the orientation `quat`, by the gyro / accelerometer filter
 * of doc/state_estimation_kf.md section 2 (the document's first stage), and the contact
 * `trust`, ramped in and out over the stance phase as in the Cheetah 3 filter the document
 * follows and gated by the touch sensor (scripts/mujoco_aliengo.py:101-118, touch_state).  The
 * stance phase is decided on the integers mpcqp_leg_torques decides it on, so trust is 0
 * exactly where that call reports swing_state > 0.  One thread per robot, one launch, no
 * atomics, allocation, synchronisation or host read: it can be captured into a HIP graph (the
 * filter's record lives in caller memory, so a replay advances it).  Float64 arithmetic on the
 * float32 inputs, each float32 output rounded once.
 *
 *   flags        0 (reserved)
 *   gyro, accel  [B][3]  angular rate w_b and the accelerometer's specific force a_b, body
 *                        frame (at rest a_b = R^T (0, 0, g)), as for mpcqp_estimate
 *   tick         [B]     control-iteration counters, as for mpcqp_leg_torques; nullable
 *                        without gait
 *   iterations_between_mpc, gait [B][MPCQP_GAIT_STRIDE]   as for mpcqp_leg_torques; gait nullable
 *   touch        [B][4]  the touch sensor per foot (FL, FR, RL, RR); nullable
 *   att_state    [B][MPCQP_ATT_STRIDE] float64 in/out, 16-byte aligned: q (w, x, y, z),
 *                        initialised (0 / 1), gyro bias b[3].  An all-zero record is "not
 *                        initialised".  A caller may seed q, b and initialised = 1 itself; q
 *                        is normalised by the tick, so any length from 1e-140 to 1e140 will do
 *                        (below, the squares the normalisation sums are subnormal: at 1e-160
 *                        the result is unit to 5e-4 only).
 *                        A seeded q of length 0, or one so long that the tick's products of
 *                        its entries overflow (1e150, say), is misuse: that tick writes a NaN q under
 *                        MPCQP_STATUS_OK, and from the next tick on the robot is refused
 *                        (MPCQP_STATUS_NONFINITE, record unchanged) until it is reseeded
 * Outputs, each nullable (a NULL output is not written):
 *   quat         [B][4]  (w, x, y, z), unit length; its sign is not canonicalised
 *   gyro_out     [B][3]  w_b - b, the input bitwise while b = 0
 *   trust        [B][4]  in [0, 1]; needs gait and tick, or touch
 *   status       [B]     MPCQP_STATUS_OK, or MPCQP_STATUS_NONFINITE for a robot with a
 *                        non-finite gyro, accel, touch or record value: its record is not
 *                        written, quat / gyro_out are formed from the record as it was
 *                        (identity, b = 0 if not initialised), a non-finite touch makes its
 *                        four trusts 0; no other robot is affected
 * The orientation tick, with n = |a_b| and m = a_b / n (n > 0):
 *   record not initialised: q = normalise(1 + m_z, m_y, -m_x, 0), the shortest arc with
 *     R(q)^T e_z = m and zero yaw ((0, 1, 0, 0) for m_z < -1 + 1e-12, identity for n = 0),
 *     b = 0, initialised = 1; no integration on this tick
 *   else  u = R(q)^T e_z (the third row of mpcqp_kinematics' R_q),  e = m x u (0 for n = 0),
 *         gamma = clamp(1 - |n - g| / g, 0, 1) (0 for n = 0): the document's kappa heuristic,
 *         omega = w_b - b + kappa_ref gamma e,   b <- b - bias_gain gamma e dt,
 *         theta = omega dt,  dq = (cos(|theta| / 2), sin(|theta| / 2) theta / |theta|)
 *         ((1, theta / 2) for |theta| < 1e-8),  q <- normalise(q (x) dq)
 * which is the document's R_{k+1} = R_k exp([w_b + kappa w_corr]x dt); the bias term is the
 * integral term of Mahony's filter (the document's ref. [3]) and is off by default.  Yaw is
 * not corrected: it is unobservable without exteroception, as the document says.
 * The trust of a leg, with swing_decide's cs and nsw = (period - dur) ibm (mpcqp_leg_torques):
 *   0 in swing (1 <= cs <= nsw); 1 for a leg that never swings (nsw <= 0) or a malformed record;
 *   in stance nst = dur ibm, k = (cs == 0 ? nst : cs - nsw) in 1 .. nst, phi = (k - 1/2) / nst,
 *   trust = min(1, phi / w, (1 - phi) / w) with w = trust_window (w = 0: 1)
 *   with touch: touch <= touch_threshold forces 0; without gait: trust = (touch > threshold)
 *
 * A non-zero flag, batch <= 0, a NULL gyro, accel or att_state, a misaligned att_state, trust
 * wanted with neither gait and tick nor touch, gait without tick, or iterations_between_mpc
 * < 1 with a gait return MPCQP_ERR_ARG. */
#define MPCQP_ATT_STRIDE 8        /* doubles per robot: q (w, x, y, z), initialised, gyro bias b[3] */
int mpcqp_attitude(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* gyro, const float* accel,
                   const int32_t* tick, int32_t iterations_between_mpc, const int32_t* gait,
                   const float* touch, double* att_state, float* quat, float* gyro_out, float* trust,
                   int32_t* status, void* stream);

/* Constants of mpcqp_attitude: the time step dt (0.001) and gravity (9.81), the correction
 * gain kappa_ref in 1/s (0.1, the document's value), the bias gain (0: no bias estimate), the
 * trust window as a fraction of the stance (0.2) and the touch threshold (0).  A non-finite
 * value, dt <= 0, gravity <= 0, kappa_ref < 0, bias_gain < 0 or a trust_window outside
 * [0, 0.5] returns MPCQP_ERR_ARG and leaves the previous constants in force. */
int mpcqp_set_attitude(mpcqp_ctx* ctx, double dt, double gravity, double kappa_ref, double bias_gain,
                       double trust_window, double touch_threshold);

/* ---- the terrain plane on the device: fit from the stance feet, cones and footholds ----
 *
 * mpcqp_terrain fits, for B robots in one launch, each robot's ground plane to the world
 * positions its four feet had while last in contact: RobotData.update_terrain_normal
 * (utils/robot_data.py:186-228), which the reference defines and never calls.  It produces the
 * surface normal that the cone rows of mpcqp_solve read from words 9..11 of the robot record,
 * and the plane that mpcqp_set_ground hands to the swing leg.  One thread per robot, one
 * launch, no atomics, allocation, synchronisation or host read: it can be captured into a HIP
 * graph (the record lives in caller memory, so a replay advances it).  Float64 arithmetic on
 * the float32 inputs, each float32 output rounded once.
 *
 *   flags          MPCQP_TERRAIN_SWING_STATE: `contact` is the swing_state of mpcqp_leg_torques /
 *                  mpcqp_step, and a foot is in contact where !(swing_state > 0), the leg
 *                  controller's own rule for stance.  Without it a foot is in contact where
 *                  contact > contact_threshold (a NaN is no contact).
 *                  MPCQP_TERRAIN_ROOT_STATES: `quat` is an Isaac Gym root-state tensor [B][13];
 *                  without it [B][4] as (w, x, y, z)
 *                  MPCQP_TERRAIN_GROUND: `plane` is written for mpcqp_set_ground.  The latched
 *                  feet are foot centres, and the swing leg places a foothold at touchdown_z +
 *                  ground(x, y): under this flag the fourth word of `plane` is
 *                  d - n_z touchdown_z (float64 from the record, rounded once; touchdown_z as
 *                  mpcqp_set_swing left it), so that a foothold lies on the fitted plane
 *                  n . p = d itself -- on level ground at the height the feet were latched at,
 *                  as with no ground registered.  The record, `normal`, `normal_base` and
 *                  `robot` are the same with and without it.
 *   pos_feet      [B][4][3]  the feet in the world frame (mpcqp_kinematics' pos_feet,
 *                             mpcqp_estimate's feet_world)
 *   contact        [B][4]
 *   quat           nullable; read for normal_base alone
 *   terrain_state  [B][MPCQP_TERRAIN_STRIDE] float64 in/out, 16-byte aligned: history[4][3] at 0,
 *                  initialised (0 / 1) at 12, n[3] at 13, d at 16, fitted (0 / 1) at 17, two
 *                  zero words.  An all-zero record is "not initialised".
 *   robot          nullable, in/out [B][MPCQP_ROBOT_STRIDE]: words 9..11 are written with
 *                  `normal`, no other word is touched
 * Outputs, each nullable (a NULL output is not written):
 *   normal         [B][3]  n, unit length, n_z > 0
 *   plane          [B][4]  n, d: the plane n . p = d through the centroid of the history
 *                          (n, d - n_z touchdown_z under MPCQP_TERRAIN_GROUND)
 *   normal_base    [B][3]  R_base^T n (terrain_normal_est_yaw_aligned, :227), R_base the float32
 *                          quat2matrix of mpcqp_plan; needs quat
 *   status         [B]     MPCQP_STATUS_OK, or MPCQP_STATUS_NONFINITE for a robot with a
 *                          non-finite foot among those it would latch, or a non-finite word in
 *                          an initialised record: its record is not written and its outputs are
 *                          formed from the record as it was ((0, 0, 1) and d = 0 if not
 *                          initialised); no other robot is affected.  A non-finite foot that
 *                          is not latched is ignored.
 * One tick, with c_i the contact decision of foot i:
 *   latch   a record not initialised takes all four feet, whatever c_i says, and n = (0, 0, 1);
 *           an initialised one takes foot i where c_i holds
 *   fit     mu = the mean of the history, S = sum_i (h_i - mu)(h_i - mu)^T; l0 <= l1 <= l2 its
 *           eigenvalues and n_fit the eigenvector of l0 (6 cyclic Jacobi sweeps), flipped to
 *           n_z >= 0
 *   accept  l2 > 0, l1 - l0 > flat_tol l2 (the points span a plane: they are not collinear or
 *           coincident) and n_fit_z >= cos_max_tilt:
 *           n <- normalise((1 - blend) n + blend n_fit), fitted = 1; otherwise n stays, fitted = 0
 *   d = n . mu either way
 * Two deviations from the reference, which takes a row of numpy's eigenvector matrix where the
 * eigenvector is the column, and whose seeding of the history is a no-op comparison so that it
 * starts from four zero points: this is the column, and the first tick seeds all four feet.
 * cos_max_tilt > 0 also keeps the normal off world +-x, where the solve's cone rows have no
 * tangent frame.
 *
 * An unknown flag, batch < 0, a NULL pos_feet, contact or terrain_state, a misaligned
 * terrain_state or normal_base without quat return MPCQP_ERR_ARG; batch == 0 is MPCQP_OK. */
#define MPCQP_TERRAIN_STRIDE 20      /* doubles per robot */
#define MPCQP_TERRAIN_SWING_STATE 1
#define MPCQP_TERRAIN_ROOT_STATES 2
#define MPCQP_TERRAIN_GROUND 4
int mpcqp_terrain(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* pos_feet, const float* contact,
                  const float* quat, double* terrain_state, float* robot, float* normal, float* plane,
                  float* normal_base, int32_t* status, void* stream);

/* Constants of mpcqp_terrain: the contact threshold (0.5), flat_tol (1e-3), the cosine of the
 * steepest plane accepted (0.5) and the weight of a new fit in n (1: no filter, as the
 * reference).  A non-finite value, flat_tol outside [0, 1), cos_max_tilt outside (0, 1] or
 * blend outside (0, 1] returns MPCQP_ERR_ARG and leaves the previous constants in force. */
int mpcqp_set_terrain(mpcqp_ctx* ctx, double contact_threshold, double flat_tol, double cos_max_tilt,
                      double blend);

/* The swing leg's ground: `plane` is a caller-owned device buffer [capacity][4] of (n, d), what
 * mpcqp_terrain writes, read by every later mpcqp_leg_torques* and mpcqp_step launch; it must
 * outlive them.  Robot b < capacity in swing places its foothold at
 * z = touchdown_z + ground(x, y), ground(x, y) = (d - n_x x - n_y y) / n_z, and its swing apex
 * at swing_height + (ground(lift-off) + ground(foothold)) / 2.  A plane that is non-finite or
 * has n_z <= 0 counts as none, as does b >= capacity: that robot walks on the reference's flat
 * ground, bitwise as with nothing registered.  Stance legs do not read it.  ground(x, y) is
 * the height of the surface under a foot whose centre rides -touchdown_z above it; a plane
 * fitted through foot centres (mpcqp_terrain) is handed over with MPCQP_TERRAIN_GROUND, which
 * subtracts n_z touchdown_z from d so that the foothold lies on the fitted plane.  NULL or capacity 0
 * disables; capacity < 0, or a NULL plane with capacity > 0, returns MPCQP_ERR_ARG. */
int mpcqp_set_ground(mpcqp_ctx* ctx, const float* plane, int32_t capacity);

/* The predicted trajectory of a force sequence, its cost and cone margin (mpcqp_predict) are
 * declared in mpcqp_predict_abi.h, which includes this file. */

int mpcqp_destroy(mpcqp_ctx* ctx);

const char* mpcqp_last_error(const mpcqp_ctx* ctx);

int32_t mpcqp_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* MPCQP_H */

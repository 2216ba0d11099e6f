/*
 * mpcqp_plant_abi.h -- C ABI of the MI355X engine, part 3: what the joint torques do.
 *
 * A companion of mpcqp.h (same library, same context, same ABI version, same conventions:
 * device pointers owned by the caller, asynchronous on `stream`, MPCQP_OK or a negative error
 * code, mpcqp_last_error() for the text).  mpcqp.h declares the control path from the
 * simulator's state tensors to the joint torques; this header declares the stage that turns
 * the torques back into those tensors, which the reference's scripts hand to a simulator
 * (gym.simulate, sim.step()).  A caller includes this file alone: it includes mpcqp.h.
 */
#ifndef MPCQP_PLANT_ABI_H
#define MPCQP_PLANT_ABI_H

#include "mpcqp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rigid-body plant on the device: one control iteration of every robot's physics ----
 *
 * mpcqp_plant advances, for B robots in one launch, each robot's physical state by dt_control
 * under the joint torques it is given and writes the next root_states / dof_states in the
 * simulator's layout with the raw sensors, so that mpcqp_step -> mpcqp_plant -> mpcqp_step runs
 * with nothing on the host.  The model is the one the MPC assumes, with the nonlinear rotation
 * kept and the contact decided by the ground instead of the gait table: a single rigid body on
 * four massless legs with point feet of mass foot_mass.  Per substep of h = dt_control / substeps
 * and per leg, with Rq the rotation of the record's quaternion: q = ik(Rq^T (p_f - pos)),
 * g = (Rq J_b(q))^-T tau_leg is the force the leg puts on its foot.
 *   a foot in contact   the ground reaction is f = -g.  n . f <= 0 releases the foot: it goes on
 *                       as a free foot in the same substep, from rest.  Otherwise the tangential
 *                       part is scaled back onto the cone |f_t| <= mu n . f and the foot stays
 *                       pinned: sliding is not modelled.  The body receives f at the foot
 *   a free foot         a point mass under g plus gravity, semi-implicit Euler (v_f += h a,
 *                       p_f += h v_f); the body receives -g at the foot.  Below the plane and
 *                       moving into it afterwards, the foot is projected onto the plane, stopped
 *                       and marked in contact
 *   the body            v += h (sum F / m + gravity), pos += h v; the attitude turns by
 *                       exp(h w*), w* = w + h I_w^-1 (sum r x F - w x I_w w), I_w = Rq I Rq^T, and
 *                       the angular momentum I_w w + h sum r x F is carried through the turn
 *                       (w = I_w'^-1 of it on the new attitude), so free flight conserves it
 * One lane per leg, a robot's legs in adjacent lanes, their forces summed by cross-lane moves;
 * no LDS, atomics, allocation, synchronisation or host read: it can be captured into a HIP
 * graph.  Float64 arithmetic; each float32 output rounded once.
 *
 *   flags        0 (reserved)
 *   tau          [B][12]  joint torques (hip, thigh, calf per leg FL, FR, RL, RR), mpcqp_step's
 *   robot        [B][MPCQP_ROBOT_STRIDE] as for mpcqp_solve: mass, the inertia and mu are read,
 *                        the normal is not
 *   geom         [B][MPCQP_KIN_STRIDE] as for mpcqp_kinematics
 *   plane        [B][4] (n, d), the ground n . p = d per robot, in mpcqp_set_ground's convention
 *                        (n unit length); NULL: level ground at the constant ground_z
 *   plant_state  [B][MPCQP_PLANT_STRIDE] float64, in/out, 16-byte aligned: pos 3, quat (w, x, y,
 *                        z) 4, lin_vel 3, ang_vel 3 (world frame), foot positions 12 (world),
 *                        foot velocities 12, contact 4 (0 / 1), the flag word (bit l: an inverse-
 *                        kinematics clamp bit on leg l during this call -- the foot beyond the
 *                        leg's reach, folded onto the thigh joint or inside the hip's cylinder;
 *                        cos(calf) is held in [-1 + 2^-90, 1 - 2^-90]), the count of calls; words
 *                        43..47 are kept
 * Outputs:
 *   root_states  [B][13]  pos, quat (x, y, z, w), lin_vel, ang_vel (world frame)
 *   dof_states   [B][12][2]  (q, qdot) per joint, 8-byte aligned: q = ik(Rq^T (p_f - pos)),
 *                        qdot = J_b^-1 Rq^T (v_f - v - w x (p_f - pos))
 *   gyro         [B][3]  nullable: Rq^T w
 *   accel        [B][3]  nullable: Rq^T (a_body - gravity vector), the last substep's; at rest on
 *                        level ground (0, 0, +g)
 *   touch        [B][4]  nullable: the contact flags, 0 / 1
 *   status       [B]     nullable: MPCQP_STATUS_OK, or MPCQP_STATUS_NONFINITE for a robot with a
 *                        non-finite torque, a non-finite or non-invertible record (robot[0..7],
 *                        geom, plane, plant_state; mass <= 0, a singular inertia, a zero
 *                        quaternion) or a non-finite result: its plant_state is untouched and
 *                        its outputs are rewritten from the untouched record (accel as at rest);
 *                        no other robot is affected
 * dt_control and gravity are mpcqp_set_planner's.  A non-zero flag, batch < 0, a NULL tau, robot,
 * geom, plant_state, root_states or dof_states, or a misaligned plant_state or dof_states return
 * MPCQP_ERR_ARG with nothing written; batch == 0 is MPCQP_OK. */
#define MPCQP_PLANT_STRIDE 48
#define MPCQP_PLANT_MAX_SUBSTEPS 16
int mpcqp_plant(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* tau, const float* robot,
                const double* geom, const float* plane, double* plant_state, float* root_states,
                float* dof_states, float* gyro, float* accel, float* touch, int32_t* status, void* stream);

/* Fills records from a pose given in the loop's own tensors (a device launch, one thread per
 * robot): the body from root_states, the feet by forward kinematics of dof_states' angles
 * (their rates are not read), foot velocities zero, contact where n . p_f - d <= contact_tol,
 * flag word and call count zero.  plane as for mpcqp_plant.  batch < 0, a NULL root_states,
 * dof_states, geom or plant_state, or a misaligned plant_state return MPCQP_ERR_ARG with nothing
 * written; batch == 0 is MPCQP_OK. */
int mpcqp_plant_reset(mpcqp_ctx* ctx, int32_t batch, const float* root_states, const float* dof_states,
                      const double* geom, const float* plane, double* plant_state, void* stream);

/* The plant's constants: the mass of a foot (default 0.15 kg), the substeps per call (1, at most
 * MPCQP_PLANT_MAX_SUBSTEPS), the height of the level ground used without a plane (default: the
 * swing leg's touchdown_z, followed until this call sets a value) and the distance from the
 * plane within which mpcqp_plant_reset marks a foot in contact (1e-4).  A non-finite value, a
 * non-positive foot_mass or substeps outside 1..16 return MPCQP_ERR_ARG and the constants stay. */
int mpcqp_set_plant(mpcqp_ctx* ctx, double foot_mass, int32_t substeps, double ground_z, double contact_tol);

#ifdef __cplusplus
}
#endif

#endif /* MPCQP_PLANT_ABI_H */

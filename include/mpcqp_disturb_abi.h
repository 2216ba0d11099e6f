/*
 * mpcqp_disturb_abi.h -- C ABI of the MI355X engine, part 6: what disturbs a robot -- sensors that
 * are not exact, and a shove.
 *
 * A companion of mpcqp.h (same library, same context, same ABI version, same conventions:
 * device pointers owned by the caller, asynchronous on `stream`, MPCQP_OK or a negative error
 * code, mpcqp_last_error() for the text).  mpcqp_plant_abi.h declares the plant, whose sensors
 * are exact and which takes torques and nothing else; this header declares the stage between
 * the plant and the sensing chain (mpcqp_attitude, mpcqp_estimate) and an impulse on the plant's
 * record.  The reference has neither: its scripts read a simulator's sensors as they come
 * (gym.simulate, sim.step()).  A caller includes this file alone: it includes mpcqp.h.
 */
#ifndef MPCQP_DISTURB_ABI_H
#define MPCQP_DISTURB_ABI_H

#include "mpcqp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the sensor model on the device: noisy IMU, encoders, touch ----
 *
 * mpcqp_sensors turns, for B robots in one launch per control iteration, the plant's exact
 * gyro / accel / dof_states / touch into what sensors would report, reproducible word for word
 * from a seed.  Per robot, with s its scale (1 without `scale`), dt = dt_control and z standard
 * normals:
 *   record not initialised   b_g = s bias0_gyro z_walk, b_a likewise (the turn-on bias); each
 *                            foot's history has all 32 bits set to the current reading, so the
 *                            start makes no edges; initialised = 1; no walk in this call
 *   record initialised       b += s walk sqrt(dt) z_walk
 *   always                   gyro_m = f32(gyro + (b_g + s sigma_gyro z)), accel likewise;
 *                            q_m = q + s sigma_q z, then rint(q_m / q_lsb) q_lsb when q_lsb > 0;
 *                            qdot_m = qdot + s sigma_qd z;
 *                            hist_f = ((hist_f << 1) | (touch_f > 0)) mod 2^32, the reading is
 *                            bit touch_lag of it, 1.0 or 0.0, and 0.0 where it is dropped;
 *                            count += 1
 * A term that is zero is not added, so with every constant zero gyro_m, accel_m and dof_states_m
 * are their inputs bit by bit.  Float64 arithmetic on the float32 inputs; each float32 output
 * rounded once.
 *
 * The generator is Philox4x32-10 and has no state but the record's count: block j = 0..15 of a
 * call has the counter (count mod 2^32, count div 2^32, id, j) and the key (seed mod 2^32, seed
 * div 2^32).  A word w gives u = (w + 0.5) 2^-32; a pair (w0, w1) gives two normals by
 * Box-Muller in float64, r = sqrt(-2 ln u0), z0 = r cos 2 pi u1, z1 = r sin 2 pi u1 (|z| <= 6.77);
 * ln, sin and cos are evaluated by IEEE operations spelled out in the engine (within 1e-15 of the
 * exact value), not by a library, so every build of it gives the same bits.
 *   block j = 0..11   joint j: words 0, 1 give (z for q, z for qdot); words 2, 3 are not used
 *   block 12 + a      IMU axis a: words 0, 1 give (gyro white, accel white), words 2, 3 (gyro
 *                     walk, accel walk)
 *   block 15          word f is foot f's dropout draw: dropped iff word < floor(p_drop 2^32)
 * The draws and the record's advance do not depend on which groups are NULL (without touch the
 * histories stay as they are).  16 lanes per robot, a lane per block; the robot-wide refusal is
 * a vote of the 16 lanes; no LDS, atomics, allocation, synchronisation or host read: it can be
 * captured into a HIP graph, and since the record lives in caller memory a replay advances it.
 *
 *   flags        0 (reserved)
 *   gyro, accel  [B][3]      float32, the plant's; each nullable together with its output
 *   dof_states   [B][12][2]  (q, qdot) per joint, 8-byte aligned; nullable with its output
 *   touch        [B][4]      > 0: contact; nullable with its output
 *   scale        [B]         float32, nullable: multiplies every sigma, walk and bias0 of that
 *                            robot; not q_lsb, touch_lag or p_drop
 *   sense_state  [B][MPCQP_SENSE_STRIDE] float64, in/out, 16-byte aligned: b_g 3, b_a 3,
 *                            initialised, the count of accepted calls, the robot's id, the four
 *                            feet's histories (integers below 2^32 held exactly); words 13..15
 *                            are kept.  All-zero but for the id is the start.  The id is read
 *                            from the record, not from the launch's row, so a call on rows
 *                            [k, B) through offset pointers draws what the whole-batch call draws
 * Outputs, the shapes of their inputs; an output may be its input buffer:
 *   gyro_m, accel_m, dof_states_m, touch_m
 *   status       [B]  nullable: MPCQP_STATUS_OK, or MPCQP_STATUS_NONFINITE for a robot with a
 *                            non-finite input, a non-finite or negative scale, a non-finite
 *                            record word 0..12, a count outside [0, 2^53) or an id or history
 *                            outside [0, 2^32): its record is untouched, count included, its
 *                            outputs are its inputs; no other robot is affected
 * dt_control is mpcqp_set_planner's.  A non-zero flag, batch < 0, a NULL sense_state, an input
 * without its output or an output without its input, or a misaligned sense_state, dof_states or
 * dof_states_m return MPCQP_ERR_ARG with nothing written; batch == 0 is MPCQP_OK. */
#define MPCQP_SENSE_STRIDE 16
int mpcqp_sensors(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* gyro, const float* accel,
                  const float* dof_states, const float* touch, const float* scale, double* sense_state,
                  float* gyro_m, float* accel_m, float* dof_states_m, float* touch_m, int32_t* status, void* stream);

/* The sensor model's constants, held by the context (the reference's scripts take a simulator's
 * sensors as they are: gym.simulate, sim.step()): the seed; white noise per sample of the gyro
 * (rad/s) and the accelerometer (m/s^2); their bias random walks per sqrt(s); their turn-on
 * biases (1 sigma); the encoders' white noise on q (rad) and qdot (rad/s) and the encoder step
 * q_lsb (rad; 0: not quantised); the touch sensors' lag in calls, 0..31, and the probability that
 * a reading is dropped, in [0, 1).  All default to zero.  A non-finite or negative value, a
 * touch_lag outside 0..31 or a p_drop outside [0, 1) return MPCQP_ERR_ARG and the previous
 * constants stay.  Launches already enqueued keep the constants they were given. */
int mpcqp_set_sensors(mpcqp_ctx* ctx, uint64_t seed, double sigma_gyro, double sigma_accel, double walk_gyro,
                      double walk_accel, double bias0_gyro, double bias0_accel, double sigma_q, double sigma_qd,
                      double q_lsb, int32_t touch_lag, double p_drop);

/* ---- a push: an impulse on the plant's record ----
 *
 * One launch, one thread per robot (the reference's scripts never disturb the robot:
 * gym.simulate, sim.step()): v += J / m and w += I_w^-1 ((Rq r) x J), with Rq the rotation of the
 * record's quaternion and I_w = Rq I Rq^T from the robot record, exactly as mpcqp_plant forms it.
 * Feet, contacts, flag word and call count are not written: a pinned foot stays pinned, which
 * is the plant's model.  A zero impulse leaves the record bit by bit.  A force F over a tick is
 * the impulse F dt_control, given every tick; the plant's accelerometer does not see an impulse.
 *
 *   impulse      [B][3]  float32, world frame, N s
 *   point        [B][3]  float32, nullable: where it acts, in the body frame from the centre of
 *                        mass; NULL: at the centre of mass (the rate is then not written)
 *   robot        [B][MPCQP_ROBOT_STRIDE] as for mpcqp_plant: mass and inertia are read
 *   plant_state  [B][MPCQP_PLANT_STRIDE] float64, in/out, 16-byte aligned: mpcqp_plant's
 *   status       [B]     nullable: MPCQP_STATUS_OK, or MPCQP_STATUS_NONFINITE for a robot with a
 *                        non-finite impulse or point, a non-finite or non-invertible record
 *                        (robot[0..7], plant_state; mass <= 0, a singular inertia, a zero
 *                        quaternion) or a non-finite result: its plant_state is untouched; no
 *                        other robot is affected
 * batch < 0, a NULL impulse, robot or plant_state, or a misaligned plant_state return
 * MPCQP_ERR_ARG with nothing written; batch == 0 is MPCQP_OK.  No allocation, synchronisation
 * or host read: it can be captured into a HIP graph. */
int mpcqp_push(mpcqp_ctx* ctx, int32_t batch, const float* impulse, const float* point, const float* robot,
               double* plant_state, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MPCQP_DISTURB_ABI_H */

/*
 * mpcqp_gait_abi.h -- C ABI of the MI355X engine, part 5: which gait each robot walks, and when
 * it changes.
 *
 * A companion of mpcqp.h (same library, same context, same ABI version, same conventions:
 * device pointers owned by the caller, asynchronous on `stream`, MPCQP_OK or a negative error
 * code, mpcqp_last_error() for the text).  mpcqp.h's control calls take a per-robot gait record
 * and a per-robot control-iteration counter; this header declares the stage that owns the two.
 * A caller includes this file alone: it includes mpcqp.h.
 */
#ifndef MPCQP_GAIT_ABI_H
#define MPCQP_GAIT_ABI_H

#include "mpcqp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the gait scheduler on the device: per-robot gait switches at safe ticks ----
 *
 * The reference changes gait by hand: scripts/mujoco_aliengo.py:121-155 stands under
 * Gait.STANDING, then builds fresh objects and restarts iter_counter at 0 under Gait.TROTTING10;
 * within one Gait the clock is Gait.set_iteration and the swing state Gait.get_swing_state
 * (gait.py:76-121).  mpcqp_gait_schedule does both for B robots in one launch per control
 * iteration: it advances each robot's counter and replaces a robot's record by a library entry
 * only at a tick where that cuts no swing.  All quantities are integers.  With a record
 * g = (P, off[4], dur[4]), ibm = iterations_between_mpc and the counters cs, nsw of
 * mpcqp_leg_torques (cs = (tick mod ibm P) shifted by (off + dur) ibm, nsw = (P - dur) ibm):
 *   mid-swing   leg l at tick t: it swings at all and 1 <= cs < nsw.  cs == 0 (about to lift),
 *               cs > nsw (stance) and cs == nsw (its last swing tick) are not mid-swing
 *   seam        t is a seam of g: t mod ibm == 0 and no leg is mid-swing at t
 *   entry       e(g): the smallest s in [0, P) such that s ibm is a seam of g; it does not depend
 *               on ibm and is 0 for every member of the reference's Gait
 *   switch      robot b, with a request w != current at its tick t (after this call's advance),
 *               switches iff since >= min_hold and t is a seam of gait[b] as it lies there:
 *               gait[b] = library[w], tick[b] = e(library[w]) ibm, the four armed slots of
 *               swing_mem[b] (word 8 l of leg l) = 0 and no other word of it, current = w,
 *               since = 0, switches += 1.  Otherwise the request stays latched and only the clock
 *               advances
 * A switch leaves tick[b] mod ibm as it was, so one fleet-wide MPCQP_STEP_MPC decision stays
 * right for every robot; and the leg controller sees no swing that begins anywhere but at its
 * first tick, but for the single cs == nsw tick at an entry, which the reference's own tick 0 has.
 */
#define MPCQP_GAIT_MAX 16
#define MPCQP_SCHED_STRIDE 8
#define MPCQP_GAIT_ADVANCE 1

/* Sets the library, held by the context like the swing constants: the records a robot can be
 * switched to (the reference's are the members of Gait, gait.py:16-22, read by gait.py:76-121;
 * scripts/mujoco_aliengo.py:121-155 picks two of them by hand): records [count][MPCQP_GAIT_STRIDE] int32 on the host, 1 <= count <=
 * MPCQP_GAIT_MAX.  Each record must have 1 <= P <= 2048, 0 <= dur_l <= P, |off_l| <= 4 P and an
 * entry segment, which is stored beside it.  Anything else returns MPCQP_ERR_ARG and the
 * previous library stays.  Launches already enqueued keep the library they were given. */
int mpcqp_set_gaits(mpcqp_ctx* ctx, int32_t count, const int32_t* records);

/* The scheduler's constants (scripts/mujoco_aliengo.py:121-155 switches on a fixed iteration
 * count instead, and gait.py:76-121 knows one gait).  min_hold >= 0: control iterations a robot keeps a gait before it may switch
 * again (default 0).  idle_gait = -1 disables the automatic choice (the default; the other
 * values are then only checked to be finite); otherwise idle_gait and move_gait must lie in the
 * library, 0 <= v_stop <= v_go (m/s), 0 <= w_stop <= w_go (rad/s) and dwell >= 0 (calls), all
 * finite.  Anything else returns MPCQP_ERR_ARG and the previous constants stay.  A later
 * mpcqp_set_gaits that drops idle_gait or move_gait from the library disables the automatic
 * choice. */
int mpcqp_set_gait_schedule(mpcqp_ctx* ctx, int32_t min_hold, int32_t idle_gait, int32_t move_gait, double v_go,
                            double v_stop, double w_go, double w_stop, int32_t dwell);

/* One launch; no allocation, synchronisation or host read: it can be captured into a HIP graph
 * (gait.py:76-121, scripts/mujoco_aliengo.py:121-155).
 *
 *   flags        MPCQP_GAIT_ADVANCE: add 1 to each robot's tick and `since` before deciding;
 *                        every call but the first after a reset passes it
 *   iterations_between_mpc   >= 1, as for mpcqp_leg_torques
 *   want         [B] int32, nullable: the library index the caller wants per robot, latched in
 *                        the record until honoured or replaced; -1: no new request (an earlier
 *                        one stays latched; asking for the current index withdraws it); any
 *                        other value outside the library: MPCQP_STATUS_UNSUPPORTED for that
 *                        robot, treated as no new request.  NULL: the automatic choice, from
 *   vel_body_des [B][3], yaw_rate_des [B]   float64, mpcqp_plan's, required when want is NULL:
 *                        move_gait when vx^2 + vy^2 > v_go^2 or |yaw| > w_go; idle_gait once the
 *                        command has been at or below both stop thresholds for `dwell`
 *                        consecutive calls, this one included; in between the latched request is
 *                        kept and the calm count restarts.  A non-finite command:
 *                        MPCQP_STATUS_NONFINITE, and nothing about that robot changes but its
 *                        clock
 *   sched_state  [B][MPCQP_SCHED_STRIDE] int32, in/out, 16-byte aligned: the current library
 *                        index (-1: the record was set by hand; the seam test always uses gait[b]
 *                        as it lies there), the latched request, `since` (control iterations
 *                        since the last switch, saturating), `switches`, the calm count, the
 *                        robot's tick just before its last switch; words 6 and 7 are kept.
 *                        All-zero is a valid start: library entry 0, nothing pending
 *   gait         [B][MPCQP_GAIT_STRIDE], tick [B]   int32, in/out: what mpcqp_step,
 *                        mpcqp_leg_torques and mpcqp_attitude take
 *   swing_mem    [B][MPCQP_SWING_STRIDE] float64, in/out, nullable, 16-byte aligned: only the
 *                        armed slots of a robot that switches are written; NULL: they are the
 *                        caller's business
 * Outputs, each nullable:
 *   iteration    [B]     (tick / ibm) mod P after this call, what mpcqp_plan takes; written for
 *                        every robot, and the one output that costs every robot divisions
 *   switched     [B]     1 where this call switched, else 0
 *   status       [B]     MPCQP_STATUS_OK; MPCQP_STATUS_UNSUPPORTED for a want outside the
 *                        library, or for a robot whose tick is negative or is INT32_MAX under
 *                        MPCQP_GAIT_ADVANCE, which is left untouched; MPCQP_STATUS_NONFINITE as
 *                        above.  No other robot is affected
 * A robot that does not switch stores only its clock words.  Unknown flags, batch < 0,
 * iterations_between_mpc < 1, a NULL sched_state, gait or tick, no library set, want NULL with
 * the automatic choice disabled or without vel_body_des and yaw_rate_des, a misaligned
 * sched_state or swing_mem, or an entry tick e(g) iterations_between_mpc beyond INT32_MAX return
 * MPCQP_ERR_ARG with nothing written; batch == 0 is MPCQP_OK. */
int mpcqp_gait_schedule(mpcqp_ctx* ctx, int32_t batch, int32_t flags, int32_t iterations_between_mpc,
                        const int32_t* want, const double* vel_body_des, const double* yaw_rate_des,
                        int32_t* sched_state, int32_t* gait, int32_t* tick, double* swing_mem, int32_t* iteration,
                        int32_t* switched, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MPCQP_GAIT_ABI_H */

/*
 * mpcqp_predict_abi.h -- C ABI of the MI355X engine, part 2: what a force sequence does.
 *
 * A companion of mpcqp.h (same library, same context, same ABI version, same conventions:
 * device pointers owned by the caller, asynchronous on `stream`, MPCQP_OK or a negative error
 * code, mpcqp_last_error() for the text).  mpcqp.h declares the control path; this header
 * declares the evaluation of its result.  A caller includes this file alone: it includes
 * mpcqp.h.
 */
#ifndef MPCQP_PREDICT_ABI_H
#define MPCQP_PREDICT_ABI_H

#include "mpcqp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the predicted trajectory on the device: states, cost, cone margin ----
 *
 * mpcqp_predict evaluates, for B robots in one launch, what a force sequence U does under the
 * model of mpcqp_solve: the state trajectory the QP believes it has planned,
 *   com_traj = Sx @ xt + Su @ contact_forces        linear_mpc/mpc.py:293-294
 * (ModelPredictiveController.__visulize_com_traj_solution, the reference's debug plot), its
 * tracking cost, and how close U sits to its friction cones -- all from U alone, independent of
 * the solver's internal state, so that a caller can grade any iterate (one returned under
 * MPCQP_STATUS_MAX_ITER included).  Sx and Su (13N x 12N per robot) are never built: A_d - I is
 * nilpotent, so the rollout is two running sums of U.  One wavefront per robot, one launch, no
 * atomics, allocation, synchronisation or host read: it can be captured into a HIP graph.
 * Float64 arithmetic on the float32 inputs with the model's float32 roundings (cos / sin of the
 * yaw, I_w, its inverse, inv(I_w)[r]x and 1/m, mpc.py:178-190); each float32 output rounded once.
 *
 *   flags        0 (reserved)
 *   x0, xref, contact, feet, robot   as for mpcqp_solve, read the same way (16-byte chunk loads)
 *   U            [B][N][12]  the sequence to evaluate, usually mpcqp_solve's output; every entry
 *                        is used as given, swing-leg entries included (Su @ contact_forces does
 *                        not mask them either).  Staged like the other inputs: up to 12 bytes
 *                        either side of a robot's slice are read and ignored
 * N, dt and the weights (diagonal, or full through mpcqp_set_weights) are the context's.
 * Outputs, each nullable (a NULL output is not written; with all three NULL nothing is launched):
 *   X            [B][N][13]  x_1 .. x_N, laid out as xref:
 *                        x_{t+1} = x0 + (t+1) n1 + C(t+1, 2) n2 + X0 P0_t + X1 P1_t,
 *                        P0_t = sum_{j<=t} u_j,  P1_t = sum_{j<=t} (t - j) u_j = P1_{t-1} + P0_{t-1}
 *                        with n1 = (A_d - I) x0, n2 = (A_d - I)^2 x0, X0 = B_d, X1 = (A_d - I) B_d;
 *                        component 12 stays x0[12]
 *   report       [B][MPCQP_PREDICT_REPORT] float64:
 *                        0  J = sum_t e_t^T Q e_t + sum_t u_t^T R u_t, e_t = x_{t+1} - xref_t taken
 *                           before the float32 rounding of X
 *                        1  J_free, the same for U = 0: J - J_free = 1/2 U^T H U + g^T U, the QP's
 *                           objective, so an optimum has J <= J_free (U = 0 is feasible)
 *                        2  the cone margin: the smallest slack over the six one-sided rows (four
 *                           pyramid rows, n.f >= 0, contact * fz_max - n.f >= 0, in the frame of
 *                           robot[9..11]) of every foot-step with contact > 0; >= 0 means
 *                           feasible, +inf without a stance foot-step
 *                        3  the swing residual: the largest |U| entry among foot-steps whose
 *                           contact is not > 0; 0 for anything mpcqp_solve wrote
 *   status       [B]     MPCQP_STATUS_OK, or MPCQP_STATUS_NONFINITE for a robot with an input
 *                        mpcqp_solve refuses, a non-finite U entry, or a non-finite result from
 *                        finite inputs (mass 0, a singular inertia): its X and report are all
 *                        zeros; no other robot is affected
 * A non-zero flag, batch < 0 or a NULL x0, xref, contact, feet, robot or U return MPCQP_ERR_ARG;
 * batch == 0 is MPCQP_OK. */
#define MPCQP_PREDICT_REPORT 4
int mpcqp_predict(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* x0, const float* xref,
                  const float* contact, const float* feet, const float* robot, const float* U, float* X,
                  double* report, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MPCQP_PREDICT_ABI_H */

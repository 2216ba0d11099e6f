/*
 * mpcqp_certify_abi.h -- C ABI of the MI355X engine, part 4: how far a force sequence is from the
 * optimum.
 *
 * A companion of mpcqp.h (same library, same context, same ABI version, same conventions:
 * device pointers owned by the caller, asynchronous on `stream`, MPCQP_OK or a negative error
 * code, mpcqp_last_error() for the text).  mpcqp_predict_abi.h says what a force sequence does;
 * this header grades it.  A caller includes this file alone: it includes mpcqp.h.
 */
#ifndef MPCQP_CERTIFY_ABI_H
#define MPCQP_CERTIFY_ABI_H

#include "mpcqp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the optimality certificate on the device: gradient and duality gap of U ----
 *
 * mpcqp_certify evaluates, for B robots in one launch, the gradient of the QP's objective
 *   phi(U) = J - J_free = 1/2 U^T H U + g^T U          (J, J_free: mpcqp_predict's report)
 * at a force sequence U, and from it a bound on phi(U) - phi*, the distance to the optimum of
 * mpcqp_solve's QP -- all from U alone, independent of the solver's internal state, so that a
 * caller can grade any iterate (one returned under MPCQP_STATUS_MAX_ITER included) of any solver
 * class.  H, g and Su are never built: the gradient is the adjoint of mpcqp_predict's two running
 * sums, a backward scan.  One wavefront per robot, one launch, no atomics, allocation,
 * synchronisation or host read: it can be captured into a HIP graph.  Float64 arithmetic on the
 * float32 inputs with the model's float32 roundings, as mpcqp_predict.
 *
 *   flags        0 (reserved)
 *   x0, xref, contact, feet, robot, U   as for mpcqp_predict, read the same way (16-byte chunk
 *                        loads: up to 12 bytes either side of a robot's slice are read and
 *                        ignored); every entry of U is used as given, swing-leg entries included
 * N, dt and the weights (diagonal, or full through mpcqp_set_weights) are the context's.
 * Outputs, each nullable (a NULL output is not written; with all three NULL nothing is launched):
 *   G            [B][N][12]  grad phi = H U + g, laid out as U, each entry rounded once:
 *                        G_j  = 2 (X0^T S0_j + X1^T S1_j) + 2 (R u)_j,   X0 = B_d, X1 = (A_d - I) B_d,
 *                        S0_j = sum_{t>=j} Q e_t,  S1_j = sum_{t>=j} (t - j) Q e_t = S1_{j+1} + S0_{j+1},
 *                        e_t = x_{t+1} - xref_t in float64
 *   report       [B][MPCQP_CERTIFY_REPORT] float64:
 *                        0  the objective phi(U); report[0] - report[1] of mpcqp_predict
 *                        1  the gap: sum over the 4 N foot-steps of g_k . u_k - m_k, where m_k is
 *                           the smallest value g_k . v takes over the foot-step's feasible set:
 *                           for contact > 0 the friction pyramid in the frame (t1, t2, n) of
 *                           robot[9..11] cut off at ub = max(0, contact * fz_max),
 *                             m_k = min(0, ub (g_k.n - mu |g_k.t1| - mu |g_k.t2|)),
 *                           and 0 for any other foot-step (the QP forces it to 0)
 *                        2  lower = objective - gap.  phi is convex, so lower <= phi* for any finite
 *                           U, feasible or not; for a feasible U (mpcqp_predict: cone margin >= 0,
 *                           swing residual 0)  0 <= phi(U) - phi* <= gap
 *                        3  the largest single foot-step term g_k . u_k - m_k
 *                        The gap is a first-order bound.  It is tight at the optimum and loose
 *                        far from it: it needs no multiplier estimate and no active-set tolerance,
 *                        and in exchange it overstates the suboptimality of a U that is far from
 *                        the optimum by a large factor.
 *   status       [B]     MPCQP_STATUS_OK, or MPCQP_STATUS_NONFINITE for a robot with an input
 *                        mpcqp_solve refuses, a non-finite U entry, or a non-finite result from
 *                        finite inputs (mass 0, a singular inertia): its G and report are all
 *                        zeros; no other robot is affected
 * A non-zero flag, batch < 0 or a NULL x0, xref, contact, feet, robot or U return MPCQP_ERR_ARG
 * with nothing written; batch == 0 is MPCQP_OK. */
#define MPCQP_CERTIFY_REPORT 4
int mpcqp_certify(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* x0, const float* xref,
                  const float* contact, const float* feet, const float* robot, const float* U,
                  float* G, double* report, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MPCQP_CERTIFY_ABI_H */

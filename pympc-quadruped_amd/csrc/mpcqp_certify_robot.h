// mpcqp_certify_robot.h -- per-robot algebra of the optimality certificate (mpcqp_certify.h), host-
// and device-callable so tests/ can check it on the CPU.
//
// phi(U) = J - J_free = 1/2 U^T H U + g^T U is the QP's objective (mpcqp_predict_robot.h computes
// J and J_free).  Its gradient is the adjoint of the rollout's two running sums:
//   x_{t+1} depends on u_j through X0 + (t - j) X1 for t >= j, so with e_t = x_{t+1} - xref_t
//   G_j  = 2 (X0^T S0_j + X1^T S1_j) + 2 (R u)_j,
//   S0_j = sum_{t>=j} Q e_t,   S1_j = sum_{t>=j} (t - j) Q e_t = S1_{j+1} + S0_{j+1}.
// The feasible set is a product over foot-steps of friction pyramids cut off at ub = contact fz_max
// (a swing foot-step: {0}), and a linear function g . v over one of them is smallest at the apex
// or at one of the four corners of the cut:
//   m = min(0, ub (g.n - mu |g.t1| - mu |g.t2|)).
// By convexity phi* >= phi(U) + min_V G . (V - U) = phi(U) - gap, gap = sum_k (g_k . u_k - m_k):
// a first-order bound, tight at the optimum and loose far from it.
//
//   cert_frame_entry   entry k of t1, t2 or n: prd_cone_entry's frame, read from its rows at mu = 0
//   cert_scan_step     one step of the backward scan of one state component
//   cert_state_grad    one entry of X0^T S0_j + X1^T S1_j (the transpose of prd_forced_entry)
//   cert_foot_term     g_k . u_k - m_k of one foot-step
//   cert_robot_host    (host build only) one robot, entry after entry in the order above
//
// Float64 on the caller's float32 inputs, FP contraction off, as mpcqp_predict_robot.h.
#pragma once
#include "mpcqp_predict_robot.h"

constexpr int CERT_REPORT = 4;                              // MPCQP_CERTIFY_REPORT
constexpr int CERT_OBJECTIVE = 0, CERT_GAP = 1, CERT_LOWER = 2, CERT_WORST = 3;

// entry k of axis 0: t1, 1: t2, 2: n of the frame the cone rows use.  With mu = 0 the rows 0, 2
// and 4 of prd_cone_entry are t1, t2 and n themselves.
__host__ __device__ inline double cert_frame_entry(const float* robot, int axis, int k) {
  float rec[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) rec[i] = i == 7 ? 0.f : robot[i];
  return prd_cone_entry(rec, 2 * axis, k);
}

// one step of a state component's backward sums: (S0_{j+1}, S1_{j+1}) -> (S0_j, S1_j)
__host__ __device__ inline void cert_scan_step(double* s0, double* s1, double qe) {
#pragma clang fp contract(off)
  *s1 = *s1 + *s0;
  *s0 = *s0 + qe;
}

// column c of X0 and X1 against the backward sums: (X0^T S0_j + X1^T S1_j)[c], the transpose of
// prd_forced_entry.  K, G: [3][12] row-major; s: (S0_j, S1_j) interleaved, [13][2]
__host__ __device__ inline double cert_state_grad(const double* K, const double* G, double minv, double h, int c,
                                                  const double* s) {
#pragma clang fp contract(off)
  const double a0 = 0.5 * h * h, a1 = h * h;
  const int ax = c % 3;
  double rot = 0.0, ang = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    rot = rot + G[PRD_NU * a + c] * (a0 * s[2 * a] + a1 * s[2 * a + 1]);
    ang = ang + K[PRD_NU * a + c] * s[2 * (6 + a)];
  }
  const double pos = minv * (a0 * s[2 * (3 + ax)] + a1 * s[2 * (3 + ax) + 1]);
  const double vel = (h * minv) * s[2 * (9 + ax)];
  return ((rot + pos) + h * ang) + vel;
}

// g . u - m of one foot-step: fr the frame [3][3] (t1, t2, n), ub = max(0, contact fz_max) of a
// stance foot-step, stance false for one the QP forces to 0 (m = 0).  *m receives m_k.
__host__ __device__ inline double cert_foot_term(const double* fr, double mu, double ub, bool stance, const double* g,
                                                 const float* u, double* m) {
#pragma clang fp contract(off)
  const double dot = (g[0] * (double)u[0] + g[1] * (double)u[1]) + g[2] * (double)u[2];
  double mk = 0.0;
  if (stance) {
    const double g1 = (g[0] * fr[0] + g[1] * fr[1]) + g[2] * fr[2];
    const double g2 = (g[0] * fr[3] + g[1] * fr[4]) + g[2] * fr[5];
    const double gn = (g[0] * fr[6] + g[1] * fr[7]) + g[2] * fr[8];
    const double v = ub * ((gn - mu * fabs(g1)) - mu * fabs(g2));
    mk = v < 0.0 ? v : (v == v ? 0.0 : v);   // min(0, v); a NaN stays one
  }
  *m = mk;
  return dot - mk;
}

#ifndef __HIPCC__
// One robot on the host: what one wavefront of mpcqp_certify_kernel computes, with the sums over
// the wave taken in index order: prd_rollout_host (J and J_free are prd_robot_host's to the bit),
// then the backward scan, the gradient and the foot-step terms.  q, r, W as prd_rollout_host.  Gf
// (float32), Gd (the entries before their rounding), report and status are nullable.
inline void cert_robot_host(int N, double h, const double* q, const double* r, const double* W, const float* x0,
                            const float* xref, const float* contact, const float* feet, const float* robot,
                            const float* U, float* Gf, double* Gd, double* report, int32_t* status) {
  static thread_local PrdRollout ro;
  static thread_local double S[PRD_MAX_N][PRD_NX][2], gd[PRD_MAX_N * PRD_NU];
  double rep[CERT_REPORT] = {0.0, 0.0, 0.0, 0.0};
  bool finite = prd_rollout_host(N, h, q, r, W, x0, xref, contact, feet, robot, U, &ro, S);
  if (finite) {
    double fr[9];
    for (int e = 0; e < 9; ++e) fr[e] = cert_frame_entry(robot, e / 3, e % 3);
    // the backward scan: S[j][.][0] holds Q e_j until S0_j replaces it
    for (int sc = 0; sc < PRD_NX; ++sc) {
      double s0 = 0.0, s1 = 0.0;
      for (int j = N - 1; j >= 0; --j) {
        cert_scan_step(&s0, &s1, S[j][sc][0]);
        S[j][sc][0] = s0, S[j][sc][1] = s1;
      }
    }
    for (int e = 0; e < PRD_NU * N; ++e) {
      gd[e] = 2.0 * cert_state_grad(ro.K, ro.G, ro.minv, h, e % PRD_NU, &S[e / PRD_NU][0][0]) + 2.0 * ro.ru[e];
      if (!isfinite((float)gd[e])) finite = false;
    }
    double gap = 0.0, worst = -INFINITY;
    for (int k = 0; k < 4 * N; ++k) {
      const bool stance = contact[k] > 0.f;
      double ub = stance ? (double)contact[k] * (double)robot[8] : 0.0, m;
      ub = ub > 0.0 ? ub : 0.0;
      const double term = cert_foot_term(fr, (double)robot[7], ub, stance, gd + 3 * k, U + 3 * k, &m);
      gap += term;
      worst = term > worst ? term : worst;
    }
    rep[CERT_OBJECTIVE] = (ro.je + ro.ju) - ro.jf, rep[CERT_GAP] = gap;
    rep[CERT_LOWER] = rep[CERT_OBJECTIVE] - gap, rep[CERT_WORST] = worst;
    for (int k = 0; k < CERT_REPORT; ++k)
      if (!isfinite(rep[k])) finite = false;
  }
  for (int e = 0; e < PRD_NU * N; ++e) {
    if (Gf) Gf[e] = finite ? (float)gd[e] : 0.f;
    if (Gd) Gd[e] = finite ? gd[e] : 0.0;
  }
  for (int k = 0; k < CERT_REPORT; ++k)
    if (report) report[k] = finite ? rep[k] : 0.0;
  if (status) status[0] = finite ? PRD_STATUS_OK : PRD_STATUS_NONFINITE;
}
#endif

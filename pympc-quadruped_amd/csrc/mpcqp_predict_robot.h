// mpcqp_predict_robot.h -- per-robot algebra of the predicted trajectory (mpcqp_predict.h), host-
// and device-callable so tests/ can check it on the CPU.
//
// com_traj = Sx x0 + Su U (mpc.py:293-294) for one robot without Sx or Su: A_d - I is nilpotent,
// so A^k B_d = X0 + k X1 (header comment of mpcqp_form.h) and
//   x_{t+1} = x0 + (t+1) n1 + C(t+1, 2) n2 + X0 P0_t + X1 P1_t,
//   P0_t = sum_{j<=t} u_j,   P1_t = sum_{j<=t} (t - j) u_j = P1_{t-1} + P0_{t-1}.
//
//   prd_yaw, prd_inertia_inv, prd_kg_column, prd_minv, prd_cone_entry
//                    the head of form_model restated per entry: R_z, I_w, inv(I_w),
//                    K = inv(I_w)[r]x, G = R_z^T K, 1/m and the cone rows, with the reference's
//                    float32 roundings in the same places (mpc.py:178-190, :239-245)
//   prd_n1, prd_n2   n1 = Nm x0, n2 = Nm^2 x0 (form_e)
//   prd_scan_step    one step of the two running sums of one input column
//   prd_free_entry, prd_forced_entry   one entry of x_{t+1}: the U = 0 part and the part U adds
//   prd_foot_slack   the smallest slack of a stance foot-step's six one-sided cone rows
//   prd_rollout_host (host build only) what the predicted trajectory and the certificate share of
//                    one robot, entry after entry in the order above: model, sums, errors, costs
//   prd_robot_host   (host build only) that, then the cone margin and the swing residual
//
// Everything is float64 on the caller's float32 inputs; FP contraction is off so the host build
// and the device build round alike (they differ in the order of the sums over the wave alone).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

constexpr int PRD_NX = 13, PRD_NU = 12, PRD_MAX_N = 32;   // NX, NU, MPCQP_MAX_HORIZON
constexpr int PRD_REPORT = 4;                              // MPCQP_PREDICT_REPORT
constexpr int PRD_COST = 0, PRD_COST_FREE = 1, PRD_MARGIN = 2, PRD_SWING = 3;
constexpr int PRD_STATUS_OK = 0, PRD_STATUS_NONFINITE = 4;   // MPCQP_STATUS_OK, MPCQP_STATUS_NONFINITE

__host__ __device__ inline double prd_f32r(double v) { return (double)(float)v; }

// float32(cos yaw), float32(sin yaw) of the model yaw x0[2] (mpc.py:178-180)
__host__ __device__ inline void prd_yaw(const float* x0, double* c, double* s) {
  const double yaw = (double)x0[2];
#ifdef __HIP_DEVICE_COMPILE__
  double sy, cy;
  sincos(yaw, &sy, &cy);   // as form_model: the same values as cos and sin apart
#else
  const double sy = sin(yaw), cy = cos(yaw);
#endif
  *c = prd_f32r(cy);
  *s = prd_f32r(sy);
}

// R_z[a][b] from its float32 entries
__host__ __device__ inline double prd_rz(double c, double s, int a, int b) {
  return a == 2 ? (b == 2 ? 1.0 : 0.0) : (b == 2 ? 0.0 : (a == b ? c : (a == 0 ? -s : s)));
}

// inv(I_w), I_w = float32(float32(R_z I_B) R_z^T), by the adjugate in float64 and stored float32
// (mpc.py:182, :189); inv[9] row-major.  robot: the record (mass, ixx ixy ixz iyy iyz izz, ...)
__host__ __device__ inline void prd_inertia_inv(double c, double s, const float* robot, double* inv) {
#pragma clang fp contract(off)
  const double ib[3][3] = {{(double)robot[1], (double)robot[2], (double)robot[3]},
                           {(double)robot[2], (double)robot[4], (double)robot[5]},
                           {(double)robot[3], (double)robot[5], (double)robot[6]}};
  double ri[3][3], I[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      ri[i][j] = prd_f32r(prd_rz(c, s, i, 0) * ib[0][j] + prd_rz(c, s, i, 1) * ib[1][j] + prd_rz(c, s, i, 2) * ib[2][j]);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      I[i][j] = prd_f32r(ri[i][0] * prd_rz(c, s, j, 0) + ri[i][1] * prd_rz(c, s, j, 1) + ri[i][2] * prd_rz(c, s, j, 2));
  }
  const double det = I[0][0] * (I[1][1] * I[2][2] - I[1][2] * I[2][1]) - I[0][1] * (I[1][0] * I[2][2] - I[1][2] * I[2][0]) +
                     I[0][2] * (I[1][0] * I[2][1] - I[1][1] * I[2][0]);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int r1 = (j + 1) % 3, r2 = (j + 2) % 3, c1 = (i + 1) % 3, c2 = (i + 2) % 3;
      const double cof = I[r1][c1] * I[r2][c2] - I[r1][c2] * I[r2][c1];   // adj(I)[i][j]
      inv[3 * i + j] = prd_f32r(cof / det);
    }
  }
}

// column `col` of K = float32(inv(I_w) [r_leg]x) (mpc.py:188-189) and of G = R_z^T K
__host__ __device__ inline void prd_kg_column(double c, double s, const double* inv, const float* feet, int col,
                                              double* k, double* g) {
#pragma clang fp contract(off)
  const int leg = col / 3, j = col % 3;
  const double rx = (double)feet[3 * leg], ry = (double)feet[3 * leg + 1], rzz = (double)feet[3 * leg + 2];
  const double sk0 = (j == 0) ? 0.0 : (j == 1 ? -rzz : ry);   // column j of [r]x
  const double sk1 = (j == 0) ? rzz : (j == 1 ? 0.0 : -rx);
  const double sk2 = (j == 0) ? -ry : (j == 1 ? rx : 0.0);
#pragma unroll
  for (int a = 0; a < 3; ++a) k[a] = prd_f32r(inv[3 * a] * sk0 + inv[3 * a + 1] * sk1 + inv[3 * a + 2] * sk2);
#pragma unroll
  for (int i = 0; i < 3; ++i) g[i] = prd_rz(c, s, 0, i) * k[0] + prd_rz(c, s, 1, i) * k[1] + prd_rz(c, s, 2, i) * k[2];
}

// I / m in float32 (mpc.py:190)
__host__ __device__ inline double prd_minv(const float* robot) { return prd_f32r(1.0 / (double)robot[0]); }

// entry k of the one-sided cone row rr (a_rr . f >= b_rr) in the (t1, t2, n) frame of the record's
// surface normal: rows 0..3 the pyramid, 4 n . f >= 0, 5 -n . f >= -contact fz_max (mpc.py:239-257
// for n = e_z); what form_model writes to mt.rows
__host__ __device__ inline double prd_cone_entry(const float* robot, int rr, int k) {
#pragma clang fp contract(off)
  double nx = (double)robot[9], ny = (double)robot[10], nz = (double)robot[11];
  const double nn = sqrt(nx * nx + ny * ny + nz * nz);
  if (!(nn > 0.0)) {
    nx = 0.0, ny = 0.0, nz = 1.0;
  } else {
    nx /= nn, ny /= nn, nz /= nn;
  }
  double t1x = 1.0 - nx * nx, t1y = -nx * ny, t1z = -nx * nz;
  const double tn = sqrt(t1x * t1x + t1y * t1y + t1z * t1z);
  t1x /= tn, t1y /= tn, t1z /= tn;
  const double t2x = ny * t1z - nz * t1y, t2y = nz * t1x - nx * t1z, t2z = nx * t1y - ny * t1x;
  const double mu = (double)robot[7];
  const double nk = k == 0 ? nx : (k == 1 ? ny : nz);
  const double t1k = k == 0 ? t1x : (k == 1 ? t1y : t1z);
  const double t2k = k == 0 ? t2x : (k == 1 ? t2y : t2z);
  return rr == 0 ? t1k + mu * nk : rr == 1 ? -t1k + mu * nk : rr == 2 ? t2k + mu * nk : rr == 3 ? -t2k + mu * nk
         : rr == 4 ? nk : -nk;
}

// n1 = Nm x0 and n2 = Nm^2 x0, component sc (form_e)
__host__ __device__ inline double prd_n1(const float* x0, double c, double s, double h, int sc) {
#pragma clang fp contract(off)
  const double g12 = (double)x0[12];
  if (sc < 3)
    return h * (prd_rz(c, s, 0, sc) * (double)x0[6] + prd_rz(c, s, 1, sc) * (double)x0[7] + prd_rz(c, s, 2, sc) * (double)x0[8]);
  if (sc < 6) return h * (double)x0[6 + sc] + (sc == 5 ? 0.5 * h * h * g12 : 0.0);
  return sc == 11 ? h * g12 : 0.0;
}
__host__ __device__ inline double prd_n2(const float* x0, double h, int sc) {
#pragma clang fp contract(off)
  return sc == 5 ? h * h * (double)x0[12] : 0.0;
}

// one step of an input column's running sums: (P0_{t-1}, P1_{t-1}) -> (P0_t, P1_t)
__host__ __device__ inline void prd_scan_step(double* p0, double* p1, float u) {
#pragma clang fp contract(off)
  *p1 = *p1 + *p0;
  *p0 = *p0 + (double)u;
}

// x_{t+1}[sc] for U = 0: x0 + (t+1) n1 + C(t+1, 2) n2
__host__ __device__ inline double prd_free_entry(double x0s, double n1, double n2, int t) {
#pragma clang fp contract(off)
  const double k = (double)(t + 1);
  return (x0s + k * n1) + (0.5 * k * (k - 1.0)) * n2;
}

// what U adds to x_{t+1}[sc]: row sc of X0 P0_t + X1 P1_t, X0 = [G h^2/2; S h^2/(2m); K h; S h/m; 0],
// X1 = [G h^2; S h^2/m; 0; 0; 0].  K, G: [3][12] row-major; p: (P0_t, P1_t) interleaved, [12][2]
__host__ __device__ inline double prd_forced_entry(const double* K, const double* G, double minv, double h, int sc,
                                                   const double* p) {
#pragma clang fp contract(off)
  const double a0 = 0.5 * h * h, a1 = h * h;
  double acc = 0.0;
  if (sc < 3) {
#pragma unroll
    for (int c = 0; c < PRD_NU; ++c) acc = acc + G[PRD_NU * sc + c] * (a0 * p[2 * c] + a1 * p[2 * c + 1]);
  } else if (sc < 6) {
#pragma unroll
    for (int leg = 0; leg < 4; ++leg) acc = acc + (a0 * p[2 * (3 * leg + sc - 3)] + a1 * p[2 * (3 * leg + sc - 3) + 1]);
    acc = minv * acc;
  } else if (sc < 9) {
#pragma unroll
    for (int c = 0; c < PRD_NU; ++c) acc = acc + K[PRD_NU * (sc - 6) + c] * p[2 * c];
    acc = h * acc;
  } else if (sc < 12) {
#pragma unroll
    for (int leg = 0; leg < 4; ++leg) acc = acc + p[2 * (3 * leg + sc - 9)];
    acc = (h * minv) * acc;
  }
  return acc;
}

// The smallest slack of the six one-sided rows of a stance foot-step: rows [6][3] row-major, f
// its force, ub = contact * fz_max (mpc.py:257).  *finite is cleared where a slack is not finite.
__host__ __device__ inline double prd_foot_slack(const double* rows, double ub, const float* f, bool* finite) {
#pragma clang fp contract(off)
  double m = INFINITY;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double sl = (rows[3 * r] * (double)f[0] + rows[3 * r + 1] * (double)f[1]) + rows[3 * r + 2] * (double)f[2];
    if (r == 5) sl = ub + sl;
    if (!isfinite(sl)) *finite = false;
    m = sl < m ? sl : m;
  }
  return m;
}

// the inputs mpcqp_solve refuses (form_stage), and a non-finite U entry
__host__ __device__ inline bool prd_bad_value(float w, bool is_contact) { return is_contact ? w == INFINITY : !isfinite(w); }

#ifndef __HIPCC__
// The rollout of one robot on the host, what prd_robot_host and cert_robot_host share: the model
// head, the forward sums, the entries of X before their rounding, the errors and the three costs,
// entry after entry in the order a wavefront's lanes take them, the sums over the wave in index
// order.
struct PrdRollout {
  double K[3 * PRD_NU], G[3 * PRD_NU], minv;
  double P[PRD_MAX_N][PRD_NU][2];   // (P0_t, P1_t) per input column
  double E[PRD_MAX_N][PRD_NX][2];   // (e_t, e_t for U = 0)
  double x[PRD_MAX_N * PRD_NX];     // x_{t+1}
  double ru[PRD_MAX_N * PRD_NU];    // R u
  double je, jf, ju;                // J = je + ju, J_free = jf
};

// q [13], r [12] the diagonal weights; W the full Q (13 x 13) then R (12 x 12), or NULL.  S, where
// the caller asks for it, receives Q e_t in S[t][.][0].  Returns false, with *ro untouched, for
// the inputs the kernels refuse.
inline bool prd_rollout_host(int N, double h, const double* q, const double* r, const double* W, const float* x0,
                             const float* xref, const float* contact, const float* feet, const float* robot,
                             const float* U, PrdRollout* ro, double (*S)[PRD_NX][2]) {
  bool bad = false;
  for (int i = 0; i < PRD_NX; ++i) bad |= prd_bad_value(x0[i], false);
  for (int i = 0; i < 12; ++i) bad |= prd_bad_value(feet[i], false) || prd_bad_value(robot[i], false);
  for (int i = 0; i < 4 * N; ++i) bad |= prd_bad_value(contact[i], true);
  for (int i = 0; i < PRD_NX * N; ++i) bad |= prd_bad_value(xref[i], false);
  for (int i = 0; i < PRD_NU * N; ++i) bad |= prd_bad_value(U[i], false);
  if (bad) return false;
  double c = 0.0, s = 0.0, inv[9], n1[PRD_NX], n2[PRD_NX];
  prd_yaw(x0, &c, &s);
  prd_inertia_inv(c, s, robot, inv);
  ro->minv = prd_minv(robot);
  for (int col = 0; col < PRD_NU; ++col) {
    double k[3], g[3];
    prd_kg_column(c, s, inv, feet, col, k, g);
    for (int a = 0; a < 3; ++a) ro->K[PRD_NU * a + col] = k[a], ro->G[PRD_NU * a + col] = g[a];
  }
  for (int sc = 0; sc < PRD_NX; ++sc) n1[sc] = prd_n1(x0, c, s, h, sc), n2[sc] = prd_n2(x0, h, sc);
  for (int col = 0; col < PRD_NU; ++col) {
    double p0 = 0.0, p1 = 0.0;
    for (int t = 0; t < N; ++t) {
      prd_scan_step(&p0, &p1, U[PRD_NU * t + col]);
      ro->P[t][col][0] = p0, ro->P[t][col][1] = p1;
    }
  }
  double je = 0.0, jf = 0.0, ju = 0.0;
  for (int e = 0; e < PRD_NX * N; ++e) {
    const int t = e / PRD_NX, sc = e % PRD_NX;
    const double xf = prd_free_entry((double)x0[sc], n1[sc], n2[sc], t);
    const double x = xf + prd_forced_entry(ro->K, ro->G, ro->minv, h, sc, &ro->P[t][0][0]);
    ro->x[e] = x;
    const double ee = x - (double)xref[e], ef = xf - (double)xref[e];
    ro->E[t][sc][0] = ee, ro->E[t][sc][1] = ef;
    if (!W) {
      const double qe = q[sc] * ee;
      if (S) S[t][sc][0] = qe;
      je += qe * ee, jf += q[sc] * ef * ef;
    }
  }
  if (W) {
    for (int e = 0; e < PRD_NX * N; ++e) {
      const int t = e / PRD_NX, sc = e % PRD_NX;
      double a = 0.0, af = 0.0;
      for (int j = 0; j < PRD_NX; ++j) a += W[PRD_NX * sc + j] * ro->E[t][j][0], af += W[PRD_NX * sc + j] * ro->E[t][j][1];
      if (S) S[t][sc][0] = a;
      je += ro->E[t][sc][0] * a, jf += ro->E[t][sc][1] * af;
    }
  }
  for (int e = 0; e < PRD_NU * N; ++e) {
    const int t = e / PRD_NU, col = e % PRD_NU;
    double ru = 0.0;
    if (W) {
      for (int j = 0; j < PRD_NU; ++j) ru += W[PRD_NX * PRD_NX + PRD_NU * col + j] * (double)U[PRD_NU * t + j];
    } else {
      ru = r[col] * (double)U[e];
    }
    ro->ru[e] = ru;
    ju += (double)U[e] * ru;
  }
  ro->je = je, ro->jf = jf, ro->ju = ju;
  return true;
}

// One robot on the host, entry after entry: what one wavefront of mpcqp_predict_kernel computes,
// with the sums over the wave taken in index order.  q, r, W as prd_rollout_host.  X, Xd (the
// entries before their float32 rounding), report and status are nullable.
inline void prd_robot_host(int N, double h, const double* q, const double* r, const double* W, const float* x0,
                           const float* xref, const float* contact, const float* feet, const float* robot,
                           const float* U, float* X, double* Xd, double* report, int32_t* status) {
  static thread_local PrdRollout ro;
  double rep[PRD_REPORT] = {0.0, 0.0, 0.0, 0.0};
  bool finite = prd_rollout_host(N, h, q, r, W, x0, xref, contact, feet, robot, U, &ro, nullptr);
  if (finite) {
    for (int e = 0; e < PRD_NX * N; ++e)
      if (!isfinite((float)ro.x[e])) finite = false;
    double rows[18];
    for (int e = 0; e < 18; ++e) rows[e] = prd_cone_entry(robot, e / 3, e % 3);
    double margin = INFINITY, swing = 0.0;
    for (int k = 0; k < 4 * N; ++k) {
      const float* f = U + 3 * k;
      if (contact[k] > 0.f) {
        const double sl = prd_foot_slack(rows, (double)contact[k] * (double)robot[8], f, &finite);
        margin = sl < margin ? sl : margin;
      } else {
        for (int a = 0; a < 3; ++a) swing = fabs((double)f[a]) > swing ? fabs((double)f[a]) : swing;
      }
    }
    rep[PRD_COST] = ro.je + ro.ju, rep[PRD_COST_FREE] = ro.jf, rep[PRD_MARGIN] = margin, rep[PRD_SWING] = swing;
    if (!isfinite(rep[PRD_COST]) || !isfinite(rep[PRD_COST_FREE])) finite = false;
  }
  for (int e = 0; e < PRD_NX * N; ++e) {
    if (X) X[e] = finite ? (float)ro.x[e] : 0.f;
    if (Xd) Xd[e] = finite ? ro.x[e] : 0.0;
  }
  for (int k = 0; k < PRD_REPORT; ++k)
    if (report) report[k] = finite ? rep[k] : 0.0;
  if (status) status[0] = finite ? PRD_STATUS_OK : PRD_STATUS_NONFINITE;
}
#endif

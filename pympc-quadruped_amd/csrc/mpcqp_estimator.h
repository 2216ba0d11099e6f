// mpcqp_estimator.h -- the base-state estimator on the device: one tick of the 18-state
// IMU + leg-kinematics Kalman filter of every robot in one launch (included by mpcqp.hip
// inside its anonymous namespace, after mpcqp_kinematics.h).  It is the second stage of
// doc/state_estimation_kf.md (after MIT Cheetah 3), fed by the sensor set
// scripts/mujoco_aliengo.py:101-118 collects, and fills the gap RobotData.update leaves for
// state_estimation=True (utils/robot_data.py raises NotImplementedError).
//
//   x = [p_b, v_b, p_1 .. p_4] (world), P 18 x 18, y in R^28 (include/mpcqp.h has the step).
//
// The measurement covariance is diagonal, so the update runs as 28 scalar updates in
// sequence: a measurement row has at most two non-zeros (+1, -1), h = P c^T is a difference
// of two columns of P, and P -= h h^T / s is a rank-1 update.  No 28 x 28 factorisation.
// The leg algebra is mpcqp_kin_leg.h; all arithmetic is float64 with FP contraction off,
// and each float32 output is rounded once, at its store.
#include <math.h>
#include <string.h>

#include "mpcqp_kin_leg.h"

constexpr int EST_NX = 18, EST_INIT = 18, EST_P = 24, EST_STRIDE = 352;

struct EstParams {
  int dof_layout;   // 1: `q` points at a dof-state tensor [B][12][2] (pos, vel per DOF)
  double dt, gravity, sigma_p, sigma_v, sigma_f, r_p, r_v, r_z, suspicion, p0, contact_height;
};

// A robot is spread over 18 lanes of a wavefront, lane j holding x_j and column j of P in
// registers (18 doubles, every index a compile-time constant after unrolling); a workgroup
// is one wavefront with kEstRobots = 3 robots in lanes 0..53.  P stays bitwise symmetric
// through the tick (the prediction and the rank-1 updates are written so that entry (i, j)
// and entry (j, i) round alike), so lane j forms its h_j = (c P)_j from its own column.
// What crosses lanes goes through LDS: h and x of every scalar update (double-buffered, one
// barrier per update), the three columns the prediction moves, the per-leg measurements.
constexpr int kEstRobots = 3;
constexpr int kEstThreads = 64;

struct EstLeg {
  double r[3], rd[3], t, k;   // R_q p_i, R_q (w x p_i + J_i qd_i), clipped trust, 1 + (1 - t) s
};

struct EstShared {
  double P[EST_NX * EST_NX];             // a robot's P, row-major: the columns as the lanes hold them
  double __attribute__((aligned(16))) h[2][EST_NX];
  double x[2][EST_NX];
  double xm[EST_NX];                     // x^-, the state before the prediction
  EstLeg leg[4];
  double acc[3], wworld[3];              // R_q a_b - g e_z, R_q w_b
  int bad[4];                            // a non-finite input seen by leg lane l
  // lane j saw a non-finite x_j, P column j or `initialised` word: a byte per lane, read back as three words
  unsigned char __attribute__((aligned(16))) rec_bad[24];
};

__device__ inline bool est_finite3(const double* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

__global__ __launch_bounds__(kEstThreads) void mpcqp_estimate_kernel(
    EstParams ep, int B, const float* __restrict__ quat, const float* __restrict__ gyro,
    const float* __restrict__ accel, const float* __restrict__ q, const float* __restrict__ qdot,
    const float* __restrict__ trust, const double* __restrict__ geom, double* __restrict__ est_state,
    float* __restrict__ root_states, float* __restrict__ feet_world, int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ EstShared shared[kEstRobots + 1];   // + the idle lanes' slot
  const int t = threadIdx.x;
  const int r = t / EST_NX, j = t - r * EST_NX;
  const int b = blockIdx.x * kEstRobots + r;
  // lanes 54..63 and the tail workgroup's lanes past the batch touch no memory; they keep
  // walking through the barriers on a slot of their own that nobody reads
  const bool live = r < kEstRobots && b < B;
  EstShared& sh = shared[r];
  double* rec = est_state + (size_t)EST_STRIDE * (live ? b : 0);

  // ---- the record: x_j, column j of P; an all-zero record starts from (0, P0 I)
  // (a NaN `initialised` word is non-zero: the record counts as initialised, and is refused).
  double x = 0.0, Pc[EST_NX], iw = 0.0;
#pragma unroll
  for (int i = 0; i < EST_NX; ++i) Pc[i] = 0.0;
  // Every load of the record is issued here, before the `initialised` word is looked at,
  // and none of them is used until the leg algebra below is done: the record and the sensors
  // are in flight together, one memory latency and not three in a row.
  if (live) {
    iw = rec[EST_INIT];
    x = rec[j];
#pragma unroll
    for (int i = 0; i < EST_NX; ++i) Pc[i] = rec[EST_P + EST_NX * i + j];
  }

  // ---- the sensors: lane l < 4 of a robot does leg l (step 1)
  double qw = 0.0, qx = 0.0, qy = 0.0, qz = 0.0;
  if (live && j < 4) {
    const int leg = j;
    const size_t bl = (size_t)b * 4 + leg;
    double ql[3], qd[3], w[3], ab[3], g[5];
    qw = (double)quat[4 * (size_t)b], qx = (double)quat[4 * (size_t)b + 1], qy = (double)quat[4 * (size_t)b + 2],
    qz = (double)quat[4 * (size_t)b + 3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      w[k] = (double)gyro[3 * (size_t)b + k];
      ab[k] = (double)accel[3 * (size_t)b + k];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) g[k] = geom[KIN_STRIDE * (size_t)b + k];
    const float tr = trust[bl];
    // (the joints last: their layout is a branch, and a load behind it would wait for them)
    if (ep.dof_layout) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        ql[k] = (double)q[(bl * 3 + k) * 2];
        qd[k] = (double)q[(bl * 3 + k) * 2 + 1];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        ql[k] = (double)q[bl * 3 + k];
        qd[k] = (double)qdot[bl * 3 + k];
      }
    }
    bool ok = isfinite(qw) && isfinite(qx) && isfinite(qy) && isfinite(qz) && est_finite3(w) && est_finite3(ab) &&
              est_finite3(ql) && est_finite3(qd) && isfinite(tr);
#pragma unroll
    for (int k = 0; k < 5; ++k) ok = ok && isfinite(g[k]);
    sh.bad[leg] = ok ? 0 : 1;

    double Rq[9], p[3], pth[3], Jb[9], u[3];
    kin_quat2matrix(qw, qx, qy, qz, Rq);
    kin_leg_chain(g, leg, ql, p, pth, Jb);
    EstLeg& L = sh.leg[leg];
    swing_mat3(Rq, p, L.r);
    swing_mat3(Jb, qd, u);
    u[0] = (w[1] * p[2] - w[2] * p[1]) + u[0];
    u[1] = (w[2] * p[0] - w[0] * p[2]) + u[1];
    u[2] = (w[0] * p[1] - w[1] * p[0]) + u[2];
    swing_mat3(Rq, u, L.rd);
    const double tc = (double)fminf(fmaxf(tr, 0.0f), 1.0f);
    L.t = tc;
    L.k = 1.0 + (1.0 - tc) * ep.suspicion;
    if (leg == 0) {
      swing_mat3(Rq, ab, sh.acc);
      sh.acc[2] = sh.acc[2] - ep.gravity;
      swing_mat3(Rq, w, sh.wworld);
    }
  }
  // a fresh record: whatever it holds beyond its `initialised` word is discarded
  if (live && !(iw != 0.0)) {
    x = 0.0;
#pragma unroll
    for (int i = 0; i < EST_NX; ++i) Pc[i] = i == j ? ep.p0 : 0.0;
  }
  const double x_minus = x;
  // An initialised record that holds a non-finite x, P or `initialised` word is refused like
  // a non-finite input.  Each lane judges what it holds and the verdicts meet in LDS; they
  // are read in the store phase, many barriers on.  (A fresh record's 0 and p0 I pass.)
  // The verdict itself is formed below, among the prediction's LDS reads.
  sh.xm[j] = x;
#pragma unroll
  for (int i = 0; i < EST_NX; ++i) sh.P[EST_NX * i + j] = Pc[i];
  __syncthreads();

  const double dt = ep.dt;

  // ---- the prediction (step 4): x = A x^- + B a, P = A P A^T + Q with A = I + dt E_pv.
  // (P + dt (Pa + Pb)) + dt^2 Pc with Pa = P[i + 3][j] (i < 3), Pb = P[i][j + 3] (j < 3),
  // Pc = P[i + 3][j + 3]: transposing swaps Pa and Pb, so a symmetric P stays one bitwise.
  if (j < 3) {
    x = (x + dt * sh.xm[j + 3]) + (0.5 * dt * dt) * sh.acc[j];
  } else if (j < 6) {
    x = x + dt * sh.acc[j - 3];
  }
  {
    const double qj = dt * (j < 3 ? ep.sigma_p : j < 6 ? ep.sigma_v : ep.sigma_f * sh.leg[j >= 6 ? (j - 6) / 3 : 0].k);
    // the record's verdict (see above), here so that it runs while the reads below are on
    // their way.  0 * v is 0 for a finite v and NaN for any other, and a NaN survives the
    // sums: twenty multiply-adds on two chains, nothing compared until the end.
    double z0 = 0.0 * iw, z1 = 0.0 * x_minus;
#pragma unroll
    for (int i = 0; i < EST_NX; i += 2) {
      z0 = fma(0.0, Pc[i], z0);
      z1 = fma(0.0, Pc[i + 1], z1);
    }
    sh.rec_bad[j] = (z0 + z1) == 0.0 ? 0 : 1;
    double Pn[EST_NX];
#pragma unroll
    for (int i = 0; i < EST_NX; ++i) {
      const double pa = i < 3 ? Pc[i + 3] : 0.0;
      // (every lane reads, from a column that exists, and lanes 3 .. 17 discard: a read
      // under a branch would wait for its own latency, eighteen times in a row)
      const int jc = j < 3 ? j + 3 : j;
      const double pbv = sh.P[EST_NX * i + jc];
      const double pb = j < 3 ? pbv : 0.0;
      double v = Pc[i] + dt * (pa + pb);
      if (i < 3) {
        const double pcv = sh.P[EST_NX * (i + 3) + jc];
        v = v + (dt * dt) * (j < 3 ? pcv : 0.0);
      }
      Pn[i] = i == j ? v + qj : v;
    }
#pragma unroll
    for (int i = 0; i < EST_NX; ++i) Pc[i] = Pn[i];
  }

  // ---- the update (steps 3, 5, 6): 28 scalar measurements, each with the row
  // c = e_ia - e_ib (ib < 0: e_ia alone), the value y built from x^- and the variance rv
#define EST_SCALAR_UPDATE(m, ia, ib, yv, rv)                                        \
  {                                                                                 \
    const int par = (m) & 1;                                                        \
    const double hj = (ib) >= 0 ? Pc[ia] - Pc[(ib) >= 0 ? (ib) : 0] : Pc[ia];       \
    sh.h[par][j] = hj;                                             \
    sh.x[par][j] = x;                                              \
    __syncthreads();                                                                \
    const double* hh = sh.h[par];                                                   \
    const double* xx = sh.x[par];                                                   \
    const double s = ((ib) >= 0 ? hh[ia] - hh[(ib) >= 0 ? (ib) : 0] : hh[ia]) + (rv); \
    const double cx = (ib) >= 0 ? xx[ia] - xx[(ib) >= 0 ? (ib) : 0] : xx[ia];       \
    const double inv = 1.0 / s;                                                     \
    x = x + (hj * inv) * ((yv) - cx);                                               \
    _Pragma("unroll") for (int i = 0; i < EST_NX; ++i) Pc[i] = Pc[i] - (hh[i] * hj) * inv; \
  }
#pragma unroll
  for (int leg = 0; leg < 4; ++leg) {
    const EstLeg& L = sh.leg[leg];
#pragma unroll
    for (int k = 0; k < 3; ++k) EST_SCALAR_UPDATE(3 * leg + k, k, 6 + 3 * leg + k, -L.r[k], ep.r_p)
  }
#pragma unroll
  for (int leg = 0; leg < 4; ++leg) {
    const EstLeg& L = sh.leg[leg];
    const double rv = ep.r_v * L.k;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      EST_SCALAR_UPDATE(12 + 3 * leg + k, 3 + k, -1, (1.0 - L.t) * sh.xm[3 + k] + L.t * (-L.rd[k]), rv)
  }
#pragma unroll
  for (int leg = 0; leg < 4; ++leg) {
    const EstLeg& L = sh.leg[leg];
    EST_SCALAR_UPDATE(24 + leg, 8 + 3 * leg, -1, L.t * ep.contact_height + (1.0 - L.t) * (sh.xm[2] + L.r[2]),
                      ep.r_z * L.k)
  }
#undef EST_SCALAR_UPDATE

  // ---- P <- (P + P^T) / 2 (exact where P is symmetric already, which it is unless the
  // caller seeded one that is not)
  // (every lane is past its reads of sh.P: 28 barriers lie between)
#pragma unroll
  for (int i = 0; i < EST_NX; ++i) sh.P[EST_NX * i + j] = Pc[i];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < EST_NX; ++i) Pc[i] = 0.5 * (Pc[i] + sh.P[EST_NX * j + i]);

  if (!live) return;
  unsigned long long rb[3];
  memcpy(rb, sh.rec_bad, sizeof rb);   // bytes 18 .. 23 belong to nobody
  const bool bad = (sh.bad[0] | sh.bad[1] | sh.bad[2] | sh.bad[3]) != 0 || (rb[0] | rb[1] | (rb[2] & 0xffffull)) != 0;
  // ---- stores: a robot with a non-finite input or record keeps its record, and its
  // outputs are formed from the state as it was (step 7)
  if (!bad) {
    rec[j] = x;
#pragma unroll
    for (int i = 0; i < EST_NX; ++i) rec[EST_P + EST_NX * i + j] = Pc[i];
    if (j == 0) rec[EST_INIT] = 1.0;
  }
  const double xo = bad ? x_minus : x;
  if (j < 6) {
    if (root_states != nullptr) root_states[13 * (size_t)b + (j < 3 ? j : j + 4)] = (float)xo;
  } else if (feet_world != nullptr) {
    feet_world[12 * (size_t)b + j - 6] = (float)xo;
  }
  if (j == 0) {
    if (root_states != nullptr) {
      float* rs = root_states + 13 * (size_t)b;
      rs[3] = (float)qx, rs[4] = (float)qy, rs[5] = (float)qz, rs[6] = (float)qw;
#pragma unroll
      for (int k = 0; k < 3; ++k) rs[10 + k] = (float)sh.wworld[k];
    }
    if (status != nullptr) status[b] = bad ? MPCQP_STATUS_NONFINITE : MPCQP_STATUS_OK;
  }
}

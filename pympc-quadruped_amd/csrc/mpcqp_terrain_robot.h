// mpcqp_terrain_robot.h -- per-robot algebra of the terrain plane (mpcqp_terrain.h), host- and
// device-callable so tests/ can check it on the CPU.
//
//   ter_eig     eigenvalues of a symmetric 3 x 3 and the eigenvector of the smallest, by cyclic Jacobi
//   ter_tick    one tick: latch the feet in contact, fit the plane, accept or hold
//               RobotData.update_terrain_normal                         utils/robot_data.py:186-228
//   ter_robot   one robot's share of a launch: loads, the tick, the stores
//
// Everything is float64 on the caller's float32 inputs; FP contraction is off so the host build
// and the device build round alike.  Every array index is a compile-time constant (unrolled
// loops, template arguments), so the device build keeps everything in registers.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

// the record (doubles): history[4][3], initialised (0 / 1), n[3], d, fitted (0 / 1), two zero words
constexpr int TER_HIST = 0, TER_INIT = 12, TER_N = 13, TER_D = 16, TER_FITTED = 17, TER_STRIDE = 20;
constexpr int TER_STATUS_OK = 0, TER_STATUS_NONFINITE = 4;   // MPCQP_STATUS_OK, MPCQP_STATUS_NONFINITE
constexpr int TER_SWING_STATE = 1, TER_ROOT_STATES = 2;      // MPCQP_TERRAIN_SWING_STATE, MPCQP_TERRAIN_ROOT_STATES
constexpr int TER_GROUND = 4;   // MPCQP_TERRAIN_GROUND: `plane` is the swing leg's ground, d - n_z touchdown_z
constexpr int TER_ROBOT_STRIDE = 16, TER_ROBOT_NORMAL = 9;   // MPCQP_ROBOT_STRIDE, MPCQP_ROBOT_NORMAL: the cone rows' normal
constexpr int TER_SWEEPS = 6;   // 4 reach numpy.linalg.eigh's vector to 3e-15, 3 leave 2e-5

struct TerParams {
  double contact_threshold, flat_tol, cos_max_tilt, blend;
  int flags;
  // the swing leg's (mpcqp_set_swing); read under TER_GROUND alone.  Last, so that an initialiser
  // list that stops at `flags` keeps its meaning and leaves this zero
  double touchdown_z;
};

// a tenth of a record: the record is 16-byte aligned, so it moves as ten of these
struct alignas(16) TerPair {
  double a, b;
};

// One Jacobi rotation of the symmetric A (full storage) in the (P, Q) plane, accumulated into
// the columns of V; skipped where the off-diagonal entry is 0.
template <int P, int Q>
__host__ __device__ inline void ter_rotate(double (&A)[3][3], double (&V)[3][3]) {
#pragma clang fp contract(off)
  constexpr int R = 3 - P - Q;
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  // the smaller root of t^2 + 2 theta t - 1; theta^2 overflowing gives t = 0, a rotation by nothing
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  A[P][P] = A[P][P] - t * apq;
  A[Q][Q] = A[Q][Q] + t * apq;
  A[P][Q] = A[Q][P] = 0.0;
  const double arp = A[R][P], arq = A[R][Q];
  A[R][P] = A[P][R] = c * arp - s * arq;
  A[R][Q] = A[Q][R] = s * arp + c * arq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vp = V[k][P], vq = V[k][Q];
    V[k][P] = c * vp - s * vq;
    V[k][Q] = s * vp + c * vq;
  }
}

// Eigenvalues l[0] <= l[1] <= l[2] of the symmetric S (row-major, 9 words) and the unit
// eigenvector v of l[0]: TER_SWEEPS cyclic Jacobi sweeps over (0,1), (0,2), (1,2).
__host__ __device__ inline void ter_eig(const double* S, double* l, double* v) {
#pragma clang fp contract(off)
  double A[3][3], V[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      A[i][j] = S[3 * i + j];
      V[i][j] = i == j ? 1.0 : 0.0;
    }
  }
#pragma unroll
  for (int sweep = 0; sweep < TER_SWEEPS; ++sweep) {
    ter_rotate<0, 1>(A, V);
    ter_rotate<0, 2>(A, V);
    ter_rotate<1, 2>(A, V);
  }
  const double d0 = A[0][0], d1 = A[1][1], d2 = A[2][2];
  const int i0 = (d0 <= d1 && d0 <= d2) ? 0 : (d1 <= d2 ? 1 : 2);
  const double lo01 = d0 < d1 ? d0 : d1, hi01 = d0 < d1 ? d1 : d0;
  l[0] = lo01 < d2 ? lo01 : d2;
  l[2] = hi01 > d2 ? hi01 : d2;
  const double m = hi01 < d2 ? hi01 : d2;   // the median: max(lo01, min(hi01, d2))
  l[1] = lo01 > m ? lo01 : m;
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = i0 == 0 ? V[k][0] : i0 == 1 ? V[k][1] : V[k][2];
}

// the record as it was, for the outputs of a robot whose tick is refused: the level plane
// through the origin if it was not initialised
__host__ __device__ inline void ter_as_was(const double* rec, double* out) {
  const bool init = rec[TER_INIT] != 0.0;
#pragma unroll
  for (int k = 0; k < TER_STRIDE; ++k) out[k] = init ? rec[k] : 0.0;
  if (!init) out[TER_N + 2] = 1.0;
}

// One tick.  rec: the record as it is; feet: the four feet in the world frame, [4][3]; c: the
// contact decision per foot.  out: the record after the tick -- or, where a foot to be latched
// or a word of an initialised record is non-finite (returns false), the record as it was.
//   latch     a record not initialised takes all four feet and n = (0, 0, 1); an initialised
//             one takes foot i where c[i] holds                                    (:189-192)
//   fit       mu the mean of the history, S = sum (h_i - mu)(h_i - mu)^T, n_fit the
//             eigenvector of its smallest eigenvalue, flipped to n_z >= 0          (:219-226)
//   accept    l2 > 0, l1 - l0 > flat_tol l2 (the points span a plane) and n_fit_z >= cos_max_tilt:
//             n <- normalise((1 - blend) n + blend n_fit), fitted = 1; else n stays, fitted = 0
//   d = n . mu either way: the plane n . p = d through the centroid
// The reference takes a row of numpy's eigenvector matrix where the eigenvector is the column,
// and starts from a history of zeros; both are deviations.
__host__ __device__ inline bool ter_tick(const TerParams& tp, const double* rec, const double* feet, const bool* c,
                                         double* out) {
#pragma clang fp contract(off)
  const bool init = rec[TER_INIT] != 0.0;
  bool ok = true;
  if (init) {
#pragma unroll
    for (int k = 0; k < TER_STRIDE; ++k) ok = ok && isfinite(rec[k]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!init || c[i]) ok = ok && isfinite(feet[3 * i]) && isfinite(feet[3 * i + 1]) && isfinite(feet[3 * i + 2]);
  }
  if (!ok) {
    ter_as_was(rec, out);
    return false;
  }
  double h[12], n[3] = {0.0, 0.0, 1.0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool take = !init || c[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) h[3 * i + k] = take ? feet[3 * i + k] : rec[TER_HIST + 3 * i + k];
  }
  if (init) {
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = rec[TER_N + k];
  }
  double mu[3], S[9];
#pragma unroll
  for (int k = 0; k < 3; ++k) mu[k] = (((h[k] + h[3 + k]) + h[6 + k]) + h[9 + k]) / 4.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int s = r; s < 3; ++s) {
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) acc = acc + (h[3 * i + r] - mu[r]) * (h[3 * i + s] - mu[s]);
      S[3 * r + s] = S[3 * s + r] = acc;
    }
  }
  double l[3], nf[3];
  ter_eig(S, l, nf);
  if (nf[2] < 0.0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) nf[k] = -nf[k];
  }
  bool fitted = l[2] > 0.0 && (l[1] - l[0]) > tp.flat_tol * l[2] && nf[2] >= tp.cos_max_tilt;
  if (fitted) {
    double nb[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) nb[k] = (1.0 - tp.blend) * n[k] + tp.blend * nf[k];
    const double len = sqrt((nb[0] * nb[0] + nb[1] * nb[1]) + nb[2] * nb[2]);
    fitted = len > 0.0;   // a caller-seeded n opposite to the fit: hold
    if (fitted) {
#pragma unroll
      for (int k = 0; k < 3; ++k) n[k] = nb[k] / len;
    }
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) out[TER_HIST + k] = h[k];
  out[TER_INIT] = 1.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) out[TER_N + k] = n[k];
  out[TER_D] = (n[0] * mu[0] + n[1] * mu[1]) + n[2] * mu[2];
  out[TER_FITTED] = fitted ? 1.0 : 0.0;
  out[18] = out[19] = 0.0;
  return true;
}

// the float32 quat2matrix of the plan kernel (plan_quat2matrix, robot_data.py:75), restated
// here so that the host build has it
__host__ __device__ inline void ter_quat2matrix(float qw, float qx, float qy, float qz, float (&R)[9]) {
#pragma clang fp contract(off)
  const float ww = (qw * qw), xx = (qx * qx), yy = (qy * qy), zz = (qz * qz);
  R[0] = (((ww + xx) - yy) - zz);
  R[1] = 2.f * ((qx * qy) - (qw * qz));
  R[2] = 2.f * ((qw * qy) + (qx * qz));
  R[3] = 2.f * ((qw * qz) + (qx * qy));
  R[4] = (((ww - xx) + yy) - zz);
  R[5] = 2.f * ((qy * qz) - (qw * qx));
  R[6] = 2.f * ((qx * qz) - (qw * qy));
  R[7] = 2.f * ((qw * qx) + (qy * qz));
  R[8] = (((ww - xx) - yy) + zz);
}

// the contact decision: contact > threshold (a NaN is no contact), or with TER_SWING_STATE the
// leg controller's own rule for stance, !(swing_state > 0)
__host__ __device__ inline bool ter_contact(const TerParams& tp, float value) {
  return (tp.flags & TER_SWING_STATE) ? !(value > 0.0f) : (double)value > tp.contact_threshold;
}

// Robot b's share of mpcqp_terrain: `quat`, `robot` and every output are nullable.  A refused
// robot: the record is not written, the status is TER_STATUS_NONFINITE and the outputs come
// from the record as it was.  The latched feet are foot centres, and the swing leg places a
// foothold at touchdown_z + ground(x, y) (mpcqp_set_ground): under TER_GROUND the fourth word of
// `plane` is d - n_z touchdown_z, the plane whose ground() + touchdown_z is the fitted plane
// itself, so that a foothold lands on n . p = d.  The record keeps d.
__host__ __device__ inline void ter_robot(const TerParams& tp, size_t b, const float* pos_feet, const float* contact,
                                          const float* quat, double* terrain_state, float* robot, float* normal,
                                          float* plane, float* normal_base, int32_t* status) {
#pragma clang fp contract(off)
  TerPair* rp = (TerPair*)(terrain_state + TER_STRIDE * b);
  double rec[TER_STRIDE], out[TER_STRIDE], feet[12];
  bool c[4];
#pragma unroll
  for (int k = 0; k < TER_STRIDE / 2; ++k) {
    const TerPair p = rp[k];
    rec[2 * k] = p.a, rec[2 * k + 1] = p.b;
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) feet[k] = (double)pos_feet[12 * b + k];
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = ter_contact(tp, contact[4 * b + i]);
  const bool ok = ter_tick(tp, rec, feet, c, out);
  if (ok) {
#pragma unroll
    for (int k = 0; k < TER_STRIDE / 2; ++k) {
      TerPair p;
      p.a = out[2 * k], p.b = out[2 * k + 1];
      rp[k] = p;
    }
  }
  const float n32[3] = {(float)out[TER_N], (float)out[TER_N + 1], (float)out[TER_N + 2]};
  if (normal != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) normal[3 * b + k] = n32[k];
  }
  if (robot != nullptr) {   // the cone rows' surface normal, words 9..11 of the robot record
#pragma unroll
    for (int k = 0; k < 3; ++k) robot[TER_ROBOT_STRIDE * b + TER_ROBOT_NORMAL + k] = n32[k];
  }
  if (plane != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) plane[4 * b + k] = n32[k];
    plane[4 * b + 3] =
        (tp.flags & TER_GROUND) ? (float)(out[TER_D] - out[TER_N + 2] * tp.touchdown_z) : (float)out[TER_D];
  }
  if (normal_base != nullptr) {   // R_base^T n (:227), R_base the float32 quat2matrix widened
    float qw, qx, qy, qz;
    if (tp.flags & TER_ROOT_STATES) {   // [pos(3), quat(x, y, z, w), ...] (isaacgym_a1.py:119-128)
      const float* rs = quat + 13 * b;
      qx = rs[3], qy = rs[4], qz = rs[5], qw = rs[6];
    } else {
      qw = quat[4 * b], qx = quat[4 * b + 1], qy = quat[4 * b + 2], qz = quat[4 * b + 3];
    }
    float R[9];
    ter_quat2matrix(qw, qx, qy, qz, R);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      normal_base[3 * b + k] =
          (float)(((double)R[k] * out[TER_N] + (double)R[3 + k] * out[TER_N + 1]) + (double)R[6 + k] * out[TER_N + 2]);
  }
  if (status != nullptr) status[b] = ok ? TER_STATUS_OK : TER_STATUS_NONFINITE;
}

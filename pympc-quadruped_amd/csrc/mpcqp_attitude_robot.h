// mpcqp_attitude_robot.h -- per-robot algebra of the orientation filter and the contact
// trust (mpcqp_attitude.h), host- and device-callable so tests/ can check it on the CPU.
//
//   att_tick    one tick of the gyro / accelerometer orientation filter   doc/state_estimation_kf.md, section 2
//   att_trust   one leg's contact trust from the gait phase               the stance ramp of the Cheetah 3 filter,
//                                                                         on swing_decide's integers (gait.py:102-121)
//   att_robot   one robot's share of a launch: loads, both of the above, the touch sensor
//               (scripts/mujoco_aliengo.py:101-118, touch_state) and the stores
//
// Everything is float64 on the caller's float32 inputs; FP contraction is off so the host
// build and the device build round alike.  Nothing here depends on a lane.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "mpcqp_kin_leg.h"   // kin_quat2matrix's formula; swing_counts (mpcqp_swing_leg.h)

// the record (doubles): q (w, x, y, z), initialised (0 / 1), gyro bias b[3]
constexpr int ATT_Q = 0, ATT_INIT = 4, ATT_BIAS = 5, ATT_STRIDE = 8;
constexpr int ATT_STATUS_OK = 0, ATT_STATUS_NONFINITE = 4;   // MPCQP_STATUS_OK, MPCQP_STATUS_NONFINITE

struct AttParams {
  double dt, gravity, kappa_ref, bias_gain, trust_window, touch_threshold;
};

// half a record: the record is 16-byte aligned, so it moves as four of these
struct alignas(16) AttPair {
  double a, b;
};

__host__ __device__ inline bool att_finite3(const double* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

// the record as it was, for the outputs of a robot whose tick is refused: identity with zero
// bias if it was not initialised
__host__ __device__ inline void att_as_was(const double* rec, double* out) {
  const bool init = rec[ATT_INIT] != 0.0;
#pragma unroll
  for (int k = 0; k < ATT_STRIDE; ++k) out[k] = init ? rec[k] : 0.0;
  if (!init) out[ATT_Q] = 1.0;
}

// One orientation tick.  rec: the record as it is; w, a: gyro and accelerometer (specific
// force; at rest a = R^T (0, 0, g)).  out: the record after the tick -- or, for a non-finite
// input or record value (returns false), the record as it was, identity with zero bias if it
// was not initialised: what the outputs are formed from.
//   record not initialised: q = the shortest arc with R(q)^T e_z = a / |a| and zero yaw,
//     b = 0, no integration;
//   else, with m = a / |a|, u = R(q)^T e_z, e = m x u, gamma = clamp(1 - | |a| - g | / g, 0, 1):
//     omega = w - b + kappa_ref gamma e,  b -= bias_gain gamma e dt,
//     q <- normalise(q (x) exp(omega dt / 2))
// which is the document's R_{k+1} = R_k exp([w_b + kappa w_corr]x dt) (deviations).
__host__ __device__ inline bool att_tick(const AttParams& ap, const double* rec, const double* w, const double* a,
                                         double* out) {
#pragma clang fp contract(off)
  bool ok = att_finite3(w) && att_finite3(a);
#pragma unroll
  for (int k = 0; k < ATT_STRIDE; ++k) ok = ok && isfinite(rec[k]);
  const bool init = rec[ATT_INIT] != 0.0;
  if (!ok) {
    att_as_was(rec, out);
    return false;
  }
  const double n = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
  double m[3] = {0.0, 0.0, 0.0};
  if (n > 0.0) {
    m[0] = a[0] / n;
    m[1] = a[1] / n;
    m[2] = a[2] / n;
  }
  out[ATT_INIT] = 1.0;
  if (!init) {
    double q0 = 1.0, q1 = 0.0, q2 = 0.0;
    if (n > 0.0) {
      if (m[2] < -1.0 + 1e-12) {
        q0 = 0.0, q1 = 1.0;
      } else {
        const double c = 1.0 + m[2];
        const double s = sqrt((c * c + m[1] * m[1]) + m[0] * m[0]);
        q0 = c / s, q1 = m[1] / s, q2 = -m[0] / s;
      }
    }
    out[0] = q0, out[1] = q1, out[2] = q2, out[3] = 0.0;
    out[ATT_BIAS] = out[ATT_BIAS + 1] = out[ATT_BIAS + 2] = 0.0;
    return true;
  }
  const double qw = rec[0], qx = rec[1], qy = rec[2], qz = rec[3];
  // u = R(q)^T e_z: the third row of kin_quat2matrix
  double R[9];
  kin_quat2matrix(qw, qx, qy, qz, R);
  const double u[3] = {R[6], R[7], R[8]};
  double e[3] = {0.0, 0.0, 0.0}, gamma = 0.0;
  if (n > 0.0) {
    e[0] = m[1] * u[2] - m[2] * u[1];
    e[1] = m[2] * u[0] - m[0] * u[2];
    e[2] = m[0] * u[1] - m[1] * u[0];
    gamma = 1.0 - fabs(n - ap.gravity) / ap.gravity;
    gamma = gamma < 0.0 ? 0.0 : gamma > 1.0 ? 1.0 : gamma;
  }
  const double kg = ap.kappa_ref * gamma, bg = ap.bias_gain * gamma;
  double th[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double b = rec[ATT_BIAS + k];
    th[k] = ((w[k] - b) + kg * e[k]) * ap.dt;
    out[ATT_BIAS + k] = b - (bg * e[k]) * ap.dt;
  }
  const double t = sqrt((th[0] * th[0] + th[1] * th[1]) + th[2] * th[2]);
  double dw = 1.0, sc = 0.5;
  if (!(t < 1e-8)) {
    const double half = 0.5 * t;
    dw = cos(half);
    sc = sin(half) / t;
  }
  const double dx = sc * th[0], dy = sc * th[1], dz = sc * th[2];
  // q (x) dq, Hamilton
  const double pw = ((qw * dw - qx * dx) - qy * dy) - qz * dz;
  const double px = ((qw * dx + qx * dw) + qy * dz) - qz * dy;
  const double py = ((qw * dy - qx * dz) + qy * dw) + qz * dx;
  const double pz = ((qw * dz + qx * dy) - qy * dx) + qz * dw;
  const double s = sqrt(((pw * pw + px * px) + py * py) + pz * pz);
  out[0] = pw / s, out[1] = px / s, out[2] = py / s, out[3] = pz / s;
  return true;
}

// One leg's contact trust at control iteration `tick`, on swing_decide's own integers
// (swing_counts): 0 exactly when swing_decide returns a swing state; 1 for a leg that never
// swings or a malformed record; in stance, with nst = dur ibm control iterations of stance,
// k = 1 .. nst the one this is and phi = (k - 1/2) / nst, the ramp min(1, phi / w, (1 - phi) / w)
// over the window w (w = 0: 1).
__host__ __device__ inline double att_trust(int tick, int ibm, int period, int off, int dur, double window) {
#pragma clang fp contract(off)
  long long cs, nsw;
  if (!swing_counts(tick, ibm, period, off, dur, &cs, &nsw)) return 1.0;
  if (cs != 0 && cs <= nsw) return 0.0;
  const long long nst = (long long)dur * ibm;
  if (nst <= 0 || !(window > 0.0)) return 1.0;
  const long long k = cs == 0 ? nst : cs - nsw;
  const double phi = ((double)k - 0.5) / (double)nst;
  const double up = phi / window, down = (1.0 - phi) / window;
  double t = 1.0;
  if (up < t) t = up;
  if (down < t) t = down;
  return t;
}

// Robot b's share of mpcqp_attitude: `tick` / `gait` / `touch` and every output are nullable.
// A non-finite gyro, accel, record or touch value: the record is not written, the status is
// ATT_STATUS_NONFINITE and quat / gyro_out come from the record as it was; a non-finite
// touch also sets the robot's four trusts to 0.
__host__ __device__ inline void att_robot(const AttParams& ap, size_t b, const float* gyro, const float* accel,
                                          const int32_t* tick, int ibm, const int32_t* gait, const float* touch,
                                          double* att_state, float* quat, float* gyro_out, float* trust,
                                          int32_t* status) {
#pragma clang fp contract(off)
  AttPair* rp = (AttPair*)(att_state + ATT_STRIDE * b);
  double rec[ATT_STRIDE], out[ATT_STRIDE], w[3], a[3];
#pragma unroll
  for (int k = 0; k < ATT_STRIDE / 2; ++k) {
    const AttPair p = rp[k];
    rec[2 * k] = p.a, rec[2 * k + 1] = p.b;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    w[k] = (double)gyro[3 * b + k];
    a[k] = (double)accel[3 * b + k];
  }
  float tv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  bool touch_ok = true;
  if (touch != nullptr) {
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      tv[l] = touch[4 * b + l];
      touch_ok = touch_ok && isfinite(tv[l]);
    }
  }
  const bool ok = att_tick(ap, rec, w, a, out) && touch_ok;
  if (ok) {
#pragma unroll
    for (int k = 0; k < ATT_STRIDE / 2; ++k) {
      AttPair p;
      p.a = out[2 * k], p.b = out[2 * k + 1];
      rp[k] = p;
    }
  } else if (!touch_ok) {
    att_as_was(rec, out);   // att_tick went through on its own
  }
  if (quat != nullptr) {
#pragma unroll
    for (int k = 0; k < 4; ++k) quat[4 * b + k] = (float)out[k];
  }
  if (gyro_out != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) gyro_out[3 * b + k] = (float)(w[k] - out[ATT_BIAS + k]);
  }
  if (trust != nullptr) {
    int g[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int tk = 0;
    if (gait != nullptr) {
#pragma unroll
      for (int k = 0; k < 9; ++k) g[k] = gait[9 * b + k];
      tk = tick[b];
    }
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      double t = gait != nullptr ? att_trust(tk, ibm, g[0], g[1 + l], g[5 + l], ap.trust_window) : 1.0;
      if (touch != nullptr && !((double)tv[l] > ap.touch_threshold)) t = 0.0;
      trust[4 * b + l] = touch_ok ? (float)t : 0.0f;
    }
  }
  if (status != nullptr) status[b] = ok ? ATT_STATUS_OK : ATT_STATUS_NONFINITE;
}

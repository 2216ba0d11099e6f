// mpcqp_sensors_robot.h -- per-robot algebra of the sensor model and of the push
// (mpcqp_sensors.h), host- and device-callable so tests/ can check it on the CPU against
// tests/disturb_ref.py.  The reference has neither: its scripts read a simulator's sensors as
// they come and never disturb the robot (gym.simulate, sim.step()).
//
//   sense_philox    one Philox4x32-10 block
//   sense_normals   two words -> two standard normals (Box-Muller, float64)
//   sense_joint     block j = 0..11: one joint's (q, qdot) as the encoder reads it
//   sense_axis      block 12 + a:    one IMU axis, its two bias words advanced
//   sense_feet      block 15:        the four touch sensors, their histories advanced
//   sense_robot     the 16 blocks of one robot strung together (the host build;
//                   mpcqp_sensors_kernel strings the same functions together with one lane per block)
//   push_robot      an impulse on one robot's plant record
//
// A robot's draws are a pure function of (seed, its id, its count of accepted calls): block j of
// a call has the counter (count mod 2^32, count div 2^32, id, j) and the key (seed mod 2^32,
// seed div 2^32).  Everything but the generator is float64 on the float32 inputs; FP contraction
// is off and log, sin and cos are spelled out here, so the host build, the device build and the
// restatement give the same bits.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "mpcqp_plant_robot.h"

// the record: SENSE_STRIDE float64 words per robot
constexpr int SENSE_BIAS_G = 0, SENSE_BIAS_A = 3, SENSE_INIT = 6, SENSE_COUNT = 7, SENSE_ID = 8, SENSE_HIST = 9,
              SENSE_WORDS = 13, SENSE_STRIDE = 16;
constexpr int SENSE_BLOCKS = 16;      // Philox blocks per robot and call: 12 joints, 3 axes, the feet
constexpr int SENSE_STATUS_OK = 0, SENSE_STATUS_NONFINITE = 4;
constexpr int SENSE_MAX_LAG = 31;

struct SenseParams {
  uint32_t key0, key1;                // seed mod 2^32, seed div 2^32
  double sigma_gyro, sigma_accel;     // white, per sample
  double walk_gyro, walk_accel;       // bias random walk per sqrt(s)
  double bias0_gyro, bias0_accel;     // turn-on bias, 1 sigma
  double sigma_q, sigma_qd, q_lsb;
  double sqrt_dt;                     // sqrt(dt_control)
  uint32_t drop;                      // floor(p_drop 2^32): a reading is dropped iff its word < drop
  int touch_lag;                      // 0 .. SENSE_MAX_LAG
};

__host__ __device__ inline void sense_mulhilo(uint32_t a, uint32_t b, uint32_t* hi, uint32_t* lo) {
  const uint64_t p = (uint64_t)a * (uint64_t)b;
  *hi = (uint32_t)(p >> 32);
  *lo = (uint32_t)p;
}

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3; SC11).
__host__ __device__ inline void sense_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                             uint32_t k1, uint32_t* out) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t h0, l0, h1, l1;
    sense_mulhilo(0xD2511F53u, c0, &h0, &l0);
    sense_mulhilo(0xCD9E8D57u, c2, &h1, &l1);
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// ln x for a normal x > 0, and sin, cos of 2 pi u for u in [0, 1], spelled out in IEEE operations
// (+, -, *, /, each rounded once, no contraction) so that the host build, the device build and
// the NumPy restatement give the same bits: a library's log, sin and cos differ between the three
// in the last place, and a turn-on bias one ulp off is a run that is not reproduced word for
// word.  The evaluation is the classical one (Sun's fdlibm, e_log.c, k_sin.c, k_cos.c: the
// argument split as 2^k (1 + f), s = f / (2 + f) and an even polynomial in s; the angle reduced
// exactly to a quarter turn and |y| <= pi / 4, then the two kernels' polynomials), within 1e-15
// of the exact value relative to the result's size, which is all a noise sample needs.
__host__ __device__ inline double sense_log(double x) {
#pragma clang fp contract(off)
  uint64_t b;
  memcpy(&b, &x, 8);
  int k = (int)(b >> 52) - 1023;
  const uint64_t m = b & 0xFFFFFFFFFFFFFull;
  const bool up = m >= 0x6A09E667F3BCDull;   // the mantissa of sqrt(2): 1 + f lies in [sqrt(1/2), sqrt(2))
  k += up ? 1 : 0;
  b = m | ((up ? 1022ull : 1023ull) << 52);
  double xm;
  memcpy(&xm, &b, 8);
  const double f = xm - 1.0, dk = (double)k;
  const double s = f / (2.0 + f), z = s * s, w = z * z;
  const double t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01));
  const double t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)));
  const double R = t2 + t1, hfsq = 0.5 * f * f;
  return dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + dk * 1.90821492927058770002e-10)) - f);
}

__host__ __device__ inline void sense_sincos_turn(double u, double* sn, double* cs) {
#pragma clang fp contract(off)
  const double kf = floor(4.0 * u + 0.5);      // the nearest quarter turn, 0 .. 4
  const double y = 6.283185307179586 * (u - 0.25 * kf);   // u - kf / 4 is exact, |y| <= pi / 4
  const double z = y * y;
  const double rs = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
  const double s = y + (z * y) * (-1.66666666666666324348e-01 + z * rs);
  const double rc = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 + z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
  const double c = 1.0 - (0.5 * z - z * rc);
  const int q = (int)kf & 3;
  *sn = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
  *cs = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
}

// u = (w + 0.5) 2^-32 lies in (0, 1): r = sqrt(-2 ln u0) <= 6.77, z0 = r cos 2 pi u1, z1 = r sin 2 pi u1.
__host__ __device__ inline void sense_normals(uint32_t w0, uint32_t w1, double* z0, double* z1) {
#pragma clang fp contract(off)
  const double u0 = ((double)w0 + 0.5) * 2.3283064365386963e-10;   // 2^-32
  const double u1 = ((double)w1 + 0.5) * 2.3283064365386963e-10;
  const double r = sqrt(-2.0 * sense_log(u0));
  double sn, cs;
  sense_sincos_turn(u1, &sn, &cs);
  *z0 = r * cs;
  *z1 = r * sn;
}

// x + add, and x itself (its sign of zero too) where there is nothing to add: with every
// constant zero the stage is then the identity bit by bit.
__host__ __device__ inline double sense_add(double x, double add) {
#pragma clang fp contract(off)
  return add == 0.0 ? x : x + add;
}

// Block j = 0..11, joint j: the normals of words 0, 1 are (zq, zqd); words 2, 3 are not used.
// s is the robot's scale.
__host__ __device__ inline void sense_joint(const SenseParams& P, double s, double zq, double zqd, float q, float qd,
                                            float* qm, float* qdm) {
#pragma clang fp contract(off)
  double a = sense_add((double)q, (s * P.sigma_q) * zq);
  if (P.q_lsb > 0.0) a = rint(a / P.q_lsb) * P.q_lsb;
  *qm = (float)a;
  *qdm = (float)sense_add((double)qd, (s * P.sigma_qd) * zqd);
}

// Block 12 + a, IMU axis a: the normals of words 0, 1 are (zg, za), the white noise of gyro and
// accelerometer, those of words 2, 3 (zwg, zwa), the walk's.  A record that is not initialised
// draws its turn-on bias from the walk's normals and does not walk in that call.  bg, ba: the
// axis' two bias words, in/out.
__host__ __device__ inline void sense_axis(const SenseParams& P, double s, double zg, double za, double zwg, double zwa,
                                           bool init, float gyro, float accel, double* bg, double* ba, float* gm,
                                           float* am) {
#pragma clang fp contract(off)
  if (init) {
    *bg = sense_add(*bg, ((s * P.walk_gyro) * P.sqrt_dt) * zwg);
    *ba = sense_add(*ba, ((s * P.walk_accel) * P.sqrt_dt) * zwa);
  } else {
    *bg = (s * P.bias0_gyro) * zwg;
    *ba = (s * P.bias0_accel) * zwa;
  }
  *gm = (float)sense_add((double)gyro, *bg + (s * P.sigma_gyro) * zg);
  *am = (float)sense_add((double)accel, *ba + (s * P.sigma_accel) * za);
}

// Block 15, the feet: word f is foot f's dropout draw.  hist: the four histories (integers below
// 2^32 held in float64), in/out; touch NULL: the histories stay and nothing is written.
__host__ __device__ inline void sense_feet(const SenseParams& P, const uint32_t* w, bool init, const float* touch,
                                           double* hist, float* touch_m) {
  if (touch == nullptr) return;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const uint32_t now = touch[f] > 0.f ? 1u : 0u;
    const uint32_t h = init ? ((uint32_t)hist[f] << 1) | now : 0u - now;   // the start makes no edges
    const bool on = ((h >> P.touch_lag) & 1u) != 0u && !(w[f] < P.drop);
    hist[f] = (double)h;
    touch_m[f] = on ? 1.f : 0.f;
  }
}

// Whether word k of a record can be used: finite, and where it is read as an integer within that
// integer's range -- the count in [0, 2^53), the id and the four histories in [0, 2^32) -- so that
// no conversion is undefined and the host and the device draw alike.
__host__ __device__ inline bool sense_word_ok(int k, double v) {
  if (!isfinite(v)) return false;
  if (k == SENSE_COUNT) return v >= 0.0 && v < 9007199254740992.0;
  if (k == SENSE_ID || (k >= SENSE_HIST && k < SENSE_WORDS)) return v >= 0.0 && v < 4294967296.0;
  return true;
}

// The scale of a robot (NULL: 1) and whether it is usable: finite and not negative.
__host__ __device__ inline bool sense_scale(const float* scale, double* s) {
  *s = scale != nullptr ? (double)*scale : 1.0;
  return isfinite(*s) && *s >= 0.0;
}

// One call of one robot: rec [SENSE_STRIDE] in/out, the four groups (in, out) each nullable as a
// pair, an output may be its input.  A non-finite input, a non-finite or negative scale or a
// record word 0 .. SENSE_WORDS - 1 that is not finite or outside its integer's range
// (sense_word_ok) refuses the robot: SENSE_STATUS_NONFINITE, the
// record untouched, its outputs its inputs.
__host__ __device__ inline int sense_robot(const SenseParams& P, double* rec, const float* gyro, const float* accel,
                                           const float* dofs, const float* touch, const float* scale, float* gyro_m,
                                           float* accel_m, float* dofs_m, float* touch_m) {
  double s;
  bool ok = sense_scale(scale, &s);
  for (int k = 0; k < SENSE_WORDS; ++k) ok = ok && sense_word_ok(k, rec[k]);
  for (int k = 0; k < 3; ++k) {
    if (gyro != nullptr) ok = ok && isfinite(gyro[k]);
    if (accel != nullptr) ok = ok && isfinite(accel[k]);
  }
  for (int k = 0; k < 24; ++k)
    if (dofs != nullptr) ok = ok && isfinite(dofs[k]);
  for (int k = 0; k < 4; ++k)
    if (touch != nullptr) ok = ok && isfinite(touch[k]);
  if (!ok) {
    for (int k = 0; k < 3; ++k) {
      if (gyro != nullptr) gyro_m[k] = gyro[k];
      if (accel != nullptr) accel_m[k] = accel[k];
    }
    for (int k = 0; k < 24; ++k)
      if (dofs != nullptr) dofs_m[k] = dofs[k];
    for (int k = 0; k < 4; ++k)
      if (touch != nullptr) touch_m[k] = touch[k];
    return SENSE_STATUS_NONFINITE;
  }
  const bool init = rec[SENSE_INIT] != 0.0;
  const uint64_t count = (uint64_t)rec[SENSE_COUNT];
  const uint32_t c0 = (uint32_t)count, c1 = (uint32_t)(count >> 32), id = (uint32_t)(uint64_t)rec[SENSE_ID];
  uint32_t w[4];
  for (int j = 0; j < 12; ++j) {
    sense_philox(c0, c1, id, (uint32_t)j, P.key0, P.key1, w);
    double zq, zqd;
    sense_normals(w[0], w[1], &zq, &zqd);
    if (dofs != nullptr) sense_joint(P, s, zq, zqd, dofs[2 * j], dofs[2 * j + 1], dofs_m + 2 * j, dofs_m + 2 * j + 1);
  }
  for (int a = 0; a < 3; ++a) {
    sense_philox(c0, c1, id, (uint32_t)(12 + a), P.key0, P.key1, w);
    float gm, am;
    double zg, za, zwg, zwa;
    sense_normals(w[0], w[1], &zg, &za);
    sense_normals(w[2], w[3], &zwg, &zwa);
    sense_axis(P, s, zg, za, zwg, zwa, init, gyro != nullptr ? gyro[a] : 0.f, accel != nullptr ? accel[a] : 0.f, rec + SENSE_BIAS_G + a,
               rec + SENSE_BIAS_A + a, &gm, &am);
    if (gyro != nullptr) gyro_m[a] = gm;
    if (accel != nullptr) accel_m[a] = am;
  }
  sense_philox(c0, c1, id, 15u, P.key0, P.key1, w);
  sense_feet(P, w, init, touch, rec + SENSE_HIST, touch_m);
  rec[SENSE_INIT] = 1.0;
  rec[SENSE_COUNT] = rec[SENSE_COUNT] + 1.0;
  return SENSE_STATUS_OK;
}

// An impulse J (world frame, N s) on the plant record rec [PLANT_STRIDE] at the body-frame point
// r = point from the centre of mass (at_point false: at the centre of mass, point is not read): v += J / m, w += I_w^-1 ((Rq r) x J) with
// I_w = Rq I Rq^T as plant_body_substep forms it.  Feet, contacts, flag word and call count are
// not written; a zero impulse leaves the record bit by bit.  A non-finite impulse or point, a
// non-finite or non-invertible robot record or plant record, or a non-finite result refuses the
// robot: PLANT_STATUS_NONFINITE and the record untouched.
__host__ __device__ inline int push_robot(double* rec, const float* impulse, const float* point, bool at_point,
                                          const float* robot) {
#pragma clang fp contract(off)
  PlantConst C;
  bool ok = plant_const_load(robot, &C) && plant_all_finite(rec, PLANT_WORDS);
  double J[3], r[3] = {0.0, 0.0, 0.0}, v[3], w[3];
  for (int k = 0; k < 3; ++k) {
    J[k] = (double)impulse[k];
    ok = ok && isfinite(impulse[k]);
    if (at_point) {
      r[k] = (double)point[k];
      ok = ok && isfinite(point[k]);
    }
  }
  const double* qt = rec + PLANT_QUAT;
  ok = ok && ((qt[0] * qt[0] + qt[1] * qt[1]) + qt[2] * qt[2]) + qt[3] * qt[3] > 0.0;
  if (!ok) return PLANT_STATUS_NONFINITE;
  for (int k = 0; k < 3; ++k) {
    v[k] = sense_add(rec[PLANT_VEL + k], J[k] / C.m);
    w[k] = rec[PLANT_OMEGA + k];
  }
  if (at_point) {
    double Rq[9], rw[3], t[3], dw[3];
    kin_quat2matrix(qt[0], qt[1], qt[2], qt[3], Rq);
    swing_mat3(Rq, r, rw);
    plant_cross(rw, J, t);
    plant_world_apply(Rq, C.Ii, t, dw);
    for (int k = 0; k < 3; ++k) w[k] = sense_add(w[k], dw[k]);
  }
  if (!(plant_all_finite(v, 3) && plant_all_finite(w, 3))) return PLANT_STATUS_NONFINITE;
  for (int k = 0; k < 3; ++k) {
    rec[PLANT_VEL + k] = v[k];
    rec[PLANT_OMEGA + k] = w[k];
  }
  return PLANT_STATUS_OK;
}

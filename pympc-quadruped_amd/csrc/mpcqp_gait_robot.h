// mpcqp_gait_robot.h -- per-robot decision of the gait scheduler (mpcqp_gait.h), host- and
// device-callable so tests/ can check it on the CPU.
//
//   gait_mid_swing   is a leg between its first and its last swing tick     gait.py:102-121, on
//                                                                           swing_counts' integers
//   gait_seam        may a robot's record be replaced at this tick
//   gait_entry       the segment a record is entered at                     the restart at iter_counter 0
//                                                                           of scripts/mujoco_aliengo.py:121-155
//   gait_auto        the request the command asks for (thresholds, dwell)
//   gait_robot       one robot's share of a launch: clock, request, switch, stores
//
// Everything is an integer but the command of the automatic choice (float64, contraction off so
// that the host build and the device build compare alike).  Nothing here depends on a lane; the
// library record of a switching robot comes through `fetch`: the kernel's reads the context's
// device copy, the host build's a host array.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "mpcqp_swing_leg.h"   // swing_counts, SW_ARMED, SW_LEG_STRIDE

// the record (int32 words): the library index in force (-1: a record set by hand), the latched
// request, control iterations since the last switch (saturating), the number of switches, the
// calm counter of the automatic choice, the tick just before the last switch; two words kept
constexpr int SCHED_CUR = 0, SCHED_PENDING = 1, SCHED_SINCE = 2, SCHED_SWITCHES = 3, SCHED_CALM = 4,
              SCHED_LAST = 5, SCHED_STRIDE = 8;
constexpr int GAIT_WORDS = 9;        // MPCQP_GAIT_STRIDE: period, offsets[4], durations[4]
constexpr int GAIT_LIB_WORDS = 10;   // a library entry: the record and its entry segment
constexpr int GAIT_LIB_MAX = 16;     // MPCQP_GAIT_MAX
constexpr int GAIT_MAX_PERIOD = 2048;
constexpr int GAIT_SWING_WORDS = 4 * SW_LEG_STRIDE;   // MPCQP_SWING_STRIDE
constexpr int GAIT_ADVANCE = 1;      // MPCQP_GAIT_ADVANCE
constexpr int GAIT_STATUS_OK = 0, GAIT_STATUS_NONFINITE = 4, GAIT_STATUS_UNSUPPORTED = 5;
constexpr int GAIT_INT_MAX = 2147483647;

struct GaitParams {
  int count;       // library entries
  int ibm;         // iterations_between_mpc
  int flags;
  int min_hold;
  int idle, move;  // the automatic choice's two entries (idle < 0: disabled)
  int dwell;
  double v_go2, v_stop2, w_go, w_stop;   // the speeds squared
};

// half a record: the record is 16-byte aligned, so it moves as two of these
struct alignas(16) GaitQuad {
  int32_t a, b, c, d;
};

// Leg (off, dur) of a record of period P is mid-swing at tick t: past its first swing tick and
// before its last.  cs == 0 (about to lift), cs == nsw (the last swing tick, which a fresh start
// repeats as its one-tick hold at tick 0) and cs > nsw (stance) are not, nor is a leg that never
// swings.
__host__ __device__ inline bool gait_mid_swing(int t, int ibm, int period, int off, int dur) {
  long long cs, nsw;
  if (!swing_counts(t, ibm, period, off, dur, &cs, &nsw)) return false;
  return cs >= 1 && cs < nsw;
}

// t (>= 0) is a seam of the record g: a multiple of ibm at which no leg is mid-swing
__host__ __device__ inline bool gait_seam(int t, int ibm, const int* g) {
  if ((unsigned)t % (unsigned)ibm != 0u) return false;
  bool mid = false;
#pragma unroll
  for (int l = 0; l < 4; ++l) mid = mid || gait_mid_swing(t, ibm, g[0], g[1 + l], g[5 + l]);
  return !mid;
}

// The smallest segment s in [0, P) whose first tick is a seam of g, or -1 where there is none.
// In segments the seam condition does not depend on ibm, so it is taken at ibm = 1.
inline int gait_entry(const int* g) {
  for (int s = 0; s < g[0]; ++s)
    if (gait_seam(s, 1, g)) return s;
  return -1;
}

// A library record is valid: 1 <= P <= 2048, 0 <= dur <= P, |off| <= 4 P
inline bool gait_record_valid(const int* g) {
  if (g[0] < 1 || g[0] > GAIT_MAX_PERIOD) return false;
  for (int l = 0; l < 4; ++l) {
    if (g[5 + l] < 0 || g[5 + l] > g[0]) return false;
    if (g[1 + l] > 4 * g[0] || g[1 + l] < -4 * g[0]) return false;
  }
  return true;
}

// The library mpcqp_set_gaits keeps, from `count` records of GAIT_WORDS words: entries of
// GAIT_LIB_WORDS words into lib (GAIT_LIB_MAX entries, the unused ones zero).  Returns 0, or with
// lib untouched 1 for a count outside 1 .. GAIT_LIB_MAX or no records, 2 for a record out of
// range and 3 for one that cannot be entered (*which: its index).
inline int gait_library(int count, const int* records, int* lib, int* which) {
  *which = -1;
  if (count < 1 || count > GAIT_LIB_MAX || records == nullptr) return 1;
  int out[GAIT_LIB_MAX * GAIT_LIB_WORDS] = {};
  for (int i = 0; i < count; ++i) {
    int* e = out + GAIT_LIB_WORDS * i;
    for (int k = 0; k < GAIT_WORDS; ++k) e[k] = records[GAIT_WORDS * i + k];
    *which = i;
    if (!gait_record_valid(e)) return 2;
    e[GAIT_WORDS] = gait_entry(e);
    if (e[GAIT_WORDS] < 0) return 3;
  }
  for (int k = 0; k < GAIT_LIB_MAX * GAIT_LIB_WORDS; ++k) lib[k] = out[k];
  return 0;
}

// (tick / ibm) mod P, mpcqp_plan's `iteration`, on swing_counts' own reduction of the tick (a
// negative tick counts from the end of the span); 0 for a record without a period
__host__ __device__ inline int gait_iteration(int t, int ibm, int period) {
  if (period <= 0) return 0;
  const long long span = (long long)ibm * period;
  long long c = (long long)t % span;
  if (c < 0) c += span;
  return (int)(c / ibm);
}

// The automatic choice for one robot: move above either go threshold; idle once the command has
// been at or below both stop thresholds for `dwell` consecutive calls, this one included; in
// between the latched request stays and the calm count restarts.  False for a non-finite
// command, with nothing changed.
__host__ __device__ inline bool gait_auto(const GaitParams& gp, double vx, double vy, double yaw, int* pending,
                                          int* calm) {
#pragma clang fp contract(off)
  if (!(isfinite(vx) && isfinite(vy) && isfinite(yaw))) return false;
  const double v2 = vx * vx + vy * vy, w = fabs(yaw);
  if (v2 > gp.v_go2 || w > gp.w_go) {
    *pending = gp.move;
    *calm = 0;
  } else if (v2 <= gp.v_stop2 && w <= gp.w_stop) {
    if (*calm < GAIT_INT_MAX) *calm += 1;
    if (*calm >= gp.dwell) *pending = gp.idle;
  } else {
    *calm = 0;
  }
  return true;
}

// Robot b's share of mpcqp_gait_schedule.  `want`, `vel_body_des` / `yaw_rate_des` (used when
// want is NULL), `swing_mem`, `iteration`, `switched` and `status` are nullable.
// fetch(w, rec): library entry w's GAIT_LIB_WORDS words into rec.  A robot that does not switch
// stores its tick and the halves of its record that changed; one whose tick is refused stores
// nothing but the outputs.
template <class Fetch>
__host__ __device__ inline void gait_robot(const GaitParams& gp, size_t b, const int32_t* want,
                                           const double* vel_body_des, const double* yaw_rate_des,
                                           int32_t* sched_state, int32_t* gait, int32_t* tick, double* swing_mem,
                                           int32_t* iteration, int32_t* switched, int32_t* status, Fetch fetch) {
  GaitQuad* rp = (GaitQuad*)(sched_state + SCHED_STRIDE * b);
  const bool advance = (gp.flags & GAIT_ADVANCE) != 0;
  int t = tick[b];
  int st = GAIT_STATUS_OK, did = 0;
  if (t < 0 || (advance && t == GAIT_INT_MAX)) {
    st = GAIT_STATUS_UNSUPPORTED;   // the clock cannot advance: the robot is left as it is
  } else {
    const GaitQuad lo = rp[0], hi = rp[1];
    int cur = lo.a, pending = lo.b, since = lo.c, switches = lo.d, calm = hi.a, last = hi.b;
    if (advance) {
      t += 1;
      if (since < GAIT_INT_MAX) since += 1;
    }
    if (want != nullptr) {
      const int w = want[b];
      if (w >= 0 && w < gp.count)
        pending = w;
      else if (w != -1)
        st = GAIT_STATUS_UNSUPPORTED;   // an index outside the library: no request
    } else {
      const double vx = vel_body_des[3 * b], vy = vel_body_des[3 * b + 1], yaw = yaw_rate_des[b];
      if (!gait_auto(gp, vx, vy, yaw, &pending, &calm)) st = GAIT_STATUS_NONFINITE;
    }
    // only a robot with a request in force reaches a division: its tick against ibm, and on an
    // aligned tick swing_counts' remainders
    if (st != GAIT_STATUS_NONFINITE && pending != cur && pending >= 0 && pending < gp.count && since >= gp.min_hold) {
      int g[GAIT_WORDS];
#pragma unroll
      for (int k = 0; k < GAIT_WORDS; ++k) g[k] = gait[GAIT_WORDS * b + k];
      if (gait_seam(t, gp.ibm, g)) {
        int rec[GAIT_LIB_WORDS];
        fetch(pending, rec);
#pragma unroll
        for (int k = 0; k < GAIT_WORDS; ++k) gait[GAIT_WORDS * b + k] = rec[k];
        last = t;
        t = rec[GAIT_WORDS] * gp.ibm;   // the entry segment's first tick: congruent to the old one mod ibm
        if (swing_mem != nullptr) {
#pragma unroll
          for (int l = 0; l < 4; ++l) swing_mem[GAIT_SWING_WORDS * b + SW_LEG_STRIDE * l + SW_ARMED] = 0.0;
        }
        cur = pending;
        since = 0;
        switches = (int)((unsigned)switches + 1u);
        did = 1;
      }
    }
    tick[b] = t;
    GaitQuad nlo;
    nlo.a = cur, nlo.b = pending, nlo.c = since, nlo.d = switches;
    rp[0] = nlo;
    if (calm != hi.a || last != hi.b) {
      GaitQuad nhi = hi;
      nhi.a = calm, nhi.b = last;
      rp[1] = nhi;
    }
  }
  if (iteration != nullptr) iteration[b] = gait_iteration(t, gp.ibm, gait[GAIT_WORDS * b]);
  if (switched != nullptr) switched[b] = did;
  if (status != nullptr) status[b] = st;
}

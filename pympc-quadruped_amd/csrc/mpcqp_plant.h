// mpcqp_plant.h -- the rigid-body plant on the device: for every robot in one launch the physical
// state advanced by one control iteration under the joint torques it is given, and the next
// root_states / dof_states in the simulator's layout with the raw sensors (included by mpcqp.hip
// inside its anonymous namespace, after mpcqp_predict.h).  The algebra is mpcqp_plant_robot.h;
// this file maps a wavefront's lanes onto it.
//
// One lane per leg, a robot's four legs in adjacent lanes (a quad), 16 robots per wavefront, one
// wavefront per workgroup -- the shape of mpcqp_step_kernel without its LDS record:
//   load     lane l of a quad loads words 12 l .. 12 l + 11 of the robot's float64 record as six
//            16-byte loads: the 384-byte record is read once.  Every word is then handed to the
//            lanes that need it by DPP quad broadcasts: the body (13 words) to all four, a leg's
//            foot position, velocity and contact flag to its own lane
//   substep  each lane its leg (plant_leg_substep); the four forces and moments meet through two
//            DPP quad exchanges, (F0 + F1) + (F2 + F3) on every lane; each lane then advances the
//            body for itself (plant_body_substep: all four get the same bits), so nothing is
//            broadcast back.  The substeps loop here
//   outputs  each lane its leg's joint angles and rates; lane 0 of the quad the root state and
//            the sensors.  The pass that forms them is the loop's last, so that the inverse
//            kinematics -- the bulk of the code -- stands once
//   store    the record is assembled back into the four 12-word chunks by quad broadcasts and
//            stored with six 16-byte stores per lane (lane 3: three and one word, the record's
//            43 words end in its chunk)
// No LDS, no atomics, no allocation, synchronisation or host read: the launch can be captured
// into a HIP graph.  No private memory: every array index is a compile-time constant after
// unrolling.
#include "mpcqp_plant_robot.h"

static_assert(PLANT_STRIDE == MPCQP_PLANT_STRIDE, "record stride");
static_assert(PLANT_STATUS_OK == MPCQP_STATUS_OK && PLANT_STATUS_NONFINITE == MPCQP_STATUS_NONFINITE, "status words");
static_assert(PLANT_STRIDE == 4 * 12 && PLANT_WORDS <= PLANT_STRIDE, "four chunks of twelve words");

constexpr int kPlantRobots = 16;   // per wavefront and workgroup
constexpr int kPlantThreads = 64;

// A DPP move inside the quad: CTRL is the quad_perm selector (two bits per destination lane).
template <int CTRL>
__device__ __forceinline__ double plant_quad_move(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
// the value of quad lane S on all four lanes
template <int S>
__device__ __forceinline__ double plant_quad_bcast(double v) {
  return plant_quad_move<S * 0x55>(v);
}
// v0 + v1 + v2 + v3 as (own pair) + (other pair): the same bits on all four lanes
__device__ __forceinline__ double plant_quad_sum(double v) {
#pragma clang fp contract(off)
  v = v + plant_quad_move<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v = v + plant_quad_move<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  return v;
}
__device__ __forceinline__ int plant_quad_or(int v) {
  v |= __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false);
  v |= __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false);
  return v;
}

// A launch-wide value moved into a vector register, where the compiler no longer knows that all
// lanes hold the same: it then stays out of the scalar registers, which the float64 constants of
// the trigonometric code fill (a value held there across the whole kernel is spilled and
// reloaded around every call of them).
template <typename T>
__device__ __forceinline__ T plant_per_lane(T v) {
  asm volatile("" : "+v"(v));
  return v;
}

// Word W of the record, W a compile-time constant, from the chunk registers c[12] of the quad:
// the same value on all four lanes.
template <int W>
__device__ __forceinline__ double plant_word(const double (&c)[12]) {
  return plant_quad_bcast<W / 12>(c[W % 12]);
}
// Word BASE + STEP leg + K for this lane's leg: the four candidates, then a select.
template <int BASE, int STEP, int K>
__device__ __forceinline__ double plant_leg_word(const double (&c)[12], int leg) {
  const double w0 = plant_word<BASE + K>(c), w1 = plant_word<BASE + STEP + K>(c),
               w2 = plant_word<BASE + 2 * STEP + K>(c), w3 = plant_word<BASE + 3 * STEP + K>(c);
  return leg == 0 ? w0 : leg == 1 ? w1 : leg == 2 ? w2 : w3;
}

// The state of a robot as its lanes hold it: the body on every lane, the lane's own leg.
struct PlantLane {
  double pos[3], quat[4], v[3], w[3];
  double pf[3], vf[3];
  bool contact, contact_finite;   // the leg's contact word: set, and finite as loaded
};

__device__ __forceinline__ void plant_unpack(const double (&c)[12], int leg, PlantLane& s, double* flags, double* tick) {
  s.pos[0] = plant_word<PLANT_POS>(c);
  s.pos[1] = plant_word<PLANT_POS + 1>(c);
  s.pos[2] = plant_word<PLANT_POS + 2>(c);
  s.quat[0] = plant_word<PLANT_QUAT>(c);
  s.quat[1] = plant_word<PLANT_QUAT + 1>(c);
  s.quat[2] = plant_word<PLANT_QUAT + 2>(c);
  s.quat[3] = plant_word<PLANT_QUAT + 3>(c);
  s.v[0] = plant_word<PLANT_VEL>(c);
  s.v[1] = plant_word<PLANT_VEL + 1>(c);
  s.v[2] = plant_word<PLANT_VEL + 2>(c);
  s.w[0] = plant_word<PLANT_OMEGA>(c);
  s.w[1] = plant_word<PLANT_OMEGA + 1>(c);
  s.w[2] = plant_word<PLANT_OMEGA + 2>(c);
  s.pf[0] = plant_leg_word<PLANT_FEET, 3, 0>(c, leg);
  s.pf[1] = plant_leg_word<PLANT_FEET, 3, 1>(c, leg);
  s.pf[2] = plant_leg_word<PLANT_FEET, 3, 2>(c, leg);
  s.vf[0] = plant_leg_word<PLANT_FVEL, 3, 0>(c, leg);
  s.vf[1] = plant_leg_word<PLANT_FVEL, 3, 1>(c, leg);
  s.vf[2] = plant_leg_word<PLANT_FVEL, 3, 2>(c, leg);
  const double ct = plant_leg_word<PLANT_CONTACT, 1, 0>(c, leg);
  s.contact = ct != 0.0;
  s.contact_finite = isfinite(ct);
  *flags = plant_word<PLANT_FLAGS>(c);
  *tick = plant_word<PLANT_TICK>(c);
}

// Word W of the record to store, from the lanes' state: a body word is on every lane, a leg's
// word comes from its lane.
template <int W>
__device__ __forceinline__ double plant_pack_word(const PlantLane& s, double flags, double tick) {
  if constexpr (W < PLANT_QUAT) return s.pos[W - PLANT_POS];
  else if constexpr (W < PLANT_VEL) return s.quat[W - PLANT_QUAT];
  else if constexpr (W < PLANT_OMEGA) return s.v[W - PLANT_VEL];
  else if constexpr (W < PLANT_FEET) return s.w[W - PLANT_OMEGA];
  else if constexpr (W < PLANT_FVEL) return plant_quad_bcast<(W - PLANT_FEET) / 3>(s.pf[(W - PLANT_FEET) % 3]);
  else if constexpr (W < PLANT_CONTACT) return plant_quad_bcast<(W - PLANT_FVEL) / 3>(s.vf[(W - PLANT_FVEL) % 3]);
  else if constexpr (W < PLANT_FLAGS) return plant_quad_bcast<W - PLANT_CONTACT>(s.contact ? 1.0 : 0.0);
  else if constexpr (W == PLANT_FLAGS) return flags;
  else if constexpr (W == PLANT_TICK) return tick;
  else return 0.0;
}
// Word I of this lane's chunk: word 12 leg + I.
template <int I>
__device__ __forceinline__ double plant_pack_chunk(const PlantLane& s, double flags, double tick, int leg) {
  const double w0 = plant_pack_word<I>(s, flags, tick), w1 = plant_pack_word<12 + I>(s, flags, tick),
               w2 = plant_pack_word<24 + I>(s, flags, tick), w3 = plant_pack_word<36 + I>(s, flags, tick);
  return leg == 0 ? w0 : leg == 1 ? w1 : leg == 2 ? w2 : w3;
}

__device__ __forceinline__ bool plant_lane_finite(const PlantLane& s) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    ok = ok & isfinite(s.pos[k]) & isfinite(s.v[k]) & isfinite(s.w[k]) & isfinite(s.pf[k]) & isfinite(s.vf[k]);
#pragma unroll
  for (int k = 0; k < 4; ++k) ok = ok & isfinite(s.quat[k]);
  return ok;
}

// One lane's float32 outputs, held in registers until the robot's status is known.
struct PlantOut {
  float q[3], qd[3], gyro[3], accel[3], root[13];
};

// The outputs of one robot from the lanes' state, the attitude's matrix and the leg's
// plant_leg_state (q, r, Ji).  Returns whether every float32 output of this lane is finite.
__device__ __forceinline__ bool plant_lane_outputs(const PlantLane& s, const double* Rq, const double* q, const double* r,
                                                   const double* Ji, const double* spec, PlantOut& o) {
#pragma clang fp contract(off)
  double qd[3], gb[3], ab[3];
  plant_leg_rate(Rq, r, Ji, s.v, s.w, s.vf, qd);
  swing_mat3t(Rq, s.w, gb);
  swing_mat3t(Rq, spec, ab);
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o.q[k] = (float)q[k];
    o.qd[k] = (float)qd[k];
    o.gyro[k] = (float)gb[k];
    o.accel[k] = (float)ab[k];
    o.root[k] = (float)s.pos[k];
    o.root[3 + k] = (float)s.quat[1 + k];
    o.root[7 + k] = (float)s.v[k];
    o.root[10 + k] = (float)s.w[k];
    ok = ok & isfinite(o.q[k]) & isfinite(o.qd[k]) & isfinite(o.gyro[k]) & isfinite(o.accel[k]);
  }
  o.root[6] = (float)s.quat[0];
#pragma unroll
  for (int k = 0; k < 13; ++k) ok = ok & isfinite(o.root[k]);
  return ok;
}

// The chunk of this lane: words 12 leg .. 12 leg + 11 of the robot's record, six 16-byte loads.
__device__ __forceinline__ void plant_load_chunk(const double2* __restrict__ chunk, double (&c)[12]) {
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double2 v = chunk[k];
    c[2 * k] = v.x;
    c[2 * k + 1] = v.y;
  }
}

__global__ __launch_bounds__(kPlantThreads) void mpcqp_plant_kernel(
    PlantParams P, int B, const float* __restrict__ taug, const float* __restrict__ robotg,
    const double* __restrict__ geomg, const float* __restrict__ planeg, double* __restrict__ stateg,
    float* __restrict__ root, float* __restrict__ dofs, float* __restrict__ gyro, float* __restrict__ accel,
    float* __restrict__ touch, int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  const int leg = t & 3;
  const int b = blockIdx.x * kPlantRobots + (t >> 2);
  if (b >= B) return;   // whole quads leave: a quad's four lanes share b
  const size_t bs = (size_t)b;

  // this lane's output addresses, formed now: a null output stays null.  Held per lane they live in
  // vector registers, where there is room; the six uniform pointers would sit in scalar
  // registers across the whole kernel, which the trigonometric code needs for its constants
  const size_t bl = bs * 4 + leg;
  float2* const dofs_p = plant_per_lane(dofs != nullptr ? reinterpret_cast<float2*>(dofs + bl * 6) : nullptr);   // 24 bytes per leg
  float* const touch_p = plant_per_lane(touch != nullptr ? touch + bl : nullptr);
  float* const root_p = plant_per_lane(root != nullptr && leg == 0 ? root + bs * 13 : nullptr);
  float* const gyro_p = plant_per_lane(gyro != nullptr && leg == 0 ? gyro + bs * 3 : nullptr);
  float* const accel_p = plant_per_lane(accel != nullptr && leg == 0 ? accel + bs * 3 : nullptr);
  int32_t* const status_p = plant_per_lane(status != nullptr && leg == 0 ? status + bs : nullptr);
  // the constants of the launch likewise
  PlantParams Q;
  Q.dt_control = plant_per_lane(P.dt_control);
  Q.gravity = plant_per_lane(P.gravity);
  Q.foot_mass = plant_per_lane(P.foot_mass);
  Q.ground_z = plant_per_lane(P.ground_z);
  Q.contact_tol = 0.0;   // mpcqp_plant_reset's
  Q.substeps = plant_per_lane(P.substeps);

  // ---- load: the record's chunk, the leg's torques, the robot's constants
  double2* const chunk = reinterpret_cast<double2*>(stateg + bs * PLANT_STRIDE + 12 * leg);
  double c[12];
  plant_load_chunk(chunk, c);
  double tau[3], geom[5];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float v = taug[(bs * 4 + leg) * 3 + k];
    tau[k] = (double)v;
    ok = ok & isfinite(v);
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    geom[k] = geomg[bs * KIN_STRIDE + k];
    ok = ok & isfinite(geom[k]);
  }
  PlantConst C;
  ok = plant_const_load(robotg + bs * MPCQP_ROBOT_STRIDE, &C) && ok;
  ok = plant_const_plane(planeg != nullptr ? planeg + bs * 4 : nullptr, Q.ground_z, &C) && ok;
  PlantLane s;
  double flags, tick;
  plant_unpack(c, leg, s, &flags, &tick);
  ok = ok && plant_lane_finite(s) && s.contact_finite && isfinite(flags) && isfinite(tick);
  ok = ok && ((s.quat[0] * s.quat[0] + s.quat[1] * s.quat[1]) + s.quat[2] * s.quat[2]) + s.quat[3] * s.quat[3] > 0.0;
  bool refused = plant_quad_or(ok ? 0 : 1) != 0;   // quad-uniform, as every decision on it below

  // ---- the substeps, then the outputs: one loop, so that the legs' inverse kinematics stands
  // once in the code.  Pass `it` < substeps advances the state; the pass after the last substep
  // forms the outputs of the new state.  A refused robot goes straight to an output pass over
  // the untouched record (read again: nothing has been stored) with the specific force of a
  // robot at rest -- at the start for a bad input, after the substeps for a non-finite state,
  // after the output pass for a float32 output that is not finite.
  const double h = Q.dt_control / (double)Q.substeps;
  double spec[3] = {0.0, 0.0, Q.gravity};
  bool cl = false;
  PlantOut o;
  int it = refused ? Q.substeps : 0;
  for (;;) {
    double Rq[9], r[3], q[3], Ji[9], gl[5];
    // the geometry and the leg index taken anew in every pass: what the compiler derives from them
    // (the special cases of atan2 on thigh_y, the masks of leg == k) is then formed where it is
    // used, not ahead of the loop and held in scalar registers across it
#pragma unroll
    for (int k = 0; k < 5; ++k) gl[k] = plant_per_lane(geom[k]);
    const int legl = plant_per_lane(leg);
    kin_quat2matrix(s.quat[0], s.quat[1], s.quat[2], s.quat[3], Rq);
    const bool c1 = plant_leg_state(gl, legl, Rq, s.pos, s.pf, r, q, Ji);
    if (it >= Q.substeps) {
      const bool fin = plant_lane_outputs(s, Rq, q, r, Ji, spec, o);
      cl = cl || c1;
      if (refused || plant_quad_or(fin ? 0 : 1) == 0) break;
      refused = true;
    } else {
      double F[3], M[3], SF[3], SM[3];
      cl = cl || c1;
      plant_leg_force(Q, C, Rq, r, Ji, tau, h, s.pf, s.vf, &s.contact, F, M);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        SF[k] = plant_quad_sum(F[k]);
        SM[k] = plant_quad_sum(M[k]);
      }
      plant_body_substep(Q, C, h, SF, SM, s.pos, s.quat, s.v, s.w, Rq, spec);
      ++it;
      if (it == Q.substeps) refused = plant_quad_or(plant_lane_finite(s) ? 0 : 1) != 0;
    }
    if (refused) {
      plant_load_chunk(chunk, c);
      plant_unpack(c, legl, s, &flags, &tick);
      spec[0] = 0.0;
      spec[1] = 0.0;
      spec[2] = Q.gravity;
    }
  }

  // ---- store
  if (dofs_p != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) dofs_p[k] = make_float2(o.q[k], o.qd[k]);
  }
  if (touch_p != nullptr) *touch_p = s.contact ? 1.f : 0.f;
  if (root_p != nullptr) {
#pragma unroll
    for (int k = 0; k < 13; ++k) root_p[k] = o.root[k];
  }
  if (gyro_p != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) gyro_p[k] = o.gyro[k];
  }
  if (accel_p != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) accel_p[k] = o.accel[k];
  }
  if (status_p != nullptr) *status_p = refused ? MPCQP_STATUS_NONFINITE : MPCQP_STATUS_OK;
  if (!refused) {
    flags = (double)plant_quad_or(cl ? 1 << leg : 0);
    tick = tick + 1.0;
    const int leg = plant_per_lane(t & 3);   // formed anew: the selects below do not reach back to the load's
    double w[12];
    w[0] = plant_pack_chunk<0>(s, flags, tick, leg);
    w[1] = plant_pack_chunk<1>(s, flags, tick, leg);
    w[2] = plant_pack_chunk<2>(s, flags, tick, leg);
    w[3] = plant_pack_chunk<3>(s, flags, tick, leg);
    w[4] = plant_pack_chunk<4>(s, flags, tick, leg);
    w[5] = plant_pack_chunk<5>(s, flags, tick, leg);
    w[6] = plant_pack_chunk<6>(s, flags, tick, leg);
    w[7] = plant_pack_chunk<7>(s, flags, tick, leg);
    w[8] = plant_pack_chunk<8>(s, flags, tick, leg);
    w[9] = plant_pack_chunk<9>(s, flags, tick, leg);
    w[10] = plant_pack_chunk<10>(s, flags, tick, leg);
    w[11] = plant_pack_chunk<11>(s, flags, tick, leg);
    // lane 3 stores words 36 .. 42 alone: words 43 .. 47 (the stride's padding) keep what they held
#pragma unroll
    for (int k = 0; k < 3; ++k) chunk[k] = make_double2(w[2 * k], w[2 * k + 1]);
    if (leg == 3) {
      reinterpret_cast<double*>(chunk)[6] = w[6];
    } else {
#pragma unroll
      for (int k = 3; k < 6; ++k) chunk[k] = make_double2(w[2 * k], w[2 * k + 1]);
    }
  }
}

// mpcqp_plant_reset: one thread per robot, the header's plant_robot_reset as it stands.
__global__ __launch_bounds__(64) void mpcqp_plant_reset_kernel(PlantParams P, int B, const float* __restrict__ root,
                                                               const float* __restrict__ dofs,
                                                               const double* __restrict__ geom,
                                                               const float* __restrict__ plane,
                                                               double* __restrict__ state) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const size_t bs = (size_t)b;
  double rec[PLANT_STRIDE];
  plant_robot_reset(P, root + bs * 13, dofs + bs * 24, geom + bs * KIN_STRIDE, plane != nullptr ? plane + bs * 4 : nullptr, rec);
  double2* out = reinterpret_cast<double2*>(state + bs * PLANT_STRIDE);
#pragma unroll
  for (int k = 0; k < PLANT_STRIDE / 2; ++k) out[k] = make_double2(rec[2 * k], rec[2 * k + 1]);
}

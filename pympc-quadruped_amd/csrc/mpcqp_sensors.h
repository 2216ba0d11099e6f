// mpcqp_sensors.h -- the sensor model and the push on the device: between the plant and the
// sensing chain, what a robot's IMU, encoders and touch sensors would report of the plant's exact
// outputs (white noise, a bias that is drawn at turn-on and walks, encoder quantisation, a touch
// signal that lags and drops out), one launch per control iteration; and an impulse on the
// plant's record (included by mpcqp.hip inside its anonymous namespace, after mpcqp_gait.h).
// The reference has neither: its scripts read a simulator's sensors as they come
// (gym.simulate, sim.step()).  The algebra is mpcqp_sensors_robot.h; this file maps a wavefront's
// lanes onto it.
//
// mpcqp_sensors_kernel: 16 lanes per robot, four robots per wavefront, four wavefronts per
// workgroup.  A lane is one Philox block of its robot, and the block's index is the lane's:
//   lanes 0..11   joint j: its (q, qdot) pair, one 8-byte load and store; one Box-Muller pair
//   lanes 12..14  IMU axis a with the axis' two bias words; two Box-Muller pairs
//   lane  15      the four feet with their histories, the robot's initialised word and count
// Every lane reads the three record words all share (initialised, count, id) and word `lane` of
// the record for the finiteness check itself: the 128-byte record is one cache line, and a value
// handed round by cross-lane moves would save no memory transaction.  The one thing the 16 lanes
// must agree on is the refusal -- a robot with a non-finite input, scale or record word draws
// nothing and keeps its record -- which is a ballot masked to the robot's 16 lanes: no LDS, no
// barrier.  The first Box-Muller pair runs on every lane at once and the second on the IMU lanes
// alone, so a wavefront pays for two, not three.  No atomics, allocation, synchronisation or
// host read: the launch can be captured into a HIP graph.  No private memory: every array index
// is a compile-time constant after unrolling.  An output may be its input: each lane reads what
// it writes before it writes it, and the in/out groups carry no __restrict__.
//
// mpcqp_push_kernel: one thread per robot, the header's push_robot on a register copy of the
// record's body words.
#include "mpcqp_sensors_robot.h"

static_assert(SENSE_STRIDE == MPCQP_SENSE_STRIDE, "record stride");
static_assert(SENSE_STATUS_OK == MPCQP_STATUS_OK && SENSE_STATUS_NONFINITE == MPCQP_STATUS_NONFINITE, "status words");
static_assert(SENSE_BLOCKS == 16 && SENSE_STRIDE == 16, "one lane per block and per record word");

// A value made opaque to the compiler where it stands: what follows uses this instruction's
// output, so the load behind it is neither moved past this point nor issued again.
__device__ __forceinline__ double sense_pin(double v) {
  asm volatile("" : "+v"(v));
  return v;
}

constexpr int kSenseThreads = 256;
constexpr int kSenseRobots = kSenseThreads / SENSE_BLOCKS;   // per workgroup

__global__ __launch_bounds__(kSenseThreads) void mpcqp_sensors_kernel(
    SenseParams P, int B, const float* gyro, const float* accel, const float* dofs, const float* touch,
    const float* __restrict__ scale, double* __restrict__ state, float* gyro_m, float* accel_m, float* dofs_m,
    float* touch_m, int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  const int l = t & (SENSE_BLOCKS - 1);
  const int b = blockIdx.x * kSenseRobots + t / SENSE_BLOCKS;
  if (b >= B) return;   // whole robots leave: a robot's 16 lanes share b
  const size_t bs = (size_t)b;
  double* const rec = state + bs * SENSE_STRIDE;
  const bool joint = l < 12, feet = l == 15, axis = !joint && !feet;
  const int a = l - 12;

  // ---- load: the shared words, this lane's word for the check, this lane's inputs
  // Ordering.  Lanes 12..15 later store words that other lanes of the robot read here, and only
  // the wavefront's program order puts the reads first.  Every read of a shared word feeds the
  // vote and every store is control-dependent on the vote, so no read can move below a store.
  // The three words all lanes share pass through sense_pin on the way: from there on they are
  // the outputs of an opaque instruction, not loads, so the compiler can neither sink the loads
  // into the branches below nor repeat them there.  (Reading them through a volatile pointer
  // pins them as well and measured 0.1 us slower in a graph, 4.36 against 4.25 us.)
  const double mine = rec[l];
  const double initw = sense_pin(rec[SENSE_INIT]), countw = sense_pin(rec[SENSE_COUNT]), idw = sense_pin(rec[SENSE_ID]);
  double s;
  bool ok = sense_scale(scale != nullptr ? scale + bs : nullptr, &s);
  ok = ok && (l >= SENSE_WORDS || sense_word_ok(l, mine));
  ok = ok && isfinite(initw) && isfinite(countw) && isfinite(idw);
  float in0 = 0.f, in1 = 0.f, in2 = 0.f, in3 = 0.f;   // (q, qdot), (gyro, accel) or the four feet
  double w0 = 0.0, w1 = 0.0, w2 = 0.0, w3 = 0.0;      // (b_g, b_a) or the four histories
  if (joint) {
    if (dofs != nullptr) {
      const float2 v = reinterpret_cast<const float2*>(dofs)[bs * 12 + l];
      in0 = v.x;
      in1 = v.y;
    }
  } else if (axis) {
    if (gyro != nullptr) in0 = gyro[bs * 3 + a];
    if (accel != nullptr) in1 = accel[bs * 3 + a];
    w0 = rec[SENSE_BIAS_G + a];
    w1 = rec[SENSE_BIAS_A + a];
  } else {
    if (touch != nullptr) {
      in0 = touch[bs * 4];
      in1 = touch[bs * 4 + 1];
      in2 = touch[bs * 4 + 2];
      in3 = touch[bs * 4 + 3];
    }
    w0 = rec[SENSE_HIST];
    w1 = rec[SENSE_HIST + 1];
    w2 = rec[SENSE_HIST + 2];
    w3 = rec[SENSE_HIST + 3];
  }
  ok = ok && isfinite(in0) && isfinite(in1) && isfinite(in2) && isfinite(in3);

  // ---- the robot's refusal: a vote over its 16 lanes
  const unsigned long long votes = __ballot(!ok);
  const bool refused = ((votes >> (t & 48)) & 0xffffull) != 0ull;

  float out0 = in0, out1 = in1, out2 = in2, out3 = in3;   // a refused robot's outputs are its inputs
  if (!refused) {
    const bool init = initw != 0.0;
    const uint64_t count = (uint64_t)countw;
    uint32_t w[4];
    sense_philox((uint32_t)count, (uint32_t)(count >> 32), (uint32_t)(uint64_t)idw, (uint32_t)l, P.key0, P.key1, w);
    double z0, z1;
    sense_normals(w[0], w[1], &z0, &z1);
    if (joint) {
      sense_joint(P, s, z0, z1, in0, in1, &out0, &out1);
    } else if (axis) {
      double z2, z3;
      sense_normals(w[2], w[3], &z2, &z3);
      sense_axis(P, s, z0, z1, z2, z3, init, in0, in1, &w0, &w1, &out0, &out1);
      rec[SENSE_BIAS_G + a] = w0;
      rec[SENSE_BIAS_A + a] = w1;
    } else {
      if (touch != nullptr) {
        const float tin[4] = {in0, in1, in2, in3};
        double h[4] = {w0, w1, w2, w3};
        float tm[4];
        sense_feet(P, w, init, tin, h, tm);
        out0 = tm[0], out1 = tm[1], out2 = tm[2], out3 = tm[3];
        rec[SENSE_HIST] = h[0];
        rec[SENSE_HIST + 1] = h[1];
        rec[SENSE_HIST + 2] = h[2];
        rec[SENSE_HIST + 3] = h[3];
      }
      rec[SENSE_INIT] = 1.0;
      rec[SENSE_COUNT] = countw + 1.0;
    }
  }

  // ---- store
  if (joint) {
    if (dofs_m != nullptr) reinterpret_cast<float2*>(dofs_m)[bs * 12 + l] = make_float2(out0, out1);
    if (l == 0 && status != nullptr) status[bs] = refused ? MPCQP_STATUS_NONFINITE : MPCQP_STATUS_OK;
  } else if (axis) {
    if (gyro_m != nullptr) gyro_m[bs * 3 + a] = out0;
    if (accel_m != nullptr) accel_m[bs * 3 + a] = out1;
  } else if (touch_m != nullptr) {
    touch_m[bs * 4] = out0;
    touch_m[bs * 4 + 1] = out1;
    touch_m[bs * 4 + 2] = out2;
    touch_m[bs * 4 + 3] = out3;
  }
}

// mpcqp_push: one thread per robot.  The record's 43 words are read (a non-finite one refuses the
// robot, as in mpcqp_plant); velocity and rate alone are written, and only where the robot is
// not refused.
__global__ __launch_bounds__(64) void mpcqp_push_kernel(int B, const float* __restrict__ impulse,
                                                        const float* __restrict__ point,
                                                        const float* __restrict__ robot, double* __restrict__ state,
                                                        int32_t* __restrict__ status) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;   // lanes past the batch touch no memory
  const size_t bs = (size_t)b;
  double rec[PLANT_STRIDE];
  const double2* in = reinterpret_cast<const double2*>(state + bs * PLANT_STRIDE);
#pragma unroll
  for (int k = 0; k < PLANT_STRIDE / 2; ++k) {
    const double2 v = in[k];
    rec[2 * k] = v.x;
    rec[2 * k + 1] = v.y;
  }
  float J[3], r[3], rb[8];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    J[k] = impulse[bs * 3 + k];
    r[k] = point != nullptr ? point[bs * 3 + k] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) rb[k] = robot[bs * MPCQP_ROBOT_STRIDE + k];
  const int st = push_robot(rec, J, r, point != nullptr, rb);
  if (status != nullptr) status[bs] = st;
  if (st != PLANT_STATUS_OK) return;
  double* out = state + bs * PLANT_STRIDE;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    out[PLANT_VEL + k] = rec[PLANT_VEL + k];
    out[PLANT_OMEGA + k] = rec[PLANT_OMEGA + k];
  }
}

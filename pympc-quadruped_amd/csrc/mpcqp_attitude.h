// mpcqp_attitude.h -- the orientation filter and the contact trust on the device: what
// mpcqp_estimate takes as `quat` and `trust`, for every robot in one launch (included by
// mpcqp.hip inside its anonymous namespace, after mpcqp_estimator.h).  It is the first stage
// of doc/state_estimation_kf.md (section 2: the gyro integrated, pitch and roll de-drifted
// towards the accelerometer's gravity direction) and the stance-phase trust ramp of the
// Cheetah 3 filter the document follows, gated by the touch sensor of
// scripts/mujoco_aliengo.py:101-118.  The algebra is mpcqp_attitude_robot.h.
//
// One thread per robot: a robot is 8 doubles of record, 6 + 4 floats of sensors and a
// 9-word gait record, and its tick is one short dependent chain (two square roots, a sincos,
// a handful of divisions), so there is nothing to spread over lanes and nothing to share
// between them -- no LDS, no barrier.  A workgroup is one wavefront: the launch is
// latency-bound at any fleet size (B = 8192 is 128 wavefronts on 256 CUs), so every
// wavefront gets a CU, and a SIMD, of its own.
#include "mpcqp_attitude_robot.h"

constexpr int kAttThreads = 64;

__global__ __launch_bounds__(kAttThreads) void mpcqp_attitude_kernel(
    AttParams ap, int B, int ibm, const float* __restrict__ gyro, const float* __restrict__ accel,
    const int32_t* __restrict__ tick, const int32_t* __restrict__ gait, const float* __restrict__ touch,
    double* __restrict__ att_state, float* __restrict__ quat, float* __restrict__ gyro_out,
    float* __restrict__ trust, int32_t* __restrict__ status) {
  const int b = blockIdx.x * kAttThreads + threadIdx.x;
  if (b >= B) return;   // lanes past the batch touch no memory
  att_robot(ap, (size_t)b, gyro, accel, tick, ibm, gait, touch, att_state, quat, gyro_out, trust, status);
}

// mpcqp_gait.h -- the gait scheduler on the device: the stage that owns every robot's gait
// record and control-iteration counter, one launch per control iteration (included by mpcqp.hip
// inside its anonymous namespace, after mpcqp_plant.h).  It replaces what the reference does by
// hand between two runs -- fresh Gait objects and iter_counter back at 0
// (scripts/mujoco_aliengo.py:121-155, gait.py:76-121) -- by a switch at a tick where no leg is
// between its first and its last swing tick.  The decision is mpcqp_gait_robot.h.
//
// One thread per robot: a robot is 8 words of record, its tick and, only while a request waits
// on an aligned tick, its 9-word gait record; nothing is shared between robots, so there is no
// LDS and no barrier, and a workgroup is one wavefront as in mpcqp_attitude.h.  The library (at
// most 16 entries of 10 words, 640 bytes that stay in the caches) is read only by the lanes
// that switch, at most once per robot and seam, with three vector loads each; a lane that does
// not switch issues no load of it.  Neither staging it in LDS (a load of the whole library and
// a barrier in every wavefront of every launch, for a read that almost no launch makes) nor a
// readfirstlane loop towards scalar loads (the compiler folds "the uniform index equals mine"
// back into the per-lane address and emits the same vector loads) buys anything.
#include "mpcqp_gait_robot.h"

constexpr int kGaitThreads = 64;

// Library entry w for the lane that asks.  w lies in [0, count): gait_robot checks it before it
// asks.  Plain vector loads (see the head of this file).
struct GaitFetch {
  const int32_t* __restrict__ lib;
  __device__ void operator()(int w, int* rec) const {
    const int32_t* __restrict__ e = lib + GAIT_LIB_WORDS * w;
#pragma unroll
    for (int k = 0; k < GAIT_LIB_WORDS; ++k) rec[k] = e[k];
  }
};

__global__ __launch_bounds__(kGaitThreads) void mpcqp_gait_kernel(
    GaitParams gp, int B, const int32_t* __restrict__ lib, const int32_t* __restrict__ want,
    const double* __restrict__ vel_body_des, const double* __restrict__ yaw_rate_des, int32_t* __restrict__ sched_state,
    int32_t* __restrict__ gait, int32_t* __restrict__ tick, double* __restrict__ swing_mem,
    int32_t* __restrict__ iteration, int32_t* __restrict__ switched, int32_t* __restrict__ status) {
  const int b = blockIdx.x * kGaitThreads + threadIdx.x;
  if (b >= B) return;   // lanes past the batch touch no memory
  gait_robot(gp, (size_t)b, want, vel_body_des, yaw_rate_des, sched_state, gait, tick, swing_mem, iteration, switched,
             status, GaitFetch{lib});
}

// mpcqp_terrain.h -- the terrain plane on the device: each robot's ground plane fitted to the
// world positions its feet had while in contact, for every robot in one launch (included by
// mpcqp.hip inside its anonymous namespace, after mpcqp_attitude.h).  It is
// RobotData.update_terrain_normal (utils/robot_data.py:186-228), which the reference defines
// and never calls; here it produces the surface normal the cone rows read from the robot
// record and the ground plane of the swing leg (mpcqp_set_ground).  The algebra is
// mpcqp_terrain_robot.h.
//
// One thread per robot, as mpcqp_attitude_kernel: a robot is 20 doubles of record and 12 + 4
// floats of input, its tick one dependent chain (18 Jacobi rotations), so there is nothing to
// spread over lanes and nothing to share between them -- no LDS, no barrier.  A workgroup is
// one wavefront.
#include "mpcqp_terrain_robot.h"

constexpr int kTerThreads = 64;

__global__ __launch_bounds__(kTerThreads) void mpcqp_terrain_kernel(
    TerParams tp, int B, const float* __restrict__ pos_feet, const float* __restrict__ contact,
    const float* __restrict__ quat, double* __restrict__ terrain_state, float* robot, float* __restrict__ normal,
    float* __restrict__ plane, float* __restrict__ normal_base, int32_t* __restrict__ status) {
  const int b = blockIdx.x * kTerThreads + threadIdx.x;
  if (b >= B) return;   // lanes past the batch touch no memory
  ter_robot(tp, (size_t)b, pos_feet, contact, quat, terrain_state, robot, normal, plane, normal_base, status);
}

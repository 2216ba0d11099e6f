// mpcqp.hip -- MI355X (gfx950) batched convex-MPC QP engine: the context and the C ABI.  The
// device code is in the headers included below (mpcqp_device.h: the prelude; one kernel header
// per stage; mpcqp_classes.h: the solve's kernels), the solve's routing in mpcqp_solve_plan.h.
//
// Replaces, for a batch of independent robots, the per-tick formulate-and-solve of
// ModelPredictiveController._solve_mpc (/root/reference/linear_mpc/mpc.py:262-290):
// model (mpc.py:173-192), discretisation (:194-208), condensing and H/g (:211-235),
// friction-cone rows (:237-260) and the Drake-branch QP (:277-286)
//
//   min 1/2 U^T H U + g^T U   s.t.  lb <= C U <= ub,   C = kron(I_4N, cone)
//
// generalised to a per-robot cone normal (normal = e_z reproduces mpc.py exactly).
//
// ONE WORKGROUP PER ROBOT, nothing but the inputs and outputs touches HBM:
//   class NV =  64: 2 waves, n = 3 * #stance <= 64   (mpcqp_kernel_64)
//   class NV =  96: 6 waves, 4 x 6 tiles, n <= 96   (mpcqp_kernel_96, fed by a
//                   device queue the first class fills)
//   class NV = 128: 8 waves, n <= 126                (mpcqp_kernel_128, fed by a
//                   device queue the first class fills)
//   large class:    1 wave, n up to 12 N = 240       (mpcqp_kernel_ipm: Riccati-factored
//                   interior point + exact active-set polish, mpcqp_ipm.h)
// Formulation in closed form (mpcqp_form.h); H^-1 by a symmetric sweep over
// register tiles; Goldfarb-Idnani dual active set in projected form with the
// reduced inverse Hessian and the multiplier map in registers (mpcqp_solve.h).

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <cmath>
#include <initializer_list>
#include <string.h>

#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "mpcqp.h"
#include "mpcqp_predict_abi.h"
#include "mpcqp_plant_abi.h"
#include "mpcqp_certify_abi.h"
#include "mpcqp_gait_abi.h"
#include "mpcqp_disturb_abi.h"
#include "mpcqp_solve_plan.h"

namespace {

#include "mpcqp_device.h"
#include "mpcqp_form.h"
#include "mpcqp_combo_asm.h"
#include "mpcqp_solve.h"
#include "mpcqp_ipm.h"
#include "mpcqp_plan.h"
#include "mpcqp_swing.h"
#include "mpcqp_kinematics.h"
#include "mpcqp_step.h"
#include "mpcqp_estimator.h"
#include "mpcqp_attitude.h"
#include "mpcqp_terrain.h"
#include "mpcqp_predict.h"
#include "mpcqp_certify.h"
#include "mpcqp_plant.h"
#include "mpcqp_gait.h"
#include "mpcqp_sensors.h"
// the kernel headers' constants are those of include/mpcqp.h
static_assert(MPCQP_KIN_STRIDE == KIN_STRIDE, "geometry record: include/mpcqp.h and mpcqp_kin_leg.h agree");
static_assert(EST_STRIDE == MPCQP_EST_STRIDE, "estimator record stride");
static_assert(ATT_STRIDE == MPCQP_ATT_STRIDE, "attitude record stride");
static_assert(ATT_STATUS_OK == MPCQP_STATUS_OK && ATT_STATUS_NONFINITE == MPCQP_STATUS_NONFINITE, "status words");
static_assert(TER_STRIDE == MPCQP_TERRAIN_STRIDE, "terrain record stride");
static_assert(TER_ROBOT_STRIDE == MPCQP_ROBOT_STRIDE && TER_ROBOT_NORMAL == MPCQP_ROBOT_NORMAL &&
                  MPCQP_ROBOT_NORMAL + 3 <= MPCQP_ROBOT_STRIDE, "the normal's words of the robot record");
static_assert(TER_SWING_STATE == MPCQP_TERRAIN_SWING_STATE && TER_ROOT_STATES == MPCQP_TERRAIN_ROOT_STATES, "flags");
static_assert(TER_GROUND == MPCQP_TERRAIN_GROUND, "flags");
static_assert(TER_STATUS_OK == MPCQP_STATUS_OK && TER_STATUS_NONFINITE == MPCQP_STATUS_NONFINITE, "status words");
static_assert(SCHED_STRIDE == MPCQP_SCHED_STRIDE && GAIT_WORDS == MPCQP_GAIT_STRIDE && GAIT_LIB_MAX == MPCQP_GAIT_MAX &&
                  GAIT_SWING_WORDS == MPCQP_SWING_STRIDE && GAIT_ADVANCE == MPCQP_GAIT_ADVANCE, "scheduler record and library");
static_assert(GAIT_STATUS_OK == MPCQP_STATUS_OK && GAIT_STATUS_NONFINITE == MPCQP_STATUS_NONFINITE &&
                  GAIT_STATUS_UNSUPPORTED == MPCQP_STATUS_UNSUPPORTED, "status words");

#include "mpcqp_classes.h"

}  // namespace

// ============================================================== C ABI
// Device queues of one stream: three queues of [count, next, finished, pad, robots...
// (cap)] -- class 64 -> class 96, -> class 128, -> the interior-point class.  Calls on
// one stream are ordered, so the count / reset protocol of the queued kernels is
// safe; calls on different streams of one context use different queue sets.
struct QueueSet {
  hipStream_t stream;
  int cap;
  int* buf;
  unsigned long long used;   // last use (LRU eviction beyond kMaxQueueSets streams)
  // the interior-point class runs on a side stream forked from `stream` after the first
  // (routing) class and joined back at the end of the call (created on first use)
  hipStream_t side;
  hipEvent_t ev_fork, ev_join;
  hipEvent_t ev_done;   // recorded on `stream` after each call's last launch (eviction waits on it)
};

// Releases a queue set's device resources (the caller has synchronised the device).
static void release_set(QueueSet& q) {
  if (q.buf) (void)hipFree(q.buf);
  if (q.ev_fork) (void)hipEventDestroy(q.ev_fork);
  if (q.ev_join) (void)hipEventDestroy(q.ev_join);
  if (q.ev_done) (void)hipEventDestroy(q.ev_done);
  q.ev_done = nullptr;
  if (q.side) (void)hipStreamDestroy(q.side);
  q.buf = nullptr;
  q.ev_fork = q.ev_join = nullptr;
  q.side = nullptr;
}

struct mpcqp_ctx {
  // mpcqp_create sets params, device, ncu, q_full / r_full and prio_tab; every other default is here
  mpcqp_params params;
  int device = 0;
  int stance_hint = 0;   // max stance foot-steps per robot promised by the caller (0: none)
  int stance_min = 0;    // min stance foot-steps per robot promised by the caller
  int order = 1;         // dispatch order (mpcqp_set_order): 1 = predicted-cost order, 0 = batch order
  int ncu = 0;
  std::vector<QueueSet> queues;
  unsigned long long use_clock = 0;
  // class 64's setup-priority table (kPrioTab u64, solve_robot) and the launch epoch its entries
  // carry: a launch's entries beat every earlier launch's, so the table is cleared only at
  // creation and when the 32-bit epoch wraps
  unsigned long long* prio_tab = nullptr;
  unsigned prio_epoch = 0;
  // the interior-point class's global slots (Riccati S_k; at N <= 16 also M_k, M_k^T and the
  // saved iterate): kIpmPerCU per CU, one pool for every stream of the context (the slots in
  // use never exceed the class's resident workgroups, whichever launches they belong to),
  // ipm_slot_doubles(horizon) each, then the slot bitmap; allocated on first use
  double* sscratch = nullptr;
  int sslots = 0;
  double* wdev = nullptr;   // full Q (13 x 13) then R (12 x 12) on the device (mpcqp_set_weights); nullptr: diagonal
  bool xr = false;          // R couples different legs: the interior-point class's XR instantiations
  double q_full[13 * 13];   // the current weights as whole matrices (host copies: a NULL argument
  double r_full[12 * 12];   // of mpcqp_set_weights keeps that matrix, off-diagonal entries included)
  std::vector<double*> retired;   // earlier full-weight buffers (in-flight solves may read them)
  unsigned char* warm = nullptr;   // warm-start memory (caller-owned device buffer), mpcqp_set_warm_start
  int warm_cap = 0;
  double dt_control = 0.001;    // planner constants (mpcqp_set_planner); linear_mpc_configs.py:6
  double gravity = 9.81;        // linear_mpc_configs.py:13
  double max_pos_error = 0.1;   // mpc.py:121
  double swing_height = 0.1;    // swing constants (mpcqp_set_swing); robot_configs.py:54
  double touchdown_z = -0.0255; // swing_foot_trajectory_generator.py:120
  double vel_gain = 0.03;       // swing_foot_trajectory_generator.py:116
  double kp_swing[9] = {700.0, 0.0, 0.0, 0.0, 700.0, 0.0, 0.0, 0.0, 700.0};   // robot_configs.py:55-56
  double kd_swing[9] = {20.0, 0.0, 0.0, 0.0, 20.0, 0.0, 0.0, 0.0, 20.0};
  // estimator constants (mpcqp_set_estimator): the Cheetah 3 software's noise values folded into
  // rates (include/mpcqp.h)
  EstParams est{0, 0.001, 9.81, 0.001, 0.0098, 0.002, 0.001, 0.1, 0.001, 100.0, 100.0, 0.0};
  // orientation-filter and contact-trust constants (mpcqp_set_attitude): the document's kappa_ref,
  // no bias estimate; the trust ramps over the first and last fifth of the stance
  AttParams att{0.001, 9.81, 0.1, 0.0, 0.2, 0.0};
  // terrain-plane constants (mpcqp_set_terrain): a contact flag of 1 counts, the fit unfiltered as
  // in the reference, held where the feet are nearly collinear or the plane steeper than 60 degrees
  TerParams ter{0.5, 1e-3, 0.5, 1.0, 0, 0.0};
  const float* ground = nullptr;   // the swing leg's ground planes (caller-owned device buffer), mpcqp_set_ground
  int ground_cap = 0;
  // plant constants (mpcqp_set_plant); ground_z follows the swing's touchdown_z until it is set
  double plant_foot_mass = 0.15;
  int plant_substeps = 1;
  double plant_ground_z = 0.0;
  bool plant_ground_set = false;
  double plant_contact_tol = 1e-4;
  // the gait library (mpcqp_set_gaits): entries of GAIT_LIB_WORDS words, the record and its entry
  // segment, on the host and on the device; and the scheduler's constants (mpcqp_set_gait_schedule)
  int gait_count = 0;
  int gait_lib[GAIT_LIB_MAX * GAIT_LIB_WORDS] = {};
  int32_t* gait_dev = nullptr;
  std::vector<int32_t*> gait_retired;   // earlier libraries (in-flight launches may read them)
  int sched_min_hold = 0;
  int sched_idle = -1, sched_move = -1, sched_dwell = 0;
  double sched_v_go = 0.0, sched_v_stop = 0.0, sched_w_go = 0.0, sched_w_stop = 0.0;
  // the sensor model's constants (mpcqp_set_sensors): all zero, the stage is the identity on values
  uint64_t sense_seed = 0;
  double sense_sigma_gyro = 0.0, sense_sigma_accel = 0.0, sense_walk_gyro = 0.0, sense_walk_accel = 0.0;
  double sense_bias0_gyro = 0.0, sense_bias0_accel = 0.0, sense_sigma_q = 0.0, sense_sigma_qd = 0.0, sense_q_lsb = 0.0;
  int sense_touch_lag = 0;
  double sense_p_drop = 0.0;
  std::string err;
};

static int set_err(mpcqp_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

// After a kernel launch: MPCQP_OK, or the launch error as "<what>: <HIP's text>".
static int launched(mpcqp_ctx* ctx, const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return MPCQP_OK;
  return set_err(ctx, MPCQP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// MPCQP_OK for a 16-byte aligned record buffer, else the refusal that names it.
static int aligned16(mpcqp_ctx* ctx, const void* p, const char* name) {
  if (((uintptr_t)p & 15) == 0) return MPCQP_OK;
  return set_err(ctx, MPCQP_ERR_ARG, std::string(name) + " is not 16-byte aligned");
}

static bool all_finite(std::initializer_list<double> values) {
  for (double v : values)
    if (!std::isfinite(v)) return false;
  return true;
}

// The swing-leg constants of a launch: every kernel that moves a swing leg takes them from here.
static SwingParams swing_params(const mpcqp_ctx* ctx, int ibm, int root_layout) {
  SwingParams sp;
  sp.ibm = ibm;
  sp.root_layout = root_layout;
  sp.dt_control = ctx->dt_control;
  sp.gravity = ctx->gravity;
  sp.swing_height = ctx->swing_height;
  sp.touchdown_z = ctx->touchdown_z;
  sp.vel_gain = ctx->vel_gain;
  memcpy(sp.Kp, ctx->kp_swing, sizeof(sp.Kp));
  memcpy(sp.Kd, ctx->kd_swing, sizeof(sp.Kd));
  sp.ground = ctx->ground;
  sp.ground_cap = ctx->ground_cap;
  return sp;
}

// Makes the context's device current for one ABI call and restores the caller's.
struct DeviceScope {
  int prev = -1;
  bool ok = false;
  explicit DeviceScope(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// At most this many streams keep a queue set; a new stream beyond them takes over the
// least recently used set with its buffers, once the event recorded after that set's last
// call has completed (its stream may still run launches that use it, and may already have
// been destroyed by the caller: the event outlives it).  No device-wide synchronisation.
constexpr int kMaxQueueSets = 8;
// Full-weight buffers retired by mpcqp_set_weights before one device-wide release.
constexpr size_t kMaxRetired = 64;

// The queue set of `st`, holding at least `batch` robots per queue (grown on demand;
// the old buffer is freed once the stream's earlier launches are done).
static QueueSet* stream_queues(mpcqp_ctx* ctx, hipStream_t st, int batch, int* err, int* cap) {
  *err = MPCQP_OK;
  QueueSet* qs = nullptr;
  for (auto& q : ctx->queues)
    if (q.stream == st) qs = &q;
  if (qs) qs->used = ++ctx->use_clock;
  if (qs && qs->cap >= batch) {
    *cap = qs->cap;
    return qs;
  }
  if (!qs && (int)ctx->queues.size() >= kMaxQueueSets) {
    QueueSet* lru = &ctx->queues[0];
    for (auto& q : ctx->queues)
      if (q.used < lru->used) lru = &q;
    // ev_done is recorded after every call that launched anything on the set, on its error
    // paths too; without one, wait for the whole device
    const hipError_t se = lru->ev_done ? hipEventSynchronize(lru->ev_done) : hipDeviceSynchronize();
    if (se != hipSuccess) {
      *err = set_err(ctx, MPCQP_ERR_HIP, "queue eviction: sync failed");
      return nullptr;
    }
    // every launch that used the set is done: its queues are back at rest (each kernel
    // resets its header) -- the new stream reuses them as they are
    lru->stream = st;
    lru->used = ++ctx->use_clock;
    qs = lru;
  }
  if (!qs) {
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
      *err = set_err(ctx, MPCQP_ERR_HIP, "queue event creation failed");
      return nullptr;
    }
    ctx->queues.push_back(QueueSet{st, 0, nullptr, ++ctx->use_clock, nullptr, nullptr, nullptr, ev});
    qs = &ctx->queues.back();
  }
  if (qs->buf) {
    if (hipStreamSynchronize(st) != hipSuccess) {
      *err = set_err(ctx, MPCQP_ERR_HIP, "queue growth: stream sync failed");
      return nullptr;
    }
    (void)hipFree(qs->buf);
    qs->buf = nullptr;
    qs->cap = 0;
  }
  // three queues of 4 + batch ints, then the dispatch order (mpcqp_order_kernel) of batch ints
  const size_t bytes = sizeof(int) * (3 * (4 + (size_t)batch) + (size_t)batch);
  if (hipMalloc(&qs->buf, bytes) != hipSuccess) {
    qs->buf = nullptr;
    *err = set_err(ctx, MPCQP_ERR_ALLOC, "queue allocation failed");
    return nullptr;
  }
  if (hipMemsetAsync(qs->buf, 0, bytes, st) != hipSuccess) {
    *err = set_err(ctx, MPCQP_ERR_HIP, "queue init failed");
    return nullptr;
  }
  qs->cap = batch;
  *cap = batch;
  return qs;
}

// The side stream and fork / join events of a queue set (created on first use).
static bool side_stream(QueueSet* qs) {
  if (!qs->side && hipStreamCreateWithFlags(&qs->side, hipStreamNonBlocking) != hipSuccess) {
    qs->side = nullptr;
    return false;
  }
  if (!qs->ev_fork && hipEventCreateWithFlags(&qs->ev_fork, hipEventDisableTiming) != hipSuccess) {
    qs->ev_fork = nullptr;
    return false;
  }
  if (!qs->ev_join && hipEventCreateWithFlags(&qs->ev_join, hipEventDisableTiming) != hipSuccess) {
    qs->ev_join = nullptr;
    return false;
  }
  return true;
}

extern "C" {

int32_t mpcqp_abi_version(void) { return MPCQP_ABI_VERSION; }

void mpcqp_default_params(mpcqp_params* p, int32_t horizon) {
  if (!p) return;
  static const double q[13] = {5., 5., 10., 10., 10., 50., 0.01, 0.01, 0.2, 0.2, 0.2, 0.2, 0.};
  memset(p, 0, sizeof(*p));
  p->horizon = horizon;
  p->max_iter = 0;
  p->dt = 0.05;
  for (int i = 0; i < 13; ++i) p->q_diag[i] = q[i];
  for (int i = 0; i < 12; ++i) p->r_diag[i] = 1e-5;
}

int mpcqp_create(const mpcqp_params* p, int32_t device, mpcqp_ctx** out) {
  if (!p || !out) return MPCQP_ERR_ARG;
  *out = nullptr;
  if (p->horizon < 1 || p->horizon > kMaxN) return MPCQP_ERR_ARG;
  if (!(p->dt > 0.0)) return MPCQP_ERR_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return MPCQP_ERR_HIP;
  mpcqp_ctx* ctx = new (std::nothrow) mpcqp_ctx();
  if (!ctx) return MPCQP_ERR_ALLOC;
  ctx->params = *p;
  ctx->device = device;
  for (int i = 0; i < 13 * 13; ++i) ctx->q_full[i] = (i % 14 == 0) ? p->q_diag[i / 14] : 0.0;
  for (int i = 0; i < 12 * 12; ++i) ctx->r_full[i] = (i % 13 == 0) ? p->r_diag[i / 13] : 0.0;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->ncu = prop.multiProcessorCount;
  if (ctx->ncu <= 0) ctx->ncu = 256;
  {
    DeviceScope dev(device);
    if (!dev.ok || hipMalloc(&ctx->prio_tab, sizeof(unsigned long long) * kPrioTab) != hipSuccess) {
      delete ctx;
      return MPCQP_ERR_ALLOC;
    }
    // cleared and waited for, so a first launch on any stream finds it cleared
    if (hipMemsetAsync(ctx->prio_tab, 0, sizeof(unsigned long long) * kPrioTab, nullptr) != hipSuccess ||
        hipStreamSynchronize(nullptr) != hipSuccess) {
      (void)hipFree(ctx->prio_tab);
      delete ctx;
      return MPCQP_ERR_HIP;
    }
  }
  *out = ctx;
  return MPCQP_OK;
}

int mpcqp_set_warm_start(mpcqp_ctx* ctx, void* memory, int32_t capacity) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (capacity < 0 || (capacity > 0 && !memory))
    return set_err(ctx, MPCQP_ERR_ARG, "warm start: capacity < 0, or no memory for capacity > 0");
  ctx->warm = capacity > 0 ? static_cast<unsigned char*>(memory) : nullptr;
  ctx->warm_cap = capacity > 0 ? capacity : 0;
  return MPCQP_OK;
}

int mpcqp_set_order(mpcqp_ctx* ctx, int32_t mode) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (mode != 0 && mode != 1) return set_err(ctx, MPCQP_ERR_ARG, "order: mode must be 0 or 1");
  ctx->order = mode;
  return MPCQP_OK;
}

int mpcqp_set_stance_hint(mpcqp_ctx* ctx, int32_t max_stance) {
  return mpcqp_set_stance_range(ctx, 0, max_stance);
}

int mpcqp_set_stance_range(mpcqp_ctx* ctx, int32_t min_stance, int32_t max_stance) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (min_stance < 0 || max_stance < 0 || (max_stance > 0 && min_stance > max_stance))
    return set_err(ctx, MPCQP_ERR_ARG, "stance range: min > max or negative");
  // a schedule has at most 4 N stance foot-steps: a larger minimum would route the whole
  // batch past every class mpcqp_solve launches (and leave the outputs unwritten)
  if (min_stance > 4 * ctx->params.horizon)
    return set_err(ctx, MPCQP_ERR_ARG, "stance range: min_stance > 4 * horizon");
  ctx->stance_min = min_stance;
  ctx->stance_hint = max_stance;
  return MPCQP_OK;
}

// What every kernel takes from the context: the horizon, dt and the weights.  The kernels that
// evaluate a given U (mpcqp_predict, mpcqp_certify) take nothing else; enqueue_solve adds what
// is the solve's.
static KParams eval_params(const mpcqp_ctx* ctx) {
  KParams kp;
  kp.N = ctx->params.horizon;
  kp.max_iter = 0;
  kp.dt = ctx->params.dt;
  for (int i = 0; i < NX; ++i) kp.q[i] = ctx->params.q_diag[i];
  for (int i = 0; i < NU; ++i) kp.r[i] = ctx->params.r_diag[i];
  kp.wfull = ctx->wdev;
  kp.warm = nullptr;
  kp.warm_cap = 0;
  return kp;
}

// The interior-point kernel of a plan: [ipm_size][ipm_full][latency, throughput, XR].  Only
// N <= 16 has a throughput layout and only full weights an XR one (solve_plan plans no other).
using IpmKernel = decltype(&mpcqp_kernel_ipm<false, 16>);
static const IpmKernel kIpmKernels[3][2][3] = {
    {{mpcqp_kernel_ipm<false, 16>, mpcqp_kernel_ipm<false, 16, true>, nullptr},
     {mpcqp_kernel_ipm<true, 16>, mpcqp_kernel_ipm<true, 16, true>, mpcqp_kernel_ipm<true, 16, false, true>}},
    {{mpcqp_kernel_ipm<false, kDenseN>, nullptr, nullptr},
     {mpcqp_kernel_ipm<true, kDenseN>, nullptr, mpcqp_kernel_ipm<true, kDenseN, false, true>}},
    {{mpcqp_kernel_ipm<false, kMaxN>, nullptr, nullptr},
     {mpcqp_kernel_ipm<true, kMaxN>, nullptr, mpcqp_kernel_ipm<true, kMaxN, false, true>}}};

// Everything mpcqp_solve enqueues on `stream`, for mpcqp_solve and mpcqp_step: the arguments are
// checked (batch > 0, no NULL required pointer) and the context's device is current.
static int enqueue_solve(mpcqp_ctx* ctx, int32_t batch, const float* x0, const float* xref, const float* contact,
                         const float* feet, const float* robot, float* u0, float* U, int32_t* status,
                         int32_t* iters, void* stream) {
  KParams kp = eval_params(ctx);
  kp.max_iter = ctx->params.max_iter;
  kp.warm = ctx->warm;
  kp.warm_cap = ctx->warm_cap;
  const bool full = ctx->wdev != nullptr;   // the dense classes' full-weight instantiations
  hipStream_t st = (hipStream_t)stream;
  // which classes launch, which one takes the batch, and the launches' schedule
  const SolvePlan plan = solve_plan(
      SolveInput{kp.N, ctx->stance_min, ctx->stance_hint, ctx->order, ctx->ncu, batch, full, ctx->xr});
  QueueSet* qs = nullptr;
  int cap = 0;
  if (plan.queues) {
    int qerr = MPCQP_OK;
    qs = stream_queues(ctx, st, batch, &qerr, &cap);
    if (!qs) return qerr;
  }
  // the set's layout: the queues into classes 96, 128 and the interior point (4 + cap ints each),
  // then the order; a class that does not launch has no queue
  const size_t qstride = 4 + (size_t)cap;
  auto queue_into = [&](int cls) -> int* { return plan.launch[cls] ? qs->buf + (cls - 1) * qstride : nullptr; };
  int *const q1 = queue_into(kClass96), *const q2 = queue_into(kClass128), *const q3 = queue_into(kClassIpm);
  int* const perm = plan.order ? qs->buf + 3 * qstride : nullptr;
  // the first class takes the batch directly: robot = workgroup, or perm's
  auto direct_B = [&](int cls) -> int { return plan.first == cls ? batch : 0; };
  const size_t sstride = (size_t)ipm_slot_doubles(kp.N);   // doubles per slot
  if (plan.launch[kClassIpm] && !ctx->sscratch) {   // the interior-point class's global slots (first use)
    const int slots = 32 * ((kIpmPerCU * ctx->ncu + 31) / 32);
    const size_t sbytes = sizeof(double) * sstride * (size_t)slots;
    if (hipMalloc(&ctx->sscratch, sbytes + slots / 8) != hipSuccess) {
      ctx->sscratch = nullptr;
      return set_err(ctx, MPCQP_ERR_ALLOC, "interior-point scratch allocation failed");
    }
    // the slot bitmap after the slots: all free (every solve releases its slot); cleared on this
    // stream and waited for, so a launch on any stream of the context finds it cleared
    if (hipMemsetAsync((char*)ctx->sscratch + sbytes, 0, slots / 8, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
      (void)hipFree(ctx->sscratch);
      ctx->sscratch = nullptr;
      return set_err(ctx, MPCQP_ERR_HIP, "interior-point scratch init failed");
    }
    ctx->sslots = slots;
  }
  // the interior-point class (one wave per robot, latency-bound) on a side stream as soon
  // as the first class has routed its robots, beside classes 96 / 128 instead of behind
  // them; the caller's stream waits for it at the end of the call
  const bool fork = plan.fork && side_stream(qs);
  // one launch of `grid` workgroups, and its error under the class's name
  auto launch = [&](const char* what, auto kern, int grid, int threads, unsigned lds, hipStream_t s,
                    auto... args) -> int {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, s, args...);
    return launched(ctx, what);
  };
  bool ipm_done = false;
  auto launch_ipm = [&](hipStream_t s) -> int {
    // one workgroup per robot of the batch (the queued ones beyond the count exit at once)
    unsigned* sbits = (unsigned*)(ctx->sscratch + sstride * ctx->sslots);
    ipm_done = true;
    return launch("launch (ipm)", kIpmKernels[plan.ipm_size][plan.ipm_full][plan.ipm_xr ? 2 : plan.ipm_thru], batch,
                  LANES, 0, s, kp, x0, xref, contact, feet, robot, u0, U, (int*)status, (int*)iters, q3,
                  direct_B(kClassIpm), ctx->sscratch, sbits, ctx->sslots / 32);
  };
  auto fork_ipm = [&]() -> int {
    if (!fork || ipm_done) return MPCQP_OK;
    if (hipEventRecord(qs->ev_fork, st) != hipSuccess || hipStreamWaitEvent(qs->side, qs->ev_fork, 0) != hipSuccess)
      return set_err(ctx, MPCQP_ERR_HIP, "interior-point fork failed");
    if (const int le = launch_ipm(qs->side)) return le;
    if (hipEventRecord(qs->ev_join, qs->side) != hipSuccess) return set_err(ctx, MPCQP_ERR_HIP, "join record failed");
    return MPCQP_OK;
  };
  // an error after a launch still marks the queue set's last use: eviction waits on ev_done
  auto failed = [&](int code) -> int {
    if (fork && ipm_done) (void)hipStreamWaitEvent(st, qs->ev_join, 0);   // the side stream's launch too
    if (qs) (void)hipEventRecord(qs->ev_done, st);
    return code;
  };
  int rc = MPCQP_OK;
  if (plan.order && (rc = launch("launch (order)", mpcqp_order_kernel, plan.order_segs, 1024, 0, st, (int)batch, kp.N,
                                 x0, xref, perm, plan.order_mode)) != MPCQP_OK)
    return failed(rc);
  if (plan.launch[kClass64]) {
    if (plan.prio && ++ctx->prio_epoch == 0) {   // the epoch wrapped: earlier entries would win for ever
      if (hipMemsetAsync(ctx->prio_tab, 0, sizeof(unsigned long long) * kPrioTab, st) != hipSuccess)
        return failed(set_err(ctx, MPCQP_ERR_HIP, "priority table reset failed"));
      ctx->prio_epoch = 1;
    }
    rc = launch("launch",
                plan.prio ? (full ? mpcqp_kernel_64<true, true> : mpcqp_kernel_64<false, true>)
                          : (full ? mpcqp_kernel_64<true> : mpcqp_kernel_64<false>),
                batch, Cfg<64>::NT, kDiagLds, st, kp, (int)batch, x0, xref, contact, feet, robot, u0, U, (int*)status,
                (int*)iters, q1, q2, q3, perm, plan.prio ? ctx->prio_tab : (unsigned long long*)nullptr,
                ctx->prio_epoch);
    if (rc != MPCQP_OK || (rc = fork_ipm()) != MPCQP_OK) return failed(rc);
  }
  if (plan.launch[kClass96]) {
    rc = launch("launch (96)", full ? mpcqp_kernel_96<true> : mpcqp_kernel_96<false>, batch, Cfg<96>::NT, 0, st, kp,
                x0, xref, contact, feet, robot, u0, U, (int*)status, (int*)iters, q1, q2, q3, direct_B(kClass96),
                plan.first == kClass96 ? perm : nullptr);
    if (rc != MPCQP_OK || (rc = fork_ipm()) != MPCQP_OK) return failed(rc);
  }
  if (plan.launch[kClass128]) {
    rc = launch("launch (128)", full ? mpcqp_kernel_128<true> : mpcqp_kernel_128<false>, batch, Cfg<128>::NT, 0, st,
                kp, x0, xref, contact, feet, robot, u0, U, (int*)status, (int*)iters, q2, q3, direct_B(kClass128),
                plan.first == kClass128 ? perm : nullptr);
    if (rc != MPCQP_OK || (rc = fork_ipm()) != MPCQP_OK) return failed(rc);
  }
  if (plan.launch[kClassIpm] && !ipm_done) {   // the interior-point class takes the batch directly (or no side stream)
    if ((rc = launch_ipm(st)) != MPCQP_OK) return failed(rc);
  } else if (fork && hipStreamWaitEvent(st, qs->ev_join, 0) != hipSuccess) {
    return failed(set_err(ctx, MPCQP_ERR_HIP, "interior-point join failed"));
  }
  if (qs && hipEventRecord(qs->ev_done, st) != hipSuccess) return set_err(ctx, MPCQP_ERR_HIP, "queue event record failed");
  return MPCQP_OK;
}

int mpcqp_solve(mpcqp_ctx* ctx, int32_t batch, const float* x0, const float* xref, const float* contact,
                const float* feet, const float* robot, float* u0, float* U, int32_t* status, int32_t* iters,
                void* stream) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (batch < 0) return set_err(ctx, MPCQP_ERR_ARG, "batch < 0");
  if (batch == 0) return MPCQP_OK;
  if (!x0 || !xref || !contact || !feet || !robot || !u0)
    return set_err(ctx, MPCQP_ERR_ARG, "null input/output pointer");
  DeviceScope dev(ctx->device);
  if (!dev.ok) return set_err(ctx, MPCQP_ERR_HIP, "hipSetDevice failed");
  return enqueue_solve(ctx, batch, x0, xref, contact, feet, robot, u0, U, status, iters, stream);
}

int mpcqp_set_weights(mpcqp_ctx* ctx, const double* Q, const double* R) {
  if (!ctx) return MPCQP_ERR_ARG;
  double q[NX * NX], r[NU * NU];
  memcpy(q, Q ? Q : ctx->q_full, sizeof(q));   // NULL keeps the current matrix
  memcpy(r, R ? R : ctx->r_full, sizeof(r));
  // symmetric and finite (the reference's kron(I_N, Q) enters H = 2 Su^T Qbar Su; an
  // asymmetric Q would make H asymmetric, which no QP solver of the reference accepts)
  double qmax = 0.0, rmax = 0.0;
  bool finite = true;   // per entry: fmax drops a NaN operand
  for (int i = 0; i < NX * NX; ++i) {
    finite = finite && std::isfinite(q[i]);
    qmax = fmax(qmax, fabs(q[i]));
  }
  for (int i = 0; i < NU * NU; ++i) {
    finite = finite && std::isfinite(r[i]);
    rmax = fmax(rmax, fabs(r[i]));
  }
  if (!finite) return set_err(ctx, MPCQP_ERR_ARG, "weights: non-finite entry");
  bool diag = true, cross = false;
  for (int i = 0; i < NX; ++i)
    for (int j = 0; j < NX; ++j) {
      if (fabs(q[i * NX + j] - q[j * NX + i]) > 1e-12 * qmax) return set_err(ctx, MPCQP_ERR_ARG, "weights: Q not symmetric");
      if (i != j && q[i * NX + j] != 0.0) diag = false;
    }
  for (int i = 0; i < NU; ++i)
    for (int j = 0; j < NU; ++j) {
      if (fabs(r[i * NU + j] - r[j * NU + i]) > 1e-12 * rmax) return set_err(ctx, MPCQP_ERR_ARG, "weights: R not symmetric");
      if (i != j && r[i * NU + j] != 0.0) diag = false;
      if (i / 3 != j / 3 && r[i * NU + j] != 0.0) cross = true;
    }
  DeviceScope dev(ctx->device);
  if (!dev.ok) return set_err(ctx, MPCQP_ERR_HIP, "hipSetDevice failed");
  // Device work first, into a fresh buffer; the context changes only once it all succeeded
  // (a failed allocation or upload leaves the previous weights in force).
  double* nb = nullptr;
  if (!diag) {
    if (hipMalloc(&nb, sizeof(double) * (NX * NX + NU * NU)) != hipSuccess)
      return set_err(ctx, MPCQP_ERR_ALLOC, "weights: allocation failed");
    double host[NX * NX + NU * NU];
    memcpy(host, q, sizeof(q));
    memcpy(host + NX * NX, r, sizeof(r));
    if (hipMemcpy(nb, host, sizeof(host), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(nb);
      return set_err(ctx, MPCQP_ERR_HIP, "weights: upload failed");
    }
  }
  // launches on any stream (non-blocking ones included) may still read the previous
  // buffer: it is retired, not freed (2.5 KB each), and released at mpcqp_destroy -- or,
  // past kMaxRetired changes, all at once after a device synchronisation
  if (ctx->wdev) {
    if (ctx->retired.size() >= kMaxRetired) {
      if (hipDeviceSynchronize() != hipSuccess) {
        if (nb) (void)hipFree(nb);
        return set_err(ctx, MPCQP_ERR_HIP, "weights: device sync failed");
      }
      for (double* o : ctx->retired) (void)hipFree(o);
      ctx->retired.clear();
    }
    ctx->retired.push_back(ctx->wdev);
  }
  ctx->wdev = nb;   // nullptr: the diagonal fast path (the weights live in the kernel arguments)
  ctx->xr = cross;
  memcpy(ctx->q_full, q, sizeof(q));
  memcpy(ctx->r_full, r, sizeof(r));
  for (int i = 0; i < NX; ++i) ctx->params.q_diag[i] = q[i * (NX + 1)];
  for (int i = 0; i < NU; ++i) ctx->params.r_diag[i] = r[i * (NU + 1)];
  return MPCQP_OK;
}

int mpcqp_set_planner(mpcqp_ctx* ctx, double dt_control, double gravity, double max_pos_error) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (!all_finite({dt_control, gravity, max_pos_error}))
    return set_err(ctx, MPCQP_ERR_ARG, "non-finite planner constant");
  if (dt_control < 0.0 || max_pos_error < 0.0)
    return set_err(ctx, MPCQP_ERR_ARG, "negative planner constant (dt_control, max_pos_error)");
  ctx->dt_control = dt_control;
  ctx->gravity = gravity;
  ctx->max_pos_error = max_pos_error;
  return MPCQP_OK;
}

static int launch_plan(mpcqp_ctx* ctx, int32_t batch, int32_t flags, int root_layout, const float* quat,
                       const float* pos, const float* omega, const float* vel, const float* rot,
                       const double* vel_body_des, const double* yaw_rate_des, const int32_t* gait,
                       const int32_t* iteration, const float* height_des, double* plan_state, float* x0,
                       float* xref, float* contact, void* stream) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (batch < 0) return set_err(ctx, MPCQP_ERR_ARG, "batch < 0");
  if (batch == 0) return MPCQP_OK;
  if (!quat || (!root_layout && (!pos || !omega || !vel)) || !vel_body_des || !yaw_rate_des || !plan_state ||
      !x0)
    return set_err(ctx, MPCQP_ERR_ARG, "null planner input/output pointer");
  if (flags & ~(MPCQP_PLAN_REFERENCE | MPCQP_PLAN_NO_INTEGRATE))
    return set_err(ctx, MPCQP_ERR_ARG, "unknown planner flags");
  const int mpc_tick = (flags & MPCQP_PLAN_REFERENCE) ? 1 : 0;
  if (mpc_tick && (!height_des || !xref))
    return set_err(ctx, MPCQP_ERR_ARG, "null height/xref pointer on an MPC tick");
  if (mpc_tick && gait && (!iteration || !contact))
    return set_err(ctx, MPCQP_ERR_ARG, "gait given without iteration/contact");
  DeviceScope dev(ctx->device);
  if (!dev.ok) return set_err(ctx, MPCQP_ERR_HIP, "hipSetDevice failed");
  PlanParams pp;
  pp.N = ctx->params.horizon;
  pp.mpc_tick = mpc_tick;
  pp.root_layout = root_layout;
  pp.integrate = (flags & MPCQP_PLAN_NO_INTEGRATE) ? 0 : 1;
  pp.dt = ctx->params.dt;
  pp.dt_control = ctx->dt_control;
  pp.gravity = ctx->gravity;
  pp.max_pos_error = ctx->max_pos_error;
  hipLaunchKernelGGL(mpcqp_plan_kernel, dim3((batch + kPlanRobots - 1) / kPlanRobots), dim3(kPlanThreads), 0,
                     (hipStream_t)stream, pp, (int)batch, quat, pos, omega, vel, rot, vel_body_des, yaw_rate_des,
                     gait, iteration, height_des, plan_state, x0, xref, contact);
  return launched(ctx, "plan launch");
}

int mpcqp_plan(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* quat, const float* pos,
               const float* omega, const float* vel, const float* rot, const double* vel_body_des,
               const double* yaw_rate_des, const int32_t* gait, const int32_t* iteration,
               const float* height_des, double* plan_state, float* x0, float* xref, float* contact,
               void* stream) {
  return launch_plan(ctx, batch, flags, 0, quat, pos, omega, vel, rot, vel_body_des, yaw_rate_des, gait,
                     iteration, height_des, plan_state, x0, xref, contact, stream);
}

int mpcqp_plan_root_states(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* root_states,
                           const double* vel_body_des, const double* yaw_rate_des, const int32_t* gait,
                           const int32_t* iteration, const float* height_des, double* plan_state, float* x0,
                           float* xref, float* contact, void* stream) {
  return launch_plan(ctx, batch, flags, 1, root_states, nullptr, nullptr, nullptr, nullptr, vel_body_des,
                     yaw_rate_des, gait, iteration, height_des, plan_state, x0, xref, contact, stream);
}

int mpcqp_stance_torques(mpcqp_ctx* ctx, int32_t batch, const float* jac, const float* contact,
                         int32_t contact_stride, const float* u0, float* tau, void* stream) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (batch < 0 || contact_stride < 4) return set_err(ctx, MPCQP_ERR_ARG, "batch < 0 or contact_stride < 4");
  if (batch == 0) return MPCQP_OK;
  if (!jac || !contact || !u0 || !tau) return set_err(ctx, MPCQP_ERR_ARG, "null torque pointer");
  DeviceScope dev(ctx->device);
  if (!dev.ok) return set_err(ctx, MPCQP_ERR_HIP, "hipSetDevice failed");
  const int threads = (int)batch * 12;
  hipLaunchKernelGGL(mpcqp_stance_torque_kernel, dim3((threads + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     (int)batch, jac, contact, (int)contact_stride, u0, tau);
  return launched(ctx, "torque launch");
}

int mpcqp_set_swing(mpcqp_ctx* ctx, double swing_height, const double* Kp, const double* Kd, double touchdown_z,
                    double vel_gain) {
  if (!ctx) return MPCQP_ERR_ARG;
  bool finite = all_finite({swing_height, touchdown_z, vel_gain});
  for (int i = 0; i < 9 && finite; ++i)
    finite = (!Kp || std::isfinite(Kp[i])) && (!Kd || std::isfinite(Kd[i]));
  if (!finite) return set_err(ctx, MPCQP_ERR_ARG, "non-finite swing constant");
  ctx->swing_height = swing_height;
  ctx->touchdown_z = touchdown_z;
  ctx->vel_gain = vel_gain;
  if (Kp) memcpy(ctx->kp_swing, Kp, sizeof(ctx->kp_swing));
  if (Kd) memcpy(ctx->kd_swing, Kd, sizeof(ctx->kd_swing));
  return MPCQP_OK;
}

static int launch_leg_torques(mpcqp_ctx* ctx, int32_t batch, int32_t flags, int root_layout, const int32_t* tick,
                              int32_t iterations_between_mpc, const float* quat, const float* pos, const float* vel,
                              const float* rot, const double* vel_body_des, const double* yaw_rate_des,
                              const int32_t* gait, const float* thighs, const float* pos_feet,
                              const float* foot_pos_base, const float* foot_vel_base, const float* jac,
                              const float* u0, double* swing_mem, float* tau, float* swing_state, float* pos_target,
                              float* vel_target, void* stream) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (batch < 0) return set_err(ctx, MPCQP_ERR_ARG, "batch < 0");
  if (flags != 0) return set_err(ctx, MPCQP_ERR_ARG, "unknown leg-torque flags");
  if (iterations_between_mpc < 1) return set_err(ctx, MPCQP_ERR_ARG, "iterations_between_mpc < 1");
  if (batch == 0) return MPCQP_OK;
  if (!tick || !quat || (!root_layout && (!pos || !vel)) || !vel_body_des || !yaw_rate_des || !gait || !thighs ||
      !pos_feet || !foot_pos_base || !foot_vel_base || !jac || !u0 || !swing_mem || !tau)
    return set_err(ctx, MPCQP_ERR_ARG, "null leg-torque input/output pointer");
  if (int rc = aligned16(ctx, swing_mem, "swing_mem")) return rc;
  DeviceScope dev(ctx->device);
  if (!dev.ok) return set_err(ctx, MPCQP_ERR_HIP, "hipSetDevice failed");
  const SwingParams sp = swing_params(ctx, iterations_between_mpc, root_layout);
  hipLaunchKernelGGL(mpcqp_leg_torque_kernel, dim3((batch + kSwingRobots - 1) / kSwingRobots), dim3(kSwingThreads),
                     0, (hipStream_t)stream, sp, (int)batch, tick, quat, pos, vel, rot, vel_body_des, yaw_rate_des,
                     gait, thighs, pos_feet, foot_pos_base, foot_vel_base, jac, u0, swing_mem, tau, swing_state,
                     pos_target, vel_target);
  return launched(ctx, "leg-torque launch");
}

int mpcqp_leg_torques(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const int32_t* tick,
                      int32_t iterations_between_mpc, const float* quat, const float* pos, const float* vel,
                      const float* rot, const double* vel_body_des, const double* yaw_rate_des, const int32_t* gait,
                      const float* thighs, const float* pos_feet, const float* foot_pos_base,
                      const float* foot_vel_base, const float* jac, const float* u0, double* swing_mem, float* tau,
                      float* swing_state, float* pos_target, float* vel_target, void* stream) {
  return launch_leg_torques(ctx, batch, flags, 0, tick, iterations_between_mpc, quat, pos, vel, rot, vel_body_des,
                            yaw_rate_des, gait, thighs, pos_feet, foot_pos_base, foot_vel_base, jac, u0, swing_mem,
                            tau, swing_state, pos_target, vel_target, stream);
}

int mpcqp_leg_torques_root_states(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const int32_t* tick,
                                  int32_t iterations_between_mpc, const float* root_states,
                                  const double* vel_body_des, const double* yaw_rate_des, const int32_t* gait,
                                  const float* thighs, const float* pos_feet, const float* foot_pos_base,
                                  const float* foot_vel_base, const float* jac, const float* u0, double* swing_mem,
                                  float* tau, float* swing_state, float* pos_target, float* vel_target,
                                  void* stream) {
  return launch_leg_torques(ctx, batch, flags, 1, tick, iterations_between_mpc, root_states, nullptr, nullptr,
                            nullptr, vel_body_des, yaw_rate_des, gait, thighs, pos_feet, foot_pos_base,
                            foot_vel_base, jac, u0, swing_mem, tau, swing_state, pos_target, vel_target, stream);
}

static int launch_kinematics(mpcqp_ctx* ctx, int32_t batch, int32_t flags, int root_layout, const float* quat,
                             const float* pos, const float* vel, const float* omega, const float* rot,
                             const float* q, const float* qdot, const double* geom, float* feet, float* thighs,
                             float* pos_feet, float* foot_pos_base, float* foot_vel_base, float* jac,
                             void* stream) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (batch < 0) return set_err(ctx, MPCQP_ERR_ARG, "batch < 0");
  if (flags != 0) return set_err(ctx, MPCQP_ERR_ARG, "unknown kinematics flags");
  if (batch == 0) return MPCQP_OK;
  if (!quat || !q || !geom || (!root_layout && (!pos || !vel || !omega || !qdot)))
    return set_err(ctx, MPCQP_ERR_ARG, "null kinematics input pointer");
  DeviceScope dev(ctx->device);
  if (!dev.ok) return set_err(ctx, MPCQP_ERR_HIP, "hipSetDevice failed");
  KinParams kp;
  kp.root_layout = root_layout;
  hipLaunchKernelGGL(mpcqp_kinematics_kernel, dim3((batch + kKinRobots - 1) / kKinRobots), dim3(kKinThreads), 0,
                     (hipStream_t)stream, kp, (int)batch, quat, pos, vel, omega, rot, q, qdot, geom, feet, thighs,
                     pos_feet, foot_pos_base, foot_vel_base, jac);
  return launched(ctx, "kinematics launch");
}

int mpcqp_kinematics(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* quat, const float* pos,
                     const float* vel, const float* omega, const float* rot, const float* q, const float* qdot,
                     const double* geom, float* feet, float* thighs, float* pos_feet, float* foot_pos_base,
                     float* foot_vel_base, float* jac, void* stream) {
  return launch_kinematics(ctx, batch, flags, 0, quat, pos, vel, omega, rot, q, qdot, geom, feet, thighs, pos_feet,
                           foot_pos_base, foot_vel_base, jac, stream);
}

int mpcqp_kinematics_root_states(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* root_states,
                                 const float* dof_states, const double* geom, float* feet, float* thighs,
                                 float* pos_feet, float* foot_pos_base, float* foot_vel_base, float* jac,
                                 void* stream) {
  return launch_kinematics(ctx, batch, flags, 1, root_states, nullptr, nullptr, nullptr, nullptr, dof_states,
                           nullptr, geom, feet, thighs, pos_feet, foot_pos_base, foot_vel_base, jac, stream);
}

// ---- the control tick in one call (mpcqp_step.h; isaacgym_a1.py:117-162): one STEP_WHOLE
// launch, or on an MPC tick STEP_FRONT, what mpcqp_solve enqueues and STEP_BACK
int mpcqp_step(mpcqp_ctx* ctx, int32_t batch, int32_t flags, int32_t iter_counter, const int32_t* tick,
               int32_t iterations_between_mpc, const float* root_states, const float* dof_states,
               const double* geom, const double* vel_body_des, const double* yaw_rate_des, const int32_t* gait,
               const float* height_des, const float* robot, double* plan_state, double* swing_mem, float* x0,
               float* xref, float* contact, float* feet, float* u0, float* tau, int32_t* status, int32_t* iters,
               float* thighs, float* pos_feet, float* foot_pos_base, float* foot_vel_base, float* jac,
               float* swing_state, float* pos_target, float* vel_target, void* stream) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (batch < 0) return set_err(ctx, MPCQP_ERR_ARG, "batch < 0");
  if (flags & ~MPCQP_STEP_MPC) return set_err(ctx, MPCQP_ERR_ARG, "unknown step flags");
  if (iterations_between_mpc < 1) return set_err(ctx, MPCQP_ERR_ARG, "iterations_between_mpc < 1");
  if (batch == 0) return MPCQP_OK;
  if (!root_states || !dof_states || !geom || !vel_body_des || !yaw_rate_des || !gait || !plan_state ||
      !swing_mem || !x0 || !u0 || !tau)
    return set_err(ctx, MPCQP_ERR_ARG, "null step input/output pointer");
  const bool mpc = (flags & MPCQP_STEP_MPC) != 0;
  if (mpc && (!height_des || !robot || !xref || !contact || !feet))
    return set_err(ctx, MPCQP_ERR_ARG, "null height/robot/xref/contact/feet pointer on an MPC tick");
  if (int rc = aligned16(ctx, swing_mem, "swing_mem")) return rc;
  DeviceScope dev(ctx->device);
  if (!dev.ok) return set_err(ctx, MPCQP_ERR_HIP, "hipSetDevice failed");
  StepParams sp;
  sp.N = ctx->params.horizon;
  sp.dt = ctx->params.dt;
  sp.max_pos_error = ctx->max_pos_error;
  sp.sw = swing_params(ctx, iterations_between_mpc, 1);
  const dim3 grid((batch + kStepRobots - 1) / kStepRobots), block(kStepThreads);
  hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto kern, const char* what) -> int {
    hipLaunchKernelGGL(kern, grid, block, 0, st, sp, (int)batch, (int)iter_counter, tick, root_states, dof_states,
                       geom, vel_body_des, yaw_rate_des, gait, height_des, plan_state, swing_mem, x0, xref, contact,
                       feet, (const float*)u0, tau, thighs, pos_feet, foot_pos_base, foot_vel_base, jac,
                       swing_state, pos_target, vel_target);
    return launched(ctx, what);
  };
  if (!mpc) return launch(mpcqp_step_kernel<STEP_WHOLE>, "step launch");
  int rc = launch(mpcqp_step_kernel<STEP_FRONT>, "step launch (front)");
  if (rc != MPCQP_OK) return rc;
  rc = enqueue_solve(ctx, batch, x0, xref, contact, feet, robot, u0, nullptr, status, iters, stream);
  if (rc != MPCQP_OK) return rc;
  return launch(mpcqp_step_kernel<STEP_BACK>, "step launch (back)");
}

// ---- the base-state estimator (mpcqp_estimator.h): the Kalman filter doc/state_estimation_kf.md
// derives (second stage) on the sensors scripts/mujoco_aliengo.py:101-118 collects; the reference
// raises NotImplementedError in its place (RobotData.update, state_estimation=True).  An invalid
// constant leaves the previous set in force.
int mpcqp_set_estimator(mpcqp_ctx* ctx, double dt, double gravity, double sigma_p, double sigma_v, double sigma_f,
                        double r_p, double r_v, double r_z, double suspicion, double p0, double contact_height) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (!all_finite({dt, gravity, sigma_p, sigma_v, sigma_f, r_p, r_v, r_z, suspicion, p0, contact_height}))
    return set_err(ctx, MPCQP_ERR_ARG, "non-finite estimator constant");
  if (!(dt > 0.0)) return set_err(ctx, MPCQP_ERR_ARG, "estimator: dt <= 0");
  if (!(r_p > 0.0) || !(r_v > 0.0) || !(r_z > 0.0) || !(p0 > 0.0))
    return set_err(ctx, MPCQP_ERR_ARG, "estimator: r_p, r_v, r_z and p0 must be > 0");
  if (sigma_p < 0.0 || sigma_v < 0.0 || sigma_f < 0.0 || suspicion < 0.0)
    return set_err(ctx, MPCQP_ERR_ARG, "estimator: a process rate or the suspicion factor is < 0");
  ctx->est = EstParams{0, dt, gravity, sigma_p, sigma_v, sigma_f, r_p, r_v, r_z, suspicion, p0, contact_height};
  return MPCQP_OK;
}

int mpcqp_estimate(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* quat, const float* gyro,
                   const float* accel, const float* q, const float* qdot, const float* trust, const double* geom,
                   double* est_state, float* root_states, float* feet_world, int32_t* status, void* stream) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (batch <= 0) return set_err(ctx, MPCQP_ERR_ARG, "estimate: batch <= 0");
  if (flags & ~MPCQP_EST_DOF_STATES) return set_err(ctx, MPCQP_ERR_ARG, "unknown estimator flags");
  const int dof_layout = (flags & MPCQP_EST_DOF_STATES) ? 1 : 0;
  if (!quat || !gyro || !accel || !q || (!dof_layout && !qdot) || !trust || !geom || !est_state)
    return set_err(ctx, MPCQP_ERR_ARG, "null estimator input/state pointer");
  if (int rc = aligned16(ctx, est_state, "est_state")) return rc;
  DeviceScope dev(ctx->device);
  if (!dev.ok) return set_err(ctx, MPCQP_ERR_HIP, "hipSetDevice failed");
  EstParams ep = ctx->est;
  ep.dof_layout = dof_layout;
  hipLaunchKernelGGL(mpcqp_estimate_kernel, dim3((batch + kEstRobots - 1) / kEstRobots), dim3(kEstThreads), 0,
                     (hipStream_t)stream, ep, (int)batch, quat, gyro, accel, q, qdot, trust, geom, est_state,
                     root_states, feet_world, status);
  return launched(ctx, "estimator launch");
}

// ---- the orientation filter and the contact trust (mpcqp_attitude.h): the first stage of
// doc/state_estimation_kf.md (section 2) and the stance-phase trust ramp, producing the `quat`
// and `trust` of mpcqp_estimate from the raw sensors scripts/mujoco_aliengo.py:101-118 collects.
// An invalid constant leaves the previous set in force.
int mpcqp_set_attitude(mpcqp_ctx* ctx, double dt, double gravity, double kappa_ref, double bias_gain,
                       double trust_window, double touch_threshold) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (!all_finite({dt, gravity, kappa_ref, bias_gain, trust_window, touch_threshold}))
    return set_err(ctx, MPCQP_ERR_ARG, "non-finite attitude constant");
  if (!(dt > 0.0) || !(gravity > 0.0)) return set_err(ctx, MPCQP_ERR_ARG, "attitude: dt and gravity must be > 0");
  if (kappa_ref < 0.0 || bias_gain < 0.0) return set_err(ctx, MPCQP_ERR_ARG, "attitude: kappa_ref or bias_gain is < 0");
  if (trust_window < 0.0 || trust_window > 0.5)
    return set_err(ctx, MPCQP_ERR_ARG, "attitude: trust_window outside [0, 0.5]");
  ctx->att = AttParams{dt, gravity, kappa_ref, bias_gain, trust_window, touch_threshold};
  return MPCQP_OK;
}

int mpcqp_attitude(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* gyro, const float* accel,
                   const int32_t* tick, int32_t iterations_between_mpc, const int32_t* gait, const float* touch,
                   double* att_state, float* quat, float* gyro_out, float* trust, int32_t* status, void* stream) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (flags != 0) return set_err(ctx, MPCQP_ERR_ARG, "unknown attitude flags");
  if (batch <= 0) return set_err(ctx, MPCQP_ERR_ARG, "attitude: batch <= 0");
  if (!gyro || !accel || !att_state) return set_err(ctx, MPCQP_ERR_ARG, "null attitude input/state pointer");
  if (int rc = aligned16(ctx, att_state, "att_state")) return rc;
  if (gait && !tick) return set_err(ctx, MPCQP_ERR_ARG, "attitude: gait given without tick");
  if (trust && !gait && !touch)
    return set_err(ctx, MPCQP_ERR_ARG, "attitude: trust wanted with neither gait and tick nor touch");
  if (gait && iterations_between_mpc < 1) return set_err(ctx, MPCQP_ERR_ARG, "attitude: iterations_between_mpc < 1");
  DeviceScope dev(ctx->device);
  if (!dev.ok) return set_err(ctx, MPCQP_ERR_HIP, "hipSetDevice failed");
  hipLaunchKernelGGL(mpcqp_attitude_kernel, dim3((batch + kAttThreads - 1) / kAttThreads), dim3(kAttThreads), 0,
                     (hipStream_t)stream, ctx->att, (int)batch, (int)iterations_between_mpc, gyro, accel, tick, gait,
                     touch, att_state, quat, gyro_out, trust, status);
  return launched(ctx, "attitude launch");
}

// ---- the terrain plane (mpcqp_terrain.h): RobotData.update_terrain_normal (robot_data.py:186-228)
// for every robot, producing the surface normal of the cone rows and the swing leg's ground plane.
// An invalid constant leaves the previous set in force.
int mpcqp_set_terrain(mpcqp_ctx* ctx, double contact_threshold, double flat_tol, double cos_max_tilt, double blend) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (!all_finite({contact_threshold, flat_tol, cos_max_tilt, blend}))
    return set_err(ctx, MPCQP_ERR_ARG, "non-finite terrain constant");
  if (flat_tol < 0.0 || !(flat_tol < 1.0)) return set_err(ctx, MPCQP_ERR_ARG, "terrain: flat_tol outside [0, 1)");
  if (!(cos_max_tilt > 0.0) || cos_max_tilt > 1.0)
    return set_err(ctx, MPCQP_ERR_ARG, "terrain: cos_max_tilt outside (0, 1]");
  if (!(blend > 0.0) || blend > 1.0) return set_err(ctx, MPCQP_ERR_ARG, "terrain: blend outside (0, 1]");
  ctx->ter = TerParams{contact_threshold, flat_tol, cos_max_tilt, blend, 0, 0.0};
  return MPCQP_OK;
}

int mpcqp_set_ground(mpcqp_ctx* ctx, const float* plane, int32_t capacity) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (capacity < 0 || (capacity > 0 && !plane))
    return set_err(ctx, MPCQP_ERR_ARG, "ground: capacity < 0, or no plane for capacity > 0");
  ctx->ground = capacity > 0 ? plane : nullptr;
  ctx->ground_cap = capacity > 0 ? capacity : 0;
  return MPCQP_OK;
}

int mpcqp_terrain(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* pos_feet, const float* contact,
                  const float* quat, double* terrain_state, float* robot, float* normal, float* plane,
                  float* normal_base, int32_t* status, void* stream) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (flags & ~(MPCQP_TERRAIN_SWING_STATE | MPCQP_TERRAIN_ROOT_STATES | MPCQP_TERRAIN_GROUND))
    return set_err(ctx, MPCQP_ERR_ARG, "unknown terrain flags");
  if (batch < 0) return set_err(ctx, MPCQP_ERR_ARG, "terrain: batch < 0");
  if (!pos_feet || !contact || !terrain_state)
    return set_err(ctx, MPCQP_ERR_ARG, "null terrain input/state pointer");
  if (int rc = aligned16(ctx, terrain_state, "terrain_state")) return rc;
  if (normal_base && !quat) return set_err(ctx, MPCQP_ERR_ARG, "terrain: normal_base wanted without quat");
  if (batch == 0) return MPCQP_OK;
  DeviceScope dev(ctx->device);
  if (!dev.ok) return set_err(ctx, MPCQP_ERR_HIP, "hipSetDevice failed");
  TerParams tp = ctx->ter;
  tp.flags = flags;
  tp.touchdown_z = ctx->touchdown_z;   // as mpcqp_set_swing left it: the swing leg of the next launch reads the same
  hipLaunchKernelGGL(mpcqp_terrain_kernel, dim3((batch + kTerThreads - 1) / kTerThreads), dim3(kTerThreads), 0,
                     (hipStream_t)stream, tp, (int)batch, pos_feet, contact, quat, terrain_state, robot, normal, plane,
                     normal_base, status);
  return launched(ctx, "terrain launch");
}

// One launch of a kernel that evaluates a given U, one wavefront per robot: mpcqp_predict_kernel
// or mpcqp_certify_kernel, instantiations `k` in the order <16, false>, <16, true>, <kMaxN, false>,
// <kMaxN, true>.  `what` names the call in the error texts; `out` is X or G.
using EvalKernel = void (*)(KParams, int, const float*, const float*, const float*, const float*, const float*,
                            const float*, float*, double*, int32_t*);
static int launch_eval(mpcqp_ctx* ctx, const char* what, const EvalKernel (&k)[4], int32_t batch, int32_t flags,
                       const float* x0, const float* xref, const float* contact, const float* feet,
                       const float* robot, const float* U, float* out, double* report, int32_t* status,
                       void* stream) {
  if (!ctx) return MPCQP_ERR_ARG;
  const std::string w(what);
  if (flags != 0) return set_err(ctx, MPCQP_ERR_ARG, "unknown " + w + " flags");
  if (batch < 0) return set_err(ctx, MPCQP_ERR_ARG, w + ": batch < 0");
  if (!x0 || !xref || !contact || !feet || !robot || !U) return set_err(ctx, MPCQP_ERR_ARG, "null " + w + " input pointer");
  if (batch == 0 || (!out && !report && !status)) return MPCQP_OK;
  DeviceScope dev(ctx->device);
  if (!dev.ok) return set_err(ctx, MPCQP_ERR_HIP, "hipSetDevice failed");
  const KParams kp = eval_params(ctx);
  // the instantiation whose LDS holds this horizon and these weights
  hipLaunchKernelGGL(k[2 * (kp.N > 16) + (kp.wfull != nullptr)], dim3(batch), dim3(LANES), 0, (hipStream_t)stream, kp,
                     (int)batch, x0, xref, contact, feet, robot, U, out, report, status);
  return launched(ctx, (w + " launch").c_str());
}

// The trajectory the QP believes a force sequence produces (com_traj = Sx x0 + Su U,
// mpc.py:293-294), its cost, cone margin and swing residual (mpcqp_predict.h).
int mpcqp_predict(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* x0, const float* xref,
                  const float* contact, const float* feet, const float* robot, const float* U, float* X,
                  double* report, int32_t* status, void* stream) {
  static const EvalKernel k[4] = {mpcqp_predict_kernel<16, false>, mpcqp_predict_kernel<16, true>,
                                  mpcqp_predict_kernel<kMaxN, false>, mpcqp_predict_kernel<kMaxN, true>};
  return launch_eval(ctx, "predict", k, batch, flags, x0, xref, contact, feet, robot, U, X, report, status, stream);
}

// The gradient of the QP's objective at a force sequence, the objective and the duality gap the
// friction pyramids give in closed form (mpcqp_certify.h).
int mpcqp_certify(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* x0, const float* xref,
                  const float* contact, const float* feet, const float* robot, const float* U, float* G,
                  double* report, int32_t* status, void* stream) {
  static const EvalKernel k[4] = {mpcqp_certify_kernel<16, false>, mpcqp_certify_kernel<16, true>,
                                  mpcqp_certify_kernel<kMaxN, false>, mpcqp_certify_kernel<kMaxN, true>};
  return launch_eval(ctx, "certify", k, batch, flags, x0, xref, contact, feet, robot, U, G, report, status, stream);
}

// ---- the rigid-body plant (mpcqp_plant.h): the stage the reference's scripts hand to a simulator
// (gym.simulate, sim.step()), as a single rigid body on massless legs.  An invalid constant leaves
// the previous set in force.
int mpcqp_set_plant(mpcqp_ctx* ctx, double foot_mass, int32_t substeps, double ground_z, double contact_tol) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (!all_finite({foot_mass, ground_z, contact_tol})) return set_err(ctx, MPCQP_ERR_ARG, "non-finite plant constant");
  if (!(foot_mass > 0.0)) return set_err(ctx, MPCQP_ERR_ARG, "plant: foot_mass <= 0");
  if (substeps < 1 || substeps > MPCQP_PLANT_MAX_SUBSTEPS)
    return set_err(ctx, MPCQP_ERR_ARG, "plant: substeps outside 1..16");
  ctx->plant_foot_mass = foot_mass;
  ctx->plant_substeps = substeps;
  ctx->plant_ground_z = ground_z;
  ctx->plant_ground_set = true;
  ctx->plant_contact_tol = contact_tol;
  return MPCQP_OK;
}

static PlantParams plant_params(const mpcqp_ctx* ctx) {
  PlantParams pp;
  pp.dt_control = ctx->dt_control;
  pp.gravity = ctx->gravity;
  pp.foot_mass = ctx->plant_foot_mass;
  pp.ground_z = ctx->plant_ground_set ? ctx->plant_ground_z : ctx->touchdown_z;
  pp.contact_tol = ctx->plant_contact_tol;
  pp.substeps = ctx->plant_substeps;
  return pp;
}

int mpcqp_plant(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* tau, const float* robot, const double* geom,
                const float* plane, double* plant_state, float* root_states, float* dof_states, float* gyro,
                float* accel, float* touch, int32_t* status, void* stream) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (flags != 0) return set_err(ctx, MPCQP_ERR_ARG, "unknown plant flags");
  if (batch < 0) return set_err(ctx, MPCQP_ERR_ARG, "plant: batch < 0");
  if (!tau || !robot || !geom || !plant_state || !root_states || !dof_states)
    return set_err(ctx, MPCQP_ERR_ARG, "null plant input/state/output pointer");
  if (int rc = aligned16(ctx, plant_state, "plant_state")) return rc;
  if ((uintptr_t)dof_states & 7) return set_err(ctx, MPCQP_ERR_ARG, "plant: dof_states is not 8-byte aligned");
  if (batch == 0) return MPCQP_OK;
  DeviceScope dev(ctx->device);
  if (!dev.ok) return set_err(ctx, MPCQP_ERR_HIP, "hipSetDevice failed");
  hipLaunchKernelGGL(mpcqp_plant_kernel, dim3((batch + kPlantRobots - 1) / kPlantRobots), dim3(kPlantThreads), 0,
                     (hipStream_t)stream, plant_params(ctx), (int)batch, tau, robot, geom, plane, plant_state,
                     root_states, dof_states, gyro, accel, touch, status);
  return launched(ctx, "plant launch");
}

int mpcqp_plant_reset(mpcqp_ctx* ctx, int32_t batch, const float* root_states, const float* dof_states,
                      const double* geom, const float* plane, double* plant_state, void* stream) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (batch < 0) return set_err(ctx, MPCQP_ERR_ARG, "plant reset: batch < 0");
  if (!root_states || !dof_states || !geom || !plant_state)
    return set_err(ctx, MPCQP_ERR_ARG, "null plant reset input/state pointer");
  if (int rc = aligned16(ctx, plant_state, "plant_state")) return rc;
  if (batch == 0) return MPCQP_OK;
  DeviceScope dev(ctx->device);
  if (!dev.ok) return set_err(ctx, MPCQP_ERR_HIP, "hipSetDevice failed");
  hipLaunchKernelGGL(mpcqp_plant_reset_kernel, dim3((batch + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                     plant_params(ctx), (int)batch, root_states, dof_states, geom, plane, plant_state);
  return launched(ctx, "plant reset launch");
}

// ---- the gait scheduler (mpcqp_gait.h): what scripts/mujoco_aliengo.py:121-155 does by hand
// between two runs (fresh Gait objects, iter_counter back at 0; gait.py:76-121), per robot and at
// a tick that cuts no swing.  An invalid library or constant leaves the previous one in force.
int mpcqp_set_gaits(mpcqp_ctx* ctx, int32_t count, const int32_t* records) {
  if (!ctx) return MPCQP_ERR_ARG;
  int lib[GAIT_LIB_MAX * GAIT_LIB_WORDS] = {};
  int which = -1;
  switch (gait_library(count, records, lib, &which)) {
    case 0: break;
    case 1: return set_err(ctx, MPCQP_ERR_ARG, "gaits: count outside 1..16 or no records");
    case 2:
      return set_err(ctx, MPCQP_ERR_ARG, "gaits: record " + std::to_string(which) +
                                             " needs 1 <= P <= 2048, 0 <= dur <= P and |off| <= 4 P");
    default: return set_err(ctx, MPCQP_ERR_ARG, "gaits: record " + std::to_string(which) + " has no entry segment");
  }
  DeviceScope dev(ctx->device);
  if (!dev.ok) return set_err(ctx, MPCQP_ERR_HIP, "hipSetDevice failed");
  // into a fresh buffer; the context changes only once the upload succeeded
  int32_t* nb = nullptr;
  if (hipMalloc(&nb, sizeof(lib)) != hipSuccess) return set_err(ctx, MPCQP_ERR_ALLOC, "gaits: allocation failed");
  if (hipMemcpy(nb, lib, sizeof(lib), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(nb);
    return set_err(ctx, MPCQP_ERR_HIP, "gaits: upload failed");
  }
  // launches on any stream may still read the previous buffer: retired, not freed (640 bytes
  // each), and released at mpcqp_destroy -- or, past kMaxRetired changes, after a synchronisation
  if (ctx->gait_dev) {
    if (ctx->gait_retired.size() >= kMaxRetired) {
      if (hipDeviceSynchronize() != hipSuccess) {
        (void)hipFree(nb);
        return set_err(ctx, MPCQP_ERR_HIP, "gaits: device sync failed");
      }
      for (int32_t* o : ctx->gait_retired) (void)hipFree(o);
      ctx->gait_retired.clear();
    }
    ctx->gait_retired.push_back(ctx->gait_dev);
  }
  ctx->gait_dev = nb;
  ctx->gait_count = count;
  memcpy(ctx->gait_lib, lib, sizeof(lib));
  if (ctx->sched_idle >= count || ctx->sched_move >= count) ctx->sched_idle = ctx->sched_move = -1;
  return MPCQP_OK;
}

int mpcqp_set_gait_schedule(mpcqp_ctx* ctx, int32_t min_hold, int32_t idle_gait, int32_t move_gait, double v_go,
                            double v_stop, double w_go, double w_stop, int32_t dwell) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (min_hold < 0) return set_err(ctx, MPCQP_ERR_ARG, "gait schedule: min_hold < 0");
  if (!all_finite({v_go, v_stop, w_go, w_stop})) return set_err(ctx, MPCQP_ERR_ARG, "non-finite gait schedule constant");
  if (idle_gait != -1) {
    if (idle_gait < 0 || idle_gait >= ctx->gait_count || move_gait < 0 || move_gait >= ctx->gait_count)
      return set_err(ctx, MPCQP_ERR_ARG, "gait schedule: idle_gait or move_gait outside the library");
    if (v_stop < 0.0 || v_stop > v_go || w_stop < 0.0 || w_stop > w_go)
      return set_err(ctx, MPCQP_ERR_ARG, "gait schedule: needs 0 <= v_stop <= v_go and 0 <= w_stop <= w_go");
    if (dwell < 0) return set_err(ctx, MPCQP_ERR_ARG, "gait schedule: dwell < 0");
  }
  ctx->sched_min_hold = min_hold;
  ctx->sched_idle = idle_gait;
  ctx->sched_move = idle_gait == -1 ? -1 : move_gait;
  ctx->sched_v_go = v_go, ctx->sched_v_stop = v_stop, ctx->sched_w_go = w_go, ctx->sched_w_stop = w_stop;
  ctx->sched_dwell = dwell;
  return MPCQP_OK;
}

int mpcqp_gait_schedule(mpcqp_ctx* ctx, int32_t batch, int32_t flags, int32_t iterations_between_mpc,
                        const int32_t* want, const double* vel_body_des, const double* yaw_rate_des,
                        int32_t* sched_state, int32_t* gait, int32_t* tick, double* swing_mem, int32_t* iteration,
                        int32_t* switched, int32_t* status, void* stream) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (flags & ~MPCQP_GAIT_ADVANCE) return set_err(ctx, MPCQP_ERR_ARG, "unknown gait schedule flags");
  if (batch < 0) return set_err(ctx, MPCQP_ERR_ARG, "gait schedule: batch < 0");
  if (iterations_between_mpc < 1) return set_err(ctx, MPCQP_ERR_ARG, "iterations_between_mpc < 1");
  if (!sched_state || !gait || !tick) return set_err(ctx, MPCQP_ERR_ARG, "null gait schedule state pointer");
  if (ctx->gait_count < 1) return set_err(ctx, MPCQP_ERR_ARG, "gait schedule: no library set (mpcqp_set_gaits)");
  if (!want && ctx->sched_idle < 0)
    return set_err(ctx, MPCQP_ERR_ARG, "gait schedule: no want and the automatic choice is disabled");
  if (!want && (!vel_body_des || !yaw_rate_des))
    return set_err(ctx, MPCQP_ERR_ARG, "gait schedule: the automatic choice needs vel_body_des and yaw_rate_des");
  if (int rc = aligned16(ctx, sched_state, "sched_state")) return rc;
  if (int rc = aligned16(ctx, swing_mem, "swing_mem")) return rc;
  for (int i = 0; i < ctx->gait_count; ++i)
    if ((long long)ctx->gait_lib[GAIT_LIB_WORDS * i + GAIT_WORDS] * iterations_between_mpc > GAIT_INT_MAX)
      return set_err(ctx, MPCQP_ERR_ARG, "gait schedule: an entry tick is beyond INT32_MAX");
  if (batch == 0) return MPCQP_OK;
  DeviceScope dev(ctx->device);
  if (!dev.ok) return set_err(ctx, MPCQP_ERR_HIP, "hipSetDevice failed");
  GaitParams gp;
  gp.count = ctx->gait_count;
  gp.ibm = iterations_between_mpc;
  gp.flags = flags;
  gp.min_hold = ctx->sched_min_hold;
  gp.idle = ctx->sched_idle, gp.move = ctx->sched_move;
  gp.dwell = ctx->sched_dwell;
  gp.v_go2 = ctx->sched_v_go * ctx->sched_v_go, gp.v_stop2 = ctx->sched_v_stop * ctx->sched_v_stop;
  gp.w_go = ctx->sched_w_go, gp.w_stop = ctx->sched_w_stop;
  hipLaunchKernelGGL(mpcqp_gait_kernel, dim3((batch + kGaitThreads - 1) / kGaitThreads), dim3(kGaitThreads), 0,
                     (hipStream_t)stream, gp, (int)batch, (const int32_t*)ctx->gait_dev, want, vel_body_des,
                     yaw_rate_des, sched_state, gait, tick, swing_mem, iteration, switched, status);
  return launched(ctx, "gait schedule launch");
}

// ---- the sensor model and the push (mpcqp_sensors.h): the reference's scripts read a simulator's
// sensors as they come and never disturb the robot (gym.simulate, sim.step()).  An invalid
// constant leaves the previous set in force.
int mpcqp_set_sensors(mpcqp_ctx* ctx, uint64_t seed, double sigma_gyro, double sigma_accel, double walk_gyro,
                      double walk_accel, double bias0_gyro, double bias0_accel, double sigma_q, double sigma_qd,
                      double q_lsb, int32_t touch_lag, double p_drop) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (!all_finite({sigma_gyro, sigma_accel, walk_gyro, walk_accel, bias0_gyro, bias0_accel, sigma_q, sigma_qd, q_lsb,
                   p_drop}))
    return set_err(ctx, MPCQP_ERR_ARG, "non-finite sensor constant");
  for (double v : {sigma_gyro, sigma_accel, walk_gyro, walk_accel, bias0_gyro, bias0_accel, sigma_q, sigma_qd, q_lsb})
    if (v < 0.0) return set_err(ctx, MPCQP_ERR_ARG, "negative sensor constant");
  if (touch_lag < 0 || touch_lag > SENSE_MAX_LAG) return set_err(ctx, MPCQP_ERR_ARG, "sensors: touch_lag outside 0..31");
  if (!(p_drop >= 0.0 && p_drop < 1.0)) return set_err(ctx, MPCQP_ERR_ARG, "sensors: p_drop outside [0, 1)");
  ctx->sense_seed = seed;
  ctx->sense_sigma_gyro = sigma_gyro, ctx->sense_sigma_accel = sigma_accel;
  ctx->sense_walk_gyro = walk_gyro, ctx->sense_walk_accel = walk_accel;
  ctx->sense_bias0_gyro = bias0_gyro, ctx->sense_bias0_accel = bias0_accel;
  ctx->sense_sigma_q = sigma_q, ctx->sense_sigma_qd = sigma_qd, ctx->sense_q_lsb = q_lsb;
  ctx->sense_touch_lag = touch_lag;
  ctx->sense_p_drop = p_drop;
  return MPCQP_OK;
}

int mpcqp_sensors(mpcqp_ctx* ctx, int32_t batch, int32_t flags, const float* gyro, const float* accel,
                  const float* dof_states, const float* touch, const float* scale, double* sense_state,
                  float* gyro_m, float* accel_m, float* dof_states_m, float* touch_m, int32_t* status, void* stream) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (flags != 0) return set_err(ctx, MPCQP_ERR_ARG, "unknown sensors flags");
  if (batch < 0) return set_err(ctx, MPCQP_ERR_ARG, "sensors: batch < 0");
  if (!sense_state) return set_err(ctx, MPCQP_ERR_ARG, "null sense_state pointer");
  if (!gyro != !gyro_m || !accel != !accel_m || !dof_states != !dof_states_m || !touch != !touch_m)
    return set_err(ctx, MPCQP_ERR_ARG, "sensors: an input and its output are given together or not at all");
  if (int rc = aligned16(ctx, sense_state, "sense_state")) return rc;
  if (((uintptr_t)dof_states | (uintptr_t)dof_states_m) & 7)
    return set_err(ctx, MPCQP_ERR_ARG, "sensors: dof_states or dof_states_m is not 8-byte aligned");
  if (batch == 0) return MPCQP_OK;
  DeviceScope dev(ctx->device);
  if (!dev.ok) return set_err(ctx, MPCQP_ERR_HIP, "hipSetDevice failed");
  SenseParams sp;
  sp.key0 = (uint32_t)ctx->sense_seed, sp.key1 = (uint32_t)(ctx->sense_seed >> 32);
  sp.sigma_gyro = ctx->sense_sigma_gyro, sp.sigma_accel = ctx->sense_sigma_accel;
  sp.walk_gyro = ctx->sense_walk_gyro, sp.walk_accel = ctx->sense_walk_accel;
  sp.bias0_gyro = ctx->sense_bias0_gyro, sp.bias0_accel = ctx->sense_bias0_accel;
  sp.sigma_q = ctx->sense_sigma_q, sp.sigma_qd = ctx->sense_sigma_qd, sp.q_lsb = ctx->sense_q_lsb;
  sp.sqrt_dt = std::sqrt(ctx->dt_control);
  sp.drop = (uint32_t)std::floor(ctx->sense_p_drop * 4294967296.0);
  sp.touch_lag = ctx->sense_touch_lag;
  hipLaunchKernelGGL(mpcqp_sensors_kernel, dim3((batch + kSenseRobots - 1) / kSenseRobots), dim3(kSenseThreads), 0,
                     (hipStream_t)stream, sp, (int)batch, gyro, accel, dof_states, touch, scale, sense_state, gyro_m,
                     accel_m, dof_states_m, touch_m, status);
  return launched(ctx, "sensors launch");
}

int mpcqp_push(mpcqp_ctx* ctx, int32_t batch, const float* impulse, const float* point, const float* robot,
               double* plant_state, int32_t* status, void* stream) {
  if (!ctx) return MPCQP_ERR_ARG;
  if (batch < 0) return set_err(ctx, MPCQP_ERR_ARG, "push: batch < 0");
  if (!impulse || !robot || !plant_state) return set_err(ctx, MPCQP_ERR_ARG, "null push input/state pointer");
  if (int rc = aligned16(ctx, plant_state, "plant_state")) return rc;
  if (batch == 0) return MPCQP_OK;
  DeviceScope dev(ctx->device);
  if (!dev.ok) return set_err(ctx, MPCQP_ERR_HIP, "hipSetDevice failed");
  hipLaunchKernelGGL(mpcqp_push_kernel, dim3((batch + 63) / 64), dim3(64), 0, (hipStream_t)stream, (int)batch, impulse,
                     point, robot, plant_state, status);
  return launched(ctx, "push launch");
}

int mpcqp_destroy(mpcqp_ctx* ctx) {
  if (ctx) {
    DeviceScope dev(ctx->device);
    // hipFree synchronises the device before releasing the memory: no per-stream sync
    // (a recorded stream may already have been destroyed by the caller)
    for (auto& q : ctx->queues) release_set(q);
    if (ctx->sscratch) (void)hipFree(ctx->sscratch);
    if (ctx->prio_tab) (void)hipFree(ctx->prio_tab);
    if (ctx->wdev) (void)hipFree(ctx->wdev);
    for (double* o : ctx->retired) (void)hipFree(o);
    if (ctx->gait_dev) (void)hipFree(ctx->gait_dev);
    for (int32_t* o : ctx->gait_retired) (void)hipFree(o);
  }
  delete ctx;
  return MPCQP_OK;
}

const char* mpcqp_last_error(const mpcqp_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

}  // extern "C"

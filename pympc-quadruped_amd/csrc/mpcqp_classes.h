// mpcqp_classes.h -- the solve's kernels (included by mpcqp.hip inside its anonymous namespace,
// after every kernel header): the dispatch order, and one __global__ wrapper per capacity
// class around solve_robot (mpcqp_solve.h) / solve_robot_ipm (mpcqp_ipm.h) with the queue
// protocol that feeds it.  Which of them a call launches is mpcqp_solve_plan.h's decision.


// Workgroups are dealt round-robin over the 8 XCDs (block bid runs on XCD bid % 8,
// MI355X_MICROARCH.md "Workgroup dispatch"; speed only, never correctness).  Block bid
// solves robot xcd_robot(bid, B): each XCD takes one contiguous range of robots, so
// neighbouring robots -- whose input records and u0 / status / iters entries share
// cache lines -- meet in one L2 and their lines are fetched and written back once.
// A bijection of [0, B) for every B.
__device__ __forceinline__ int xcd_robot(int bid, int B) {
  const int x = bid & 7, i = bid >> 3, q = B >> 3, r = B & 7;
  return x * q + (x < r ? x : r) + i;
}

// ---- Dispatch order (ABI 6, mpcqp_set_order).  A robot's active set -- and so its solve
// time -- grows with the horizontal velocity correction its cone forces must supply: on the
// benchmark batches |v0 - vref_0| has correlation 0.87 (config 2) / 0.85 (config 4) with the
// iteration count (tools/order_sim.py).  mpcqp_order_kernel sorts each dispatch segment by
// that key, largest first, so that in a batch that queues on the CUs (configs 3 to 5) the longest
// robots start first and the launch ends near its mean load instead of behind a late long
// robot (configs 3 / 4 / 5 +7.7 / +6.2 / +3.7 %, profiles/r5_combo/ab_order.txt).  Only the
// robot -> workgroup map changes: every robot's solve is bitwise the same.
constexpr int kOrderBuckets = 256;

__device__ __forceinline__ float order_key(const float* __restrict__ x0g, const float* __restrict__ xrefg, int N,
                                           int r) {
  const float ex = x0g[(size_t)r * NX + 9] - xrefg[(size_t)r * N * NX + 9];
  const float ey = x0g[(size_t)r * NX + 10] - xrefg[(size_t)r * N * NX + 10];
  const float k = ex * ex + ey * ey;
  return k >= 0.0f && k <= 3.0e38f ? k : 0.0f;   // NaN / inf: no preference
}

// One 1024-thread workgroup per segment, a counting sort into 256 key buckets, largest first
// (the order within a bucket is the atomics' order: it is a schedule, not a result).  A segment
// is the robots start + stride j (j < len), and rank r goes to position start + stride r:
//   mode 0: the 8 contiguous XCD ranges of class 64 (xcd_robot: the robots of blocks x, x + 8,
//           ...), so a sorted range keeps its robots on their XCD's L2;
//   mode 1: ceil(B / 1024) interleaved segments (stride = their count) for classes 96 / 128
//           taking the batch directly: position s + S r holds segment s's r-th heaviest robot,
//           so the workgroups dispatched first get the heaviest robots of every segment.
// Buckets: sqrt(key / max key) in 256 steps (|v0 - vref_0| relative to the batch's largest).
__global__ __launch_bounds__(1024) void mpcqp_order_kernel(int B, int N, const float* __restrict__ x0g,
                                                           const float* __restrict__ xrefg, int* __restrict__ perm,
                                                           int mode) {
  __shared__ int hist[kOrderBuckets], cursor[kOrderBuckets];
  __shared__ unsigned kmax_bits;
  __shared__ int wsum[kOrderBuckets / LANES];
  const int seg = blockIdx.x, tid = threadIdx.x, lane = tid & (LANES - 1);
  int start, stride, len;
  if (mode == 0) {
    const int q = B >> 3, r = B & 7;
    start = seg * q + (seg < r ? seg : r);
    stride = 1;
    len = q + (seg < r ? 1 : 0);
  } else {
    const int S = (B + kOrderSeg - 1) / kOrderSeg;
    start = seg;
    stride = S;
    len = (B - seg + S - 1) / S;
  }
  constexpr int KPT = kOrderMax / 1024;   // keys per thread
  float key[KPT];
  float kmx = 0.0f;
#pragma unroll
  for (int t = 0; t < KPT; ++t) {
    const int j = tid + 1024 * t;
    key[t] = j < len ? order_key(x0g, xrefg, N, start + stride * j) : 0.0f;
    kmx = fmaxf(kmx, key[t]);
  }
  if (tid < kOrderBuckets) hist[tid] = cursor[tid] = 0;
  if (tid == 0) kmax_bits = 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmx = fmaxf(kmx, __shfl_xor(kmx, o));
  __syncthreads();
  if (lane == 0) atomicMax(&kmax_bits, __float_as_uint(kmx));   // non-negative floats order as bits
  __syncthreads();
  const float inv = kmax_bits ? 1.0f / __uint_as_float(kmax_bits) : 0.0f;
  int bk[KPT];
#pragma unroll
  for (int t = 0; t < KPT; ++t) {
    const int j = tid + 1024 * t;
    const int b = min(kOrderBuckets - 1, (int)((float)kOrderBuckets * sqrtf(key[t] * inv)));
    bk[t] = kOrderBuckets - 1 - b;   // descending: the largest keys first
    if (j < len) atomicAdd(&hist[bk[t]], 1);
  }
  __syncthreads();
  // exclusive scan of the 256 bucket counts (4 waves)
  if (tid < kOrderBuckets) {
    const int v = hist[tid];
    int x = v;
#pragma unroll
    for (int o = 1; o < LANES; o <<= 1) {
      const int y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    if (lane == LANES - 1) wsum[tid >> 6] = x;
    hist[tid] = x - v;   // exclusive within the wave
  }
  __syncthreads();
  if (tid < kOrderBuckets) {
    int off = 0;
    for (int w = 0; w < (tid >> 6); ++w) off += wsum[w];
    hist[tid] += off;
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < KPT; ++t) {
    const int j = tid + 1024 * t;
    if (j < len) {
      const int pos = hist[bk[t]] + atomicAdd(&cursor[bk[t]], 1);
      perm[start + stride * pos] = start + stride * j;
    }
  }
}

// kIpmPerCU slots per CU are enough (mpcqp_solve_plan.h): every layout is LDS-bound to fewer
template <int NM, bool FULL, bool MG>
constexpr bool ipm_within_slots() {
  return sizeof(IpmSharedT<NM, FULL, MG>) > 160 * 1024 / (kIpmPerCU + 1);
}
static_assert(ipm_within_slots<16, false, true>() && ipm_within_slots<16, true, true>() &&
                  ipm_within_slots<16, false, false>() && ipm_within_slots<16, true, false>() &&
                  ipm_within_slots<kDenseN, false, false>() && ipm_within_slots<kDenseN, true, false>() &&
                  ipm_within_slots<kMaxN, false, false>() && ipm_within_slots<kMaxN, true, false>(),
              "an interior-point layout fits more workgroups on a CU than kIpmPerCU slots");

// Class NV = 64: one 2-wave workgroup per robot of the batch.  Robots with more
// than 64 stance variables are appended to `queue` (when given) for class 96, those
// with more than 96 to `queue_big` (when given) for class 128.
// PRIO: the instantiation with the setup priority (solve_robot), for a batch the chip holds at
// once; without it the kernel has none of that code and ignores its last two arguments.
template <bool FULL, bool PRIO = false>
__global__ __launch_bounds__(Cfg<64>::NT) __attribute__((amdgpu_waves_per_eu(2, Cfg<64>::NW))) void mpcqp_kernel_64(
    KParams P, int B, const float* __restrict__ x0g, const float* __restrict__ xrefg,
    const float* __restrict__ contactg, const float* __restrict__ feetg, const float* __restrict__ robotg,
    float* __restrict__ u0g, float* __restrict__ Ug, int* __restrict__ statusg, int* __restrict__ itersg,
    int* __restrict__ queue, int* __restrict__ queue_big, int* __restrict__ queue_ipm, const int* __restrict__ perm,
    unsigned long long* __restrict__ prio_tab, unsigned prio_epoch) {
  if ((int)blockIdx.x >= B) return;
  int b = xcd_robot(blockIdx.x, B);
  if (perm) b = uni(perm[b]);   // the dispatch order (mpcqp_order_kernel, mode 0)
  // the setup priority's value (solve_robot): the dispatch order's key under this launch's epoch
  // (non-negative floats order as their bits)
  unsigned long long prio_val = 0ull;
  if constexpr (PRIO)
    prio_val = ((unsigned long long)prio_epoch << 32) | __float_as_uint(order_key(x0g, xrefg, P.N, b));
  __shared__ SharedT<64> sm;
  solve_robot<64, FULL, PRIO>(P, b, sm, x0g, xrefg, contactg, feetg, robotg, u0g, Ug, statusg, itersg, queue, queue_big,
                  queue_ipm, prio_tab, prio_val);
}

// ---- The queued classes' protocol (classes 96 / 128 / interior point).  A launch has one
// workgroup per robot of the batch (the host cannot know the queue length without a sync);
// the ones beyond the queue count exit at once.  The last queued robot's workgroup to finish
// resets the counters for the next launch (queue[0] = count, queue[2] = finished workgroups,
// queue[4..] = robot indices).  A class that takes the batch directly (direct_B > 0: the caller's
// stance range rules the classes before it out) touches no queue: robot = workgroup, or perm's.
__device__ __forceinline__ int queue_count(const int* queue) {
  return uni(__hip_atomic_load(&queue[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
// only the cnt workers count themselves (no contended atomic from the idle rest)
__device__ __forceinline__ void queue_done(int* queue, int cnt) {
  if (atomicAdd(&queue[2], 1) == cnt - 1) {
    atomicExch(&queue[0], 0);
    atomicExch(&queue[2], 0);
  }
}

// Class NV = 96: one 6-wave workgroup (4 x 6 register tiles) per robot queued by
// class 64 (64 < n <= 96: the N = 16 trot / pace / bound schedules); robots with more
// stance variables go on to class 128 through `qout`.
template <bool FULL>
__global__ __launch_bounds__(Cfg<96>::NT) __attribute__((amdgpu_waves_per_eu((Cfg<96>::NW + 3) / 4, (Cfg<96>::NW + 3) / 4))) void mpcqp_kernel_96(
    KParams P, const float* __restrict__ x0g, const float* __restrict__ xrefg,
    const float* __restrict__ contactg, const float* __restrict__ feetg, const float* __restrict__ robotg,
    float* __restrict__ u0g, float* __restrict__ Ug, int* __restrict__ statusg, int* __restrict__ itersg,
    int* __restrict__ queue, int* __restrict__ qout, int* __restrict__ q_ipm, int direct_B,
    const int* __restrict__ perm) {
  __shared__ SharedT<96> sm;
  const int tid = threadIdx.x;
  const int k = blockIdx.x;
  if (direct_B > 0) {   // the caller's stance range rules class 64 out: robot = workgroup (or perm[k])
    if (k < direct_B)
      solve_robot<96, FULL>(P, perm ? uni(perm[k]) : k, sm, x0g, xrefg, contactg, feetg, robotg, u0g, Ug, statusg,
                            itersg, qout, nullptr, q_ipm);
    return;
  }
  const int cnt = queue_count(queue);
  if (k < cnt) {
    const int b = uni(queue[4 + k]);
    solve_robot<96, FULL>(P, b, sm, x0g, xrefg, contactg, feetg, robotg, u0g, Ug, statusg, itersg, qout, nullptr, q_ipm);
    if (tid == 0) queue_done(queue, cnt);
  }
}

// Class NV = 128: one 8-wave workgroup per queued robot.  Workloads that fit class 64 skip
// this launch via mpcqp_set_stance_hint.
template <bool FULL>
__global__ __launch_bounds__(Cfg<128>::NT) void mpcqp_kernel_128(
    KParams P, const float* __restrict__ x0g, const float* __restrict__ xrefg,
    const float* __restrict__ contactg, const float* __restrict__ feetg, const float* __restrict__ robotg,
    float* __restrict__ u0g, float* __restrict__ Ug, int* __restrict__ statusg, int* __restrict__ itersg,
    int* __restrict__ queue, int* __restrict__ q_ipm, int direct_B, const int* __restrict__ perm) {
  __shared__ SharedT<128> sm;
  const int tid = threadIdx.x;
  const int k = blockIdx.x;
  if (direct_B > 0) {
    if (k < direct_B)
      solve_robot<128, FULL>(P, perm ? uni(perm[k]) : k, sm, x0g, xrefg, contactg, feetg, robotg, u0g, Ug, statusg,
                             itersg, q_ipm, nullptr, q_ipm);
    return;
  }
  const int cnt = queue_count(queue);
  if (k < cnt) {
    const int b = uni(queue[4 + k]);
    solve_robot<128, FULL>(P, b, sm, x0g, xrefg, contactg, feetg, robotg, u0g, Ug, statusg, itersg, q_ipm, nullptr, q_ipm);
    if (tid == 0) queue_done(queue, cnt);
  }
}

// A free slot of the interior-point class's global S_k scratch: one bit per slot in `bits`
// (nw words), claimed with atomicOr, released with atomicAnd.  The search terminates: a slot
// holder never waits for anything before it releases its slot, and there are at least as
// many slots as workgroups of the class can be resident at once (kIpmPerCU per CU, every
// layout LDS-bound to at most that: the static_assert above), so a free one exists whenever
// a workgroup searches.  Called by one lane.
__device__ __forceinline__ int ipm_claim_slot(unsigned* bits, int nw, int start) {
  for (int i = 0;; ++i) {
    if (i >= nw) __builtin_amdgcn_s_sleep(2);   // a full sweep found none: back off (never expected)
    const int w = (start + i) % nw;
    unsigned m = ~__hip_atomic_load(&bits[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (m) {
      const int bit = __builtin_ctz(m);
      const unsigned old = atomicOr(&bits[w], 1u << bit);
      if (!(old & (1u << bit))) return 32 * w + bit;
      m &= ~old & ~(1u << bit);
    }
  }
}

// Large class (n > 128, and every robot at N > 20): Riccati-factored interior point +
// active-set polish (mpcqp_ipm.h), one wave per robot; its Riccati S_k in a global slot
// claimed for the robot's solve (sbits: slot bitmap, nsw words).  The queued classes' count and
// reset.  FULL: non-diagonal weights (mpcqp_set_weights).
// One wave per SIMD at most (LDS bounds a CU to 3 or 4 of these workgroups): the wave may take
// the whole 512-register file, so values beyond the 256 arch VGPRs live in AGPRs, not scratch
// XR: an R with cross-leg couplings (full-weight latency layouts only)
template <bool FULL, int NM, bool MG = false, bool XR = false>
__global__ __launch_bounds__(LANES) __attribute__((amdgpu_waves_per_eu(1, 1))) void mpcqp_kernel_ipm(
    KParams P, const float* __restrict__ x0g, const float* __restrict__ xrefg,
    const float* __restrict__ contactg, const float* __restrict__ feetg, const float* __restrict__ robotg,
    float* __restrict__ u0g, float* __restrict__ Ug, int* __restrict__ statusg, int* __restrict__ itersg,
    int* __restrict__ queue, int direct_B, double* __restrict__ sscratch, unsigned* __restrict__ sbits,
    int nsw) {
  __shared__ IpmSharedT<NM, FULL, MG> sm;
  const int tid = threadIdx.x;
  const int k = blockIdx.x;
  // direct_B > 0: the caller's stance range (or N > 20) rules the dense classes out, robot = k
  const bool direct = direct_B > 0;
  const int cnt = direct ? direct_B : queue_count(queue);
  if (k >= cnt) return;   // idle workgroups touch no counter
  const int b = direct ? k : uni(queue[4 + k]);
  int slot = 0;
  if (tid == 0) slot = ipm_claim_slot(sbits, nsw, k % nsw);
  slot = __builtin_amdgcn_readlane(slot, 0);
  solve_robot_ipm<FULL, NM, MG, XR>(P, b, sm, sscratch + (size_t)slot * IpmSlot<NM>::SIZE, x0g, xrefg, contactg, feetg, robotg, u0g,
                            Ug, statusg, itersg);
  if (tid == 0) {
    atomicAnd(&sbits[slot >> 5], ~(1u << (slot & 31)));   // the solve's S_k reads are done
    // only the queued robots count themselves; the last one resets the queue
    if (!direct) queue_done(queue, cnt);
  }
}

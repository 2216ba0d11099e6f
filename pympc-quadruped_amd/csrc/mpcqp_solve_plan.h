// mpcqp_solve_plan.h -- what one mpcqp_solve call launches, decided from the context's
// settings and the batch size alone: plain C++ with no HIP and no allocation, so tests/ can
// drive it on the CPU (tests/test_solve_plan.py).  enqueue_solve (mpcqp.hip) computes the
// plan and carries it out; the kernels (mpcqp_classes.h) take their constants from here.
//
// A robot has n = 3 * #stance <= 12 N variables.  Robots with more than 64 are queued
// for class 96, more than 96 for class 128, more than 128 for the interior-point
// class -- each queued launch skipped when no robot can need it (horizon, or the
// caller's stance range).  When the range rules out the smaller classes, the first
// class that can be needed takes the batch directly (one workgroup per robot) and
// routes the larger robots on.
//
// Only the classes launched and the robots they take change a result; the order, the
// priority, the interior-point layout and the fork are a schedule.
#pragma once

// class 64's capacity (stance variables)
constexpr int kCap64 = 64;
constexpr int kDenseN = 20;   // the dense classes' LDS layouts hold N <= 20; longer horizons go to
                              // the interior-point class, sized for N <= kMaxN
constexpr int kOrderMax = 8192;   // class 64: robots per XCD range the order kernel takes (8 per thread)
constexpr int kOrderSeg = 1024;   // classes 96 / 128: robots per interleaved segment (one per thread)
constexpr int kOrderMin = 64;     // smaller batches keep their order (nothing to balance)
// interior-point class: global S_k slots per CU.  Every layout takes more than a fifth of a
// CU's LDS, so at most kIpmPerCU of its (one-wave) workgroups are resident on a CU at once
// and a claim finds a free slot without waiting (ipm_claim_slot).
constexpr int kIpmPerCU = 4;

// the classes, in launch order
enum SolveClass { kClass64 = 0, kClass96 = 1, kClass128 = 2, kClassIpm = 3 };

struct SolveInput {
  int horizon;
  int stance_min, stance_hint;   // the caller's stance range in foot-steps (mpcqp_set_stance_range); 0: none
  int order;         // mpcqp_set_order
  int ncu;
  int batch;
  bool full;         // non-diagonal weights (mpcqp_set_weights)
  bool xr;           // R couples different legs
};

struct SolvePlan {
  int first;         // the first class launched (SolveClass): it takes the batch as it stands (class 64's
                     // B, the others' direct_B) and the order's perm; the later ones are fed by its queues
  bool launch[4];    // per SolveClass
  bool queues;       // the stream's queue set is needed (a queued class, or the order's perm)
  bool order;        // mpcqp_order_kernel ahead of the first class
  int order_mode, order_segs;   // its mode (0: class 64's XCD ranges, 1: interleaved segments) and workgroups
  bool prio;         // class 64 with the setup priority
  int ipm_size;      // the interior-point LDS layout NM: 0 = 16, 1 = kDenseN, 2 = kMaxN
  bool ipm_thru;     // throughput layout (else latency)
  bool ipm_xr;       // the XR instantiation (12 x 12 stage weights, latency layouts)
  bool ipm_full;     // its FULL instantiation: non-diagonal weights, which a cross-leg R always is
  bool fork;         // the interior-point launch on the side stream, if the stream can be had
};

inline SolvePlan solve_plan(const SolveInput& in) {
  SolvePlan p = {};
  const int nmax_h = 12 * in.horizon;
  const int nmax = in.stance_hint > 0 && 3 * in.stance_hint < nmax_h ? 3 * in.stance_hint : nmax_h;
  const int nmin = 3 * in.stance_min;
  // horizons beyond the dense classes' LDS layouts (N > kDenseN): the interior-point class
  // takes the whole batch directly, whatever the stance counts
  const bool ipm_only = in.horizon > kDenseN;
  const bool large = ipm_only || nmax > kCap64, huge = !ipm_only && nmax > 96, giant = ipm_only || nmax > 128;
  // When the interior-point class may be needed beside the dense ones, class 64 routes the
  // batch (a formulation-stage pass, microseconds) so the interior-point launch forks onto
  // its side stream at once -- a dense class taking the batch directly would route its
  // standing robots only as its own workgroups run, and the fork would wait for all of it.
  p.first = ipm_only || nmin > 128 ? kClassIpm : giant ? kClass64 : nmin > 96 ? kClass128 : nmin > kCap64 ? kClass96 : kClass64;
  p.launch[kClass64] = p.first == kClass64;
  p.launch[kClass96] = large && p.first <= kClass96;
  p.launch[kClass128] = huge && p.first <= kClass128;
  p.launch[kClassIpm] = giant;
  // the dispatch order (mpcqp_order_kernel) of the first class's launch: class 64 sorts its 8 XCD
  // ranges (each <= kOrderMax robots), classes 96 / 128 taking the batch directly sort interleaved
  // segments of <= kOrderSeg; the interior-point class and small batches keep the batch order
  // -- only when the batch queues on the CUs: a batch the chip holds at once (config 2: 1024
  // robots = 4 per CU) gains nothing from its order (the heaviest robots' CU-mates are lighter
  // either way, measured) and would pay the sort launch (config 2 -1.5 %, profiles/r5_combo/)
  const int resident = (p.first == kClass64 ? 4 : 1) * in.ncu;   // class 64: 4 workgroups per CU; 96 / 128: 1
  p.order = in.order && in.batch >= kOrderMin && in.batch > resident && p.first < kClassIpm &&
            (p.first > kClass64 || in.batch <= 8 * kOrderMax);
  p.order_mode = p.first == kClass64 ? 0 : 1;
  p.order_segs = p.first == kClass64 ? 8 : (in.batch + kOrderSeg - 1) / kOrderSeg;
  p.queues = large || p.order;
  // the setup priority (solve_robot) only for a batch the chip holds at once, whose launch lasts
  // as long as its slowest robot; a batch that queues on the CUs is throughput-bound, and there
  // the raised robots' gain did not cover their CU-mates' loss (config 3 -0.2 to -0.5 %, measured)
  p.prio = p.first == kClass64 && in.batch <= resident;
  // the LDS layout for the horizon: N <= 16 (the reference's default) three robots per CU,
  // N <= 20 one, longer horizons (up to kMaxN) one
  p.ipm_size = in.horizon <= 16 ? 0 : in.horizon <= kDenseN ? 1 : 2;
  // A cross-leg R takes the XR instantiations: 12 x 12 stage weights, latency layouts.
  p.ipm_xr = in.xr;
  p.ipm_full = in.full || in.xr;
  // N <= 16: the throughput layout (four robots per CU, M_k in the global slot) when the
  // class takes a batch larger than three robots per CU can hold at once; otherwise -- a
  // single drop-in robot, or robots queued from a mixed batch, whose latency is the
  // launch's tail -- the latency layout (M_k in LDS, three per CU)
  p.ipm_thru = !in.xr && in.horizon <= 16 && p.first == kClassIpm && in.batch > 3 * in.ncu;
  // the interior-point class (one wave per robot, latency-bound) on a side stream as soon
  // as the first class has routed its robots, beside classes 96 / 128 instead of behind
  // them; the caller's stream waits for it at the end of the call
  p.fork = giant && p.first < kClassIpm;
  return p;
}

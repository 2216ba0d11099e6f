// mpcqp_certify.h -- the optimality certificate on the device: for every robot in one launch the
// gradient G = H U + g of the QP's objective phi at a force sequence U, phi(U) itself, and the
// duality gap the friction pyramids give in closed form (included by mpcqp.hip inside its
// anonymous namespace, after mpcqp_predict.h).  The algebra is mpcqp_certify_robot.h; this file
// maps a wavefront's lanes onto it.
//
// One wavefront per robot, one robot per workgroup, as mpcqp_predict_kernel.  The
// stage, the head, the forward scan and the error pass are mpcqp_predict.h's rollout_* functions,
// the ones mpcqp_predict_kernel calls, so that J and J_free are predict's to the bit:
//   stage    rollout_stage
//   head     rollout_head_scan, the cone lanes 12..20 writing the nine entries of the cone frame
//   forward  (t1, t2, n); lanes 0..11 the running sums P0 / P1 of their input column, into LDS
//   -- sync --
//   errors   rollout_errors, Q e_t going to S[t][.][0]
//   -- sync --
//   backward lanes 0..12 the sums S0 / S1 of their state component from t = N - 1 down, S0_t
//            taking the place of Q e_t
//   -- sync --
//   gradient the 12 N entries of G dealt over the lanes (entry e = lane + 64 i, i < 3 or 6), the
//            float32 kept in a register until the robot's status is known, the float64 into the
//            LDS the forward sums have left (P[t][c][0])
//   -- sync --
//   gap      the 4 N foot-step terms g_k . u_k - m_k, two per lane
//   report   per-lane partial sums reduced across the wave with __shfl_xor; no atomics
#include "mpcqp_certify_robot.h"

static_assert(CERT_REPORT == MPCQP_CERTIFY_REPORT, "report stride");

// entries of G per lane: 3 at NM = 16, 6 at NM = 32
constexpr int certify_per_lane(int NM) { return (NU * NM + LANES - 1) / LANES; }

// Per-robot LDS: the rollout's, with the cone frame and the backward sums S added: 9 808 bytes at
// <16, false> (16 robots in a CU's 160 KiB), 27 008 at <32, true>.
template <int NM, bool FULL>
struct alignas(16) CertifyShared : RolloutShared<NM, FULL> {
  double frame[10];              // t1, t2, n of the cone rows, [3][3]
  double S[NM][NX][2];           // (Q e_t, then S0_t; S1_t) per state component
};
static_assert(sizeof(CertifyShared<16, false>) == 9808 && sizeof(CertifyShared<16, true>) == 15424 &&
                  sizeof(CertifyShared<kMaxN, false>) == 18064 && sizeof(CertifyShared<kMaxN, true>) == 27008,
              "DESIGN.md 4.4j states the LDS sizes");
static_assert(CERT_OBJECTIVE == 0 && CERT_GAP == 1 && CERT_LOWER == 2 && CERT_WORST == 3,
              "rollout_store takes the report words in their order");

template <int NM, bool FULL>
__global__ __launch_bounds__(LANES) void mpcqp_certify_kernel(
    KParams P, int B, const float* __restrict__ x0g, const float* __restrict__ xrefg,
    const float* __restrict__ contactg, const float* __restrict__ feetg, const float* __restrict__ robotg,
    const float* __restrict__ Ug, float* __restrict__ Gg, double* __restrict__ reportg, int32_t* __restrict__ statusg) {
#pragma clang fp contract(off)   // as mpcqp_certify_robot.h: the host build differs in the wave sums' order alone
  constexpr int kPerLane = certify_per_lane(NM);
  __shared__ CertifyShared<NM, FULL> sm;
  const int b = blockIdx.x;
  if (b >= B) return;
  const int lane = threadIdx.x;
  const int N = P.N;
  const double h = P.dt;
  constexpr bool full = FULL;
  bool finite = rollout_stage(sm, N, b, lane, x0g, xrefg, contactg, feetg, robotg, Ug);
  float gv[kPerLane];
#pragma unroll
  for (int i = 0; i < kPerLane; ++i) gv[i] = 0.f;
  double objective = 0.0, gap = 0.0, worst = 0.0;
  if (finite) {
    const float* const rec = sm.in + IN_ROBOT;
    rollout_head_scan<FULL, 9>(sm, P, N, h, lane, [&](int e) { sm.frame[e] = cert_frame_entry(rec, e / 3, e % 3); });
    // ---- errors: Q e_t into S, the costs as predict takes them
    const double minv = sm.minv;
    double je = 0.0, jf = 0.0, ju = 0.0;
    rollout_errors<NM, FULL>(
        sm, N, h, lane, &je, &jf, [](int, double) {}, [&](int t, int sc, double qe) { sm.S[t][sc][0] = qe; });
    fsync<LANES>();
    // ---- backward scan: lanes 0..12, one state component each; S0_t replaces Q e_t
    if (lane < NX) {
      double s0 = 0.0, s1 = 0.0;
      for (int t = N - 1; t >= 0; --t) {
        cert_scan_step(&s0, &s1, sm.S[t][lane][0]);
        sm.S[t][lane][0] = s0;
        sm.S[t][lane][1] = s1;
      }
    }
    fsync<LANES>();
    // ---- entries of G, 12 N dealt over the lanes
    bool lane_ok = true;
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) {
      const int e = lane + LANES * i;
      if (e < NU * N) {
        const int t = e / NU, col = e % NU;
        const double u = (double)sm.u[e];
        double ru = 0.0;
        if constexpr (full) {
#pragma unroll
          for (int j = 0; j < NU; ++j) ru += sm.W[NX * NX + NU * col + j] * (double)sm.u[NU * t + j];
        } else {
          ru = sm.r[col] * u;
        }
        ju += u * ru;
        const double g = 2.0 * cert_state_grad(sm.K, sm.G, minv, h, col, &sm.S[t][0][0]) + 2.0 * ru;
        gv[i] = (float)g;
        lane_ok = lane_ok && isfinite(gv[i]);
        sm.P[t][col][0] = g;   // the forward sums were last read before two syncs
      }
    }
    fsync<LANES>();
    // ---- the foot-step terms: 4 N <= 128, two per lane
    double gp = 0.0, wt = -INFINITY;
    const double fzmax = (double)rec[8], mu = (double)rec[7];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int k = lane + LANES * i;
      if (k < 4 * N) {
        const float ct = sm.in[IN_CONTACT + k];
        const bool stance = ct > 0.f;
        double ub = stance ? (double)ct * fzmax : 0.0, m;
        ub = ub > 0.0 ? ub : 0.0;
        const int t = k / 4, leg = k % 4;
        const double g[3] = {sm.P[t][3 * leg][0], sm.P[t][3 * leg + 1][0], sm.P[t][3 * leg + 2][0]};
        const double term = cert_foot_term(sm.frame, mu, ub, stance, g, sm.u + 3 * k, &m);
        gp += term;
        wt = term > wt ? term : wt;
      }
    }
    // ---- reduce across the wave
    objective = (predict_wave_sum(je) + predict_wave_sum(ju)) - predict_wave_sum(jf);
    gap = predict_wave_sum(gp);
    worst = predict_wave_max(wt);
    finite = !__any(!lane_ok) && isfinite(objective) && isfinite(gap) && isfinite(objective - gap) && isfinite(worst);
  }
  rollout_store<NU>(finite, N, b, lane, gv, Gg, objective, gap, objective - gap, worst, reportg, statusg);
}

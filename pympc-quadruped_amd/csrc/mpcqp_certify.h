// mpcqp_certify.h -- the optimality certificate on the device: for every robot in one launch the
// gradient G = H U + g of the QP's objective phi at a force sequence U, phi(U) itself, and the
// duality gap the friction pyramids give in closed form (included by mpcqp.hip inside its
// anonymous namespace, after mpcqp_predict.h).  The algebra is mpcqp_certify_robot.h; this file
// maps a wavefront's lanes onto it.
//
// One wavefront per robot, one robot per workgroup, as mpcqp_predict_kernel:
//   stage    as predict: form_stage's chunk loads and predict_stage_u
//   head     lanes 0..11 one column of K and G each, lanes 12..20 the nine entries of the cone
//            frame (t1, t2, n), lanes 32..44 n1 / n2 and the diagonal weights, every lane the
//            full weights if set
//   forward  lanes 0..11 the running sums P0 / P1 of their input column, into LDS
//   -- sync --
//   errors   the 13 N entries e_t dealt over the lanes; Q e_t goes to S[t][.][0] (through E and a
//            second pass with the full Q, as predict's cost), the costs J and J_free summed on
//            the way exactly as predict sums them
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

// Per-robot LDS: PredictShared's staged inputs, model head and forward sums, with the cone frame
// for the cone rows and the backward sums S added: 9 808 bytes at <16, false> (16 robots in a
// CU's 160 KiB), 27 008 at <32, true>.
template <int NM, bool FULL>
struct alignas(16) CertifyShared {
  static constexpr int IN_XREF = IN_CONTACT + 4 * NM, IN_END = IN_XREF + NX * NM;
  float in[IN_END];              // staged inputs, form_stage's layout (x0, feet, record, contact, xref)
  float u[NU * NM];              // staged U
  double K[3 * NU];              // inv(I_w)[r_leg]x, float32-rounded
  double G[3 * NU];              // R_z^T K
  double frame[10];              // t1, t2, n of the cone rows, [3][3]
  double n1[16], n2[16];         // Nm x0, Nm^2 x0
  double q[16], r[NU];           // diagonal weights
  double minv;                   // float32(1/m)
  double pad;
  double P[NM][NU][2];           // (P0_t, P1_t) per input column; after the errors P[t][c][0] is G's float64 entry
  double S[NM][NX][2];           // (Q e_t, then S0_t; S1_t) per state component
  double E[FULL ? NM : 1][NX][2];               // (e_t, e_t for U = 0): the full-Q pass reads them back
  double W[FULL ? NX * NX + NU * NU : 2];       // full Q then R (KParams::wfull)
};
static_assert(sizeof(CertifyShared<16, false>) == 9808 && sizeof(CertifyShared<16, true>) == 15424 &&
                  sizeof(CertifyShared<kMaxN, false>) == 18064 && sizeof(CertifyShared<kMaxN, true>) == 27008,
              "DESIGN.md 4.4j states the LDS sizes");

template <int NM, bool FULL>
__global__ __launch_bounds__(LANES) void mpcqp_certify_kernel(
    KParams P, int B, const float* __restrict__ x0g, const float* __restrict__ xrefg,
    const float* __restrict__ contactg, const float* __restrict__ feetg, const float* __restrict__ robotg,
    const float* __restrict__ Ug, float* __restrict__ Gg, double* __restrict__ reportg, int32_t* __restrict__ statusg) {
#pragma clang fp contract(off)   // as mpcqp_certify_robot.h: the host build differs in the wave sums' order alone
  constexpr int kPerLane = certify_per_lane(NM);
  constexpr int kErrPerLane = predict_per_lane(NM);
  using Shared = CertifyShared<NM, FULL>;
  __shared__ Shared sm;
  const int b = blockIdx.x;
  if (b >= B) return;
  const int lane = threadIdx.x;
  const int N = P.N;
  const double h = P.dt;
  constexpr bool full = FULL;
  // ---- stage: the six input slices; a refused robot computes nothing
  const bool bad_u = predict_stage_u(sm.u, Ug + (size_t)b * N * NU, NU * N, lane);
  const bool ok_in = form_stage<LANES>(sm, N, b, lane, x0g, xrefg, contactg, feetg, robotg);
  bool finite = ok_in && !__any(bad_u);   // wave-uniform
  fsync<LANES>();                         // the staged slices are read by other lanes below
  float gv[kPerLane];
#pragma unroll
  for (int i = 0; i < kPerLane; ++i) gv[i] = 0.f;
  double objective = 0.0, gap = 0.0, worst = 0.0;
  if (finite) {
    const float* const x0 = sm.in + IN_X0;
    const float* const rec = sm.in + IN_ROBOT;
    // ---- head
    double c, s;
    prd_yaw(x0, &c, &s);
    if (lane < NU) {
      double inv[9], k[3], g[3];
      prd_inertia_inv(c, s, rec, inv);
      prd_kg_column(c, s, inv, sm.in + IN_FEET, lane, k, g);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        sm.K[NU * a + lane] = k[a];
        sm.G[NU * a + lane] = g[a];
      }
      sm.r[lane] = P.r[lane];
    } else if (lane < NU + 9) {
      const int e = lane - NU;
      sm.frame[e] = cert_frame_entry(rec, e / 3, e % 3);
    } else if (lane >= 32 && lane < 32 + NX) {
      const int sc = lane - 32;
      sm.n1[sc] = prd_n1(x0, c, s, h, sc);
      sm.n2[sc] = prd_n2(x0, h, sc);
      sm.q[sc] = P.q[sc];
      if (sc == 0) sm.minv = prd_minv(rec);
    }
    if constexpr (full)
      for (int e = lane; e < NX * NX + NU * NU; e += LANES) sm.W[e] = P.wfull[e];
    // ---- forward scan: lanes 0..11, one input column each
    if (lane < NU) {
      double p0 = 0.0, p1 = 0.0;
      for (int t = 0; t < N; ++t) {
        prd_scan_step(&p0, &p1, sm.u[NU * t + lane]);
        sm.P[t][lane][0] = p0;
        sm.P[t][lane][1] = p1;
      }
    }
    fsync<LANES>();
    // ---- errors e_t and Q e_t, 13 N dealt over the lanes; the costs as predict takes them
    const double minv = sm.minv;
    double je = 0.0, jf = 0.0, ju = 0.0;
#pragma unroll
    for (int i = 0; i < kErrPerLane; ++i) {
      const int e = lane + LANES * i;
      if (e < NX * N) {
        const int t = e / NX, sc = e % NX;
        const double xref = (double)sm.in[Shared::IN_XREF + e];
        const double xf = prd_free_entry((double)x0[sc], sm.n1[sc], sm.n2[sc], t);
        const double x = xf + prd_forced_entry(sm.K, sm.G, minv, h, sc, &sm.P[t][0][0]);
        const double ee = x - xref, ef = xf - xref;
        if constexpr (full) {
          sm.E[t][sc][0] = ee;
          sm.E[t][sc][1] = ef;
        } else {
          const double qs = sm.q[sc];
          const double qe = qs * ee;
          sm.S[t][sc][0] = qe;
          je += qe * ee;
          jf += qs * ef * ef;
        }
      }
    }
    if constexpr (full) {
      fsync<LANES>();
      for (int e = lane; e < NX * N; e += LANES) {
        const int t = e / NX, sc = e % NX;
        double a = 0.0, af = 0.0;
#pragma unroll
        for (int j = 0; j < NX; ++j) {
          const double w = sm.W[NX * sc + j];
          a += w * sm.E[t][j][0];
          af += w * sm.E[t][j][1];
        }
        sm.S[t][sc][0] = a;
        je += sm.E[t][sc][0] * a;
        jf += sm.E[t][sc][1] * af;
      }
    }
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
  // ---- stores: a refused robot's G and report are zeros
  if (Gg != nullptr) {
    float* const Gb = Gg + (size_t)b * N * NU;
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) {
      const int e = lane + LANES * i;
      if (e < NU * N) Gb[e] = finite ? gv[i] : 0.f;
    }
  }
  if (lane < CERT_REPORT && reportg != nullptr) {
    const double v = lane == CERT_OBJECTIVE ? objective : lane == CERT_GAP ? gap : lane == CERT_LOWER ? objective - gap : worst;
    reportg[(size_t)b * CERT_REPORT + lane] = finite ? v : 0.0;
  }
  if (lane == 0 && statusg != nullptr) statusg[b] = finite ? MPCQP_STATUS_OK : MPCQP_STATUS_NONFINITE;
}

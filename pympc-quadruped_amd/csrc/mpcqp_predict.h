// mpcqp_predict.h -- the predicted trajectory on the device: for every robot in one launch the
// states x_1 .. x_N the QP believes a force sequence U produces (com_traj = Sx x0 + Su U,
// mpc.py:293-294), the tracking cost of U and of U = 0, the smallest cone slack and the largest
// swing-leg entry (included by mpcqp.hip inside its anonymous namespace, after mpcqp_terrain.h).
// The algebra is mpcqp_predict_robot.h; this file maps a wavefront's lanes onto it.
//
// One wavefront per robot, one robot per workgroup:
//   stage    form_stage's 16-byte chunk loads for x0, feet, record, contact, xref; U's 48 N bytes
//            the same way (predict_stage_u)
//   head     lanes 0..11 one column of K and G each (every one of them inverts I_w for itself: 60
//            flops against a pass through LDS), lanes 12..29 the 18 cone-row entries, lanes
//            32..44 n1 / n2 and the diagonal weights, every lane the full weights if set
//   scan     lanes 0..11 the two running sums of their input column over t <= N - 1, into LDS
//   -- one wave-level sync --
//   entries  the 13 N entries of X dealt over the lanes (entry e = lane + 64 i, i < 4 or 7), each kept
//            in a register until the robot's status is known; e_t and its U = 0 twin go to LDS
//            for the full-Q cost alone
//   report   per-lane partial sums of the cost, minimum of the slacks, maximum of the swing
//            entries, reduced across the wave with __shfl_xor; no atomics
// Stage, head, scan and the error part of the entries are the rollout_* functions below, written
// once for this kernel and mpcqp_certify_kernel (mpcqp_certify.h), with the store epilogue; what
// a kernel does with its cone lanes and with each entry it hands them as a lambda.
// The model is the head of form_model restated (mpcqp_predict_robot.h), not a call of it: a
// FormT<32> / FormY / RobotMetaT<32> instantiation carries the suffix sums, the Hessian blocks and
// the full-weight work of the solve, 32 KB of LDS before U and the scans are added where this
// kernel needs 20 in all, and form_model's bodies stay as they are.
// Four instantiations, <NM = 16 or 32, FULL>: the LDS of a launch is what its horizon and weights
// need, so that a CU holds 16 robots and more at N <= 16 with diagonal weights.
#include "mpcqp_predict_robot.h"

static_assert(PRD_NX == NX && PRD_NU == NU && PRD_MAX_N == kMaxN, "dimensions: mpcqp_device.h and mpcqp_predict_robot.h agree");
static_assert(PRD_REPORT == MPCQP_PREDICT_REPORT, "report stride");
static_assert(PRD_STATUS_OK == MPCQP_STATUS_OK && PRD_STATUS_NONFINITE == MPCQP_STATUS_NONFINITE, "status words");

// entries of X per lane: 4 at NM = 16, 7 at NM = 32
constexpr int predict_per_lane(int NM) { return (NX * NM + LANES - 1) / LANES; }

// Per-robot LDS of the rollout, what mpcqp_predict_kernel and mpcqp_certify_kernel both stage and
// compute, sized for horizons N <= NM (NM = 16 or 32, as the interior-point class sizes its own)
// and, FULL alone, for the full weights.  What a launch needs decides how many robots a CU holds
// at once.
template <int NM, bool FULL>
struct alignas(16) RolloutShared {
  static constexpr int IN_XREF = IN_CONTACT + 4 * NM, IN_END = IN_XREF + NX * NM;
  float in[IN_END];              // staged inputs, form_stage's layout (x0, feet, record, contact, xref)
  float u[NU * NM];              // staged U
  double K[3 * NU];              // inv(I_w)[r_leg]x, float32-rounded
  double G[3 * NU];              // R_z^T K
  double n1[16], n2[16];         // Nm x0, Nm^2 x0
  double q[16], r[NU];           // diagonal weights
  double minv;                   // float32(1/m)
  double pad;
  double P[NM][NU][2];           // (P0_t, P1_t) per input column
  double E[FULL ? NM : 1][NX][2];               // (e_t, e_t for U = 0): the full-Q pass reads them back
  double W[FULL ? NX * NX + NU * NU : 2];       // full Q then R (KParams::wfull)
};

// The rollout and the cone rows: 6 544 bytes at <16, false>, 20 416 at <32, true>.
template <int NM, bool FULL>
struct alignas(16) PredictShared : RolloutShared<NM, FULL> {
  double rows[18];               // one-sided cone rows, [6][3]
};
static_assert(sizeof(PredictShared<kMaxN, true>) == 20416 && sizeof(PredictShared<16, false>) == 6544,
              "DESIGN.md 4.4h states the LDS sizes");

// U's slice staged as form_stage stages the other five: the 16-byte-aligned chunks that cover
// it, a lane keeping the floats of its chunk that fall inside the slice (a chunk never crosses
// a page).  Returns whether this lane saw a non-finite entry.
__device__ __forceinline__ bool predict_stage_u(float* __restrict__ dst, const float* __restrict__ src, int len, int lane) {
  const uintptr_t a = (uintptr_t)src;
  const int nch = (int)(((a + 4 * (uintptr_t)len + 15) >> 4) - (a >> 4));
  bool bad = false;
  for (int c = lane; c < nch; c += LANES) {
    const uintptr_t base = (a & ~(uintptr_t)15) + 16 * (uintptr_t)c;
    const float4 v = *reinterpret_cast<const float4*>(base);
    const int e = (int)(((intptr_t)base - (intptr_t)a) >> 2);   // slice index of v.x (may be < 0)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float w = j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w;
      const int k = e + j;
      if (k >= 0 && k < len) {
        dst[k] = w;
        bad |= prd_bad_value(w, false);
      }
    }
  }
  return bad;
}

__device__ __forceinline__ double predict_wave_sum(double v) {
#pragma unroll
  for (int m = 1; m < LANES; m <<= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ double predict_wave_min(double v) {
#pragma unroll
  for (int m = 1; m < LANES; m <<= 1) {
    const double o = __shfl_xor(v, m);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ double predict_wave_max(double v) {
#pragma unroll
  for (int m = 1; m < LANES; m <<= 1) {
    const double o = __shfl_xor(v, m);
    v = o > v ? o : v;
  }
  return v;
}

// ---- the rollout both kernels run, each piece once.  sm: a PredictShared or a CertifyShared.

// stage: the six input slices.  Returns, wave-uniform, whether the robot is taken: a refused
// robot computes nothing.
template <class Shared>
__device__ __forceinline__ bool rollout_stage(Shared& sm, int N, int b, int lane, const float* __restrict__ x0g,
                                              const float* __restrict__ xrefg, const float* __restrict__ contactg,
                                              const float* __restrict__ feetg, const float* __restrict__ robotg,
                                              const float* __restrict__ Ug) {
  const bool bad_u = predict_stage_u(sm.u, Ug + (size_t)b * N * NU, NU * N, lane);
  const bool ok_in = form_stage<LANES>(sm, N, b, lane, x0g, xrefg, contactg, feetg, robotg);
  const bool finite = ok_in && !__any(bad_u);
  fsync<LANES>();   // the staged slices are read by other lanes below
  return finite;
}

// head and forward scan, to the sync after which every lane may read them.  Lanes 0..11 one column
// of K and G and, after it, that input column's running sums; lanes 12..12 + CONE - 1 are the
// caller's, cone(lane - 12), for its form of the cone (predict: the 18 row entries, certify: the
// 9 of the frame); lanes 32..44 n1 / n2 and the diagonal weights; every lane the full weights if
// set.  N and h are P's, read by the kernel ahead of the stage so that the loads are not waited
// for here.
template <bool FULL, int CONE, class Shared, class Cone>
__device__ __forceinline__ void rollout_head_scan(Shared& sm, const KParams& P, int N, double h, int lane,
                                                  Cone&& cone) {
#pragma clang fp contract(off)
  static_assert(NU + CONE <= 32, "the cone lanes end where the lanes of n1 / n2 begin");
  const float* const x0 = sm.in + IN_X0;
  const float* const rec = sm.in + IN_ROBOT;
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
  } else if (lane < NU + CONE) {
    cone(lane - NU);
  } else if (lane >= 32 && lane < 32 + NX) {
    const int sc = lane - 32;
    sm.n1[sc] = prd_n1(x0, c, s, h, sc);
    sm.n2[sc] = prd_n2(x0, h, sc);
    sm.q[sc] = P.q[sc];
    if (sc == 0) sm.minv = prd_minv(rec);
  }
  if constexpr (FULL)
    for (int e = lane; e < NX * NX + NU * NU; e += LANES) sm.W[e] = P.wfull[e];
  if (lane < NU) {
    double p0 = 0.0, p1 = 0.0;
    for (int t = 0; t < N; ++t) {
      prd_scan_step(&p0, &p1, sm.u[NU * t + lane]);
      sm.P[t][lane][0] = p0;
      sm.P[t][lane][1] = p1;
    }
  }
  fsync<LANES>();
}

// The 13 N error entries dealt over the lanes, entry e = lane + 64 i: x_{t+1}[sc] for U = 0 and for
// U, e_t and its U = 0 twin, and this lane's part of the two tracking costs added to *je and
// *jf.  The full weights go through E and a second pass over W.  The caller is handed
// state(i, x), x before its float32 rounding, and weighted(t, sc, (Q e_t)[sc]).
template <int NM, bool FULL, class Shared, class State, class Weighted>
__device__ __forceinline__ void rollout_errors(Shared& sm, int N, double h, int lane, double* je, double* jf,
                                               State&& state, Weighted&& weighted) {
#pragma clang fp contract(off)
  const float* const x0 = sm.in + IN_X0;
  const double minv = sm.minv;
#pragma unroll
  for (int i = 0; i < predict_per_lane(NM); ++i) {
    const int e = lane + LANES * i;
    if (e < NX * N) {
      const int t = e / NX, sc = e % NX;
      const double xref = (double)sm.in[Shared::IN_XREF + e];
      const double xf = prd_free_entry((double)x0[sc], sm.n1[sc], sm.n2[sc], t);
      const double x = xf + prd_forced_entry(sm.K, sm.G, minv, h, sc, &sm.P[t][0][0]);
      state(i, x);
      const double ee = x - xref, ef = xf - xref;
      if constexpr (FULL) {
        sm.E[t][sc][0] = ee;
        sm.E[t][sc][1] = ef;
      } else {
        const double qs = sm.q[sc];
        const double qe = qs * ee;
        weighted(t, sc, qe);
        *je += qe * ee;
        *jf += qs * ef * ef;
      }
    }
  }
  if constexpr (FULL) {
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
      weighted(t, sc, a);
      *je += sm.E[t][sc][0] * a;
      *jf += sm.E[t][sc][1] * af;
    }
  }
}

// The stores: the PER float32 entries a lane holds of the robot's WIDTH N (entry e = lane + 64 i),
// the four report words and the status; a refused robot's entries and report are zeros.
template <int WIDTH, int PER>
__device__ __forceinline__ void rollout_store(bool finite, int N, int b, int lane, const float (&v)[PER],
                                              float* __restrict__ outg, double r0, double r1, double r2, double r3,
                                              double* __restrict__ reportg, int32_t* __restrict__ statusg) {
  if (outg != nullptr) {
    float* const ob = outg + (size_t)b * N * WIDTH;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = lane + LANES * i;
      if (e < WIDTH * N) ob[e] = finite ? v[i] : 0.f;
    }
  }
  if (lane < 4 && reportg != nullptr) {
    const double w = lane == 0 ? r0 : lane == 1 ? r1 : lane == 2 ? r2 : r3;
    reportg[(size_t)b * 4 + lane] = finite ? w : 0.0;
  }
  if (lane == 0 && statusg != nullptr) statusg[b] = finite ? MPCQP_STATUS_OK : MPCQP_STATUS_NONFINITE;
}
static_assert(PRD_REPORT == 4 && PRD_COST == 0 && PRD_COST_FREE == 1 && PRD_MARGIN == 2 && PRD_SWING == 3,
              "rollout_store takes the report words in their order");

template <int NM, bool FULL>
__global__ __launch_bounds__(LANES) void mpcqp_predict_kernel(
    KParams P, int B, const float* __restrict__ x0g, const float* __restrict__ xrefg,
    const float* __restrict__ contactg, const float* __restrict__ feetg, const float* __restrict__ robotg,
    const float* __restrict__ Ug, float* __restrict__ Xg, double* __restrict__ reportg, int32_t* __restrict__ statusg) {
#pragma clang fp contract(off)   // as mpcqp_predict_robot.h: the host build differs in the wave sums' order alone
  constexpr int kPredictPerLane = predict_per_lane(NM);
  __shared__ PredictShared<NM, FULL> sm;
  const int b = blockIdx.x;
  if (b >= B) return;
  const int lane = threadIdx.x;
  const int N = P.N;
  const double h = P.dt;
  bool finite = rollout_stage(sm, N, b, lane, x0g, xrefg, contactg, feetg, robotg, Ug);
  float xv[kPredictPerLane];
#pragma unroll
  for (int i = 0; i < kPredictPerLane; ++i) xv[i] = 0.f;
  double cost = 0.0, cost_free = 0.0, margin = 0.0, swing = 0.0;
  if (finite) {
    const float* const rec = sm.in + IN_ROBOT;
    rollout_head_scan<FULL, 18>(sm, P, N, h, lane, [&](int e) { sm.rows[e] = prd_cone_entry(rec, e / 3, e % 3); });
    // ---- entries of X, each kept in a register until the robot's status is known
    bool lane_ok = true;
    double je = 0.0, jf = 0.0, ju = 0.0;
    rollout_errors<NM, FULL>(
        sm, N, h, lane, &je, &jf,
        [&](int i, double x) {
          xv[i] = (float)x;
          lane_ok = lane_ok && isfinite(xv[i]);
        },
        [](int, int, double) {});
    if constexpr (FULL) {
      for (int e = lane; e < NU * N; e += LANES) {
        const int t = e / NU, col = e % NU;
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < NU; ++j) a += sm.W[NX * NX + NU * col + j] * (double)sm.u[NU * t + j];
        ju += (double)sm.u[e] * a;
      }
    } else {
      for (int e = lane; e < NU * N; e += LANES) {
        const double u = (double)sm.u[e];
        ju += sm.r[e % NU] * u * u;
      }
    }
    // ---- the cone margin and the swing residual: 4 N <= 128 foot-steps, two per lane
    double mg = INFINITY, sw = 0.0;
    const double fzmax = (double)rec[8];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int k = lane + LANES * i;
      if (k < 4 * N) {
        const float ct = sm.in[IN_CONTACT + k];
        const float* const f = sm.u + 3 * k;
        if (ct > 0.f) {
          const double sl = prd_foot_slack(sm.rows, (double)ct * fzmax, f, &lane_ok);
          mg = sl < mg ? sl : mg;
        } else {
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            const double v = fabs((double)f[a]);
            sw = v > sw ? v : sw;
          }
        }
      }
    }
    // ---- reduce across the wave
    cost = predict_wave_sum(je) + predict_wave_sum(ju);
    cost_free = predict_wave_sum(jf);
    margin = predict_wave_min(mg);
    swing = predict_wave_max(sw);
    finite = !__any(!lane_ok) && isfinite(cost) && isfinite(cost_free);
  }
  rollout_store<NX>(finite, N, b, lane, xv, Xg, cost, cost_free, margin, swing, reportg, statusg);
}


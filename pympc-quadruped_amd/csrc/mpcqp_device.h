// mpcqp_device.h -- the device prelude every kernel header is built on (included by mpcqp.hip
// inside its anonymous namespace, after mpcqp_solve_plan.h and ahead of mpcqp_form.h): the
// dimensions and KParams, the stamp macros of the diagnostic build, lane / DPP helpers, wave
// min / max / argmin, the Newton reciprocal, the 16-byte LDS vector loads and stores.

constexpr int NX = 13;      // state dimension (mpc.py:26)
constexpr int NU = 12;      // input dimension (mpc.py:28)
constexpr int LANES = 64;
constexpr int kMaxN = MPCQP_MAX_HORIZON;   // the longest horizon mpcqp_create accepts (include/mpcqp.h)
static_assert(kMaxN >= kDenseN && 4 * kMaxN <= 2 * LANES, "stance lists cover 4 N <= 128 entries");
static_assert(MPCQP_WARM_BYTES == 4 * kMaxN, "warm-start memory: one byte per (stage, leg)");
// staged inputs (floats)
constexpr int IN_X0 = 0, IN_FEET = 13, IN_ROBOT = 25, IN_CONTACT = 44;   // + FormT<NM>::IN_XREF

typedef double d2 __attribute__((ext_vector_type(2)));
typedef double d4 __attribute__((ext_vector_type(4)));   // v_mfma_f64_16x16x4 accumulators (mpcqp_ipm.h)

struct KParams {
  int N;
  int max_iter;
  double dt;
  double q[NX];
  double r[NU];
  const double* wfull;   // device: full Q (13 x 13) then R (12 x 12), row-major; nullptr = diagonal q, r
  unsigned char* warm;   // device: per-robot warm-start memory (mpcqp_set_warm_start), or nullptr
  int warm_cap;          // robots with memory
};

// Diagnostic build only (-DMPCQP_STAMPS): per-phase s_memtime stamps and per-section
// cycle accumulators of the active-set loop, written to U (>= 32 floats per robot);
// the shipped kernel executes no stamp.
#ifdef MPCQP_STAMPS
#define STAMP(i)                                \
  do {                                          \
    __builtin_amdgcn_sched_barrier(0);          \
    stamps_[i] = __builtin_amdgcn_s_memtime();  \
    __builtin_amdgcn_sched_barrier(0);          \
  } while (0)
// sub-stamps of the first phase (stage, stance, model; slots 9..11 of the stamp buffer)
#define SUBSTAMP(i)                               \
  do {                                            \
    __builtin_amdgcn_sched_barrier(0);            \
    substamps_[i] = __builtin_amdgcn_s_memtime(); \
    __builtin_amdgcn_sched_barrier(0);            \
  } while (0)
// section accumulators live one per lane (lane k holds section k): a uniform
// compare, no runtime-indexed private array (that would go to scratch, and the
// next barrier's vmcnt wait would absorb the scratch latency)
#define SEC(k)                                                   \
  do {                                                           \
    __builtin_amdgcn_sched_barrier(0);                           \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();  \
    if (lane == seccur_) secacc_ += t_ - seclast_;               \
    seclast_ = t_;                                               \
    seccur_ = (k);                                               \
    __builtin_amdgcn_sched_barrier(0);                           \
  } while (0)
#define CNT(k) (secacc_ += (lane == (k)) ? 1ull : 0ull)
#ifndef MPCQP_SOLO_LDS
// stamps builds only (tools/solo_stamps.py): extra dynamic LDS per class-64 workgroup, so that one
// robot holds a CU alone -- each robot's solo latency against its four robots per CU
#define MPCQP_SOLO_LDS 0
#endif
constexpr unsigned kDiagLds = MPCQP_SOLO_LDS;
constexpr int kStampU64 = 256;   // stamp slots per robot (the stamps build's U buffer: 512 floats per robot)
static_assert(32 + 24 * 8 <= kStampU64, "eight waves' section accumulators");
#else
constexpr unsigned kDiagLds = 0;
#define CNT(k) \
  do {         \
  } while (0)
#define STAMP(i) \
  do {           \
  } while (0)
#define SUBSTAMP(i) \
  do {              \
  } while (0)
#define SEC(k) \
  do {         \
  } while (0)
#endif

__device__ __forceinline__ double f32r(double v) { return (double)(float)v; }

__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }

__device__ __forceinline__ double readlane_d(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// wave-uniform double kept in SGPRs (frees the VGPR pair a uniform VALU result
// would otherwise occupy for its whole live range)
__device__ __forceinline__ double sgpr_d(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readfirstlane((int)(b & 0xffffffffll));
  const int hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// Compile-time loop: f(std::integral_constant<int, I>{}) for I = 0..N-1 (register
// arrays indexed by I stay in registers).
template <typename F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
  const long long bits = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp((int)bits, (int)bits, CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(bits >> 32), (int)(bits >> 32), CTRL, 0xF, 0xF, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
constexpr int DPP_XOR1 = 0xB1;      // quad_perm [1,0,3,2]
constexpr int DPP_XOR2 = 0x4E;      // quad_perm [2,3,0,1]
constexpr int DPP_HMIRROR = 0x141;  // row_half_mirror: i <-> 7-i within 8 lanes
constexpr int DPP_MIRROR = 0x140;   // row_mirror: i <-> 15-i within 16 lanes

// v_min_f64 / v_max_f64 without the NaN canonicalisation fmin/fmax carry (no
// operand here is NaN: +inf marks "no candidate")
__device__ __forceinline__ double vmin(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ double vmax(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_m(double v) {   // rows outside ROWMASK keep v
  const long long bits = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp((int)bits, (int)bits, CTRL, ROWMASK, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(bits >> 32), (int)(bits >> 32), CTRL, ROWMASK, 0xF, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
constexpr int DPP_BCAST15 = 0x142;  // row_bcast:15 -- lane 15 of each row to the next row
constexpr int DPP_BCAST31 = 0x143;  // row_bcast:31 -- lane 31 to rows 2 and 3

// Cross-lane min / max over the wave: butterfly inside 16-lane rows, then the
// row_bcast chain leaves the result in lane 63
__device__ __forceinline__ double wave_min(double v) {
  v = vmin(v, dpp_d<DPP_XOR1>(v));
  v = vmin(v, dpp_d<DPP_XOR2>(v));
  v = vmin(v, dpp_d<DPP_HMIRROR>(v));
  v = vmin(v, dpp_d<DPP_MIRROR>(v));
  v = vmin(v, dpp_m<DPP_BCAST15, 0xA>(v));
  v = vmin(v, dpp_m<DPP_BCAST31, 0xC>(v));
  return readlane_d(v, 63);
}
__device__ __forceinline__ double wave_max_d(double v) {
  v = vmax(v, dpp_d<DPP_XOR1>(v));
  v = vmax(v, dpp_d<DPP_XOR2>(v));
  v = vmax(v, dpp_d<DPP_HMIRROR>(v));
  v = vmax(v, dpp_d<DPP_MIRROR>(v));
  v = vmax(v, dpp_m<DPP_BCAST15, 0xA>(v));
  v = vmax(v, dpp_m<DPP_BCAST31, 0xC>(v));
  return readlane_d(v, 63);
}

// 1/d: hardware reciprocal estimate refined by two Newton steps (~1 ulp; d is a
// normal, well-scaled pivot / curvature, never 0, inf or denormal here)
__device__ __forceinline__ double rcp_nr(double d) {
  double y = __builtin_amdgcn_rcp(d);
  double e = fma(-d, y, 1.0);
  y = fma(y, e, y);
  e = fma(-d, y, 1.0);
  return fma(y, e, y);
}
// a / b with one residual correction of the quotient
__device__ __forceinline__ double div_nr(double a, double b) {
  const double y = rcp_nr(b);
  const double q = a * y;
  return fma(fma(-b, q, a), y, q);
}

// 8 / 4 consecutive doubles starting at element 8k / 4k (16-B aligned LDS vectors)
__device__ __forceinline__ void ld8(double (&v)[8], const double* base, int k) {
  const d2* p = reinterpret_cast<const d2*>(base + 8 * k);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const d2 x = p[i];
    v[2 * i] = x[0];
    v[2 * i + 1] = x[1];
  }
}
__device__ __forceinline__ void st8(double* base, int k, const double (&v)[8]) {
  d2* p = reinterpret_cast<d2*>(base + 8 * k);
#pragma unroll
  for (int i = 0; i < 4; ++i) p[i] = d2{v[2 * i], v[2 * i + 1]};
}
// TW consecutive doubles starting at element TW k (TW even; 16-B aligned LDS vectors)
template <int TW>
__device__ __forceinline__ void ldt(double (&v)[TW], const double* base, int k) {
  const d2* p = reinterpret_cast<const d2*>(base + TW * k);
#pragma unroll
  for (int i = 0; i < TW / 2; ++i) {
    const d2 x = p[i];
    v[2 * i] = x[0];
    v[2 * i + 1] = x[1];
  }
}
template <int TW>
__device__ __forceinline__ void stt(double* base, int k, const double (&v)[TW]) {
  d2* p = reinterpret_cast<d2*>(base + TW * k);
#pragma unroll
  for (int i = 0; i < TW / 2; ++i) p[i] = d2{v[2 * i], v[2 * i + 1]};
}
// TW consecutive doubles starting at element TS k (TS >= TW: a padded tile-column stride)
template <int TW, int TS>
__device__ __forceinline__ void lds_t(double (&v)[TW], const double* base, int k) {
  const d2* p = reinterpret_cast<const d2*>(base + TS * k);
#pragma unroll
  for (int i = 0; i < TW / 2; ++i) {
    const d2 x = p[i];
    v[2 * i] = x[0];
    v[2 * i + 1] = x[1];
  }
}
// 4 consecutive doubles at p (16-B aligned)
__device__ __forceinline__ void ld4s(double (&v)[4], const double* p) {
  const d2 a = reinterpret_cast<const d2*>(p)[0], b = reinterpret_cast<const d2*>(p)[1];
  v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
}
__device__ __forceinline__ void st4s(double* p, const double (&v)[4]) {
  reinterpret_cast<d2*>(p)[0] = d2{v[0], v[1]};
  reinterpret_cast<d2*>(p)[1] = d2{v[2], v[3]};
}
__device__ __forceinline__ void ld4(double (&v)[4], const double* base, int k) {
  const d2* p = reinterpret_cast<const d2*>(base + 4 * k);
  const d2 a = p[0], b = p[1];
  v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
}
__device__ __forceinline__ void st4(double* base, int k, const double (&v)[4]) {
  d2* p = reinterpret_cast<d2*>(base + 4 * k);
  p[0] = d2{v[0], v[1]};
  p[1] = d2{v[2], v[3]};
}

// ---- wave argmin with an f32 pre-selection.  Round-to-nearest f64 -> f32 is
// monotone, so the f64 minimum's f32 image is the f32 minimum: a unique f32
// minimum IS the exact answer; f32 ties fall back to the f64 reduction.  The
// f32 reduction is one DPP-encoded v_min_f32 per stage.
// The six stages are one asm statement: each DPP read of the previous stage's VGPR needs
// two wait states (s_nop 1), and separate statements made hipcc pad every boundary again.
__device__ __forceinline__ float wave_min_f32(float v) {
  asm volatile(
      "s_nop 1\n\t"
      "v_min_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_min_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_min_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_min_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_min_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_min_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf"
      : "+v"(v));
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
// lowest lane holding the wave minimum of v (+inf = no candidate); vmin_out = that minimum
__device__ __forceinline__ int wave_argmin_d(double v, double& vmin_out) {
  const float f = (float)v;
  const float fm = wave_min_f32(f);
  const unsigned long long cand = __ballot(f == fm);
  int l;
  if (__popcll(cand) == 1) {
    l = uni(__builtin_ctzll(cand));
    vmin_out = readlane_d(v, l);
  } else if (fm == INFINITY && __ballot(v < INFINITY) == 0ull) {
    // no candidate in any lane (e.g. no active slot blocks the step): the common
    // all-+inf tie needs no f64 reduction
    l = 0;
    vmin_out = INFINITY;
  } else {
    const double vv = (f == fm) ? v : INFINITY;
    const double m = wave_min(vv);
    l = uni(__builtin_ctzll(__ballot(vv == m)));
    vmin_out = m;
  }
  return l;
}

// lowest lane holding the f32-rounded wave minimum of v; vmin_out = v in that lane.
// Not the exact f64 argmin on f32 ties -- for choices where any deterministic
// near-minimal lane will do (every wave computes the same lane).
__device__ __forceinline__ int wave_argmin_f32(double v, double& vmin_out) {
  const float f = (float)v;
  const float fm = wave_min_f32(f);
  const int l = uni(__builtin_ctzll(__ballot(f == fm)));
  vmin_out = readlane_d(v, l);
  return l;
}

// class 64's setup-priority table (solve_robot): one u64 per CU, indexed by XCC_ID and the
// CU / SH / SE fields of HW_ID (12 bits)
constexpr int kPrioTab = 4096;

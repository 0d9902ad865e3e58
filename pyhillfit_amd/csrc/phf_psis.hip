// phf_psis.hip — streaming PSIS-LOO: per data point, the exact M + 1 smallest log-likelihoods of all draws, the non-tail and lppd sums,
// and the Pareto-smoothed leave-one-out estimate with its k-hat (include/pyhillfit_amd.h, "PSIS-LOO"; DESIGN.md §3, "PSIS-LOO").
//
// PSIS-LOO (Vehtari, Simpson, Gelman, Yao & Gabry, JMLR 2024; r_eff = 1) needs, per point, the M = ceil(min(S/5, 3 sqrt S)) largest
// log importance ratios r = -l, i.e. the M smallest l, and the cutoff, the (M+1)-th smallest.  Nothing else of the draws matters
// individually: every other draw enters only through sum exp(-l) (the raw non-tail weights; PSIS's truncation never reaches them, see
// the reduce) and through sum exp(l) (lppd).
//
// Accumulate.  Mapping as WAIC's (phf_pointwise.hip): one lane = one chain, one wavefront = 64 chains of one problem and a block of
// kPtBlock of its points (wave-uniform).  Per (problem, point, chain) the workspace holds
//   fields  [Q][stride][kFields][C]: m_nt, s_nt  online log-sum-exp of -l over the draws NOT in the heap (every rejected or evicted
//                                                value lands here exactly once: an exact non-tail denominator with no "all minus tail"
//                                                cancellation)
//                                    m_all, s_all online log-sum-exp of +l over all draws (lppd)
//                                    fill, inserts heap fill count, heap insertions so far (fill-ups and evictions)
//   heap    [Q][stride][k][C]: a bounded max-heap of the k smallest l the chain has produced (slot 0 = root, children 2i+1, 2i+2)
//   thr     [Q][stride]: T, an upper bound on the point's final cutoff: the top of the 1/16-binade bucket that holds the (M+1)-th
//           smallest value of all heaps together (at least M + 1 held values lie at or below it; the cutoff over more draws can only
//           be lower).  A draw l >= T can never be in the tail and goes straight to the non-tail sum.  T is recomputed
//           (psis_threshold_kernel) after every 1024th row of the run up to row 8192, then after every 8192nd, at the same rows however
//           the calls cut them.
// The heap root and T stay in registers: the common draw (l >= min(root of a full heap, T)) touches no heap memory; an insertion
// sifts in HBM.  With k = M + 1 (the default whenever the workspace fits kExactBudget) every point is exact by construction, and T
// keeps the insertions near the global tail's own rate.
// Deterministic: no atomics, every accumulator is produced by one lane in row order and round-trips through HBM exactly, T changes
// only at fixed rows, so the result is bit-identical however the rows are cut into calls.
//
// Reduce, one workgroup per (problem, point) (a persistent grid of at most kReduceGroups workgroups):
//   1. exact radix select (8 passes of 8 bits) of the (M+1)-th smallest order-preserving 64-bit key among the C x k heap entries
//      (integer histograms in LDS: counts, order-independent);
//   2. the M + 1 smallest gathered into LDS (M + 1 <= kLdsTail) or the workgroup's HBM scratch, then a bitonic sort ascending;
//   3. exactness: a chain's dropped values are all >= its final heap root h_c, so the selection is exact unless a chain has a FULL
//      heap with h_c < cutoff; such a point is written NaN with determined = 0;
//   4. the unselected heap entries (and the cutoff itself) are folded into the chains' non-tail sums, chain by chain in a fixed order,
//      then merged by a fixed tree; the same for lppd;
//   5. the generalised Pareto fit of Zhang & Stephens (2009) on the device: lane g = grid point g sums log1p(-b_g x) over the tail in
//      ascending order; profile-likelihood weights; k-hat from the posterior-mean b; the weakly informative adjustment;
//   6. smoothing by rank, the cap at the largest raw ratio, truncation at S^(3/4) x the mean weight, and
//      [elpd_loo_i, lppd_i, k-hat_i, sigma-hat_i, determined_i].
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pyhillfit_amd.h"
#include "phf_host_checks.h"
#include "phf_point_block.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
static_assert(kWaves == kPtWaves, "the accumulate kernel is launched with the point-block mapping's workgroup");
constexpr int kFields = 6;              // m_nt, s_nt, m_all, s_all, fill, inserts
constexpr int kOut = 5;                 // elpd_loo, lppd, k-hat, sigma-hat, determined
constexpr int kLdsTail = 8192;          // tail entries (M + 1) the reduce keeps in LDS; beyond, the HBM scratch
constexpr int64_t kMaxTail = (1 << 20) - 1;   // the longest tail M accepted
constexpr int kMaxGrid = 30 + 1024;     // Zhang-Stephens grid points: 30 + floor(sqrt(M)) <= 30 + 1023
constexpr int kReduceGroups = 256;      // workgroups of the reduce's persistent grid (each owns one HBM scratch slot)
constexpr double kEps = 2.220446049250313e-16;
constexpr int64_t kThresholdRows = 1024;                  // T is recomputed after every 1024th row up to row 8192, then every 8192nd
constexpr int64_t kThresholdRowsLate = 8192;
constexpr double kExactBudget = 32.0 * 1024 * 1024 * 1024;  // default: k = M + 1 while the workspace stays within 32 GiB

int64_t tail_length_of(int64_t S) {
  const double s = (double)S;
  const double a = s / 5.0, b = 3.0 * __builtin_sqrt(s);
  return (int64_t)__builtin_ceil(a < b ? a : b);
}

int64_t pow2_at_least(int64_t n) {
  int64_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

struct Layout {
  int64_t M;          // tail length
  int k;              // heap capacity per chain
  bool hbm;           // M + 1 > kLdsTail: the reduce sorts in HBM scratch
  int64_t p2;         // pow2 >= M + 1 (the sort's length)
  int groups;         // reduce workgroups
  size_t fields, thr, heap, scratch;   // doubles of each region
  size_t bytes() const { return (fields + thr + heap + scratch) * sizeof(double); }
};

struct PsisArgs {
  phf_pointwise_points pts;
  const double* rows;             // [nr][Q][stride_cols][C]
  int64_t nr, first_row, total_rows;
  int32_t Q, stride_cols, C, ne;
  int32_t ncg, npb;               // 64-chain groups, point blocks
  int32_t units;
  int32_t k;                      // heap capacity per chain
  int32_t M;                      // tail length
  int32_t p2;                     // the sort's length (HBM path)
  double* fields;                 // [Q][ps][kFields][C]
  double* thr;                    // [Q][ps]
  double* heap;                   // [Q][ps][k][C]
  double* scratch;                // [groups][2][p2] (HBM path)
  double* out;                    // reduce: [kOut][Q][ps]
  double* tail_out;               // reduce, optional: [Q][ps][M + 1]
};

// online log-sum-exp: x into (m, s) with s = sum exp(. - m); -inf adds nothing (NaN is never produced by the likelihoods)
__device__ inline void lse_add(double x, double& m, double& s, phf_ktab k_exp) {
  if (!(x > -PHF_INF)) return;
  const double d = x - m;                                          // +inf while m = -inf: then e = 0, s = 1
  const bool up = d > 0.0;
  const double e = phf_exp_fast_k(-__builtin_fabs(d), k_exp);
  s = up ? phf_fma(s, e, 1.0) : s + e;
  m = up ? x : m;
}

// one draw l of one chain at one point: the heap (base H, slot stride C) of capacity K with fill f and root h in registers
__device__ inline void psis_take(double l, double T, double& h, int& f, double& m_nt, double& s_nt, double& ins, double* H, size_t C,
                                 int K, phf_ktab k_exp) {
  if (!(l < T)) {                                                  // at or above the bound on the cutoff: never in the tail
    lse_add(-l, m_nt, s_nt, k_exp);
  } else if (f < K) {                                                     // filling: sift up from slot f
    int i = f;
    while (i > 0) {
      const int parent = (i - 1) >> 1;
      const double pv = H[(size_t)parent * C];
      if (!(pv < l)) break;
      H[(size_t)i * C] = pv;
      i = parent;
    }
    H[(size_t)i * C] = l;
    h = f == 0 ? l : (l > h ? l : h);
    ++f;
    ins += 1.0;
  } else if (l < h) {                                              // evict the root into the non-tail sum, sift l down
    lse_add(-h, m_nt, s_nt, k_exp);
    int i = 0;
    double root = l;
    for (;;) {
      const int c1 = 2 * i + 1;
      if (c1 >= K) break;
      const double v1 = H[(size_t)c1 * C];
      const double v2 = c1 + 1 < K ? H[(size_t)(c1 + 1) * C] : -PHF_INF;
      const bool right = v2 > v1;
      const double vb = right ? v2 : v1;
      if (!(vb > l)) break;
      H[(size_t)i * C] = vb;
      if (i == 0) root = vb;
      i = right ? c1 + 1 : c1;
    }
    H[(size_t)i * C] = l;
    h = root;
    ins += 1.0;
  } else {
    lse_add(-l, m_nt, s_nt, k_exp);
  }
}

template <int LIK>
__global__ __launch_bounds__(kThreads) void psis_accumulate_kernel(const PsisArgs a) {
  PHF_MATH_TABLES_TO_LDS();
  if (LIK == kGiven) { } else if (LIK == kHierarchical) PHF_ERFC_TABLE_TO_LDS(); else PHF_LOGPHI_TABLE_TO_LDS();
  phf_point_block b;
  if (!phf_point_block_open<LIK>(a, b)) return;
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  const size_t C = (size_t)a.C;
  const int K = a.k;
  const bool fresh = a.first_row == 0;
  double h[kPtBlock], thr[kPtBlock], m_nt[kPtBlock], s_nt[kPtBlock], m_all[kPtBlock], s_all[kPtBlock], ins[kPtBlock];
  int f[kPtBlock];
  const size_t at0 = (size_t)b.q * a.pts.stride + b.p0;
  double* st = a.fields + at0 * kFields * C + b.c;
  double* hp = a.heap + at0 * K * C + b.c;
#pragma unroll
  for (int j = 0; j < kPtBlock; ++j) {
    const double* sj = st + (size_t)j * kFields * C;
    const bool load = !fresh && j < b.np;
    thr[j] = load ? a.thr[at0 + j] : PHF_INF;
    m_nt[j] = load ? sj[0] : -PHF_INF;
    s_nt[j] = load ? sj[C] : 0.0;
    m_all[j] = load ? sj[2 * C] : -PHF_INF;
    s_all[j] = load ? sj[3 * C] : 0.0;
    f[j] = load ? (int)sj[4 * C] : 0;
    ins[j] = load ? sj[5 * C] : 0.0;
    h[j] = f[j] > 0 ? hp[(size_t)j * K * C] : -PHF_INF;
  }
  for (int64_t r = 0; r < a.nr; ++r)
    phf_point_block_row<LIK>(a, b, b.xr + (size_t)r * b.rstep, k_exp, k_log, [&](int j, double l) {
      lse_add(l, m_all[j], s_all[j], k_exp);
      psis_take(l, thr[j], h[j], f[j], m_nt[j], s_nt[j], ins[j], hp + (size_t)j * K * C, C, K, k_exp);
    });
#pragma unroll
  for (int j = 0; j < kPtBlock; ++j)
    if (j < b.np) {
      double* sj = st + (size_t)j * kFields * C;
      sj[0] = m_nt[j]; sj[C] = s_nt[j]; sj[2 * C] = m_all[j]; sj[3 * C] = s_all[j]; sj[4 * C] = (double)f[j]; sj[5 * C] = ins[j];
    }
}

// order-preserving key: a < b (doubles, -0 == +0) <=> key(a) < key(b) (unsigned)
__device__ inline uint64_t key_of(double v) {
  const uint64_t u = __double_as_longlong(v + 0.0);                // -0 -> +0
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ inline double value_of(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

__global__ __launch_bounds__(kThreads) void psis_init_thr_kernel(double* thr, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) thr[i] = PHF_INF;
}

// T of one (problem, point) per workgroup: an upper bound on the (M+1)-th smallest value held in all heaps together, the top edge of
// its bucket of the order-preserving key's upper 16 bits (two radix passes, integer LDS histograms: 1/16 of a binade wide).  At least
// M + 1 held values lie at or below T, and later draws can only lower the cutoff, so a draw >= T is never in the tail.  T only decreases.
__global__ __launch_bounds__(kThreads) void psis_threshold_kernel(const PsisArgs a) {
  __shared__ uint32_t hist[256];
  __shared__ uint64_t s_prefix;
  __shared__ uint32_t s_rank, s_maxfill;
  __shared__ unsigned long long s_held;
  const int64_t unit = blockIdx.x;
  const int tid = threadIdx.x;
  const int ps = a.pts.stride;
  const int q = (int)(unit / ps), p = (int)(unit % ps);
  if (p >= clamp_count(a.pts.count[q], ps)) return;
  const size_t C = (size_t)a.C;
  const double* F = a.fields + (size_t)unit * kFields * C;
  const double* H = a.heap + (size_t)unit * a.k * C;
  if (tid == 0) { s_maxfill = 0; s_held = 0; s_prefix = 0; s_rank = (uint32_t)a.M; }
  __syncthreads();
  uint32_t mf = 0;
  unsigned long long held = 0;
  for (int c = tid; c < a.C; c += kThreads) {
    const uint32_t f = (uint32_t)F[4 * C + c];
    mf = f > mf ? f : mf;
    held += f;
  }
  atomicMax(&s_maxfill, mf);
  atomicAdd(&s_held, held);
  __syncthreads();
  if (s_held < (unsigned long long)a.M + 1) return;                // fewer than M + 1 held values: no bound yet (uniform)
  const int64_t entries = (int64_t)s_maxfill * a.C;
  uint64_t mask = 0;
  for (int shift = 56; shift >= 48; shift -= 8) {
    for (int b = tid; b < 256; b += kThreads) hist[b] = 0;
    __syncthreads();
    const uint64_t prefix = s_prefix;
    for (int64_t i = tid; i < entries; i += kThreads) {
      const int64_t slot = i / a.C, c = i - slot * a.C;
      if (slot < (int64_t)F[4 * C + c]) {
        const uint64_t key = key_of(H[i]);
        if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1u);
      }
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t cum = 0;
      for (int b = 0; b < 256; ++b) {
        if (s_rank < cum + hist[b]) { s_rank -= cum; s_prefix = prefix | ((uint64_t)b << shift); break; }
        cum += hist[b];
      }
    }
    mask |= 0xffull << shift;
    __syncthreads();
  }
  if (tid == 0) {
    const double t = value_of(s_prefix | 0x0000ffffffffffffull);   // the bucket's largest key
    if (t < a.thr[unit]) a.thr[unit] = t;
  }
}

// ---- reduce ----------------------------------------------------------------------------------------------------------------------

__device__ inline void lse_merge(double& m, double& s, double m2, double s2) {
  if (s2 == 0.0) return;
  if (s == 0.0) { m = m2; s = s2; return; }
  const double mx = m > m2 ? m : m2;
  s = s * exp(m - mx) + s2 * exp(m2 - mx);
  m = mx;
}

struct ReduceShared {
  double red_a[kThreads], red_b[kThreads];
  double b[kMaxGrid], l[kMaxGrid], w[kMaxGrid];
  uint32_t hist[256];
  uint32_t maxfill;
  uint64_t prefix;
  int32_t rank, count_less, count_eq;
  double scalar;                  // the first quartile, then the posterior-mean b
};

// sum over the workgroup of each thread's v, by a fixed tree (thread 0 returns the total; all threads get it)
__device__ double block_sum(double v, ReduceShared& sh) {
  __syncthreads();
  sh.red_a[threadIdx.x] = v;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh.red_a[threadIdx.x] += sh.red_a[threadIdx.x + o];
    __syncthreads();
  }
  const double r = sh.red_a[0];
  __syncthreads();
  return r;
}

__device__ void block_lse(double& m, double& s, ReduceShared& sh) {
  __syncthreads();
  sh.red_a[threadIdx.x] = m;
  sh.red_b[threadIdx.x] = s;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      double mm = sh.red_a[threadIdx.x], ss = sh.red_b[threadIdx.x];
      lse_merge(mm, ss, sh.red_a[threadIdx.x + o], sh.red_b[threadIdx.x + o]);
      sh.red_a[threadIdx.x] = mm;
      sh.red_b[threadIdx.x] = ss;
    }
    __syncthreads();
  }
  m = sh.red_a[0];
  s = sh.red_b[0];
  __syncthreads();
}

// GPD quantile at probability p, shape k, scale sigma
__device__ inline double gpd_quantile(double p, double k, double sigma) {
  const double t = log1p(-p);
  return k == 0.0 ? -sigma * t : sigma * expm1(-k * t) / k;
}

// one (problem, point): the tail buffers T (sorted keys, then the tail values) and X (exceedances) hold p2 >= M + 1 entries
__device__ void psis_reduce_unit(const PsisArgs& a, int64_t unit, uint64_t* T, double* X, ReduceShared& sh) {
  const int tid = threadIdx.x;
  const int ps = a.pts.stride;
  const int q = (int)(unit / ps), p = (int)(unit % ps);
  const size_t C = (size_t)a.C;
  const size_t plane = (size_t)a.Q * ps;
  const int M = a.M, K = a.k;
  const double S = (double)a.total_rows * (double)a.C;
  if (p >= clamp_count(a.pts.count[q], ps)) {
    if (tid < kOut) a.out[tid * plane + unit] = tid == kOut - 1 ? 0.0 : PHF_NAN;
    return;
  }
  const double* F = a.fields + (size_t)unit * kFields * C;
  const double* H = a.heap + (size_t)unit * K * C;
  // entry i = slot i / C of chain i % C, up to the largest fill (with the bound T the heaps mostly stay far from full)
  if (tid == 0) sh.maxfill = 0;
  __syncthreads();
  uint32_t mf = 0;
  for (int c = tid; c < a.C; c += kThreads) mf = (uint32_t)F[4 * C + c] > mf ? (uint32_t)F[4 * C + c] : mf;
  atomicMax(&sh.maxfill, mf);
  __syncthreads();
  const int64_t entries = (int64_t)sh.maxfill * a.C;

  // 1. radix select of the key of rank M (0-based) among the valid heap entries
  if (tid == 0) { sh.prefix = 0; sh.rank = M; }
  uint64_t mask = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    for (int b = tid; b < 256; b += kThreads) sh.hist[b] = 0;
    __syncthreads();
    const uint64_t prefix = sh.prefix;
    for (int64_t i = tid; i < entries; i += kThreads) {
      const int64_t slot = i / a.C, c = i - slot * a.C;
      if (slot < (int64_t)F[4 * C + c]) {
        const uint64_t key = key_of(H[i]);
        if ((key & mask) == prefix) atomicAdd(&sh.hist[(key >> shift) & 255], 1u);
      }
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t cum = 0;
      const uint32_t rank = (uint32_t)sh.rank;
      for (int b = 0; b < 256; ++b) {
        if (rank < cum + sh.hist[b]) {
          sh.rank = (int32_t)(rank - cum);
          sh.prefix = prefix | ((uint64_t)b << shift);
          break;
        }
        cum += sh.hist[b];
      }
    }
    mask |= 0xffull << shift;
    __syncthreads();
  }
  const uint64_t kstar = sh.prefix;
  const int need_eq = sh.rank + 1;                                 // copies of kstar among the M + 1 selected
  const int less = M + 1 - need_eq;

  // 2. gather: every key < kstar, then need_eq copies of kstar; exactness check on the full heaps' roots
  if (tid == 0) { sh.count_less = 0; sh.count_eq = 0; }
  __syncthreads();
  int bad = 0;
  for (int64_t i = tid; i < entries; i += kThreads) {
    const int64_t slot = i / a.C, c = i - slot * a.C;
    const int fill = (int)F[4 * C + c];
    if (slot < fill) {
      const uint64_t key = key_of(H[i]);
      if (key < kstar) T[atomicAdd(&sh.count_less, 1)] = key;      // positions vary, the sort below fixes the order
      else if (key == kstar) atomicAdd(&sh.count_eq, 1);
      if (slot == 0 && fill == K && a.total_rows > K && key < kstar) bad = 1;   // a full heap that dropped draws, root below the cutoff
    }
  }
  const int undetermined = __syncthreads_or(bad);
  const int n_eq = sh.count_eq;
  for (int64_t j = less + tid; j < a.p2; j += kThreads) T[j] = j <= M ? kstar : ~0ull;
  __syncthreads();

  // 3. bitonic sort of T[0, p2) ascending (p2 = the power of two >= M + 1 this buffer was padded to)
  const int64_t n2 = a.p2;
  for (int64_t size = 2; size <= n2; size <<= 1)
    for (int64_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (int64_t i = tid; i < n2 / 2; i += kThreads) {
        const int64_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool asc = (lo & size) == 0;
        const uint64_t u = T[lo], v = T[hi];
        if ((u > v) == asc) { T[lo] = v; T[hi] = u; }
      }
      __syncthreads();
    }
  const double t0 = value_of(T[0]), tM = value_of(T[M]);
  if (a.tail_out)
    for (int j = tid; j <= M; j += kThreads) a.tail_out[(size_t)unit * (M + 1) + j] = value_of(T[j]);

  // 4. lppd and the non-tail sum, chain by chain in a fixed order, then a fixed tree
  double m_all = -PHF_INF, s_all = 0.0, m_nt = -PHF_INF, s_nt = 0.0;
  for (int64_t c = tid; c < a.C; c += kThreads) {
    lse_merge(m_all, s_all, F[2 * C + c], F[3 * C + c]);
    double mc = F[c], sc = F[C + c];
    const int fill = (int)F[4 * C + c];
    for (int slot = 0; slot < fill; ++slot) {
      const double v = H[(size_t)slot * C + c];
      if (key_of(v) > kstar) lse_merge(mc, sc, -v, 1.0);
    }
    lse_merge(m_nt, s_nt, mc, sc);
  }
  block_lse(m_all, s_all, sh);
  block_lse(m_nt, s_nt, sh);
  lse_merge(m_nt, s_nt, -tM, (double)(n_eq - need_eq + 1));       // the unselected copies of the cutoff, and the cutoff itself
  const double lppd = (m_all + log(s_all)) - log(S);

  double elpd = PHF_NAN, khat = PHF_NAN, sigma = PHF_NAN;
  if (undetermined) {
    if (tid == 0) {
      for (int o = 0; o < kOut - 1; ++o) a.out[o * plane + unit] = PHF_NAN;
      a.out[(kOut - 1) * plane + unit] = 0.0;
    }
    return;
  }
  if (t0 == -PHF_INF) {                                            // some draw has p(y_i | theta) = 0: its ratio is infinite
    if (tid == 0) {
      a.out[unit] = -PHF_INF; a.out[plane + unit] = lppd; a.out[2 * plane + unit] = PHF_INF; a.out[3 * plane + unit] = PHF_NAN;
      a.out[4 * plane + unit] = 1.0;
    }
    return;
  }

  // 5. the tail as values (T, in place) and shifted raw weights: W_j = exp(t0 - t_j) <= 1, W_cut = exp(t0 - tM); exceedances X_j
  //    = W_j - W_cut, descending in j (j = 0: the largest ratio)
  const double wcut = exp(t0 - tM);
  double* TV = reinterpret_cast<double*>(T);
  for (int j = tid; j < M; j += kThreads) {
    const double t = value_of(T[j]);
    TV[j] = t;
    X[j] = exp(t0 - t) - wcut;
  }
  __syncthreads();
  const bool fit = M >= 5 && X[0] > X[M - 1];
  if (fit) {
    const int mg = 30 + (int)__builtin_sqrt((double)M);
    if (tid == 0) {
      double xs = X[M - (int)(M / 4.0 + 0.5)];                     // first quartile: ascending index floor(M/4 + 1/2) - 1
      for (int j = M - 1; xs == 0.0 && j >= 0; --j) xs = X[j];    // over a quarter ties with the cutoff: the smallest positive one
      sh.scalar = xs;
    }
    __syncthreads();
    const double inv_max = 1.0 / X[0], xs3 = 3.0 * sh.scalar;
    for (int g = tid; g < mg; g += kThreads) {
      const double b = inv_max + (1.0 - __builtin_sqrt((double)mg / (g + 0.5))) / xs3;
      double acc = 0.0;
      for (int j = M - 1; j >= 0; --j) acc += log1p(-b * X[j]);   // ascending x
      const double kk = acc / M;
      sh.b[g] = b;
      sh.l[g] = M * (log(-b / kk) - kk - 1.0);
    }
    __syncthreads();
    for (int g = tid; g < mg; g += kThreads) {
      double acc = 0.0;
      for (int h2 = 0; h2 < mg; ++h2) acc += exp(sh.l[h2] - sh.l[g]);
      sh.w[g] = 1.0 / acc;
    }
    __syncthreads();
    if (tid == 0) {
      double wsum = 0.0;
      for (int g = 0; g < mg; ++g) wsum += sh.w[g] >= 10.0 * kEps ? sh.w[g] : 0.0;
      double bpost = 0.0;
      for (int g = 0; g < mg; ++g) bpost += sh.w[g] >= 10.0 * kEps ? sh.b[g] * (sh.w[g] / wsum) : 0.0;
      sh.scalar = bpost;
    }
    __syncthreads();
    const double bpost = sh.scalar;
    double part = 0.0;
    for (int j = tid; j < M; j += kThreads) part += log1p(-bpost * X[j]);
    const double kraw = block_sum(part, sh) / M;
    sigma = -kraw / bpost;
    khat = (M * kraw + 10.0 * 0.5) / (M + 10.0);
    // smoothing: the j-th largest ratio (ascending rank M - 1 - j) takes the GPD quantile at (M - j - 1/2)/M, capped at 1
    for (int j = tid; j < M; j += kThreads) {
      const double wq = wcut + gpd_quantile((M - j - 0.5) / M, khat, sigma);
      X[j] = wq < 1.0 ? wq : 1.0;
    }
  } else {
    khat = M < 5 ? PHF_INF : 0.0;                                  // too short a tail to fit; an equal tail has nothing to smooth
    sigma = M < 5 ? PHF_NAN : 0.0;
    for (int j = tid; j < M; j += kThreads) X[j] = exp(t0 - TV[j]);
  }
  __syncthreads();

  // 6. truncation at S^(3/4) x the mean weight (never reaches the non-tail weights, all <= W_cut: DESIGN.md), then elpd_loo
  const double w_nt = s_nt * exp(m_nt + t0);
  double part = 0.0;
  for (int j = tid; j < M; j += kThreads) part += X[j];
  const double den0 = w_nt + block_sum(part, sh);
  const double cap = exp(0.75 * log(S)) * (den0 / S);
  double pw = 0.0, pn = 0.0;
  for (int j = tid; j < M; j += kThreads) {
    const double w = X[j] < cap ? X[j] : cap;
    pw += w;
    pn += exp(log(w) + (TV[j] - t0));                              // w_j exp(l_j), in units of exp(t0)
  }
  const double den = w_nt + block_sum(pw, sh);
  const double num = (S - M) + block_sum(pn, sh);                  // a raw non-tail weight times exp(l) is exp(t0) exactly
  elpd = (t0 + log(num)) - log(den);
  if (tid == 0) {
    a.out[unit] = elpd; a.out[plane + unit] = lppd; a.out[2 * plane + unit] = khat; a.out[3 * plane + unit] = sigma;
    a.out[4 * plane + unit] = 1.0;
  }
  __syncthreads();
}

template <bool HBM>
__global__ __launch_bounds__(kThreads) void psis_reduce_kernel(const PsisArgs a) {
  __shared__ ReduceShared sh;
  __shared__ uint64_t lds_t[HBM ? 1 : kLdsTail];
  __shared__ double lds_x[HBM ? 1 : kLdsTail];
  uint64_t* T = HBM ? reinterpret_cast<uint64_t*>(a.scratch + (size_t)blockIdx.x * 2 * a.p2) : lds_t;
  double* X = HBM ? a.scratch + (size_t)blockIdx.x * 2 * a.p2 + a.p2 : lds_x;
  const int64_t units = (int64_t)a.Q * a.pts.stride;
  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    psis_reduce_unit(a, unit, T, X, sh);
    __syncthreads();
  }
}

// the rows after which T is recomputed: fixed, so the launches are cut at the same rows however the calls cut the run
int64_t next_threshold_row(int64_t r) {
  const int64_t b = r < kThresholdRowsLate ? kThresholdRows : kThresholdRowsLate;
  return (r / b + 1) * b;
}

// validate a shape and lay out its workspace; PHF_OK or PHF_ERR_INVALID_ARGUMENT with the reason
int layout_of(const char* who, int num_problems, int stride, int num_chains, int64_t total_rows, int tail_per_chain, Layout* L) {
  int rc = phf_check_positive(who, "num_problems, stride and num_chains", {num_problems, stride, num_chains});
  if (rc != PHF_OK) return rc;
  if (total_rows < 1 || (double)total_rows * num_chains < 2.0)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: total_rows must be positive and total_rows x num_chains at least 2 (got %lld x %d)", who,
                     (long long)total_rows, num_chains);
  if (tail_per_chain < 0) return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: tail_per_chain must be >= 0 (0: the default rule)", who);
  const double S = (double)total_rows * num_chains;
  if (S > 0x1p52) return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: total_rows x num_chains too large", who);
  const int64_t M = tail_length_of((int64_t)S);
  if (M > kMaxTail)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: the tail length M = %lld exceeds %lld (fewer draws per point)", who, (long long)M,
                     (long long)kMaxTail);
  const int64_t pts = (int64_t)num_problems * stride;
  const int64_t whole = M + 1 < total_rows ? M + 1 : total_rows;   // a chain never needs more: all of its draws, or the whole tail
  const bool hbm = M + 1 > kLdsTail;
  const int64_t p2 = pow2_at_least(M + 1);
  const int groups = (int)(pts < kReduceGroups ? pts : kReduceGroups);
  const double scratch = hbm ? (double)groups * 2 * p2 : 0.0;
  const double exact_bytes = ((double)pts * (kFields + whole) * num_chains + pts + scratch) * sizeof(double);
  const int64_t dflt = exact_bytes <= kExactBudget ? whole : 2 * ((M + 1 + num_chains - 1) / num_chains) + 32;
  int64_t k = tail_per_chain == 0 ? dflt : tail_per_chain;
  if (k > whole) k = whole;
  const int64_t held = (k < total_rows ? k : total_rows) * (int64_t)num_chains;
  if (held < M + 1)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: tail_per_chain %lld x %d chains holds fewer than the M + 1 = %lld smallest values", who,
                     (long long)k, num_chains, (long long)(M + 1));
  const double units = (double)num_problems * ((num_chains + 63) / 64) * ((stride + kPtBlock - 1) / kPtBlock);
  if ((rc = phf_check_grid(who, {units, (double)num_problems * stride, (double)k * num_chains})) != PHF_OK) return rc;
  L->M = M;
  L->k = (int)k;
  L->hbm = hbm;
  L->p2 = p2;
  L->groups = groups;
  L->fields = (size_t)pts * kFields * num_chains;
  L->thr = (size_t)pts;
  L->heap = (size_t)pts * k * num_chains;
  L->scratch = L->hbm ? (size_t)L->groups * 2 * L->p2 : 0;
  return PHF_OK;
}

}  // namespace

extern "C" int64_t phf_psis_tail_length(int num_chains, int64_t total_rows) {
  Layout L;
  if (layout_of("phf_psis_tail_length", 1, 1, num_chains, total_rows, 0, &L) != PHF_OK) return 0;
  return L.M;
}

extern "C" int phf_psis_tail_per_chain(int num_problems, int stride, int num_chains, int64_t total_rows, int tail_per_chain) {
  Layout L;
  if (layout_of("phf_psis_tail_per_chain", num_problems, stride, num_chains, total_rows, tail_per_chain, &L) != PHF_OK) return 0;
  return L.k;
}

extern "C" size_t phf_psis_workspace_bytes(int num_problems, int stride, int num_chains, int64_t total_rows, int tail_per_chain) {
  Layout L;
  if (layout_of("phf_psis_workspace_bytes", num_problems, stride, num_chains, total_rows, tail_per_chain, &L) != PHF_OK) return 0;
  return L.bytes();
}

extern "C" int phf_psis_init(int num_problems, int stride, int num_chains, int64_t total_rows, int tail_per_chain, double* workspace,
                             size_t workspace_bytes, void* stream) {
  static const char* who = "phf_psis_init";
  Layout L;
  int rc = layout_of(who, num_problems, stride, num_chains, total_rows, tail_per_chain, &L);
  if (rc != PHF_OK) return rc;
  // the fields (fill counts) and T = +inf: a heap slot is read only once written
  if ((rc = phf_init_workspace(who, "psis", workspace, workspace_bytes, L.bytes(), L.fields * sizeof(double), stream)) != PHF_OK) return rc;
  hipLaunchKernelGGL(psis_init_thr_kernel, dim3(blocks_for((int64_t)L.thr, kThreads)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     workspace + L.fields, (int64_t)L.thr);
  return phf_check_launch("psis_init_thr_kernel");
}

namespace {

// phf_psis_accumulate and phf_psis_accumulate_given (likelihood == kGiven): one validation, one launch loop
int psis_accumulate(const char* who, const phf_pointwise_points* pts, int likelihood, int num_expts, const double* rows, int64_t num_rows,
                    int num_problems, int row_stride_cols, int num_chains, int64_t first_row, int64_t total_rows, int tail_per_chain,
                    double* workspace, size_t workspace_bytes, void* stream) {
  int rc = phf_check_points(who, pts, num_problems, 0);
  if (rc != PHF_OK) return rc;
  Layout L;
  if ((rc = layout_of(who, num_problems, pts->stride, num_chains, total_rows, tail_per_chain, &L)) != PHF_OK) return rc;
  if (likelihood != kGiven && (rc = phf_check_likelihood(who, likelihood, num_expts)) != PHF_OK) return rc;   // phf_psis_accumulate's own codes
  const int cols = likelihood == kGiven ? pts->stride : likelihood == kHierarchical ? 5 + 2 * num_expts : likelihood + 1;
  if ((rc = phf_check_row_stride(who, row_stride_cols, cols, "is smaller than the columns the likelihood reads")) != PHF_OK) return rc;
  if ((rc = phf_check_row_window(who, num_rows, first_row, total_rows)) != PHF_OK) return rc;
  if (!rows || !workspace) return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
  if ((rc = phf_check_workspace(who, "psis", workspace, workspace_bytes, L.bytes())) != PHF_OK) return rc;
  if (num_rows == 0) return PHF_OK;
  PsisArgs a = {};
  a.pts = *pts; a.rows = rows; a.nr = num_rows; a.first_row = first_row; a.total_rows = total_rows;
  a.Q = num_problems; a.stride_cols = row_stride_cols; a.C = num_chains; a.ne = num_expts;
  a.k = L.k; a.M = (int32_t)L.M; a.fields = workspace; a.thr = workspace + L.fields; a.heap = workspace + L.fields + L.thr;
  a.ncg = (num_chains + 63) / 64; a.npb = (pts->stride + kPtBlock - 1) / kPtBlock;
  a.units = num_problems * a.ncg * a.npb;
  const dim3 grid(blocks_for(a.units, kWaves)), block(kThreads);
  const dim3 tgrid((unsigned)((int64_t)num_problems * pts->stride));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t rstep = (size_t)num_problems * row_stride_cols * num_chains;
  // one launch per block between threshold rows (the same rows whatever the calls), T recomputed at each threshold row
  for (int64_t r = first_row, end = first_row + num_rows; r < end;) {
    const int64_t nb = next_threshold_row(r), b = nb < end ? nb : end;
    a.rows = rows + (size_t)(r - first_row) * rstep; a.first_row = r; a.nr = b - r;
    if (likelihood == 1) hipLaunchKernelGGL(psis_accumulate_kernel<1>, grid, block, 0, s, a);
    else if (likelihood == 2) hipLaunchKernelGGL(psis_accumulate_kernel<2>, grid, block, 0, s, a);
    else if (likelihood == kHierarchical) hipLaunchKernelGGL(psis_accumulate_kernel<kHierarchical>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(psis_accumulate_kernel<kGiven>, grid, block, 0, s, a);
    if ((rc = phf_check_launch("psis_accumulate_kernel")) != PHF_OK) return rc;
    if (b == nb && b < total_rows) {
      hipLaunchKernelGGL(psis_threshold_kernel, tgrid, block, 0, s, a);
      if ((rc = phf_check_launch("psis_threshold_kernel")) != PHF_OK) return rc;
    }
    r = b;
  }
  return PHF_OK;
}

}  // namespace

extern "C" int phf_psis_accumulate(const phf_pointwise_points* pts, int likelihood, int num_expts, const double* rows, int64_t num_rows,
                                   int num_problems, int row_stride_cols, int num_chains, int64_t first_row, int64_t total_rows,
                                   int tail_per_chain, double* workspace, size_t workspace_bytes, void* stream) {
  // the sibling's code is not this entry's to take: 0 fails the range check inside, after the points and the layout as before
  return psis_accumulate("phf_psis_accumulate", pts, likelihood == kGiven ? 0 : likelihood, num_expts, rows, num_rows, num_problems,
                         row_stride_cols, num_chains, first_row, total_rows, tail_per_chain, workspace, workspace_bytes, stream);
}

extern "C" int phf_psis_accumulate_given(const phf_pointwise_points* pts, const double* rows, int64_t num_rows, int num_problems,
                                         int row_stride_cols, int num_chains, int64_t first_row, int64_t total_rows, int tail_per_chain,
                                         double* workspace, size_t workspace_bytes, void* stream) {
  return psis_accumulate("phf_psis_accumulate_given", pts, kGiven, 0, rows, num_rows, num_problems, row_stride_cols, num_chains, first_row,
                         total_rows, tail_per_chain, workspace, workspace_bytes, stream);
}

extern "C" int phf_psis_reduce(const phf_pointwise_points* pts, int num_problems, int num_chains, int64_t total_rows, int tail_per_chain,
                               double* workspace, size_t workspace_bytes, double* out, double* tail_out, void* stream) {
  static const char* who = "phf_psis_reduce";
  int rc = phf_check_points(who, pts, num_problems, 0);
  if (rc != PHF_OK) return rc;
  Layout L;
  if ((rc = layout_of(who, num_problems, pts->stride, num_chains, total_rows, tail_per_chain, &L)) != PHF_OK) return rc;
  if (!workspace || !out) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_psis_reduce: null pointer");
  if ((rc = phf_check_workspace(who, "psis", workspace, workspace_bytes, L.bytes())) != PHF_OK) return rc;
  PsisArgs a = {};
  a.pts = *pts; a.Q = num_problems; a.C = num_chains; a.total_rows = total_rows;
  a.k = L.k; a.M = (int32_t)L.M; a.p2 = (int32_t)L.p2;
  a.fields = workspace; a.thr = workspace + L.fields; a.heap = a.thr + L.thr; a.scratch = a.heap + L.heap;
  a.out = out; a.tail_out = tail_out;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (L.hbm) hipLaunchKernelGGL(psis_reduce_kernel<true>, dim3(L.groups), dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(psis_reduce_kernel<false>, dim3(L.groups), dim3(kThreads), 0, s, a);
  return phf_check_launch("psis_reduce_kernel");
}

// phf_quantiles.hip — posterior quantiles and dose-response credible bands from exact-count histograms (include/pyhillfit_amd.h).
//
// Per slot (problem, column) — a column of the rows, or one dose of the Hill curve (curve bands) — the workspace keeps B bins of the
// grid of phf_grid.h: an anchor a (the first finite value, in (row, chain) order, of all rows accumulated), a power-of-two base width
// w0 and a level k, t = (x - a) * (1/w0), j = floor(t * 2^-k) + B/2.
// Each accumulate call runs
//   prepare  one workgroup per slot (phf_grid_prepare): anchor, min/max, the least level holding the running [min, max], the merge;
//   bin      workgroups of (slot, slice of the call's values): a workgroup-private uint32 histogram in LDS (a wavefront whose lanes
//            all fall in one bin adds once), flushed to the uint64 counts in HBM with integer atomics for its non-zero bins only.
// Integer counts are order-independent: the result is bit-identical whatever the launch shape, the arrival order or the row cuts.
// A value that is not finite, or whose t is not (|x - a| beyond ~2^980 w0), is counted apart and never binned.
// Hierarchical bands (phf_hier_bands.h): two more value sources read columns 0..3 (alpha, beta, mu, s) of a hierarchical row — the
// curve of the inferred underlying effect (Hill = alpha, pIC50 = mu) and of a predicted future experiment (Hill*, pIC50* drawn by
// inversion from the draw's own Philox block, addressed by the GLOBAL row index).  A value is a pure function of (problem, dose,
// row, chain): prepare and bin each recompute it, D doses of one draw recompute the draw's block, two logits and one exp.
// reduce: one workgroup per slot, a prefix sum over the bins; for each p the bin of the rank r = ceil(p N) draw (clamped to [1, N];
// numpy's quantile(method="inverted_cdf")), its edges clamped to [min, max], and a value interpolated linearly by rank in the bin.
#include <hip/hip_runtime.h>

#include "../../include/pyhillfit_amd.h"
#include "phf_host_checks.h"
#include "phf_grid.h"
#include "phf_hier_bands.h"
#include "phf_pointwise.h"

namespace {

constexpr int kPrepThreads = kGridPrepThreads;
constexpr int kBinThreads = 512;
constexpr int kReduceThreads = 256;
constexpr int kHdr = PHF_GRID_HDR;
constexpr int kOutHead = kGridOutHead;
constexpr int kOutPerProb = 4;          // value, lo, hi, bin
constexpr int kMaxBins = 32768, kMaxProbs = 64;
constexpr int64_t kMaxFlat = 0x7fffffff;      // rows x chains of one call: a 31-bit flat index
constexpr int kUnderlying = 3, kFuture = 4;   // value sources after the column (0) and the single-level curves (1, 2)
constexpr int kDrawThreads = 256;

struct QArgs {
  const double* rows;             // [nr][Q][stride][C]
  const double* ln_dose;          // curves: [Q][G]
  unsigned n;                     // nr * C values per slot in this call
  int Q, stride, C, B, G;
  int spp;                        // slots per problem: columns + curve points
  int first, count;               // this launch's slot columns [first, first + count) of every problem
  int splits;
  unsigned per_split;
  unsigned long long* counts;     // [S][B]
  double* hdr;                    // [S][kHdr]
  unsigned long long* nonfinite;  // [S]
  const uint32_t* problem_id;     // hierarchical bands: [Q], the global problem number of each problem
  uint32_t chain_id_base, k0, k1; // ... and the stream's chain offset and key
  uint32_t first_row;             // ... and the global index of rows[0]
};

struct QReduceArgs {
  int B, S, P;
  double probs[kMaxProbs];
  const unsigned long long* counts;
  const double* hdr;
  const unsigned long long* nonfinite;
  double* out;                    // [S][kOutHead + kOutPerProb P]
};

// value i (= row * C + chain) of launch column k of problem q: a column of the rows (MODEL 0), the Hill curve of model MODEL at dose k
// (1, 2), or the hierarchical model's curve at dose k of the underlying effect (3) / of a future experiment (4): count doses each
template <int MODEL>
__device__ inline double q_value(const QArgs& a, int q, int k, unsigned i, phf_ktab k_exp, phf_ktab k_log) {
  const unsigned r = i / (unsigned)a.C, c = i - r * (unsigned)a.C;
  const double* x = a.rows + ((size_t)r * a.Q + q) * a.stride * (size_t)a.C + c;
  if (MODEL == 0) return x[(size_t)(a.first + k) * a.C];
  if (MODEL >= kUnderlying) {
    const size_t C = (size_t)a.C;
    return phf_band_value_k(MODEL == kFuture ? PHF_BAND_FUTURE : PHF_BAND_UNDERLYING, a.ln_dose[(size_t)q * a.count + k], x[0], x[C], x[2 * C],
                            x[3 * C], a.chain_id_base + c, a.problem_id[q], a.first_row + r, a.k0, a.k1, k_exp, k_log);
  }
  const double pic50 = x[0], hill = MODEL == 2 ? x[a.C] : 1.0;
  if (!__builtin_isfinite(pic50) || !__builtin_isfinite(hill)) return PHF_NAN;
  return phf_pw_pred(MODEL, a.ln_dose[(size_t)q * a.G + k], hill, PHF_LN10 * (6.0 - pic50), k_exp);
}

// the 2^(j/64) table of phf_exp_* into LDS (the Hill curve needs no other table); the future experiment's draws take logarithms: the log table too
template <int MODEL>
__device__ inline void load_tables() {
#if defined(__HIP_DEVICE_COMPILE__)
  if (MODEL == kFuture) {
    PHF_MATH_TABLES_TO_LDS();
  } else if (MODEL != 0) {
    for (int i = threadIdx.x; i < 64; i += blockDim.x) phf_lds_exp2[i] = phf_t_exp2[i];
    __syncthreads();
  }
#endif
}

// the log polynomial in vector registers where the value source takes logarithms (PHF_KFETCH_V), nothing otherwise
#define Q_KFETCH_LOG(name)                                          \
  double name##_buf[PHF_K_LOG_N];                                   \
  if (MODEL == kFuture) {                                           \
    PHF_UNROLL                                                      \
    for (int phf_i_ = 0; phf_i_ < PHF_K_LOG_N; ++phf_i_) {          \
      name##_buf[phf_i_] = phf_k_log[phf_i_];                       \
      asm volatile("" : "+v"(name##_buf[phf_i_]));                  \
    }                                                               \
  }                                                                 \
  const phf_ktab name = name##_buf

// ---- prepare: anchor, min/max, level, merge (phf_grid.h) -----------------------------------------------------------------------------
template <int MODEL>
__global__ __launch_bounds__(kPrepThreads) void q_prepare_kernel(const QArgs a) {
  extern __shared__ unsigned long long s_merge[];              // [B/2]
  load_tables<MODEL>();
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  Q_KFETCH_LOG(k_log);
  const int q = blockIdx.x / a.count, k = blockIdx.x % a.count;
  const size_t s = (size_t)q * a.spp + a.first + k;
  phf_grid_prepare<1>(a.hdr + s * kHdr, a.counts + s * a.B, a.B, a.n, s_merge,
                      [&](unsigned i) { return q_value<MODEL>(a, q, k, i, k_exp, k_log); });
}

// ---- bin: LDS histogram per workgroup, flushed with integer atomics ----------------------------------------------------------------
template <int MODEL>
__global__ __launch_bounds__(kBinThreads) void q_bin_kernel(const QArgs a) {
  extern __shared__ unsigned s_hist[];                          // [B]
  load_tables<MODEL>();
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  Q_KFETCH_LOG(k_log);
  const int split = blockIdx.x % a.splits;
  const int slot = blockIdx.x / a.splits;
  const int q = slot / a.count, k = slot % a.count;
  const size_t s = (size_t)q * a.spp + a.first + k;
  unsigned i0, i1;
  phf_grid_split_range(a.n, split, a.per_split, &i0, &i1);
  phf_grid_bin_values<kBinThreads>(a.hdr + s * kHdr, a.counts + s * a.B, a.nonfinite + s, a.B, i0, i1, s_hist,
                                   [&](unsigned i) { return q_value<MODEL>(a, q, k, i, k_exp, k_log); });
}

// ---- reduce ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kReduceThreads) void q_reduce_kernel(const QReduceArgs a) {
  __shared__ unsigned long long s_sum[kReduceThreads];
  const int s = blockIdx.x, tid = threadIdx.x;
  const unsigned long long* cnt = a.counts + (size_t)s * a.B;
  const double* h = a.hdr + (size_t)s * kHdr;
  double* o = a.out + (size_t)s * (kOutHead + kOutPerProb * a.P);
  const int chunk = a.B / kReduceThreads > 0 ? a.B / kReduceThreads : 1;
  const int used = a.B / chunk;                                 // threads holding a chunk of the bins
  unsigned long long mine = 0;
  if (tid < used)
    for (int j = tid * chunk; j < (tid + 1) * chunk; ++j) mine += cnt[j];
  s_sum[tid] = mine;
  __syncthreads();
  if (tid == 0) {                                               // exclusive prefix sum of the chunks, in order
    unsigned long long run = 0;
    for (int t = 0; t < kReduceThreads; ++t) {
      const unsigned long long v = s_sum[t];
      s_sum[t] = run;
      run += v;
    }
    phf_grid_write_head(h, run, a.nonfinite[s], o);
    for (int p = 0; p < a.P; ++p)
      for (int f = 0; f < kOutPerProb; ++f) o[kOutHead + kOutPerProb * p + f] = PHF_NAN;
  }
  __syncthreads();
  const unsigned long long before = s_sum[tid];
  const double N = o[2];
  if (N == 0.0 || tid >= used) return;
  const double mn = h[PHF_GRID_MIN], mx = h[PHF_GRID_MAX], width = __builtin_ldexp(h[PHF_GRID_W0], (int)h[PHF_GRID_LEVEL]);
  const double anchor = h[PHF_GRID_ANCHOR];
  const int half = a.B / 2;
  for (int p = 0; p < a.P; ++p) {
    double r = __builtin_ceil(a.probs[p] * N);
    r = __builtin_fmin(__builtin_fmax(r, 1.0), N);
    const unsigned long long rank = (unsigned long long)r;
    if (!(before < rank && rank <= before + mine)) continue;   // exactly one thread holds the rank-r draw
    unsigned long long cum = before;
    int j = tid * chunk;
    for (; j < (tid + 1) * chunk - 1; ++j) {
      if (cum + cnt[j] >= rank) break;
      cum += cnt[j];
    }
    const double e = (double)(j - half) * width;                // exact: a small integer times a power of two
    double lo = __builtin_fmax(anchor + e, mn), hi = __builtin_fmin(anchor + (e + width), mx);
    lo = __builtin_fmin(lo, hi);
    const double nb = (double)cnt[j];
    const double v = lo + (hi - lo) * (((double)(rank - cum) - 0.5) / nb);
    double* op = o + kOutHead + kOutPerProb * p;
    op[0] = v; op[1] = lo; op[2] = hi; op[3] = (double)j;
  }
}

// ---- batch evaluator of the band draws ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDrawThreads) void hier_band_draws_kernel(int64_t m, const double* theta, const uint32_t* counter, uint32_t k0,
                                                                       uint32_t k1, double* out) {
  PHF_MATH_TABLES_TO_LDS();
  const int64_t i = (int64_t)blockIdx.x * kDrawThreads + threadIdx.x;
  if (i >= m) return;
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  double hill, pic50;
  phf_band_future_k(theta[i], theta[m + i], theta[2 * m + i], theta[3 * m + i], counter[3 * i], counter[3 * i + 1], counter[3 * i + 2], k0,
                    k1, k_exp, k_log, &hill, &pic50);
  out[2 * i] = hill;
  out[2 * i + 1] = pic50;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
struct Layout {
  size_t slots, counts_bytes, hdr_bytes, nf_bytes;
  size_t total() const { return counts_bytes + hdr_bytes + nf_bytes; }
};

Layout layout_of(int num_problems, int num_columns, int curve_points, int bins) {
  Layout l;
  l.slots = (size_t)num_problems * (size_t)(num_columns + curve_points);
  l.counts_bytes = l.slots * (size_t)bins * 8;
  l.hdr_bytes = l.slots * kHdr * 8;
  l.nf_bytes = l.slots * 8;
  return l;
}

int check_geometry(const char* who, int num_problems, int num_columns, int curve_points, int bins) {
  if (num_problems < 1 || num_columns < 0 || curve_points < 0 || num_columns + curve_points < 1)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: num_problems must be positive, num_columns and curve_points non-negative, not both 0", who);
  if (phf_grid_check_bins(who, bins, kMaxBins) != PHF_OK) return PHF_ERR_INVALID_ARGUMENT;
  if ((double)num_problems * (num_columns + curve_points) > 2147483647.0 / 8)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: too many slots (fewer problems per workspace)", who);
  return PHF_OK;
}

int check_rows(const char* who, const double* rows, int64_t num_rows, int row_stride_cols, int num_chains, int needed_cols,
               int64_t first_row, int64_t total_rows) {
  int rc = phf_check_positive(who, "num_chains and row_stride_cols", {num_chains, row_stride_cols});
  if (rc != PHF_OK) return rc;
  if (row_stride_cols < needed_cols)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: row_stride_cols (%d) is smaller than the columns read (%d)", who, row_stride_cols, needed_cols);
  if ((rc = phf_check_row_window(who, num_rows, first_row, total_rows)) != PHF_OK) return rc;
  if ((double)num_rows * num_chains > (double)kMaxFlat)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: num_rows x num_chains must stay below 2^31 per call (accumulate in shorter segments)", who);
  if (num_rows > 0 && !rows) return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: null rows", who);
  return PHF_OK;
}

template <int MODEL>
int launch(QArgs a, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int slots = a.Q * a.count;
  const phf_grid_split split = phf_grid_split_of(a.n, slots);
  a.splits = split.splits; a.per_split = split.per_split;
  const size_t merge_lds = (size_t)a.B / 2 * 8, hist_lds = (size_t)a.B * 4;
  int rc;
  if ((rc = allow_lds(q_prepare_kernel<MODEL>, merge_lds, "hipFuncSetAttribute(q_prepare_kernel)")) != PHF_OK) return rc;
  if ((rc = allow_lds(q_bin_kernel<MODEL>, hist_lds, "hipFuncSetAttribute(q_bin_kernel)")) != PHF_OK) return rc;
  hipLaunchKernelGGL(q_prepare_kernel<MODEL>, dim3(slots), dim3(kPrepThreads), merge_lds, st, a);
  if ((rc = phf_check_launch("q_prepare_kernel")) != PHF_OK) return rc;
  hipLaunchKernelGGL(q_bin_kernel<MODEL>, dim3((unsigned)slots * a.splits), dim3(kBinThreads), hist_lds, st, a);
  return phf_check_launch("q_bin_kernel");
}

QArgs args_of(const double* rows, int64_t num_rows, int num_problems, int row_stride_cols, int num_chains, int num_columns,
              int curve_points, int bins, void* workspace) {
  const Layout l = layout_of(num_problems, num_columns, curve_points, bins);
  QArgs a = {};
  a.rows = rows; a.n = (unsigned)(num_rows * num_chains);
  a.Q = num_problems; a.stride = row_stride_cols; a.C = num_chains; a.B = bins; a.G = curve_points;
  a.spp = num_columns + curve_points;
  char* base = static_cast<char*>(workspace);
  a.counts = reinterpret_cast<unsigned long long*>(base);
  a.hdr = reinterpret_cast<double*>(base + l.counts_bytes);
  a.nonfinite = reinterpret_cast<unsigned long long*>(base + l.counts_bytes + l.hdr_bytes);
  return a;
}

}  // namespace

extern "C" size_t phf_quantiles_workspace_bytes(int num_problems, int num_columns, int curve_points, int bins) {
  if (check_geometry("phf_quantiles_workspace_bytes", num_problems, num_columns, curve_points, bins) != PHF_OK) return 0;
  return layout_of(num_problems, num_columns, curve_points, bins).total();
}

extern "C" int phf_quantiles_init(int num_problems, int num_columns, int curve_points, int bins, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  static const char* who = "phf_quantiles_init";
  int rc = check_geometry(who, num_problems, num_columns, curve_points, bins);
  if (rc != PHF_OK) return rc;
  const size_t need = layout_of(num_problems, num_columns, curve_points, bins).total();
  return phf_init_workspace(who, "quantiles", workspace, workspace_bytes, need, need, stream);
}

extern "C" int phf_quantiles_accumulate(const double* rows, int64_t num_rows, int num_problems, int row_stride_cols, int num_chains,
                                        int num_columns, int curve_points, int bins, int64_t first_row, int64_t total_rows,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  static const char* who = "phf_quantiles_accumulate";
  int rc = check_geometry(who, num_problems, num_columns, curve_points, bins);
  if (rc != PHF_OK) return rc;
  if (num_columns < 1) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_quantiles_accumulate: the workspace has no columns");
  if ((rc = check_rows(who, rows, num_rows, row_stride_cols, num_chains, num_columns, first_row, total_rows)) != PHF_OK) return rc;
  if ((rc = phf_check_workspace(who, "quantiles", workspace, workspace_bytes, layout_of(num_problems, num_columns, curve_points, bins).total())) != PHF_OK) return rc;
  if (num_rows == 0) return PHF_OK;
  QArgs a = args_of(rows, num_rows, num_problems, row_stride_cols, num_chains, num_columns, curve_points, bins, workspace);
  a.first = 0; a.count = num_columns;
  return launch<0>(a, stream);
}

extern "C" int phf_quantiles_accumulate_curves(const double* rows, int64_t num_rows, int num_problems, int row_stride_cols,
                                               int num_chains, int model, const double* ln_doses, int num_columns, int curve_points,
                                               int bins, int64_t first_row, int64_t total_rows, void* workspace, size_t workspace_bytes,
                                               void* stream) {
  static const char* who = "phf_quantiles_accumulate_curves";
  int rc = check_geometry(who, num_problems, num_columns, curve_points, bins);
  if (rc != PHF_OK) return rc;
  if (model != 1 && model != 2) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_quantiles_accumulate_curves: model must be 1 or 2");
  if (curve_points < 1) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_quantiles_accumulate_curves: the workspace has no curve points");
  if (!ln_doses) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_quantiles_accumulate_curves: null ln_doses");
  if ((rc = check_rows(who, rows, num_rows, row_stride_cols, num_chains, model, first_row, total_rows)) != PHF_OK) return rc;
  if ((rc = phf_check_workspace(who, "quantiles", workspace, workspace_bytes, layout_of(num_problems, num_columns, curve_points, bins).total())) != PHF_OK) return rc;
  if (num_rows == 0) return PHF_OK;
  QArgs a = args_of(rows, num_rows, num_problems, row_stride_cols, num_chains, num_columns, curve_points, bins, workspace);
  a.ln_dose = ln_doses; a.first = num_columns; a.count = curve_points;
  return model == 1 ? launch<1>(a, stream) : launch<2>(a, stream);
}

extern "C" int phf_quantiles_accumulate_hier_curves(const double* rows, int64_t num_rows, int num_problems, int row_stride_cols,
                                                    int num_chains, const double* ln_doses, int num_columns, int num_doses, int bins,
                                                    int64_t first_row, int64_t total_rows, const uint32_t* problem_id,
                                                    uint32_t chain_id_base, uint64_t seed, void* workspace, size_t workspace_bytes,
                                                    void* stream) {
  static const char* who = "phf_quantiles_accumulate_hier_curves";
  if (num_doses < 1 || num_doses > (1 << 20))
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_quantiles_accumulate_hier_curves: num_doses must be in [1, 2^20]");
  const int curve_points = 2 * num_doses;
  int rc = check_geometry(who, num_problems, num_columns, curve_points, bins);
  if (rc != PHF_OK) return rc;
  if (!ln_doses) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_quantiles_accumulate_hier_curves: null ln_doses");
  if (!problem_id) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_quantiles_accumulate_hier_curves: null problem_id");
  if ((rc = check_rows(who, rows, num_rows, row_stride_cols, num_chains, 4, first_row, total_rows)) != PHF_OK) return rc;
  if (total_rows > 4294967296LL)
    return phf_fail(PHF_ERR_INVALID_ARGUMENT,
                    "phf_quantiles_accumulate_hier_curves: total_rows must fit the 32-bit row word of the random stream");
  if ((rc = phf_check_workspace(who, "quantiles", workspace, workspace_bytes, layout_of(num_problems, num_columns, curve_points, bins).total())) != PHF_OK) return rc;
  if (num_rows == 0) return PHF_OK;
  QArgs a = args_of(rows, num_rows, num_problems, row_stride_cols, num_chains, num_columns, curve_points, bins, workspace);
  a.ln_dose = ln_doses; a.problem_id = problem_id; a.chain_id_base = chain_id_base;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.first_row = (uint32_t)first_row;
  a.first = num_columns; a.count = num_doses;
  if ((rc = launch<kUnderlying>(a, stream)) != PHF_OK) return rc;
  a.first = num_columns + num_doses;
  return launch<kFuture>(a, stream);
}

extern "C" int phf_hier_band_draws(int64_t m, const double* theta, const uint32_t* counter, uint64_t seed, double* out, void* stream) {
  if (m < 0 || (m > 0 && (!theta || !counter || !out)))
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_band_draws: m must be >= 0 and the arrays non-null");
  if (m == 0) return PHF_OK;
  hipLaunchKernelGGL(hier_band_draws_kernel, dim3((unsigned)((m + kDrawThreads - 1) / kDrawThreads)), dim3(kDrawThreads), 0,
                     static_cast<hipStream_t>(stream), m, theta, counter, (uint32_t)seed, (uint32_t)(seed >> 32), out);
  return phf_check_launch("phf_hier_band_draws");
}

extern "C" int phf_quantiles_reduce(int num_problems, int num_columns, int curve_points, int bins, const double* probs, int num_probs,
                                    const void* workspace, size_t workspace_bytes, double* out, void* stream) {
  static const char* who = "phf_quantiles_reduce";
  int rc = check_geometry(who, num_problems, num_columns, curve_points, bins);
  if (rc != PHF_OK) return rc;
  if (num_probs < 1 || num_probs > kMaxProbs || !probs)
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_quantiles_reduce: 1 to 64 probabilities, in host memory");
  for (int p = 0; p < num_probs; ++p)
    if (!(probs[p] >= 0.0 && probs[p] <= 1.0)) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_quantiles_reduce: probabilities must lie in [0, 1]");
  const Layout l = layout_of(num_problems, num_columns, curve_points, bins);
  if ((rc = phf_check_workspace(who, "quantiles", workspace, workspace_bytes, l.total())) != PHF_OK) return rc;
  if (!out) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_quantiles_reduce: null out");
  QReduceArgs a = {};
  a.B = bins; a.S = (int)l.slots; a.P = num_probs;
  for (int p = 0; p < num_probs; ++p) a.probs[p] = probs[p];
  const char* base = static_cast<const char*>(workspace);
  a.counts = reinterpret_cast<const unsigned long long*>(base);
  a.hdr = reinterpret_cast<const double*>(base + l.counts_bytes);
  a.nonfinite = reinterpret_cast<const unsigned long long*>(base + l.counts_bytes + l.hdr_bytes);
  a.out = out;
  hipLaunchKernelGGL(q_reduce_kernel, dim3((unsigned)l.slots), dim3(kReduceThreads), 0, static_cast<hipStream_t>(stream), a);
  return phf_check_launch("q_reduce_kernel");
}

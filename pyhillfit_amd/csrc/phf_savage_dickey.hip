// phf_savage_dickey.hip — Savage-Dickey Bayes factor B12 of "Hill = 1" against "Hill free" from the model-2 draws (phf_savage_dickey.h;
// DESIGN.md §3, "Savage-Dickey Bayes factor"): per (problem, chain) the sums over the used rows of r = L(Hill = 1) / mean_h L(h), the
// mean over Hill's prior support taken by a P-panel Gauss-Kronrod rule at the draw's (pIC50, sigma).
//
// Mapping: one wavefront per (problem, chain), walking the call's used rows in row order.  The pair's merged entries (ln conc,
// response, weight) sit in the wavefront's own slice of LDS and the node table [3][15 P] once per block: every lane reads an entry at
// the same address (a broadcast).  The draw's (pIC50, sigma) are wave-uniform; lane t evaluates l(h) at its nodes t, t + 64, ... and
// lane 15 P mod 64 also at h = 1 (phf_sd_lane: the host twin runs the very same function for t = 0..63), keeping two online
// log-sum-exps; a butterfly of __shfl_xor, the lower lane's part first, merges the lanes — lane 0 ends with the tree of phf_mg_tree —
// and lane 0's registers hold the chain's eight sums, read from the accumulator at the start and written back once at the end:
// however the calls cut the rows, every sum sees the same additions in the same order.  No atomics, nothing merged across chains;
// exp2, log and log Phi tables in LDS.
#include <hip/hip_runtime.h>

#include "../../include/pyhillfit_amd.h"
#include "phf_common.h"
#include "phf_savage_dickey.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxStride = 256;         // entries per pair the per-wave LDS slices are sized for (4 x 3 x 256 doubles = 24 KiB)
constexpr int kCols = 4;                // a model-2 row: pIC50, Hill, sigma, log-target

struct SdArgs {
  phf_points pts;
  const double* nodes;            // [3][15 P]
  const double* rows;             // [nr][Q][kCols][C]; the first used row of the call is local row r0, then every `every`-th
  double* acc;                    // [Q][C][PHF_SD_ACC_DOUBLES]
  int64_t r0, used;
  int32_t every, Q, C;
};

extern __shared__ __attribute__((aligned(16))) double sd_smem[];

template <int P>
__global__ __launch_bounds__(kThreads) void savage_dickey_kernel(const SdArgs a) {
  constexpr int NQ = PHF_SD_PANEL_NODES * P;
  PHF_MATH_TABLES_TO_LDS();
  PHF_LOGPHI_TABLE_TO_LDS();
  double* nodes = sd_smem;                                               // [3][NQ]
  for (int i = threadIdx.x; i < 3 * NQ; i += kThreads) nodes[i] = a.nodes[i];
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
  const int64_t unit = (int64_t)blockIdx.x * kWaves + wave;              // wave-uniform: (problem, chain)
  if (unit >= (int64_t)a.Q * a.C) return;
  const int lane = threadIdx.x & 63;
  const int q = (int)(unit / a.C), c = (int)(unit % a.C);
  const int ps = a.pts.stride;                                           // 1..kMaxStride (checked by the launcher)
  double* lc = sd_smem + 3 * NQ + (size_t)wave * 3 * ps;                  // this wavefront's entries: ln conc [ps], y [ps], w [ps]
  double* yv = lc + ps;
  double* wv = yv + ps;
  int n_other, n_cens;
  phf_sd_counts(a.pts.counts + 4 * (size_t)q, ps, &n_other, &n_cens);
  const size_t at = (size_t)q * ps;
  for (int j = 0; j < n_other + n_cens; ++j) {                           // every lane stores the same values: the slice belongs to this
    lc[j] = a.pts.ln_conc[at + j];                                       // wavefront alone, and a lane reads back what it wrote itself
    yv[j] = a.pts.response[at + j];
    wv[j] = a.pts.weight[at + j];
  }
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  double* acc = a.acc + (size_t)unit * PHF_SD_ACC_DOUBLES;
  double s[PHF_SD_ACC_DOUBLES];
  PHF_UNROLL
  for (int i = 0; i < PHF_SD_ACC_DOUBLES; ++i) s[i] = acc[i];
  const size_t C = (size_t)a.C;
  for (int64_t u = 0; u < a.used; ++u) {
    const double* x = a.rows + (((size_t)(a.r0 + u * a.every) * a.Q + q) * kCols) * C + c;
    const double pic50 = x[0], sigma = x[2 * C];
    if (!phf_sd_draw_ok(pic50, sigma)) {                                 // a wave-uniform branch
      s[PHF_SD_SKIPPED] += 1.0;
      continue;
    }
    const double ln_ic50 = PHF_LN10 * (6.0 - pic50), inv_s = phf_rcp(sigma);
    phf_mg_lse f, g;
    double e1;
    phf_sd_lane(lane, NQ, nodes, lc, yv, wv, n_other, n_cens, ln_ic50, inv_s, k_exp, &f, &g, &e1);
    e1 = __shfl(e1, NQ % 64, 64);
    for (int o = 32; o > 0; o >>= 1) {
      phf_mg_lse of, og;
      of.m = __shfl_xor(f.m, o, 64); of.s = __shfl_xor(f.s, o, 64);
      og.m = __shfl_xor(g.m, o, 64); og.s = __shfl_xor(g.s, o, 64);
      f = (lane & o) ? phf_mg_merge(of, f, k_exp) : phf_mg_merge(f, of, k_exp);     // the lower lane's part first
      g = (lane & o) ? phf_mg_merge(og, g, k_exp) : phf_mg_merge(g, og, k_exp);
    }
    phf_sd_draw_add(f, g, e1, k_exp, k_log, s);                          // lane 0 holds the tree; the other lanes' sums are never stored
  }
  if (lane == 0) {
    PHF_UNROLL
    for (int i = 0; i < PHF_SD_ACC_DOUBLES; ++i) acc[i] = s[i];
  }
}

size_t lds_bytes(int panels, int stride) {
  return ((size_t)3 * PHF_SD_PANEL_NODES * panels + (size_t)kWaves * 3 * stride) * sizeof(double);
}

}  // namespace

extern "C" int phf_savage_dickey_accumulator_doubles(void) { return PHF_SD_ACC_DOUBLES; }

extern "C" int phf_savage_dickey_nodes(int panels) { return phf_sd_panels_ok(panels) ? PHF_SD_PANEL_NODES * panels : -1; }

extern "C" int64_t phf_savage_dickey_rows_used(int64_t first_row, int64_t num_rows, int every) {
  if (first_row < 0 || num_rows < 0 || every < 1) return -1;
  return phf_sd_rows_used(first_row, num_rows, every);
}

extern "C" int phf_savage_dickey_accumulate(const phf_points* pts, int panels, const double* nodes, const double* rows, int64_t num_rows,
                                            int num_problems, int row_stride_cols, int num_chains, int64_t first_row, int every,
                                            double* accumulators, size_t accumulator_bytes, void* stream) {
  static const char* who = "phf_savage_dickey_accumulate";
  if (!phf_sd_panels_ok(panels))
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: panels must be 16, 32 or 64 (got %d)", who, panels);
  if (!pts || !pts->ln_conc || !pts->response || !pts->weight || !pts->counts)
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_savage_dickey_accumulate: null points");
  if (!nodes || !rows || !accumulators) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_savage_dickey_accumulate: null pointer");
  if (row_stride_cols != kCols)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: row_stride_cols must be %d, the columns of a model-2 row (pIC50, Hill, sigma, log-target), got %d",
                     who, kCols, row_stride_cols);
  if (every < 1) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_savage_dickey_accumulate: every must be >= 1");
  if (num_chains < 1) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_savage_dickey_accumulate: num_chains must be positive");
  if (num_problems < 1 || pts->num_pairs != num_problems)
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_savage_dickey_accumulate: the points must have one pair per problem");
  if (pts->stride < 1 || pts->stride > kMaxStride)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: 1..%d entries per pair (stride %d)", who, kMaxStride, pts->stride);
  if (num_rows < 0 || first_row < 0) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_savage_dickey_accumulate: num_rows and first_row must be >= 0");
  const int64_t units = (int64_t)num_problems * num_chains;
  if (units > (2147483647ll - kWaves) * kWaves) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_savage_dickey_accumulate: too many (problem, chain) units");
  if (accumulator_bytes < (size_t)units * PHF_SD_ACC_DOUBLES * sizeof(double))
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: the accumulators are smaller than num_problems x num_chains x %d doubles", who, PHF_SD_ACC_DOUBLES);
  const int64_t used = phf_sd_rows_used(first_row, num_rows, every);
  if (used == 0) return PHF_OK;                                          // no row of the call is used: no launch
  SdArgs a = {};
  a.pts = *pts; a.nodes = nodes; a.rows = rows; a.acc = accumulators;
  a.r0 = (every - first_row % every) % every; a.used = used;
  a.every = every; a.Q = num_problems; a.C = num_chains;
  const dim3 grid((unsigned)((units + kWaves - 1) / kWaves)), block(kThreads);
  const size_t lds = lds_bytes(panels, pts->stride);
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (panels) {
    case 16: hipLaunchKernelGGL(savage_dickey_kernel<16>, grid, block, lds, s, a); break;
    case 32: hipLaunchKernelGGL(savage_dickey_kernel<32>, grid, block, lds, s, a); break;
    default: hipLaunchKernelGGL(savage_dickey_kernel<64>, grid, block, lds, s, a); break;
  }
  return phf_check_launch(who);
}

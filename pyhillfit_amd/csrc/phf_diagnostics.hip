// phf_diagnostics.hip — split-R-hat, multi-chain ESS and MCSE of every (problem, column), accumulated while the rows stream past.
//
// The estimators are those of the Stan reference manual (Gelman et al., BDA3 11.4-11.5; Vehtari et al. 2021) WITHOUT rank
// normalisation: every chain is split into two half-chains of h = floor(N/2) rows (the middle row of an odd N is dropped) and
// the finished quantity per half-chain is its mean and its autocovariance acov(k), k = 0..L, L = min(K, h-1).  Geyer's
// truncation over the chain-averaged autocovariances runs on the host (pyhillfit_amd/diagnostics.py).
//
// Per (problem, column, chain) the workspace holds, with y = x - x0 (x0 = the half-chain's first value, against cancellation:
// the log-target sits near -40 with an sd near 1):
//   Q[k] = sum_{n=k}^{m-1} y_n y_{n-k}  (k = 0..L),  the first L values, a ring of the last L values, x0 and S = sum y_n.
// When the half-chain closes, h acov(k) = Q_k - ybar (A_k + B_k) + (h - k) ybar^2 with A_k = S - (sum of the last k values) and
// B_k = S - (sum of the first k values); half 0's acov goes to a finished array, half 1's replaces Q in place.
//
// Mapping.  Lag kernel: one lane = one chain (the rows are [rows][Q][stride][C], chain fastest: a wavefront reads 512 contiguous
// bytes of one (problem, column)), one wavefront = a block of 32 lags (1..L; lag 0 is the update kernel's), so 32 accumulators
// and a 32-value window of past values live in registers (183 VGPRs with hipcc: 2 waves per SIMD; a block of 16 lags fits 3 waves
// but doubles the loads per FMA.  The loads are L1/L2 hits: the four wavefronts of a workgroup are consecutive lag blocks of the
// same rows).  The row loop is
// unrolled by 32 so that the window is a ring with compile-time indices: nothing moves.  Update kernel: one lane per chain,
// serial over the rows (S, Q[0], the first and last L values).  Reduce kernel: one wavefront per (problem, column, lag) adds
// over the chains in a fixed order (lane l takes chains l, l+64, ...; then a fixed butterfly).
//
// Deterministic: no atomics, every value is produced by one lane in row order, and accumulators round-trip through HBM exactly,
// so the result is bit-identical however the rows are cut into calls and whatever the launch shape.
#include <hip/hip_runtime.h>

#include "../../include/pyhillfit_amd.h"
#include "phf_half_chains.h"
#include "phf_host_checks.h"
#include "phf_device_util.h"

#define PHF_DIAG_UNROLL _Pragma("unroll")

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kLagBlock = 32;

// workspace fields per (problem, column), each [num_chains] doubles
struct Layout {
  int L;
  int64_t h;
  int F;
  __host__ __device__ int q_(int k) const { return k; }                       // Q[k], k = 0..L; half 1's acov after it closes
  __host__ __device__ int head(int i) const { return L + 1 + i; }             // y_0..y_{L-1}
  __host__ __device__ int ring(int i) const { return 2 * L + 1 + i; }         // y_m at slot m mod L
  __host__ __device__ int x0() const { return 3 * L + 1; }
  __host__ __device__ int s() const { return 3 * L + 2; }
  __host__ __device__ int fin(int k) const { return 3 * L + 3 + k; }          // half 0's acov(k), k = 0..L
  __host__ __device__ int xbar(int half) const { return 4 * L + 4 + half; }
};

Layout layout_of(int lags, int64_t total_rows) {
  Layout l;
  l.h = total_rows / 2;
  l.L = (int)(lags < l.h - 1 ? lags : l.h - 1);
  l.F = 4 * l.L + 6;
  return l;
}

struct DiagArgs {
  const double* rows;             // first row of this sub-segment: [nr][Q][stride][C]
  int64_t nr;                     // rows in this sub-segment (all in one half-chain)
  int64_t m0;                     // half-chain index of its first row
  int32_t Q, stride, C, cols;
  Layout lay;
  double* ws;                     // [Q][cols][F][C]
  int32_t ncg, nlb;               // 64-chain groups, lag blocks
  int64_t units;
  int32_t half;
  double* out;                    // reduce: [Q][cols][L+3]
};

// y at half-chain index idx < m0 + nr: 0 before the half's start, the ring for rows of earlier calls, else this call's rows
// (branch-free: one load whatever the source, so the unrolled row loop does not grow three paths per row)
__device__ inline double past_value(const DiagArgs& a, const double* xr, const double* st, size_t rstep, int64_t idx, double x0) {
  const bool here = idx >= a.m0;
  const double* p = here ? xr + (size_t)(idx - a.m0) * rstep : st + (size_t)a.lay.ring(idx < 0 ? 0 : (int)(idx % a.lay.L)) * a.C;
  const double v = *p - (here ? x0 : 0.0);
  return idx < 0 ? 0.0 : v;
}

// Q[k] += sum over this sub-segment's rows m of y_m y_{m-k}, k = k0..k0+31 (k0 = 1 + 32 * lag block)
__global__ __launch_bounds__(kThreads) void diag_lag_kernel(const DiagArgs a) {
  const int64_t unit = (int64_t)blockIdx.x * kWaves + threadIdx.x / 64;
  if (unit >= a.units) return;
  const int lb = (int)(unit % a.nlb);
  int64_t rest = unit / a.nlb;
  const int cg = (int)(rest % a.ncg); rest /= a.ncg;
  const int j = (int)(rest % a.cols);
  const int q = (int)(rest / a.cols);
  const int c = cg * 64 + (threadIdx.x & 63);
  if (c >= a.C) return;
  const int L = a.lay.L;
  const int k0 = 1 + kLagBlock * lb;
  const size_t rstep = (size_t)a.Q * a.stride * a.C;
  const double* xr = a.rows + ((size_t)q * a.stride + j) * a.C + c;
  double* st = a.ws + ((size_t)q * a.cols + j) * a.lay.F * a.C + c;
  const double x0 = a.m0 == 0 ? xr[0] : st[(size_t)a.lay.x0() * a.C];

  double acc[kLagBlock], win[kLagBlock];
  PHF_DIAG_UNROLL
  for (int i = 0; i < kLagBlock; ++i) acc[i] = (a.m0 > 0 && k0 + i <= L) ? st[(size_t)a.lay.q_(k0 + i) * a.C] : 0.0;
  // invariant before row m = m0 + base + u: win[(u - i) & 31] = y_{m-k0-i} for i = 1..31 (0 beyond lag L or before the half's start)
  win[0] = 0.0;
  PHF_DIAG_UNROLL
  for (int i = 1; i < kLagBlock; ++i) win[kLagBlock - i] = k0 + i <= L ? past_value(a, xr, st, rstep, a.m0 - k0 - i, x0) : 0.0;
  for (int64_t base = 0; base < a.nr; base += kLagBlock) {
    PHF_DIAG_UNROLL
    for (int u = 0; u < kLagBlock; ++u) {
      if (base + u < a.nr) {
        const int64_t m = a.m0 + base + u;
        win[u] = past_value(a, xr, st, rstep, m - k0, x0);
        const double y = xr[(size_t)(base + u) * rstep] - x0;
        PHF_DIAG_UNROLL
        for (int i = 0; i < kLagBlock; ++i) acc[i] = __builtin_fma(y, win[(u - i) & (kLagBlock - 1)], acc[i]);
      }
    }
  }
  PHF_DIAG_UNROLL
  for (int i = 0; i < kLagBlock; ++i)
    if (k0 + i <= L) st[(size_t)a.lay.q_(k0 + i) * a.C] = acc[i];
}

// x0, S, Q[0], the first L values and the ring of the last L values; one lane per (problem, column, chain), serial over the rows
__global__ __launch_bounds__(kThreads) void diag_update_kernel(const DiagArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.units) return;
  const int c = (int)(i % a.C);
  const int64_t qj = i / a.C;
  const int j = (int)(qj % a.cols), q = (int)(qj / a.cols);
  const int L = a.lay.L;
  const size_t rstep = (size_t)a.Q * a.stride * a.C, C = (size_t)a.C;
  const double* xr = a.rows + ((size_t)q * a.stride + j) * a.C + c;
  double* st = a.ws + ((size_t)q * a.cols + j) * a.lay.F * a.C + c;
  const double x0 = a.m0 == 0 ? xr[0] : st[a.lay.x0() * C];
  double S = a.m0 == 0 ? 0.0 : st[a.lay.s() * C];
  double q0 = a.m0 == 0 ? 0.0 : st[a.lay.q_(0) * C];
  const int64_t ring_from = a.nr - L;
  for (int64_t r = 0; r < a.nr; ++r) {
    const double y = xr[(size_t)r * rstep] - x0;
    const int64_t m = a.m0 + r;
    S += y;
    q0 = __builtin_fma(y, y, q0);
    if (m < L) st[(size_t)a.lay.head((int)m) * C] = y;
    if (r >= ring_from) st[(size_t)a.lay.ring((int)(m % L)) * C] = y;
  }
  st[a.lay.x0() * C] = x0;
  st[a.lay.s() * C] = S;
  st[a.lay.q_(0) * C] = q0;
}

// the half-chain `a.half` has seen its h rows: acov(k) for k = 0..L and its mean
__global__ __launch_bounds__(kThreads) void diag_close_kernel(const DiagArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.units) return;
  const int c = (int)(i % a.C);
  const int64_t qj = i / a.C;
  double* st = a.ws + (size_t)qj * a.lay.F * a.C + c;
  const size_t C = (size_t)a.C;
  const int L = a.lay.L;
  const int64_t h = a.lay.h;
  const double S = st[a.lay.s() * C], hd = (double)h;
  const double ybar = S / hd;
  double first = 0.0, last = 0.0;
  for (int k = 0; k <= L; ++k) {
    if (k > 0) {
      first += st[(size_t)a.lay.head(k - 1) * C];
      last += st[(size_t)a.lay.ring((int)((h - k) % L)) * C];
    }
    const double ab = (S - last) + (S - first);
    const double acov = (st[(size_t)a.lay.q_(k) * C] - ybar * ab + (double)(h - k) * ybar * ybar) / hd;
    st[(size_t)(a.half == 0 ? a.lay.fin(k) : a.lay.q_(k)) * C] = acov;
  }
  st[(size_t)a.lay.xbar(a.half) * C] = st[a.lay.x0() * C] + ybar;
}

// out[q][j][k] = mean over the 2C half-chains of acov(k), k = 0..L; out[q][j][L+1] = mean of the half-chain means;
// out[q][j][L+2] = their variance (divisor 2C - 1) = B/h.  One wavefront per (problem, column, k in 0..L+1).
__global__ __launch_bounds__(kThreads) void diag_reduce_kernel(const DiagArgs a) {
  const int64_t unit = (int64_t)blockIdx.x * kWaves + threadIdx.x / 64;
  if (unit >= a.units) return;
  const int lane = threadIdx.x & 63;
  const int L = a.lay.L;
  const int k = (int)(unit % (L + 2));
  const int64_t qj = unit / (L + 2);
  const double* st = a.ws + (size_t)qj * a.lay.F * a.C;
  const size_t C = (size_t)a.C;
  const double M = 2.0 * a.C;
  double* o = a.out + (size_t)qj * (L + 3);
  if (k <= L) {
    double s = 0.0;
    for (int c = lane; c < a.C; c += 64) s += st[(size_t)a.lay.fin(k) * C + c] + st[(size_t)a.lay.q_(k) * C + c];
    s = wave_sum(s);
    if (lane == 0) o[k] = s / M;
  } else {
    double s = 0.0;
    for (int c = lane; c < a.C; c += 64) s += st[(size_t)a.lay.xbar(0) * C + c] + st[(size_t)a.lay.xbar(1) * C + c];
    const double mean = wave_sum(s) / M;
    double v = 0.0;
    for (int c = lane; c < a.C; c += 64) {
      const double d0 = st[(size_t)a.lay.xbar(0) * C + c] - mean, d1 = st[(size_t)a.lay.xbar(1) * C + c] - mean;
      v += d0 * d0 + d1 * d1;
    }
    v = wave_sum(v);
    if (lane == 0) { o[L + 1] = mean; o[L + 2] = v / (M - 1.0); }
  }
}

// shared argument checks of the four entries; on success fills the layout
int check_shape(const char* who, int num_problems, int num_columns, int num_chains, int64_t total_rows, int lags, Layout* lay) {
  int rc = phf_check_positive(who, "num_problems, num_columns and num_chains", {num_problems, num_columns, num_chains});
  if (rc != PHF_OK) return rc;
  if (lags < 1) return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: the lag limit K must be positive (got %d)", who, lags);
  if (total_rows < 8)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: a half-chain needs h = floor(total_rows / 2) >= 4 rows (total_rows = %lld)", who,
                     (long long)total_rows);
  *lay = layout_of(lags, total_rows);
  const double units = (double)num_problems * num_columns * ((num_chains + 63) / 64) * ((lay->L + kLagBlock - 1) / kLagBlock);
  return phf_check_grid(who, {units / kWaves, (double)num_problems * num_columns * num_chains / kThreads});
}

size_t workspace_bytes_of(int num_problems, int num_columns, int num_chains, const Layout& lay) {
  return (size_t)num_problems * num_columns * (size_t)lay.F * num_chains * sizeof(double);
}

}  // namespace

extern "C" size_t phf_diagnostics_workspace_bytes(int num_problems, int num_columns, int num_chains, int64_t total_rows, int lags) {
  Layout lay;
  if (check_shape("phf_diagnostics_workspace_bytes", num_problems, num_columns, num_chains, total_rows, lags, &lay) != PHF_OK) return 0;
  return workspace_bytes_of(num_problems, num_columns, num_chains, lay);
}

extern "C" int phf_diagnostics_effective_lags(int64_t total_rows, int lags) {
  if (lags < 1 || total_rows < 8) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_diagnostics_effective_lags: need K >= 1 and total_rows >= 8");
  return layout_of(lags, total_rows).L;
}

extern "C" int phf_diagnostics_init(int num_problems, int num_columns, int num_chains, int64_t total_rows, int lags, double* workspace,
                                    size_t workspace_bytes, void* stream) {
  static const char* who = "phf_diagnostics_init";
  Layout lay;
  const int rc = check_shape(who, num_problems, num_columns, num_chains, total_rows, lags, &lay);
  if (rc != PHF_OK) return rc;
  const size_t need = workspace_bytes_of(num_problems, num_columns, num_chains, lay);
  return phf_init_workspace(who, "diagnostics", workspace, workspace_bytes, need, need, stream);
}

extern "C" int phf_diagnostics_accumulate(const double* rows, int64_t num_rows, int num_problems, int row_stride_cols, int num_chains,
                                          int num_columns, int64_t first_row, int64_t total_rows, int lags, double* workspace,
                                          size_t workspace_bytes, void* stream) {
  static const char* who = "phf_diagnostics_accumulate";
  Layout lay;
  int rc = check_shape(who, num_problems, num_columns, num_chains, total_rows, lags, &lay);
  if (rc != PHF_OK) return rc;
  if ((rc = phf_check_row_window(who, num_rows, first_row, total_rows)) != PHF_OK) return rc;
  if ((rc = phf_check_row_stride(who, row_stride_cols, num_columns, "must be >= num_columns")) != PHF_OK) return rc;
  if (!rows || !workspace) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_diagnostics_accumulate: null pointer");
  if ((rc = phf_check_workspace(who, "diagnostics", workspace, workspace_bytes, workspace_bytes_of(num_problems, num_columns, num_chains, lay))) != PHF_OK)
    return rc;
  if (num_rows == 0) return PHF_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  DiagArgs a = {};
  a.Q = num_problems; a.stride = row_stride_cols; a.C = num_chains; a.cols = num_columns; a.lay = lay; a.ws = workspace;
  a.ncg = (num_chains + 63) / 64; a.nlb = (lay.L + kLagBlock - 1) / kLagBlock;
  const size_t row_doubles = (size_t)num_problems * row_stride_cols * num_chains;
  const int64_t per_chain = (int64_t)num_problems * num_columns * num_chains;
  for (int half = 0; half < 2; ++half) {
    phf_half_segment seg;
    if (!phf_half_cut(total_rows, first_row, num_rows, half, &seg)) continue;
    a.rows = rows + (size_t)seg.offset * row_doubles;
    a.nr = seg.nr; a.m0 = seg.m0; a.half = half;
    a.units = (int64_t)num_problems * num_columns * a.ncg * a.nlb;
    hipLaunchKernelGGL(diag_lag_kernel, dim3(blocks_for(a.units, kWaves)), dim3(kThreads), 0, s, a);
    if ((rc = phf_check_launch("diag_lag_kernel")) != PHF_OK) return rc;
    a.units = per_chain;
    hipLaunchKernelGGL(diag_update_kernel, dim3(blocks_for(a.units, kThreads)), dim3(kThreads), 0, s, a);
    if ((rc = phf_check_launch("diag_update_kernel")) != PHF_OK) return rc;
    if (seg.closes) {
      hipLaunchKernelGGL(diag_close_kernel, dim3(blocks_for(a.units, kThreads)), dim3(kThreads), 0, s, a);
      if ((rc = phf_check_launch("diag_close_kernel")) != PHF_OK) return rc;
    }
  }
  return PHF_OK;
}

extern "C" int phf_diagnostics_reduce(int num_problems, int num_columns, int num_chains, int64_t total_rows, int lags,
                                      const double* workspace, size_t workspace_bytes, double* out, void* stream) {
  static const char* who = "phf_diagnostics_reduce";
  Layout lay;
  int rc = check_shape(who, num_problems, num_columns, num_chains, total_rows, lags, &lay);
  if (rc != PHF_OK) return rc;
  if (!workspace || !out) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_diagnostics_reduce: null pointer");
  if ((rc = phf_check_workspace(who, "diagnostics", workspace, workspace_bytes, workspace_bytes_of(num_problems, num_columns, num_chains, lay))) != PHF_OK)
    return rc;
  DiagArgs a = {};
  a.Q = num_problems; a.C = num_chains; a.cols = num_columns; a.lay = lay; a.ws = const_cast<double*>(workspace); a.out = out;
  a.units = (int64_t)num_problems * num_columns * (lay.L + 2);
  hipLaunchKernelGGL(diag_reduce_kernel, dim3(blocks_for(a.units, kWaves)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  return phf_check_launch("diag_reduce_kernel");
}

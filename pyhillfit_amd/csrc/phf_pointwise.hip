// phf_pointwise.hip — pointwise log-likelihood of every data point and WAIC's streaming accumulators (include/pyhillfit_amd.h).
//
// Batch evaluators: one thread per parameter vector, serial over its problem's points (phf_pointwise.h).  They serve the tests and
// the chain-file tool (pyhillfit_amd/chain_waic.py).
//
// Streaming accumulator.  WAIC needs, per data point p and over the S draws, LSE_p = ln sum exp(l_p) and the variance of l_p.
// Per (problem, point, chain) the workspace holds, in one lane's registers while a segment's rows stream past:
//   m, s        running max and s = sum exp(l - m): online log-sum-exp (one exponential per draw: exp(-|l - m|) scales s or the new term)
//   x0, A, B    the chain's first l, A = sum (l - x0), B = sum (l - x0)^2: the variance without cancellation (l of a censored point
//               sits anywhere from -0 to -40, its spread over draws can be far below that)
// Mapping: one lane = one chain (the rows are [rows][Q][stride][C], chain fastest: a wavefront reads 512 contiguous bytes of one
// (problem, column)); one wavefront = 64 chains of one problem and a block of kPtBlock of its points, so the points are wave-uniform
// (scalar loads) and kPtBlock x 5 accumulators live in registers; the wavefronts of the other point blocks re-read the same theta
// from L1/L2.  Reduce: one wavefront per (problem, point) merges the chains in a fixed order (lane l takes chains l, l+64, ...;
// then a fixed butterfly): log-sum-exp pairs exactly, variances by Chan's formula.
//
// Deterministic: no atomics, every accumulator is produced by one lane in row order and round-trips through HBM exactly, so the
// result is bit-identical however the rows are cut into calls and whatever the launch shape.
#include <hip/hip_runtime.h>

#include "../../include/pyhillfit_amd.h"
#include "phf_host_checks.h"
#include "phf_point_block.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
static_assert(kWaves == kPtWaves, "the accumulate kernel is launched with the point-block mapping's workgroup");
constexpr int kFields = 5;              // m, s, x0, A, B

// ---- batch evaluators ------------------------------------------------------------------------------------------------------------
template <int MODEL>
__global__ __launch_bounds__(kThreads) void pw_sl_batch_kernel(const phf_pointwise_points pts, int64_t m, const int32_t* problem_index,
                                                               const double* theta, double* out) {
  PHF_MATH_TABLES_TO_LDS();
  PHF_LOGPHI_TABLE_TO_LDS();
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  const int q = problem_index[i];
  double* o = out + (size_t)i * pts.stride;
  if (q < 0 || q >= pts.num_problems) {
    for (int p = 0; p < pts.stride; ++p) o[p] = PHF_NAN;
    return;
  }
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  const double pic50 = theta[i], hill = MODEL == 2 ? theta[(size_t)m + i] : 1.0, sigma = theta[(size_t)MODEL * m + i];
  const double ln_ic50 = PHF_LN10 * (6.0 - pic50);
  const phf_pw_sigma sg = phf_pw_sigma_terms(sigma, k_log);
  const size_t row = (size_t)q * pts.stride;
  const int n = clamp_count(pts.count[q], pts.stride);
  for (int p = 0; p < pts.stride; ++p)
    o[p] = p < n ? phf_pw_sl_point(MODEL, pts.ln_conc[row + p], pts.response[row + p], clamp_tag(pts.tag[row + p], 2), hill, ln_ic50, sg, k_exp)
                 : PHF_NAN;
}

__global__ __launch_bounds__(kThreads) void pw_hier_batch_kernel(const phf_pointwise_points pts, int ne, int64_t m, const int32_t* problem_index,
                                                                 const double* theta, double* out) {
  PHF_MATH_TABLES_TO_LDS();
  PHF_ERFC_TABLE_TO_LDS();
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  const int q = problem_index[i];
  double* o = out + (size_t)i * pts.stride;
  if (q < 0 || q >= pts.num_problems) {
    for (int p = 0; p < pts.stride; ++p) o[p] = PHF_NAN;
    return;
  }
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  const phf_pw_sigma sg = phf_pw_sigma_terms(theta[(size_t)(4 + 2 * ne) * m + i], k_log);
  const size_t row = (size_t)q * pts.stride;
  const int n = clamp_count(pts.count[q], pts.stride);
  for (int p = 0; p < pts.stride; ++p) {
    if (p >= n) { o[p] = PHF_NAN; continue; }
    const int e = clamp_tag(pts.tag[row + p], ne - 1);
    const double ln_ic50 = PHF_LN10 * (6.0 - theta[(size_t)(4 + 2 * e) * m + i]);
    o[p] = phf_pw_hier_point(pts.ln_conc[row + p], pts.response[row + p], theta[(size_t)(5 + 2 * e) * m + i], ln_ic50, sg, k_exp, k_log);
  }
}

// ---- streaming accumulator -------------------------------------------------------------------------------------------------------
struct WaicArgs {
  phf_pointwise_points pts;
  const double* rows;             // [nr][Q][stride][C]
  int64_t nr, first_row, total_rows;
  int32_t Q, stride_cols, C, ne;
  int32_t ncg, npb;               // 64-chain groups, point blocks
  int32_t units;
  double* ws;                     // [Q][pts.stride][kFields][C]
  double* out;                    // reduce: [2][Q][pts.stride]
};

// one draw l into a chain's accumulators; `first`: the chain's first draw of all
__device__ inline void waic_update(double l, bool first, double& m, double& s, double& x0, double& A, double& B, phf_ktab k_exp) {
  if (first) { m = l; s = 1.0; x0 = l; A = 0.0; B = 0.0; return; }
  const double d = l - m;
  const bool up = d > 0.0;
  const double e = phf_exp_fast_k(-__builtin_fabs(d), k_exp);      // exp(-|l - m|) (0 for a -inf draw: the clamp)
  s = up ? phf_fma(s, e, 1.0) : s + e;
  m = up ? l : m;
  const double y = l - x0;
  A += y;
  B = phf_fma(y, y, B);
}

template <int LIK>
__global__ __launch_bounds__(kThreads) void waic_accumulate_kernel(const WaicArgs a) {
  PHF_MATH_TABLES_TO_LDS();
  if (LIK == kGiven) { } else if (LIK == kHierarchical) PHF_ERFC_TABLE_TO_LDS(); else PHF_LOGPHI_TABLE_TO_LDS();
  phf_point_block b;
  if (!phf_point_block_open<LIK>(a, b)) return;
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  const size_t C = (size_t)a.C;
  double acc[kPtBlock][kFields];
  double* st = a.ws + ((size_t)b.q * a.pts.stride + b.p0) * kFields * C + b.c;
#pragma unroll
  for (int k = 0; k < kPtBlock; ++k)
#pragma unroll
    for (int f = 0; f < kFields; ++f) acc[k][f] = k < b.np ? st[((size_t)k * kFields + f) * C] : 0.0;
  for (int64_t r = 0; r < a.nr; ++r) {
    const bool first = a.first_row + r == 0;
    phf_point_block_row<LIK>(a, b, b.xr + (size_t)r * b.rstep, k_exp, k_log, [&](int k, double l) {
      waic_update(l, first, acc[k][0], acc[k][1], acc[k][2], acc[k][3], acc[k][4], k_exp);
    });
  }
#pragma unroll
  for (int k = 0; k < kPtBlock; ++k)
    if (k < b.np) {
#pragma unroll
      for (int f = 0; f < kFields; ++f) st[((size_t)k * kFields + f) * C] = acc[k][f];
    }
}

// a summary of draws: count, mean, sum of squared deviations; running max and sum of exp(l - max)
struct Part {
  double n, mean, m2, mx, sx;
};

__device__ inline Part merge(const Part& a, const Part& b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  Part r;
  r.n = a.n + b.n;
  const double delta = b.mean - a.mean;
  r.mean = a.mean + delta * (b.n / r.n);                          // Chan, Golub & LeVeque (1979)
  r.m2 = (a.m2 + b.m2) + delta * delta * (a.n * b.n / r.n);
  r.mx = a.mx > b.mx ? a.mx : b.mx;
  r.sx = r.mx == -PHF_INF ? a.sx + b.sx : a.sx * exp(a.mx - r.mx) + b.sx * exp(b.mx - r.mx);
  return r;
}

// out[0][q][p] = LSE over all chains' draws, out[1][q][p] = their variance (divisor S - 1); one wavefront per (problem, point)
__global__ __launch_bounds__(kThreads) void waic_reduce_kernel(const WaicArgs a) {
  const int64_t unit = (int64_t)blockIdx.x * kWaves + threadIdx.x / 64;
  if (unit >= a.units) return;
  const int lane = threadIdx.x & 63;
  const int ps = a.pts.stride;
  const int q = (int)(unit / ps), p = (int)(unit % ps);
  const size_t C = (size_t)a.C;
  const double* st = a.ws + (size_t)unit * kFields * C;
  const double N = (double)a.total_rows;
  Part acc = {0.0, 0.0, 0.0, -PHF_INF, 0.0};
  for (int c = lane; c < a.C; c += 64) {
    const double A = st[3 * C + c], B = st[4 * C + c];              // fields: m, s, x0, A, B
    const double am = A / N;
    const Part one = {N, st[2 * C + c] + am, B - A * am, st[c], st[C + c]};
    acc = merge(acc, one);
  }
  for (int o = 32; o > 0; o >>= 1) {
    Part other;
    other.n = __shfl_xor(acc.n, o, 64);
    other.mean = __shfl_xor(acc.mean, o, 64);
    other.m2 = __shfl_xor(acc.m2, o, 64);
    other.mx = __shfl_xor(acc.mx, o, 64);
    other.sx = __shfl_xor(acc.sx, o, 64);
    acc = (lane & o) ? merge(other, acc) : merge(acc, other);       // the lower lane's part first: the same order on both partners
  }
  if (lane == 0) {
    const size_t at = (size_t)q * ps + p;
    const size_t plane = (size_t)a.Q * ps;
    a.out[at] = acc.mx + log(acc.sx);
    a.out[plane + at] = acc.m2 / (acc.n - 1.0);
  }
}

int check_shape(const char* who, int num_problems, int stride, int num_chains, int64_t total_rows) {
  const int rc = phf_check_positive(who, "num_problems, stride and num_chains", {num_problems, stride, num_chains});
  if (rc != PHF_OK) return rc;
  if (total_rows < 1) return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: total_rows must be positive (got %lld)", who, (long long)total_rows);
  const double units = (double)num_problems * ((num_chains + 63) / 64) * ((stride + kPtBlock - 1) / kPtBlock);
  return phf_check_grid(who, {units, (double)num_problems * stride});
}

size_t workspace_bytes_of(int num_problems, int stride, int num_chains) {
  return (size_t)num_problems * stride * kFields * (size_t)num_chains * sizeof(double);
}

}  // namespace

extern "C" int phf_pointwise_loglik_single_level(const phf_pointwise_points* pts, int model, int64_t m, const int32_t* problem_index,
                                                 const double* theta, double* out, void* stream) {
  static const char* who = "phf_pointwise_loglik_single_level";
  int rc = phf_check_points(who, pts, 0, 0);
  if (rc != PHF_OK) return rc;
  if (model != 1 && model != 2) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_pointwise_loglik_single_level: model must be 1 or 2");
  if (m < 0 || (m > 0 && (!problem_index || !theta || !out)))
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_pointwise_loglik_single_level: m must be >= 0 and the arrays non-null");
  if (m == 0) return PHF_OK;
  const dim3 grid(blocks_for(m, kThreads)), block(kThreads);
  if (model == 1) hipLaunchKernelGGL(pw_sl_batch_kernel<1>, grid, block, 0, (hipStream_t)stream, *pts, m, problem_index, theta, out);
  else hipLaunchKernelGGL(pw_sl_batch_kernel<2>, grid, block, 0, (hipStream_t)stream, *pts, m, problem_index, theta, out);
  return phf_check_launch(who);
}

extern "C" int phf_pointwise_loglik_hierarchical(const phf_pointwise_points* pts, int num_expts, int64_t m, const int32_t* problem_index,
                                                 const double* theta, double* out, void* stream) {
  static const char* who = "phf_pointwise_loglik_hierarchical";
  int rc = phf_check_points(who, pts, 0, 0);
  if (rc != PHF_OK) return rc;
  if (num_expts < 1) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_pointwise_loglik_hierarchical: num_expts must be positive");
  if (m < 0 || (m > 0 && (!problem_index || !theta || !out)))
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_pointwise_loglik_hierarchical: m must be >= 0 and the arrays non-null");
  if (m == 0) return PHF_OK;
  hipLaunchKernelGGL(pw_hier_batch_kernel, dim3(blocks_for(m, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, *pts, num_expts, m,
                     problem_index, theta, out);
  return phf_check_launch(who);
}

extern "C" size_t phf_waic_workspace_bytes(int num_problems, int stride, int num_chains, int64_t total_rows) {
  if (check_shape("phf_waic_workspace_bytes", num_problems, stride, num_chains, total_rows) != PHF_OK) return 0;
  return workspace_bytes_of(num_problems, stride, num_chains);
}

extern "C" int phf_waic_init(int num_problems, int stride, int num_chains, int64_t total_rows, double* workspace, size_t workspace_bytes,
                             void* stream) {
  static const char* who = "phf_waic_init";
  const int rc = check_shape(who, num_problems, stride, num_chains, total_rows);
  if (rc != PHF_OK) return rc;
  const size_t need = workspace_bytes_of(num_problems, stride, num_chains);
  return phf_init_workspace(who, "waic", workspace, workspace_bytes, need, need, stream);
}

namespace {

// phf_waic_accumulate and phf_waic_accumulate_given (likelihood == kGiven): one validation, one launch
int waic_accumulate(const char* who, const phf_pointwise_points* pts, int likelihood, int num_expts, const double* rows, int64_t num_rows,
                    int num_problems, int row_stride_cols, int num_chains, int64_t first_row, int64_t total_rows, double* workspace,
                    size_t workspace_bytes, void* stream) {
  int rc = phf_check_points(who, pts, num_problems, 0);
  if (rc != PHF_OK) return rc;
  if ((rc = check_shape(who, num_problems, pts->stride, num_chains, total_rows)) != PHF_OK) return rc;
  if (likelihood != kGiven && (rc = phf_check_likelihood(who, likelihood, num_expts)) != PHF_OK) return rc;   // phf_waic_accumulate's own codes
  const int cols = likelihood == kGiven ? pts->stride : likelihood == kHierarchical ? 5 + 2 * num_expts : likelihood + 1;
  if ((rc = phf_check_row_stride(who, row_stride_cols, cols, "is smaller than the columns the likelihood reads")) != PHF_OK) return rc;
  if ((rc = phf_check_row_window(who, num_rows, first_row, total_rows)) != PHF_OK) return rc;
  if (!rows || !workspace) return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
  if ((rc = phf_check_workspace(who, "waic", workspace, workspace_bytes, workspace_bytes_of(num_problems, pts->stride, num_chains))) != PHF_OK)
    return rc;
  if (num_rows == 0) return PHF_OK;
  WaicArgs a = {};
  a.pts = *pts; a.rows = rows; a.nr = num_rows; a.first_row = first_row; a.total_rows = total_rows;
  a.Q = num_problems; a.stride_cols = row_stride_cols; a.C = num_chains; a.ne = num_expts; a.ws = workspace;
  a.ncg = (num_chains + 63) / 64; a.npb = (pts->stride + kPtBlock - 1) / kPtBlock;
  a.units = num_problems * a.ncg * a.npb;
  const dim3 grid(blocks_for(a.units, kWaves)), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (likelihood == 1) hipLaunchKernelGGL(waic_accumulate_kernel<1>, grid, block, 0, s, a);
  else if (likelihood == 2) hipLaunchKernelGGL(waic_accumulate_kernel<2>, grid, block, 0, s, a);
  else if (likelihood == kHierarchical) hipLaunchKernelGGL(waic_accumulate_kernel<kHierarchical>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(waic_accumulate_kernel<kGiven>, grid, block, 0, s, a);
  return phf_check_launch("waic_accumulate_kernel");
}

}  // namespace

extern "C" int phf_waic_accumulate(const phf_pointwise_points* pts, int likelihood, int num_expts, const double* rows, int64_t num_rows,
                                   int num_problems, int row_stride_cols, int num_chains, int64_t first_row, int64_t total_rows,
                                   double* workspace, size_t workspace_bytes, void* stream) {
  // the sibling's code is not this entry's to take: 0 fails the range check inside, after the points and the shape as before
  return waic_accumulate("phf_waic_accumulate", pts, likelihood == kGiven ? 0 : likelihood, num_expts, rows, num_rows, num_problems, row_stride_cols, num_chains, first_row, total_rows,
                         workspace, workspace_bytes, stream);
}

extern "C" int phf_waic_accumulate_given(const phf_pointwise_points* pts, const double* rows, int64_t num_rows, int num_problems,
                                         int row_stride_cols, int num_chains, int64_t first_row, int64_t total_rows, double* workspace,
                                         size_t workspace_bytes, void* stream) {
  return waic_accumulate("phf_waic_accumulate_given", pts, kGiven, 0, rows, num_rows, num_problems, row_stride_cols, num_chains, first_row,
                         total_rows, workspace, workspace_bytes, stream);
}

extern "C" int phf_waic_reduce(int num_problems, int stride, int num_chains, int64_t total_rows, const double* workspace,
                               size_t workspace_bytes, double* out, void* stream) {
  static const char* who = "phf_waic_reduce";
  int rc = check_shape(who, num_problems, stride, num_chains, total_rows);
  if (rc != PHF_OK) return rc;
  if (!workspace || !out) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_waic_reduce: null pointer");
  if ((rc = phf_check_workspace(who, "waic", workspace, workspace_bytes, workspace_bytes_of(num_problems, stride, num_chains))) != PHF_OK) return rc;
  WaicArgs a = {};
  a.pts.stride = stride; a.Q = num_problems; a.C = num_chains; a.total_rows = total_rows; a.ws = const_cast<double*>(workspace);
  a.out = out;
  a.units = num_problems * stride;
  hipLaunchKernelGGL(waic_reduce_kernel, dim3(blocks_for(a.units, kWaves)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  return phf_check_launch("waic_reduce_kernel");
}

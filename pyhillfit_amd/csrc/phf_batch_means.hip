// phf_batch_means.hip — ESS and MCSE beyond the lag limit: batch means on a dyadic ladder of batch sizes for every
// (problem, column, chain), accumulated while the rows stream past (the routine itself: phf_batch_means.h; the estimator on the
// host: pyhillfit_amd/batch_means.py; DESIGN.md §3, "ESS beyond the lag limit").
//
// Accumulate kernel: one lane = one chain, a wavefront = 64 chains of one (problem, column); the rows are [rows][Q][stride][C], chain
// fastest, so a wavefront reads 512 contiguous bytes per row and the state (chain fastest as well) moves in the same lines.  Aligned
// groups of 32 rows are unrolled: levels 0..4 and their pending sums sit in registers under compile-time indices, levels >= 5 are
// touched in HBM once per 32 rows; the unaligned head and tail of a sub-segment go row by row against HBM.  The host cuts a segment
// at the half-chain boundary, so a launch sees rows of one half-chain only.  No atomics, no LDS, no cross-lane traffic; every
// accumulator round-trips through HBM exactly, so the state is bit-identical however the rows are cut into calls.
//
// Reduce kernel: one wavefront per (problem, column, level with n_l = floor(h / 2^l) >= 2 batches), plus one per (problem, column) for
// the half-chain means.  Lane l adds chains l, l + 64, ... (half 0's term, then half 1's), then a fixed butterfly (xor 32, 16, .., 1).
#include <hip/hip_runtime.h>

#include "../../include/pyhillfit_amd.h"
#include "phf_batch_means.h"
#include "phf_host_checks.h"
#include "phf_device_util.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct BmArgs {
  const double* rows;             // first row of this sub-segment: [nr][Q][stride][C]
  int64_t nr;                     // rows in this sub-segment (all in one half-chain)
  int64_t m0;                     // half-chain index of its first row
  int64_t h;
  int32_t Q, stride, C, cols, nl, half, ncg;
  int64_t units;
  double* ws;                     // [Q][cols][5 nl + 2][C]
  double* out;                    // reduce: [Q][cols][nl + 1]
};

__global__ __launch_bounds__(kThreads) void batch_means_accumulate_kernel(const BmArgs a) {
  const int64_t unit = (int64_t)blockIdx.x * kWaves + threadIdx.x / 64;
  if (unit >= a.units) return;
  const int cg = (int)(unit % a.ncg);
  const int64_t qj = unit / a.ncg;
  const int j = (int)(qj % a.cols), q = (int)(qj / a.cols);
  const int c = cg * 64 + (threadIdx.x & 63);
  if (c >= a.C) return;
  const size_t rstep = (size_t)a.Q * a.stride * a.C;
  const double* xr = a.rows + ((size_t)q * a.stride + j) * a.C + c;
  double* st = a.ws + (size_t)qj * PHF_BM_FIELDS(a.nl) * a.C + c;
  phf_bm_rows(xr, rstep, a.nr, a.m0, a.half, st, (size_t)a.C, a.nl);
}

// out[q][j][l] = mean over the 2C half-chains of the variance of the batch means of level l, l = 0..nl-2 (l = 0: W);
// out[q][j][nl-1] = mean of the half-chain means; out[q][j][nl] = their variance (divisor 2C - 1) = B/h
__global__ __launch_bounds__(kThreads) void batch_means_reduce_kernel(const BmArgs a) {
  const int64_t unit = (int64_t)blockIdx.x * kWaves + threadIdx.x / 64;
  if (unit >= a.units) return;
  const int lane = threadIdx.x & 63;
  const int nl = a.nl;
  const int k = (int)(unit % nl);
  const int64_t qj = unit / nl;
  const double* st = a.ws + (size_t)qj * PHF_BM_FIELDS(nl) * a.C;
  const size_t C = (size_t)a.C;
  const double M = 2.0 * a.C;
  double* o = a.out + (size_t)qj * (nl + 1);
  if (k < nl - 1) {
    const double n = (double)(a.h >> k), b = (double)((int64_t)1 << k);
    double s = 0.0;
    for (int c = lane; c < a.C; c += 64) {
      const double v0 = phf_bm_block_mean_variance(st[(size_t)phf_bm_s1(nl, 0, k) * C + c], st[(size_t)phf_bm_s2(nl, 0, k) * C + c], n, b);
      const double v1 = phf_bm_block_mean_variance(st[(size_t)phf_bm_s1(nl, 1, k) * C + c], st[(size_t)phf_bm_s2(nl, 1, k) * C + c], n, b);
      s += v0 + v1;
    }
    s = wave_sum(s);
    if (lane == 0) o[k] = s / M;
  } else {
    const double hd = (double)a.h;
    double s = 0.0;
    for (int c = lane; c < a.C; c += 64) {
      const double m0 = st[(size_t)phf_bm_x0(0) * C + c] + st[(size_t)phf_bm_s1(nl, 0, 0) * C + c] / hd;
      const double m1 = st[(size_t)phf_bm_x0(1) * C + c] + st[(size_t)phf_bm_s1(nl, 1, 0) * C + c] / hd;
      s += m0 + m1;
    }
    const double mean = wave_sum(s) / M;
    double v = 0.0;
    for (int c = lane; c < a.C; c += 64) {
      const double d0 = st[(size_t)phf_bm_x0(0) * C + c] + st[(size_t)phf_bm_s1(nl, 0, 0) * C + c] / hd - mean;
      const double d1 = st[(size_t)phf_bm_x0(1) * C + c] + st[(size_t)phf_bm_s1(nl, 1, 0) * C + c] / hd - mean;
      v += d0 * d0 + d1 * d1;
    }
    v = wave_sum(v);
    if (lane == 0) { o[nl - 1] = mean; o[nl] = v / (M - 1.0); }
  }
}

// shared argument checks of the four entries; on success *nl = floor(log2 h) + 1
int check_shape(const char* who, int num_problems, int num_columns, int num_chains, int64_t total_rows, int* nl) {
  int rc = phf_check_positive(who, "num_problems, num_columns and num_chains", {num_problems, num_columns, num_chains});
  if (rc != PHF_OK) return rc;
  if (total_rows < 4)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: a half-chain needs h = floor(total_rows / 2) >= 2 rows (total_rows = %lld)", who,
                     (long long)total_rows);
  *nl = phf_bm_levels(total_rows / 2);
  const double units = (double)num_problems * num_columns * ((num_chains + 63) / 64 > *nl ? (num_chains + 63) / 64 : *nl);
  return phf_check_grid(who, {units / kWaves});
}

size_t workspace_bytes_of(int num_problems, int num_columns, int num_chains, int nl) {
  return (size_t)num_problems * num_columns * (size_t)PHF_BM_FIELDS(nl) * num_chains * sizeof(double);
}

}  // namespace

extern "C" size_t phf_batch_means_workspace_bytes(int num_problems, int num_columns, int num_chains, int64_t total_rows) {
  int nl;
  if (check_shape("phf_batch_means_workspace_bytes", num_problems, num_columns, num_chains, total_rows, &nl) != PHF_OK) return 0;
  return workspace_bytes_of(num_problems, num_columns, num_chains, nl);
}

extern "C" int phf_batch_means_levels(int64_t total_rows) {
  if (total_rows < 4) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_batch_means_levels: need total_rows >= 4");
  return phf_bm_levels(total_rows / 2);
}

extern "C" int phf_batch_means_init(int num_problems, int num_columns, int num_chains, int64_t total_rows, double* workspace,
                                    size_t workspace_bytes, void* stream) {
  static const char* who = "phf_batch_means_init";
  int nl;
  const int rc = check_shape(who, num_problems, num_columns, num_chains, total_rows, &nl);
  if (rc != PHF_OK) return rc;
  const size_t need = workspace_bytes_of(num_problems, num_columns, num_chains, nl);
  return phf_init_workspace(who, "batch_means", workspace, workspace_bytes, need, need, stream);
}

extern "C" int phf_batch_means_accumulate(const double* rows, int64_t num_rows, int num_problems, int row_stride_cols, int num_chains,
                                          int num_columns, int64_t first_row, int64_t total_rows, double* workspace,
                                          size_t workspace_bytes, void* stream) {
  static const char* who = "phf_batch_means_accumulate";
  int nl;
  int rc = check_shape(who, num_problems, num_columns, num_chains, total_rows, &nl);
  if (rc != PHF_OK) return rc;
  if ((rc = phf_check_row_window(who, num_rows, first_row, total_rows)) != PHF_OK) return rc;
  if ((rc = phf_check_row_stride(who, row_stride_cols, num_columns, "must be >= num_columns")) != PHF_OK) return rc;
  if (!rows || !workspace) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_batch_means_accumulate: null pointer");
  if ((rc = phf_check_workspace(who, "batch_means", workspace, workspace_bytes, workspace_bytes_of(num_problems, num_columns, num_chains, nl))) != PHF_OK)
    return rc;
  if (num_rows == 0) return PHF_OK;
  BmArgs a = {};
  a.Q = num_problems; a.stride = row_stride_cols; a.C = num_chains; a.cols = num_columns; a.nl = nl; a.ws = workspace;
  a.h = total_rows / 2;
  a.ncg = (num_chains + 63) / 64;
  a.units = (int64_t)num_problems * num_columns * a.ncg;
  const size_t row_doubles = (size_t)num_problems * row_stride_cols * num_chains;
  for (int half = 0; half < 2; ++half) {
    phf_half_segment seg;
    if (!phf_half_cut(total_rows, first_row, num_rows, half, &seg)) continue;
    a.rows = rows + (size_t)seg.offset * row_doubles;
    a.nr = seg.nr; a.m0 = seg.m0; a.half = half;
    hipLaunchKernelGGL(batch_means_accumulate_kernel, dim3(blocks_for(a.units, kWaves)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    if ((rc = phf_check_launch("batch_means_accumulate_kernel")) != PHF_OK) return rc;
  }
  return PHF_OK;
}

extern "C" int phf_batch_means_reduce(int num_problems, int num_columns, int num_chains, int64_t total_rows, const double* workspace,
                                      size_t workspace_bytes, double* out, void* stream) {
  static const char* who = "phf_batch_means_reduce";
  int nl;
  int rc = check_shape(who, num_problems, num_columns, num_chains, total_rows, &nl);
  if (rc != PHF_OK) return rc;
  if (!workspace || !out) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_batch_means_reduce: null pointer");
  if ((rc = phf_check_workspace(who, "batch_means", workspace, workspace_bytes, workspace_bytes_of(num_problems, num_columns, num_chains, nl))) != PHF_OK)
    return rc;
  BmArgs a = {};
  a.Q = num_problems; a.C = num_chains; a.cols = num_columns; a.nl = nl; a.h = total_rows / 2;
  a.ws = const_cast<double*>(workspace); a.out = out;
  a.units = (int64_t)num_problems * num_columns * nl;
  hipLaunchKernelGGL(batch_means_reduce_kernel, dim3(blocks_for(a.units, kWaves)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  return phf_check_launch("batch_means_reduce_kernel");
}

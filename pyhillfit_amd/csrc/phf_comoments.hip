// phf_comoments.hip — the co-moments of the parameter columns per half-chain, accumulated while the rows stream past, and their
// reduction to the within- and between-chain covariance matrices W and B/h (posterior correlations, multivariate R-hat:
// pyhillfit_amd/correlations.py).  The state, the operation order and the reduction order are phf_comoments.h's; the host build of
// that header is the twin these kernels are held to, bit for bit.
//
// Mapping.  Accumulate: one lane = one chain (the rows are [rows][Q][stride][C], chain fastest: a wavefront reads 512 contiguous
// bytes of one (problem, column)); one wavefront = (problem, block of 64 chains, tile (bi <= bj) of T x T column pairs).  The tile's
// accumulators stay in registers across the call's row loop; a row costs the tile 2T loads (T on the diagonal) for T^2 fmas.  The
// diagonal tiles also own S, x0 and the non-finite flag of their columns (the flag is only ever stored as 1.0, so tiles cannot
// disagree), tile (0, 0) the row count.  The four wavefronts of a workgroup are consecutive tiles of the same rows: their re-reads
// are L1/L2 hits.  d <= 4 (single-level) is one T = 4 diagonal tile: every row is read once, d (d + 1) / 2 + d accumulators in one
// lane.  Larger d (hierarchical) takes T = 8: 64 accumulators = 128 VGPRs.  Columns past d in a ragged last tile are neither loaded
// nor stored (wave-uniform guards).  Reduce: one wavefront per (problem, i <= j) and one per (problem, i).
//
// Deterministic: no atomics, every accumulator is one sequential chain of operations in row order and round-trips through HBM
// exactly, so the result is bit-identical however the rows are cut into calls and whatever the tile and launch shape.  fp64 VALU
// with explicit fma, no MFMA: a matrix instruction's internal summation order cannot be restated on the host.
#include <hip/hip_runtime.h>

#include "../../include/pyhillfit_amd.h"
#include "phf_host_checks.h"
#include "phf_comoments.h"
#include "phf_device_util.h"

#define PHF_CM_UNROLL _Pragma("unroll")

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSmallTile = 4;      // d <= 4: one diagonal tile
constexpr int kTile = 8;
constexpr int kMaxColumns = 1024;

struct CmArgs {
  const double* rows;             // first row of this sub-segment: [nr][Q][stride][C]
  int64_t nr;                     // rows in this sub-segment (all in one half-chain)
  int64_t m0;                     // half-chain index of its first row
  int64_t h;
  int32_t Q, stride, C, d, half;
  int32_t ncg, nb, ntile;         // 64-chain groups, column blocks, tiles (bi <= bj)
  int64_t units;
  double* ws;                     // [Q][2][F][C]
  double* out;                    // reduce: [Q][PHF_CM_OUT_DOUBLES(d)]
};

template <int T, bool DIAG>
__device__ __forceinline__ void cm_tile(const CmArgs& a, int q, int c, int bi, int bj) {
  const int d = a.d, i0 = bi * T, j0 = bj * T;
  const int ni = d - i0 < T ? d - i0 : T, nj = d - j0 < T ? d - j0 : T;
  const size_t C = (size_t)a.C, rstep = (size_t)a.Q * a.stride * C;
  const double* xr = a.rows + (size_t)q * a.stride * C + c;
  double* st = a.ws + ((size_t)q * 2 + a.half) * PHF_CM_FIELDS(d) * C + c;
  const bool fresh = a.m0 == 0;

  double x0i[T], x0j[T], s[T], acc[T][T];
  PHF_CM_UNROLL
  for (int u = 0; u < T; ++u) {
    x0i[u] = u < ni ? (fresh ? xr[(size_t)(i0 + u) * C] : st[(size_t)phf_cm_x0(i0 + u) * C]) : 0.0;
    x0j[u] = (!DIAG && u < nj) ? (fresh ? xr[(size_t)(j0 + u) * C] : st[(size_t)phf_cm_x0(j0 + u) * C]) : 0.0;
    s[u] = (DIAG && !fresh && u < ni) ? st[(size_t)phf_cm_s(d, i0 + u) * C] : 0.0;
    PHF_CM_UNROLL
    for (int v = 0; v < T; ++v)
      acc[u][v] = (!fresh && u < ni && v < nj && (!DIAG || u <= v)) ? st[(size_t)phf_cm_p(d, phf_cm_pair(d, i0 + u, j0 + v)) * C] : 0.0;
  }
  bool bad = false;
  for (int64_t r = 0; r < a.nr; ++r) {
    const double* x = xr + (size_t)r * rstep;
    double yi[T], yj[T];
    PHF_CM_UNROLL
    for (int u = 0; u < T; ++u) {
      yi[u] = u < ni ? x[(size_t)(i0 + u) * C] - x0i[u] : 0.0;
      yj[u] = DIAG ? yi[u] : (u < nj ? x[(size_t)(j0 + u) * C] - x0j[u] : 0.0);
    }
    if (DIAG) {
      PHF_CM_UNROLL
      for (int u = 0; u < T; ++u) {
        s[u] = phf_cm_add(s[u], yi[u]);
        bad |= !phf_cm_finite(yi[u]);
      }
    }
    PHF_CM_UNROLL
    for (int u = 0; u < T; ++u) {
      PHF_CM_UNROLL
      for (int v = 0; v < T; ++v)
        if (!DIAG || u <= v) acc[u][v] = phf_cm_mad(acc[u][v], yi[u], yj[v]);
    }
  }
  PHF_CM_UNROLL
  for (int u = 0; u < T; ++u) {
    if (u < ni) {
      if (DIAG) {
        if (fresh) st[(size_t)phf_cm_x0(i0 + u) * C] = x0i[u];
        st[(size_t)phf_cm_s(d, i0 + u) * C] = s[u];
      }
      PHF_CM_UNROLL
      for (int v = 0; v < T; ++v)
        if (v < nj && (!DIAG || u <= v)) st[(size_t)phf_cm_p(d, phf_cm_pair(d, i0 + u, j0 + v)) * C] = acc[u][v];
    }
  }
  if (DIAG) {
    if (bi == 0) st[(size_t)phf_cm_rows(d) * C] = (double)(a.m0 + a.nr);
    if (bad) st[(size_t)phf_cm_flag(d) * C] = 1.0;
  }
}

template <int T>
__global__ __launch_bounds__(kThreads) void cm_accumulate_kernel(const CmArgs a) {
  const int64_t unit = (int64_t)blockIdx.x * kWaves + threadIdx.x / 64;
  if (unit >= a.units) return;
  const int t = (int)(unit % a.ntile);
  const int64_t rest = unit / a.ntile;
  const int cg = (int)(rest % a.ncg), q = (int)(rest / a.ncg);
  const int c = cg * 64 + (threadIdx.x & 63);
  if (c >= a.C) return;
  int bi = 0, left = t;                                   // tile t of the row-major upper triangle of nb x nb blocks
  while (left >= a.nb - bi) { left -= a.nb - bi; ++bi; }
  const int bj = bi + left;
  if (bi == bj) cm_tile<T, true>(a, q, c, bi, bj);
  else cm_tile<T, false>(a, q, c, bi, bj);
}

__device__ inline int wave_sum_int(int v) {
  PHF_CM_UNROLL
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ inline int wave_min_int(int v) {
  PHF_CM_UNROLL
  for (int o = 32; o > 0; o >>= 1) {
    const int w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}

// one wavefront per (problem, pair i <= j): W_ij and (B/h)_ij; one per (problem, i): the grand mean and T_i; that of i = 0 the tail
__global__ __launch_bounds__(kThreads) void cm_reduce_kernel(const CmArgs a) {
  const int64_t unit = (int64_t)blockIdx.x * kWaves + threadIdx.x / 64;
  if (unit >= a.units) return;
  const int lane = threadIdx.x & 63;
  const int d = a.d, np = PHF_CM_PAIRS(d), per = np + d;
  const int u = (int)(unit % per);
  const int64_t q = unit / per;
  const double* wsq = a.ws + (size_t)q * 2 * PHF_CM_FIELDS(d) * a.C;
  double* o = a.out + (size_t)q * PHF_CM_OUT_DOUBLES(d);
  const double h = (double)a.h;
  int n, k0;
  phf_cm_lane_used(wsq, a.C, d, lane, &n, &k0);
  const int m = wave_sum_int(n), first = wave_min_int(k0);
  if (u < np) {
    int i = 0, left = u;
    while (left >= d - i) { left -= d - i; ++i; }
    const int j = i + left;
    const double refi = m >= 1 ? phf_cm_mean_of(wsq, a.C, d, h, first, i) : 0.0;
    const double refj = m >= 1 ? phf_cm_mean_of(wsq, a.C, d, h, first, j) : 0.0;
    double sums[4];
    phf_cm_lane_pair(wsq, a.C, d, h, i, j, refi, refj, lane, sums);
    PHF_CM_UNROLL
    for (int k = 0; k < 4; ++k) sums[k] = wave_sum(sums[k]);
    double w, bh;
    phf_cm_finish_pair(sums, m, &w, &bh);
    if (lane == 0) { o[u] = w; o[np + u] = bh; }
  } else {
    const int i = u - np;
    const double refi = m >= 1 ? phf_cm_mean_of(wsq, a.C, d, h, first, i) : 0.0;
    const double t = wave_sum(phf_cm_lane_mean(wsq, a.C, d, h, i, refi, lane));
    if (lane == 0) {
      o[2 * np + i] = phf_cm_finish_mean(refi, t, m);
      o[2 * np + d + i] = t;
      if (i == 0) {
        o[2 * np + 2 * d] = (double)m;
        o[2 * np + 2 * d + 1] = (double)(2 * a.C - m);
        o[2 * np + 2 * d + 2] = h;
        o[2 * np + 2 * d + 3] = 0.0;
      }
    }
  }
}

int tile_edge(int d) { return d <= kSmallTile ? kSmallTile : kTile; }

// shared argument checks of the four entries
int check_shape(const char* who, int num_problems, int num_columns, int num_chains, int64_t total_rows) {
  int rc = phf_check_positive(who, "num_problems, num_columns and num_chains", {num_problems, num_columns, num_chains});
  if (rc != PHF_OK) return rc;
  if (num_columns > kMaxColumns) return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: at most %d columns (got %d)", who, kMaxColumns, num_columns);
  if (total_rows < 2 * PHF_CM_MIN_HALF)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: a half-chain needs h = floor(total_rows / 2) >= 4 rows (total_rows = %lld)", who,
                     (long long)total_rows);
  const int nb = (num_columns + tile_edge(num_columns) - 1) / tile_edge(num_columns);
  const double tiles = (double)num_problems * ((num_chains + 63) / 64) * (nb * (nb + 1) / 2);
  const double reduce_units = (double)num_problems * (PHF_CM_PAIRS(num_columns) + num_columns);
  return phf_check_grid(who, {tiles / kWaves, reduce_units / kWaves});
}

size_t workspace_bytes_of(int num_problems, int num_columns, int num_chains) {
  return (size_t)num_problems * 2 * (size_t)PHF_CM_FIELDS(num_columns) * num_chains * sizeof(double);
}

}  // namespace

extern "C" size_t phf_comoments_workspace_bytes(int num_problems, int num_columns, int num_chains, int64_t total_rows) {
  if (check_shape("phf_comoments_workspace_bytes", num_problems, num_columns, num_chains, total_rows) != PHF_OK) return 0;
  return workspace_bytes_of(num_problems, num_columns, num_chains);
}

extern "C" int phf_comoments_init(int num_problems, int num_columns, int num_chains, int64_t total_rows, double* workspace,
                                  size_t workspace_bytes, void* stream) {
  static const char* who = "phf_comoments_init";
  const int rc = check_shape(who, num_problems, num_columns, num_chains, total_rows);
  if (rc != PHF_OK) return rc;
  const size_t need = workspace_bytes_of(num_problems, num_columns, num_chains);
  return phf_init_workspace(who, "comoments", workspace, workspace_bytes, need, need, stream);
}

extern "C" int phf_comoments_accumulate(const double* rows, int64_t num_rows, int num_problems, int row_stride_cols, int num_chains,
                                        int num_columns, int64_t first_row, int64_t total_rows, double* workspace, size_t workspace_bytes,
                                        void* stream) {
  static const char* who = "phf_comoments_accumulate";
  int rc = check_shape(who, num_problems, num_columns, num_chains, total_rows);
  if (rc != PHF_OK) return rc;
  if ((rc = phf_check_row_window(who, num_rows, first_row, total_rows)) != PHF_OK) return rc;
  if ((rc = phf_check_row_stride(who, row_stride_cols, num_columns, "must be >= num_columns")) != PHF_OK) return rc;
  if (!rows || !workspace) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_comoments_accumulate: null pointer");
  if ((rc = phf_check_workspace(who, "comoments", workspace, workspace_bytes, workspace_bytes_of(num_problems, num_columns, num_chains))) != PHF_OK)
    return rc;
  if (num_rows == 0) return PHF_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  CmArgs a = {};
  a.Q = num_problems; a.stride = row_stride_cols; a.C = num_chains; a.d = num_columns; a.ws = workspace; a.h = total_rows / 2;
  const int T = tile_edge(num_columns);
  a.ncg = (num_chains + 63) / 64; a.nb = (num_columns + T - 1) / T; a.ntile = a.nb * (a.nb + 1) / 2;
  a.units = (int64_t)num_problems * a.ncg * a.ntile;
  const size_t row_doubles = (size_t)num_problems * row_stride_cols * num_chains;
  for (int half = 0; half < 2; ++half) {
    phf_half_segment seg;
    if (!phf_half_cut(total_rows, first_row, num_rows, half, &seg)) continue;
    a.rows = rows + (size_t)seg.offset * row_doubles;
    a.nr = seg.nr; a.m0 = seg.m0; a.half = half;
    if (T == kSmallTile) hipLaunchKernelGGL(cm_accumulate_kernel<kSmallTile>, dim3(blocks_for(a.units, kWaves)), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL(cm_accumulate_kernel<kTile>, dim3(blocks_for(a.units, kWaves)), dim3(kThreads), 0, s, a);
    if ((rc = phf_check_launch("cm_accumulate_kernel")) != PHF_OK) return rc;
  }
  return PHF_OK;
}

extern "C" int phf_comoments_reduce(int num_problems, int num_columns, int num_chains, int64_t total_rows, const double* workspace,
                                    size_t workspace_bytes, double* out, void* stream) {
  static const char* who = "phf_comoments_reduce";
  int rc = check_shape(who, num_problems, num_columns, num_chains, total_rows);
  if (rc != PHF_OK) return rc;
  if (!workspace || !out) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_comoments_reduce: null pointer");
  if ((rc = phf_check_workspace(who, "comoments", workspace, workspace_bytes, workspace_bytes_of(num_problems, num_columns, num_chains))) != PHF_OK)
    return rc;
  CmArgs a = {};
  a.Q = num_problems; a.C = num_chains; a.d = num_columns; a.ws = const_cast<double*>(workspace); a.out = out; a.h = total_rows / 2;
  a.units = (int64_t)num_problems * (PHF_CM_PAIRS(num_columns) + num_columns);
  hipLaunchKernelGGL(cm_reduce_kernel, dim3(blocks_for(a.units, kWaves)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  return phf_check_launch("cm_reduce_kernel");
}

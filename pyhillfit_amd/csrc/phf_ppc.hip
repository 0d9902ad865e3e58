// phf_ppc.hip — posterior predictive checks, streamed while the samplers' rows go past (include/pyhillfit_amd.h, DESIGN.md §3,
// "Posterior predictive checks").
//
// Per draw theta (one row of one chain) of problem q, one replicate y_rep of each of its n points (phf_ppc.h), and five test
// quantities T, each of the observed responses y and of y_rep under the same theta: the deviance -2 sum l, the mean, the sd (divisor
// n - 1), the number of zeros and of hundreds.  The workspace holds, per (problem, field, chain), a double:
//   fields 4 s + 0..3   statistic s: #{T(y_rep) > T(y)}, #{T(y_rep) = T(y)}, sum T(y_rep), sum T(y)   (counts are exact integers)
//   field  20           draws outside the likelihood's support (sigma <= 1e-3 or NaN), left out of everything else
//   field  21 + p       sum over the draws of point p's P(y_rep < y_p) + P(y_rep = y_p)/2   (the predictive PIT, analytic)
// Kernels:
//   statistics  one lane per chain (rows are [rows][Q][stride][C], chain fastest: coalesced), one wavefront per (problem, 64 chains);
//               the problem's points sit in the wavefront's slice of LDS; each lane loops over all n points of its draw (the T's
//               sum over points): pred once per (draw, point) for l(y), the replicate and l(y_rep); the T's in registers
//   PIT         WAIC's mapping: one wavefront per (problem, 64 chains, 4 points), the points wave-uniform, 4 sums in registers
//   reduce      one wavefront per (problem, field): lane l sums chains l, l + 64, ... in order, then a fixed butterfly
//   replicate   the host-callable batch evaluator: one thread per parameter vector, the same per-draw code as the statistics kernel
// Deterministic: no atomics, every sum is owned by one lane, accumulates in row order and round-trips through HBM exactly, so the
// results are bit-identical however the rows are cut into calls.  The random words depend on (chain id, problem id, row, point
// block, seed) alone: not on the cut, the launch shape, the rank or the sampler path that made the rows.
#include <hip/hip_runtime.h>

#include "../../include/pyhillfit_amd.h"
#include "phf_host_checks.h"
#include "phf_point_block.h"
#include "phf_ppc.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
static_assert(kWaves == kPtWaves, "the PIT kernel is launched with the point-block mapping's workgroup");
constexpr int kStats = PHF_PPC_STATS;
constexpr int kInvalid = 4 * kStats;    // field of the invalid-draw count
constexpr int kHead = kInvalid + 1;     // first PIT field
constexpr int kMaxStride = 512;         // points per problem: the statistics kernel's LDS (4 x 512 x 20 bytes)

template <int LIK>
__device__ inline double sigma_of(const double* x, size_t cs, int ne) {
  return x[(LIK == kHierarchical ? (size_t)(4 + 2 * ne) : (size_t)LIK) * cs];
}

__device__ inline bool valid_sigma(double s) { return s > PHF_SIGMA_FLOOR; }

// T(y) or T(y_rep) from the sums over points: sum l, sum (v - ybar), sum (v - ybar)^2, #zeros, #hundreds
__device__ inline void finish_stats(double sum_l, double s1, double s2, double zeros, double hundreds, double ybar, double inv_n,
                                    double inv_nm1, double* t) {
  t[0] = -2.0 * sum_l;
  t[1] = ybar + s1 * inv_n;
  t[2] = phf_sqrt_nonneg((s2 - (s1 * s1) * inv_n) * inv_nm1);
  t[3] = zeros;
  t[4] = hundreds;
}

// per problem: the mean of y, 1/n, 1/(n - 1) (0 for n = 1)
struct ObsConst {
  double ybar, inv_n, inv_nm1;
};

__device__ inline ObsConst obs_const(const double* yv, int n) {
  double s = 0.0;
  for (int p = 0; p < n; ++p) s += yv[p];
  ObsConst o;
  o.inv_n = phf_rcp((double)n);
  o.inv_nm1 = n > 1 ? phf_rcp((double)(n - 1)) : 0.0;
  o.ybar = s * o.inv_n;
  return o;
}

// One draw (a valid theta: x[k * cs] is column k) of a problem's n points: t_obs[5] and t_rep[5]; y_rep[p] if WRITE.
template <int LIK, bool WRITE>
__device__ __forceinline__ void ppc_draw(const double* lc, const double* yv, const int* tg, int n, const double* x, size_t cs, int ne,
                                         uint32_t cid, uint32_t pid, uint32_t row, uint32_t k0, uint32_t k1, const ObsConst& oc,
                                         phf_ktab k_exp, phf_ktab k_log, double* y_rep, double* t_obs, double* t_rep) {
  const double sigma = sigma_of<LIK>(x, cs, ne);
  const phf_pw_sigma sg = phf_pw_sigma_terms(sigma, k_log);
  const double ln_ic50 = LIK == kHierarchical ? 0.0 : PHF_LN10 * (6.0 - x[0]);
  const double hill = LIK == 2 ? x[cs] : 1.0;
  double lo = 0.0, lr = 0.0, o1 = 0.0, o2 = 0.0, oz = 0.0, oh = 0.0, r1 = 0.0, r2 = 0.0, rz = 0.0, rh = 0.0;
  const int nb = (n + 3) / 4;
  for (int b = 0; b < nb; ++b) {
    const phf_u32x4 w = phf_philox_mh(cid, pid, row, PHF_PPC_DOMAIN | (uint32_t)b, k0, k1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int p = 4 * b + k;
      if (p < n) {
        const double y = yv[p];
        double yr, l_o, l_r;
        if (LIK == kHierarchical) {
          const int e = clamp_tag(tg[p], ne - 1);
          const double li = PHF_LN10 * (6.0 - x[(size_t)(4 + 2 * e) * cs]);
          const double pred = phf_pw_pred(2, lc[p], x[(size_t)(5 + 2 * e) * cs], li, k_exp);
          const double lm = phf_log_fast_k(phf_trunc_mass(pred, sg.inv_s, k_exp), k_log);
          l_o = phf_ppc_hier_point_at(pred, y, lm, sg);
          yr = phf_ppc_rep_hier(pred, sigma, sg.inv_s, w.w[k]);
          l_r = phf_ppc_hier_point_at(pred, yr, lm, sg);
        } else {
          const double pred = phf_pw_pred(LIK, lc[p], hill, ln_ic50, k_exp);
          l_o = phf_ppc_sl_point_at(pred, y, clamp_tag(tg[p], 2), sg);
          yr = phf_ppc_rep_sl(pred, sigma, w.w[k]);
          l_r = phf_ppc_sl_point_at(pred, yr, phf_ppc_sl_tag(yr), sg);
        }
        if (WRITE) y_rep[p] = yr;
        lo += l_o;
        lr += l_r;
        const double dy = y - oc.ybar, dr = yr - oc.ybar;
        o1 += dy; o2 = phf_fma(dy, dy, o2);
        r1 += dr; r2 = phf_fma(dr, dr, r2);
        oz += y == 0.0 ? 1.0 : 0.0; oh += y == 100.0 ? 1.0 : 0.0;
        rz += yr == 0.0 ? 1.0 : 0.0; rh += yr == 100.0 ? 1.0 : 0.0;
      }
    }
  }
  finish_stats(lo, o1, o2, oz, oh, oc.ybar, oc.inv_n, oc.inv_nm1, t_obs);
  finish_stats(lr, r1, r2, rz, rh, oc.ybar, oc.inv_n, oc.inv_nm1, t_rep);
}

struct PpcArgs {
  phf_pointwise_points pts;
  const double* rows;             // [nr][Q][stride_cols][C]
  int64_t nr, first_row, total_rows;
  int32_t Q, stride_cols, C, ne;
  int32_t ncg, npb;               // 64-chain groups, point blocks (PIT)
  int32_t units;
  const uint32_t* problem_id;     // [Q]
  uint32_t chain_id_base, k0, k1;
  double* ws;                     // [Q][kHead + pts.stride][C]
};

__device__ inline size_t fields_of(int stride) { return (size_t)kHead + stride; }

// LDS slice of one wavefront: ln_conc[stride], y[stride] (doubles), tag[stride] (int32)
__host__ __device__ inline size_t slice_doubles(int stride) { return 2 * (size_t)stride + ((size_t)stride + 1) / 2; }

template <int LIK>
__global__ __launch_bounds__(kThreads) void ppc_stats_kernel(const PpcArgs a) {
  extern __shared__ double s_pts[];
  PHF_MATH_TABLES_TO_LDS();
  if (LIK == kHierarchical) {
    PHF_ERFC_TABLE_TO_LDS();
  } else {
    PHF_LOGPHI_TABLE_TO_LDS();
    PHF_NORMAL_TABLE_TO_LDS();
  }
  const int wave = threadIdx.x / 64, lane = threadIdx.x & 63;
  const int unit = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves + wave));       // wave-uniform
  const bool live = unit < a.units;
  const int ps = a.pts.stride;
  const int q = live ? unit / a.ncg : 0, cg = live ? unit % a.ncg : 0;
  const int n = live ? clamp_count(a.pts.count[q], ps) : 0;
  double* s_lc = s_pts + (size_t)wave * slice_doubles(ps);
  double* s_y = s_lc + ps;
  int* s_tg = reinterpret_cast<int*>(s_y + ps);
  for (int p = lane; p < n; p += 64) {
    const size_t at = (size_t)q * ps + p;
    s_lc[p] = a.pts.ln_conc[at];
    s_y[p] = a.pts.response[at];
    s_tg[p] = a.pts.tag[at];
  }
  __syncthreads();
  const int c = cg * 64 + lane;
  if (n == 0 || c >= a.C) return;
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  const size_t C = (size_t)a.C;
  double* st = a.ws + (size_t)q * fields_of(ps) * C + c;
  double acc[kStats][4];
#pragma unroll
  for (int s = 0; s < kStats; ++s)
#pragma unroll
    for (int f = 0; f < 4; ++f) acc[s][f] = st[(size_t)(4 * s + f) * C];
  double invalid = st[(size_t)kInvalid * C];
  const ObsConst oc = obs_const(s_y, n);
  const uint32_t cid = a.chain_id_base + (uint32_t)c, pid = a.problem_id[q];
  const size_t rstep = (size_t)a.Q * a.stride_cols * C;
  const double* xr = a.rows + (size_t)q * a.stride_cols * C + c;
  for (int64_t r = 0; r < a.nr; ++r) {
    const double* x = xr + (size_t)r * rstep;
    if (!valid_sigma(sigma_of<LIK>(x, C, a.ne))) {
      invalid += 1.0;
      continue;
    }
    double to[kStats], tr[kStats];
    ppc_draw<LIK, false>(s_lc, s_y, s_tg, n, x, C, a.ne, cid, pid, (uint32_t)(a.first_row + r), a.k0, a.k1, oc, k_exp, k_log, nullptr,
                         to, tr);
#pragma unroll
    for (int s = 0; s < kStats; ++s) {
      acc[s][0] += tr[s] > to[s] ? 1.0 : 0.0;
      acc[s][1] += tr[s] == to[s] ? 1.0 : 0.0;
      acc[s][2] += tr[s];
      acc[s][3] += to[s];
    }
  }
#pragma unroll
  for (int s = 0; s < kStats; ++s)
#pragma unroll
    for (int f = 0; f < 4; ++f) st[(size_t)(4 * s + f) * C] = acc[s][f];
  st[(size_t)kInvalid * C] = invalid;
}

template <int LIK>
__global__ __launch_bounds__(kThreads) void ppc_pit_kernel(const PpcArgs a) {
  PHF_MATH_TABLES_TO_LDS();
  if (LIK == kHierarchical) PHF_ERFC_TABLE_TO_LDS();
  phf_point_block b;
  if (!phf_point_block_open<LIK>(a, b)) return;
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  const size_t C = (size_t)a.C;
  double acc[kPtBlock];
  double* st = a.ws + ((size_t)b.q * fields_of(a.pts.stride) + kHead + b.p0) * C + b.c;
#pragma unroll
  for (int k = 0; k < kPtBlock; ++k) acc[k] = k < b.np ? st[(size_t)k * C] : 0.0;
  for (int64_t r = 0; r < a.nr; ++r) {
    const double* x = b.xr + (size_t)r * b.rstep;
    const double sigma = sigma_of<LIK>(x, C, a.ne);
    if (!valid_sigma(sigma)) continue;
    const double inv_s = phf_rcp(sigma);
    if (LIK == kHierarchical) {
#pragma unroll
      for (int k = 0; k < kPtBlock; ++k) {
        if (k < b.np) {
          const double li = PHF_LN10 * (6.0 - x[(size_t)(4 + 2 * b.tg[k]) * C]);
          const double pred = phf_pw_pred(2, b.lc[k], x[(size_t)(5 + 2 * b.tg[k]) * C], li, k_exp);
          acc[k] += phf_ppc_pit_hier(pred, b.yv[k], inv_s, k_exp);
        }
      }
    } else {
      const double ln_ic50 = PHF_LN10 * (6.0 - x[0]), hill = LIK == 2 ? x[C] : 1.0;
#pragma unroll
      for (int k = 0; k < kPtBlock; ++k) {
        if (k < b.np) acc[k] += phf_ppc_pit_sl(phf_pw_pred(LIK, b.lc[k], hill, ln_ic50, k_exp), b.yv[k], b.tg[k], inv_s);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kPtBlock; ++k)
    if (k < b.np) st[(size_t)k * C] = acc[k];
}

// out[u] = the sum over chains of workspace field u (u = q * fields + f), chains in a fixed order
__global__ __launch_bounds__(kThreads) void ppc_reduce_kernel(const double* ws, int64_t units, int num_chains, double* out) {
  const int64_t unit = (int64_t)blockIdx.x * kWaves + threadIdx.x / 64;
  if (unit >= units) return;
  const int lane = threadIdx.x & 63;
  const double* st = ws + (size_t)unit * num_chains;
  double s = 0.0;
  for (int c = lane; c < num_chains; c += 64) s += st[c];
  for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);   // a + b == b + a: both partners hold the same sum
  if (lane == 0) out[unit] = s;
}

// batch evaluator: vector i of problem problem_index[i] at theta[.][i] with counter (chain id, problem id, row) = counter[i][0..2]
template <int LIK>
__global__ __launch_bounds__(kThreads) void ppc_replicate_kernel(const phf_pointwise_points pts, int ne, int64_t m,
                                                                 const int32_t* problem_index, const double* theta,
                                                                 const uint32_t* counter, uint32_t k0, uint32_t k1, double* y_rep,
                                                                 double* stats) {
  PHF_MATH_TABLES_TO_LDS();
  if (LIK == kHierarchical) {
    PHF_ERFC_TABLE_TO_LDS();
  } else {
    PHF_LOGPHI_TABLE_TO_LDS();
    PHF_NORMAL_TABLE_TO_LDS();
  }
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  const int q = problem_index[i];
  double* yo = y_rep + (size_t)i * pts.stride;
  double* so = stats + (size_t)i * 2 * kStats;
  const int n = (q < 0 || q >= pts.num_problems) ? 0 : clamp_count(pts.count[q], pts.stride);
  const double* x = theta + i;
  if (n == 0 || !valid_sigma(sigma_of<LIK>(x, (size_t)m, ne))) {
    for (int p = 0; p < pts.stride; ++p) yo[p] = PHF_NAN;
    for (int s = 0; s < 2 * kStats; ++s) so[s] = PHF_NAN;
    return;
  }
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  const size_t row = (size_t)q * pts.stride;
  const ObsConst oc = obs_const(pts.response + row, n);
  ppc_draw<LIK, true>(pts.ln_conc + row, pts.response + row, pts.tag + row, n, x, (size_t)m, ne, counter[3 * i], counter[3 * i + 1],
                      counter[3 * i + 2], k0, k1, oc, k_exp, k_log, yo, so, so + kStats);
  for (int p = n; p < pts.stride; ++p) yo[p] = PHF_NAN;
}

int check_shape(const char* who, int num_problems, int stride, int num_chains, int64_t total_rows) {
  const int rc = phf_check_positive(who, "num_problems, stride and num_chains", {num_problems, stride, num_chains});
  if (rc != PHF_OK) return rc;
  if (stride > kMaxStride) return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: at most %d points per problem (stride %d)", who, kMaxStride, stride);
  if (total_rows < 1) return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: total_rows must be positive (got %lld)", who, (long long)total_rows);
  const double units = (double)num_problems * ((num_chains + 63) / 64) * ((stride + kPtBlock - 1) / kPtBlock);
  return phf_check_grid(who, {units, (double)num_problems * (kHead + stride)});
}

size_t workspace_bytes_of(int num_problems, int stride, int num_chains) {
  return (size_t)num_problems * (kHead + (size_t)stride) * (size_t)num_chains * sizeof(double);
}

}  // namespace

extern "C" size_t phf_ppc_workspace_bytes(int num_problems, int stride, int num_chains, int64_t total_rows) {
  if (check_shape("phf_ppc_workspace_bytes", num_problems, stride, num_chains, total_rows) != PHF_OK) return 0;
  return workspace_bytes_of(num_problems, stride, num_chains);
}

extern "C" int phf_ppc_init(int num_problems, int stride, int num_chains, int64_t total_rows, double* workspace, size_t workspace_bytes,
                            void* stream) {
  static const char* who = "phf_ppc_init";
  const int rc = check_shape(who, num_problems, stride, num_chains, total_rows);
  if (rc != PHF_OK) return rc;
  const size_t need = workspace_bytes_of(num_problems, stride, num_chains);
  return phf_init_workspace(who, "ppc", workspace, workspace_bytes, need, need, stream);
}

extern "C" int phf_ppc_accumulate(const phf_pointwise_points* pts, int likelihood, int num_expts, const double* rows, int64_t num_rows,
                                  int num_problems, int row_stride_cols, int num_chains, int64_t first_row, int64_t total_rows,
                                  const uint32_t* problem_id, uint32_t chain_id_base, uint64_t seed, double* workspace,
                                  size_t workspace_bytes, void* stream) {
  static const char* who = "phf_ppc_accumulate";
  int rc = phf_check_points(who, pts, num_problems, kMaxStride);
  if (rc != PHF_OK) return rc;
  if ((rc = check_shape(who, num_problems, pts->stride, num_chains, total_rows)) != PHF_OK) return rc;
  if ((rc = phf_check_likelihood(who, likelihood, num_expts)) != PHF_OK) return rc;
  const int cols = likelihood == kHierarchical ? 5 + 2 * num_expts : likelihood + 1;
  if ((rc = phf_check_row_stride(who, row_stride_cols, cols, "is smaller than the columns the likelihood reads")) != PHF_OK) return rc;
  if ((rc = phf_check_row_window(who, num_rows, first_row, total_rows)) != PHF_OK) return rc;
  if (total_rows > 4294967296LL)
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_ppc_accumulate: total_rows must fit the 32-bit row word of the random stream");
  if (!rows || !workspace || !problem_id) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_ppc_accumulate: null pointer");
  if ((rc = phf_check_workspace(who, "ppc", workspace, workspace_bytes, workspace_bytes_of(num_problems, pts->stride, num_chains))) != PHF_OK)
    return rc;
  if (num_rows == 0) return PHF_OK;
  PpcArgs a = {};
  a.pts = *pts; a.rows = rows; a.nr = num_rows; a.first_row = first_row; a.total_rows = total_rows;
  a.Q = num_problems; a.stride_cols = row_stride_cols; a.C = num_chains; a.ne = num_expts; a.ws = workspace;
  a.problem_id = problem_id; a.chain_id_base = chain_id_base; a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
  a.ncg = (num_chains + 63) / 64; a.npb = (pts->stride + kPtBlock - 1) / kPtBlock;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // statistics: one wavefront per (problem, 64 chains)
  a.units = num_problems * a.ncg;
  const dim3 sgrid(blocks_for(a.units, kWaves)), block(kThreads);
  const size_t lds = kWaves * slice_doubles(pts->stride) * sizeof(double);
  if (likelihood == 1) hipLaunchKernelGGL(ppc_stats_kernel<1>, sgrid, block, lds, s, a);
  else if (likelihood == 2) hipLaunchKernelGGL(ppc_stats_kernel<2>, sgrid, block, lds, s, a);
  else hipLaunchKernelGGL(ppc_stats_kernel<kHierarchical>, sgrid, block, lds, s, a);
  if ((rc = phf_check_launch("ppc_stats_kernel")) != PHF_OK) return rc;
  // PIT: one wavefront per (problem, 64 chains, 4 points)
  a.units = num_problems * a.ncg * a.npb;
  const dim3 pgrid(blocks_for(a.units, kWaves));
  if (likelihood == 1) hipLaunchKernelGGL(ppc_pit_kernel<1>, pgrid, block, 0, s, a);
  else if (likelihood == 2) hipLaunchKernelGGL(ppc_pit_kernel<2>, pgrid, block, 0, s, a);
  else hipLaunchKernelGGL(ppc_pit_kernel<kHierarchical>, pgrid, block, 0, s, a);
  return phf_check_launch("ppc_pit_kernel");
}

extern "C" int phf_ppc_reduce(int num_problems, int stride, int num_chains, int64_t total_rows, const double* workspace,
                              size_t workspace_bytes, double* out, void* stream) {
  static const char* who = "phf_ppc_reduce";
  int rc = check_shape(who, num_problems, stride, num_chains, total_rows);
  if (rc != PHF_OK) return rc;
  if (!workspace || !out) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_ppc_reduce: null pointer");
  if ((rc = phf_check_workspace(who, "ppc", workspace, workspace_bytes, workspace_bytes_of(num_problems, stride, num_chains))) != PHF_OK) return rc;
  const int64_t units = (int64_t)num_problems * (kHead + stride);
  hipLaunchKernelGGL(ppc_reduce_kernel, dim3(blocks_for(units, kWaves)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), workspace,
                     units, num_chains, out);
  return phf_check_launch("ppc_reduce_kernel");
}

extern "C" int phf_ppc_replicate(const phf_pointwise_points* pts, int likelihood, int num_expts, int64_t m, const int32_t* problem_index,
                                 const double* theta, const uint32_t* counter, uint64_t seed, double* y_rep, double* stats,
                                 void* stream) {
  static const char* who = "phf_ppc_replicate";
  int rc = phf_check_points(who, pts, 0, kMaxStride);
  if (rc != PHF_OK) return rc;
  if ((rc = phf_check_likelihood(who, likelihood, num_expts)) != PHF_OK) return rc;
  if (m < 0 || (m > 0 && (!problem_index || !theta || !counter || !y_rep || !stats)))
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_ppc_replicate: m must be >= 0 and the arrays non-null");
  if (m == 0) return PHF_OK;
  const dim3 grid(blocks_for(m, kThreads)), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  if (likelihood == 1)
    hipLaunchKernelGGL(ppc_replicate_kernel<1>, grid, block, 0, s, *pts, num_expts, m, problem_index, theta, counter, k0, k1, y_rep, stats);
  else if (likelihood == 2)
    hipLaunchKernelGGL(ppc_replicate_kernel<2>, grid, block, 0, s, *pts, num_expts, m, problem_index, theta, counter, k0, k1, y_rep, stats);
  else
    hipLaunchKernelGGL(ppc_replicate_kernel<kHierarchical>, grid, block, 0, s, *pts, num_expts, m, problem_index, theta, counter, k0, k1,
                       y_rep, stats);
  return phf_check_launch(who);
}

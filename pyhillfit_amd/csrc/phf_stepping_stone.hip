// phf_stepping_stone.hip — stepping-stone evidence of the tempered ladder, streamed over the sampler's rows (include/pyhillfit_amd.h).
//
// Stepping stone (Xie, Lewis, Fan, Kuo & Chen 2011): rung k's draws theta ~ p_t_k estimate the ratio
//     r_k = Z(t_k+1) / Z(t_k) = E_t_k[ L(theta)^Delta_k ],     Delta_k = t_k+1 - t_k,
// per chain c over its n rows:  log r_kc = LSE_j(Delta_k l_kcj) - ln n,  l = log L(theta; t = 1) (phf_sl_log_target's ll1, pi_bit
// included: the sampler's own untempered log-likelihood).
// Per (problem, chain) the workspace holds, in one lane's registers while a segment's rows stream past:
//   m            running max of x = Delta l
//   s1, s2       sum exp(x - m), sum exp(2 (x - m)): the chain's weight sums (online, rescaled when m grows)
//   sl, n        sum of l, rows seen
// x = -inf (l = -inf, Delta > 0) adds nothing; Delta = 0 gives x = 0 for every draw (L^0 = 1, as the sampler's t = 0 ignores l)
// unless l is NaN; a NaN l makes s1, s2 and sl NaN for good.
// Mapping: one lane = one chain (the rows are [rows][Q][stride][C], chain fastest: a wavefront reads 512 contiguous bytes of one
// (problem, column)); one wavefront = 64 chains of one problem, so the problem's entries are wave-uniform.  Reduce: one wavefront
// per problem merges the chains in a fixed order (lane l takes chains l, l+64, ...; then a fixed butterfly).
//
// Deterministic: no atomics, every accumulator is produced by one lane in row order and round-trips through HBM exactly, so the
// result is bit-identical however the rows are cut into calls and whatever the launch shape.
#include <hip/hip_runtime.h>

#include "../../include/pyhillfit_amd.h"
#include "phf_host_checks.h"
#include "phf_device_util.h"
#include "phf_model.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kFields = 5;              // m, s1, s2, sl, n
constexpr int kOut = 7;                 // log r, se, log r of chain 0, ESS, n, mean l, chains with a NaN log r

struct SsArgs {
  phf_points pts;
  int32_t model;
  const int32_t* pair_index;      // [Q]
  const double* delta;            // [Q]
  const double* rows;             // [nr][Q][stride_cols][C]
  int64_t nr, first_row, total_rows;
  int32_t Q, stride_cols, C, ncg;
  int32_t units;
  double* ws;                     // [Q][kFields][C]
  double* out;                    // reduce: [Q][kOut]
};

template <int MODEL>
__global__ __launch_bounds__(kThreads) void ss_accumulate_kernel(const SsArgs a) {
  PHF_MATH_TABLES_TO_LDS();
  PHF_LOGPHI_TABLE_TO_LDS();
  constexpr int D = MODEL + 1;
  const int unit = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves + threadIdx.x / 64));   // wave-uniform
  if (unit >= a.units) return;
  const int q = unit / a.ncg, cg = unit % a.ncg;
  const int c = cg * 64 + (threadIdx.x & 63);
  if (c >= a.C) return;
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  const size_t C = (size_t)a.C;
  double* st = a.ws + (size_t)q * kFields * C + c;
  double m = st[0], s1 = st[C], s2 = st[2 * C], sl = st[3 * C], n = st[4 * C];
  if (a.first_row == 0) { m = -PHF_INF; s1 = 0.0; s2 = 0.0; sl = 0.0; n = 0.0; }
  const int pair = __builtin_amdgcn_readfirstlane(a.pair_index[q]);
  const double delta = a.delta[q];
  if (pair < 0 || pair >= a.pts.num_pairs) {                       // no access out of bounds: the problem's results are NaN
    st[C] = PHF_NAN; st[2 * C] = PHF_NAN; st[3 * C] = PHF_NAN; st[4 * C] = n + (double)a.nr;
    return;
  }
  const int32_t* cnt = a.pts.counts + 4 * pair;
  const int n_other = cnt[0], n_cens = cnt[1] + cnt[2];
  const size_t at = (size_t)pair * a.pts.stride;
  const double* lc = a.pts.ln_conc + at;
  const double* yv = a.pts.response + at;
  const double* wv = a.pts.weight + at;
  const double pi_bit = a.pts.pi_bit[pair], n_other_points = a.pts.extra[2 * pair], ss_within = a.pts.extra[2 * pair + 1];
  const size_t rstep = (size_t)a.Q * a.stride_cols * C;
  const double* xr = a.rows + (size_t)q * a.stride_cols * C + c;
  for (int64_t r = 0; r < a.nr; ++r) {
    const double* x = xr + (size_t)r * rstep;
    double th[D];
#pragma unroll
    for (int i = 0; i < D; ++i) th[i] = x[(size_t)i * C];
    double lik, prior, l;
    phf_sl_log_target(MODEL, lc, yv, wv, n_other, n_cens, n_other_points, ss_within, pi_bit, 1.0, th, k_exp, k_log, &lik, &prior, &l);
    sl += l;
    n += 1.0;
    const double v = delta == 0.0 ? (l == l ? 0.0 : l) : delta * l;
    if (v > m) {                                                   // a new max: rescale the sums
      const double e = exp(m - v);                                 // 0 when m = -inf
      s1 = s1 * e + 1.0;
      s2 = s2 * (e * e) + 1.0;
      m = v;
    } else if (v != -PHF_INF) {                                    // -inf: weight 0; NaN: exp(NaN) poisons both sums
      const double e = exp(v - m);
      s1 += e;
      s2 += e * e;
    }
  }
  st[0] = m; st[C] = s1; st[2 * C] = s2; st[3 * C] = sl; st[4 * C] = n;
}

// a log-sum-exp in two parts: max and the sum of exp(. - max)
struct Lse {
  double mx, sx;
};

__device__ inline Lse lse_merge(const Lse& a, const Lse& b) {
  Lse r;
  r.mx = a.mx > b.mx ? a.mx : b.mx;
  if (!(a.mx == a.mx) || !(b.mx == b.mx)) r.mx = PHF_NAN;
  r.sx = r.mx == -PHF_INF ? a.sx + b.sx : a.sx * exp(a.mx - r.mx) + b.sx * exp(b.mx - r.mx);
  return r;
}

__device__ inline Lse lse_shfl(const Lse& a, int o) { return Lse{__shfl_xor(a.mx, o, 64), __shfl_xor(a.sx, o, 64)}; }

// count, mean, sum of squared deviations (Chan, Golub & LeVeque 1979)
struct Part {
  double n, mean, m2;
};

__device__ inline Part part_merge(const Part& a, const Part& b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  Part r;
  r.n = a.n + b.n;
  const double d = b.mean - a.mean;
  r.mean = a.mean + d * (b.n / r.n);
  r.m2 = (a.m2 + b.m2) + d * d * (a.n * b.n / r.n);
  return r;
}

__device__ inline double chain_log_r(double m, double s1, double n) {
  return (m == -PHF_INF && s1 == 0.0) ? -PHF_INF : m + log(s1) - log(n);   // all weights 0: -inf, not -inf + log 0 = NaN
}

// out[q] = (pooled log r, se, chain-0 log r, ESS, n, mean l, chains with a NaN log r); one wavefront per problem
__global__ __launch_bounds__(kThreads) void ss_reduce_kernel(const SsArgs a) {
  const int q = (int)(blockIdx.x * kWaves + threadIdx.x / 64);
  if (q >= a.Q) return;
  const int lane = threadIdx.x & 63;
  const size_t C = (size_t)a.C;
  const double* st = a.ws + (size_t)q * kFields * C;
  // pass 1: pooled LSE of the chains' log r; LSE of the weights and of their squares over all draws; sum of l; NaN chains
  Lse lr = {-PHF_INF, 0.0}, w1 = {-PHF_INF, 0.0}, w2 = {-PHF_INF, 0.0};
  double sl = 0.0, nan_chains = 0.0;
  for (int c = lane; c < a.C; c += 64) {
    const double m = st[c], s1 = st[C + c], s2 = st[2 * C + c], n = st[4 * C + c];
    const double v = chain_log_r(m, s1, n);
    if (!(v == v)) nan_chains += 1.0;
    lr = lse_merge(lr, Lse{v, 1.0});
    w1 = lse_merge(w1, Lse{m, s1});
    w2 = lse_merge(w2, Lse{2.0 * m, s2});
    sl += st[3 * C + c];
  }
  for (int o = 32; o > 0; o >>= 1) {
    const Lse olr = lse_shfl(lr, o), ow1 = lse_shfl(w1, o), ow2 = lse_shfl(w2, o);
    const double osl = __shfl_xor(sl, o, 64), onan = __shfl_xor(nan_chains, o, 64);
    const bool hi = (lane & o) != 0;                                // the lower lane's part first: the same order on both partners
    lr = hi ? lse_merge(olr, lr) : lse_merge(lr, olr);
    w1 = hi ? lse_merge(ow1, w1) : lse_merge(w1, ow1);
    w2 = hi ? lse_merge(ow2, w2) : lse_merge(w2, ow2);
    sl = hi ? osl + sl : sl + osl;
    nan_chains = hi ? onan + nan_chains : nan_chains + onan;
  }
  const double log_c = log((double)a.C);
  const double pooled = lr.mx == -PHF_INF ? -PHF_INF : lr.mx + log(lr.sx) - log_c;
  // pass 2: the spread of the chains' ratios r_c / r around the pooled r (divisor C - 1)
  Part p = {0.0, 0.0, 0.0};
  for (int c = lane; c < a.C; c += 64) {
    const double v = exp(chain_log_r(st[c], st[C + c], st[4 * C + c]) - pooled);
    p = part_merge(p, Part{1.0, v, 0.0});
  }
  for (int o = 32; o > 0; o >>= 1) {
    const Part op = {__shfl_xor(p.n, o, 64), __shfl_xor(p.mean, o, 64), __shfl_xor(p.m2, o, 64)};
    p = (lane & o) ? part_merge(op, p) : part_merge(p, op);
  }
  if (lane == 0) {
    const double n0 = st[4 * C];
    double* o = a.out + (size_t)q * kOut;
    o[0] = pooled;
    o[1] = a.C > 1 ? sqrt(p.m2 / (p.n - 1.0)) / sqrt((double)a.C) : PHF_NAN;
    o[2] = chain_log_r(st[0], st[C], n0);
    o[3] = w1.mx == -PHF_INF ? 0.0 : (w1.sx * w1.sx) / w2.sx;     // (sum w)^2 / sum w^2, w = exp(x - max): both sums share the max
    o[4] = n0;
    o[5] = sl / ((double)a.C * n0);
    o[6] = nan_chains;
  }
}

// out[p] = sd_c(v_c) / sqrt(C), v_c = sum_k<R-1 r_kc / r_k over pair p's rungs (replica sets); one wavefront per pair
__global__ __launch_bounds__(kThreads) void ss_reduce_joint_kernel(const SsArgs a, int num_pairs, int rungs, const double* reduced) {
  const int p = (int)(blockIdx.x * kWaves + threadIdx.x / 64);
  if (p >= num_pairs) return;
  const int lane = threadIdx.x & 63;
  const size_t C = (size_t)a.C;
  Part part = {0.0, 0.0, 0.0};
  for (int c = lane; c < a.C; c += 64) {
    double v = 0.0;
    for (int k = 0; k < rungs - 1; ++k) {
      const int q = p * rungs + k;
      const double* st = a.ws + (size_t)q * kFields * C;
      v += exp(chain_log_r(st[c], st[C + c], st[4 * C + c]) - reduced[(size_t)q * kOut]);
    }
    part = part_merge(part, Part{1.0, v, 0.0});
  }
  for (int o = 32; o > 0; o >>= 1) {
    const Part op = {__shfl_xor(part.n, o, 64), __shfl_xor(part.mean, o, 64), __shfl_xor(part.m2, o, 64)};
    part = (lane & o) ? part_merge(op, part) : part_merge(part, op);
  }
  if (lane == 0) a.out[p] = a.C > 1 ? sqrt(part.m2 / (part.n - 1.0)) / sqrt((double)a.C) : PHF_NAN;
}

int check_shape(const char* who, int num_problems, int num_chains, int64_t total_rows) {
  const int rc = phf_check_positive(who, "num_problems and num_chains", {num_problems, num_chains});
  if (rc != PHF_OK) return rc;
  if (total_rows < 1) return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: total_rows must be positive (got %lld)", who, (long long)total_rows);
  return phf_check_grid(who, {(double)num_problems * ((num_chains + 63) / 64)});
}

size_t workspace_bytes_of(int num_problems, int num_chains) {
  return (size_t)num_problems * kFields * (size_t)num_chains * sizeof(double);
}

}  // namespace

extern "C" size_t phf_stepping_stone_workspace_bytes(int num_problems, int num_chains, int64_t total_rows) {
  if (check_shape("phf_stepping_stone_workspace_bytes", num_problems, num_chains, total_rows) != PHF_OK) return 0;
  return workspace_bytes_of(num_problems, num_chains);
}

extern "C" int phf_stepping_stone_init(int num_problems, int num_chains, int64_t total_rows, double* workspace, size_t workspace_bytes,
                                       void* stream) {
  static const char* who = "phf_stepping_stone_init";
  const int rc = check_shape(who, num_problems, num_chains, total_rows);
  if (rc != PHF_OK) return rc;
  const size_t need = workspace_bytes_of(num_problems, num_chains);
  return phf_init_workspace(who, "stepping_stone", workspace, workspace_bytes, need, need, stream);
}

extern "C" int phf_stepping_stone_accumulate(const phf_points* pts, int model, const int32_t* pair_index, const double* delta,
                                             const double* rows, int64_t num_rows, int num_problems, int row_stride_cols, int num_chains,
                                             int64_t first_row, int64_t total_rows, double* workspace, size_t workspace_bytes, void* stream) {
  static const char* who = "phf_stepping_stone_accumulate";
  int rc = check_shape(who, num_problems, num_chains, total_rows);
  if (rc != PHF_OK) return rc;
  if (!pts || pts->num_pairs < 1 || pts->stride < 1 || !pts->ln_conc || !pts->response || !pts->weight || !pts->counts || !pts->pi_bit ||
      !pts->extra)
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_stepping_stone_accumulate: null or empty points");
  if (model != 1 && model != 2) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_stepping_stone_accumulate: model must be 1 or 2");
  if ((rc = phf_check_row_stride(who, row_stride_cols, model + 1, "is smaller than the model's parameters")) != PHF_OK) return rc;
  if ((rc = phf_check_row_window(who, num_rows, first_row, total_rows)) != PHF_OK) return rc;
  if (!pair_index || !delta || !rows || !workspace) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_stepping_stone_accumulate: null pointer");
  if ((rc = phf_check_workspace(who, "stepping_stone", workspace, workspace_bytes, workspace_bytes_of(num_problems, num_chains))) != PHF_OK) return rc;
  if (num_rows == 0) return PHF_OK;
  SsArgs a = {};
  a.pts = *pts; a.model = model; a.pair_index = pair_index; a.delta = delta; a.rows = rows; a.nr = num_rows; a.first_row = first_row;
  a.total_rows = total_rows; a.Q = num_problems; a.stride_cols = row_stride_cols; a.C = num_chains; a.ws = workspace;
  a.ncg = (num_chains + 63) / 64;
  a.units = num_problems * a.ncg;
  const dim3 grid(blocks_for(a.units, kWaves)), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (model == 1) hipLaunchKernelGGL(ss_accumulate_kernel<1>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(ss_accumulate_kernel<2>, grid, block, 0, s, a);
  return phf_check_launch("ss_accumulate_kernel");
}

extern "C" int phf_stepping_stone_reduce(int num_problems, int num_chains, int64_t total_rows, const double* workspace,
                                         size_t workspace_bytes, double* out, void* stream) {
  static const char* who = "phf_stepping_stone_reduce";
  int rc = check_shape(who, num_problems, num_chains, total_rows);
  if (rc != PHF_OK) return rc;
  if (!workspace || !out) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_stepping_stone_reduce: null pointer");
  if ((rc = phf_check_workspace(who, "stepping_stone", workspace, workspace_bytes, workspace_bytes_of(num_problems, num_chains))) != PHF_OK) return rc;
  SsArgs a = {};
  a.Q = num_problems; a.C = num_chains; a.total_rows = total_rows; a.ws = const_cast<double*>(workspace); a.out = out;
  hipLaunchKernelGGL(ss_reduce_kernel, dim3(blocks_for(num_problems, kWaves)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  return phf_check_launch("ss_reduce_kernel");
}

extern "C" int phf_stepping_stone_reduce_joint(int num_pairs, int rungs_per_pair, int num_chains, int64_t total_rows, const double* workspace,
                                               size_t workspace_bytes, const double* reduced, double* out, void* stream) {
  if (num_pairs < 1 || rungs_per_pair < 1 || (double)num_pairs * rungs_per_pair > 2147483647.0)
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_stepping_stone_reduce_joint: num_pairs and rungs_per_pair must be positive");
  const int Q = num_pairs * rungs_per_pair;
  static const char* who = "phf_stepping_stone_reduce_joint";
  int rc = check_shape(who, Q, num_chains, total_rows);
  if (rc != PHF_OK) return rc;
  if (!workspace || !reduced || !out) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_stepping_stone_reduce_joint: null pointer");
  if ((rc = phf_check_workspace(who, "stepping_stone", workspace, workspace_bytes, workspace_bytes_of(Q, num_chains))) != PHF_OK) return rc;
  SsArgs a = {};
  a.Q = Q; a.C = num_chains; a.total_rows = total_rows; a.ws = const_cast<double*>(workspace); a.out = out;
  hipLaunchKernelGGL(ss_reduce_joint_kernel, dim3(blocks_for(num_pairs, kWaves)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a,
                     num_pairs, rungs_per_pair, reduced);
  return phf_check_launch("ss_reduce_joint_kernel");
}

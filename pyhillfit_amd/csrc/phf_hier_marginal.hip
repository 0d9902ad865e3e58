// phf_hier_marginal.hip — marginal log-likelihood of whole experiments of the hierarchical model (phf_hier_marginal.h; DESIGN.md §3,
// "Integrated leave-one-experiment-out"): the Q x Q tensor rule over the population distribution of one draw.
//
// Mapping: one wavefront per (draw, experiment).  The draw's (alpha, beta, mu, s, sigma) and the experiment's points are
// wave-uniform: the wavefront compacts the points of its experiment (tag == e, in point order) into its own slice of LDS once and
// every lane then reads them at the same address (a broadcast); the node table [3][Q] sits in LDS once per block.  Lane t owns the
// Hill nodes t mod min(Q, 64) + 64 i and loops over its pIC50 nodes (phf_mg_lane: the host twin runs the very same function for
// t = 0..63); each lane keeps two online log-sum-exps (all nodes, even-even nodes); a butterfly of __shfl_xor, the lower lane's part
// first, merges the lanes — lane 0 ends with the tree of phf_mg_tree.  No atomics; exp2, log and erfc tables in LDS.
//
// The streaming entry reads the samplers' row buffer [rows][Q][stride][C] and uses exactly the global rows r with r mod every == 0,
// however the calls cut the rows; the per-chain running maximum of the gap is folded by a second kernel, one thread per
// (problem, experiment, chain) over the call's used rows in row order (a maximum: no rounding, any order gives the same bits).
#include <hip/hip_runtime.h>

#include "../../include/pyhillfit_amd.h"
#include "phf_common.h"
#include "phf_hier_marginal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxStride = 512;         // points per problem row the per-wave LDS slices are sized for (4 x 2 x 512 doubles = 32 KiB)
constexpr int kMaxExpts = 64;

struct MgArgs {
  phf_pointwise_points pts;
  const double* nodes;            // [3][nq]
  int32_t nq, ne;
  int64_t units;
  // batch: theta [5 + 2 ne][m], problem_index [m]
  int64_t m;
  const int32_t* problem_index;
  const double* theta;
  // rows: [nr][Q][stride_cols][C]; the first used row of the call is local row r0, then every `every`-th
  const double* rows;
  int64_t r0;
  int32_t every, Q, stride_cols, C;
  double* out_m;                  // [units]
  double* out_g;                  // [units]
};

extern __shared__ __attribute__((aligned(16))) double mg_smem[];

template <bool ROWS>
__global__ __launch_bounds__(kThreads) void marginal_kernel(const MgArgs a) {
  PHF_MATH_TABLES_TO_LDS();
  PHF_ERFC_TABLE_TO_LDS();
  double* nodes = mg_smem;                                               // [3][nq]
  for (int i = threadIdx.x; i < 3 * a.nq; i += kThreads) nodes[i] = a.nodes[i];
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
  const int64_t unit = (int64_t)blockIdx.x * kWaves + wave;              // wave-uniform
  if (unit >= a.units) return;
  const int lane = threadIdx.x & 63;
  const int ps = a.pts.stride;
  double* lc = mg_smem + 3 * a.nq + (size_t)wave * 2 * ps;               // this wavefront's points: ln_conc [ps], then y [ps]
  double* yv = lc + ps;
  int q, e;
  double alpha, beta, mu, s, sigma;
  if (ROWS) {
    const int c = (int)(unit % a.C);
    int64_t u = unit / a.C;
    e = (int)(u % a.ne); u /= a.ne;
    q = (int)(u % a.Q); u /= a.Q;
    const size_t C = (size_t)a.C;
    const double* x = a.rows + (((size_t)(a.r0 + u * a.every) * a.Q + q) * a.stride_cols) * C + c;
    alpha = x[0]; beta = x[C]; mu = x[2 * C]; s = x[3 * C]; sigma = x[(size_t)(4 + 2 * a.ne) * C];
  } else {
    const int64_t i = unit / a.ne;
    e = (int)(unit % a.ne);
    q = a.problem_index[i];
    const size_t m = (size_t)a.m;
    alpha = a.theta[i]; beta = a.theta[m + i]; mu = a.theta[2 * m + i]; s = a.theta[3 * m + i];
    sigma = a.theta[(size_t)(4 + 2 * a.ne) * m + i];
  }
  const bool bad_q = q < 0 || q >= a.pts.num_problems;
  if (bad_q || !phf_band_valid(PHF_BAND_FUTURE, alpha, beta, mu, s) || sigma != sigma) {
    if (lane == 0) { a.out_m[unit] = PHF_NAN; a.out_g[unit] = PHF_NAN; }
    return;
  }
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  const phf_pw_sigma sg = phf_pw_sigma_terms(sigma, k_log);
  if (sg.base == -PHF_INF) {
    if (lane == 0) { a.out_m[unit] = -PHF_INF; a.out_g[unit] = 0.0; }
    return;
  }
  // the experiment's points, in point order (every lane stores the same values: the slice belongs to this wavefront alone).  All 64
  // lanes walk the problem's points, at most 512 uniform loads and stores once per wavefront, against Q^2 x n point terms of a few
  // hundred fp64 operations each: a ballot compaction would save under a thousandth of the wavefront's work at Q = 32 and less above
  int np = a.pts.count[q];
  np = np < 0 ? 0 : (np > ps ? ps : np);
  const size_t row = (size_t)q * ps;
  int n = 0;
  for (int p = 0; p < np; ++p) {
    int t = a.pts.tag[row + p];
    t = t < 0 ? 0 : (t > a.ne - 1 ? a.ne - 1 : t);
    if (t == e) {
      lc[n] = a.pts.ln_conc[row + p];
      yv[n] = a.pts.response[row + p];
      ++n;
    }
  }
  phf_mg_lse f, c;
  phf_mg_lane(lane, a.nq, nodes, n, lc, yv, alpha, beta, mu, s, sg, k_exp, k_log, &f, &c);
  for (int o = 32; o > 0; o >>= 1) {
    phf_mg_lse of, oc;
    of.m = __shfl_xor(f.m, o, 64); of.s = __shfl_xor(f.s, o, 64);
    oc.m = __shfl_xor(c.m, o, 64); oc.s = __shfl_xor(c.s, o, 64);
    f = (lane & o) ? phf_mg_merge(of, f, k_exp) : phf_mg_merge(f, of, k_exp);     // the lower lane's part first
    c = (lane & o) ? phf_mg_merge(oc, c, k_exp) : phf_mg_merge(c, oc, k_exp);
  }
  if (lane == 0) {
    const double fine = phf_mg_value(f, k_log), coarse = phf_mg_value(c, k_log);
    a.out_m[unit] = fine;
    a.out_g[unit] = phf_mg_gap(fine, coarse);
  }
}

// gap_max[j] = max(gap_max[j], g[u][j]) over the call's used rows u, j = one (problem, experiment, chain); NaN gaps are passed over
__global__ __launch_bounds__(kThreads) void gap_max_kernel(const double* g, int64_t used, int64_t per_row, double* gap_max) {
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= per_row) return;
  double mx = gap_max[j];
  for (int64_t u = 0; u < used; ++u) {
    const double v = g[u * per_row + j];
    mx = v > mx ? v : mx;
  }
  gap_max[j] = mx;
}

size_t lds_bytes(int nq, int stride) { return ((size_t)3 * nq + (size_t)kWaves * 2 * stride) * sizeof(double); }

int check_common(const char* who, const phf_pointwise_points* pts, int num_expts, const double* nodes, int num_nodes) {
  if (!pts || !pts->ln_conc || !pts->response || !pts->tag || !pts->count)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: null points", who);
  if (pts->stride < 1 || pts->num_problems < 1)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: the points must have stride >= 1 and at least one problem", who);
  if (pts->stride > kMaxStride)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: at most %d points per problem (stride %d)", who, kMaxStride, pts->stride);
  if (num_expts < 1 || num_expts > kMaxExpts)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: num_expts must be in 1..%d (got %d)", who, kMaxExpts, num_expts);
  if (!phf_mg_nodes_ok(num_nodes))
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: num_nodes must be 32, 64, 128 or 256 (got %d)", who, num_nodes);
  if (!nodes)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: null nodes", who);
  return PHF_OK;
}

template <bool ROWS>
int launch(const char* who, const MgArgs& a, hipStream_t stream) {
  const int64_t blocks = (a.units + kWaves - 1) / kWaves;
  if (blocks > 2147483647ll) {
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: launch grid too large (fewer draws per call)", who);
  }
  hipLaunchKernelGGL(marginal_kernel<ROWS>, dim3((unsigned)blocks), dim3(kThreads), lds_bytes(a.nq, a.pts.stride), stream, a);
  return phf_check_launch(who);
}

}  // namespace

extern "C" int phf_hier_marginal_loglik(const phf_pointwise_points* pts, int num_expts, const double* nodes, int num_nodes, int64_t m,
                                        const int32_t* problem_index, const double* theta, double* out, void* stream) {
  static const char* who = "phf_hier_marginal_loglik";
  int rc = check_common(who, pts, num_expts, nodes, num_nodes);
  if (rc != PHF_OK) return rc;
  if (m < 0 || (m > 0 && (!problem_index || !theta || !out)))
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_marginal_loglik: m must be >= 0 and the arrays non-null");
  if (m == 0) return PHF_OK;
  MgArgs a = {};
  a.pts = *pts; a.nodes = nodes; a.nq = num_nodes; a.ne = num_expts; a.m = m; a.problem_index = problem_index; a.theta = theta;
  a.units = m * num_expts;
  a.out_m = out; a.out_g = out + (size_t)m * num_expts;
  return launch<false>(who, a, static_cast<hipStream_t>(stream));
}

extern "C" int64_t phf_hier_marginal_rows_used(int64_t first_row, int64_t num_rows, int every) {
  if (first_row < 0 || num_rows < 0 || every < 1) return -1;
  const int64_t end = first_row + num_rows;
  return (end + every - 1) / every - (first_row + every - 1) / every;      // multiples of `every` in [first_row, end)
}

extern "C" int phf_hier_marginal_rows(const phf_pointwise_points* pts, int num_expts, const double* nodes, int num_nodes, const double* rows,
                                      int64_t num_rows, int num_problems, int row_stride_cols, int num_chains, int64_t first_row, int every,
                                      double* loglik, double* gap, double* gap_max, void* stream) {
  static const char* who = "phf_hier_marginal_rows";
  int rc = check_common(who, pts, num_expts, nodes, num_nodes);
  if (rc != PHF_OK) return rc;
  if (num_problems < 1 || pts->num_problems != num_problems)
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_marginal_rows: the points must have one row per problem");
  if (num_chains < 1) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_marginal_rows: num_chains must be positive");
  if (row_stride_cols < 5 + 2 * num_expts)
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_marginal_rows: row_stride_cols is smaller than the 5 + 2 num_expts columns of a hierarchical row");
  if (every < 1) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_marginal_rows: every must be >= 1");
  if (num_rows < 0 || first_row < 0) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_marginal_rows: num_rows and first_row must be >= 0");
  const int64_t used = phf_hier_marginal_rows_used(first_row, num_rows, every);
  if (used == 0) return PHF_OK;
  if (!rows || !loglik || !gap || !gap_max) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_marginal_rows: null pointer");
  const int64_t per_row = (int64_t)num_problems * num_expts * num_chains;
  MgArgs a = {};
  a.pts = *pts; a.nodes = nodes; a.nq = num_nodes; a.ne = num_expts; a.rows = rows;
  a.r0 = (every - first_row % every) % every; a.every = every; a.Q = num_problems; a.stride_cols = row_stride_cols; a.C = num_chains;
  a.units = used * per_row;
  a.out_m = loglik; a.out_g = gap;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((rc = launch<true>(who, a, s)) != PHF_OK) return rc;
  hipLaunchKernelGGL(gap_max_kernel, dim3((unsigned)((per_row + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, gap, used, per_row, gap_max);
  return phf_check_launch("phf_hier_marginal_rows: gap maximum");
}

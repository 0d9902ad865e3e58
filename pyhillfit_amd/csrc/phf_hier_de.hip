// phf_hier_de.hip — differential-evolution moves between the chains of one pair of the hierarchical sampler (phf_hier_de.h;
// include/pyhillfit_amd.h; DESIGN.md §3, "Differential-evolution moves").
//
// Layout: the hierarchical sampler's state [S][Q*C].  A round is two launches in stream order, sub-round h = 0 then 1: the chains whose
// index within their population of G consecutive chains has parity h move (phf_de_move), the other parity's chains are donors and are
// only read — within a launch no location is written by one lane and read by another.  No grid-wide synchronisation, no waiting on
// other workgroups, no atomics.
//
// Mapping: one lane per chain; a wavefront = 64 consecutive chains of one problem = 64 / G populations; problem, pair and points are
// wave-uniform.  The proposal goes to the caller's workspace [dim][Q*C] and the target reads it from there with the chain stride
// (coalesced across the wavefront), so no per-lane array of up to 133 doubles exists; for n_expts <= 8 the kernel is compiled per n_expts
// (the batched target unrolls: registers only), above that one kernel runs the per-experiment target.
//
// Statistics (int64, no atomics): attempts and accepts per (kind of round, problem, 64-chain block), kind 0 = ordinary, 1 = gamma == 1;
// each counter is written by lane 0 of the one wavefront that owns it, in both sub-rounds (stream order).  The readback sums the
// chain blocks in a fixed order.
#include <hip/hip_runtime.h>

#include "../../include/pyhillfit_amd.h"
#include "phf_common.h"
#include "phf_hier_de.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct DeArgs {
  phf_hier_points pts;
  phf_hier_prior prior;
  const int32_t* pair_index;      // [Q]
  const uint32_t* problem_id;     // [Q]
  const uint32_t* chain_offset;   // [Q] or NULL
  uint32_t chain_id_base;
  int32_t Q, C, ncg, G, h, kind;
  uint32_t round;
  uint32_t seed_lo, seed_hi;
  double gamma;
  double* state;                  // [S][Q*C]
  double* work;                   // [dim][Q*C]
  long long* stats;               // [2 kinds][attempts, accepts][Q][ncg]
  double* trace;                  // [Q][C][6] or NULL
};

// NE > 0: n_expts, a literal (1..8); NE == 0: pts.n_expts > 8, read at run time
template <int NE>
__global__ __launch_bounds__(kThreads) void de_round_kernel(const DeArgs a) {
  PHF_MATH_TABLES_TO_LDS();
  PHF_ERFC_TABLE_TO_LDS();
  const int unit = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves + threadIdx.x / 64));   // wave-uniform
  if (unit >= a.Q * a.ncg) return;
  // the run-time count never selects the batched target: its work arrays would be indexed at run time (scratch memory)
  const int ne = NE > 0 ? NE : (a.pts.n_expts > PHF_HIER_BATCHED_MAX_EXPTS ? a.pts.n_expts : PHF_HIER_BATCHED_MAX_EXPTS + 1);
  const int dim = 5 + 2 * ne;
  const int q = unit / a.ncg, cg = unit - q * a.ncg;
  const int lane = threadIdx.x & 63;
  const int c = cg * 64 + lane;
  const bool active = c < a.C && (c & 1) == a.h;                   // G is even and divides the first chain's global number
  bool acc = false;
  if (active) {
    PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
    PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
    const int pair = a.pair_index[q];
    const size_t nch = (size_t)a.Q * a.C;
    const size_t g = (size_t)q * a.C + c;
    const size_t g_pop = g - (size_t)(c % a.G);                    // the population's first chain
    const uint32_t cid = a.chain_id_base + (a.chain_offset ? a.chain_offset[q] : 0u) + (uint32_t)c;
    const phf_de_outcome o = phf_de_move(ne, a.pts.expt_start + (size_t)pair * (ne + 1), a.pts.ln_conc + (size_t)pair * a.pts.stride,
                                         a.pts.response + (size_t)pair * a.pts.stride, &a.prior, a.G, a.h, cid, a.problem_id[q], a.round,
                                         a.seed_lo, a.seed_hi, a.gamma, a.state + g, a.state + g_pop, a.state + (size_t)dim * nch + g,
                                         a.work + g, (int)nch, k_exp, k_log);
    acc = o.accepted != 0;
    if (a.trace) {
      double* tr = a.trace + g * 6;
      const int c_pop = c - c % a.G;
      tr[0] = (double)(c_pop + phf_de_donor_slot(o.a, a.h)); tr[1] = (double)(c_pop + phf_de_donor_slot(o.b, a.h));
      tr[2] = o.sg; tr[3] = o.log_u; tr[4] = o.lt_star; tr[5] = acc ? 1.0 : 0.0;
    }
  }
  const unsigned long long tried = __ballot(active), taken = __ballot(acc);
  if (lane == 0) {
    const size_t per = (size_t)a.Q * a.ncg;
    const size_t at = (size_t)a.kind * 2 * per + (size_t)q * a.ncg + cg;
    a.stats[at] = a.stats[at] + __popcll(tried);
    a.stats[at + per] = a.stats[at + per] + __popcll(taken);
  }
}

// out [2 kinds][attempts, accepts][Q]: one thread per entry, chain blocks summed in order
__global__ __launch_bounds__(kThreads) void de_stats_kernel(int Q, int ncg, const long long* stats, long long* out) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= 4LL * Q) return;
  const long long* s = stats + i * ncg;
  long long v = 0;
  for (int g = 0; g < ncg; ++g) v += s[g];
  out[i] = v;
}

int check_shape(const char* who, int num_problems, int num_chains) {
  if (num_problems < 1 || num_chains < 1)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: num_problems and num_chains must be positive", who);
  if ((double)num_problems * num_chains > 2147483647.0)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: num_problems * num_chains must fit in an int32", who);
  return PHF_OK;
}

size_t stats_bytes_of(int Q, int C) { return 4 * (size_t)Q * ((size_t)(C + 63) / 64) * sizeof(long long); }

template <int NE>
int launch_round(const DeArgs& a, hipStream_t s) {
  const int units = a.Q * a.ncg;
  hipLaunchKernelGGL(de_round_kernel<NE>, dim3((unsigned)((units + kWaves - 1) / kWaves)), dim3(kThreads), 0, s, a);
  return phf_check_launch("de_round_kernel");
}

int dispatch_round(const DeArgs& a, hipStream_t s) {
  switch (a.pts.n_expts) {
    case 1: return launch_round<1>(a, s);
    case 2: return launch_round<2>(a, s);
    case 3: return launch_round<3>(a, s);
    case 4: return launch_round<4>(a, s);
    case 5: return launch_round<5>(a, s);
    case 6: return launch_round<6>(a, s);
    case 7: return launch_round<7>(a, s);
    case 8: return launch_round<8>(a, s);
    default: return launch_round<0>(a, s);
  }
}

}  // namespace

extern "C" size_t phf_hier_de_workspace_bytes(int n_expts, int num_problems, int num_chains) {
  if (n_expts < 1 || n_expts > PHF_HIER_MAX_EXPTS) {
    phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_de_workspace_bytes: n_expts must be in 1..64");
    return 0;
  }
  if (check_shape("phf_hier_de_workspace_bytes", num_problems, num_chains) != PHF_OK) return 0;
  return (size_t)(5 + 2 * n_expts) * num_problems * num_chains * sizeof(double);
}

extern "C" size_t phf_hier_de_stats_bytes(int num_problems, int num_chains) {
  if (check_shape("phf_hier_de_stats_bytes", num_problems, num_chains) != PHF_OK) return 0;
  return stats_bytes_of(num_problems, num_chains);
}

extern "C" int phf_hier_de_stats_init(int num_problems, int num_chains, int64_t* stats, size_t stats_bytes, void* stream) {
  int rc = check_shape("phf_hier_de_stats_init", num_problems, num_chains);
  if (rc != PHF_OK) return rc;
  if (!stats) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_de_stats_init: null stats");
  const size_t need = stats_bytes_of(num_problems, num_chains);
  if (stats_bytes < need) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_de_stats_init: stats smaller than phf_hier_de_stats_bytes()");
  if ((rc = phf_require_device_memory(stats, "phf_hier_de_stats_init: stats")) != PHF_OK) return rc;
  if (hipMemsetAsync(stats, 0, need, static_cast<hipStream_t>(stream)) != hipSuccess) return phf_check_launch("phf_hier_de_stats_init");
  return PHF_OK;
}

extern "C" int phf_hier_de_stats_read(int num_problems, int num_chains, const int64_t* stats, size_t stats_bytes, int64_t* out, void* stream) {
  int rc = check_shape("phf_hier_de_stats_read", num_problems, num_chains);
  if (rc != PHF_OK) return rc;
  if (!stats || !out) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_de_stats_read: null pointer");
  if (stats_bytes < stats_bytes_of(num_problems, num_chains))
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_de_stats_read: stats smaller than phf_hier_de_stats_bytes()");
  hipLaunchKernelGGL(de_stats_kernel, dim3((unsigned)((4LL * num_problems + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), num_problems, (num_chains + 63) / 64, reinterpret_cast<const long long*>(stats),
                     reinterpret_cast<long long*>(out));
  return phf_check_launch("de_stats_kernel");
}

extern "C" int phf_hier_de_round(const phf_hier_points* pts, const phf_problems* prob, const phf_hier_prior* prior, int64_t round, uint64_t seed,
                                 int population, double gamma, double* state, double* workspace, size_t workspace_bytes, int64_t* stats,
                                 size_t stats_bytes, double* trace, void* stream) {
  static const char* who = "phf_hier_de_round";
  if (!pts || !prob || !prior) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_de_round: null points, problems or prior");
  if (pts->n_expts < 1 || pts->n_expts > PHF_HIER_MAX_EXPTS)
    return phf_fail(PHF_ERR_UNSUPPORTED, "phf_hier_de_round: n_expts must be in 1..64");
  if (pts->num_pairs <= 0 || pts->stride <= 0 || !pts->ln_conc || !pts->response || !pts->expt_start)
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_de_round: incomplete phf_hier_points");
  if (!prob->pair_index || !prob->problem_id) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_de_round: null pair_index or problem ids");
  const int Q = prob->num_problems, C = prob->chains_per_problem;
  int rc = check_shape(who, Q, C);
  if (rc != PHF_OK) return rc;
  if (!phf_de_population_ok(population))
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_de_round: population must be 4, 8, 16, 32 or 64");
  if (C % population != 0 || prob->chain_id_base % (uint32_t)population != 0)
    return phf_fail(PHF_ERR_INVALID_ARGUMENT,
                    "phf_hier_de_round: chains_per_problem and chain_id_base must be multiples of the population (populations are whole)");
  if (round < 1 || round > 0xFFFFFFFFLL) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_de_round: round must lie in [1, 2^32)");
  if (!(gamma > 0.0) || !(gamma < PHF_INF)) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_de_round: gamma must be positive and finite");
  if (!state || !workspace || !stats) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_de_round: null pointer");
  const int dim = 5 + 2 * pts->n_expts;
  if ((double)dim * Q * C > 2147483647.0)
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_de_round: (5 + 2 n_expts) * num_problems * num_chains must fit in an int32");
  if (workspace_bytes < (size_t)dim * Q * C * sizeof(double))
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_de_round: workspace smaller than phf_hier_de_workspace_bytes()");
  if (stats_bytes < stats_bytes_of(Q, C))
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_hier_de_round: stats smaller than phf_hier_de_stats_bytes()");
  DeArgs a = {};
  a.pts = *pts; a.prior = *prior;
  a.pair_index = prob->pair_index; a.problem_id = prob->problem_id; a.chain_offset = prob->chain_offset;
  a.chain_id_base = prob->chain_id_base;
  a.Q = Q; a.C = C; a.ncg = (C + 63) / 64; a.G = population;
  a.kind = gamma == 1.0 ? 1 : 0;
  a.round = (uint32_t)round;
  a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
  a.gamma = gamma;
  a.state = state; a.work = workspace; a.stats = reinterpret_cast<long long*>(stats); a.trace = trace;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int h = 0; h < 2; ++h) {
    a.h = h;
    if ((rc = dispatch_round(a, s)) != PHF_OK) return rc;
  }
  return PHF_OK;
}

// phf_replica_exchange.hip — replica-exchange (parallel-tempering) swaps between the rungs of PyHillTemp's ladder
// (include/pyhillfit_amd.h; DESIGN.md §3, "phf_replica_exchange.hip").
//
// Layout: the single-level sampler's state [S][Q*C] with Q = P*R problems, pair-major, rungs in temperature order (problem
// p*R + k = rung k of pair p).  Round s proposes the rung pairs (k, k+1) with k = s (mod 2) (the deterministic even-odd scheme of
// Syed, Bouchard-Cote, Deligiannidis & Doucet 2022).  Chain c of rung k swaps only with chain c of rung k+1: the C chain indices stay
// independent replica sets.  With x the state at rung k and y the one at rung k+1, the swap is accepted iff
//     log u < (t_k+1 - t_k) (l_x - l_y),
// l the untempered log-likelihood the state keeps (field 2d+3+d(d+1)/2): no likelihood is evaluated.  A NaN rejects; l = -inf moving
// to t > 0 is rejected by the formula itself.  On accept theta[d] and l change slots, and each slot's log-target becomes
// (t == 0 ? 0 : t l) + prior(theta) at its own temperature — phf_sl_log_target's arithmetic, so the sampler continues from the very
// double it would hold itself.  Mean, covariance, loga and acceptance count stay with the slot (they belong to the rung's sampler).
//
// Random stream (one Philox block of the samplers' rounds per (replica set, pair, round)):
//   counter = (chain id, problem id of rung k, s, PHF_RX_DOMAIN), key = seed;  u = phf_uniform53(words 0, 1).
// Domain map of counter word 3: the samplers' own draws 0 (single-level) and small block indices (hierarchical), posterior predictive
// checks PHF_PPC_DOMAIN | block = 0x80000000 | b, replica exchange PHF_RX_DOMAIN = 0x40000000: pairwise disjoint.
//
// Labels: an int32 per slot that moves with its state: bits 0..27 the rung the replica started on, PHF_RX_SEEN_BOTTOM once it has
// visited rung 0, PHF_RX_HEADING_DOWN (the direction bit) once it has also reached rung R-1 since; arriving at rung 0 with the
// direction bit set completes a round trip 0 -> R-1 -> 0, counted per (pair, chain).
// Statistics (int64, no atomics): attempts and accepts per (pair, rung pair, 64-chain group), each written by the one wavefront that
// owns it in a round; round trips per (pair, chain), written only by the lane that proposes (0, 1) for that chain.  The readback
// sums the chain groups in a fixed order.
//
// Mapping: one lane per (pair, proposed rung pair, chain); a wavefront = 64 chains of one rung pair, so both temperatures are
// wave-uniform.  No grid-wide synchronisation, no waiting on other workgroups, no scratch: every slot is touched by one lane.
#include <hip/hip_runtime.h>

#include "../../include/pyhillfit_amd.h"
#include "phf_common.h"
#include "phf_model.h"

#define PHF_RX_DOMAIN 0x40000000u            /* counter word 3 of every swap block */
#define PHF_RX_SEEN_BOTTOM (1 << 30)
#define PHF_RX_HEADING_DOWN (1 << 29)
#define PHF_RX_REPLICA_MASK ((1 << 28) - 1)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct RxArgs {
  const double* temperature;      // [Q]
  const uint32_t* problem_id;     // [Q]
  const uint32_t* chain_offset;   // [Q] or NULL
  uint32_t chain_id_base;
  int32_t P, R, C, ncg, npp, parity;
  uint32_t round;
  uint32_t seed_lo, seed_hi;
  int32_t units;
  double* state;                  // [S][Q*C]
  int32_t* labels;                // [Q*C]
  long long* stats;               // attempts [P][R-1][ncg], accepts [P][R-1][ncg], trips [P][C]
  double* trace;                  // [P][R-1][C][3] (u, log u, log alpha) or NULL
};

__device__ inline int arrive(int label, int rung, int R, bool* trip) {
  *trip = false;
  if (rung == R - 1 && (label & PHF_RX_SEEN_BOTTOM)) label |= PHF_RX_HEADING_DOWN;
  if (rung == 0) {
    *trip = (label & PHF_RX_HEADING_DOWN) != 0;
    label = (label & ~PHF_RX_HEADING_DOWN) | PHF_RX_SEEN_BOTTOM;
  }
  return label;
}

template <int MODEL>
__global__ __launch_bounds__(kThreads) void rx_round_kernel(const RxArgs a) {
  PHF_MATH_TABLES_TO_LDS();
  constexpr int D = MODEL + 1;
  constexpr int NTRI = D * (D + 1) / 2;
  constexpr int LT = D, LL = 2 * D + 3 + NTRI;   // state fields: log-target, untempered log-likelihood
  const int unit = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves + threadIdx.x / 64));   // wave-uniform
  if (unit >= a.units) return;
  const int per_pair = a.npp * a.ncg;
  const int p = unit / per_pair;
  const int j = (unit - p * per_pair) / a.ncg, cg = unit - p * per_pair - j * a.ncg;
  const int k = a.parity + 2 * j;
  const int lane = threadIdx.x & 63;
  const int c = cg * 64 + lane;
  const bool active = c < a.C;
  const int qa = p * a.R + k, qb = qa + 1;
  const double ta = a.temperature[qa], tb = a.temperature[qb];
  const size_t nchains = (size_t)a.P * a.R * a.C;
  bool acc = false;
  if (active) {
    PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
    const size_t ga = (size_t)qa * a.C + c, gb = (size_t)qb * a.C + c;
    double* sa = a.state + ga;
    double* sb = a.state + gb;
    const double ll_a = sa[(size_t)LL * nchains], ll_b = sb[(size_t)LL * nchains];
    const uint32_t cid = a.chain_id_base + (a.chain_offset ? a.chain_offset[qa] : 0u) + (uint32_t)c;
    const phf_u32x4 w = phf_philox_mh(cid, a.problem_id[qa], a.round, PHF_RX_DOMAIN, a.seed_lo, a.seed_hi);
    const double u = phf_uniform53(w.w[0], w.w[1]);
    const double log_u = (u < PHF_DBL_MIN) ? -PHF_INF : phf_log_pos_k(u, k_log);   // u == 0 (probability 2^-53): accept unless NaN
    const double log_alpha = (tb - ta) * (ll_a - ll_b);
    acc = log_u < log_alpha;
    if (a.trace) {
      double* tr = a.trace + (((size_t)p * (a.R - 1) + k) * a.C + c) * 3;
      tr[0] = u; tr[1] = log_u; tr[2] = log_alpha;
    }
    if (acc) {
      double xa[D], xb[D];
#pragma unroll
      for (int i = 0; i < D; ++i) { xa[i] = sa[(size_t)i * nchains]; xb[i] = sb[(size_t)i * nchains]; }
      // slot a (rung k) receives y, slot b (rung k+1) receives x
      double lik_a = ta * ll_b, lik_b = tb * ll_a;
      if (ta == 0.0) lik_a = 0.0;
      if (tb == 0.0) lik_b = 0.0;
      const double lt_a = lik_a + phf_sl_log_prior(MODEL, xb, k_log);
      const double lt_b = lik_b + phf_sl_log_prior(MODEL, xa, k_log);
#pragma unroll
      for (int i = 0; i < D; ++i) { sa[(size_t)i * nchains] = xb[i]; sb[(size_t)i * nchains] = xa[i]; }
      sa[(size_t)LT * nchains] = lt_a; sb[(size_t)LT * nchains] = lt_b;
      sa[(size_t)LL * nchains] = ll_b; sb[(size_t)LL * nchains] = ll_a;
      bool trip_a, trip_b;
      const int lab_a = arrive(a.labels[gb], k, a.R, &trip_a);
      const int lab_b = arrive(a.labels[ga], k + 1, a.R, &trip_b);
      a.labels[ga] = lab_a;
      a.labels[gb] = lab_b;
      if (trip_a) {                                                // k == 0: only this lane writes the chain's count
        const size_t tw = 2 * (size_t)a.P * (a.R - 1) * a.ncg + (size_t)p * a.C + c;
        a.stats[tw] = a.stats[tw] + 1;
      }
    }
  }
  const unsigned long long tried = __ballot(active), taken = __ballot(acc);
  if (lane == 0) {
    const size_t at = ((size_t)p * (a.R - 1) + k) * a.ncg + cg;
    const size_t half = (size_t)a.P * (a.R - 1) * a.ncg;
    a.stats[at] = a.stats[at] + __popcll(tried);
    a.stats[half + at] = a.stats[half + at] + __popcll(taken);
  }
}

// out: attempts [P][R-1], accepts [P][R-1], trips [P][C]; one thread per entry, chain groups summed in order
__global__ __launch_bounds__(kThreads) void rx_stats_kernel(int P, int R, int C, int ncg, const long long* stats, long long* out) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const long long pr = (long long)P * (R - 1);
  if (i < 2 * pr) {
    const long long* s = stats + i * ncg;
    long long v = 0;
    for (int g = 0; g < ncg; ++g) v += s[g];
    out[i] = v;
  } else if (i < 2 * pr + (long long)P * C) {
    out[i] = stats[2 * pr * ncg + (i - 2 * pr)];
  }
}

__global__ __launch_bounds__(kThreads) void rx_labels_kernel(int P, int R, int C, int32_t* labels) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (long long)P * R * C) return;
  const int k = (int)((i / C) % R);
  labels[i] = k | (k == 0 ? PHF_RX_SEEN_BOTTOM : 0);
}

int check_shape(const char* who, int num_pairs, int rungs, int num_chains) {
  if (num_pairs < 1 || num_chains < 1 || rungs < 2 || rungs > PHF_RX_REPLICA_MASK)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: num_pairs and num_chains must be positive and rungs_per_pair at least 2", who);
  if ((double)num_pairs * rungs * num_chains > 2147483647.0)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: num_pairs * rungs_per_pair * num_chains must fit in an int32", who);
  return PHF_OK;
}

size_t stats_bytes_of(int P, int R, int C) {
  const size_t ncg = (size_t)(C + 63) / 64;
  return (2 * (size_t)P * (R - 1) * ncg + (size_t)P * C) * sizeof(long long);
}

unsigned blocks_for(long long n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

extern "C" size_t phf_replica_exchange_stats_bytes(int num_pairs, int rungs_per_pair, int num_chains) {
  if (check_shape("phf_replica_exchange_stats_bytes", num_pairs, rungs_per_pair, num_chains) != PHF_OK) return 0;
  return stats_bytes_of(num_pairs, rungs_per_pair, num_chains);
}

extern "C" int phf_replica_exchange_stats_init(int num_pairs, int rungs_per_pair, int num_chains, int64_t* stats, size_t stats_bytes,
                                               void* stream) {
  int rc = check_shape("phf_replica_exchange_stats_init", num_pairs, rungs_per_pair, num_chains);
  if (rc != PHF_OK) return rc;
  if (!stats) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_replica_exchange_stats_init: null stats");
  const size_t need = stats_bytes_of(num_pairs, rungs_per_pair, num_chains);
  if (stats_bytes < need)
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_replica_exchange_stats_init: stats smaller than phf_replica_exchange_stats_bytes()");
  if ((rc = phf_require_device_memory(stats, "phf_replica_exchange_stats_init: stats")) != PHF_OK) return rc;
  if (hipMemsetAsync(stats, 0, need, static_cast<hipStream_t>(stream)) != hipSuccess) return phf_check_launch("phf_replica_exchange_stats_init");
  return PHF_OK;
}

extern "C" int phf_replica_exchange_stats_read(int num_pairs, int rungs_per_pair, int num_chains, const int64_t* stats, size_t stats_bytes,
                                               int64_t* out, void* stream) {
  int rc = check_shape("phf_replica_exchange_stats_read", num_pairs, rungs_per_pair, num_chains);
  if (rc != PHF_OK) return rc;
  if (!stats || !out) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_replica_exchange_stats_read: null pointer");
  if (stats_bytes < stats_bytes_of(num_pairs, rungs_per_pair, num_chains))
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_replica_exchange_stats_read: stats smaller than phf_replica_exchange_stats_bytes()");
  const long long n = 2LL * num_pairs * (rungs_per_pair - 1) + (long long)num_pairs * num_chains;
  hipLaunchKernelGGL(rx_stats_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), num_pairs, rungs_per_pair,
                     num_chains, (num_chains + 63) / 64, reinterpret_cast<const long long*>(stats), reinterpret_cast<long long*>(out));
  return phf_check_launch("rx_stats_kernel");
}

extern "C" int phf_replica_exchange_labels_init(int num_pairs, int rungs_per_pair, int num_chains, int32_t* labels, void* stream) {
  int rc = check_shape("phf_replica_exchange_labels_init", num_pairs, rungs_per_pair, num_chains);
  if (rc != PHF_OK) return rc;
  if (!labels) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_replica_exchange_labels_init: null labels");
  if ((rc = phf_require_device_memory(labels, "phf_replica_exchange_labels_init: labels")) != PHF_OK) return rc;
  hipLaunchKernelGGL(rx_labels_kernel, dim3(blocks_for((long long)num_pairs * rungs_per_pair * num_chains)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), num_pairs, rungs_per_pair, num_chains, labels);
  return phf_check_launch("rx_labels_kernel");
}

extern "C" int phf_replica_exchange_round(const phf_problems* prob, int model, int rungs_per_pair, int64_t round, uint64_t seed,
                                          double* state, int32_t* labels, int64_t* stats, size_t stats_bytes, double* trace, void* stream) {
  static const char* who = "phf_replica_exchange_round";
  if (!prob || !prob->temperature || !prob->problem_id)
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_replica_exchange_round: null problems, temperatures or problem ids");
  if (model != 1 && model != 2) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_replica_exchange_round: model must be 1 or 2");
  if (rungs_per_pair < 2 || prob->num_problems % rungs_per_pair != 0)
    return phf_fail(PHF_ERR_INVALID_ARGUMENT,
                    "phf_replica_exchange_round: num_problems must be a whole number of pairs of rungs_per_pair >= 2 rungs");
  const int P = prob->num_problems / rungs_per_pair, C = prob->chains_per_problem;
  int rc = check_shape(who, P, rungs_per_pair, C);
  if (rc != PHF_OK) return rc;
  if (round < 1 || round > 0xFFFFFFFFLL)
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_replica_exchange_round: round must lie in [1, 2^32)");
  if (!state || !labels || !stats) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_replica_exchange_round: null pointer");
  if (stats_bytes < stats_bytes_of(P, rungs_per_pair, C))
    return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_replica_exchange_round: stats smaller than phf_replica_exchange_stats_bytes()");
  RxArgs a = {};
  a.temperature = prob->temperature; a.problem_id = prob->problem_id; a.chain_offset = prob->chain_offset;
  a.chain_id_base = prob->chain_id_base;
  a.P = P; a.R = rungs_per_pair; a.C = C; a.ncg = (C + 63) / 64;
  a.parity = (int)(round & 1);
  a.npp = (rungs_per_pair - a.parity) / 2;                         // k = parity, parity + 2, ... while k + 1 < R
  a.round = (uint32_t)round;
  a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
  a.state = state; a.labels = labels; a.stats = reinterpret_cast<long long*>(stats); a.trace = trace;
  if ((double)P * a.npp * a.ncg > 2147483647.0) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_replica_exchange_round: launch grid too large");
  a.units = P * a.npp * a.ncg;
  if (a.units == 0) return PHF_OK;
  const dim3 grid((unsigned)((a.units + kWaves - 1) / kWaves)), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (model == 1) hipLaunchKernelGGL(rx_round_kernel<1>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(rx_round_kernel<2>, grid, block, 0, s, a);
  return phf_check_launch("rx_round_kernel");
}

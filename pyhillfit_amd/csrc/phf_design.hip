// phf_design.hip — expected information gain of one further measurement at candidate doses (phf_design.h; DESIGN.md §3, "Next dose"):
// the per-(problem, dose, slot) sums of the K + 2 category masses and of the two entropies over the draws of the samplers' rows.
//
// Mapping: one wavefront per (problem, dose, slot); slot s takes the chains c with c mod NS == s, so the wavefront's draws are the
// call's used rows in row order and, within a row, its chains in ascending order.  The wavefront walks them 64 at a time: lane l loads
// draw base + l (pIC50, Hill, sigma), decides whether it is used and computes its prediction at the dose and 1 / (sigma sqrt 2) — one
// draw per lane, so the Hill curve and the division cost each draw one lane-operation, not 64 — and a ballot counts the used and the
// skipped.  Then, draw by draw in order, the two numbers are broadcast from their lane (v_readlane, the lane index is wave-uniform)
// and every lane adds the masses of its K/64 bins and its shares of the two entropies to the sums it keeps in registers
// (phf_ds_lane_add: the host twin runs the very same function for lanes 0..63).  The sums start from the accumulator's stored
// values and go back there at the end: however the calls cut the rows, every sum sees the same additions in the same order, so
// the same rows and the same `every` give the same bits.  No atomics, nothing merged across lanes; exp2, log and erfc tables in LDS.
#include <hip/hip_runtime.h>

#include "../../include/pyhillfit_amd.h"
#include "phf_common.h"
#include "phf_design.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct DsArgs {
  const double* rows;             // [nr][Q][stride_cols][C]; the first used row of the call is local row r0, then every `every`-th
  const double* ln_doses;         // [Q][G]
  double* acc;                    // [Q][G][NS][PHF_DS_ACC_DOUBLES(K)]
  int64_t r0, used;
  int32_t model, every, Q, stride_cols, C, G, NS;
};

__device__ __forceinline__ double lane_value(double v, int l) {          // v of lane l, l wave-uniform
  const uint64_t u = phf_bits(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), l);
  return phf_from_bits(((uint64_t)hi << 32) | lo);
}

template <int NB>
__global__ __launch_bounds__(kThreads) void design_kernel(const DsArgs a) {
  constexpr int K = NB * PHF_DS_LANES;
  PHF_MATH_TABLES_TO_LDS();
  PHF_ERFC_TABLE_TO_LDS();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
  const int unit = (int)blockIdx.x * kWaves + wave;                      // wave-uniform: (problem, dose, slot)
  if (unit >= a.Q * a.G * a.NS) return;
  const int lane = threadIdx.x & 63;
  const int slot = unit % a.NS, g = (unit / a.NS) % a.G, q = unit / (a.NS * a.G);
  if (slot >= a.C) return;                                               // a slot without chains: its accumulator stays as it is
  const int chains = (a.C - slot + a.NS - 1) / a.NS;                     // chains slot, slot + NS, ... < C
  const int64_t draws = a.used * chains;
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  const double ln_dose = a.ln_doses[(size_t)q * a.G + g];
  double* acc = a.acc + (size_t)unit * PHF_DS_ACC_DOUBLES(K);
  double m[NB], pt, hf = acc[PHF_DS_OFF_HF(K) + lane], hc = acc[PHF_DS_OFF_HC(K) + lane];
  PHF_UNROLL
  for (int b = 0; b < NB; ++b) m[b] = acc[1 + lane * NB + b];
  pt = (lane == 0) ? acc[0] : ((lane == PHF_DS_LANES - 1) ? acc[K + 1] : 0.0);
  int64_t n_used = 0, n_skipped = 0;
  const size_t C = (size_t)a.C;
  for (int64_t base = 0; base < draws; base += 64) {
    const int64_t d = base + lane;
    const bool have = d < draws;
    double pic50 = 0.0, hill = 1.0, sigma = 0.0;
    if (have) {
      const int64_t u = d / chains;
      const int c = slot + (int)(d - u * chains) * a.NS;
      const double* x = a.rows + (((size_t)(a.r0 + u * a.every) * a.Q + q) * a.stride_cols) * C + c;
      pic50 = x[0];
      hill = (a.model == 1) ? 1.0 : x[C];
      sigma = x[(size_t)a.model * C];
    }
    const bool ok = have && phf_ds_draw_ok(a.model, pic50, hill, sigma);
    double pred, scale;
    phf_ds_draw_terms(a.model, ln_dose, pic50, hill, sigma, k_exp, &pred, &scale);
    const uint64_t ok_mask = __builtin_amdgcn_ballot_w64(ok);
    const int n = (int)(draws - base < 64 ? draws - base : 64);          // wave-uniform
    const int n_ok = __builtin_popcountll(ok_mask);
    n_used += n_ok;
    n_skipped += n - n_ok;
    for (int l = 0; l < n; ++l) {
      if (!((ok_mask >> l) & 1)) continue;                               // a wave-uniform branch
      const double p = lane_value(pred, l), s = lane_value(scale, l);
      phf_ds_lane_add(lane, NB, p, s, k_log, m, &pt, &hf, &hc);
    }
  }
  PHF_UNROLL
  for (int b = 0; b < NB; ++b) acc[1 + lane * NB + b] = m[b];
  if (lane == 0) {
    acc[0] = pt;
    acc[PHF_DS_OFF_USED(K)] += (double)n_used;
    acc[PHF_DS_OFF_SKIPPED(K)] += (double)n_skipped;
  }
  if (lane == PHF_DS_LANES - 1) acc[K + 1] = pt;
  acc[PHF_DS_OFF_HF(K) + lane] = hf;
  acc[PHF_DS_OFF_HC(K) + lane] = hc;
}

}  // namespace

extern "C" int phf_design_accumulator_doubles(int bins) { return phf_ds_bins_ok(bins) ? PHF_DS_ACC_DOUBLES(bins) : -1; }

extern "C" int64_t phf_design_rows_used(int64_t first_row, int64_t num_rows, int every) {
  if (first_row < 0 || num_rows < 0 || every < 1) return -1;
  return phf_ds_rows_used(first_row, num_rows, every);
}

extern "C" int phf_design_accumulate(int model, int bins, const double* rows, int64_t num_rows, int num_problems, int row_stride_cols,
                                     int num_chains, int64_t first_row, int every, const double* ln_doses, int num_doses, int num_slots,
                                     double* accumulators, size_t accumulator_bytes, void* stream) {
  static const char* who = "phf_design_accumulate";
  if (model != 1 && model != 2)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: model must be 1 or 2 (single-level), got %d", who, model);
  if (!phf_ds_bins_ok(bins))
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: bins must be 128, 256, 512 or 1024 (got %d)", who, bins);
  if (num_doses < 1) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_design_accumulate: num_doses must be >= 1");
  if (every < 1) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_design_accumulate: every must be >= 1");
  if (num_chains < 1) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_design_accumulate: num_chains must be positive");
  if (num_problems < 1) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_design_accumulate: num_problems must be positive");
  if (!phf_ds_slots_ok(num_slots))
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: num_slots must be even and in 2..%d (got %d)", who, PHF_DS_MAX_SLOTS, num_slots);
  if (row_stride_cols < model + 1)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: row_stride_cols is smaller than the %d parameter columns of model %d", who, model + 1, model);
  if (num_rows < 0 || first_row < 0) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_design_accumulate: num_rows and first_row must be >= 0");
  const int64_t units = (int64_t)num_problems * num_doses * num_slots;
  if (units > 2147483647ll - kWaves) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_design_accumulate: too many (problem, dose, slot) units");
  if (accumulator_bytes < (size_t)units * PHF_DS_ACC_DOUBLES(bins) * sizeof(double))
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: the accumulators are smaller than num_problems x num_doses x num_slots x %d doubles", who,
                     PHF_DS_ACC_DOUBLES(bins));
  const int64_t used = phf_ds_rows_used(first_row, num_rows, every);
  if (used == 0) return PHF_OK;                                          // no row of the call is used: no launch
  if (!rows || !ln_doses || !accumulators) return phf_fail(PHF_ERR_INVALID_ARGUMENT, "phf_design_accumulate: null pointer");
  DsArgs a = {};
  a.rows = rows; a.ln_doses = ln_doses; a.acc = accumulators;
  a.r0 = (every - first_row % every) % every; a.used = used;
  a.model = model; a.every = every; a.Q = num_problems; a.stride_cols = row_stride_cols; a.C = num_chains; a.G = num_doses; a.NS = num_slots;
  const dim3 grid((unsigned)((units + kWaves - 1) / kWaves)), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (bins) {
    case 128: hipLaunchKernelGGL(design_kernel<2>, grid, block, 0, s, a); break;
    case 256: hipLaunchKernelGGL(design_kernel<4>, grid, block, 0, s, a); break;
    case 512: hipLaunchKernelGGL(design_kernel<8>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(design_kernel<16>, grid, block, 0, s, a); break;
  }
  return phf_check_launch(who);
}

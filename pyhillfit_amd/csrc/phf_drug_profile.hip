// phf_drug_profile.hip — the per-drug multi-channel block profile at given concentrations (include/pyhillfit_amd.h; the values and
// the decision rules are phf_drug_profile.h's).
//
// The workspace starts with a quantiles workspace (phf_quantiles.hip) of `drugs` problems, no columns and D (K + 1) curve points:
// slot (drug, dose j, component k) is curve point j (K + 1) + k of problem `drug`, k < K the block of channel k and k = K the net
// block.  The slots are binned on the grid of phf_grid.h by its prepare and bin passes and reduced by phf_quantiles_reduce itself.
// After it stand the tallies, uint64 [drugs][D][2][K + 3]: per chain parity the draws whose dominant channel is k, whose net block is
// positive, the draws used and the draws skipped.  Each accumulate call runs
//   prepare  one workgroup per slot;
//   bin      workgroups of (slot, slice of the call's draws);
//   tally    workgroups of (drug, dose, slice of the call's draws): lane t of a wavefront keeps tally t of the draws its wavefront has
//            seen (a ballot per tally), and adds it to the workspace with one integer atomic at the end.
// A value is a pure function of (slot, row, chain) that reads the rows of up to K problems through map; draw i of a call is row i / C,
// chain i % C, so a wavefront's loads run along the chains, the contiguous dimension of the rows.  Everything kept is an integer
// count: the result is bit-identical whatever the launch shape, the arrival order or the row cuts.
#include <hip/hip_runtime.h>

#include "../../include/pyhillfit_amd.h"
#include "phf_drug_profile.h"
#include "phf_grid.h"
#include "phf_host_checks.h"

namespace {

constexpr int kBinThreads = 512;
constexpr int kTallyThreads = 256;
constexpr int kHdr = PHF_GRID_HDR;
constexpr int kMaxBins = 32768;               // phf_quantiles_reduce's
constexpr int64_t kMaxFlat = 0x7fffffff;      // rows x chains of one call: a 31-bit flat index

struct DArgs {
  phf_dp_view v;
  unsigned n;                     // nr * C draws in this call
  int drugs, B;
  int splits;
  unsigned per_split;
  unsigned long long* counts;     // [S][B], S = drugs D (K + 1)
  double* hdr;                    // [S][kHdr]
  unsigned long long* nonfinite;  // [S]
  unsigned long long* tally;      // [drugs][D][2][K + 3]
};

struct Slot {
  int drug, j, comp;
  size_t s;
};

__device__ inline Slot slot_of(const DArgs& a, int index) {
  Slot t;
  t.comp = index % (a.v.K + 1);
  t.j = index / (a.v.K + 1) % a.v.D;
  t.drug = index / ((a.v.K + 1) * a.v.D);
  t.s = (size_t)index;
  return t;
}

// the 2^(j/64) table of phf_exp_* into LDS (the Hill curve needs no other table)
__device__ inline void exp_table_to_lds() {
#if defined(__HIP_DEVICE_COMPILE__)
  for (int i = threadIdx.x; i < 64; i += blockDim.x) phf_lds_exp2[i] = phf_t_exp2[i];
  __syncthreads();
#endif
}

template <int MODEL>
__device__ inline double dp_value(const DArgs& a, const Slot& t, unsigned i, phf_ktab k_exp) {
  const unsigned r = i / (unsigned)a.v.C, c = i - r * (unsigned)a.v.C;
  return phf_dp_slot_value(MODEL, &a.v, t.drug, t.j, t.comp, (int64_t)r, (int)c, k_exp);
}

template <int MODEL>
__global__ __launch_bounds__(kGridPrepThreads) void dp_prepare_kernel(const DArgs a) {
  extern __shared__ unsigned long long s_merge[];              // [B/2]
  exp_table_to_lds();
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  const Slot t = slot_of(a, blockIdx.x);
  if (!phf_dp_slot_live(&a.v, t.drug, t.j, t.comp)) return;    // the whole workgroup: a slot that is never fed
  phf_grid_prepare<1>(a.hdr + t.s * kHdr, a.counts + t.s * a.B, a.B, a.n, s_merge,
                      [&](unsigned i) { return dp_value<MODEL>(a, t, i, k_exp); });
}

template <int MODEL>
__global__ __launch_bounds__(kBinThreads) void dp_bin_kernel(const DArgs a) {
  extern __shared__ unsigned s_hist[];                          // [B]
  exp_table_to_lds();
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  const Slot t = slot_of(a, blockIdx.x / a.splits);
  if (!phf_dp_slot_live(&a.v, t.drug, t.j, t.comp)) return;
  unsigned i0, i1;
  phf_grid_split_range(a.n, blockIdx.x % a.splits, a.per_split, &i0, &i1);
  phf_grid_bin_values<kBinThreads>(a.hdr + t.s * kHdr, a.counts + t.s * a.B, a.nonfinite + t.s, a.B, i0, i1, s_hist,
                                   [&](unsigned i) { return dp_value<MODEL>(a, t, i, k_exp); });
}

template <int MODEL>
__global__ __launch_bounds__(kTallyThreads) void dp_tally_kernel(const DArgs a) {
  exp_table_to_lds();
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  const int pair = blockIdx.x / a.splits, drug = pair / a.v.D, j = pair % a.v.D;
  const int K = a.v.K, T = PHF_DP_TALLIES(K);                    // 2 T <= 64: one lane per (parity, tally)
  if (!phf_dp_dose_live(&a.v, drug, j)) return;                  // the whole workgroup: a dose the drug does not have
  unsigned i0, i1;
  phf_grid_split_range(a.n, blockIdx.x % a.splits, a.per_split, &i0, &i1);
  const int lane = __lane_id();
  unsigned mine = 0;
  // whole wavefronts enter every trip (the ballots below want the lanes past i1 present and voting 0)
  for (unsigned base = i0 + (threadIdx.x - lane); base < i1; base += kTallyThreads) {
    const unsigned i = base + lane;
    const bool here = i < i1;
    double net = 0.0;
    int dominant = -1, ok = 0, parity = 0;
    if (here) {
      const unsigned r = i / (unsigned)a.v.C, c = i - r * (unsigned)a.v.C;
      ok = phf_dp_draw(MODEL, &a.v, drug, j, (int64_t)r, (int)c, k_exp, &net, &dominant);
      parity = (int)(c & 1u);
    }
    for (int t = 0; t < 2 * T; ++t) {
      const int par = t >= T, which = par ? t - T : t;
      const unsigned long long hits = __ballot(here && parity == par && phf_dp_tally_hit(which, K, ok, net, dominant));
      if (lane == t) mine += (unsigned)__popcll(hits);
    }
  }
  if (lane < 2 * T && mine) atomicAdd(&a.tally[(size_t)pair * 2 * T + lane], (unsigned long long)mine);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
struct Layout {
  size_t slots, grid_bytes, counts_bytes, hdr_bytes, tally_bytes;
  size_t total() const { return grid_bytes + tally_bytes; }
};

// the grid part is the quantiles workspace of (drugs, 0 columns, D (K + 1) curve points): counts, headers, non-finite counts
Layout layout_of(int drugs, int K, int D, int bins) {
  Layout l;
  l.slots = (size_t)drugs * D * (K + 1);
  l.counts_bytes = l.slots * (size_t)bins * 8;
  l.hdr_bytes = l.slots * kHdr * 8;
  l.grid_bytes = l.counts_bytes + l.hdr_bytes + l.slots * 8;
  l.tally_bytes = (size_t)drugs * D * 2 * PHF_DP_TALLIES(K) * 8;
  return l;
}

int check_geometry(const char* who, int drugs, int K, int D, int bins) {
  if (drugs < 1 || K < 1 || K > PHF_DP_MAX_CHANNELS || D < 1 || D > PHF_DP_MAX_DOSES)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: num_drugs must be positive, num_channels in [1, %d] and num_doses in [1, %d]", who,
                     PHF_DP_MAX_CHANNELS, PHF_DP_MAX_DOSES);
  if (phf_grid_check_bins(who, bins, kMaxBins) != PHF_OK) return PHF_ERR_INVALID_ARGUMENT;
  if ((double)drugs * D * (K + 1) > 2147483647.0 / 8)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: too many slots (fewer drugs per workspace)", who);
  if (layout_of(drugs, K, D, bins).grid_bytes != phf_quantiles_workspace_bytes(drugs, 0, D * (K + 1), bins))
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: the slots do not form a quantiles workspace", who);
  return PHF_OK;
}

template <int MODEL>
int launch(DArgs a, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int slots = a.drugs * a.v.D * (a.v.K + 1), pairs = a.drugs * a.v.D;
  const size_t merge_lds = (size_t)a.B / 2 * 8, hist_lds = (size_t)a.B * 4;
  int rc;
  if ((rc = allow_lds(dp_prepare_kernel<MODEL>, merge_lds, "hipFuncSetAttribute(dp_prepare_kernel)")) != PHF_OK) return rc;
  if ((rc = allow_lds(dp_bin_kernel<MODEL>, hist_lds, "hipFuncSetAttribute(dp_bin_kernel)")) != PHF_OK) return rc;
  hipLaunchKernelGGL(dp_prepare_kernel<MODEL>, dim3(slots), dim3(kGridPrepThreads), merge_lds, st, a);
  if ((rc = phf_check_launch("dp_prepare_kernel")) != PHF_OK) return rc;
  phf_grid_split split = phf_grid_split_of(a.n, slots);
  a.splits = split.splits; a.per_split = split.per_split;
  hipLaunchKernelGGL(dp_bin_kernel<MODEL>, dim3((unsigned)slots * a.splits), dim3(kBinThreads), hist_lds, st, a);
  if ((rc = phf_check_launch("dp_bin_kernel")) != PHF_OK) return rc;
  split = phf_grid_split_of(a.n, pairs);
  a.splits = split.splits; a.per_split = split.per_split;
  hipLaunchKernelGGL(dp_tally_kernel<MODEL>, dim3((unsigned)pairs * a.splits), dim3(kTallyThreads), 0, st, a);
  return phf_check_launch("dp_tally_kernel");
}

}  // namespace

extern "C" size_t phf_drug_profile_workspace_bytes(int num_drugs, int num_channels, int num_doses, int bins) {
  if (check_geometry("phf_drug_profile_workspace_bytes", num_drugs, num_channels, num_doses, bins) != PHF_OK) return 0;
  return layout_of(num_drugs, num_channels, num_doses, bins).total();
}

extern "C" size_t phf_drug_profile_tally_offset(int num_drugs, int num_channels, int num_doses, int bins) {
  if (check_geometry("phf_drug_profile_tally_offset", num_drugs, num_channels, num_doses, bins) != PHF_OK) return 0;
  return layout_of(num_drugs, num_channels, num_doses, bins).grid_bytes;
}

extern "C" double phf_drug_profile_default_weight(const char* channel) {
  return channel ? phf_dp_default_weight(channel) : 0.0;
}

extern "C" int phf_drug_profile_init(int num_drugs, int num_channels, int num_doses, int bins, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  static const char* who = "phf_drug_profile_init";
  int rc = check_geometry(who, num_drugs, num_channels, num_doses, bins);
  if (rc != PHF_OK) return rc;
  const size_t need = layout_of(num_drugs, num_channels, num_doses, bins).total();
  return phf_init_workspace(who, "drug_profile", workspace, workspace_bytes, need, need, stream);
}

extern "C" int phf_drug_profile_accumulate(const double* rows, int64_t num_rows, int num_problems, int row_stride_cols, int num_chains,
                                           int model, int num_drugs, int num_channels, int num_doses, const int32_t* channel_problem,
                                           const double* weights, const double* ln_doses, int bins, int64_t first_row,
                                           int64_t total_rows, void* workspace, size_t workspace_bytes, void* stream) {
  static const char* who = "phf_drug_profile_accumulate";
  int rc = check_geometry(who, num_drugs, num_channels, num_doses, bins);
  if (rc != PHF_OK) return rc;
  if (model != 1 && model != 2) return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: model must be 1 or 2", who);
  if ((rc = phf_check_positive(who, "num_problems, num_chains and row_stride_cols", {num_problems, num_chains, row_stride_cols})) != PHF_OK)
    return rc;
  if ((rc = phf_check_row_stride(who, row_stride_cols, model, "is smaller than the columns read (pIC50; model 2: Hill)")) != PHF_OK) return rc;
  if ((rc = phf_check_row_window(who, num_rows, first_row, total_rows)) != PHF_OK) return rc;
  if ((double)num_rows * num_chains > (double)kMaxFlat)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: num_rows x num_chains must stay below 2^31 per call (accumulate in shorter segments)", who);
  if (!channel_problem || !weights || !ln_doses)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: null channel_problem, weights or ln_doses", who);
  if (num_rows > 0 && !rows) return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: null rows", who);
  const Layout l = layout_of(num_drugs, num_channels, num_doses, bins);
  if ((rc = phf_check_workspace(who, "drug_profile", workspace, workspace_bytes, l.total())) != PHF_OK) return rc;
  if (num_rows == 0) return PHF_OK;
  DArgs a = {};
  a.v.rows = rows; a.v.map = channel_problem; a.v.weight = weights; a.v.ln_dose = ln_doses;
  a.v.Q = num_problems; a.v.stride = row_stride_cols; a.v.C = num_chains; a.v.K = num_channels; a.v.D = num_doses;
  a.n = (unsigned)(num_rows * num_chains);
  a.drugs = num_drugs; a.B = bins;
  char* base = static_cast<char*>(workspace);
  a.counts = reinterpret_cast<unsigned long long*>(base);
  a.hdr = reinterpret_cast<double*>(base + l.counts_bytes);
  a.nonfinite = reinterpret_cast<unsigned long long*>(base + l.counts_bytes + l.hdr_bytes);
  a.tally = reinterpret_cast<unsigned long long*>(base + l.grid_bytes);
  return model == 1 ? launch<1>(a, stream) : launch<2>(a, stream);
}

extern "C" int phf_drug_profile_reduce(int num_drugs, int num_channels, int num_doses, int bins, const double* probs, int num_probs,
                                       const void* workspace, size_t workspace_bytes, double* out, void* stream) {
  static const char* who = "phf_drug_profile_reduce";
  int rc = check_geometry(who, num_drugs, num_channels, num_doses, bins);
  if (rc != PHF_OK) return rc;
  const Layout l = layout_of(num_drugs, num_channels, num_doses, bins);
  if ((rc = phf_check_workspace(who, "drug_profile", workspace, workspace_bytes, l.total())) != PHF_OK) return rc;
  // the one quantile reduce, over the grid part of the workspace (its own checks: the probabilities, out)
  return phf_quantiles_reduce(num_drugs, 0, num_doses * (num_channels + 1), bins, probs, num_probs, workspace, l.grid_bytes, out, stream);
}

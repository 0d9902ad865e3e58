// phf_sensitivity.hip — power-scaling sensitivity of prior and likelihood, streamed over the samplers' rows (include/pyhillfit_amd.h;
// phf_sensitivity.h holds the arithmetic, shared with the host build the tests compare against).
//
// Per (problem, column) slot the workspace keeps, on ONE grid (phf_grid.h, the grid the quantiles bin on: the base counts here are
// the quantiles' counts), five uint64 arrays of B bins:
// the base counts and the integer masses m = floor(w 2^20 + 1/2) of the four (component, direction) weights.  Integer sums do not
// depend on the order: the arrays are identical however the rows arrive or are cut into calls.  Per (problem, component) c_ref is the
// first finite component in (row, chain) order of all rows accumulated.  Per (problem, component, direction, chain) sum w, sum w^2 and
// the clamped count, and per column sum w, sum w d, sum w d^2 (d = x - the slot's anchor), are owned by one lane in row order.
//
// An accumulate call walks its rows in blocks of the workspace's scratch region (so the region is bounded whatever the call's size):
//   components  lane = chain, wavefront = 64 chains of a problem (the problem's points are wave-uniform): the two components of every
//               draw, ONCE, into the scratch;
//   reference   one workgroup per (problem, component): c_ref, if it is not set yet;
//   weights     lane = chain: the four weights of every draw into the scratch (0 = the component is not finite), the chain's sums;
//   prepare     one workgroup per slot: anchor, min/max, level, the merge of the five arrays;
//   columns     wavefront = (problem, column, 64 chains): the chain's column sums of the base and the four weights, in registers;
//   bin         workgroups of (slot, slice of the block's values): uint32 counts and uint64 masses in LDS, flushed with integer atomics.
// reduce: one thread per (slot, component, direction) walks the bins in order (phf_sens_cjs_sums: the sums of the cumulative
// Jensen-Shannon divergence on the CDF and on the survival function); one thread per scalar merges the chains in chain order.  Only
// per-slot scalars leave the device.
#include <hip/hip_runtime.h>

#include "../../include/pyhillfit_amd.h"
#include "phf_host_checks.h"
#include "phf_grid.h"
#include "phf_sensitivity.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPrepThreads = kGridPrepThreads;
constexpr int kBinThreads = 512;
constexpr int kHdr = PHF_GRID_HDR;
constexpr int kArrays = 5;                    // base counts, then the masses of prior down / up, likelihood down / up
constexpr int kWeights = 4;
constexpr int kDraw = 6;                      // scratch doubles per draw: the two components, the four weights
constexpr int kWFields = 4;                   // per (weight, chain): n, sum w, sum w^2, clamped
constexpr int kCFields = 3;                   // per (column, array, chain): sum w, sum w d, sum w d^2
constexpr int kSlotHead = kGridOutHead;
constexpr int kSlotPerWeight = 5;             // numerator and denominator on the CDF, on the survival function, the total mass
constexpr int kSlotOut = kSlotHead + kWeights * kSlotPerWeight;
constexpr int kColOut = 4;                    // merged sum w, sum w d, sum w d^2; between-chain standard error of the mean shift (in d)
constexpr int kMaxBins = 4096;                // 36 bytes of LDS per bin in the bin kernel: 4 096 bins are 144 KiB of a CU's 160
constexpr size_t kScratchTarget = (size_t)256 << 20;   // the scratch region: about this many bytes ...
constexpr int64_t kMinBlockRows = 16;                  // ... but at least this many rows (or all of them)
// `kind` of phf_sensitivity_accumulate: which evaluator gives the two components.  Not the `likelihood` codes of phf_point_block.h
// (kHierarchical, kGiven), which this file does not include: another entry point's argument, with values that happen to agree
constexpr int kSingle1 = 1, kSingle2 = 2, kHier = 3, kGiven = 4;

struct Layout {
  size_t slots, counts, hdr, nonfinite, cref, wsum, csum, scratch;   // byte offsets; slots = Q * columns
  size_t persistent, total;
  int64_t block_rows;
};

Layout layout_of(int Q, int ncol, int C, int64_t total_rows, int B) {
  Layout l;
  l.slots = (size_t)Q * ncol;
  size_t at = 0;
  l.counts = at; at += l.slots * kArrays * (size_t)B * 8;
  l.hdr = at; at += l.slots * kHdr * 8;
  l.nonfinite = at; at += l.slots * 8;
  l.cref = at; at += (size_t)Q * 2 * 2 * 8;
  l.wsum = at; at += (size_t)Q * kWeights * kWFields * (size_t)C * 8;
  l.csum = at; at += l.slots * kArrays * kCFields * (size_t)C * 8;
  l.persistent = at;
  const size_t per_row = (size_t)Q * kDraw * (size_t)C * 8;
  int64_t rb = (int64_t)(kScratchTarget / per_row);
  rb = rb < kMinBlockRows ? kMinBlockRows : rb;
  rb = rb > total_rows ? total_rows : rb;
  l.block_rows = rb;
  l.scratch = at; at += (size_t)rb * per_row;
  l.total = at;
  return l;
}

struct SArgs {
  phf_points sl;
  phf_hier_points hp;
  phf_hier_prior prior;
  const double* rows;              // [nr][Q][stride][C], the block's first row
  int64_t nr;
  int32_t Q, stride, C, ncol, B, ncg, units;
  int32_t prior_col, lik_col;
  double am1[2];                   // alpha - 1 of the two directions
  unsigned n;                      // nr * C values per slot in this block
  int splits;
  unsigned per_split;
  unsigned long long* counts;      // [S][kArrays][B]
  double* hdr;                     // [S][kHdr]
  unsigned long long* nonfinite;   // [S]
  double* cref;                    // [Q][2][2]: value, set
  double* wsum;                    // [Q][kWeights][kWFields][C]
  double* csum;                    // [S][kArrays][kCFields][C]
  double* scratch;                 // [nr][Q][kDraw][C]
};

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- components ----------------------------------------------------------------------------------------------------------------------
// problem q's two components (and, hierarchical, the population term) at x[i * ts]
template <int KIND>
__device__ inline void components_at(const phf_points& sl, const phf_hier_points& hp, const phf_hier_prior& prior, int q, const double* x,
                                     int ts, phf_ktab k_exp, phf_ktab k_log, double* p, double* l, double* pop) {
  if (KIND == kHier) {
    const size_t at = (size_t)q * hp.stride;
    phf_sens_hier_components(hp.n_expts, hp.expt_start + (size_t)q * (hp.n_expts + 1), hp.stride, hp.ln_conc + at, hp.response + at, x, ts,
                             &prior, k_exp, k_log, p, l, pop);
  } else {
    constexpr int D = (KIND == kSingle1 ? 1 : 2) + 1;
    constexpr int MODEL = KIND == kSingle1 ? 1 : 2;
    const int32_t* cnt = sl.counts + 4 * q;
    const int n_other = clampi(cnt[0], 0, sl.stride), n_cens = clampi(cnt[1] + cnt[2], 0, sl.stride - n_other);
    const size_t at = (size_t)q * sl.stride;
    double th[D];
#pragma unroll
    for (int i = 0; i < D; ++i) th[i] = x[(size_t)i * ts];
    phf_sens_sl_components(MODEL, sl.ln_conc + at, sl.response + at, sl.weight + at, n_other, n_cens, sl.extra[2 * q], sl.extra[2 * q + 1],
                           sl.pi_bit[q], th, k_exp, k_log, p, l);
    *pop = 0.0;
  }
}

template <int KIND>
__device__ inline void tables_to_lds() {
  PHF_MATH_TABLES_TO_LDS();
  if (KIND == kHier) PHF_ERFC_TABLE_TO_LDS(); else if (KIND != kGiven) PHF_LOGPHI_TABLE_TO_LDS();
}

template <int KIND>
__global__ __launch_bounds__(kThreads) void sens_components_kernel(const SArgs a) {
  tables_to_lds<KIND>();
  const int unit = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves + threadIdx.x / 64));   // wave-uniform
  if (unit >= a.units) return;
  const int q = unit / a.ncg, cg = unit % a.ncg;
  const int c = cg * 64 + (threadIdx.x & 63);
  if (c >= a.C) return;
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  const size_t C = (size_t)a.C;
  const size_t rstep = (size_t)a.Q * a.stride * C, sstep = (size_t)a.Q * kDraw * C;
  const double* xr = a.rows + (size_t)q * a.stride * C + c;
  double* sr = a.scratch + (size_t)q * kDraw * C + c;
  for (int64_t r = 0; r < a.nr; ++r) {
    const double* x = xr + (size_t)r * rstep;
    double p, l, pop;
    if (KIND == kGiven) { p = x[(size_t)a.prior_col * C]; l = x[(size_t)a.lik_col * C]; }
    else components_at<KIND>(a.sl, a.hp, a.prior, q, x, a.C, k_exp, k_log, &p, &l, &pop);
    double* s = sr + (size_t)r * sstep;
    s[0] = p;
    s[C] = l;
  }
}

// batch evaluator: out [3][m] = prior, likelihood, population term (0 for the single-level models) of theta[.][i] ([d][m])
template <int KIND>
__global__ __launch_bounds__(kThreads) void sens_batch_kernel(const phf_points sl, const phf_hier_points hp, const phf_hier_prior prior,
                                                              int num_problems, int64_t m, const int32_t* problem_index, const double* theta,
                                                              double* out) {
  tables_to_lds<KIND>();
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  const int q = problem_index[i];
  double p = PHF_NAN, l = PHF_NAN, pop = PHF_NAN;
  if (q >= 0 && q < num_problems) {
    PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
    PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
    components_at<KIND>(sl, hp, prior, q, theta + i, (int)m, k_exp, k_log, &p, &l, &pop);
  }
  out[i] = p;
  out[m + i] = l;
  out[2 * m + i] = pop;
}

// scratch double f of draw i (= row * C + chain) of problem q
__device__ inline double* draw_at(const SArgs& a, int q, unsigned i, int f) {
  const unsigned r = i / (unsigned)a.C, c = i - r * (unsigned)a.C;
  return a.scratch + (((size_t)r * a.Q + q) * kDraw + f) * (size_t)a.C + c;
}

// ---- reference: c_ref = the first finite component in (row, chain) order -------------------------------------------------------------
__global__ __launch_bounds__(kPrepThreads) void sens_reference_kernel(const SArgs a) {
  __shared__ unsigned s_redu[16];
  const int q = blockIdx.x / 2, comp = blockIdx.x % 2;
  double* ref = a.cref + (size_t)blockIdx.x * 2;
  if (ref[1] != 0.0) return;                                    // set by an earlier block of rows (the same answer for every thread)
  unsigned best = 0xffffffffu;
  for (unsigned i = threadIdx.x; i < a.n; i += kPrepThreads)
    if (__builtin_isfinite(*draw_at(a, q, i, comp))) { best = i; break; }
  best = block_min_u(best, s_redu);
  if (best == 0xffffffffu) return;
  if (threadIdx.x == 0) { ref[0] = *draw_at(a, q, best, comp); ref[1] = 1.0; }
}

// ---- weights: the four weights of every draw, the chain's sums -----------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void sens_weights_kernel(const SArgs a) {
  PHF_MATH_TABLES_TO_LDS();
  const int unit = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves + threadIdx.x / 64));
  if (unit >= a.units) return;
  const int q = unit / a.ncg, cg = unit % a.ncg;
  const int c = cg * 64 + (threadIdx.x & 63);
  if (c >= a.C) return;
  const size_t C = (size_t)a.C;
  const double* ref = a.cref + (size_t)q * 4;
  const double cref[2] = {ref[0], ref[2]};
  const bool have[2] = {ref[1] != 0.0, ref[3] != 0.0};
  double* st = a.wsum + (size_t)q * kWeights * kWFields * C + c;
  double acc[kWeights][kWFields];
#pragma unroll
  for (int k = 0; k < kWeights; ++k)
#pragma unroll
    for (int f = 0; f < kWFields; ++f) acc[k][f] = st[((size_t)k * kWFields + f) * C];
  const size_t sstep = (size_t)a.Q * kDraw * C;
  double* sr = a.scratch + (size_t)q * kDraw * C + c;
  for (int64_t r = 0; r < a.nr; ++r) {
    double* s = sr + (size_t)r * sstep;
#pragma unroll
    for (int comp = 0; comp < 2; ++comp) {
      const double cv = s[(size_t)comp * C];
      const bool in = have[comp] && __builtin_isfinite(cv);
#pragma unroll
      for (int dir = 0; dir < 2; ++dir) {
        const int k = 2 * comp + dir;
        int clamped = 0;
        const double wv = phf_sens_weight(a.am1[dir], in ? cv : cref[comp], cref[comp], &clamped);
        const double w = in ? wv : 0.0;
        s[(size_t)(2 + k) * C] = w;
        phf_sens_weight_step(w, clamped, &acc[k][0], &acc[k][1], &acc[k][2], &acc[k][3]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kWeights; ++k)
#pragma unroll
    for (int f = 0; f < kWFields; ++f) st[((size_t)k * kWFields + f) * C] = acc[k][f];
}

// ---- prepare: anchor, min/max, level, merge of the five arrays (phf_grid.h) -----------------------------------------------------------
__device__ inline double col_value(const SArgs& a, int q, int j, unsigned i) {
  const unsigned r = i / (unsigned)a.C, c = i - r * (unsigned)a.C;
  return a.rows[(((size_t)r * a.Q + q) * a.stride + j) * (size_t)a.C + c];
}

__global__ __launch_bounds__(kPrepThreads) void sens_prepare_kernel(const SArgs a) {
  extern __shared__ unsigned long long s_merge[];              // [B/2]
  const int q = blockIdx.x / a.ncol, j = blockIdx.x % a.ncol;
  const size_t s = blockIdx.x;
  phf_grid_prepare<kArrays>(a.hdr + s * kHdr, a.counts + s * kArrays * a.B, a.B, a.n, s_merge,
                            [&](unsigned i) { return col_value(a, q, j, i); });
}

// ---- columns: a chain's sums of one column under the base and the four weights -------------------------------------------------------
__global__ __launch_bounds__(kThreads) void sens_columns_kernel(const SArgs a) {
  const int unit = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves + threadIdx.x / 64));
  if (unit >= a.units) return;
  const int cg = unit % a.ncg, slot = unit / a.ncg;             // slot = q * ncol + j
  const int q = slot / a.ncol, j = slot % a.ncol;
  const int c = cg * 64 + (threadIdx.x & 63);
  if (c >= a.C) return;
  const double* h = a.hdr + (size_t)slot * kHdr;
  if (h[PHF_GRID_ANCHORED] == 0.0) return;                      // no finite value of this column yet: nothing enters
  const double anchor = h[PHF_GRID_ANCHOR], inv_w0 = 1.0 / h[PHF_GRID_W0];
  const size_t C = (size_t)a.C;
  double* st = a.csum + (size_t)slot * kArrays * kCFields * C + c;
  double acc[kArrays][kCFields];
#pragma unroll
  for (int k = 0; k < kArrays; ++k)
#pragma unroll
    for (int f = 0; f < kCFields; ++f) acc[k][f] = st[((size_t)k * kCFields + f) * C];
  const size_t rstep = (size_t)a.Q * a.stride * C, sstep = (size_t)a.Q * kDraw * C;
  const double* xr = a.rows + ((size_t)q * a.stride + j) * C + c;
  const double* sr = a.scratch + ((size_t)q * kDraw + 2) * C + c;
  for (int64_t r = 0; r < a.nr; ++r) {
    const double x = xr[(size_t)r * rstep];
    const int valid = phf_sens_binned(x, anchor, inv_w0);
    const double d = x - anchor;
    phf_sens_column_step(1.0, d, valid, &acc[0][0], &acc[0][1], &acc[0][2]);
    const double* w = sr + (size_t)r * sstep;
#pragma unroll
    for (int k = 0; k < kWeights; ++k) phf_sens_column_step(w[(size_t)k * C], d, valid, &acc[1 + k][0], &acc[1 + k][1], &acc[1 + k][2]);
  }
#pragma unroll
  for (int k = 0; k < kArrays; ++k)
#pragma unroll
    for (int f = 0; f < kCFields; ++f) st[((size_t)k * kCFields + f) * C] = acc[k][f];
}

// ---- bin: uint32 counts and uint64 masses in LDS, flushed with integer atomics -------------------------------------------------------
__global__ __launch_bounds__(kBinThreads) void sens_bin_kernel(const SArgs a) {
  extern __shared__ unsigned long long s_mass[];                // [kWeights][B], then unsigned [B]
  unsigned* s_hist = reinterpret_cast<unsigned*>(s_mass + (size_t)kWeights * a.B);
  const int split = blockIdx.x % a.splits;
  const int slot = blockIdx.x / a.splits;
  const int q = slot / a.ncol, j = slot % a.ncol;
  const phf_grid_view grid = phf_grid_load(a.hdr + (size_t)slot * kHdr);
  const int tid = threadIdx.x;
  for (int b = tid; b < a.B; b += kBinThreads) s_hist[b] = 0u;
  for (int b = tid; b < kWeights * a.B; b += kBinThreads) s_mass[b] = 0ull;
  __syncthreads();
  const unsigned i0 = (unsigned)split * a.per_split;
  const unsigned i1 = i0 >= a.n ? i0 : (a.n - i0 < a.per_split ? a.n : i0 + a.per_split);   // [i0, i1) within [0, n)
  unsigned nf = 0;
  for (unsigned i = i0 + tid; i < i1; i += kBinThreads) {
    const double x = col_value(a, q, j, i);
    const int b = phf_grid_index(grid, x, a.B);
    nf += b < 0;
    if (b >= 0) {
      atomicAdd(&s_hist[b], 1u);
#pragma unroll
      for (int k = 0; k < kWeights; ++k) {
        const double w = *draw_at(a, q, i, 2 + k);
        if (w > 0.0) atomicAdd(&s_mass[(size_t)k * a.B + b], (unsigned long long)phf_sens_mass(w));
      }
    }
  }
  __syncthreads();
  unsigned long long* cnt = a.counts + (size_t)slot * kArrays * a.B;
  for (int b = tid; b < a.B; b += kBinThreads) {
    const unsigned v = s_hist[b];
    if (v) {
      atomicAdd(&cnt[b], (unsigned long long)v);
#pragma unroll
      for (int k = 0; k < kWeights; ++k) {
        const unsigned long long m = s_mass[(size_t)k * a.B + b];
        if (m) atomicAdd(&cnt[(size_t)(1 + k) * a.B + b], m);
      }
    }
  }
  if (nf) atomicAdd(&a.nonfinite[slot], (unsigned long long)nf);
}

// ---- reduce --------------------------------------------------------------------------------------------------------------------------
struct RArgs {
  int Q, ncol, C, B;
  const unsigned long long* counts;
  const double* hdr;
  const unsigned long long* nonfinite;
  const double* wsum;
  const double* csum;
  double* out_slots;              // [S][kSlotOut]
  double* out_weights;            // [Q][kWeights][kWFields]
  double* out_columns;            // [S][kArrays][kColOut]
};

// one thread per (slot, weight): the bins in order; weight 0's thread also writes the slot's head
__global__ __launch_bounds__(kThreads) void sens_reduce_cjs_kernel(const RArgs a) {
  PHF_MATH_TABLES_TO_LDS();
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t S = (int64_t)a.Q * a.ncol;
  if (i >= S * kWeights) return;
  const int64_t s = i / kWeights;
  const int k = (int)(i % kWeights);
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  const unsigned long long* base = a.counts + (size_t)s * kArrays * a.B;
  double* o = a.out_slots + (size_t)s * kSlotOut;
  double r[kSlotPerWeight];
  phf_sens_cjs_sums(a.B, reinterpret_cast<const uint64_t*>(base), reinterpret_cast<const uint64_t*>(base + (size_t)(1 + k) * a.B), k_log, r);
#pragma unroll
  for (int f = 0; f < kSlotPerWeight; ++f) o[kSlotHead + k * kSlotPerWeight + f] = r[f];
  if (k == 0) {
    unsigned long long n = 0;
    for (int b = 0; b < a.B; ++b) n += base[b];
    phf_grid_write_head(a.hdr + (size_t)s * kHdr, n, a.nonfinite[s], o);
  }
}

// the chains merged in chain order: one thread per scalar of the weights' sums, one per (slot, array) of the columns' sums
__global__ __launch_bounds__(kThreads) void sens_reduce_sums_kernel(const RArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t nw = (int64_t)a.Q * kWeights * kWFields, S = (int64_t)a.Q * a.ncol;
  const size_t C = (size_t)a.C;
  if (i < nw) {
    const double* st = a.wsum + (size_t)i * C;
    double t = 0.0;
    for (int c = 0; c < a.C; ++c) t += st[c];
    a.out_weights[i] = t;
    return;
  }
  const int64_t u = i - nw;
  if (u >= S * kArrays) return;
  const int k = (int)(u % kArrays);
  const int64_t s = u / kArrays;
  const double* st = a.csum + (size_t)u * kCFields * C;
  const double* b0 = a.csum + (size_t)s * kArrays * kCFields * C;                // the base sums of the same column
  double t[kCFields] = {0.0, 0.0, 0.0};
  for (int c = 0; c < a.C; ++c)
#pragma unroll
    for (int f = 0; f < kCFields; ++f) t[f] += st[(size_t)f * C + c];
  // between-chain standard error of the mean shift: the chains' own shifts (weighted mean - base mean), divisor C' - 1, over sqrt C'
  double n = 0.0, mean = 0.0, m2 = 0.0;
  if (k > 0) {
    for (int c = 0; c < a.C; ++c) {
      const double w = st[c], nb = b0[c];
      if (!(w > 0.0) || !(nb > 0.0)) continue;
      const double shift = st[C + c] / w - b0[C + c] / nb;
      n += 1.0;
      const double dl = shift - mean;
      mean += dl / n;
      m2 += dl * (shift - mean);
    }
  }
  double* o = a.out_columns + (size_t)u * kColOut;
  o[0] = t[0]; o[1] = t[1]; o[2] = t[2];
  o[3] = (k > 0 && n > 1.0) ? sqrt(m2 / (n - 1.0) / n) : PHF_NAN;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
int fail(const char* who, const char* what) { return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: %s", who, what); }

int check_geometry(const char* who, int num_problems, int num_columns, int num_chains, int64_t total_rows, int bins) {
  const int rc = phf_check_positive(who, "num_problems, num_columns and num_chains", {num_problems, num_columns, num_chains});
  if (rc != PHF_OK) return rc;
  if (total_rows < 1) return fail(who, "total_rows must be positive");
  if (phf_grid_check_bins(who, bins, kMaxBins) != PHF_OK) return PHF_ERR_INVALID_ARGUMENT;
  if ((double)total_rows * num_chains > 4294967296.0) return fail(who, "total_rows x num_chains must not exceed 2^32 draws (the masses' uint64 sums)");
  if ((double)num_problems * num_columns * ((num_chains + 63) / 64) > 2147483647.0 / 8 || (double)num_problems * kDraw * num_chains * 8 > 1e12)
    return fail(who, "launch grid too large (fewer problems per workspace)");
  return PHF_OK;
}

bool delta_ok(double delta) { return delta > 0.0 && delta <= 0.25; }

int check_sl_points(const char* who, const phf_points* p, int num_problems) {
  if (!p || !p->ln_conc || !p->response || !p->weight || !p->counts || !p->pi_bit || !p->extra) return fail(who, "null single-level points");
  if (p->stride < 1 || p->num_pairs < 1 || (num_problems > 0 && p->num_pairs != num_problems))
    return fail(who, "the single-level points must have stride >= 1 and one pair per problem");
  return PHF_OK;
}

int check_hier_points(const char* who, const phf_hier_points* p, const phf_hier_prior* prior, int num_problems) {
  if (!p || !p->ln_conc || !p->response || !p->expt_start || !prior) return fail(who, "null hierarchical points or prior");
  if (p->n_expts < 1 || p->n_expts > PHF_HIER_MAX_EXPTS) return fail(who, "the hierarchical model takes 1..64 experiments");
  if (p->stride < 1 || p->num_pairs < 1 || (num_problems > 0 && p->num_pairs != num_problems))
    return fail(who, "the hierarchical points must have stride >= 1 and one pair per problem");
  return PHF_OK;
}

template <int KIND>
void launch_components(const SArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(sens_components_kernel<KIND>, dim3(blocks_for(a.units, kWaves)), dim3(kThreads), 0, st, a);
}

}  // namespace

extern "C" size_t phf_sensitivity_workspace_bytes(int num_problems, int num_columns, int num_chains, int64_t total_rows, int bins) {
  if (check_geometry("phf_sensitivity_workspace_bytes", num_problems, num_columns, num_chains, total_rows, bins) != PHF_OK) return 0;
  return layout_of(num_problems, num_columns, num_chains, total_rows, bins).total;
}

extern "C" int phf_sensitivity_init(int num_problems, int num_columns, int num_chains, int64_t total_rows, int bins, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  static const char* who = "phf_sensitivity_init";
  int rc = check_geometry(who, num_problems, num_columns, num_chains, total_rows, bins);
  if (rc != PHF_OK) return rc;
  const Layout l = layout_of(num_problems, num_columns, num_chains, total_rows, bins);
  return phf_init_workspace(who, "sensitivity", workspace, workspace_bytes, l.total, l.persistent, stream);
}

extern "C" int phf_sensitivity_accumulate(int kind, const phf_points* sl_points, const phf_hier_points* hier_points,
                                          const phf_hier_prior* prior, int prior_column, int likelihood_column, const double* rows,
                                          int64_t num_rows, int num_problems, int row_stride_cols, int num_chains, int num_columns,
                                          double delta, int bins, int64_t first_row, int64_t total_rows, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  static const char* who = "phf_sensitivity_accumulate";
  int rc = check_geometry(who, num_problems, num_columns, num_chains, total_rows, bins);
  if (rc != PHF_OK) return rc;
  if (kind < kSingle1 || kind > kGiven) return fail(who, "kind must be 1, 2 (single-level model), 3 (hierarchical) or 4 (given columns)");
  if (!delta_ok(delta)) return fail(who, "delta must satisfy 0 < delta <= 0.25");
  if ((rc = phf_check_row_stride(who, row_stride_cols, num_columns, "must be at least num_columns")) != PHF_OK) return rc;
  int needed = 0;
  if (kind == kSingle1 || kind == kSingle2) {
    if ((rc = check_sl_points(who, sl_points, num_problems)) != PHF_OK) return rc;
    needed = kind + 1;
  } else if (kind == kHier) {
    if ((rc = check_hier_points(who, hier_points, prior, num_problems)) != PHF_OK) return rc;
    needed = 5 + 2 * hier_points->n_expts;
  } else {
    if (prior_column < 0 || prior_column >= row_stride_cols || likelihood_column < 0 || likelihood_column >= row_stride_cols)
      return fail(who, "the given component columns must lie in [0, row_stride_cols)");
  }
  if ((rc = phf_check_row_stride(who, row_stride_cols, needed, "is smaller than the columns the model reads")) != PHF_OK) return rc;
  if ((rc = phf_check_row_window(who, num_rows, first_row, total_rows)) != PHF_OK) return rc;
  if (num_rows > 0 && !rows) return fail(who, "null rows");
  const Layout l = layout_of(num_problems, num_columns, num_chains, total_rows, bins);
  if ((rc = phf_check_workspace(who, "sensitivity", workspace, workspace_bytes, l.total)) != PHF_OK) return rc;
  if (num_rows == 0) return PHF_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(workspace);
  SArgs a = {};
  if (kind == kSingle1 || kind == kSingle2) a.sl = *sl_points;
  if (kind == kHier) { a.hp = *hier_points; a.prior = *prior; }
  a.Q = num_problems; a.stride = row_stride_cols; a.C = num_chains; a.ncol = num_columns; a.B = bins;
  a.ncg = (num_chains + 63) / 64;
  a.prior_col = prior_column; a.lik_col = likelihood_column;
  a.am1[PHF_SENS_DOWN] = phf_sens_alpha_m1(delta, PHF_SENS_DOWN);
  a.am1[PHF_SENS_UP] = phf_sens_alpha_m1(delta, PHF_SENS_UP);
  a.counts = reinterpret_cast<unsigned long long*>(base + l.counts);
  a.hdr = reinterpret_cast<double*>(base + l.hdr);
  a.nonfinite = reinterpret_cast<unsigned long long*>(base + l.nonfinite);
  a.cref = reinterpret_cast<double*>(base + l.cref);
  a.wsum = reinterpret_cast<double*>(base + l.wsum);
  a.csum = reinterpret_cast<double*>(base + l.csum);
  a.scratch = reinterpret_cast<double*>(base + l.scratch);
  const size_t merge_lds = (size_t)bins / 2 * 8, bin_lds = (size_t)bins * (kWeights * 8 + 4);
  if ((rc = allow_lds(sens_bin_kernel, bin_lds, "hipFuncSetAttribute(sens_bin_kernel)")) != PHF_OK) return rc;
  const size_t row_doubles = (size_t)num_problems * row_stride_cols * (size_t)num_chains;
  const int slots = num_problems * num_columns;
  for (int64_t r0 = 0; r0 < num_rows; r0 += l.block_rows) {     // blocks of the scratch region's rows
    a.rows = rows + (size_t)r0 * row_doubles;
    a.nr = num_rows - r0 < l.block_rows ? num_rows - r0 : l.block_rows;
    a.n = (unsigned)(a.nr * num_chains);
    a.units = num_problems * a.ncg;
    if (kind == kSingle1) launch_components<kSingle1>(a, st);
    else if (kind == kSingle2) launch_components<kSingle2>(a, st);
    else if (kind == kHier) launch_components<kHier>(a, st);
    else launch_components<kGiven>(a, st);
    if ((rc = phf_check_launch("sens_components_kernel")) != PHF_OK) return rc;
    hipLaunchKernelGGL(sens_reference_kernel, dim3(2 * num_problems), dim3(kPrepThreads), 0, st, a);
    if ((rc = phf_check_launch("sens_reference_kernel")) != PHF_OK) return rc;
    hipLaunchKernelGGL(sens_weights_kernel, dim3(blocks_for(a.units, kWaves)), dim3(kThreads), 0, st, a);
    if ((rc = phf_check_launch("sens_weights_kernel")) != PHF_OK) return rc;
    hipLaunchKernelGGL(sens_prepare_kernel, dim3(slots), dim3(kPrepThreads), merge_lds, st, a);
    if ((rc = phf_check_launch("sens_prepare_kernel")) != PHF_OK) return rc;
    SArgs c = a;
    c.units = slots * a.ncg;
    hipLaunchKernelGGL(sens_columns_kernel, dim3(blocks_for(c.units, kWaves)), dim3(kThreads), 0, st, c);
    if ((rc = phf_check_launch("sens_columns_kernel")) != PHF_OK) return rc;
    const phf_grid_split split = phf_grid_split_of(a.n, slots);
    a.splits = split.splits; a.per_split = split.per_split;
    hipLaunchKernelGGL(sens_bin_kernel, dim3((unsigned)slots * a.splits), dim3(kBinThreads), bin_lds, st, a);
    if ((rc = phf_check_launch("sens_bin_kernel")) != PHF_OK) return rc;
  }
  return PHF_OK;
}

extern "C" int phf_sensitivity_reduce(int num_problems, int num_columns, int num_chains, int64_t total_rows, int bins, const void* workspace,
                                      size_t workspace_bytes, double* out_slots, double* out_weights, double* out_columns,
                                      double* out_per_chain, void* stream) {
  static const char* who = "phf_sensitivity_reduce";
  int rc = check_geometry(who, num_problems, num_columns, num_chains, total_rows, bins);
  if (rc != PHF_OK) return rc;
  const Layout l = layout_of(num_problems, num_columns, num_chains, total_rows, bins);
  if ((rc = phf_check_workspace(who, "sensitivity", workspace, workspace_bytes, l.total)) != PHF_OK) return rc;
  if (!out_slots || !out_weights || !out_columns) return fail(who, "null out");
  const char* base = static_cast<const char*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  RArgs a = {};
  a.Q = num_problems; a.ncol = num_columns; a.C = num_chains; a.B = bins;
  a.counts = reinterpret_cast<const unsigned long long*>(base + l.counts);
  a.hdr = reinterpret_cast<const double*>(base + l.hdr);
  a.nonfinite = reinterpret_cast<const unsigned long long*>(base + l.nonfinite);
  a.wsum = reinterpret_cast<const double*>(base + l.wsum);
  a.csum = reinterpret_cast<const double*>(base + l.csum);
  a.out_slots = out_slots; a.out_weights = out_weights; a.out_columns = out_columns;
  hipLaunchKernelGGL(sens_reduce_cjs_kernel, dim3(blocks_for((int64_t)l.slots * kWeights, kThreads)), dim3(kThreads), 0, st, a);
  if ((rc = phf_check_launch("sens_reduce_cjs_kernel")) != PHF_OK) return rc;
  const int64_t scalars = (int64_t)num_problems * kWeights * kWFields + (int64_t)l.slots * kArrays;
  hipLaunchKernelGGL(sens_reduce_sums_kernel, dim3(blocks_for(scalars, kThreads)), dim3(kThreads), 0, st, a);
  if ((rc = phf_check_launch("sens_reduce_sums_kernel")) != PHF_OK) return rc;
  if (out_per_chain) {                                          // the per-chain sums as they stand (tests): the weights', then the columns'
    if (hipMemcpyAsync(out_per_chain, base + l.wsum, l.persistent - l.wsum, hipMemcpyDeviceToDevice, st) != hipSuccess)
      return phf_check_launch(who);
  }
  return PHF_OK;
}

extern "C" int phf_sensitivity_components(int kind, const phf_points* sl_points, const phf_hier_points* hier_points,
                                          const phf_hier_prior* prior, int64_t m, const int32_t* problem_index, const double* theta,
                                          double* out, void* stream) {
  static const char* who = "phf_sensitivity_components";
  int rc;
  if (kind != kSingle1 && kind != kSingle2 && kind != kHier) return fail(who, "kind must be 1, 2 (single-level model) or 3 (hierarchical)");
  int dim, num_problems;
  if (kind == kHier) {
    if ((rc = check_hier_points(who, hier_points, prior, 0)) != PHF_OK) return rc;
    dim = 5 + 2 * hier_points->n_expts; num_problems = hier_points->num_pairs;
  } else {
    if ((rc = check_sl_points(who, sl_points, 0)) != PHF_OK) return rc;
    dim = kind + 1; num_problems = sl_points->num_pairs;
  }
  if (m < 0 || (m > 0 && (!problem_index || !theta || !out))) return fail(who, "m must be >= 0 and the arrays non-null");
  if ((double)m * dim > 2147483647.0) return fail(who, "m x dim must stay below 2^31 (evaluate in batches)");
  if (m == 0) return PHF_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(blocks_for(m, kThreads)), block(kThreads);
  const phf_points sl = kind == kHier ? phf_points{} : *sl_points;
  const phf_hier_points hp = kind == kHier ? *hier_points : phf_hier_points{};
  const phf_hier_prior pr = kind == kHier ? *prior : phf_hier_prior{};
  if (kind == kSingle1) hipLaunchKernelGGL(sens_batch_kernel<kSingle1>, grid, block, 0, st, sl, hp, pr, num_problems, m, problem_index, theta, out);
  else if (kind == kSingle2) hipLaunchKernelGGL(sens_batch_kernel<kSingle2>, grid, block, 0, st, sl, hp, pr, num_problems, m, problem_index, theta, out);
  else hipLaunchKernelGGL(sens_batch_kernel<kHier>, grid, block, 0, st, sl, hp, pr, num_problems, m, problem_index, theta, out);
  return phf_check_launch(who);
}

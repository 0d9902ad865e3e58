/* phf_grid.h — the adaptive exact-count histogram grid of the streaming analyses, once ("Posterior quantiles"):
 * phf_quantiles.hip bins on it and phf_sensitivity.hip bins on the same grid, so sensitivity's base counts are the quantiles' counts.
 *
 * Per slot an 8-double header holds the grid: an anchor a (the first finite value, in (row, chain) order, of all values accumulated),
 * a power-of-two base width w0 = 2^(floor(log2 max(|a|, 2^-30)) - 40), the running [min, max] and a level k:
 *     t = (x - a) * (1/w0)          (1/w0 is a power of two: the same double as (x - a)/w0)
 *     j = floor(t * 2^-k) + B/2     (t * 2^-k by ldexp: exact)
 * The operation order is the contract: the subtraction, the multiplication by the exact reciprocal, ldexp, floor.  Every translation
 * unit is compiled with -ffp-contract=off and nothing here is an fma, so every build gives the same bins.
 *
 * Part A, the scalar rule, compiles as C11 with gcc (the tests' ground truth) and into the kernels.  Parts B (the device code: the
 * prepare pass, the bin index of a value, the bin pass, the output head) and C (the host's sizing and refusal) are for hipcc only. */
#ifndef PHF_GRID_H
#define PHF_GRID_H

#include "phf_math.h"

/* ---- A: the scalar rule ------------------------------------------------------------------------------------------------------------ */
#define PHF_GRID_HDR 8           /* doubles of a slot's header: the six below, then two unused */
#define PHF_GRID_ANCHOR 0
#define PHF_GRID_W0 1
#define PHF_GRID_MIN 2
#define PHF_GRID_MAX 3
#define PHF_GRID_LEVEL 4
#define PHF_GRID_ANCHORED 5      /* 0 until the slot has seen a finite value */
#define PHF_GRID_MAX_LEVEL 1100  /* no pair of finite t needs more */

/* w0 of a (finite) anchor: the frexp exponent - 1 is floor(log2 m) */
PHF_HD double phf_grid_w0(double anchor) {
  const double m = __builtin_fmax(__builtin_fabs(anchor), 0x1p-30);
#if defined(__HIP_DEVICE_COMPILE__)
  const int e = __builtin_amdgcn_frexp_exp(m);
#else
  int e;
  (void)__builtin_frexp(m, &e);
#endif
  return __builtin_ldexp(1.0, e - 41);
}

/* the grid coordinate; inv_w0 = 1 / w0, a power of two: exact */
PHF_HD double phf_grid_t(double x, double anchor, double inv_w0) { return (x - anchor) * inv_w0; }

/* a value is binned when its grid coordinate is finite (|x - a| up to ~2^980 w0); the others are counted apart */
PHF_HD int phf_grid_binned(double x, double anchor, double inv_w0) { return __builtin_isfinite(phf_grid_t(x, anchor, inv_w0)); }

/* do the B bins of level k hold [tmin, tmax]? */
PHF_HD int phf_grid_holds(double tmin, double tmax, int k, int B) {
  return __builtin_floor(__builtin_ldexp(tmin, -k)) >= -(double)(B / 2) && __builtin_floor(__builtin_ldexp(tmax, -k)) < (double)(B / 2);
}

/* the bin of a finite t at level k; the level holds [min, max]: the clamp is a guard */
PHF_HD int phf_grid_bin(double t, int k, int B) {
  const double f = __builtin_floor(__builtin_ldexp(t, -k)) + (double)(B / 2);
  return (int)__builtin_fmin(__builtin_fmax(f, 0.0), (double)(B - 1));
}

#if defined(__HIPCC__)
/* ---- B: device code ---------------------------------------------------------------------------------------------------------------- */
#include "phf_device_util.h"

constexpr int kGridPrepThreads = 256;    // threads of a prepare workgroup (one per slot)
constexpr int kGridOutHead = 8;          // min, max, binned draws, non-finite, bin width, level, anchor, w0

// prepare, one workgroup per slot: the anchor (the first call with a finite value), a min/max pass over the call's n values, then the
// least level k' >= k whose bins hold the running [min, max]; when k' > k the slot's ARRAYS count arrays ([ARRAYS][B] at counts) merge
// 2^(k'-k)-fold in place (floor(floor(y)/2^m) = floor(y/2^m): the final counts are those of binning every value at the final level,
// the least one holding the global [min, max] — the same however the rows are cut into calls).  value(i) is the call's value i, a pure
// function of i; s_merge is the workgroup's dynamic LDS, [B/2].
template <int ARRAYS, typename Value>
__device__ __forceinline__ void phf_grid_prepare(double* h, unsigned long long* counts, int B, unsigned n, unsigned long long* s_merge,
                                                 Value value) {
  __shared__ double s_red[16];
  __shared__ unsigned s_redu[16];
  __shared__ int s_level[2];
  const int tid = threadIdx.x;
  if (h[PHF_GRID_ANCHORED] == 0.0) {                           // not anchored yet: the first finite value in (row, chain) order
    unsigned best = 0xffffffffu;
    for (unsigned i = tid; i < n; i += kGridPrepThreads)
      if (__builtin_isfinite(value(i))) { best = i; break; }
    best = block_min_u(best, s_redu);
    if (best == 0xffffffffu) return;                           // nothing finite yet: the bin pass counts every value apart
    if (tid == 0) {
      const double x = value(best);
      h[PHF_GRID_ANCHOR] = x;
      h[PHF_GRID_W0] = phf_grid_w0(x);
      h[PHF_GRID_MIN] = x; h[PHF_GRID_MAX] = x; h[PHF_GRID_LEVEL] = 0.0; h[PHF_GRID_ANCHORED] = 1.0;
    }
    __syncthreads();
  }
  const double anchor = h[PHF_GRID_ANCHOR], inv_w0 = 1.0 / h[PHF_GRID_W0];
  double lo = PHF_INF, hi = -PHF_INF;
  for (unsigned i = tid; i < n; i += kGridPrepThreads) {
    const double x = value(i);
    if (phf_grid_binned(x, anchor, inv_w0)) { lo = __builtin_fmin(lo, x); hi = __builtin_fmax(hi, x); }
  }
  lo = block_min(lo, s_red);
  hi = block_max(hi, s_red);
  if (tid == 0) {
    const double mn = __builtin_fmin(h[PHF_GRID_MIN], lo), mx = __builtin_fmax(h[PHF_GRID_MAX], hi);
    const int k0 = (int)h[PHF_GRID_LEVEL];
    int k1 = k0;
    const double tmin = phf_grid_t(mn, anchor, inv_w0), tmax = phf_grid_t(mx, anchor, inv_w0);
    while (!phf_grid_holds(tmin, tmax, k1, B) && k1 < PHF_GRID_MAX_LEVEL) ++k1;
    h[PHF_GRID_MIN] = mn; h[PHF_GRID_MAX] = mx; h[PHF_GRID_LEVEL] = (double)k1;
    s_level[0] = k0; s_level[1] = k1;
  }
  __syncthreads();
  const int k0 = s_level[0], k1 = s_level[1];
  if (k1 == k0) return;
  // merge: new bin of old j = ((j - B/2) >> D) + B/2 (an arithmetic shift is floor division); D >= log2 B acts as log2 B
  int log2B = 0;
  while ((1 << log2B) < B) ++log2B;
  const int D = k1 - k0 < log2B ? k1 - k0 : log2B;
  const int half = B / 2;
  const int nlo = half + ((-half) >> D), nn = half + ((half - 1) >> D) - nlo + 1;   // nn <= B/2
  for (int arr = 0; arr < ARRAYS; ++arr) {
    for (int i = tid; i < nn; i += kGridPrepThreads) s_merge[i] = 0ull;
    __syncthreads();
    unsigned long long* cnt = counts + (size_t)arr * B;
    for (int j = tid; j < B; j += kGridPrepThreads) {
      const unsigned long long c = cnt[j];
      if (c) atomicAdd(&s_merge[((j - half) >> D) + half - nlo], c);
    }
    __syncthreads();
    for (int j = tid; j < B; j += kGridPrepThreads) cnt[j] = (j >= nlo && j < nlo + nn) ? s_merge[j - nlo] : 0ull;
    if (arr + 1 < ARRAYS) __syncthreads();
  }
}

// a slot's grid as a bin kernel reads it, and the bin of a value on it: -1 for a value counted apart (not finite, t not finite, or
// the slot not anchored yet)
struct phf_grid_view {
  bool anchored;
  double anchor, inv_w0;
  int level;
};

__device__ inline phf_grid_view phf_grid_load(const double* h) {
  phf_grid_view g;
  g.anchored = h[PHF_GRID_ANCHORED] != 0.0;
  g.anchor = h[PHF_GRID_ANCHOR];
  g.inv_w0 = 1.0 / h[PHF_GRID_W0];
  g.level = (int)h[PHF_GRID_LEVEL];
  return g;
}

__device__ inline int phf_grid_index(const phf_grid_view& g, double x, int B) {
  int j = -1;
  if (g.anchored) {
    const double t = phf_grid_t(x, g.anchor, g.inv_w0);
    if (__builtin_isfinite(t)) j = phf_grid_bin(t, g.level, B);
  }
  return j;
}

// the bin pass of one workgroup of THREADS threads over the call's values [i0, i1) of a slot: a workgroup-private uint32 histogram in
// LDS (s_hist, the workgroup's dynamic LDS, [B]; a wavefront whose lanes all fall in one bin adds once), flushed to the slot's uint64
// counts with integer atomics for its non-zero bins only; the values counted apart go to *nonfinite.  value(i) as in phf_grid_prepare.
template <int THREADS, typename Value>
__device__ __forceinline__ void phf_grid_bin_values(const double* h, unsigned long long* cnt, unsigned long long* nonfinite, int B,
                                                    unsigned i0, unsigned i1, unsigned* s_hist, Value value) {
  const phf_grid_view grid = phf_grid_load(h);
  const int tid = threadIdx.x;
  for (int j = tid; j < B; j += THREADS) s_hist[j] = 0u;
  __syncthreads();
  unsigned nf = 0;
  const int lane = __lane_id();
  for (unsigned i = i0 + tid; i < i1; i += THREADS) {
    const double x = value(i);
    const int j = phf_grid_index(grid, x, B);
    nf += j < 0;
    const unsigned long long active = __ballot(1);
    const int j0 = __builtin_amdgcn_readfirstlane(j);
    if (__ballot(j != j0) == 0) {                                // the whole wavefront in one bin (a stuck or constant column)
      if (j0 >= 0 && lane == __ffsll((long long)active) - 1) atomicAdd(&s_hist[j0], (unsigned)__popcll(active));
    } else if (j >= 0) {
      atomicAdd(&s_hist[j], 1u);
    }
  }
  __syncthreads();
  for (int j = tid; j < B; j += THREADS) {
    const unsigned c = s_hist[j];
    if (c) atomicAdd(&cnt[j], (unsigned long long)c);
  }
  if (nf) atomicAdd(nonfinite, (unsigned long long)nf);
}

// the values [i0, i1) of split `split` of a bin launch (phf_grid_split_of, below) over n values
__device__ inline void phf_grid_split_range(unsigned n, int split, unsigned per_split, unsigned* i0, unsigned* i1) {
  *i0 = (unsigned)split * per_split;
  *i1 = *i0 >= n ? *i0 : (n - *i0 < per_split ? n : *i0 + per_split);   // [i0, i1) within [0, n)
}

// the kGridOutHead doubles a reduce writes per slot
__device__ inline void phf_grid_write_head(const double* h, unsigned long long binned, unsigned long long nonfinite, double* o) {
  const bool anchored = h[PHF_GRID_ANCHORED] != 0.0;
  o[0] = anchored ? h[PHF_GRID_MIN] : PHF_NAN;
  o[1] = anchored ? h[PHF_GRID_MAX] : PHF_NAN;
  o[2] = (double)binned;
  o[3] = (double)nonfinite;
  o[4] = anchored ? __builtin_ldexp(h[PHF_GRID_W0], (int)h[PHF_GRID_LEVEL]) : PHF_NAN;
  o[5] = h[PHF_GRID_LEVEL];
  o[6] = anchored ? h[PHF_GRID_ANCHOR] : PHF_NAN;
  o[7] = anchored ? h[PHF_GRID_W0] : PHF_NAN;
}

/* ---- C: host code ------------------------------------------------------------------------------------------------------------------ */
constexpr int kGridMinBins = 64;
constexpr int64_t kGridValuesPerBlock = 131072;   // values one bin workgroup takes before a call's slot is split over more
constexpr int kGridTargetBlocks = 4096;           // ... up to about this many bin workgroups per launch

// a bin launch over `slots` slots of n values each: workgroups per slot, values per workgroup
struct phf_grid_split {
  int splits;
  unsigned per_split;
};

inline phf_grid_split phf_grid_split_of(unsigned n, int slots) {
  const int64_t want = (n + kGridValuesPerBlock - 1) / kGridValuesPerBlock;
  const int64_t room = kGridTargetBlocks / slots > 1 ? kGridTargetBlocks / slots : 1;
  phf_grid_split s;
  s.splits = (int)(want < room ? (want > 0 ? want : 1) : room);
  s.per_split = (unsigned)((n + s.splits - 1) / s.splits);
  return s;
}

// bins: a power of two in [kGridMinBins, max_bins] (the caller's bin kernel sets max_bins by its LDS per bin)
inline int phf_grid_check_bins(const char* who, int bins, int max_bins) {
  if (bins >= kGridMinBins && bins <= max_bins && (bins & (bins - 1)) == 0) return PHF_OK;
  return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: bins must be a power of two in [%d, %d] (got %d)", who, kGridMinBins, max_bins, bins);
}
#endif /* __HIPCC__ */

#endif /* PHF_GRID_H */

// phf_point_block.h — the point-block mapping of the kernels that stream the samplers' rows past per-point accumulators (WAIC's
// accumulate in phf_pointwise.hip, PSIS-LOO's in phf_psis.hip, the predictive PIT in phf_ppc.hip); device only.
//
// One lane = one chain (the rows are [rows][Q][stride][C], chain fastest: a wavefront reads 512 contiguous bytes of one (problem,
// column)); one wavefront = 64 chains of one problem and a block of kPtBlock of its points, so the points are wave-uniform (scalar
// loads) and the block's accumulators live in registers.  The kernels' argument structs share the fields read here: pts, rows, Q,
// stride_cols, C, ne, ncg (64-chain groups), npb (point blocks), units.
#ifndef PHF_POINT_BLOCK_H
#define PHF_POINT_BLOCK_H

#include <hip/hip_runtime.h>

#include "phf_device_util.h"
#include "phf_pointwise.h"

constexpr int kPtBlock = 4;             // points per wavefront
constexpr int kPtWaves = 4;             // wavefronts per workgroup of these kernels (256 threads)
constexpr int kHierarchical = 3;        // `likelihood` of the hierarchical layout (1 | 2: single-level model 1 | 2)
constexpr int kGiven = 4;               // the *_accumulate_given entries: l of point p is column p of the row

struct phf_point_block {
  int q, c, p0, np;                     // problem, chain, first point, live points (1..kPtBlock)
  double lc[kPtBlock], yv[kPtBlock];    // ln concentration and response of the points
  int tg[kPtBlock];                     // tag: censoring (single-level) or experiment (hierarchical), clamped
  const double* xr;                     // the lane's value of column 0 in the call's first row; the next row is rstep further
  size_t rstep;
};

// this lane's block of the launch: false where the unit, the block or the chain lies beyond the data (nothing to do)
template <int LIK, typename Args>
__device__ __forceinline__ bool phf_point_block_open(const Args& a, phf_point_block& b) {
  const int unit = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kPtWaves + threadIdx.x / 64));   // wave-uniform
  if (unit >= a.units) return false;
  const int pb = unit % a.npb;
  const int cg = (unit / a.npb) % a.ncg;
  b.q = unit / a.npb / a.ncg;
  const int ps = a.pts.stride;
  const int n = clamp_count(a.pts.count[b.q], ps);
  b.p0 = pb * kPtBlock;
  if (b.p0 >= n) return false;
  b.np = n - b.p0 < kPtBlock ? n - b.p0 : kPtBlock;
  b.c = cg * 64 + (threadIdx.x & 63);
  if (b.c >= a.C) return false;
#pragma unroll
  for (int k = 0; k < kPtBlock; ++k) {
    const int p = k < b.np ? b.p0 + k : b.p0;                      // a block's missing points repeat its first (never stored)
    const size_t at = (size_t)b.q * ps + p;
    b.lc[k] = LIK == kGiven ? 0.0 : a.pts.ln_conc[at];
    b.yv[k] = LIK == kGiven ? 0.0 : a.pts.response[at];
    b.tg[k] = LIK == kGiven ? 0 : clamp_tag(a.pts.tag[at], LIK == kHierarchical ? a.ne - 1 : 2);
  }
  const size_t C = (size_t)a.C;
  b.rstep = (size_t)a.Q * a.stride_cols * C;
  b.xr = a.rows + (size_t)b.q * a.stride_cols * C + b.c;
  return true;
}

// the pointwise log-likelihoods of one row x (x[k * C] is column k) at the block's live points: take(k, l), k ascending
template <int LIK, typename Args, typename Take>
__device__ __forceinline__ void phf_point_block_row(const Args& a, const phf_point_block& b, const double* x, phf_ktab k_exp,
                                                    phf_ktab k_log, Take take) {
  const size_t C = (size_t)a.C;
  if (LIK == kGiven) {
#pragma unroll
    for (int k = 0; k < kPtBlock; ++k)
      if (k < b.np) take(k, x[(size_t)(b.p0 + k) * C]);
  } else if (LIK == kHierarchical) {
    const phf_pw_sigma sg = phf_pw_sigma_terms(x[(size_t)(4 + 2 * a.ne) * C], k_log);
#pragma unroll
    for (int k = 0; k < kPtBlock; ++k) {
      if (k < b.np) {
        const double ln_ic50 = PHF_LN10 * (6.0 - x[(size_t)(4 + 2 * b.tg[k]) * C]);
        take(k, phf_pw_hier_point(b.lc[k], b.yv[k], x[(size_t)(5 + 2 * b.tg[k]) * C], ln_ic50, sg, k_exp, k_log));
      }
    }
  } else {
    const double pic50 = x[0], hill = LIK == 2 ? x[C] : 1.0;
    const double ln_ic50 = PHF_LN10 * (6.0 - pic50);
    const phf_pw_sigma sg = phf_pw_sigma_terms(x[(size_t)LIK * C], k_log);
#pragma unroll
    for (int k = 0; k < kPtBlock; ++k)
      if (k < b.np) take(k, phf_pw_sl_point(LIK, b.lc[k], b.yv[k], b.tg[k], hill, ln_ic50, sg, k_exp));
  }
}

#endif  // PHF_POINT_BLOCK_H

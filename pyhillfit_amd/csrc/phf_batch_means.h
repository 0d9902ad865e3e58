/* phf_batch_means.h — batch means on a dyadic ladder of batch sizes (the "blocking" method of Flyvbjerg & Petersen 1989; the estimator
 * behind mcmcse), accumulated per chain while the rows stream past.  ONE routine per chain, shared by the gfx950 kernel
 * (phf_batch_means.hip) and a host build (tests/test_batch_means_host.py), like phf_hier_de.h.  Plain C, compiled with
 * -ffp-contract=off: only additions and multiplications, in the order written here ("ESS beyond the lag limit").
 *
 * A chain of N rows gives two half-chains of h = floor(N/2) rows, as in phf_diagnostics.hip: half 0 = rows 0..h-1, half 1 = the last h
 * rows (the middle row of an odd N is dropped).  Within a half, row m (0-based) carries y_m = x_m - x_0 (x_0 the half's first value:
 * a pIC50 of 4.548 +- 0.002 keeps its digits).  Levels l = 0..NL-1, NL = floor(log2 h) + 1, batch size b = 2^l, batches aligned to the
 * half's start; trailing rows that do not fill a batch at level l are not used there.  The sum of a batch of level l+1 is
 * (left child) + (right child), in that order: a binary counter.  Level l holds one pending child sum exactly when bit l of m is set
 * after row m - so the depth of the cascade at row m is the number of trailing one bits of m, the same in every chain.
 * Per level and half:  S1 = sum of the batch sums,  S2 = sum of their squares (batch sum * batch sum, then added), in batch order.
 *
 * State of one (problem, column, chain): PHF_BM_FIELDS(NL) = 5 NL + 2 doubles, field f at st[f * cs] (cs = the chain count: the chain
 * index is fastest in memory):  x0[half] | pend[l] | S1[0][l] | S2[0][l] | S1[1][l] | S2[1][l].  Every value round-trips through
 * memory exactly and is produced in row order, so the state is bit-identical however the rows are cut into calls.
 *
 * phf_bm_rows() takes an unaligned head and tail row by row against memory (phf_bm_push) and aligned groups of 32 rows with levels
 * 0..4 in locals under compile-time indices (on the GPU: registers; an array indexed by a run-time level would go to scratch);
 * levels >= 5 are touched in memory once per 32 rows.  Both paths do the same operations in the same order.                      */
#ifndef PHF_BATCH_MEANS_H
#define PHF_BATCH_MEANS_H

#include <stddef.h>
#include <stdint.h>

#include "phf_half_chains.h" /* PHF_HD; the split into half-chains */

#if defined(__HIPCC__)
#define PHF_BM_UNROLL _Pragma("unroll")
#else
#define PHF_BM_UNROLL
#endif

#define PHF_BM_GROUP 32        /* rows per aligned group */
#define PHF_BM_GROUP_LEVELS 5  /* log2(PHF_BM_GROUP): levels 0..4 have their pending sums in locals within a group */
#define PHF_BM_FIELDS(nl) (5 * (nl) + 2)

/* NL = floor(log2 h) + 1 for h >= 1 */
PHF_HD int phf_bm_levels(int64_t h) {
  int nl = 0;
  while (h > 0) { ++nl; h >>= 1; }
  return nl;
}

PHF_HD int phf_bm_x0(int half) { return half; }
PHF_HD int phf_bm_pend(int l) { return 2 + l; }
PHF_HD int phf_bm_s1(int nl, int half, int l) { return 2 + nl + 2 * half * nl + l; }
PHF_HD int phf_bm_s2(int nl, int half, int l) { return 2 + nl + (2 * half + 1) * nl + l; }

/* phf_half_of under this header's earlier name: the host shims of the test suites of earlier commits, built against this
 * header, call it.  Not a second statement of the rule, and nothing in this tree uses it. */
PHF_HD int phf_bm_half_of(int64_t total_rows, int64_t n, int64_t* m) { return phf_half_of(total_rows, n, m); }

/* a finished batch of level l: into S1 and S2 of that level */
PHF_HD void phf_bm_add_block(double* st, size_t cs, int nl, int half, int l, double sum) {
  double* s1 = st + (size_t)phf_bm_s1(nl, half, l) * cs;
  double* s2 = st + (size_t)phf_bm_s2(nl, half, l) * cs;
  const double sq = sum * sum;
  *s1 = *s1 + sum;
  *s2 = *s2 + sq;
}

/* `carry` is a batch sum of level `from` that row m completes (already added to that level's S1, S2): binary-counter cascade upward */
PHF_HD void phf_bm_cascade(double* st, size_t cs, int nl, int half, int64_t m, int from, double carry) {
  for (int l = from; l < nl; ++l) {
    double* p = st + (size_t)phf_bm_pend(l) * cs;
    if (!((m >> l) & 1) || l + 1 >= nl) { *p = carry; return; }         /* the left child waits (l + 1 >= nl cannot happen for m < h) */
    carry = *p + carry;                                                  /* left + right */
    phf_bm_add_block(st, cs, nl, half, l + 1, carry);
  }
}

/* row m of a half-chain, y = x - x0, straight against memory */
PHF_HD void phf_bm_push(double* st, size_t cs, int nl, int half, int64_t m, double y) {
  phf_bm_add_block(st, cs, nl, half, 0, y);
  phf_bm_cascade(st, cs, nl, half, m, 0, y);
}

/* nr rows of ONE half-chain, the first of them row m0 of the half: row r at x[r * rstep].  m0 + nr <= h. */
PHF_HD void phf_bm_rows(const double* x, size_t rstep, int64_t nr, int64_t m0, int half, double* st, size_t cs, int nl) {
  double x0;
  if (m0 == 0) { x0 = x[0]; st[(size_t)phf_bm_x0(half) * cs] = x0; }
  else x0 = st[(size_t)phf_bm_x0(half) * cs];
  int64_t r = 0;
  for (; r < nr && ((m0 + r) & (PHF_BM_GROUP - 1)); ++r) phf_bm_push(st, cs, nl, half, m0 + r, x[(size_t)r * rstep] - x0);
  if (r + PHF_BM_GROUP <= nr) {                  /* m0 + r is a multiple of 32 and h >= 32: levels 0..5 exist, none of 0..4 is pending */
    double s1[PHF_BM_GROUP_LEVELS + 1], s2[PHF_BM_GROUP_LEVELS + 1], pend[PHF_BM_GROUP_LEVELS];
    PHF_BM_UNROLL
    for (int l = 0; l <= PHF_BM_GROUP_LEVELS; ++l) {
      s1[l] = st[(size_t)phf_bm_s1(nl, half, l) * cs];
      s2[l] = st[(size_t)phf_bm_s2(nl, half, l) * cs];
    }
    PHF_BM_UNROLL
    for (int l = 0; l < PHF_BM_GROUP_LEVELS; ++l) pend[l] = 0.0;
    for (; r + PHF_BM_GROUP <= nr; r += PHF_BM_GROUP) {
      double carry = 0.0;
      PHF_BM_UNROLL
      for (int u = 0; u < PHF_BM_GROUP; ++u) {
        carry = x[(size_t)(r + u) * rstep] - x0;
        s1[0] = s1[0] + carry;
        s2[0] = s2[0] + carry * carry;
        PHF_BM_UNROLL
        for (int l = 0; l < PHF_BM_GROUP_LEVELS; ++l) {
          if (((u + 1) & ((1 << (l + 1)) - 1)) == 0) {               /* bits 0..l of u are set: row u completes a batch of level l + 1 */
            carry = pend[l] + carry;
            s1[l + 1] = s1[l + 1] + carry;
            s2[l + 1] = s2[l + 1] + carry * carry;
          } else if (((u + 1) & ((1 << l) - 1)) == 0) {              /* bits 0..l-1 set, bit l clear: the cascade stops here */
            pend[l] = carry;
          }
        }
      }
      phf_bm_cascade(st, cs, nl, half, m0 + r + PHF_BM_GROUP - 1, PHF_BM_GROUP_LEVELS, carry);   /* carry: the group's sum, a level-5 batch */
    }
    PHF_BM_UNROLL
    for (int l = 0; l <= PHF_BM_GROUP_LEVELS; ++l) {
      st[(size_t)phf_bm_s1(nl, half, l) * cs] = s1[l];
      st[(size_t)phf_bm_s2(nl, half, l) * cs] = s2[l];
    }
    PHF_BM_UNROLL
    for (int l = 0; l < PHF_BM_GROUP_LEVELS; ++l) st[(size_t)phf_bm_pend(l) * cs] = pend[l];   /* dead values, but the state stays the row-by-row one bit for bit */
  }
  for (; r < nr; ++r) phf_bm_push(st, cs, nl, half, m0 + r, x[(size_t)r * rstep] - x0);
}

/* the variance of the batch means of one half-chain at one level: n = floor(h / b) >= 2 batches of b rows */
PHF_HD double phf_bm_block_mean_variance(double s1, double s2, double n, double b) {
  return (s2 - s1 * s1 / n) / ((n - 1.0) * (b * b));
}

#endif /* PHF_BATCH_MEANS_H */

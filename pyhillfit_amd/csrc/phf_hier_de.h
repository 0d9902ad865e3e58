/* phf_hier_de.h — the differential-evolution move between the chains of one pair of the hierarchical sampler (ter Braak 2006, DE-MC;
 * DESIGN.md §3, "Differential-evolution moves"), as ONE function per chain, shared by the gfx950 kernel (phf_hier_de.hip) and a host
 * build (tests/test_de_moves_host.py) like phf_hier_marginal.h and phf_sensitivity.h.
 *
 * The chains of a pair form populations of G consecutive chains (G = 4, 8, 16, 32 or 64; population = global chain number / G).  A round
 * has two sub-rounds h = 0, 1: in sub-round h the chains whose index within the population has parity h are updated, the n = G/2 chains
 * of the other parity are the donors and are only read.  For the updated chain x:
 *
 *   words w0..w3 = one Philox block of the samplers' rounds, counter (global chain id, problem id, round, PHF_DE_DOMAIN | h), key = seed
 *   a' = floor(w0 n / 2^32),  b' = floor(w1 (n-1) / 2^32),  b' += (b' >= a');   a = min(a', b'), b = max(a', b')     (donor numbers 0..n-1)
 *   sign = the top bit of w2 (set: -1);   sg = sign gamma
 *   x' = x + sg (x_a - x_b)                 a subtraction, a multiplication, an addition per coordinate — no fused multiply-add
 *   accept iff log u < L(x') - L(x),  u = (w3 + 1/2) / 2^32,  L(x) the log-target the state holds, L(x') = phf_hier_log_target_any
 *
 * The unordered pair {a, b} and a fair sign make the proposal exactly symmetric (x' -> x needs the same pair and the other sign: the
 * same probability), whatever the small non-uniformity of the index draw.  A NaN rejects (every comparison with it is false), and so
 * does L(x') = -inf: an accept never leaves the support.  On accept theta and the log-target change; nothing else of the state does.
 *
 * Counter word 3 of the Philox blocks in use: the samplers' small block indices, replica exchange 0x40000000, posterior predictive
 * checks 0x80000000 | b, hierarchical bands 0xC0000000; PHF_DE_DOMAIN | h = 0x20000000 | h is disjoint from all of them.          */
#ifndef PHF_HIER_DE_H
#define PHF_HIER_DE_H

#include "phf_hier_model.h"

#define PHF_DE_DOMAIN 0x20000000u

typedef struct phf_de_outcome {
  int a, b;          /* the donors' numbers among the n donors of the population, a < b */
  double sg;         /* sign gamma */
  double log_u;
  double lt_star;    /* L(x') */
  int accepted;
} phf_de_outcome;

PHF_HD int phf_de_population_ok(int G) { return G == 4 || G == 8 || G == 16 || G == 32 || G == 64; }

/* index of donor j (0..G/2-1) of sub-round h within its population: the chains of the other parity, in order */
PHF_HD int phf_de_donor_slot(int j, int h) { return 2 * j + (1 - h); }

/* the unordered donor pair a < b among n >= 2 donors, and the sign */
PHF_HD void phf_de_pick(uint32_t w0, uint32_t w1, uint32_t w2, int n, int* a, int* b, double* sign) {
  const int a1 = (int)(((uint64_t)w0 * (uint64_t)(uint32_t)n) >> 32);
  int b1 = (int)(((uint64_t)w1 * (uint64_t)(uint32_t)(n - 1)) >> 32);
  b1 += (b1 >= a1) ? 1 : 0;
  *a = a1 < b1 ? a1 : b1;
  *b = a1 < b1 ? b1 : a1;
  *sign = (w2 >> 31) ? -1.0 : 1.0;
}

/* One chain's move in sub-round h.
 *   x     this chain's theta, coordinate i at x[i * ts]             (read; written on accept)
 *   pop   theta of the FIRST chain of this chain's population, chain j's coordinate i at pop[i * ts + j]   (donors: read only)
 *   lt    this chain's log-target                                   (read; written on accept)
 *   star  where the proposal goes, coordinate i at star[i * ts]     (the target reads it from there)
 * n_expts a literal at the kernels' call sites for n_expts <= PHF_HIER_BATCHED_MAX_EXPTS (phf_hier_log_target_any then folds to the
 * unrolled batched target: no array is indexed at run time). */
PHF_HD phf_de_outcome phf_de_move(int n_expts, const int* expt_start, const double* lc, const double* y, const phf_hier_prior* pr,
                                  int G, int h, uint32_t chain_id, uint32_t problem_id, uint32_t round, uint32_t seed_lo, uint32_t seed_hi,
                                  double gamma, double* x, const double* pop, double* lt, double* star, int ts, phf_ktab k_exp,
                                  phf_ktab k_log) {
  const int dim = 5 + 2 * n_expts;
  phf_de_outcome o;
  const phf_u32x4 w = phf_philox_mh(chain_id, problem_id, round, PHF_DE_DOMAIN | (uint32_t)h, seed_lo, seed_hi);
  double sign;
  phf_de_pick(w.w[0], w.w[1], w.w[2], G / 2, &o.a, &o.b, &sign);
  o.sg = sign * gamma;
  o.log_u = phf_log_pos_k(phf_unit_open32(w.w[3]), k_log);
  const double* xa = pop + phf_de_donor_slot(o.a, h);
  const double* xb = pop + phf_de_donor_slot(o.b, h);
  for (int i = 0; i < dim; ++i) {
    const double diff = xa[i * ts] - xb[i * ts];
    const double step = o.sg * diff;
    star[i * ts] = x[i * ts] + step;
  }
  o.lt_star = phf_hier_log_target_any(n_expts, expt_start, lc, y, star, ts, pr, k_exp, k_log);
  o.accepted = o.log_u < o.lt_star - *lt;                          /* NaN: false */
  if (o.accepted) {
    for (int i = 0; i < dim; ++i) x[i * ts] = star[i * ts];
    *lt = o.lt_star;
  }
  return o;
}

#endif /* PHF_HIER_DE_H */

/* phf_hier_marginal.h — the marginal log-likelihood of one whole experiment of the hierarchical model ("Integrated
 * leave-one-experiment-out"): its (Hill_i, pIC50_i) integrated out against the population distribution of one draw
 * phi = (alpha, beta, mu, s, sigma), columns 0..3 and 4 + 2 Ne of a hierarchical row,
 *
 *   m_i(phi) = ln INT INT  PROD_j TN(y_ij | pred(c_ij; H, P), sigma)  loglogistic(H; alpha, beta)  logistic(P; mu, s)  1[P >= -2]  dH dP.
 *
 * The point term is phf_pw_hier_point.  The density on P is the factor the sampled joint carries: it is NOT renormalised for the
 * bound at -2 (the reference does not either).
 *
 * Rule.  H = alpha exp(a / beta), P = mu + s b make a and b standard logistic.  Tensor rule on (a, b) with Q nodes a side:
 *   x_k = -L + k h, k < Q, L = 16, h = 2 L / Q;      ln w_k = ln lambda(x_k) - ln SUM_k lambda(x_k),  lambda(x) = e^-x / (1 + e^-x)^2,
 *   m_i = LSE over (k, l) of  (ln w_k + ln w_l) + SUM_j l_j(H_k, P_l, sigma),      nodes with P_l < -2 left out,
 *   H_k = alpha * phf_exp_fast(x_k / beta)  (a plain IEEE division),    P_l = fma(s, x_l, mu),    the sum over j from 0 in point order.
 * The same pass forms m_i^coarse from the nodes with k and l both even, their weights renormalised over the even nodes; the gap
 * g_i = |m_i - m_i^coarse| (0 when both are the same infinity) is the rule's own error estimate.
 * sigma <= 1e-3 gives m_i = -inf (every point term is); parameters that phf_band_valid(PHF_BAND_FUTURE, ...) rejects give NaN, NaN.
 *
 * Table: `nodes` is [3][Q] doubles made ONCE on the host in fp64 (pyhillfit_amd/marginal.py: node_table) and read by the twin and
 * the kernel alike: x_k, ln w_k, ln w_k^coarse (the last is read at even k only).
 *
 * Order of operations, the same on host and device (the device result is bit-identical to the host build of this header):
 *   lanes   64 of them.  With KQ = min(Q, 64) and NP = 64 / KQ, lane t owns the Hill nodes k = t mod KQ, + 64, + 128, ... < Q (outer
 *           loop, ascending) and the pIC50 nodes l = t / KQ, + NP, + 2 NP, ... < Q (inner loop, ascending).  Q = 32: two lanes share
 *           a Hill node and take the even / the odd pIC50 nodes.
 *   lane    two online log-sum-exps (max M, S = sum exp(t - M)), one over all its nodes and one over its even-even nodes, one
 *           exponential per term: phf_mg_add.
 *   merge   a binary tree over the lanes, strides 32, 16, ..., 1, the lower lane's part first: phf_mg_merge (what a butterfly of
 *           __shfl_xor leaves in lane 0).
 *   value   M + phf_log_fast(S).
 *
 * Tables on the device: PHF_MATH_TABLES_TO_LDS() and PHF_ERFC_TABLE_TO_LDS(). */
#ifndef PHF_HIER_MARGINAL_H
#define PHF_HIER_MARGINAL_H

#include "phf_hier_bands.h"
#include "phf_pointwise.h"

#define PHF_MG_HALF_WIDTH 16.0                  /* L */
#define PHF_MG_LANES 64
#define PHF_MG_PIC50_MIN (-2.0)                 /* the support's lower bound on pIC50 */
#define PHF_MG_DEFAULT_NODES 128

typedef struct { double m, s; } phf_mg_lse;     /* max and sum of exp(term - max); empty: (-inf, 0) */

PHF_HD int phf_mg_nodes_ok(int Q) { return Q == 32 || Q == 64 || Q == 128 || Q == 256; }

PHF_HD phf_mg_lse phf_mg_empty(void) {
  phf_mg_lse a;
  a.m = -PHF_INF;
  a.s = 0.0;
  return a;
}

/* one term t (never +inf; -inf adds nothing, also to an empty sum: exp_fast drops the NaN of -inf - -inf to exp(-746) = 0) */
PHF_HD void phf_mg_add(phf_mg_lse* a, double t, phf_ktab k_exp) {
  const double d = t - a->m;
  const int up = d > 0.0;
  const double e = phf_exp_fast_k(-__builtin_fabs(d), k_exp);
  a->s = up ? phf_fma(a->s, e, 1.0) : a->s + e;
  a->m = up ? t : a->m;
}

/* a then b */
PHF_HD phf_mg_lse phf_mg_merge(phf_mg_lse a, phf_mg_lse b, phf_ktab k_exp) {
  phf_mg_lse r;
  r.m = a.m > b.m ? a.m : b.m;
  const double ea = phf_exp_fast_k(a.m - r.m, k_exp), eb = phf_exp_fast_k(b.m - r.m, k_exp);
  r.s = phf_fma(a.s, ea, b.s * eb);
  return r;
}

PHF_HD double phf_mg_value(phf_mg_lse a, phf_ktab k_log) { return a.m + phf_log_fast_k(a.s, k_log); }

PHF_HD double phf_mg_gap(double fine, double coarse) { return fine == coarse ? 0.0 : __builtin_fabs(fine - coarse); }

/* lane `lane`'s share of the rule for valid (alpha, beta, mu, s): the experiment's n points at ln_conc[j], y[j] */
PHF_HD void phf_mg_lane(int lane, int Q, const double* nodes, int n, const double* ln_conc, const double* y, double alpha,
                        double beta, double mu, double s, phf_pw_sigma sg, phf_ktab k_exp, phf_ktab k_log, phf_mg_lse* fine,
                        phf_mg_lse* coarse) {
  const int kq = Q < PHF_MG_LANES ? Q : PHF_MG_LANES, np = PHF_MG_LANES / kq;
  const double *x = nodes, *lw = nodes + Q, *lwc = nodes + 2 * Q;
  phf_mg_lse f = phf_mg_empty(), c = phf_mg_empty();
  for (int k = lane % kq; k < Q; k += PHF_MG_LANES) {
    const double hill = alpha * phf_exp_fast_k(x[k] / beta, k_exp);
    const double lwk = lw[k], lwck = lwc[k];
    for (int l = lane / kq; l < Q; l += np) {
      const double pic50 = phf_fma(s, x[l], mu);
      if (pic50 < PHF_MG_PIC50_MIN) continue;
      const double ln_ic50 = PHF_LN10 * (6.0 - pic50);
      double sum = 0.0;
      for (int j = 0; j < n; ++j) sum += phf_pw_hier_point(ln_conc[j], y[j], hill, ln_ic50, sg, k_exp, k_log);
      phf_mg_add(&f, (lwk + lw[l]) + sum, k_exp);
      if (!((k | l) & 1)) phf_mg_add(&c, (lwck + lwc[l]) + sum, k_exp);
    }
  }
  *fine = f;
  *coarse = c;
}

/* the tree over per-lane parts a[PHF_MG_LANES] (overwritten); the result is a[0] */
PHF_HD phf_mg_lse phf_mg_tree(phf_mg_lse* a, phf_ktab k_exp) {
  for (int o = PHF_MG_LANES / 2; o > 0; o >>= 1)
    for (int t = 0; t < o; ++t) a[t] = phf_mg_merge(a[t], a[t + o], k_exp);
  return a[0];
}

/* host form of the whole rule (the kernel runs phf_mg_lane in its 64 lanes and the tree as shuffles): out[0] = m_i, out[1] = g_i */
PHF_HD void phf_mg_experiment(int Q, const double* nodes, int n, const double* ln_conc, const double* y, double alpha, double beta,
                              double mu, double s, double sigma, double* out) {
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  if (!phf_band_valid(PHF_BAND_FUTURE, alpha, beta, mu, s) || sigma != sigma) {
    out[0] = PHF_NAN;
    out[1] = PHF_NAN;
    return;
  }
  const phf_pw_sigma sg = phf_pw_sigma_terms(sigma, k_log);
  if (sg.base == -PHF_INF) {                    /* at or below the sigma floor: every term is -inf */
    out[0] = -PHF_INF;
    out[1] = 0.0;
    return;
  }
  phf_mg_lse f[PHF_MG_LANES], c[PHF_MG_LANES];
  for (int t = 0; t < PHF_MG_LANES; ++t) phf_mg_lane(t, Q, nodes, n, ln_conc, y, alpha, beta, mu, s, sg, k_exp, k_log, &f[t], &c[t]);
  const double fine = phf_mg_value(phf_mg_tree(f, k_exp), k_log), coarse = phf_mg_value(phf_mg_tree(c, k_exp), k_log);
  out[0] = fine;
  out[1] = phf_mg_gap(fine, coarse);
}

#endif /* PHF_HIER_MARGINAL_H */

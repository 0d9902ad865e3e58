/* phf_savage_dickey.h — the Bayes factor B12 of "Hill fixed at 1" (model 1) against "Hill free" (model 2) from the t = 1 draws of the
 * model-2 fit alone, by the Savage-Dickey density ratio (Dickey 1971; Verdinelli & Wasserman 1995), Rao-Blackwellised over Hill
 * ("Savage-Dickey Bayes factor").
 *
 * Model 1 is model 2 at Hill = 1, the priors on pIC50 and sigma are the same independent factors in both models (phf_sl_log_prior: one
 * expression) and Hill's prior is uniform on [0, PHF_HILL_UPPER], so
 *
 *   B12 = p(Hill = 1 | y, M2) / pi(Hill = 1 | M2) = E_{(pIC50, sigma) | y, M2} [ r ],
 *   r   = L(pIC50, 1, sigma) / ( (1 / PHF_HILL_UPPER) INT_0^PHF_HILL_UPPER L(pIC50, h, sigma) dh ).
 *
 * A draw's own Hill column is not read.  This holds ONLY for these nested priors: the assertions below stand guard.
 *
 * l(h), the part of the model-2 log-likelihood at the draw's (pIC50, sigma) that depends on h, over the pair's merged entries
 * (include/pyhillfit_amd.h, phf_points: n_other uncensored entries, then n_cens censored ones):
 *   sse  = SUM_j w_j (y_j - pred_j(h))^2     as sse <- fma(w_j r_j, r_j, sse) from 0, in entry order, pred_j = phf_pw_pred(2, ...)
 *   cens = SUM_j w_j log Phi(z_j(h))         as cens <- fma(w_j, phf_log_ndtr_tab(z_j, -z_j / sqrt 2), cens) from 0, in entry order
 *   l(h) = fma(-sse, 0.5 (1/sigma)^2, cens)
 * -n ln sigma, the pi term and the within-entry sum of squares do not depend on h and cancel in r.
 *
 * Rule.  `nodes` is [3][Q] doubles, Q = 15 P, made ONCE on the host in fp64 (pyhillfit_amd/savage_dickey.py: node_table) and read by
 * the twin and the kernel alike: [0, 10] in P equal panels, on each the 15-point Gauss-Kronrod rule; rows h_k, ln w_k (Kronrod:
 * fine), ln w_k (the 7 embedded Gauss nodes with the Gauss weights: coarse; -inf at the other 8 nodes).
 *   log m_fine = LSE_k (ln w_k + l(h_k)) - ln 10,   log m_coarse likewise,   log r = l(1) - log m,   r = phf_exp_fast(log r).
 *
 * Order of operations, the same on host and device (the device accumulators are bit-identical to the host build of this header):
 *   lanes   64 of them; lane t owns the nodes t, t + 64, ... <= Q in ascending order, "node Q" being h = 1.0, whose l is l(1) and
 *           enters no sum (so lane Q mod 64 evaluates it: at P = 16 and 32 a lane that would idle in the last round).
 *   lane    two online log-sum-exps (phf_mg_lse of phf_hier_marginal.h), fine over all its nodes, coarse over its Gauss nodes.
 *   merge   the binary tree of phf_mg_tree: strides 32, 16, ..., 1, the lower lane's part first.
 *   sums    per (problem, chain), PHF_SD_ACC_DOUBLES doubles, every one the plain left-to-right sum (or maximum) over the chain's
 *           used rows in row order, started from the stored value; nothing is merged across chains on the device; no atomics.
 *             [0] draws used   [1] draws skipped   [2] SUM r_fine   [3] SUM r_fine^2 (acc + r r)   [4] max r_fine
 *             [5] SUM r_coarse [6] max |log r_fine - log r_coarse|   [7] spare, 0
 * A draw with sigma <= PHF_SIGMA_FLOOR, or whose pIC50 or sigma is not finite, is skipped and counted.
 *
 * Tables on the device: PHF_MATH_TABLES_TO_LDS() and PHF_LOGPHI_TABLE_TO_LDS(). */
#ifndef PHF_SAVAGE_DICKEY_H
#define PHF_SAVAGE_DICKEY_H

#include <stddef.h>

#include "phf_hier_marginal.h"
#include "phf_pointwise.h"

#define PHF_SD_LANES 64
#define PHF_SD_PANEL_NODES 15
#define PHF_SD_DEFAULT_PANELS 32
#define PHF_SD_MAX_PANELS 64
#define PHF_SD_HILL_NULL 1.0                    /* model 1's Hill */
#define PHF_SD_LN_HILL_RANGE PHF_LN10           /* ln of the length of Hill's prior support */
#define PHF_SD_ACC_DOUBLES 8
#define PHF_SD_USED 0
#define PHF_SD_SKIPPED 1
#define PHF_SD_SUM_R 2
#define PHF_SD_SUM_R2 3
#define PHF_SD_MAX_R 4
#define PHF_SD_SUM_RC 5
#define PHF_SD_MAX_GAP 6

/* the nesting the density ratio rests on: Hill uniform on [0, 10] under model 2 (phf_sl_log_target: hill < 0.0 | hill > PHF_HILL_UPPER,
 * no other Hill term), model 1 inside it, and everything else of the two priors one expression (phf_sl_log_prior) */
#if defined(__cplusplus)
static_assert(PHF_HILL_UPPER == 10.0, "ln 10 is the log of the length of Hill's prior support");
static_assert(PHF_SD_HILL_NULL > 0.0 && PHF_SD_HILL_NULL < PHF_HILL_UPPER, "model 1 must lie inside model 2's Hill support");
#else
_Static_assert(PHF_HILL_UPPER == 10.0, "ln 10 is the log of the length of Hill's prior support");
_Static_assert(PHF_SD_HILL_NULL > 0.0 && PHF_SD_HILL_NULL < PHF_HILL_UPPER, "model 1 must lie inside model 2's Hill support");
#endif

PHF_HD int phf_sd_panels_ok(int P) { return P == 16 || P == 32 || P == 64; }

PHF_HD int phf_sd_finite(double x) { return __builtin_fabs(x) < PHF_INF; }      /* false for NaN */

PHF_HD int phf_sd_draw_ok(double pic50, double sigma) { return phf_sd_finite(pic50) & phf_sd_finite(sigma) & (sigma > PHF_SIGMA_FLOOR); }

/* l(h) of the pair's entries lc, y, w at the draw's ln IC50 and 1 / sigma */
PHF_HD double phf_sd_ell(const double* lc, const double* y, const double* w, int n_other, int n_cens, double h, double ln_ic50,
                         double inv_s, phf_ktab k_exp) {
  double sse = 0.0, cens = 0.0;
  for (int j = 0; j < n_other; ++j) {
    const double r = y[j] - phf_pw_pred(2, lc[j], h, ln_ic50, k_exp);
    sse = phf_fma(w[j] * r, r, sse);
  }
  for (int j = n_other; j < n_other + n_cens; ++j) {
    const double z = phf_censored_z(phf_pw_pred(2, lc[j], h, ln_ic50, k_exp), y[j], inv_s);
    cens = phf_fma(w[j], phf_log_ndtr_tab(z, -z * PHF_INV_SQRT2), cens);
  }
  return phf_fma(-sse, 0.5 * inv_s * inv_s, cens);
}

/* lane `lane`'s share of one draw: its two log-sum-exps and, in lane Q mod 64, l(1) (else 0) */
PHF_HD void phf_sd_lane(int lane, int Q, const double* nodes, const double* lc, const double* y, const double* w, int n_other, int n_cens,
                        double ln_ic50, double inv_s, phf_ktab k_exp, phf_mg_lse* fine, phf_mg_lse* coarse, double* ell_null) {
  const double *x = nodes, *lw = nodes + Q, *lwc = nodes + 2 * Q;
  phf_mg_lse f = phf_mg_empty(), c = phf_mg_empty();
  double e1 = 0.0;
  for (int k = lane; k <= Q; k += PHF_SD_LANES) {
    const int node = k < Q;
    const double h = node ? x[k] : PHF_SD_HILL_NULL;
    const double ell = phf_sd_ell(lc, y, w, n_other, n_cens, h, ln_ic50, inv_s, k_exp);
    if (node) {
      phf_mg_add(&f, lw[k] + ell, k_exp);
      if (lwc[k] > -PHF_INF) phf_mg_add(&c, lwc[k] + ell, k_exp);
    } else {
      e1 = ell;
    }
  }
  *fine = f;
  *coarse = c;
  *ell_null = e1;
}

/* log r = l(1) - log m from a merged log-sum-exp */
PHF_HD double phf_sd_log_r(phf_mg_lse m, double ell_null, phf_ktab k_log) {
  return ell_null - (phf_mg_value(m, k_log) - PHF_SD_LN_HILL_RANGE);
}

/* one used draw, from the merged log-sum-exps and l(1), added to the chain's accumulator a[PHF_SD_ACC_DOUBLES] */
PHF_HD void phf_sd_draw_add(phf_mg_lse fine, phf_mg_lse coarse, double ell_null, phf_ktab k_exp, phf_ktab k_log, double* a) {
  const double lrf = phf_sd_log_r(fine, ell_null, k_log), lrc = phf_sd_log_r(coarse, ell_null, k_log);
  const double rf = phf_exp_fast_k(lrf, k_exp), rc = phf_exp_fast_k(lrc, k_exp);
  const double gap = phf_mg_gap(lrf, lrc);
  a[PHF_SD_USED] += 1.0;
  a[PHF_SD_SUM_R] += rf;
  a[PHF_SD_SUM_R2] += rf * rf;
  a[PHF_SD_MAX_R] = rf > a[PHF_SD_MAX_R] ? rf : a[PHF_SD_MAX_R];
  a[PHF_SD_SUM_RC] += rc;
  a[PHF_SD_MAX_GAP] = gap > a[PHF_SD_MAX_GAP] ? gap : a[PHF_SD_MAX_GAP];
}

/* the number of rows r in [first_row, first_row + num_rows) with r mod every == 0 */
PHF_HD int64_t phf_sd_rows_used(int64_t first_row, int64_t num_rows, int every) {
  const int64_t end = first_row + num_rows;
  return (end + every - 1) / every - (first_row + every - 1) / every;
}

/* the entry counts of problem q from its phf_points counts row, clamped into the stride (no access out of bounds) */
PHF_HD void phf_sd_counts(const int32_t* cnt, int stride, int* n_other, int* n_cens) {
  const int o = cnt[0] < 0 ? 0 : (cnt[0] > stride ? stride : cnt[0]);
  const int64_t cz = (int64_t)cnt[1] + cnt[2];
  *n_other = o;
  *n_cens = cz < 0 ? 0 : (cz > stride - o ? stride - o : (int)cz);
}

#if !defined(__HIP_DEVICE_COMPILE__)
/* one draw (host form): the merged log-sum-exps and l(1); what the kernel's 64 lanes and its butterfly compute */
static void phf_sd_draw_host(int P, const double* nodes, const double* lc, const double* y, const double* w, int n_other, int n_cens,
                             double pic50, double sigma, phf_mg_lse* fine, phf_mg_lse* coarse, double* ell_null) {
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  const int Q = PHF_SD_PANEL_NODES * P;
  const double ln_ic50 = PHF_LN10 * (6.0 - pic50), inv_s = phf_rcp(sigma);
  phf_mg_lse f[PHF_SD_LANES], c[PHF_SD_LANES];
  double e1 = 0.0;
  for (int t = 0; t < PHF_SD_LANES; ++t) {
    double e;
    phf_sd_lane(t, Q, nodes, lc, y, w, n_other, n_cens, ln_ic50, inv_s, k_exp, &f[t], &c[t], &e);
    if (t == Q % PHF_SD_LANES) e1 = e;
  }
  *fine = phf_mg_tree(f, k_exp);
  *coarse = phf_mg_tree(c, k_exp);
  *ell_null = e1;
}

/* host form of the kernel: the model-2 rows [num_rows][NQ][cols][C] of a call into acc [NQ][C][PHF_SD_ACC_DOUBLES]; the entries of
 * problem q are row q of ln_conc, response, weight ([NQ][stride]) and counts ([NQ][4]) */
static void phf_sd_accumulate_host(int P, const double* nodes, const double* ln_conc, const double* response, const double* weight,
                                   const int32_t* counts, int stride, const double* rows, int64_t num_rows, int NQ, int cols, int C,
                                   int64_t first_row, int every, double* acc) {
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  const int64_t used = phf_sd_rows_used(first_row, num_rows, every), r0 = (every - first_row % every) % every;
  for (int q = 0; q < NQ; ++q) {
    int n_other, n_cens;
    phf_sd_counts(counts + 4 * q, stride, &n_other, &n_cens);
    const double *lc = ln_conc + (size_t)q * stride, *y = response + (size_t)q * stride, *w = weight + (size_t)q * stride;
    for (int c = 0; c < C; ++c) {
      double* a = acc + ((size_t)q * C + c) * PHF_SD_ACC_DOUBLES;
      for (int64_t u = 0; u < used; ++u) {
        const double* x = rows + (((size_t)(r0 + u * every) * NQ + q) * cols) * (size_t)C + c;
        const double pic50 = x[0], sigma = x[2 * (size_t)C];
        if (!phf_sd_draw_ok(pic50, sigma)) {
          a[PHF_SD_SKIPPED] += 1.0;
          continue;
        }
        phf_mg_lse f, cc;
        double e1;
        phf_sd_draw_host(P, nodes, lc, y, w, n_other, n_cens, pic50, sigma, &f, &cc, &e1);
        phf_sd_draw_add(f, cc, e1, k_exp, k_log, a);
      }
    }
  }
}
#endif

#endif /* PHF_SAVAGE_DICKEY_H */

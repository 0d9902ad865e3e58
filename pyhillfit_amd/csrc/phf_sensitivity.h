/* phf_sensitivity.h — power-scaling sensitivity of prior and likelihood (Kallioinen, Paananen, Buerkner & Vehtari 2023; the method
 * of R's priorsense), host and device alike: compiles as C11 with gcc (the tests' ground truth) and into phf_sensitivity.hip.
 *
 * Power-scaling a component c(theta) of the log-target by alpha gives p_alpha(theta) ~ p(theta | y) exp((alpha - 1) c(theta)); the draws
 * of the fit are re-weighted, never re-sampled.  This header holds
 *   the component evaluators   (prior, likelihood) of the single-level models and of the hierarchical model — calls of phf_model.h and
 *                              phf_hier_model.h, no arithmetic of their own for the targets;
 *   the weight and mass rule   e = (alpha - 1)(c - c_ref) clamped to [-8, 8], w = phf_exp(e), m = floor(w 2^20 + 1/2);
 *   the per-chain steps        sum w, sum w^2, and per column sum w, sum w d, sum w d^2 (d = x - the column's anchor), sequential, phf_fma;
 *   the CJS sums               the numerators and denominators of the cumulative Jensen-Shannon divergence of a slot's base counts
 *                              against one of its weighted mass arrays, on the CDF and on the survival function, in bin order.
 * Tables: PHF_MATH_TABLES_TO_LDS() and, single-level, PHF_LOGPHI_TABLE_TO_LDS(); hierarchical, PHF_ERFC_TABLE_TO_LDS(). */
#ifndef PHF_SENSITIVITY_H
#define PHF_SENSITIVITY_H

#include "phf_grid.h"
#include "phf_hier_model.h"
#include "phf_math.h"
#include "phf_model.h"

#define PHF_SENS_CLAMP 8.0                      /* |e| <= 8: a weight lies in [e^-8, e^8] */
#define PHF_SENS_MASS_ONE 0x1p20                /* the integer mass of weight 1 */
#define PHF_SENS_INV_LN2 0x1.71547652b82fep+0   /* 1 / ln 2 */
#define PHF_SENS_PRIOR 0                        /* components */
#define PHF_SENS_LIKELIHOOD 1
#define PHF_SENS_DOWN 0                         /* directions: alpha = 1/(1 + delta), alpha = 1 + delta */
#define PHF_SENS_UP 1

/* ---- components ------------------------------------------------------------------------------------------------------------------
 * single-level model 1 | 2, th = (pIC50, sigma) | (pIC50, Hill, sigma), the sampler's merged entries (phf_points): prior =
 * phf_sl_log_prior, likelihood = out_ll1 of phf_sl_log_target: their sum is the row's log-target column at t = 1, bit for bit.  A vector
 * with an entry that is not finite (no sampler saves one; the targets' helpers are not defined there) gives NaN, NaN. */
PHF_HD void phf_sens_sl_components(int model, const double* lc, const double* y, const double* w, int n_other, int n_cens,
                                   double n_other_points, double ss_within, double pi_bit, const double* th, phf_ktab k_exp,
                                   phf_ktab k_log, double* out_prior, double* out_lik) {
  double lik, prior, ll1;
  phf_sl_log_target(model, lc, y, w, n_other, n_cens, n_other_points, ss_within, pi_bit, 1.0, th, k_exp, k_log, &lik, &prior, &ll1);
  const int defined = __builtin_isfinite(th[0]) & __builtin_isfinite(th[1]) & (model == 1 ? 1 : __builtin_isfinite(th[model]));
  const double pr = phf_sl_log_prior(model, th, k_log);
  *out_prior = defined ? pr : PHF_NAN;
  *out_lik = defined ? ll1 : PHF_NAN;
}

/* hierarchical, th[i * ts] = [alpha, beta, mu, s, pIC50_1, Hill_1, ..., sigma], the per-experiment form of the target for every Ne:
 *   prior       the five shifted-Gamma hyper-priors (phf_hier_common.prior), the top-level priors;
 *   likelihood  -(n ln sigma + SSE / (2 sigma^2) + sum trunc) over all experiments;
 *   population  the log-logistic and logistic terms of the (Hill_i, pIC50_i): neither component.
 * (likelihood + population) + prior is phf_hier_log_target_by_experiment in its own order of additions.  Outside the support the target
 * is -inf and so are all three; a vector with an entry that is not finite gives NaN for all three.  An experiment's points are
 * expt_start[i] .. expt_start[i + 1] - 1, clamped to [0, max_pts). */
PHF_HD void phf_sens_hier_components(int n_expts, const int32_t* expt_start, int max_pts, const double* lc, const double* y,
                                     const double* th, int ts, const phf_hier_prior* pr, phf_ktab k_exp, phf_ktab k_log,
                                     double* out_prior, double* out_lik, double* out_pop) {
  const int dim = 5 + 2 * n_expts;
  const phf_hier_common c = phf_hier_common_terms(th[0], th[1 * ts], th[2 * ts], th[3 * ts], th[(dim - 1) * ts], pr, k_log);
  double sse = 0.0, trunc = 0.0, hyper = 0.0;
  int bad = 0, n_pts = 0;
  for (int i = 0; i < n_expts; ++i) {
    int s0 = expt_start[i], s1 = expt_start[i + 1];
    s0 = s0 < 0 ? 0 : (s0 > max_pts ? max_pts : s0);
    s1 = s1 < s0 ? s0 : (s1 > max_pts ? max_pts : s1);
    double a, b, h;
    int bi;
    phf_hier_experiment_terms(&c, th[(4 + 2 * i) * ts], th[(5 + 2 * i) * ts], lc + s0, y + s0, s1 - s0, k_exp, k_log, &a, &b, &h, &bi);
    sse += a; trunc += b; hyper += h; bad |= bi;
    n_pts = s1;
  }
  const double lik = -(phf_fma((double)n_pts, c.log_sigma, sse * (0.5 * c.inv_s * c.inv_s)) + trunc);
  const int outside = bad | c.bad;
  int defined = 1;
  for (int i = 0; i < dim; ++i) defined &= __builtin_isfinite(th[i * ts]);
  *out_prior = !defined ? PHF_NAN : outside ? -PHF_INF : c.prior;
  *out_lik = !defined ? PHF_NAN : outside ? -PHF_INF : lik;
  *out_pop = !defined ? PHF_NAN : outside ? -PHF_INF : hyper;
}

/* ---- weights and masses ----------------------------------------------------------------------------------------------------------
 * alpha - 1 of a direction (host side: one IEEE division) */
PHF_HD double phf_sens_alpha_m1(double delta, int direction) {
  const double alpha = direction == PHF_SENS_UP ? 1.0 + delta : 1.0 / (1.0 + delta);
  return alpha - 1.0;
}

/* w = exp(clamp((alpha - 1)(c - c_ref))) of a draw with finite c: one subtraction, one multiplication, the clamp, phf_exp */
PHF_HD double phf_sens_weight(double alpha_m1, double c, double c_ref, int* clamped) {
  const double e = alpha_m1 * (c - c_ref);
  *clamped = (e < -PHF_SENS_CLAMP) | (e > PHF_SENS_CLAMP);
  return phf_exp(__builtin_fmin(__builtin_fmax(e, -PHF_SENS_CLAMP), PHF_SENS_CLAMP));
}

/* m = floor(w 2^20 + 1/2).  w <= e^8 (phf_exp(8) 2^20 < 3 125 783 400 < 2^31.6) and a workspace takes at most 2^32 draws, so a sum of masses
 * stays below 2^63.6 < 2^64: the uint64 arrays cannot wrap.  w >= e^-8 gives m >= 351: a mass of 0 only ever means "no weight". */
PHF_HD uint64_t phf_sens_mass(double w) { return (uint64_t)__builtin_floor(w * PHF_SENS_MASS_ONE + 0.5); }

/* ---- per-chain steps (sequential in row order) -----------------------------------------------------------------------------------
 * one draw's weight of one (component, direction) into the chain's n, sum w, sum w^2 and clamped count; w == 0: the draw's component is
 * not finite (or no draw's has been yet) and it enters nothing */
PHF_HD void phf_sens_weight_step(double w, int clamped, double* n, double* sw, double* sw2, double* ncl) {
  if (w > 0.0) {
    *n += 1.0;
    *sw += w;
    *sw2 = phf_fma(w, w, *sw2);
    *ncl += (double)clamped;
  }
}

/* one draw's column value, as d = x - anchor, into the chain's sum w, sum w d, sum w d^2 of that column (the base sums take w = 1);
 * valid: the histogram bins this value (phf_sens_binned) */
PHF_HD void phf_sens_column_step(double w, double d, int valid, double* cw, double* swd, double* swd2) {
  if (valid && w > 0.0) {
    *cw += w;
    *swd = phf_fma(w, d, *swd);
    *swd2 = phf_fma(w * d, d, *swd2);
  }
}

/* the histogram bins this value (phf_grid.h) */
PHF_HD int phf_sens_binned(double x, double anchor, double inv_w0) { return phf_grid_binned(x, anchor, inv_w0); }

/* ---- cumulative Jensen-Shannon sums ----------------------------------------------------------------------------------------------
 * P log2(2P / (P + Q)) + Q log2(2Q / (P + Q)), 0 log 0 = 0 */
PHF_HD double phf_sens_js_term(double p, double q, phf_ktab k_log) {
  const double s = p + q;
  double t = 0.0;
  if (p > 0.0) t = p * (phf_log_pos_k(phf_div(2.0 * p, s), k_log) * PHF_SENS_INV_LN2);
  if (q > 0.0) t += q * (phf_log_pos_k(phf_div(2.0 * q, s), k_log) * PHF_SENS_INV_LN2);
  return t;
}

/* base[j], mass[j], j < bins: out = (numerator, denominator) on the CDF, then on the survival function, then
 * the total mass — summed in bin order over the bins from the first to the last one that holds a base draw (the uniform bin width
 * cancels; beyond them both CDFs are 0 or 1 and would only dilute the denominators).  No base draw or no mass: all 0. */
PHF_HD void phf_sens_cjs_sums(int bins, const uint64_t* base, const uint64_t* mass, phf_ktab k_log, double* out) {
  uint64_t nb = 0, nm = 0;
  int jlo = bins, jhi = -1;
  for (int j = 0; j < bins; ++j) {
    nb += base[j]; nm += mass[j];
    if (base[j]) { jhi = j; if (jlo == bins) jlo = j; }
  }
  out[0] = 0.0; out[1] = 0.0; out[2] = 0.0; out[3] = 0.0; out[4] = (double)nm;
  if (nb == 0 || nm == 0) return;
  const double dnb = (double)nb, dnm = (double)nm;
  uint64_t cb = 0, cm = 0;
  double num_c = 0.0, den_c = 0.0, num_s = 0.0, den_s = 0.0;
  for (int j = jlo; j <= jhi; ++j) {
    cb += base[j]; cm += mass[j];
    const double p = phf_div((double)cb, dnb), q = phf_div((double)cm, dnm);
    const double ps = phf_div((double)(nb - cb), dnb), qs = phf_div((double)(nm - cm), dnm);
    num_c += phf_sens_js_term(p, q, k_log);
    den_c += p + q;
    num_s += phf_sens_js_term(ps, qs, k_log);
    den_s += ps + qs;
  }
  out[0] = num_c; out[1] = den_c; out[2] = num_s; out[3] = den_s;
}

#endif /* PHF_SENSITIVITY_H */

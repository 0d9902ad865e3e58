/* phf_model.h — the single-level Hill-curve log-target and the per-iteration random draws, written once
 * and compiled both into the gfx950 kernels and into the host twin (oracle/), so the two evaluate the very
 * same fp64 operation sequence.
 *
 * What it computes is the reference's (python/doseresponse.py):
 *   dose_response_model :84-85, pic50_to_ic50 :87-88, log_data_likelihood_model_{1,2}_capped :203-248,
 *   log_priors_model_{1,2} :166-184, log_pic50_exponential :151-156, log_gamma_prior :304-317.
 * How it computes it is shaped for the fp64 VALU (see phf_math.h): per-point work is done 4 (uncensored) or
 * 2 (censored) points at a time so independent polynomial chains interleave, and the IEEE divisions of a
 * group — 1/(1+x) of the Hill curves — are shared through a product tree (one division + a few multiplies
 * instead of one division each).  Logarithms, exponentials, the censored entries' log Phi and the proposals'
 * normals come from the LDS tables of phf_math.h (no division, no erfcx, no Box-Muller).
 *
 * Entry layout (include/pyhillfit_amd.h, phf_points): n_other uncensored entries first (0 < y < 100), then the
 * n_cens censored ones (y == 0, then y == 100).  Arrays must be readable up to index n_other + n_cens - 1.
 * An entry stands for w data points at one concentration.  The reference's sums over points (:244-247) regroup
 * exactly: the curve depends on the point only through its concentration, so for replicates at one concentration
 *     sum_j (y_j - pred)^2 = sum_j (y_j - ybar)^2 + w (ybar - pred)^2      (uncensored; first term constant in theta)
 *     sum_j log Phi(z(pred)) = w log Phi(z(pred))                            (censored)
 * and the per-iteration cost scales with the number of distinct concentrations (Crumb: 4 doses x 3-6 experiments).
 * w = 1, ybar = y, ss_within = 0 is the unmerged form.
 */
#ifndef PHF_MODEL_H
#define PHF_MODEL_H

#include "phf_math.h"
#include "phf_philox.h"

#define PHF_SIGMA_FLOOR 1e-3                    /* sigma_uniform_lower, doseresponse.py:12  */
#define PHF_PIC50_RATE 0.2                      /* doseresponse.py:14  */
#define PHF_PIC50_LOWER (-3.0)                  /* doseresponse.py:16  */
#define PHF_HILL_UPPER 10.0                     /* doseresponse.py:18  */
#define PHF_SIGMA_LOC 1e-3                      /* doseresponse.py:24  */
#define PHF_SIGMA_SHAPE_M1 4.0                  /* sigma_shape - 1, doseresponse.py:22 */
#define PHF_SIGMA_INV_SCALE (4.0 / (6.0 - 1e-3)) /* 1/sigma_scale, doseresponse.py:25 */
#define PHF_HILL_ARG_CAP 40.0                   /* exp(40): 100/(1+x) already rounds pred to exactly 100 */

/* Hill-curve denominator 1 + (dose/IC50)^hill = 1 + exp(hill (ln dose - ln IC50))   (doseresponse.py:84-88) */
PHF_HD double phf_hill_den(int model, double ln_conc, double hill, double ln_ic50, phf_ktab k_exp) {
  const double a = (model == 1) ? (ln_conc - ln_ic50) : hill * (ln_conc - ln_ic50);
  return 1.0 + phf_exp_capped_k(__builtin_fmin(a, PHF_HILL_ARG_CAP), k_exp);
}

/* percent block from w = 1/(1 + x):  100 (1 - w) */
PHF_HD double phf_hill_percent(double w, phf_ktab k_exp) { return phf_fma(-PHF_K100(k_exp), w, PHF_K100(k_exp)); }
#define PHF_PCT_(w_) phf_hill_percent((w_), k_exp)      /* inside the target: k_exp is in scope */

/* z-score of a censored point: y == 0 -> (0 - pred)/sigma (logcdf, :244); y == 100 -> (pred - 100)/sigma (logsf, :245) */
PHF_HD double phf_censored_z(double pred, double y, double inv_s) {
  const double sgn = (y > 50.0) ? 1.0 : -1.0;
  return (sgn * (pred - y)) * inv_s;
}

/* log-likelihood (tempered), log-prior and UNtempered log-likelihood of one parameter vector.
 * model 1: th = (pIC50, sigma), Hill = 1;  model 2: th = (pIC50, Hill, sigma).
 * out_ll1 = log_data_likelihood(..., t = 1): what python/compute_bayes_factors.py:18-21 re-evaluates for every saved
 * sample of every rung; it falls out of the same arithmetic here, so the samplers carry it along for free.      */
PHF_HD void phf_sl_log_target(int model, const double* lc, const double* y, const double* w, int n_other, int n_cens,
                              double n_other_points, double ss_within, double pi_bit, double temperature,
                              const double* th, phf_ktab k_exp, phf_ktab k_log,
                              double* out_lik, double* out_prior, double* out_ll1) {
  const double pic50 = th[0];
  const double hill = (model == 1) ? 1.0 : th[1];
  const double sigma = (model == 1) ? th[1] : th[2];
  const double ln_ic50 = PHF_LN10 * (6.0 - pic50);
  const double sl = sigma - PHF_SIGMA_LOC;
  const double inv_s = phf_rcp(sigma);
  const double log_sigma = phf_log_pos_k(sigma, k_log);
  const double log_sl = phf_log_pos_k(sl, k_log);

  double sse = ss_within, cens = 0.0;
  int j = 0;
  for (; j + 4 <= n_other; j += 4) {              /* uncensored entries, four at a time (:247) */
    const phf_ktab ke = k_exp;
    const double d0 = phf_hill_den(model, lc[j], hill, ln_ic50, ke), d1 = phf_hill_den(model, lc[j + 1], hill, ln_ic50, ke);
    const double d2 = phf_hill_den(model, lc[j + 2], hill, ln_ic50, ke), d3 = phf_hill_den(model, lc[j + 3], hill, ln_ic50, ke);
    const double p01 = d0 * d1, p23 = d2 * d3;
    const double inv = phf_rcp(p01 * p23);
    const double i01 = inv * p23, i23 = inv * p01;
    const double r0 = y[j] - PHF_PCT_(i01 * d1), r1 = y[j + 1] - PHF_PCT_(i01 * d0);
    const double r2 = y[j + 2] - PHF_PCT_(i23 * d3), r3 = y[j + 3] - PHF_PCT_(i23 * d2);
    sse = phf_fma(w[j] * r0, r0, sse); sse = phf_fma(w[j + 1] * r1, r1, sse);
    sse = phf_fma(w[j + 2] * r2, r2, sse); sse = phf_fma(w[j + 3] * r3, r3, sse);
  }
  const int rem = n_other - j;                    /* 0..3 left: still one division */
  if (rem == 3) {
    const phf_ktab ke = k_exp;
    const double d0 = phf_hill_den(model, lc[j], hill, ln_ic50, ke), d1 = phf_hill_den(model, lc[j + 1], hill, ln_ic50, ke);
    const double d2 = phf_hill_den(model, lc[j + 2], hill, ln_ic50, ke);
    const double p01 = d0 * d1;
    const double inv = phf_rcp(p01 * d2);
    const double i01 = inv * d2;
    const double r0 = y[j] - PHF_PCT_(i01 * d1), r1 = y[j + 1] - PHF_PCT_(i01 * d0);
    const double r2 = y[j + 2] - PHF_PCT_(inv * p01);
    sse = phf_fma(w[j] * r0, r0, sse); sse = phf_fma(w[j + 1] * r1, r1, sse); sse = phf_fma(w[j + 2] * r2, r2, sse);
  } else if (rem == 2) {
    const phf_ktab ke = k_exp;
    const double d0 = phf_hill_den(model, lc[j], hill, ln_ic50, ke), d1 = phf_hill_den(model, lc[j + 1], hill, ln_ic50, ke);
    const double inv = phf_rcp(d0 * d1);
    const double r0 = y[j] - PHF_PCT_(inv * d1), r1 = y[j + 1] - PHF_PCT_(inv * d0);
    sse = phf_fma(w[j] * r0, r0, sse); sse = phf_fma(w[j + 1] * r1, r1, sse);
  } else if (rem == 1) {
    const double r = y[j] - PHF_PCT_(phf_rcp(phf_hill_den(model, lc[j], hill, ln_ic50, k_exp)));
    sse = phf_fma(w[j] * r, r, sse);
  }
  j = n_other;
  const int n = n_other + n_cens;
  /* censored entries (:244-245): log Phi(z), z <= 0, from the table of phf_math.h — it covers every z a likelihood that is not
   * -inf anyway (sigma above its floor, below) can produce */
  for (; j + 2 <= n; j += 2) {                    /* two at a time: one division for the two Hill curves */
    const phf_ktab ke = k_exp;
    const double d0 = phf_hill_den(model, lc[j], hill, ln_ic50, ke), d1 = phf_hill_den(model, lc[j + 1], hill, ln_ic50, ke);
    const double inv = phf_rcp(d0 * d1);
    const double z0 = phf_censored_z(PHF_PCT_(inv * d1), y[j], inv_s);
    const double z1 = phf_censored_z(PHF_PCT_(inv * d0), y[j + 1], inv_s);
    cens = phf_fma(w[j], phf_log_ndtr_tab(z0, -z0 * PHF_INV_SQRT2), cens);
    cens = phf_fma(w[j + 1], phf_log_ndtr_tab(z1, -z1 * PHF_INV_SQRT2), cens);
  }
  for (; j < n; ++j) {
    const double pred = PHF_PCT_(phf_rcp(phf_hill_den(model, lc[j], hill, ln_ic50, k_exp)));
    const double z = phf_censored_z(pred, y[j], inv_s);
    cens = phf_fma(w[j], phf_log_ndtr_tab(z, -z * PHF_INV_SQRT2), cens);
  }
  double a = cens - pi_bit;
  a = phf_fma(-n_other_points, log_sigma, a);                            /* :246 */
  a = phf_fma(-sse, 0.5 * inv_s * inv_s, a);                             /* :247 */
  if (sigma <= PHF_SIGMA_FLOOR) a = -PHF_INF;                            /* :238-240 (one select: t * -inf = -inf for t > 0 ...) */
  double lik = temperature * a;                                          /* :248 */
  if (temperature == 0.0) lik = 0.0;                                     /* :230-231 (... and t = 0 is 0 whatever a is) */
  *out_lik = lik;
  *out_ll1 = a;

  /* the prior: -inf outside ANY of the supports, the sum of the two terms inside (one select on one combined predicate, not one per
   * term: the reference's -inf + x and -inf + -inf are -inf either way) */
  const int outside = (pic50 < PHF_PIC50_LOWER)                          /* :151-156 */
                      | (sigma <= PHF_SIGMA_LOC)                         /* :304-317: x < loc -> -inf; x == loc -> log 0 = -inf */
                      | ((model == 2) & ((hill < 0.0) | (hill > PHF_HILL_UPPER)));   /* :181-182 */
  const double g = phf_fma(PHF_SIGMA_SHAPE_M1, log_sl, -sl * PHF_SIGMA_INV_SCALE);
  const double lp = -PHF_PIC50_RATE * pic50 + g;
  *out_prior = outside ? -PHF_INF : lp;
}

/* phf_sl_log_target with the censored entries' Hill denominators shared: the same arguments, results and fp64 operations, except
 * that a censored entry whose bit m (m = its index among the censored entries) is set in share_mask does not evaluate phf_hill_den
 * but takes den_slot[den_off[m]], the denominator an uncensored entry at the same ln_conc BITS left there in this call
 * (phf_hill_den is a pure function of (ln_conc, theta): it is the same double).  When share_mask != 0 every uncensored entry j stores
 * its denominator at den_slot[j * slot_stride]; den_slot must hold n_other such slots.  Entries keep their order, and so do both sums.
 * The samplers pass a compile-time share_mask (the mask folds away) and per-wavefront LDS slots (slot_stride = lanes of the block). */
#define PHF_SHARE_PUT_(jj, d_) do { if (share_mask) den_slot[(jj) * slot_stride] = (d_); } while (0)
#define PHF_CDEN_(jj) ((((share_mask) >> ((jj) - n_other)) & 1u) ? den_slot[den_off[(jj) - n_other]] \
                                                                 : phf_hill_den(model, lc[jj], hill, ln_ic50, k_exp))
PHF_HD void phf_sl_log_target_shared(int model, const double* lc, const double* y, const double* w, int n_other, int n_cens,
                                     double n_other_points, double ss_within, double pi_bit, double temperature,
                                     const double* th, phf_ktab k_exp, phf_ktab k_log,
                                     unsigned share_mask, const int* den_off, double* den_slot, int slot_stride,
                                     double* out_lik, double* out_prior, double* out_ll1) {
  const double pic50 = th[0];
  const double hill = (model == 1) ? 1.0 : th[1];
  const double sigma = (model == 1) ? th[1] : th[2];
  const double ln_ic50 = PHF_LN10 * (6.0 - pic50);
  const double sl = sigma - PHF_SIGMA_LOC;
  const double inv_s = phf_rcp(sigma);
  const double log_sigma = phf_log_pos_k(sigma, k_log);
  const double log_sl = phf_log_pos_k(sl, k_log);

  double sse = ss_within, cens = 0.0;
  int j = 0;
  for (; j + 4 <= n_other; j += 4) {
    const phf_ktab ke = k_exp;
    const double d0 = phf_hill_den(model, lc[j], hill, ln_ic50, ke), d1 = phf_hill_den(model, lc[j + 1], hill, ln_ic50, ke);
    const double d2 = phf_hill_den(model, lc[j + 2], hill, ln_ic50, ke), d3 = phf_hill_den(model, lc[j + 3], hill, ln_ic50, ke);
    PHF_SHARE_PUT_(j, d0); PHF_SHARE_PUT_(j + 1, d1); PHF_SHARE_PUT_(j + 2, d2); PHF_SHARE_PUT_(j + 3, d3);
    const double p01 = d0 * d1, p23 = d2 * d3;
    const double inv = phf_rcp(p01 * p23);
    const double i01 = inv * p23, i23 = inv * p01;
    const double r0 = y[j] - PHF_PCT_(i01 * d1), r1 = y[j + 1] - PHF_PCT_(i01 * d0);
    const double r2 = y[j + 2] - PHF_PCT_(i23 * d3), r3 = y[j + 3] - PHF_PCT_(i23 * d2);
    sse = phf_fma(w[j] * r0, r0, sse); sse = phf_fma(w[j + 1] * r1, r1, sse);
    sse = phf_fma(w[j + 2] * r2, r2, sse); sse = phf_fma(w[j + 3] * r3, r3, sse);
  }
  const int rem = n_other - j;
  if (rem == 3) {
    const phf_ktab ke = k_exp;
    const double d0 = phf_hill_den(model, lc[j], hill, ln_ic50, ke), d1 = phf_hill_den(model, lc[j + 1], hill, ln_ic50, ke);
    const double d2 = phf_hill_den(model, lc[j + 2], hill, ln_ic50, ke);
    PHF_SHARE_PUT_(j, d0); PHF_SHARE_PUT_(j + 1, d1); PHF_SHARE_PUT_(j + 2, d2);
    const double p01 = d0 * d1;
    const double inv = phf_rcp(p01 * d2);
    const double i01 = inv * d2;
    const double r0 = y[j] - PHF_PCT_(i01 * d1), r1 = y[j + 1] - PHF_PCT_(i01 * d0);
    const double r2 = y[j + 2] - PHF_PCT_(inv * p01);
    sse = phf_fma(w[j] * r0, r0, sse); sse = phf_fma(w[j + 1] * r1, r1, sse); sse = phf_fma(w[j + 2] * r2, r2, sse);
  } else if (rem == 2) {
    const phf_ktab ke = k_exp;
    const double d0 = phf_hill_den(model, lc[j], hill, ln_ic50, ke), d1 = phf_hill_den(model, lc[j + 1], hill, ln_ic50, ke);
    PHF_SHARE_PUT_(j, d0); PHF_SHARE_PUT_(j + 1, d1);
    const double inv = phf_rcp(d0 * d1);
    const double r0 = y[j] - PHF_PCT_(inv * d1), r1 = y[j + 1] - PHF_PCT_(inv * d0);
    sse = phf_fma(w[j] * r0, r0, sse); sse = phf_fma(w[j + 1] * r1, r1, sse);
  } else if (rem == 1) {
    const double d0 = phf_hill_den(model, lc[j], hill, ln_ic50, k_exp);
    PHF_SHARE_PUT_(j, d0);
    const double r = y[j] - PHF_PCT_(phf_rcp(d0));
    sse = phf_fma(w[j] * r, r, sse);
  }
  j = n_other;
  const int n = n_other + n_cens;
  for (; j + 2 <= n; j += 2) {
    const double d0 = PHF_CDEN_(j), d1 = PHF_CDEN_(j + 1);
    const double inv = phf_rcp(d0 * d1);
    const double z0 = phf_censored_z(PHF_PCT_(inv * d1), y[j], inv_s);
    const double z1 = phf_censored_z(PHF_PCT_(inv * d0), y[j + 1], inv_s);
    cens = phf_fma(w[j], phf_log_ndtr_tab(z0, -z0 * PHF_INV_SQRT2), cens);
    cens = phf_fma(w[j + 1], phf_log_ndtr_tab(z1, -z1 * PHF_INV_SQRT2), cens);
  }
  for (; j < n; ++j) {
    const double pred = PHF_PCT_(phf_rcp(PHF_CDEN_(j)));
    const double z = phf_censored_z(pred, y[j], inv_s);
    cens = phf_fma(w[j], phf_log_ndtr_tab(z, -z * PHF_INV_SQRT2), cens);
  }
  double a = cens - pi_bit;
  a = phf_fma(-n_other_points, log_sigma, a);
  a = phf_fma(-sse, 0.5 * inv_s * inv_s, a);
  if (sigma <= PHF_SIGMA_FLOOR) a = -PHF_INF;
  double lik = temperature * a;
  if (temperature == 0.0) lik = 0.0;
  *out_lik = lik;
  *out_ll1 = a;

  const int outside = (pic50 < PHF_PIC50_LOWER)
                      | (sigma <= PHF_SIGMA_LOC)
                      | ((model == 2) & ((hill < 0.0) | (hill > PHF_HILL_UPPER)));
  const double g = phf_fma(PHF_SIGMA_SHAPE_M1, log_sl, -sl * PHF_SIGMA_INV_SCALE);
  const double lp = -PHF_PIC50_RATE * pic50 + g;
  *out_prior = outside ? -PHF_INF : lp;
}

/* phf_sl_log_target_shared for the samplers' steady iteration: the same arguments and the same fp64 operations in the same order,
 * WITHOUT the two -inf selects.  It returns `outside` — the prior's combined predicate, as above — and leaves in out_lik, out_prior,
 * out_ll1 and out_lt (= lik + prior) the values the selects would have replaced; the caller rejects an `outside` proposal by the
 * predicate:  accept = !outside & (accept test on out_lt - lt).
 * Exact, case by case (x = lt_star - lt is the accept test's argument; both tests reject -inf and NaN):
 *   outside, lt finite: phf_sl_log_target_shared gives prior = -inf, so lt_star = lik + -inf is -inf or NaN for every lik (finite,
 *     +-inf, NaN, or the 0 of temperature 0), x is -inf or NaN and the test rejects: what the predicate does here.
 *   outside, lt = -inf (a start outside the support): lt_star is again -inf or NaN, x = lt_star + inf is NaN: reject, likewise.
 *   sigma <= PHF_SIGMA_FLOOR (the likelihood's -inf): floor and PHF_SIGMA_LOC are one double (asserted below), so this IS `outside`.
 *   not outside: neither select changes a value there either; lik, prior, ll1 are the same doubles (a NaN theta compares false
 *     everywhere, is not `outside` in either version and runs the same arithmetic).
 * theta, lt and ll1 are taken over only on accept, so the unselected values of a rejected proposal are never seen.
 * lower_clamp == 0 promises that every ln_conc of the pair is >= PHF_LN_CONC_NOCLAMP: the Hill denominators' exponentials then skip
 * the lower clamp fmax(a, -746) of phf_exp_capped_k, which cannot fire inside the support: there hill is in [0, PHF_HILL_UPPER] and
 * pic50 >= PHF_PIC50_LOWER, so ln_ic50 <= 9 ln 10 = 20.8 and the argument a = hill (ln_conc - ln_ic50) >= 10 (-50 - 20.8) = -708 (model 1:
 * >= -70.8), far above -746 (fmax(a, -746) = a: the same double).  Outside the support the exponential may return anything — the
 * proposal is rejected by the predicate — and its table index is masked (phf_exp_core_k: n & 63), so no address depends on it.  A NaN
 * argument is still dropped by the upper cap fmin(a, PHF_HILL_ARG_CAP), which stays.
 * temp0_select == 0 promises that the temperature is neither +-0 nor NaN: the select lik = 0 at temperature 0 (two v_cndmask_b32 on a
 * wave-uniform condition, every iteration) then never fires and is left out; the multiply stays (round 11).
 * A shared censored entry m reads the double at BYTE offset den_byte_off[m] from den_read: the samplers pass offsets computed once per call
 * from the base of all lanes' slots; den_byte_off[m] = 8 den_off[m] with den_read = den_slot is the form above. */
#define PHF_LN_CONC_NOCLAMP (-50.0)
#if defined(__cplusplus)
static_assert(PHF_SIGMA_FLOOR == PHF_SIGMA_LOC, "sigma <= floor must imply outside");
#else
_Static_assert(PHF_SIGMA_FLOOR == PHF_SIGMA_LOC, "sigma <= floor must imply outside");
#endif
PHF_HD double phf_hill_den_sampler(int model, double ln_conc, double hill, double ln_ic50, int lower_clamp, phf_ktab k_exp) {
  const double a = (model == 1) ? (ln_conc - ln_ic50) : hill * (ln_conc - ln_ic50);
  const double c = __builtin_fmin(a, PHF_HILL_ARG_CAP);
  return 1.0 + (lower_clamp ? phf_exp_capped_k(c, k_exp) : phf_exp_core_k(c, k_exp));
}
#define PHF_DEN_(jj) phf_hill_den_sampler(model, lc[jj], hill, ln_ic50, lower_clamp, k_exp)
#define PHF_CDEN_S_(jj) ((((share_mask) >> ((jj) - n_other)) & 1u) ? *(const double*)((const char*)den_read + den_byte_off[(jj) - n_other]) \
                                                                   : PHF_DEN_(jj))
PHF_HD int phf_sl_log_target_sampler_t(int model, const double* lc, const double* y, const double* w, int n_other, int n_cens,
                                       double n_other_points, double ss_within, double pi_bit, double temperature, int lower_clamp,
                                       int temp0_select, const double* th, phf_ktab k_exp, phf_ktab k_log,
                                       unsigned share_mask, const int* den_byte_off, const double* den_read, double* den_slot, int slot_stride,
                                       double* out_lik, double* out_prior, double* out_ll1, double* out_lt) {
  const double pic50 = th[0];
  const double hill = (model == 1) ? 1.0 : th[1];
  const double sigma = (model == 1) ? th[1] : th[2];
  const double ln_ic50 = PHF_LN10 * (6.0 - pic50);
  const double sl = sigma - PHF_SIGMA_LOC;
  const double inv_s = phf_rcp(sigma);
  const double log_sigma = phf_log_pos_k(sigma, k_log);
  const double log_sl = phf_log_pos_k(sl, k_log);

  double sse = ss_within, cens = 0.0;
  int j = 0;
  for (; j + 4 <= n_other; j += 4) {
    const double d0 = PHF_DEN_(j), d1 = PHF_DEN_(j + 1);
    const double d2 = PHF_DEN_(j + 2), d3 = PHF_DEN_(j + 3);
    PHF_SHARE_PUT_(j, d0); PHF_SHARE_PUT_(j + 1, d1); PHF_SHARE_PUT_(j + 2, d2); PHF_SHARE_PUT_(j + 3, d3);
    const double p01 = d0 * d1, p23 = d2 * d3;
    const double inv = phf_rcp(p01 * p23);
    const double i01 = inv * p23, i23 = inv * p01;
    const double r0 = y[j] - PHF_PCT_(i01 * d1), r1 = y[j + 1] - PHF_PCT_(i01 * d0);
    const double r2 = y[j + 2] - PHF_PCT_(i23 * d3), r3 = y[j + 3] - PHF_PCT_(i23 * d2);
    sse = phf_fma(w[j] * r0, r0, sse); sse = phf_fma(w[j + 1] * r1, r1, sse);
    sse = phf_fma(w[j + 2] * r2, r2, sse); sse = phf_fma(w[j + 3] * r3, r3, sse);
  }
  const int rem = n_other - j;
  if (rem == 3) {
    const double d0 = PHF_DEN_(j), d1 = PHF_DEN_(j + 1);
    const double d2 = PHF_DEN_(j + 2);
    PHF_SHARE_PUT_(j, d0); PHF_SHARE_PUT_(j + 1, d1); PHF_SHARE_PUT_(j + 2, d2);
    const double p01 = d0 * d1;
    const double inv = phf_rcp(p01 * d2);
    const double i01 = inv * d2;
    const double r0 = y[j] - PHF_PCT_(i01 * d1), r1 = y[j + 1] - PHF_PCT_(i01 * d0);
    const double r2 = y[j + 2] - PHF_PCT_(inv * p01);
    sse = phf_fma(w[j] * r0, r0, sse); sse = phf_fma(w[j + 1] * r1, r1, sse); sse = phf_fma(w[j + 2] * r2, r2, sse);
  } else if (rem == 2) {
    const double d0 = PHF_DEN_(j), d1 = PHF_DEN_(j + 1);
    PHF_SHARE_PUT_(j, d0); PHF_SHARE_PUT_(j + 1, d1);
    const double inv = phf_rcp(d0 * d1);
    const double r0 = y[j] - PHF_PCT_(inv * d1), r1 = y[j + 1] - PHF_PCT_(inv * d0);
    sse = phf_fma(w[j] * r0, r0, sse); sse = phf_fma(w[j + 1] * r1, r1, sse);
  } else if (rem == 1) {
    const double d0 = PHF_DEN_(j);
    PHF_SHARE_PUT_(j, d0);
    const double r = y[j] - PHF_PCT_(phf_rcp(d0));
    sse = phf_fma(w[j] * r, r, sse);
  }
  j = n_other;
  const int n = n_other + n_cens;
  for (; j + 2 <= n; j += 2) {
    const double d0 = PHF_CDEN_S_(j), d1 = PHF_CDEN_S_(j + 1);
    const double inv = phf_rcp(d0 * d1);
    const double z0 = phf_censored_z(PHF_PCT_(inv * d1), y[j], inv_s);
    const double z1 = phf_censored_z(PHF_PCT_(inv * d0), y[j + 1], inv_s);
    cens = phf_fma(w[j], phf_log_ndtr_tab(z0, -z0 * PHF_INV_SQRT2), cens);
    cens = phf_fma(w[j + 1], phf_log_ndtr_tab(z1, -z1 * PHF_INV_SQRT2), cens);
  }
  for (; j < n; ++j) {
    const double pred = PHF_PCT_(phf_rcp(PHF_CDEN_S_(j)));
    const double z = phf_censored_z(pred, y[j], inv_s);
    cens = phf_fma(w[j], phf_log_ndtr_tab(z, -z * PHF_INV_SQRT2), cens);
  }
  double a = cens - pi_bit;
  a = phf_fma(-n_other_points, log_sigma, a);
  a = phf_fma(-sse, 0.5 * inv_s * inv_s, a);
  *out_ll1 = a;

  const int outside = (pic50 < PHF_PIC50_LOWER)
                      | (sigma <= PHF_SIGMA_LOC)
                      | ((model == 2) & ((hill < 0.0) | (hill > PHF_HILL_UPPER)));
  const double g = phf_fma(PHF_SIGMA_SHAPE_M1, log_sl, -sl * PHF_SIGMA_INV_SCALE);
  const double lp = -PHF_PIC50_RATE * pic50 + g;
  *out_prior = lp;
  double lik = temperature * a;
  if (temp0_select && temperature == 0.0) lik = 0.0;
  *out_lik = lik;
  *out_lt = lik + lp;
  return outside;
}
/* For every temperature (the select stays), with the arguments of before round 11: what the host tests call.  It is now a wrapper, so those
 * tests run the body above through the byte-offset form of the shared read, (const char*) den_read + 8 den_off[m]: the same address as
 * den_slot[den_off[m]].  One offset per bit of share_mask (32), of which an entry is read only where its bit is set. */
PHF_HD int phf_sl_log_target_sampler(int model, const double* lc, const double* y, const double* w, int n_other, int n_cens,
                                     double n_other_points, double ss_within, double pi_bit, double temperature, int lower_clamp,
                                     const double* th, phf_ktab k_exp, phf_ktab k_log,
                                     unsigned share_mask, const int* den_off, double* den_slot, int slot_stride,
                                     double* out_lik, double* out_prior, double* out_ll1, double* out_lt) {
  int byte_off[32];
  for (int m = 0; m < n_cens && m < 32; ++m) byte_off[m] = ((share_mask >> m) & 1u) ? 8 * den_off[m] : 0;
  return phf_sl_log_target_sampler_t(model, lc, y, w, n_other, n_cens, n_other_points, ss_within, pi_bit, temperature, lower_clamp, 1, th,
                                     k_exp, k_log, share_mask, byte_off, den_slot, den_slot, slot_stride, out_lik, out_prior, out_ll1, out_lt);
}
#undef PHF_DEN_
#undef PHF_CDEN_S_
#undef PHF_SHARE_PUT_
#undef PHF_CDEN_

/* The log-prior part of phf_sl_log_target alone, in exactly its fp64 operations: what a replica-exchange swap (phf_replica_exchange.hip)
 * adds to t l when a state moves to another rung, so that the moved state's log-target is the double the sampler itself would hold. */
PHF_HD double phf_sl_log_prior(int model, const double* th, phf_ktab k_log) {
  const double pic50 = th[0];
  const double hill = (model == 1) ? 1.0 : th[1];
  const double sigma = (model == 1) ? th[1] : th[2];
  const double sl = sigma - PHF_SIGMA_LOC;
  const double log_sl = phf_log_pos_k(sl, k_log);
  const int outside = (pic50 < PHF_PIC50_LOWER)
                      | (sigma <= PHF_SIGMA_LOC)
                      | ((model == 2) & ((hill < 0.0) | (hill > PHF_HILL_UPPER)));
  const double g = phf_fma(PHF_SIGMA_SHAPE_M1, log_sl, -sl * PHF_SIGMA_INV_SCALE);
  const double lp = -PHF_PIC50_RATE * pic50 + g;
  return outside ? -PHF_INF : lp;
}

/* The random numbers of MH iteration t of one chain — ONE Philox4x32-10 block (128 bits) per iteration:
 *   d == 2: z0, z1 from words 0, 1 (phf_normal_u32: piecewise inverse CDF of a 31-bit uniform + a sign bit, |z| <= 6.34),
 *           accept uniform from words 2, 3 (53 bits: numpy's random_sample construction);
 *   d == 3: z0, z1, z2 from words 0, 1, 2, accept uniform (w + 1/2) / 2^32 from word 3.
 * Stateless: a function of (chain, problem, t, seed) alone, so a launch, a quantum or the twin may start anywhere.
 * Returns log(u) (PyHillFit.py:834-835) and the d standard normals in z (PyHillFit.py:831); z[2] = 0 for d == 2.
 * (Rounds 1-3 drew the normals by Box-Muller from 24- / 32-bit fields; the inverse CDF costs a third of the fp64 operations.) */
PHF_HD double phf_mh_draws_of_block(int d, phf_u32x4 b, phf_ktab k_log, double* z) {
  z[0] = phf_normal_u32(b.w[0]);
  z[1] = phf_normal_u32(b.w[1]);
  if (d == 2) {
    z[2] = 0.0;
    const double u = phf_uniform53(b.w[2], b.w[3]);
    const double log_u = phf_log_pos_k(u, k_log);
    return (u < PHF_DBL_MIN) ? -PHF_INF : log_u;       /* u == 0 (probability 2^-53): log 0 = -inf, accept */
  }
  z[2] = phf_normal_u32(b.w[2]);
  return phf_log_pos_k(phf_unit_open32(b.w[3]), k_log);  /* u = (w + 1/2) / 2^32 is never 0 */
}
PHF_HD double phf_mh_draws(int d, uint32_t chain_id, uint32_t problem_id, uint32_t t, uint32_t seed_lo,
                           uint32_t seed_hi, phf_ktab k_log, double* z) {
  const phf_u32x4 b = phf_philox_mh(chain_id, problem_id, t, 0u, seed_lo, seed_hi);
  return phf_mh_draws_of_block(d, b, k_log, z);
}

/* d == 3 only: the same block and the same three normals as phf_mh_draws, and the accept WORD w (u = (w + 1/2) / 2^32) in place of
 * log u — for phf_mh_accept_u32, which decides log u < x without the logarithm for nearly every w. */
PHF_HD uint32_t phf_mh_draws_w3_of_block(phf_u32x4 b, double* z) {
  z[0] = phf_normal_u32(b.w[0]);
  z[1] = phf_normal_u32(b.w[1]);
  z[2] = phf_normal_u32(b.w[2]);
  return b.w[3];
}
PHF_HD uint32_t phf_mh_draws_w3(uint32_t chain_id, uint32_t problem_id, uint32_t t, uint32_t seed_lo, uint32_t seed_hi, double* z) {
  const phf_u32x4 b = phf_philox_mh(chain_id, problem_id, t, 0u, seed_lo, seed_hi);
  return phf_mh_draws_w3_of_block(b, z);
}

/* phf_mh_draws / phf_mh_draws_w3 for the samplers' two-wavefront build: the same block from phf_philox_mh_t_uniform (phf_philox.h: seed_lo_u
 * and seed_hi_w1_u are wave-uniform copies of seed_lo and of seed_hi + 0xBB67AE85), the same conversions.  Device path only. */
PHF_HD double phf_mh_draws_uniform(int d, uint32_t chain_id, uint32_t problem_id, uint32_t t, uint32_t seed_lo, uint32_t seed_hi,
                                   uint32_t seed_lo_u, uint32_t seed_hi_w1_u, phf_ktab k_log, double* z) {
  const phf_u32x4 b = phf_philox_mh_t_uniform(chain_id, problem_id, t, seed_lo, seed_hi, seed_lo_u, seed_hi_w1_u);
  return phf_mh_draws_of_block(d, b, k_log, z);
}
PHF_HD uint32_t phf_mh_draws_w3_uniform(uint32_t chain_id, uint32_t problem_id, uint32_t t, uint32_t seed_lo, uint32_t seed_hi,
                                        uint32_t seed_lo_u, uint32_t seed_hi_w1_u, double* z) {
  const phf_u32x4 b = phf_philox_mh_t_uniform(chain_id, problem_id, t, seed_lo, seed_hi, seed_lo_u, seed_hi_w1_u);
  return phf_mh_draws_w3_of_block(b, z);
}

/* The Metropolis test  phf_log_pos_k(phf_unit_open32(w)) < x  of the d == 3 draws: the same answer for every w and every x (NaN, +-0,
 * +-inf included), with the logarithm evaluated only when some lane of the wavefront has its word next to the threshold.
 * u_w < e^x  <=>  w + 1/2 < T = 2^32 e^x, and the device estimates T in fp32:
 *   t = v_exp_f32(fma((float) x, log2 e, 32)) = T (1 + tau),  |tau| < 4e-6 for x <= 0 (the fp32 roundings of x, of log2 e and of
 *   the argument, and 2^-20 allowed for v_exp_f32: DESIGN.md section 3), so |t - T| < 2^15 words.
 * A word with |w - t| > 2^18 (one in 2^13 per lane and iteration lands inside) is decided by the sign of w - t: the band covers the
 * estimate's error eight times over, plus the fp32 rounding of w and of w - t (<= 256 words), the 1/2 of u_w, and the logarithm's
 * own error E = 3.5e-15 (max over all 2^32 words of |phf_log_pos_k(u_w) - ln u_w|: tests/test_accept_u32_host.py), which moves the
 * exact threshold by E T < 1e-4 words.  Inside the band the logarithm decides.  x > 0: t >= 2^32 (1 - tau), every w outside the
 * band accepts; NaN: every comparison is false, reject; x = -inf: t = 0, w > 2^18 rejects and the rest take the logarithm, which
 * rejects.  The host (the twin does not call this) evaluates the comparison itself. */
#define PHF_ACCEPT_U32_BAND 0x1p18f
PHF_HD int phf_mh_accept_u32(double x, uint32_t w, phf_ktab k_log) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float t = __builtin_amdgcn_exp2f(__builtin_fmaf((float)x, 0x1.715476p+0f, 32.0f));
  const float dw = (float)w - t;
  bool acc = dw < 0.0f;
  if (PHF_ANY_LANE(__builtin_fabsf(dw) <= PHF_ACCEPT_U32_BAND)) {   /* wave-uniform: the logarithm runs only when a lane needs it */
    const bool exact = phf_log_pos_k(phf_unit_open32(w), k_log) < x;
    acc = (__builtin_fabsf(dw) <= PHF_ACCEPT_U32_BAND) ? exact : acc;
  }
  return acc;
#else
  return phf_log_pos_k(phf_unit_open32(w), k_log) < x;
#endif
}

#endif /* PHF_MODEL_H */

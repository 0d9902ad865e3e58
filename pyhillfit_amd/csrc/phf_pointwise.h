/* phf_pointwise.h — the log-likelihood of ONE data point (WAIC's pointwise terms), built from the device helpers of phf_model.h,
 * phf_hier_model.h and phf_math.h; nothing of those headers is changed (the samplers' bit-identity with the twin rests on them).
 *
 *   single-level (python/doseresponse.py:203-248 of the reference, point by point instead of summed):
 *     uncensored (0 < y < 100)  -ln(2 pi)/2 - ln sigma - (y - pred)^2 / (2 sigma^2)
 *     y == 0                    ln Phi((0 - pred)/sigma)
 *     y == 100                  ln Phi((pred - 100)/sigma)
 *   hierarchical (python/PyHillFit.py:113-132): the truncated-normal density on [0, 100]
 *                               -ln(2 pi)/2 - ln sigma - (y - pred)^2 / (2 sigma^2) - ln(Phi((100 - pred)/sigma) - Phi((0 - pred)/sigma))
 *   sigma <= 1e-3 (the floor of both likelihoods' supports) gives -inf.
 *
 * The per-vector part (ln IC50, 1/sigma, ln sigma) is computed once per parameter vector by the caller (phf_pw_sigma_terms) and
 * shared by all its points.  Tables: PHF_MATH_TABLES_TO_LDS() and, single-level, PHF_LOGPHI_TABLE_TO_LDS(); hierarchical,
 * PHF_ERFC_TABLE_TO_LDS(). */
#ifndef PHF_POINTWISE_H
#define PHF_POINTWISE_H

#include "phf_hier_model.h"
#include "phf_math.h"
#include "phf_model.h"

#define PHF_HALF_LN_2PI 0x1.d67f1c864beb4p-1    /* ln(2 pi) / 2 */

#define PHF_PW_UNCENSORED 0                     /* single-level point tags (phf_pointwise_points.tag) */
#define PHF_PW_ZERO 1
#define PHF_PW_HUNDRED 2

typedef struct {
  double inv_s;       /* 1/sigma */
  double base;        /* -ln(2 pi)/2 - ln sigma, or -inf at or below the sigma floor */
} phf_pw_sigma;

PHF_HD phf_pw_sigma phf_pw_sigma_terms(double sigma, phf_ktab k_log) {
  phf_pw_sigma t;
  t.inv_s = phf_rcp(sigma);
  const double b = -PHF_HALF_LN_2PI - phf_log_pos_k(sigma, k_log);
  t.base = (sigma <= PHF_SIGMA_FLOOR) ? -PHF_INF : b;
  return t;
}

/* the Hill curve in percent: 100 (1 - 1/(1 + exp(hill (ln c - ln IC50)))), as the targets compute it (model 1: hill = 1) */
PHF_HD double phf_pw_pred(int model, double ln_conc, double hill, double ln_ic50, phf_ktab k_exp) {
  return phf_hill_percent(phf_rcp(phf_hill_den(model, ln_conc, hill, ln_ic50, k_exp)), k_exp);
}

/* single-level point of tag `tag` (0 | 1 | 2) */
PHF_HD double phf_pw_sl_point(int model, double ln_conc, double y, int tag, double hill, double ln_ic50, phf_pw_sigma sg,
                              phf_ktab k_exp) {
  const double pred = phf_pw_pred(model, ln_conc, hill, ln_ic50, k_exp);
  double l;
  if (tag == PHF_PW_UNCENSORED) {
    const double r = (y - pred) * sg.inv_s;
    l = phf_fma(-0.5 * r, r, sg.base);
  } else {
    const double z = phf_censored_z(pred, y, sg.inv_s);
    l = phf_log_ndtr_tab(z, -z * PHF_INV_SQRT2);
  }
  return sg.base == -PHF_INF ? -PHF_INF : l;
}

/* hierarchical point of an experiment with (pIC50, Hill) = ln_ic50, hill */
PHF_HD double phf_pw_hier_point(double ln_conc, double y, double hill, double ln_ic50, phf_pw_sigma sg, phf_ktab k_exp,
                                phf_ktab k_log) {
  const double pred = phf_pw_pred(2, ln_conc, hill, ln_ic50, k_exp);
  const double r = (y - pred) * sg.inv_s;
  const double trunc = phf_log_fast_k(phf_trunc_mass(pred, sg.inv_s, k_exp), k_log);
  return phf_fma(-0.5 * r, r, sg.base) - trunc;
}

#endif /* PHF_POINTWISE_H */

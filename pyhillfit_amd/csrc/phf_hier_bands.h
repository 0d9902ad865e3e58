/* phf_hier_bands.h — dose-response bands of the hierarchical model ("Hierarchical bands"): per saved draw
 * (alpha, beta, mu, s) = columns 0..3 of a hierarchical row, the Hill curve of
 *
 *   the inferred underlying effect     Hill = alpha, pIC50 = mu (no random number), and of
 *   a predicted future experiment      Hill* ~ log-logistic(scale alpha, shape beta), pIC50* ~ logistic(mu, s), by inversion:
 *                                        Hill*  = alpha exp(logit(u_H) / beta)      (a plain IEEE division: the same double on
 *                                        pIC50* = mu + s logit(u_P)                  host and device; not phf_rcp / phf_div)
 *                                      logit(u) = phf_log(u) - phf_log(1 - u).
 *
 * Uniforms: two 52-bit uniforms centred in their cells, u = (k + 1/2) 2^-52 with k = (w_a >> 6) 2^26 + (w_b >> 6): u and 1 - u are
 * both exact doubles in [2^-53, 1 - 2^-53], so |logit u| <= 36.8, no draw is infinite by its uniform, and logit(1 - u) = -logit(u)
 * bit for bit.  The Hill uniform takes words 0 and 1 of the block, the pIC50 uniform words 2 and 3.
 *
 * Random stream: ONE Philox block (the samplers' rounds) per draw,
 *   counter = (chain_id_base + chain, problem_id, global row index, PHF_BAND_DOMAIN), key = seed;
 * word 3 = 0xC0000000 is used by nothing else: the samplers put small block indices there, the posterior predictive checks
 * 0x80000000 | b with b small, replica exchange 0x40000000.  The row index is global (first_row + r): the draw does not depend on
 * how the rows are cut into calls.
 *
 * Curve value: phf_pw_pred(2, ln_dose, Hill, ln10 (6 - pIC50)) in percent, as the single-level curve bands compute it.
 * A draw whose alpha, beta, mu or s is not finite, or with alpha <= 0 or beta <= 0, gives NaN for both kinds; s <= 0 gives NaN for
 * the future experiment.  Nothing else is special-cased: a beta small enough that exp(logit/beta) overflows gives Hill* = inf
 * (or 0), whose curve is 0 or 100 percent away from the IC50 and, AT a dose equal to the IC50, the value of the curve arithmetic
 * for the argument inf * 0 = NaN — the cap min(arg, 40) of phf_hill_den drops the NaN, so that value is 100 (1 - 1/(1 + e^40)).
 *
 * Tables on the device: PHF_MATH_TABLES_TO_LDS() (exp2 and log). */
#ifndef PHF_HIER_BANDS_H
#define PHF_HIER_BANDS_H

#include "phf_philox.h"
#include "phf_pointwise.h"

#define PHF_BAND_DOMAIN 0xC0000000u             /* counter word 3 of every band draw */
#define PHF_BAND_UNDERLYING 0                   /* kinds */
#define PHF_BAND_FUTURE 1

/* (k + 1/2) 2^-52, k = (wa >> 6) 2^26 + (wb >> 6): every step is exact (k + 1/2 has 53 significant bits) */
PHF_HD double phf_band_uniform(uint32_t wa, uint32_t wb) {
  return ((double)(wa >> 6) * 67108864.0 + (double)(wb >> 6) + 0.5) * 0x1p-52;
}

/* ln(u / (1 - u)) for u of phf_band_uniform: both arguments are positive normal doubles below 1, where phf_log is phf_log_pos_k */
PHF_HD double phf_band_logit_k(double u, phf_ktab k_log) { return phf_log_pos_k(u, k_log) - phf_log_pos_k(1.0 - u, k_log); }

PHF_HD double phf_band_logit(double u) {
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  return phf_band_logit_k(u, k_log);
}

/* are (alpha, beta, mu, s) the parameters of a draw of kind `kind`? */
PHF_HD int phf_band_valid(int kind, double alpha, double beta, double mu, double s) {
  const int finite = __builtin_isfinite(alpha) && __builtin_isfinite(beta) && __builtin_isfinite(mu) && __builtin_isfinite(s);
  return finite && alpha > 0.0 && beta > 0.0 && (kind == PHF_BAND_UNDERLYING || s > 0.0);
}

/* the log-logistic(scale alpha, shape beta) quantile of u: alpha exp(logit(u) / beta); the argument of exp is never NaN for valid
 * parameters, where phf_exp_fast_k is phf_exp */
PHF_HD double phf_band_hill_k(double alpha, double beta, double u, phf_ktab k_exp, phf_ktab k_log) {
  return alpha * phf_exp_fast_k(phf_band_logit_k(u, k_log) / beta, k_exp);
}

/* the logistic(mu, s) quantile of u: mu + s logit(u) */
PHF_HD double phf_band_pic50_k(double mu, double s, double u, phf_ktab k_log) { return mu + s * phf_band_logit_k(u, k_log); }

/* (Hill*, pIC50*) of the future experiment of one draw; NaN, NaN for parameters that are not valid */
PHF_HD void phf_band_future_k(double alpha, double beta, double mu, double s, uint32_t chain_id, uint32_t problem_id, uint32_t row,
                              uint32_t k0, uint32_t k1, phf_ktab k_exp, phf_ktab k_log, double* hill, double* pic50) {
  if (!phf_band_valid(PHF_BAND_FUTURE, alpha, beta, mu, s)) {
    *hill = PHF_NAN;
    *pic50 = PHF_NAN;
    return;
  }
  const phf_u32x4 w = phf_philox_mh(chain_id, problem_id, row, PHF_BAND_DOMAIN, k0, k1);
  *hill = phf_band_hill_k(alpha, beta, phf_band_uniform(w.w[0], w.w[1]), k_exp, k_log);
  *pic50 = phf_band_pic50_k(mu, s, phf_band_uniform(w.w[2], w.w[3]), k_log);
}

PHF_HD void phf_band_future(double alpha, double beta, double mu, double s, uint32_t chain_id, uint32_t problem_id, uint32_t row,
                            uint32_t k0, uint32_t k1, double* hill, double* pic50) {
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  phf_band_future_k(alpha, beta, mu, s, chain_id, problem_id, row, k0, k1, k_exp, k_log, hill, pic50);
}

/* percent block at ln_dose of the curve (Hill, pIC50); NaN in gives NaN out */
PHF_HD double phf_band_curve_k(double ln_dose, double hill, double pic50, phf_ktab k_exp) {
  if (hill != hill || pic50 != pic50) return PHF_NAN;
  return phf_pw_pred(2, ln_dose, hill, PHF_LN10 * (6.0 - pic50), k_exp);
}

/* the value a band slot bins: the curve of kind `kind` of the draw (alpha, beta, mu, s) at ln_dose */
PHF_HD double phf_band_value_k(int kind, double ln_dose, double alpha, double beta, double mu, double s, uint32_t chain_id,
                               uint32_t problem_id, uint32_t row, uint32_t k0, uint32_t k1, phf_ktab k_exp, phf_ktab k_log) {
  if (kind == PHF_BAND_UNDERLYING)
    return phf_band_valid(PHF_BAND_UNDERLYING, alpha, beta, mu, s) ? phf_band_curve_k(ln_dose, alpha, mu, k_exp) : PHF_NAN;
  double hill, pic50;
  phf_band_future_k(alpha, beta, mu, s, chain_id, problem_id, row, k0, k1, k_exp, k_log, &hill, &pic50);
  return phf_band_curve_k(ln_dose, hill, pic50, k_exp);
}

PHF_HD double phf_band_value(int kind, double ln_dose, double alpha, double beta, double mu, double s, uint32_t chain_id,
                             uint32_t problem_id, uint32_t row, uint32_t k0, uint32_t k1) {
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  return phf_band_value_k(kind, ln_dose, alpha, beta, mu, s, chain_id, problem_id, row, k0, k1, k_exp, k_log);
}

#endif /* PHF_HIER_BANDS_H */

/* phf_ppc.h — posterior predictive checks ("Posterior predictive checks"): the replicated response of one data point,
 * its log-likelihood at a given prediction, the predictive PIT of an observed point, and the inverse normal CDF the hierarchical
 * replicate needs.  Built from phf_pointwise.h, phf_model.h, phf_hier_model.h and phf_math.h; nothing of those headers is changed.
 *
 *   single-level (a censored normal):  y_rep = clamp(pred + sigma z, 0, 100), z = phf_normal_u32(word) (|z| <= 6.34: the generator's
 *                                      cut, so P(y_rep = 0) = Phi(-pred/sigma) only down to Phi(-6.34) = 1.2e-10)
 *   hierarchical (the truncated normal on [0, 100]):
 *                                      y_rep = clamp(pred + sigma ndtri(Phi(a) + u (Phi(b) - Phi(a))), 0, 100),
 *                                      a = -pred/sigma <= 0 <= b = (100 - pred)/sigma, u = phf_unit_open32(word)
 *
 * Random stream: one Philox block (the samplers' rounds) per (draw, 4 points),
 *   counter = (chain_id_base + chain, problem_id, row, PHF_PPC_DOMAIN | point_block), key = seed;
 * the samplers' draws use word 3 for their small block indices only, so the top bit keeps the two streams disjoint. */
#ifndef PHF_PPC_H
#define PHF_PPC_H

#include "phf_pointwise.h"

#define PHF_PPC_DOMAIN 0x80000000u              /* counter word 3 of every posterior-predictive block */
#define PHF_PPC_STATS 5                         /* deviance, mean, sd, zeros, hundreds */
#define PHF_PPC_PIT_LO 0.005                    /* a point is flagged when its PIT is outside [lo, hi] */
#define PHF_PPC_PIT_HI 0.995

/* Phi^-1(p) in fp64: Wichura's AS241 (PPND16, Applied Statistics 37, 1988), relative error about 1e-16.
 * p <= 0 -> -inf, p >= 1 -> +inf, NaN -> NaN. */
PHF_HD double phf_ndtri(double p) {
  if (!(p > 0.0)) return p == 0.0 || p < 0.0 ? -PHF_INF : p;
  if (p >= 1.0) return PHF_INF;
  const double q = p - 0.5;
  if ((q < 0.0 ? -q : q) <= 0.425) {
    const double r = 0.180625 - q * q;
    const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r
                             + 4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r
                          + 1.3314166789178437745e+2) * r + 3.3871328727963666080e+0);
    const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r
                             + 2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r
                          + 4.2313330701600911252e+1) * r + 1.0);
    return phf_div(q * num, den);
  }
  double r = phf_sqrt_pos(-phf_log(q < 0.0 ? p : 1.0 - p));       /* 1 - p is exact for p >= 1/2 */
  double x;
  if (r <= 5.0) {
    r -= 1.6;
    const double num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r
                             + 1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r
                          + 4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
    const double den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r
                             + 1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r
                          + 2.05319162663775882187e+0) * r + 1.0);
    x = phf_div(num, den);
  } else {
    r -= 5.0;
    const double num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r
                             + 2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r
                          + 5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
    const double den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r
                             + 7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r
                          + 5.99832206555887937690e-1) * r + 1.0);
    x = phf_div(num, den);
  }
  return q < 0.0 ? -x : x;
}

PHF_HD double phf_ppc_clamp(double y) { return y < 0.0 ? 0.0 : (y > 100.0 ? 100.0 : y); }

/* single-level replicate of a point with prediction pred */
PHF_HD double phf_ppc_rep_sl(double pred, double sigma, uint32_t word) {
  return phf_ppc_clamp(pred + sigma * phf_normal_u32(word));
}

/* hierarchical replicate: the truncated normal on [0, 100] by inversion */
PHF_HD double phf_ppc_rep_hier(double pred, double sigma, double inv_s, uint32_t word) {
  const double pa = phf_ndtr(-pred * inv_s), pb = phf_ndtr((100.0 - pred) * inv_s);
  const double p = pa + phf_unit_open32(word) * (pb - pa);
  return phf_ppc_clamp(pred + sigma * phf_ndtri(p));
}

/* the censoring tag of a single-level response in [0, 100] (phf_pointwise.h) */
PHF_HD int phf_ppc_sl_tag(double y) { return y == 0.0 ? PHF_PW_ZERO : (y == 100.0 ? PHF_PW_HUNDRED : PHF_PW_UNCENSORED); }

/* phf_pw_sl_point with the prediction given: the same operations (the observed point's value is WAIC's l) */
PHF_HD double phf_ppc_sl_point_at(double pred, double y, int tag, phf_pw_sigma sg) {
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

/* phf_pw_hier_point with the prediction and ln(truncation mass) given */
PHF_HD double phf_ppc_hier_point_at(double pred, double y, double ln_mass, phf_pw_sigma sg) {
  const double r = (y - pred) * sg.inv_s;
  return phf_fma(-0.5 * r, r, sg.base) - ln_mass;
}

/* P(y_rep < y | theta) + P(y_rep = y | theta) / 2 of an observed single-level point of tag `tag` */
PHF_HD double phf_ppc_pit_sl(double pred, double y, int tag, double inv_s) {
  if (tag == PHF_PW_ZERO) return 0.5 * phf_ndtr(-pred * inv_s);
  if (tag == PHF_PW_HUNDRED) return 1.0 - 0.5 * phf_ndtr((pred - 100.0) * inv_s);
  return phf_ndtr((y - pred) * inv_s);
}

/* the truncated-normal CDF at y (no point masses) */
PHF_HD double phf_ppc_pit_hier(double pred, double y, double inv_s, phf_ktab k_exp) {
  const double pa = phf_ndtr(-pred * inv_s);
  const double v = (phf_ndtr((y - pred) * inv_s) - pa) * phf_rcp(phf_trunc_mass(pred, inv_s, k_exp));
  return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
}

#endif /* PHF_PPC_H */

/* phf_design.h — expected information gain of ONE further measurement at a candidate dose ("Next dose"): the mutual
 * information between the new response y and the parameters under the current posterior (Lindley 1956; Chaloner & Verdinelli 1995),
 *
 *   EIG(d) = H[ pbar(y | d) ] - E_theta H[ p(y | theta, d) ],      pbar(y | d) = E_theta p(y | theta, d),
 *
 * of a response RECORDED TO A RESOLUTION of 100/K % block.  Single-level models: a draw is (pIC50, sigma) with Hill = 1 (model 1) or
 * (pIC50, Hill, sigma) (model 2), its prediction at the dose is phf_pw_pred, and the new response is the single-level likelihood's
 * censored normal, here with K + 2 categories:
 *
 *   category 0            the point mass at 0,    Phi((0 - pred)/sigma)
 *   category 1 + k, k < K the bin (e_k, e_k+1) of (0, 100),  e_k = k 100/K  (an exact double for every K allowed)
 *   category K + 1        the point mass at 100,  1 - Phi((100 - pred)/sigma)
 *
 * Masses.  The tail at an edge is the SMALL one on the edge's side of pred, t(e) = erfc(|e - pred| / (sigma sqrt 2)) / 2 from the
 * table of phf_math.h (absolute accuracy 3.6e-17, defined as 0 from 6 sqrt 2 sigma on).  pred is in [0, 100], so the point masses are
 * t(0) and t(100), and a bin's mass is
 *   t(e_k+1) - t(e_k)          e_k+1 <= pred     (lower tails)
 *   t(e_k) - t(e_k+1)          e_k >= pred       (upper tails)
 *   (1 - t(e_k)) - t(e_k+1)    the bin holding pred,
 * never a difference of numbers near 1; clamped at 0 from below (the table's error can turn a difference of two tails of 1e-17
 * negative).  The K + 2 masses telescope to 1.  -p log p is 0 for p below the smallest normal double.
 *
 * Per draw and dose: the masses, h_fine = -SUM p log p over the K + 2 categories, and h_coarse, the same over the partition that
 * merges the bins 2 j and 2 j + 1 (the point masses stay apart): the K/2-bin value comes out of the same pass.
 * A draw with sigma <= PHF_SIGMA_FLOOR or with a parameter that is not finite is skipped and counted.
 *
 * Order of operations, the same on host and device (the device accumulators are bit-identical to the host build of this header):
 *   lanes   64 of them; lane t owns the K/64 adjacent bins t K/64 .. (t + 1) K/64 - 1 (an even number: the merged pairs are
 *           lane-local) and evaluates the K/64 + 1 edge tails around them; lane 0 also owns the point mass at 0, lane 63 that at 100.
 *   slots   the chains are dealt to NS accumulator slots (NS even), chain c to slot c mod NS, so the chains of a slot share the
 *           chain's parity c & 1; a slot's draws are the used rows in row order, and within a row its chains in ascending order.
 *   sums    per (problem, dose, slot) and lane, every accumulator is the plain left-to-right sum acc = acc + term over the slot's
 *           draws in that order, started from the accumulator's stored value: however the calls cut the rows, the same additions
 *           happen in the same order.  The lanes' entropy sums are kept apart (64 + 64 doubles); nothing is merged across lanes or
 *           slots on the device, and there are no atomics.
 * The accumulator of one (problem, dose, slot), PHF_DS_ACC_DOUBLES(K) doubles:
 *   [0]                 SUM mass at 0          [1 .. K]        SUM bin masses          [K + 1]   SUM mass at 100
 *   [K + 2 .. K + 65]   per lane SUM h_fine    [K + 66 .. K + 129]  per lane SUM h_coarse
 *   [K + 130]           draws used             [K + 131]       draws skipped           (counts, exact in a double)
 *
 * Tables on the device: PHF_MATH_TABLES_TO_LDS() and PHF_ERFC_TABLE_TO_LDS(). */
#ifndef PHF_DESIGN_H
#define PHF_DESIGN_H

#include <stddef.h>

#include "phf_pointwise.h"

#define PHF_DS_LANES 64
#define PHF_DS_DEFAULT_BINS 256
#define PHF_DS_MAX_NB 16                        /* bins of a lane at K = 1024 */
#define PHF_DS_MAX_SLOTS 64
#define PHF_DS_ACC_DOUBLES(K) ((K) + 2 + 2 * PHF_DS_LANES + 2)
#define PHF_DS_OFF_HF(K) ((K) + 2)
#define PHF_DS_OFF_HC(K) ((K) + 2 + PHF_DS_LANES)
#define PHF_DS_OFF_USED(K) ((K) + 2 + 2 * PHF_DS_LANES)
#define PHF_DS_OFF_SKIPPED(K) ((K) + 3 + 2 * PHF_DS_LANES)

PHF_HD int phf_ds_bins_ok(int K) { return K == 128 || K == 256 || K == 512 || K == 1024; }
PHF_HD int phf_ds_slots_ok(int NS) { return NS >= 2 && NS <= PHF_DS_MAX_SLOTS && !(NS & 1); }

PHF_HD int phf_ds_finite(double x) { return __builtin_fabs(x) < PHF_INF; }      /* false for NaN */

/* is the draw used?  th = (pIC50, sigma) or (pIC50, Hill, sigma) */
PHF_HD int phf_ds_draw_ok(int model, double pic50, double hill, double sigma) {
  return phf_ds_finite(pic50) & phf_ds_finite(sigma) & (sigma > PHF_SIGMA_FLOOR) & ((model == 1) | phf_ds_finite(hill));
}

/* the draw's two numbers at a dose: the prediction and 1 / (sigma sqrt 2) */
PHF_HD void phf_ds_draw_terms(int model, double ln_dose, double pic50, double hill, double sigma, phf_ktab k_exp, double* pred,
                              double* scale) {
  const double ln_ic50 = PHF_LN10 * (6.0 - pic50);
  *pred = phf_pw_pred(model, ln_dose, (model == 1) ? 1.0 : hill, ln_ic50, k_exp);
  *scale = phf_rcp(sigma) * PHF_INV_SQRT2;
}

PHF_HD double phf_ds_entr(double p, phf_ktab k_log) {
  const double l = phf_log_pos_k(p, k_log);
  return (p < PHF_DBL_MIN) ? 0.0 : -(p * l);
}

/* the small tail at edge e */
PHF_HD double phf_ds_tail(double e, double pred, double scale) { return 0.5 * phf_erfc_tab(__builtin_fabs(e - pred) * scale); }

/* the mass of the bin (lo, hi) from the tails at its edges */
PHF_HD double phf_ds_mass(double lo, double hi, double t_lo, double t_hi, double pred) {
  const double lower = t_hi - t_lo, upper = t_lo - t_hi, both = (1.0 - t_lo) - t_hi;
  return __builtin_fmax((hi <= pred) ? lower : ((lo >= pred) ? upper : both), 0.0);
}

/* the kernel walks a lane's bins a pair at a time and keeps the scheduler from interleaving the pairs: left to itself it starts
 * all K/64 + 1 table polynomials at once, twelve coefficients each, and spills at K = 1024 */
#if defined(__HIP_DEVICE_COMPILE__)
#define PHF_DS_PAIR_DONE() __builtin_amdgcn_sched_barrier(0)
#else
#define PHF_DS_PAIR_DONE() do { } while (0)
#endif

/* lane `lane`'s terms of one draw, ADDED to its sums: m[NB] the masses of its bins, *pt its point mass (lane 0: at 0; lane 63: at
 * 100; else + 0), *hf and *hc its shares of h_fine and h_coarse — the draw's share is formed first (point mass, then the bins in
 * ascending order), then added.  NB = K / 64 (2, 4, 8 or 16; a constant where the kernel calls this). */
PHF_HD void phf_ds_lane_add(int lane, int NB, double pred, double scale, phf_ktab k_log, double* m, double* pt, double* hf,
                            double* hc) {
  const double w = 100.0 / (double)(NB * PHF_DS_LANES);         /* the bin width: exact, and so is every edge k w */
  const int k0 = lane * NB;
  const double t_first = phf_ds_tail((double)k0 * w, pred, scale), t_last = phf_ds_tail((double)(k0 + NB) * w, pred, scale);
  const double p = (lane == 0) ? t_first : ((lane == PHF_DS_LANES - 1) ? t_last : 0.0);
  double f = phf_ds_entr(p, k_log), c = f, t_lo = t_first;
  PHF_DS_PAIR_DONE();
  PHF_UNROLL
  for (int b = 0; b < NB; b += 2) {
    const double e0 = (double)(k0 + b) * w, e1 = (double)(k0 + b + 1) * w, e2 = (double)(k0 + b + 2) * w;
    const double t_mid = phf_ds_tail(e1, pred, scale), t_hi = (b + 2 == NB) ? t_last : phf_ds_tail(e2, pred, scale);
    const double v0 = phf_ds_mass(e0, e1, t_lo, t_mid, pred), v1 = phf_ds_mass(e1, e2, t_mid, t_hi, pred);
    f += phf_ds_entr(v0, k_log);
    f += phf_ds_entr(v1, k_log);
    c += phf_ds_entr(v0 + v1, k_log);
    m[b] += v0;
    m[b + 1] += v1;
    t_lo = t_hi;
    PHF_DS_PAIR_DONE();
  }
  *pt += p;
  *hf += f;
  *hc += c;
}

/* the number of rows r in [first_row, first_row + num_rows) with r mod every == 0 */
PHF_HD int64_t phf_ds_rows_used(int64_t first_row, int64_t num_rows, int every) {
  const int64_t end = first_row + num_rows;
  return (end + every - 1) / every - (first_row + every - 1) / every;
}

#if !defined(__HIP_DEVICE_COMPILE__)
/* host form of the kernel: the rows [num_rows][Q][cols][C] of a call into acc [Q][G][NS][PHF_DS_ACC_DOUBLES(K)], ln_doses [Q][G] */
static void phf_ds_accumulate_host(int model, int K, const double* rows, int64_t num_rows, int Q, int cols, int C, int64_t first_row,
                                   int every, const double* ln_doses, int G, int NS, double* acc) {
  PHF_KFETCH_V(k_exp, phf_k_exp, PHF_K_EXP_N);
  PHF_KFETCH_V(k_log, phf_k_log, PHF_K_LOG_N);
  const int NB = K / PHF_DS_LANES;
  const int64_t used = phf_ds_rows_used(first_row, num_rows, every), r0 = (every - first_row % every) % every;
  for (int q = 0; q < Q; ++q)
    for (int g = 0; g < G; ++g)
      for (int s = 0; s < NS; ++s) {
        double* a = acc + (((size_t)q * G + g) * NS + s) * PHF_DS_ACC_DOUBLES(K);
        for (int64_t u = 0; u < used; ++u)
          for (int c = s; c < C; c += NS) {
            const double* x = rows + (((size_t)(r0 + u * every) * Q + q) * cols) * (size_t)C + c;
            const double pic50 = x[0], hill = (model == 1) ? 1.0 : x[C], sigma = x[(size_t)model * C];
            if (!phf_ds_draw_ok(model, pic50, hill, sigma)) {
              a[PHF_DS_OFF_SKIPPED(K)] += 1.0;
              continue;
            }
            a[PHF_DS_OFF_USED(K)] += 1.0;
            double pred, scale, none = 0.0;
            phf_ds_draw_terms(model, ln_doses[(size_t)q * G + g], pic50, hill, sigma, k_exp, &pred, &scale);
            for (int lane = 0; lane < PHF_DS_LANES; ++lane) {
              double* pt = (lane == 0) ? &a[0] : ((lane == PHF_DS_LANES - 1) ? &a[K + 1] : &none);
              phf_ds_lane_add(lane, NB, pred, scale, k_log, &a[1 + lane * NB], pt, &a[PHF_DS_OFF_HF(K) + lane], &a[PHF_DS_OFF_HC(K) + lane]);
            }
          }
      }
}
#endif

#endif /* PHF_DESIGN_H */

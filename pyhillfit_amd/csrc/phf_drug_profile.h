/* phf_drug_profile.h — the per-drug multi-channel block profile ("Drug profile"): what one post-burn-in draw of all the
 * channels of a drug says at a concentration, as host/device code: gcc builds the tests' ground truth from this text, hipcc the kernels
 * of phf_drug_profile.hip.
 *
 * A drug has K channel places, in the data file's channel order; map[drug][k] is the problem whose rows hold channel k's fit, or -1
 * when that channel was not loaded.  The channels' posteriors are independent, so row r, chain c of every loaded channel side by side
 * is one draw of the drug's joint posterior.  At dose j of the drug (ln c_j, natural log of uM):
 *   block_k = phf_pw_pred(model, ln c_j, Hill_k, ln10 (6 - pIC50_k))     percent block of channel k (model 1: Hill = 1);
 *   net     = SUM_k w_k block_k     over the loaded channels in channel order, plain multiplies and adds from 0 (no fma);
 *   dominant = the least k with the largest block_k.
 * A draw in which a loaded channel's pIC50 or Hill is not finite has no net and no dominant channel: it is counted apart.
 * A slot is (drug, dose, component): component k < K is block_k, component K the net block.  The slots of a channel that was not
 * loaded, and everything of a dose whose ln c is not finite (a drug with fewer doses than the others), are never fed. */
#ifndef PHF_DRUG_PROFILE_H
#define PHF_DRUG_PROFILE_H

#include <stddef.h>

#include "phf_pointwise.h"

#define PHF_DP_MAX_CHANNELS 16   /* K: the tally kernel keeps a drug's 2 (K + 3) counters in the lanes of a wavefront */
#define PHF_DP_MAX_DOSES 16      /* D */
#define PHF_DP_TALLIES(K) ((K) + 3)   /* per (drug, dose, chain parity): dominant[K], net > 0, draws used, draws skipped */

/* ---- the default weights: repolarising (outward) currents +1, depolarising (inward) currents -1, any other name 0.  A convention
 * after the "Bnet" of Mistry (2018), not a measurement. */
PHF_HD int phf_dp_same_name(const char* a, const char* b) {
  while (*a && *a == *b) { ++a; ++b; }
  return *a == *b;
}

PHF_HD double phf_dp_default_weight(const char* channel) {
  const char* const outward[] = {"hERG", "KvLQT1_mink", "Kv4.3", "Kir2.1"};
  const char* const inward[] = {"Nav1.5-peak", "Nav1.5-late", "Cav1.2"};
  for (int i = 0; i < 4; ++i)
    if (phf_dp_same_name(channel, outward[i])) return 1.0;
  for (int i = 0; i < 3; ++i)
    if (phf_dp_same_name(channel, inward[i])) return -1.0;
  return 0.0;
}

/* ---- the values ------------------------------------------------------------------------------------------------------------------- */
typedef struct {
  const double* rows;      /* [n][Q][stride][C]: column 0 pIC50, column 1 Hill (model 2) */
  const int32_t* map;      /* [drugs][K] */
  const double* weight;    /* [K] */
  const double* ln_dose;   /* [drugs][D] */
  int Q, stride, C, K, D;
} phf_dp_view;

/* the problem of (drug, k); anything outside [0, Q) is "not loaded" */
PHF_HD int phf_dp_problem(const phf_dp_view* v, int drug, int k) {
  const int p = v->map[(size_t)drug * v->K + k];
  return p >= 0 && p < v->Q ? p : -1;
}

/* percent block of problem p's draw (row r, chain c) at ln_c; NaN when its pIC50 or Hill is not finite */
PHF_HD double phf_dp_block(int model, const phf_dp_view* v, int p, double ln_c, int64_t r, int c, phf_ktab k_exp) {
  const double* x = v->rows + ((size_t)r * v->Q + p) * v->stride * (size_t)v->C + c;
  const double pic50 = x[0], hill = model == 2 ? x[v->C] : 1.0;
  if (!__builtin_isfinite(pic50) || !__builtin_isfinite(hill)) return PHF_NAN;
  return phf_pw_pred(model, ln_c, hill, PHF_LN10 * (6.0 - pic50), k_exp);
}

/* the decision rules of one draw of `drug` at dose j: 1 and (*net, *dominant) when every loaded channel's block is finite, else 0 and
 * (NaN, -1); a drug with no loaded channel has net 0 and no dominant channel (-1) */
PHF_HD int phf_dp_draw(int model, const phf_dp_view* v, int drug, int j, int64_t r, int c, phf_ktab k_exp, double* net, int* dominant) {
  const double ln_c = v->ln_dose[(size_t)drug * v->D + j];
  double sum = 0.0, best = -PHF_INF;
  int arg = -1, ok = 1;
  for (int k = 0; k < v->K; ++k) {
    const int p = phf_dp_problem(v, drug, k);
    if (p < 0) continue;
    const double b = phf_dp_block(model, v, p, ln_c, r, c, k_exp);
    if (!__builtin_isfinite(b)) ok = 0;
    const double term = v->weight[k] * b;
    sum = sum + term;
    if (b > best) { best = b; arg = k; }       /* strictly greater: a tie stays with the lower k */
  }
  *net = ok ? sum : PHF_NAN;
  *dominant = ok ? arg : -1;
  return ok;
}

/* does the drug have a dose j?  A drug with fewer doses than D has NaN in the places it does not use */
PHF_HD int phf_dp_dose_live(const phf_dp_view* v, int drug, int j) { return __builtin_isfinite(v->ln_dose[(size_t)drug * v->D + j]); }

/* is slot (drug, dose j, component) fed at all?  A dose the drug does not have and the block of a channel that was not loaded are not */
PHF_HD int phf_dp_slot_live(const phf_dp_view* v, int drug, int j, int comp) {
  return phf_dp_dose_live(v, drug, j) && (comp >= v->K || phf_dp_problem(v, drug, comp) >= 0);
}

/* the value of a live slot (drug, dose j, component comp) in draw (r, c) */
PHF_HD double phf_dp_slot_value(int model, const phf_dp_view* v, int drug, int j, int comp, int64_t r, int c, phf_ktab k_exp) {
  if (comp < v->K)
    return phf_dp_block(model, v, phf_dp_problem(v, drug, comp), v->ln_dose[(size_t)drug * v->D + j], r, c, k_exp);
  double net;
  int dominant;
  (void)phf_dp_draw(model, v, drug, j, r, c, k_exp, &net, &dominant);
  return net;
}

/* the tally a draw adds one to, besides "used" or "skipped": t in [0, K) dominant == t, K net > 0 */
PHF_HD int phf_dp_tally_hit(int t, int K, int ok, double net, int dominant) {
  if (t < K) return ok && dominant == t;
  if (t == K) return ok && net > 0.0;
  return t == K + 1 ? ok : !ok;
}

#endif /* PHF_DRUG_PROFILE_H */

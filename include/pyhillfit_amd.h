/* pyhillfit_amd.h — C ABI of the MI355X-native Metropolis-Hastings engine for PyHillFit's sampling step.
 *
 * The reference (mirams/PyHillFit) has no FFI: its hot path is a Python loop.  These entry points are
 * what a ctypes binding inside the reference would call instead of that loop; each cites the reference
 * code it replaces (file:line into the reference repository).  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain C, no C++/torch types; every pointer marked "device" is a HIP device pointer owned by the caller
 *     (the Python host passes torch.Tensor.data_ptr()); `stream` is a hipStream_t passed as void* (NULL = default)
 *   - every function returns PHF_OK (0) or a negative error code and never throws or exits; the message is
 *     available from phf_last_error() (thread-local).  The reference's sys.exit() on NaN
 *     (python/PyHillFit.py:126-131,188-191) becomes: NaN proposals are rejected, nothing aborts.
 *   - launches are asynchronous on `stream`; the library allocates nothing and keeps no global state, so one
 *     host thread/process per GPU may call it concurrently.
 *   - all arithmetic is IEEE fp64.  Chain-major arrays are struct-of-arrays with the chain index fastest
 *     ("[f][chain]"), so that the 64 lanes of a wavefront touch 512 contiguous bytes.
 *   - MEMORY KIND: state, moments and the queue workspace must be ordinary coarse-grained device memory (hipMalloc /
 *     torch.empty(device="cuda")): the hierarchical kernels accumulate moments with hardware fp64 atomics (global_atomic_add_f64
 *     without return) and the queued launch hands a block's state over with agent-scope release/acquire — on fine-grained, managed
 *     or host-pinned memory neither is guaranteed to take effect.  The advance calls CHECK these three (hipPointerGetAttributes:
 *     host, managed and fine-grained allocations are refused with PHF_ERR_INVALID_ARGUMENT; an address the runtime cannot classify
 *     passes; the verdicts of the calling thread's last 8 (address, device) pairs are remembered and forgotten at every *_init, so a
 *     buffer re-allocated as another kind at the same address must not be swapped in between two advances of ONE sampler).  rows
 *     and sums are written with plain stores and read by nobody inside a launch: any device-accessible memory works, and they are
 *     not checked.
 */
#ifndef PYHILLFIT_AMD_H
#define PYHILLFIT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHF_ABI_VERSION 7

enum {
  PHF_OK = 0,
  PHF_ERR_INVALID_ARGUMENT = -1,
  PHF_ERR_HIP = -2,
  PHF_ERR_UNSUPPORTED = -3,
  PHF_ERR_DRAINED = -4        /* a queued launch gave up waiting and drained (phf_single_level_queue_status): results are stale */
};

/* Dose-response data of P (drug, channel) pairs for the single-level (non-hierarchical) models.
 * Replaces the per-pair arrays built at python/PyHillFit.py:661-683 (concs, responses, the three boolean
 * masks and pi_bit).  A pair is a list of ENTRIES (ln concentration, response, weight), stored masked-group by
 * masked-group: first the k_other entries with 0 < y < 100 (where_r_other), then the k_zero entries with y == 0
 * (where_r_0), then the k_hundred entries with y == 100 (where_r_100); points outside [0,100] belong to no mask
 * and are dropped, exactly as the reference ignores them.
 * An entry stands for `weight` data points measured at the same concentration (the Crumb set repeats 4 doses
 * over 3-6 experiments).  The likelihood sums of doseresponse.py:244-247 regroup exactly —
 *     sum_j (y_j - pred)^2 = sum_j (y_j - ybar)^2 + w (ybar - pred)^2,      sum_j log Phi(z(pred)) = w log Phi(z(pred))
 * — so an uncensored entry carries the MEAN response of its points, and extra[1] the theta-independent within-group
 * sum of squares.  One entry per point (weight 1, extra[1] = 0) is equally valid; merging only saves arithmetic. */
typedef struct phf_points {
  int32_t num_pairs;        /* P */
  int32_t stride;           /* doubles per pair row in ln_conc/response/weight (>= k_other+k_zero+k_hundred) */
  const double* ln_conc;    /* device [P][stride]  natural log of the dose in uM (-inf for dose 0) */
  const double* response;   /* device [P][stride]  percent inhibition (mean over the entry's points) */
  const double* weight;     /* device [P][stride]  number of data points the entry stands for */
  const int32_t* counts;    /* device [P][4]       k_other, k_zero, k_hundred entries, n_total data rows (incl. dropped points) */
  const double* pi_bit;     /* device [P]          0.5*n_total*ln(2 pi), python/doseresponse.py:299-301 */
  const double* extra;      /* device [P][2]       number of uncensored POINTS (sum of their weights; the n ln sigma term,
                                                   doseresponse.py:246), within-group sum of squares of the merged points */
} phf_points;

/* The batch of independent Markov chains one call advances: Q problems x C chains.
 * A problem = (pair, temperature): python/PyHillFit.py runs one per pair at temperature 1
 * (:57,978-981); python/PyHillTemp.py runs one per rung of the ladder (:151-161).
 * problem_id / chain_id_base feed the Philox counter so that a chain's random stream is the same whichever
 * GPU or launch runs it.                                                                                      */
typedef struct phf_problems {
  int32_t num_problems;          /* Q */
  int32_t chains_per_problem;    /* C */
  const int32_t* pair_index;     /* device [Q]  row of phf_points */
  const double* temperature;     /* device [Q]  power the likelihood is raised to */
  const uint32_t* problem_id;    /* device [Q]  global problem number (Philox counter word 1) */
  uint32_t chain_id_base;        /* global number of local chain 0 (Philox counter word 0) */
  uint32_t kernel_hint;          /* hierarchical launches (ABI 5; was `reserved`; single-level: 0, bit 4 or bit 5 (phf_single_level_last_kernel)): which kernel THIS launch
                                    should get — bits 0-1 lanes per chain (1 | 2), bits 2-3 register build of the two-lane kernel (1 | 2
                                    wavefronts per SIMD), bit 4 (ABI 6) = 1: not the gfx950 assembly build of the iteration (A/B timing,
                                    bit-identity tests), bit 6 (ABI 7) = 1: the queue workspace of phf_hierarchical_advance_queued holds
                                    phf_hierarchical_queue_words() words; 0 = the library decides from the launch size.  A host that runs several
                                    groups side by side sets it per launch (the groups together fill the chip although each alone
                                    would not); a process-wide policy (phf_hierarchical_set_kernel_policy, PHF_HIER_LANES / _WPS) overrides it.
                                    Every choice gives the same numbers bit for bit. */
  const int32_t* launch_order;   /* device [Q] or NULL: a permutation of 0..Q-1 — the order in which the problems' wavefronts are
                                    handed to the GPU (ABI 3).  Results do not depend on it (every problem writes its own rows and
                                    state); what does is the tail of a launch whose problems differ in cost: pairs have 2..8 entries,
                                    an iteration 550..1 500 instructions, and most expensive first (what the reference's pool gets by
                                    luck or not) took 6.5 % off the full-Crumb-set launch.  NULL = 0, 1, 2, ... */
  const uint32_t* chain_offset;  /* device [Q] or NULL (ABI 4): global number of problem q's local chain 0 is chain_id_base +
                                    chain_offset[q].  Lets a launch hold ANY subset of a batch's (problem, 64-chain block) units — a
                                    rank's share when a batch is split over GPUs by blocks rather than by whole pairs
                                    (pyhillfit_amd/distributed.py:shard_blocks) — with every chain keeping its Philox stream. */
} phf_problems;

/* Adaptive-Metropolis schedule: python/PyHillFit.py:787-848 / python/PyHillTemp.py:76-123. */
typedef struct phf_mh_config {
  int32_t model;                 /* 1: (pIC50, sigma), Hill fixed to 1;  2: (pIC50, Hill, sigma); doseresponse.py:250-279 */
  int32_t thinning;              /* save every thinning-th iteration (-t) */
  int64_t adapt_start;           /* when_to_adapt: 1000*d (PyHillFit.py:787, PyHillTemp.py:83) */
  int32_t reset_mean_at_adapt_start; /* PyHillTemp.py:114-115 */
  int32_t reserved;
  uint64_t seed;                 /* Philox key (the reference seeds numpy with 25: PyHillFit.py:824-825) */
  const double* gamma;           /* device [>= max(1, t_end-adapt_start+1)]  gamma[s] = 1/(s+1)**0.6 (PyHillFit.py:841-842);
                                    never NULL: gamma[0] (any finite value) is read before the adaptation starts */
} phf_mh_config;

int phf_version(void);
const char* phf_last_error(void);

/* SIMDs of the current HIP device (4 per compute unit on CDNA: 1 024 on an MI355X in SPX mode, fewer on a partitioned one), looked up
 * once per device (ABI 4).  The launchers below decide with it which register build a launch gets (one wavefront per SIMD: the whole
 * register file) and whether a queued launch can pay; exported so that a host never has to hard-code the chip. */
int phf_simd_count(void);

/* doubles of per-chain state for the single-level sampler: theta[d], log-target, mean[d], cov[d(d+1)/2]
 * (packed lower triangle, row-major), loga, accepted-count, untempered log-likelihood of the current state
 * ->  2d + d(d+1)/2 + 4.                                                                                     */
int phf_single_level_state_size(int model);

/* Start Q*C chains.  Replaces python/PyHillFit.py:748-751,789,796-798,814 (PyHillTemp.py:63-80):
 *   theta = mean = theta0;  cov = cov_scale*diag(|theta0|) (cov_identity == 0; PyHillFit 0.05) or
 *   cov_scale*I (cov_identity != 0; PyHillTemp);  log-target of theta0;  loga = 0;  acceptance = 0.
 *   theta0    device [d][Q*C]
 *   state     device [S][Q*C]   (S = phf_single_level_state_size)
 *   row0      device [Q][d+1][C] or NULL: receives chain row 0 = (theta0, log-target)                      */
int phf_single_level_init(const phf_points* pts, const phf_problems* prob, int model, int cov_identity,
                          double cov_scale, const double* theta0, double* state, double* row0, void* stream);

/* Run MH iterations t_begin+1 .. t_end for every chain, in lock-step.  Replaces the loop
 * python/PyHillFit.py:830-856 (python/PyHillTemp.py:87-123).
 *   state     device [S][Q*C]   read, advanced, written back (so calls can be chained; also the checkpoint)
 *   rows      device [R][Q][d+1][C] or NULL, R = t_end/thinning - t_begin/thinning: the saved samples
 *             (theta, log-target) of iterations t with t % thinning == 0, in order (PyHillFit.py:847-848)
 *   moments   device [2(d+1)+1][Q*C] or NULL: running sums of x and x*x (x = theta, log-target) over the saved samples
 *             with t > moments_after (on-device replacement for reading the chain file back to get posterior
 *             means/variances); last row: sum of log_data_likelihood(theta, t = 1) over the same samples — the
 *             expectation python/compute_bayes_factors.py:11-27 needs per temperature rung (thermodynamic
 *             integration), at no extra cost.  Accumulated into, never zeroed.                               */
int phf_single_level_advance(const phf_points* pts, const phf_problems* prob, const phf_mh_config* cfg,
                             int64_t t_begin, int64_t t_end, double* state, double* rows,
                             double* moments, int64_t moments_after, void* stream);

/* Which kernel the calling thread's last phf_single_level_advance[_queued] launched (ABI 6; 0 = none yet): 1 = mh_advance_kernel (hipcc),
 * 2 = phf_sl3_advance, the hand-allocated gfx950 build of the model-2 iteration — OPT-IN (phf_problems.kernel_hint bit 5, or PHF_SL_ISA=1
 * in the environment; bit 4 vetoes it): launches without moments, more than one wavefront per SIMD, at most 32 entries per pair; same
 * numbers bit for bit, not faster than the hipcc kernel (why: DESIGN.md section 3) —, 3 = the same as a work queue. */
int phf_single_level_last_kernel(void);

/* The same advance as a WORK QUEUE inside one launch (ABI 3).  The launch is cut into quanta of `quantum` iterations; the grid is
 * only as large as the chip holds at once and its wavefronts pull (quantum, block) tasks — quantum-major, blocks in
 * prob->launch_order — from a counter, a block's quanta chaining through its state in HBM with agent-scope release/acquire.
 * Results are identical to phf_single_level_advance (same chains, rows, state, moments); what changes is the tail of a launch
 * whose problems differ in cost (the reference's unit of work, one pair, varies 2.5x in cost over the Crumb set; its process pool
 * balances that dynamically too, python/PyHillFit.py:997-1003).  Falls back to the plain launch when queueing cannot pay
 * (fewer blocks than the chip's 2 x phf_simd_count() wavefront slots, more than 16 rounds of them — the tail is then negligible —,
 * or fewer than two quanta).
 *   queue   device int32 [2 + Q * ceil(C/64)] workspace owned by the caller, zeroed by the caller when it is allocated.  Words
 *           0 .. Q*ceil(C/64) (task counter, per-block progress) are zeroed here, on the stream, before every launch; the LAST word
 *           is a sticky fault flag (ABI 4) the library only ever sets: a wavefront whose wait for a predecessor quantum does not
 *           end (cannot happen in a correct run) sets it, poisons the counter so that the launch drains, and returns WITHOUT
 *           advancing its block — the call has long returned PHF_OK by then, so check phf_single_level_queue_status() wherever the
 *           host synchronises anyway. */
int phf_single_level_advance_queued(const phf_points* pts, const phf_problems* prob, const phf_mh_config* cfg,
                                    int64_t t_begin, int64_t t_end, double* state, double* rows, double* moments,
                                    int64_t moments_after, int32_t quantum, int32_t* queue, void* stream);

/* Synchronise `stream` and read the sticky fault flag of a queue workspace (ABI 4): PHF_OK, or PHF_ERR_DRAINED if any queued launch
 * on it drained — states, rows and moments written since the flag was last zero are then stale and must be discarded.
 *   num_blocks = Q * ceil(C/64), as for the launches that used the workspace. */
int phf_single_level_queue_status(const int32_t* queue, int64_t num_blocks, void* stream);

/* Batch evaluation of the single-level log-likelihood and log-prior at M parameter vectors.
 * Replaces calls of dr.log_data_likelihood / dr.log_priors / dr.log_target
 * (python/doseresponse.py:187-189,203-248,166-184), e.g. the Bayes-factor sweep
 * python/compute_bayes_factors.py:18-21.
 *   pair_index  device [M], temperature device [M], theta device [d][M]
 *   out_lik, out_prior  device [M] (either may be NULL);  log_target = out_lik + out_prior                   */
int phf_single_level_log_target(const phf_points* pts, int model, int64_t m, const int32_t* pair_index,
                                const double* temperature, const double* theta, double* out_lik,
                                double* out_prior, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Hierarchical model (python/PyHillFit.py --hierarchical: log_target_distribution :113-193, loop :429-511).
 * theta = [alpha, beta, mu, s, pIC50_1, Hill_1, ..., pIC50_Ne, Hill_Ne, sigma], dim = 5 + 2 Ne (:178-181).
 * One call handles problems whose pairs all have the same number of experiments Ne (1 <= Ne <= PHF_HIER_MAX_EXPTS);
 * the host groups the pairs by Ne (Crumb: Ne = 3..6).  Ne <= PHF_HIER_FAST_EXPTS runs kernels compiled per Ne (state in
 * registers, proposal factor in LDS) — one lane per chain, or, for Ne = 3..6 when the launch is small enough to give every
 * wavefront a SIMD of its own, TWO lanes per chain (half the instructions per iteration; same results bit for bit;
 * phf_hierarchical_set_kernel_policy forces one or the other) —; larger Ne (the reference's synthetic set has Ne = 50,
 * dim 105) runs one WAVEFRONT per chain with the whole state in LDS: lanes take an experiment each in the target and a row
 * each in the factor.                                                                                            */
#define PHF_HIER_MAX_EXPTS 64
#define PHF_HIER_FAST_EXPTS 8

/* Points of P pairs, stored experiment by experiment (python/doseresponse.py:60-67 keeps one array per experiment). */
typedef struct phf_hier_points {
  int32_t num_pairs;          /* P */
  int32_t stride;             /* doubles per pair row in ln_conc/response */
  int32_t n_expts;            /* Ne, the same for every pair of this set */
  int32_t points_per_expt;    /* ABI 6 (was `reserved`): the point SHAPE of every pair of this set, the caller's statement about its data (like
                                 n_expts; expt_start must say the same): per | last << 4 — EVERY experiment of EVERY pair has `per` points
                                 (1..15), except that the last one has `last` (1..15) if those bits are not 0; so n > 0 alone = n points in
                                 every experiment; or (ABI 7) bit 30 + a nibble per experiment, experiment 0 in the lowest (up to 7 experiments of
                                 1..15 points: 4 + 4 + 4 + 1 + 1 = 0x40011444); 0 = the pairs differ, the shape has no such code, or unknown.  (PHF_HIER_SHAPE of
                                 pyhillfit_amd/csrc/phf_hier_model.h.)  Launches that get one lane per chain run the hand-allocated gfx950
                                 build of the iteration (two wavefronts per SIMD: same numbers) where the library has one for (n_expts,
                                 shape): n_expts == 3 with 4 + 4 + 4 points (147 of the Crumb set's 210 pairs), 2 + 2 + 2 (6), 5 + 5 + 4 (1);
                                 ABI 7: every n_expts == 4 shape of the Crumb set (4 + 4 + 4 + 1 (32 pairs), + 2 (5), + 3 (2), 2 + 2 + 2 + 1, 5 + 5 + 5 + 1) and
                                 every n_expts == 5 and 6 one (4 + 4 + 4 + 1 + 1 (5), 4 + 4 + 4 + 2 + 1 (5), 4 + 4 + 4 + 4 + 4, 5 + 5 + 4 + 2 + 2; 4 + 4 + 4 + 1 + 1 + 1 (2),
                                 4 + 4 + 4 + 4 + 2 + 1: the last two, like 2 + 2 + 2 + 1, 5 + 5 + 5 + 1 and the n_expts == 5 ones, in the fused kernel only) — through
                                 phf_hierarchical_advance_queued / _fused with a workspace of phf_hierarchical_queue_words() words and kernel_hint bit 6. */
  const double* ln_conc;      /* device [P][stride] */
  const double* response;     /* device [P][stride] */
  const int32_t* expt_start;  /* device [P][Ne+1]  first point of each experiment; [Ne] = number of points */
} phf_hier_points;

#ifndef PHF_HIER_PRIOR_DEFINED
#define PHF_HIER_PRIOR_DEFINED
/* Shifted-Gamma hyper-priors of (alpha, beta, mu, s, sigma): python/PyHillFit.py:301,340-364 */
typedef struct phf_hier_prior {
  double shape_m1[5];         /* shapes - 1 */
  double inv_scale[5];        /* 1/scales */
  double loc[5];              /* lower bounds (locs) */
} phf_hier_prior;
#endif

/* doubles of per-chain state: theta[dim], log-target, mean[dim], F[dim(dim+1)/2], loga, accepted-count.
 * F holds the adapted covariance as cov = L diag(d) L' — L unit lower triangular — in ONE packed lower triangle (row-major):
 * slot (i, j < i) = L_ij, slot (i, i) = d_i.  The factors are carried instead of the covariance: the reference's update
 * cov <- (1-g) cov + g v v' (PyHillFit.py:498-499) is applied to them as d <- (1-g) d followed by a rank-one update (Gill, Golub,
 * Murray & Saunders 1974, method C1), which is the same matrix in exact arithmetic and needs one pass over dim(dim+1)/2 numbers
 * per iteration — two fused multiply-adds per element, no square root — instead of an O(dim^3) refactorisation; the proposal
 * (PyHillFit.py:485) is theta + e^(loga/2) L sqrt(d) z.  (ABI <= 3 carried a Cholesky factor in the same slots.)          */
int phf_hierarchical_state_size(int n_expts);

/* Start chains: theta = mean = theta0, cov = diag(cov_scale*|theta0|) (PyHillFit.py:431, cov_scale 0.01), loga = 0.
 *   theta0 device [dim][Q*C];  state device [S][Q*C];  row0 device [Q][dim+1][C] or NULL.
 *   prob->temperature is ignored (the hierarchical sampler is not tempered).                                  */
int phf_hierarchical_init(const phf_hier_points* pts, const phf_problems* prob, const phf_hier_prior* prior,
                          double cov_scale, const double* theta0, double* state, double* row0, void* stream);

/* MH iterations t_begin+1 .. t_end (python/PyHillFit.py:484-511); arguments as phf_single_level_advance with
 * d = dim; cfg->model is ignored, cfg->adapt_start is 100*dim in the reference (:440).                        */
int phf_hierarchical_advance(const phf_hier_points* pts, const phf_problems* prob, const phf_hier_prior* prior,
                             const phf_mh_config* cfg, int64_t t_begin, int64_t t_end, double* state, double* rows,
                             double* moments, int64_t moments_after, void* stream);

/* The same advance as a WORK QUEUE inside one launch (ABI 6), as phf_single_level_advance_queued: where the launch runs the gfx950
 * assembly build (n_expts == 3, points_per_expt == 4, one lane per chain) AND has more 64-chain blocks than the chip holds wavefronts
 * (2 x phf_simd_count()) AND at least two quanta, it is cut into quanta of `quantum` iterations (0 = the library's choice: about 16 rounds
 * of tasks on the chip's wavefront slots, at least 100 iterations; rounded down to a multiple of the thinning) and a grid as large as the chip pulls (quantum, block) tasks from a counter, a block's quanta
 * chaining through its state in HBM with agent-scope release / acquire — the ragged last round of a launch becomes a round of short
 * tasks (147 pairs x 1 024 chains: 2 352 wavefronts on 2 048 slots).  Every other launch runs exactly as phf_hierarchical_advance.
 * Results are identical either way (same chains, rows, state, moments).
 *   queue   device int32 [2 + Q * ceil(C / 64)], owned by the caller, zeroed by the caller when allocated; words 0 .. Q ceil(C/64) are
 *           zeroed here, on the stream, before a queued launch; word 1 + Q ceil(C/64) is the sticky fault flag of
 *           phf_single_level_queue_status (same layout, same meaning: check it there wherever the host synchronises anyway).
 *           ABI 7: a workspace of phf_hierarchical_queue_words(pts, prob) words — which the caller states with kernel_hint bit 6 —
 *           also holds the device-memory scratch in which the gfx950 build of the Ne = 4 iteration keeps the last rows of the proposal
 *           factor (21 KB per resident wavefront, at most 44 MB); without that statement such launches run the hipcc kernels. */
/* CAUTION (profiles/r05/queue_progress_word_hazard.txt): do not run a queued launch of the gfx950 build BESIDE other launches of that build on the same
 * GPU (several groups of one run, a stream each) — a wavefront has been seen to wait for a block's progress word until it gave up (PHF_ERR_DRAINED
 * through the fault flag); several groups go through phf_hierarchical_advance_fused (one grid), or one after the other, or kernel_hint bit 4. */
int phf_hierarchical_advance_queued(const phf_hier_points* pts, const phf_problems* prob, const phf_hier_prior* prior,
                                    const phf_mh_config* cfg, int64_t t_begin, int64_t t_end, double* state, double* rows,
                                    double* moments, int64_t moments_after, int32_t quantum, int32_t* queue, void* stream);

/* int32 words the queue workspace of phf_hierarchical_advance_queued has to hold for launches of this (pts, prob) shape (ABI 7):
 * 2 + Q ceil(C / 64), plus the scratch of a gfx950 kernel that keeps part of the chain state in device memory (n_expts == 4 with
 * 4 + 4 + 4 + 1 / 2 / 3 points).  Reads only n_expts, points_per_expt, num_problems and chains_per_problem; no device call.  < 0: error. */
int64_t phf_hierarchical_queue_words(const phf_hier_points* pts, const phf_problems* prob);

/* EVERY launch group of a run through ONE persistent grid (ABI 7; phf_hier_fused_advance of the gfx950 code object: a body per (n_expts, point
 * shape), a wavefront that finishes a task of one group pulls the next task whatever group it belongs to).  Separate launches side by side —
 * one stream per group, what python/PyHillFit.py's pool amounts to (:997-1003) — leave a chip's workgroup slots to whichever persistent grid
 * got them first; one queue does not.  groups: 1..14 of them, each with a (n_expts, points_per_expt) the code object has a kernel for
 * (PHF_ERR_UNSUPPORTED otherwise: launch such groups one by one), no two alike; the same thinning in every cfg; t_begin a multiple of it.
 * Every chain's numbers are those of phf_hierarchical_advance, bit for bit.  queue: device int32 [phf_hierarchical_fused_queue_words()],
 * zeroed by the caller when allocated; word 1 + (the groups' blocks) is the sticky fault flag. */
typedef struct phf_hier_group {
  const phf_hier_points* pts;
  const phf_problems* prob;
  const phf_mh_config* cfg;      /* seed, thinning, adapt_start, gamma of THIS group (adapt_start = 100 dim differs with n_expts) */
  double* state;                 /* device [phf_hierarchical_state_size(n_expts)][Q C] */
  double* rows;                  /* device [rows][Q][dim + 1][C] or NULL */
  double* moments;               /* device [2 (dim + 1)][Q C] or NULL */
} phf_hier_group;
int64_t phf_hierarchical_fused_queue_words(int32_t n_groups, const phf_hier_group* groups);
int phf_hierarchical_advance_fused(int32_t n_groups, const phf_hier_group* groups, const phf_hier_prior* prior, int64_t t_begin, int64_t t_end,
                                   int64_t moments_after, int32_t quantum, int32_t* queue, void* stream);

/* Which kernel runs groups with Ne = 3..6, PROCESS-WIDE (ABI 4; A/B timing and the bit-identity tests): lanes 1 | 2 = one | two lanes
 * per chain, wps 1 | 2 = the register build of the two-lane kernel (512 | 256 registers); 0 = not forced: the launch's own
 * phf_problems.kernel_hint, else the launch size, decides.  The environment variables PHF_HIER_LANES / PHF_HIER_WPS give the initial
 * values and are read ONCE, here in the library, at the first use; the two words are plain atomics (any thread may set them). */
int phf_hierarchical_set_kernel_policy(int lanes, int wps);

/* Which kernel the calling thread's last phf_hierarchical_advance launched (ABI 6; 0 = none yet): the tests that compare kernels
 * against each other assert through it that the kernel they mean is the one that ran. */
#define PHF_HIER_KERNEL_ONE_LANE 1     /* hier_advance_kernel<Ne>: one lane per chain, hipcc */
#define PHF_HIER_KERNEL_TWO_LANES 2    /* hier_advance2_kernel<Ne, wps> */
#define PHF_HIER_KERNEL_WAVE 3         /* hier_wave_advance_kernel: one wavefront per chain (Ne > 8) */
#define PHF_HIER_KERNEL_GFX950_ISA 4   /* phf_hier3_advance: the hand-allocated gfx950 build (Ne = 3, four points per experiment) */
#define PHF_HIER_KERNEL_GFX950_ISA_QUEUED 5   /* ... as a work queue (phf_hierarchical_advance_queued) */
#define PHF_HIER_KERNEL_GFX950_ISA_FUSED 6    /* ... every group of a run in one persistent grid (phf_hierarchical_advance_fused, ABI 7) */
int phf_hierarchical_last_kernel(void);

/* log_target_distribution (python/PyHillFit.py:173-193) at M parameter vectors: theta device [dim][M]. */
int phf_hierarchical_log_target(const phf_hier_points* pts, const phf_hier_prior* prior, int64_t m,
                                const int32_t* pair_index, const double* theta, double* out, void* stream);

/* Evaluate one of the device elementary functions on an array (parity tests: the device must reproduce the
 * host build of pyhillfit_amd/csrc/phf_math.h bit for bit).
 * fn: 0 exp, 1 log, 2 erfcx(y>=0), 3 log_ndtr, 4 ndtr, 5 sqrt, 6 reciprocal, 7 sin(2 pi w/2^32), 8 cos(...)
 * 9 exp_fast, 10 log_fast, 11 log_ndtr_nonpos — the branch-free forms the kernels use
 * (for 7/8 the input doubles hold integer values w in [0, 2^32));
 * the MH loops' own division / square root without exponent-range handling (phf_math.h; correctly rounded for operands within
 * 2^-600..2^600): 12 phf_rcp(x), 13 phf_sqrt_pos(x), 14 phf_div(ln 10, x), 15 phf_sqrt_nonneg(x) (0 -> 0), 16 phf_div(x, ln 10);
 * 17 phf_normal_u32(w): the single-level sampler's standard normal of a 32-bit word (input doubles hold integer values w in [0, 2^32));
 * 18 phf_log_ndtr_tab(x): log Phi(x) from the censored likelihood's table (valid for -185 000 < x <= 0; any x is safe to pass);
 * 19 phf_erfc_tab(y): erfc(y), y >= 0, to 3.6e-17 absolute from the hierarchical target's table, 0 from y = 6 on (any y is safe to pass);
 * 20 / 21 phf_sqrt_rcp_pos(x): the reciprocal 1 / sqrt(x) (of the ROUNDED root) / the root itself — a Cholesky pivot and its reciprocal
 * from one hardware estimate (ABI 5; python/PyHillFit.py:831 draws through numpy's factorisation of the same covariance);
 * 22: n even, in = n / 2 pairs (x, w) (w an integer value in [0, 2^32)): out[2 i] = phf_mh_accept_u32(x, w) (the single-level sampler's
 * accept test for d = 3), out[2 i + 1] = phf_log_pos_k((w + 1/2) / 2^32) < x, each 1.0 or 0.0. */
int phf_debug_math(int fn, int64_t n, const double* in, double* out, void* stream);

/* The same for the hand-allocated gfx950 code object (ABI 6; tools/gen_hier_isa.py, tools/isa/phf_isa_math.py): every elementary
 * function of the assembly build of the hierarchical Ne = 3 iteration, evaluated on an array by a unit kernel of the same code object —
 * each must reproduce its C namesake in pyhillfit_amd/csrc/phf_math.h bit for bit (tests/test_gpu_isa.py).
 * fn: 0 phf_exp_fast_k, 1 phf_exp_capped_k, 2 phf_log_pos_k, 3 phf_log_fast_k, 4 phf_erfc_tab, 5 phf_rcp, 6 phf_sqrt_nonneg (in, out:
 * device double [n]); 7 phf_normal_u32, 8 phf_log_pos_k(phf_unit_open32(w)) (in: device uint32 [n], out: device double [n]);
 * 9 Philox4x32-7 (in: device uint32 [n][6] = counter words 0..3, key words 0..1 — the KEY OF ELEMENT 0 is used for the whole call,
 * as the kernels advance the key schedule on the scalar unit; out: device uint32 [n][4]). */
int phf_debug_isa(int fn, int64_t n, const void* in, void* out, void* stream);

/* The four Philox4x32-R words of n (counter, key) tuples: in device uint32 [n][6], out device uint32 [n][4].
 * phf_debug_philox: R = the rounds the samplers draw with, phf_philox_rounds() (7 since ABI 5; rounds 1-3 of this build: 10);
 * phf_debug_philox_rounds: R = 7 or 10 (both are held to the Random123 known-answer vectors).  Plays the role of the reference's
 * numpy RandomState (python/PyHillFit.py:825,831,834; python/PyHillTemp.py:88,100). */
int phf_philox_rounds(void);
int phf_debug_philox(int64_t n, const uint32_t* counter_key, uint32_t* out, void* stream);
int phf_debug_philox_rounds(int rounds, int64_t n, const uint32_t* counter_key, uint32_t* out, void* stream);

/* ---- posterior-predictive curves -------------------------------------------------------------------
 * Replaces construct_posterior_predictive_cdfs (python/construct_hierarchical_cdfs.py:32-58): for every problem q
 * and every hierarchical sample (alpha, beta, mu, s) add fisk.cdf/pdf(hill_x; c=beta, scale=alpha) and
 * logistic.cdf/pdf(pic50_x; mu, s) into running sums; the caller divides by the number of samples (:54-57).
 *   rows     device [num_rows][num_problems][row_stride][num_chains] — the row buffer phf_hierarchical_advance wrote
 *            (row_stride = dim+1; columns 0..3 = alpha, beta, mu, s), or any tensor of that shape (a chain read back
 *            from a reference-format file: row_stride 4, num_chains 1).  Chains 0..chains_used-1 of every row are used.
 *   hill_x, pic50_x  device [grid_points]  (the reference: 501 points on [0,4] and [-2,12], :33-39)
 *   chunk    samples per partial sum (fixes the order of the additions; 4096 is a good value)
 *   sums     device [num_problems][4][grid_points], curves in the order hill cdf, pic50 cdf, hill pdf, pic50 pdf;
 *            ADDED to (zero it before the first call; call once per segment of rows)
 *   scratch  device, at least phf_predictive_scratch_bytes(num_problems, num_rows*chains_used, grid_points, chunk) */
size_t phf_predictive_scratch_bytes(int num_problems, int64_t samples_per_problem, int grid_points, int chunk);
int phf_predictive_accumulate(int num_problems, const double* rows, int64_t num_rows, int row_stride, int num_chains,
                              int chains_used, int grid_points, const double* hill_x, const double* pic50_x, int chunk,
                              double* sums, double* scratch, size_t scratch_bytes, void* stream);

/* ---- convergence diagnostics: split-R-hat, multi-chain ESS, MCSE of the mean -------------------------------------------------
 * The reference runs one chain per pair and computes none of these.  Per problem q and column j, over the post-burn-in rows
 * x[m][n] of chains m = 0..C-1, n = 0..N-1: split-R-hat and multi-chain ESS as in the Stan reference manual (Gelman et al.,
 * BDA3 11.4-11.5; Vehtari et al. 2021) WITHOUT rank normalisation.  Chain m gives half-chains 2m (rows 0..h-1) and 2m+1
 * (rows N-h..N-1), h = floor(N/2) >= 4; the device accumulates, per half-chain, its mean and its autocovariance
 * acov(k) = (1/h) sum_{n=0}^{h-1-k} (x_n - mean)(x_{n+k} - mean), k = 0..L, L = min(K, h-1), while the rows stream past
 * (pyhillfit_amd/csrc/phf_diagnostics.hip); phf_diagnostics_reduce averages over the 2C half-chains and the host applies Geyer's
 * initial positive / monotone sequence (pyhillfit_amd/diagnostics.py).  Deterministic: no atomics, and the result is bit-identical
 * however the rows are cut into accumulate calls.
 *   rows       device [num_rows][num_problems][row_stride_cols][num_chains] — the samplers' row buffer (single-level,
 *              hierarchical and tempered alike) or a slice of it along the first axis; columns 0..num_columns-1 are diagnosed
 *   first_row  index of rows[0] among the total_rows post-burn-in rows; calls must come in row order, each row exactly once
 *   lags       the lag limit K (256 is the command lines' default)
 *   workspace  device, at least phf_diagnostics_workspace_bytes(...) = num_problems * num_columns * num_chains * (4L + 6) doubles;
 *              phf_diagnostics_init zeroes it (stream-ordered) before the first accumulate
 *   out        device [num_problems][num_columns][L + 3]: mean over half-chains of acov(k) for k = 0..L, then the mean of the
 *              half-chain means, then their variance with divisor 2C - 1 (= B/h); valid once all total_rows rows have arrived
 * phf_diagnostics_workspace_bytes returns 0 for an invalid shape (phf_last_error() says why); phf_diagnostics_effective_lags
 * returns L = min(K, floor(total_rows / 2) - 1) or a negative code. */
size_t phf_diagnostics_workspace_bytes(int num_problems, int num_columns, int num_chains, int64_t total_rows, int lags);
int phf_diagnostics_effective_lags(int64_t total_rows, int lags);
int phf_diagnostics_init(int num_problems, int num_columns, int num_chains, int64_t total_rows, int lags, double* workspace,
                         size_t workspace_bytes, void* stream);
int phf_diagnostics_accumulate(const double* rows, int64_t num_rows, int num_problems, int row_stride_cols, int num_chains,
                               int num_columns, int64_t first_row, int64_t total_rows, int lags, double* workspace,
                               size_t workspace_bytes, void* stream);
int phf_diagnostics_reduce(int num_problems, int num_columns, int num_chains, int64_t total_rows, int lags, const double* workspace,
                           size_t workspace_bytes, double* out, void* stream);

/* ---- ESS and MCSE beyond the lag limit: batch means on a dyadic ladder of batch sizes -----------------------------------------
 * The "blocking" method (Flyvbjerg & Petersen 1989; the estimator behind mcmcse) for chains whose autocorrelation time exceeds what
 * phf_diagnostics_* can sum.  Half-chains as above (h = floor(total_rows / 2) >= 2, M = 2C).  Per (problem, column, chain, half), with
 * y = x - (the half's first value): levels l = 0..NL-1, NL = floor(log2 h) + 1, batches of b = 2^l rows aligned to the half's start
 * (trailing rows that fill no batch are not used at that level); a batch sum of level l+1 is (left child) + (right child); per level
 * S1 = sum of the batch sums and S2 = sum of their squares, in batch order (pyhillfit_amd/csrc/phf_batch_means.h).  Deterministic: no
 * atomics, bit-identical however the rows are cut into accumulate calls.  rows, first_row, total_rows, stream: as for
 * phf_diagnostics_accumulate; the same error codes.
 *   workspace  device, phf_batch_means_workspace_bytes(...) = num_problems * num_columns * num_chains * (5 NL + 2) doubles, laid out
 *              [problem][column][field][chain] with the fields x0[2] | pending[NL] | S1[half 0][NL] | S2[half 0][NL] | S1[half 1][NL] |
 *              S2[half 1][NL]; phf_batch_means_init zeroes it (stream-ordered)
 *   out        device [num_problems][num_columns][NL + 1]: for l = 0..NL-2 (the levels with n_l = floor(h / b) >= 2 batches) the mean
 *              over the 2C half-chains of the variance of the batch means, (S2 - S1^2 / n_l) / ((n_l - 1) b^2) (l = 0: W); then the mean of
 *              the half-chain means; then their variance with divisor 2C - 1 (= B/h).  Sums over chains: lane l of a wavefront takes
 *              chains l, l + 64, ... (half 0's term + half 1's), then a butterfly over lane distances 32, 16, .., 1.
 * phf_batch_means_workspace_bytes returns 0 for an invalid shape (phf_last_error() says why); phf_batch_means_levels returns NL or a
 * negative code. */
size_t phf_batch_means_workspace_bytes(int num_problems, int num_columns, int num_chains, int64_t total_rows);
int phf_batch_means_levels(int64_t total_rows);
int phf_batch_means_init(int num_problems, int num_columns, int num_chains, int64_t total_rows, double* workspace, size_t workspace_bytes,
                         void* stream);
int phf_batch_means_accumulate(const double* rows, int64_t num_rows, int num_problems, int row_stride_cols, int num_chains,
                               int num_columns, int64_t first_row, int64_t total_rows, double* workspace, size_t workspace_bytes,
                               void* stream);
int phf_batch_means_reduce(int num_problems, int num_columns, int num_chains, int64_t total_rows, const double* workspace,
                           size_t workspace_bytes, double* out, void* stream);

/* ---- posterior correlations and multivariate R-hat: co-moments of the parameter columns per half-chain -------------------------
 * The one analysis that looks ACROSS columns.  Half-chains as for phf_diagnostics_* (h = floor(total_rows / 2) >= 4, M = 2C, the
 * middle row of an odd total_rows is never read).  Per (problem, half, chain), with y = x - (the half's first row) over the
 * d = num_columns columns 0..d-1 of a row: S_i = sum y_i and P_ij = sum y_i y_j (i <= j), as S <- S + y and P <- fma(y_i, y_j, P)
 * in row order, a row count, and a flag set by a row with a non-finite y (such a half-chain is dropped whole by the reduction).
 * Deterministic: no atomics, bit-identical however the rows are cut into accumulate calls (pyhillfit_amd/csrc/phf_comoments.h
 * holds the rules, the workspace layout and the reduction order; its host build is the kernels' twin).  rows, first_row,
 * total_rows, stream: as for phf_diagnostics_accumulate; the same error codes.  num_columns <= 1024.
 *   workspace  device, phf_comoments_workspace_bytes(...) = num_problems * 2 * num_chains * (2d + d(d+1)/2 + 2) doubles, laid out
 *              [problem][half][field][chain] with the fields x0[d] | S[d] | P[d(d+1)/2] (row-major upper triangle) | rows | flag;
 *              phf_comoments_init zeroes it (stream-ordered)
 *   out        device [num_problems][2 d(d+1)/2 + 2d + 4]: W (the mean over the m used half-chains of their sample covariances,
 *              divisor h - 1), B/h (the sample covariance of their means, divisor m - 1; both as upper triangles), the grand mean
 *              [d], the sum over half-chains of (mean - the first used half-chain's mean) [d], m, the number of half-chains dropped,
 *              h, and a spare 0; valid once all total_rows rows have arrived.  W is 0 when m = 0 and B/h when m < 2.
 * phf_comoments_workspace_bytes returns 0 for an invalid shape (phf_last_error() says why). */
size_t phf_comoments_workspace_bytes(int num_problems, int num_columns, int num_chains, int64_t total_rows);
int phf_comoments_init(int num_problems, int num_columns, int num_chains, int64_t total_rows, double* workspace, size_t workspace_bytes,
                       void* stream);
int phf_comoments_accumulate(const double* rows, int64_t num_rows, int num_problems, int row_stride_cols, int num_chains,
                             int num_columns, int64_t first_row, int64_t total_rows, double* workspace, size_t workspace_bytes,
                             void* stream);
int phf_comoments_reduce(int num_problems, int num_columns, int num_chains, int64_t total_rows, const double* workspace,
                         size_t workspace_bytes, double* out, void* stream);

/* ---- pointwise log-likelihood and WAIC -------------------------------------------------------------------------------------
 * The terms are per DATA POINT (not per merged entry).  Points of problem q are row q of the arrays, in any order the caller keeps
 * (pyhillfit_amd/waic.py: data-file order); point p < count[q] of problem q has log-likelihood, for one parameter vector:
 *   single-level (model 1: theta = (pIC50, sigma), Hill = 1; model 2: theta = (pIC50, Hill, sigma)), pred = the Hill curve in percent,
 *     tag 0 (0 < y < 100):  -ln(2 pi)/2 - ln sigma - (y - pred)^2 / (2 sigma^2)
 *     tag 1 (y == 0):       ln Phi((0 - pred)/sigma)          tag 2 (y == 100): ln Phi((pred - 100)/sigma)
 *     (points outside [0, 100] are the caller's to drop, as the sampler drops them; sigma <= 1e-3 gives -inf).  Their sum over a
 *     pair's points is the sampler's t = 1 log-likelihood + (n_total - n_uncensored) ln(2 pi)/2: the reference's pi_bit charges
 *     ln(2 pi)/2 to censored and dropped points too.
 *   hierarchical (theta = [alpha, beta, mu, s, pIC50_1, Hill_1, ..., pIC50_Ne, Hill_Ne, sigma]), tag = the point's experiment i:
 *     -ln(2 pi)/2 - ln sigma - (y - pred_i)^2 / (2 sigma^2) - ln(Phi((100 - pred_i)/sigma) - Phi((0 - pred_i)/sigma)),
 *     the truncated-normal density of the hierarchical likelihood (sigma <= 1e-3 gives -inf).
 * Device arrays; count[q] is clamped to [0, stride] and a tag outside its range to the nearest valid one (no access out of bounds). */
typedef struct phf_pointwise_points {
  int32_t num_problems;
  int32_t stride;              /* points per problem row (>= every count) */
  const double* ln_conc;       /* [num_problems][stride] natural log of the concentration */
  const double* response;      /* [num_problems][stride] */
  const int32_t* tag;          /* [num_problems][stride] single-level: 0 | 1 | 2 as above; hierarchical: experiment index 0..Ne-1 */
  const int32_t* count;        /* [num_problems] points of each problem */
} phf_pointwise_points;

/* Batch evaluators: out[i][p] = log-likelihood of point p of problem problem_index[i] at theta[.][i] ([d][m], column i = vector i;
 * d = model + 1, or 5 + 2 num_expts); out is [m][stride], NaN for p >= count.  Serve the tests and the chain-file tool. */
int phf_pointwise_loglik_single_level(const phf_pointwise_points* pts, int model, int64_t m, const int32_t* problem_index,
                                      const double* theta, double* out, void* stream);
int phf_pointwise_loglik_hierarchical(const phf_pointwise_points* pts, int num_expts, int64_t m, const int32_t* problem_index,
                                      const double* theta, double* out, void* stream);

/* Streaming WAIC accumulator (pyhillfit_amd/csrc/phf_pointwise.hip).  Over the S = total_rows x num_chains draws of problem q,
 * per point p: LSE_p = ln sum_draws exp(l_p) and var_p = the variance of l_p over the draws (divisor S - 1).
 *   likelihood  1 | 2: single-level model 1 | 2, theta = columns 0..model of a row;
 *               3: hierarchical with num_expts = Ne experiments, pIC50_i = column 4 + 2i, Hill_i = 5 + 2i, sigma = 4 + 2 Ne
 *   rows        device [num_rows][num_problems][row_stride_cols][num_chains] — the samplers' row buffer or a slice of it along the
 *               first axis (the layout phf_diagnostics_accumulate reads), problem q <-> row q of pts
 *   first_row   index of rows[0] among the total_rows rows; calls come in row order, each row exactly once
 *   workspace   device, phf_waic_workspace_bytes(...) = num_problems * stride * 5 * num_chains doubles: per (problem, point, chain) a
 *               running max and the sum of exp(l - max) (online log-sum-exp), the first l and the sums of (l - first) and its square;
 *               phf_waic_init zeroes it (stream-ordered) before the first accumulate
 *   out         device [2][num_problems][stride]: LSE_p, then var_p; valid once all total_rows rows have arrived (meaningless for p >= count)
 * Deterministic: no atomics, every accumulator is produced by one lane in row order and round-trips through HBM exactly; the chains
 * are merged in a fixed order.  Bit-identical however the rows are cut into calls.  An invalid shape gives 0 bytes /
 * PHF_ERR_INVALID_ARGUMENT without touching a GPU (phf_last_error() says why). */
size_t phf_waic_workspace_bytes(int num_problems, int stride, int num_chains, int64_t total_rows);
int phf_waic_init(int num_problems, int stride, int num_chains, int64_t total_rows, double* workspace, size_t workspace_bytes,
                  void* stream);
int phf_waic_accumulate(const phf_pointwise_points* pts, int likelihood, int num_expts, const double* rows, int64_t num_rows,
                        int num_problems, int row_stride_cols, int num_chains, int64_t first_row, int64_t total_rows, double* workspace,
                        size_t workspace_bytes, void* stream);
/* The same accumulator with a GIVEN log-likelihood (likelihood code 4 of the streaming kernels): l of point p < count[q] of problem q
 * is column p of the row, rows [num_rows][num_problems][row_stride_cols >= stride][num_chains]; of pts only stride and count are
 * read (the other arrays must still be non-null).  Workspace, init and reduce are phf_waic_*'s.  Serves the integrated
 * leave-one-experiment-out, whose "points" are the experiments. */
int phf_waic_accumulate_given(const phf_pointwise_points* pts, const double* rows, int64_t num_rows, int num_problems, int row_stride_cols,
                              int num_chains, int64_t first_row, int64_t total_rows, double* workspace, size_t workspace_bytes,
                              void* stream);
int phf_waic_reduce(int num_problems, int stride, int num_chains, int64_t total_rows, const double* workspace, size_t workspace_bytes,
                    double* out, void* stream);

/* ---- PSIS-LOO ----------------------------------------------------------------------------------------------------------------
 * Pareto-smoothed importance-sampling leave-one-out (Vehtari, Simpson, Gelman, Yao & Gabry, JMLR 2024; r_eff = 1) of every data point,
 * streamed like WAIC (pyhillfit_amd/csrc/phf_psis.hip; DESIGN.md §3, "PSIS-LOO").  Points, likelihoods and rows as phf_waic_*: the
 * same pointwise log-likelihood l.  Over the S = total_rows x num_chains draws of a point, with r = -l:
 *   M = ceil(min(S/5, 3 sqrt S)) (phf_psis_tail_length); the tail = the M smallest l, the cutoff = the (M+1)-th smallest;
 *   a generalised Pareto fit to the tail's exceedances exp(r) - exp(r_cutoff) (shifted by max r) by Zhang & Stephens (2009) with
 *   30 + floor(sqrt M) grid points, k-hat <- (M k-hat + 5)/(M + 10); the tail's ratios replaced by rank with the quantiles at
 *   (j - 1/2)/M, capped at the largest raw ratio; every weight truncated at S^(3/4) x the mean weight;
 *   elpd_loo_i = ln sum w exp(l) - ln sum w, lppd_i = ln mean exp(l).
 * Edge cases: M < 5 — no fit, k-hat = +inf, sigma-hat = NaN, the raw ratios truncated; a tail whose exceedances are all equal —
 * nothing to smooth, k-hat = 0, sigma-hat = 0; a draw with l = -inf (sigma <= 1e-3) — elpd_loo_i = -inf, k-hat = +inf, sigma-hat = NaN.
 *   tail_per_chain  k, the heap capacity per (point, chain), capped at min(M + 1, total_rows); 0: the default, k = min(M + 1,
 *                   total_rows) — every point exact by construction — whenever that workspace stays within 32 GiB, else
 *                   2 ceil((M + 1)/num_chains) + 32 (phf_psis_tail_per_chain returns the k in use).  k x num_chains (k x total_rows
 *                   if fewer) must reach M + 1.  A draw at or above the point's bound T on the cutoff (the bucket of the (M+1)-th smallest
 *                   value held by all heaps together, to 1/16 of a binade, recomputed after every 1024th row up to row 8192, then every 8192nd)
 *                   goes straight to the non-tail sum.
 *   workspace       device, phf_psis_workspace_bytes(...): [num_problems][stride][6][num_chains] doubles (a running max and sum of
 *                   exp(-l - max) over the draws not in the heap, the same of +l over all draws, the heap's fill count, the heap
 *                   insertions so far), then [num_problems][stride] doubles (T), then [num_problems][stride][k][num_chains]
 *                   doubles (a max-heap of the chain's k smallest l), then, when M + 1 > 8192, the reduce's sort scratch;
 *                   phf_psis_init zeroes the counts and sets T = +inf (stream-ordered)
 *   out             device [5][num_problems][stride]: elpd_loo_i, lppd_i, k-hat_i, sigma-hat_i, determined_i (1 or 0); valid once all
 *                   total_rows rows have arrived; NaN (determined 0) beyond a problem's count
 *   tail_out        NULL, or device [num_problems][stride][M + 1]: the M + 1 smallest l of each point, ascending
 * Exactness: the values a chain did not keep are all >= its final heap maximum, so the selection is exact unless some chain has a
 * full heap (that dropped draws) whose maximum lies below the cutoff: that point is NOT DETERMINED and written NaN, determined = 0.
 * Deterministic: no atomics in the accumulation, every accumulator produced by one lane in row order; the reduce selects by exact
 * integer counts and merges the chains in a fixed order.  Bit-identical however the rows are cut into calls.  An invalid shape gives
 * 0 / PHF_ERR_INVALID_ARGUMENT without touching a GPU (phf_last_error() says why). */
int64_t phf_psis_tail_length(int num_chains, int64_t total_rows);
int phf_psis_tail_per_chain(int num_problems, int stride, int num_chains, int64_t total_rows, int tail_per_chain);
size_t phf_psis_workspace_bytes(int num_problems, int stride, int num_chains, int64_t total_rows, int tail_per_chain);
int phf_psis_init(int num_problems, int stride, int num_chains, int64_t total_rows, int tail_per_chain, double* workspace,
                  size_t workspace_bytes, void* stream);
int phf_psis_accumulate(const phf_pointwise_points* pts, int likelihood, int num_expts, const double* rows, int64_t num_rows,
                        int num_problems, int row_stride_cols, int num_chains, int64_t first_row, int64_t total_rows, int tail_per_chain,
                        double* workspace, size_t workspace_bytes, void* stream);
int phf_psis_reduce(const phf_pointwise_points* pts, int num_problems, int num_chains, int64_t total_rows, int tail_per_chain,
                    double* workspace, size_t workspace_bytes, double* out, double* tail_out, void* stream);
/* phf_psis_accumulate with a GIVEN log-likelihood, as phf_waic_accumulate_given: l of point p is column p of the row. */
int phf_psis_accumulate_given(const phf_pointwise_points* pts, const double* rows, int64_t num_rows, int num_problems, int row_stride_cols,
                              int num_chains, int64_t first_row, int64_t total_rows, int tail_per_chain, double* workspace,
                              size_t workspace_bytes, void* stream);

/* ---- posterior quantiles and curve bands -------------------------------------------------------------------------------------
 * Exact-count histograms of every (problem, column) over all chains' draws, streamed like the diagnostics
 * (pyhillfit_amd/csrc/phf_quantiles.hip; DESIGN.md §3, "Posterior quantiles").  A workspace holds S = num_problems x (num_columns +
 * curve_points) slots; slot q (num_columns + curve_points) + c is column c of problem q's rows (c < num_columns) or the Hill curve
 * of problem q at dose c - num_columns.  Per slot: B = bins bins (a power of two in [64, 32768]), an anchor a (the first finite
 * value in (row, chain) order of all rows accumulated), w0 = 2^(floor(log2 max(|a|, 2^-30)) - 40) and a level k; a value x falls
 * in bin j = floor(((x - a) * (1/w0)) * 2^-k) + B/2, k being the least level whose bins hold the slot's [min, max].  So the counts
 * are those of binning every draw at the final grid, the same however the rows are cut into calls, and unless k = 0 a bin is at
 * most 4 (max - min) / B wide.  Values that are not finite (or lie beyond ~2^980 w0 of a) are counted apart, never binned.
 *   rows        device [num_rows][num_problems][row_stride_cols][num_chains] (the layout phf_diagnostics_accumulate reads);
 *               num_rows x num_chains < 2^31 per call; calls in row order, [first_row, first_row + num_rows) within total_rows
 *   ln_doses    curves: device [num_problems][curve_points], the natural log of each dose; the curve of model 1 | 2 is
 *               100 (1 - 1/(1 + exp(Hill (ln c - ln IC50)))) with pIC50 = column 0 and Hill = column 1 (model 2) or 1
 *   workspace   device, phf_quantiles_workspace_bytes(...): uint64 counts [S][bins], then double [S][8] (a, w0, min, max, level,
 *               anchored, 0, 0), then uint64 [S] non-finite counts; phf_quantiles_init zeroes it (stream-ordered)
 *   probs       HOST array of num_probs (1 to 64) probabilities in [0, 1]
 *   out         device [S][8 + 4 num_probs]: min, max, finite draws N, non-finite draws, bin width w0 2^k, k, a, w0; then per p the
 *               value (linear in rank inside the bin), the bin's edges lo, hi (clamped to [min, max]) and the bin index, for the
 *               rank r = ceil(p N) draw (clamped to [1, N]: numpy's quantile(method="inverted_cdf")); NaN where N = 0
 * Deterministic: integer counts (uint32 in LDS, uint64 atomics in HBM).  An invalid shape gives 0 bytes / PHF_ERR_INVALID_ARGUMENT
 * without touching a GPU (phf_last_error() says why). */
size_t phf_quantiles_workspace_bytes(int num_problems, int num_columns, int curve_points, int bins);
int phf_quantiles_init(int num_problems, int num_columns, int curve_points, int bins, void* workspace, size_t workspace_bytes,
                       void* stream);
int phf_quantiles_accumulate(const double* rows, int64_t num_rows, int num_problems, int row_stride_cols, int num_chains,
                             int num_columns, int curve_points, int bins, int64_t first_row, int64_t total_rows, void* workspace,
                             size_t workspace_bytes, void* stream);
int phf_quantiles_accumulate_curves(const double* rows, int64_t num_rows, int num_problems, int row_stride_cols, int num_chains,
                                    int model, const double* ln_doses, int num_columns, int curve_points, int bins, int64_t first_row,
                                    int64_t total_rows, void* workspace, size_t workspace_bytes, void* stream);
int phf_quantiles_reduce(int num_problems, int num_columns, int curve_points, int bins, const double* probs, int num_probs,
                         const void* workspace, size_t workspace_bytes, double* out, void* stream);

/* ---- dose-response bands of the hierarchical model ----------------------------------------------------------------------------
 * (pyhillfit_amd/csrc/phf_hier_bands.h, phf_quantiles.hip; DESIGN.md §3, "Hierarchical bands").  Rows are the hierarchical sampler's:
 * columns 0..3 = (alpha, beta, mu, s).  Per draw and dose the Hill curve, in percent, of
 *   the inferred underlying effect    Hill = alpha, pIC50 = mu;
 *   a predicted future experiment     Hill* = alpha exp(logit(u_H) / beta) (log-logistic), pIC50* = mu + s logit(u_P) (logistic),
 *                                     u = (k + 1/2) 2^-52 from two words of the draw's block (k = (w_a >> 6) 2^26 + (w_b >> 6)),
 * binned through the histograms above.  A workspace made with curve_points = 2 num_doses holds per problem the num_columns column
 * slots, then num_doses underlying-effect slots, then num_doses future-experiment slots; phf_quantiles_workspace_bytes, _init,
 * _accumulate (the columns) and _reduce serve it unchanged.  Random stream: one Philox block (the samplers' rounds) per draw,
 * counter = (chain_id_base + chain, problem_id[q], first_row + r, 0xC0000000), key = seed: disjoint from the samplers, the posterior
 * predictive checks and replica exchange, independent of how the rows are cut into calls (and of the dose: the doses of a draw
 * share its (Hill*, pIC50*)).  A draw with a non-finite alpha, beta, mu or s, alpha <= 0 or beta <= 0 (and, future experiment,
 * s <= 0) gives NaN: counted apart.
 *   ln_doses       device [num_problems][num_doses], the natural log of each dose
 *   problem_id     device [num_problems] uint32: the global problem number of each problem (the samplers' problem_id)
 *   row_stride_cols >= 4; total_rows <= 2^32; the rest as phf_quantiles_accumulate_curves
 * An invalid argument gives PHF_ERR_INVALID_ARGUMENT without touching a GPU (phf_last_error() says why). */
int phf_quantiles_accumulate_hier_curves(const double* rows, int64_t num_rows, int num_problems, int row_stride_cols, int num_chains,
                                         const double* ln_doses, int num_columns, int num_doses, int bins, int64_t first_row,
                                         int64_t total_rows, const uint32_t* problem_id, uint32_t chain_id_base, uint64_t seed,
                                         void* workspace, size_t workspace_bytes, void* stream);
/* Batch evaluator: draw i at theta[.][i] = (alpha, beta, mu, s) ([4][m]) with the stream counter counter[i][0..2] = (chain id,
 * problem id, row) and the key seed: out [m][2] = (Hill*, pIC50*); NaN, NaN for parameters that give no draw.  Serves the tests and
 * the chain-file tool. */
int phf_hier_band_draws(int64_t m, const double* theta, const uint32_t* counter, uint64_t seed, double* out, void* stream);

/* ---- marginal log-likelihood of whole experiments (integrated leave-one-experiment-out) -------------------------------------
 * (pyhillfit_amd/csrc/phf_hier_marginal.hip, phf_hier_marginal.h; DESIGN.md §3, "Integrated leave-one-experiment-out").  For a draw
 * phi = (alpha, beta, mu, s, sigma) = columns 0..3 and 4 + 2 num_expts of a hierarchical vector and experiment e (the points of pts
 * with tag == e, hierarchical points as for phf_waic_*), m_e = ln of the integral of the experiment's truncated-normal likelihood
 * over Hill ~ log-logistic(alpha, beta), pIC50 ~ logistic(mu, s) on pIC50 >= -2 (not renormalised for the bound), by the fixed
 * num_nodes x num_nodes rule of phf_hier_marginal.h, and g_e = |m_e - m_e of the even-even nodes|, the rule's own error estimate.
 *   nodes       device [3][num_nodes] doubles: x_k, ln w_k, ln w_k of the even nodes (pyhillfit_amd/marginal.py: node_table);
 *               num_nodes is 32, 64, 128 or 256
 *   sigma <= 1e-3 gives m = -inf, g = 0; parameters that are not finite, alpha, beta or s <= 0, or a problem index out of range
 *   give NaN, NaN.  An experiment without points gives m = ln of the mass of the nodes with pIC50 >= -2.
 * num_expts is 1..64; at most 512 points per problem (stride).  One wavefront per (draw, experiment), no atomics: bit-identical to
 * the host build of phf_hier_marginal.h.  An invalid argument gives PHF_ERR_INVALID_ARGUMENT without touching a GPU
 * (phf_last_error() says why). */
/* Batch evaluator: theta [5 + 2 num_expts][m], problem_index [m]; out [2][m][num_expts] = m_e, then g_e.  Serves the tests and the
 * chain-file tool. */
int phf_hier_marginal_loglik(const phf_pointwise_points* pts, int num_expts, const double* nodes, int num_nodes, int64_t m,
                             const int32_t* problem_index, const double* theta, double* out, void* stream);
/* the number of rows r in [first_row, first_row + num_rows) with r mod every == 0 (-1 for an invalid argument) */
int64_t phf_hier_marginal_rows_used(int64_t first_row, int64_t num_rows, int every);
/* Streaming: rows device [num_rows][num_problems][row_stride_cols][num_chains] (the hierarchical sampler's row buffer or a slice of
 * it), rows[0] being global post-burn-in row first_row.  Exactly the global rows r with r mod every == 0 are used, however the calls
 * cut the rows: with U = phf_hier_marginal_rows_used(first_row, num_rows, every),
 *   loglik, gap   device [U][num_problems][num_expts][num_chains]: m_e and g_e of the call's used rows, in row order
 *   gap_max       device [num_problems][num_expts][num_chains]: the running per-chain maximum of g_e, updated in place (the caller
 *                 zeroes it before the first call; NaN gaps are passed over; the chains are the caller's to fold, a maximum
 *                 has no rounding) */
int phf_hier_marginal_rows(const phf_pointwise_points* pts, int num_expts, const double* nodes, int num_nodes, const double* rows,
                           int64_t num_rows, int num_problems, int row_stride_cols, int num_chains, int64_t first_row, int every,
                           double* loglik, double* gap, double* gap_max, void* stream);

/* ---- posterior predictive checks ----------------------------------------------------------------------------------------------
 * (pyhillfit_amd/csrc/phf_ppc.hip, phf_ppc.h; DESIGN.md §3, "Posterior predictive checks").  Points, likelihoods and rows as
 * phf_waic_*.  Per draw (a row of a chain) and point, one replicated response y_rep:
 *   single-level   clamp(pred + sigma z, 0, 100), z the generator's normal of one word (|z| <= 6.34);
 *   hierarchical   the truncated normal on [0, 100] by inversion, pred + sigma ndtri(Phi(a) + u (Phi(b) - Phi(a))), clamped.
 * Random stream: one Philox block (the samplers' rounds) per (draw, 4 points), counter = (chain_id_base + chain, problem_id[q], row,
 * 0x80000000 | point block), key = seed: disjoint from every sampler draw (their word 3 is a small block index), independent of how
 * the rows are cut into calls.  Test quantities T, of y and of y_rep under the same theta, in this order: deviance -2 sum l,
 * mean, sd (divisor n - 1; 0 for n = 1), #zeros, #hundreds.  A draw with sigma <= 1e-3 (or NaN) is counted invalid and left out.
 *   problem_id     device [num_problems] uint32: the global problem number of each problem (the samplers' problem_id)
 *   workspace      device, phf_ppc_workspace_bytes(...) = num_problems * (21 + stride) * num_chains doubles; phf_ppc_init zeroes it
 *   out            device [num_problems][21 + stride] (sums over all chains): for statistic s, at 4 s + 0..3: #{T(y_rep) > T(y)},
 *                  #{T(y_rep) = T(y)}, sum T(y_rep), sum T(y); at 20 the number of invalid draws; at 21 + p the sum over the valid
 *                  draws of P(y_rep < y_p | theta) + P(y_rep = y_p | theta)/2 (the predictive PIT, analytic; 0 beyond count)
 * At most 512 points per problem (stride).  Deterministic: exact counts, every sum owned by one lane in row order, the chains
 * merged in a fixed order, no atomics: bit-identical however the rows are cut into calls.  An invalid shape gives 0 bytes /
 * PHF_ERR_INVALID_ARGUMENT without touching a GPU (phf_last_error() says why). */
size_t phf_ppc_workspace_bytes(int num_problems, int stride, int num_chains, int64_t total_rows);
int phf_ppc_init(int num_problems, int stride, int num_chains, int64_t total_rows, double* workspace, size_t workspace_bytes,
                 void* stream);
int phf_ppc_accumulate(const phf_pointwise_points* pts, int likelihood, int num_expts, const double* rows, int64_t num_rows,
                       int num_problems, int row_stride_cols, int num_chains, int64_t first_row, int64_t total_rows,
                       const uint32_t* problem_id, uint32_t chain_id_base, uint64_t seed, double* workspace, size_t workspace_bytes,
                       void* stream);
int phf_ppc_reduce(int num_problems, int stride, int num_chains, int64_t total_rows, const double* workspace, size_t workspace_bytes,
                   double* out, void* stream);
/* Batch evaluator: vector i of problem problem_index[i] at theta[.][i] ([d][m], as phf_pointwise_loglik_*) with the stream counter
 * counter[i][0..2] = (chain id, problem id, row) and the key seed: y_rep [m][stride] (NaN beyond the count) and stats [m][2][5]
 * (T(y), then T(y_rep)); all NaN for an invalid theta or problem index.  Serves the tests and the chain-file tool. */
int phf_ppc_replicate(const phf_pointwise_points* pts, int likelihood, int num_expts, int64_t m, const int32_t* problem_index,
                      const double* theta, const uint32_t* counter, uint64_t seed, double* y_rep, double* stats, void* stream);

/* ---- stepping-stone evidence of the tempered ladder ------------------------------------------------------------------------
 * Streaming accumulator (pyhillfit_amd/csrc/phf_stepping_stone.hip; DESIGN.md §3, "phf_stepping_stone.hip").  Problem q is one rung
 * (pair pair_index[q] of pts, the sampler's merged entries) with delta[q] = t_k+1 - t_k (0 for the last rung).  Over chain c's n rows,
 * with l = log L(theta; t = 1) of phf_sl_log_target (pi_bit included: the sampler's own ll1):
 *   log r_c = ln sum_j exp(delta l_j) - ln n;  pooled log r = LSE_c(log r_c) - ln C;  se = sd_c(r_c / r) / sqrt(C) (divisor C - 1);
 *   ESS = (sum w)^2 / sum w^2 over all C n draws, w = exp(delta l - max).
 * l = -inf is weight 0 (delta > 0); delta = 0 gives every draw weight 1 (log r = 0 exactly); a NaN l makes its chain's log r NaN.
 *   model       1 | 2: theta = columns 0..model of a row
 *   rows        device [num_rows][num_problems][row_stride_cols][num_chains] — the single-level sampler's row buffer or a slice of it
 *   first_row   index of rows[0] among the total_rows rows; calls come in row order, each row exactly once
 *   workspace   device, phf_stepping_stone_workspace_bytes(...) = num_problems * 5 * num_chains doubles: per (problem, field, chain)
 *               the running max m of delta l, sum exp(delta l - m), sum exp(2 (delta l - m)), sum l and the rows seen;
 *               phf_stepping_stone_init zeroes it (stream-ordered) before the first accumulate
 *   out         device [num_problems][7]: pooled log r, se (NaN for one chain), chain 0's log r, ESS, rows per chain, mean l over all
 *               draws, chains whose log r is NaN; valid once all total_rows rows have arrived
 * A pair_index outside [0, num_pairs) makes that problem's results NaN (no access out of bounds).  Deterministic: no atomics, every
 * accumulator is produced by one lane in row order and round-trips through HBM exactly; the chains are merged in a fixed order.
 * Bit-identical however the rows are cut into calls.  An invalid shape gives 0 bytes / PHF_ERR_INVALID_ARGUMENT without touching a
 * GPU (phf_last_error() says why). */
size_t phf_stepping_stone_workspace_bytes(int num_problems, int num_chains, int64_t total_rows);
int phf_stepping_stone_init(int num_problems, int num_chains, int64_t total_rows, double* workspace, size_t workspace_bytes, void* stream);
int phf_stepping_stone_accumulate(const phf_points* pts, int model, const int32_t* pair_index, const double* delta, const double* rows,
                                  int64_t num_rows, int num_problems, int row_stride_cols, int num_chains, int64_t first_row,
                                  int64_t total_rows, double* workspace, size_t workspace_bytes, void* stream);
int phf_stepping_stone_reduce(int num_problems, int num_chains, int64_t total_rows, const double* workspace, size_t workspace_bytes,
                              double* out, void* stream);
/* The standard error of a pair's log Z when its rungs are NOT independent (replica exchange: chain c of every rung is one replica set).
 * Problems p*R .. p*R + R-1 are pair p's rungs in order (num_problems = num_pairs * rungs_per_pair); reduced is phf_stepping_stone_reduce's
 * out.  Per chain v_c = sum_k<R-1 exp(log r_kc - log r_k); out[p] = sd_c(v_c) / sqrt(C) (divisor C - 1; NaN for one chain): the delta
 * method over the C independent replica sets.  One wavefront per pair, chains merged in a fixed order. */
int phf_stepping_stone_reduce_joint(int num_pairs, int rungs_per_pair, int num_chains, int64_t total_rows, const double* workspace,
                                    size_t workspace_bytes, const double* reduced, double* out, void* stream);

/* ---- replica exchange between the rungs of a tempered ladder ----------------------------------------------------------------
 * (pyhillfit_amd/csrc/phf_replica_exchange.hip; DESIGN.md §3, "phf_replica_exchange.hip").  prob is the single-level sampler's batch
 * with num_problems = P * rungs_per_pair, pair-major, rungs in temperature order; state its [S][Q*C] state.  Round `round` (>= 1)
 * proposes the rung pairs (k, k+1), k = round (mod 2), chain c with chain c, and accepts iff log u < (t_k+1 - t_k)(l_k - l_k+1), l the
 * state's untempered log-likelihood; on accept theta and l change slots and each slot's log-target is recomputed at its temperature
 * as (t == 0 ? 0 : t l) + log-prior (the sampler's own arithmetic).  u = phf_uniform53 of the Philox block counter = (chain id,
 * problem id of rung k, round, 0x40000000), key = seed.
 *   labels   device int32 [Q*C], moves with the states: bits 0..27 the starting rung, bit 30 visited rung 0, bit 29 reached rung R-1
 *            since (phf_replica_exchange_labels_init sets rung k's slots to k, rung 0's with bit 30)
 *   stats    device, phf_replica_exchange_stats_bytes(...): int64 attempts and accepts per (pair, rung pair, 64-chain group) and round
 *            trips 0 -> R-1 -> 0 per (pair, chain); phf_replica_exchange_stats_init zeroes it
 *   trace    device double [P][R-1][C][3] or NULL: (u, log u, log alpha) of every proposed (pair, rung pair, chain) (tests)
 * phf_replica_exchange_stats_read writes int64 attempts [P][R-1], accepts [P][R-1], round trips [P][C] to out (device).
 * Deterministic: every slot and counter has one writer per round; no atomics. */
size_t phf_replica_exchange_stats_bytes(int num_pairs, int rungs_per_pair, int num_chains);
int phf_replica_exchange_stats_init(int num_pairs, int rungs_per_pair, int num_chains, int64_t* stats, size_t stats_bytes, void* stream);
int phf_replica_exchange_stats_read(int num_pairs, int rungs_per_pair, int num_chains, const int64_t* stats, size_t stats_bytes,
                                    int64_t* out, void* stream);
int phf_replica_exchange_labels_init(int num_pairs, int rungs_per_pair, int num_chains, int32_t* labels, void* stream);
int phf_replica_exchange_round(const phf_problems* prob, int model, int rungs_per_pair, int64_t round, uint64_t seed, double* state,
                               int32_t* labels, int64_t* stats, size_t stats_bytes, double* trace, void* stream);

/* ---- differential-evolution moves between the chains of a pair of the hierarchical sampler ----------------------------------
 * (pyhillfit_amd/csrc/phf_hier_de.hip, phf_hier_de.h; DESIGN.md §3, "Differential-evolution moves"; ter Braak 2006).  pts, prob, prior
 * and state are the hierarchical sampler's.  The chains of a problem form populations of `population` = 4, 8, 16, 32 or 64 consecutive
 * chains by global chain number (chain_id_base + chain_offset[q] + c; chains_per_problem, chain_id_base and every chain_offset must be
 * multiples of it).  Round `round` (1 <= round < 2^32) is two launches in stream order, sub-round h = 0 then 1: the chains whose index
 * within the population has parity h move, the n = population / 2 chains of the other parity are donors and are only read.  With
 * w0..w3 the Philox block counter = (global chain id, problem id, round, 0x20000000 | h), key = seed:
 *   a' = floor(w0 n / 2^32), b' = floor(w1 (n-1) / 2^32), b' += (b' >= a'); donors a = min, b = max; sign from the top bit of w2;
 *   x' = x + (sign gamma)(x_a - x_b), one subtraction, multiplication and addition per coordinate;
 *   accept iff log u < L(x') - L(x), u = (w3 + 1/2) / 2^32, L(x) the state's log-target, L(x') the sampler's own target function.
 * A NaN or L(x') = -inf rejects.  On accept theta and the log-target of the state change: mean, factor, loga and the sampler's accepted
 * count do not.  The proposal is symmetric, so a round leaves the product of the chains' posteriors invariant; chains of one
 * population are no longer independent of each other afterwards, populations stay independent.
 *   gamma      > 0; gamma == 1.0 exactly marks a mode-jumping round (counted apart)
 *   workspace  device, phf_hier_de_workspace_bytes(n_expts, Q, C) = (5 + 2 n_expts) Q C doubles: the proposals (scratch between launches)
 *   stats      device, phf_hier_de_stats_bytes(Q, C): int64 attempts and accepts per (kind of round, problem, 64-chain block), kind 0 =
 *              ordinary, 1 = gamma == 1; one writer per counter, no atomics; phf_hier_de_stats_init zeroes it
 *   trace      device double [Q][C][6] or NULL: donor chains a and b (numbers within the problem), sign gamma, log u, L(x'), accepted
 * phf_hier_de_stats_read writes int64 [2 kinds][attempts, accepts][Q] to out (device), the chain blocks summed in order.
 * Every argument is checked before any launch: PHF_ERR_INVALID_ARGUMENT / 0 bytes without touching a GPU (phf_last_error() says why). */
size_t phf_hier_de_workspace_bytes(int n_expts, int num_problems, int num_chains);
size_t phf_hier_de_stats_bytes(int num_problems, int num_chains);
int phf_hier_de_stats_init(int num_problems, int num_chains, int64_t* stats, size_t stats_bytes, void* stream);
int phf_hier_de_stats_read(int num_problems, int num_chains, const int64_t* stats, size_t stats_bytes, int64_t* out, void* stream);
int phf_hier_de_round(const phf_hier_points* pts, const phf_problems* prob, const phf_hier_prior* prior, int64_t round, uint64_t seed,
                      int population, double gamma, double* state, double* workspace, size_t workspace_bytes, int64_t* stats,
                      size_t stats_bytes, double* trace, void* stream);

/* ---- power-scaling sensitivity of prior and likelihood ----------------------------------------------------------------------
 * (pyhillfit_amd/csrc/phf_sensitivity.hip, phf_sensitivity.h; DESIGN.md §3, "Power-scaling sensitivity"; Kallioinen, Paananen,
 * Buerkner & Vehtari 2023).  Scaling a component c(theta) of the log-target by alpha re-weights every draw by exp((alpha - 1) c); the
 * components are the log-prior and the log-likelihood, the directions alpha = 1/(1 + delta) and 1 + delta, 0 < delta <= 0.25.
 *   kind 1 | 2   single-level model 1 | 2, theta = columns 0..model of a row, sl_points = the sampler's merged entries (pair q <->
 *                problem q): prior = phf_sl_log_prior, likelihood = the untempered log-likelihood, their sum the log-target at t = 1;
 *   kind 3       hierarchical, hier_points (n_expts = Ne, pair q <-> problem q) and prior: prior = the five Gamma hyper-priors,
 *                likelihood = the truncated-normal data term; the population terms belong to neither;
 *   kind 4       given: columns prior_column and likelihood_column of the row are the two components (points and prior unused).
 * Per (problem, component) c_ref = the first finite component in (row, chain) order of all rows accumulated; a draw's weight is
 * w = exp(clamp((alpha - 1)(c - c_ref), -8, 8)), its integer mass floor(w 2^20 + 1/2).  A draw whose component is not finite enters
 * nothing of that component.  Per (problem, column) slot, columns 0..num_columns-1 of the rows, on one grid by the quantiles' rule
 * (anchor, w0, least level holding [min, max]): the base counts and the four mass arrays (prior down, prior up, likelihood down,
 * likelihood up), uint64 — identical however the rows arrive or are cut into calls.  Per (problem, weight, chain), in row order:
 * n, sum w, sum w^2, clamped draws; per (slot, array, chain): sum w, sum w d, sum w d^2, d = x - the slot's anchor (array 0: w = 1).
 *   rows        device [num_rows][num_problems][row_stride_cols][num_chains]; calls in row order, [first_row, first_row + num_rows)
 *               within total_rows; total_rows x num_chains <= 2^32
 *   bins        a power of two in [64, 4096]
 *   workspace   device, phf_sensitivity_workspace_bytes(...): the slots' arrays, the sums, and a scratch region of about 256 MiB (at
 *               least 16 rows, at most total_rows) through which an accumulate call walks its rows in blocks; phf_sensitivity_init zeroes it (stream-ordered)
 *   out_slots   device [S][28], S = num_problems x num_columns: min, max, binned draws, non-finite values, bin width, level, anchor,
 *               w0; then per weight the sums of the cumulative Jensen-Shannon divergence over the bins from the first to the last one
 *               holding a draw — numerator and denominator on the CDF, numerator and denominator on the survival function — and the
 *               total mass (phf_sens_cjs_sums)
 *   out_weights device [num_problems][4][4]: per weight n, sum w, sum w^2, clamped draws, the chains merged in chain order
 *   out_columns device [S][5][4]: per array sum w, sum w d, sum w d^2 merged in chain order, and the between-chain standard error of
 *               the weighted mean's shift from the base mean (in units of x; NaN for array 0 or fewer than two chains)
 *   out_per_chain  NULL, or device [num_problems][4][4][num_chains] then [S][5][3][num_chains] doubles: the per-chain sums (tests)
 * Every argument is checked before any launch: PHF_ERR_INVALID_ARGUMENT / 0 bytes without touching a GPU (phf_last_error() says why). */
size_t phf_sensitivity_workspace_bytes(int num_problems, int num_columns, int num_chains, int64_t total_rows, int bins);
int phf_sensitivity_init(int num_problems, int num_columns, int num_chains, int64_t total_rows, int bins, void* workspace,
                         size_t workspace_bytes, void* stream);
int phf_sensitivity_accumulate(int kind, const phf_points* sl_points, const phf_hier_points* hier_points, const phf_hier_prior* prior,
                               int prior_column, int likelihood_column, const double* rows, int64_t num_rows, int num_problems,
                               int row_stride_cols, int num_chains, int num_columns, double delta, int bins, int64_t first_row,
                               int64_t total_rows, void* workspace, size_t workspace_bytes, void* stream);
int phf_sensitivity_reduce(int num_problems, int num_columns, int num_chains, int64_t total_rows, int bins, const void* workspace,
                           size_t workspace_bytes, double* out_slots, double* out_weights, double* out_columns, double* out_per_chain,
                           void* stream);
/* Batch evaluator: theta [d][m] (d = kind + 1, or 5 + 2 Ne), problem_index [m]; out [3][m] = prior, likelihood, and the population
 * term (0 for the single-level models); NaN for a problem index out of range.  Serves the tests and the chain-file tool. */
int phf_sensitivity_components(int kind, const phf_points* sl_points, const phf_hier_points* hier_points, const phf_hier_prior* prior,
                               int64_t m, const int32_t* problem_index, const double* theta, double* out, void* stream);

/* ---- expected information gain of a next dose ---------------------------------------------------------------------------------
 * (pyhillfit_amd/csrc/phf_design.hip, phf_design.h; DESIGN.md §3, "Next dose"; Lindley 1956, Chaloner & Verdinelli 1995).  For the
 * single-level models (model 1 | 2, theta = columns 0..model of a row) and num_doses candidate doses per problem, the sums over the
 * draws of what the mutual information between one further response at the dose and the parameters needs, the response being
 * recorded to a resolution of 100/bins % block: the bins + 2 category masses of the censored normal (point masses at 0 and 100, bins
 * equal bins of (0, 100)), the entropy of the draw's masses, and the entropy over the partition that merges adjacent bin pairs.
 *   bins          128, 256, 512 or 1024
 *   rows          device [num_rows][num_problems][row_stride_cols][num_chains], rows[0] being global post-burn-in row first_row;
 *                 exactly the global rows r with r mod every == 0 are used, however the calls cut the rows
 *   ln_doses      device [num_problems][num_doses] doubles: the natural logarithm of the candidate doses (uM)
 *   num_slots     even, 2..64: chain c goes to accumulator slot c mod num_slots (so a slot's chains share the parity c & 1)
 *   accumulators  device [num_problems][num_doses][num_slots][phf_design_accumulator_doubles(bins)] doubles, zeroed by the caller
 *                 before the first call and updated in place: the mass at 0, the bins' masses, the mass at 100, per lane the sum of
 *                 the fine entropies' shares [64] and of the coarse ones [64], the draws used, the draws skipped (phf_design.h)
 * A draw with sigma <= 1e-3 or a parameter that is not finite is skipped and counted.  Every sum is a plain left-to-right sum over the
 * slot's draws in (row, chain) order that starts from the stored value: the same rows and the same `every` give the same bits
 * however the calls cut them, bit-identical to the host build of phf_design.h.  No atomics.  A call that holds no used row launches
 * nothing.  Every argument is checked before any launch: PHF_ERR_INVALID_ARGUMENT without touching a GPU (phf_last_error() says why). */
int phf_design_accumulator_doubles(int bins);   /* -1 for a bin count that is not allowed */
/* the number of rows r in [first_row, first_row + num_rows) with r mod every == 0 (-1 for an invalid argument) */
int64_t phf_design_rows_used(int64_t first_row, int64_t num_rows, int every);
int phf_design_accumulate(int model, int bins, const double* rows, int64_t num_rows, int num_problems, int row_stride_cols,
                          int num_chains, int64_t first_row, int every, const double* ln_doses, int num_doses, int num_slots,
                          double* accumulators, size_t accumulator_bytes, void* stream);

/* ---- Savage-Dickey Bayes factor B12 of "Hill = 1" (model 1) against "Hill free" (model 2) -------------------------------------
 * (pyhillfit_amd/csrc/phf_savage_dickey.hip, phf_savage_dickey.h; DESIGN.md §3, "Savage-Dickey Bayes factor").  From the t = 1 draws
 * of the MODEL-2 fit alone — what python/compute_bayes_factors.py:11-27 reaches through a 41-rung tempered ladder per pair and model:
 * B12 = p(Hill = 1 | y, M2) / pi(Hill = 1 | M2) = the posterior mean of
 *   r = L(pIC50, 1, sigma) / ((1/10) INT_0^10 L(pIC50, h, sigma) dh),
 * the integral by a fixed rule at the draw's (pIC50, sigma): [0, 10] in `panels` equal panels, the 15-point Gauss-Kronrod rule on
 * each (fine), its 7 embedded Gauss nodes (coarse).  The draw's Hill column is not read.  Valid only while model 1 is model 2 at
 * Hill = 1 with the same priors on pIC50 and sigma and a uniform prior on Hill (asserted in phf_savage_dickey.h).
 *   pts           the sampler's merged entries, pair q <-> problem q (pi_bit and extra are not read); stride <= 256
 *   panels        16, 32 or 64
 *   nodes         device [3][15 panels] doubles: h_k, ln w_k (fine), ln w_k (coarse, -inf at the nodes that are no Gauss nodes),
 *                 made on the host (pyhillfit_amd/savage_dickey.py: node_table)
 *   rows          device [num_rows][num_problems][4][num_chains], model-2 rows (pIC50, Hill, sigma, log-target): row_stride_cols must
 *                 be 4; rows[0] is global post-burn-in row first_row, and exactly the global rows r with r mod every == 0 are used,
 *                 however the calls cut the rows
 *   accumulators  device [num_problems][num_chains][8] doubles, zeroed by the caller before the first call and updated in place:
 *                 draws used, draws skipped, SUM r_fine, SUM r_fine^2, max r_fine, SUM r_coarse, max |log r_fine - log r_coarse|, 0
 * A draw with sigma <= 1e-3, or whose pIC50 or sigma is not finite, is skipped and counted.  Every sum is a plain left-to-right sum
 * over the chain's used rows in row order that starts from the stored value: the same rows and the same `every` give the same bits
 * however the calls cut them, bit-identical to the host build of phf_savage_dickey.h.  No atomics; nothing is merged across chains.
 * A call that holds no used row launches nothing.  Every argument is checked before any launch: PHF_ERR_INVALID_ARGUMENT without
 * touching a GPU (phf_last_error() says why). */
int phf_savage_dickey_accumulator_doubles(void);   /* 8 */
int phf_savage_dickey_nodes(int panels);           /* 15 panels; -1 for a panel count that is not allowed */
/* the number of rows r in [first_row, first_row + num_rows) with r mod every == 0 (-1 for an invalid argument) */
int64_t phf_savage_dickey_rows_used(int64_t first_row, int64_t num_rows, int every);
int phf_savage_dickey_accumulate(const phf_points* pts, int panels, const double* nodes, const double* rows, int64_t num_rows,
                                 int num_problems, int row_stride_cols, int num_chains, int64_t first_row, int every,
                                 double* accumulators, size_t accumulator_bytes, void* stream);

/* ---- Drug profile: the joint multi-channel block of a drug at given concentrations ------------------------------------------------
 * (pyhillfit_amd/csrc/phf_drug_profile.hip, phf_drug_profile.h; DESIGN.md §3, "Drug profile").  A drug has num_channels channel
 * places; channel_problem[drug][k] names the problem whose single-level rows hold the fit of channel k, -1 (or anything outside
 * [0, num_problems)) when it was not loaded.  Row r, chain c of every loaded channel side by side is one draw of the drug's joint
 * posterior.  Per draw and dose j: block_k = 100 (1 - 1/(1 + exp(Hill_k (ln c_j - ln IC50_k)))) as phf_quantiles_accumulate_curves
 * computes it, net = SUM_k weights[k] block_k over the loaded channels in order (plain multiplies and adds), dominant = the least k
 * with the largest block_k.  A draw in which a loaded channel's pIC50 or Hill is not finite is counted as non-finite in that
 * channel's slots and the net slot, and as skipped in the tallies.
 *   workspace   device, phf_drug_profile_workspace_bytes(...): first a quantiles workspace (above) of num_drugs problems, no columns
 *               and num_doses (num_channels + 1) curve points — slot (drug, j, k) is curve point j (num_channels + 1) + k, k =
 *               num_channels the net block; the slots of a channel that was not loaded stay empty — then, at
 *               phf_drug_profile_tally_offset(...) bytes, uint64 [num_drugs][num_doses][2][num_channels + 3]: per chain parity (chain
 *               index & 1) the draws whose dominant channel is k, the draws with net > 0, the draws used, the draws skipped
 *   rows        device [num_rows][num_problems][row_stride_cols][num_chains], column 0 pIC50 and, model 2, column 1 Hill
 *   channel_problem, weights, ln_doses   device int32 [num_drugs][num_channels], double [num_channels], double [num_drugs][num_doses]
 *               (natural log of the dose in uM; a drug with fewer doses than num_doses has NaN in the places it does not use: their
 *               slots and tallies stay empty)
 *   num_channels <= 16, num_doses <= 16, bins a power of two in [64, 32768], num_rows x num_chains < 2^31 per call
 * phf_drug_profile_reduce writes what phf_quantiles_reduce writes for those curve points, [slots][8 + 4 num_probs], by calling it.
 * Everything kept is an integer count: the workspace is bit-identical however the rows are cut into calls.  Every argument is checked
 * before any launch: PHF_ERR_INVALID_ARGUMENT without touching a GPU (phf_last_error() says why). */
size_t phf_drug_profile_workspace_bytes(int num_drugs, int num_channels, int num_doses, int bins);   /* 0 for an invalid shape */
size_t phf_drug_profile_tally_offset(int num_drugs, int num_channels, int num_doses, int bins);      /* 0 for an invalid shape */
/* the default weight of a channel by its name: +1 hERG, KvLQT1_mink, Kv4.3, Kir2.1; -1 Nav1.5-peak, Nav1.5-late, Cav1.2; else 0 */
double phf_drug_profile_default_weight(const char* channel);
int phf_drug_profile_init(int num_drugs, int num_channels, int num_doses, int bins, void* workspace, size_t workspace_bytes,
                          void* stream);
int phf_drug_profile_accumulate(const double* rows, int64_t num_rows, int num_problems, int row_stride_cols, int num_chains, int model,
                                int num_drugs, int num_channels, int num_doses, const int32_t* channel_problem, const double* weights,
                                const double* ln_doses, int bins, int64_t first_row, int64_t total_rows, void* workspace,
                                size_t workspace_bytes, void* stream);
int phf_drug_profile_reduce(int num_drugs, int num_channels, int num_doses, int bins, const double* probs, int num_probs,
                            const void* workspace, size_t workspace_bytes, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PYHILLFIT_AMD_H */

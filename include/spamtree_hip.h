/* spamtree_hip.h -- C-ABI of the MI355X (gfx950) build of spamtree's per-Gibbs-sweep DAG-node hot path.
 *
 * The boundary sits UNDER the reference's `SpamTreeMV` model object (/root/reference/src/spamtree_model.h:22-212):
 * each entry point replaces one of its hot methods; the host driver above it (spamtree_mv_mcmc,
 * /root/reference/src/spamtree_fit.cpp:5-430) keeps owning the RNG, the Metropolis step and the outputs.
 * Plain pointers and sizes only; no C++ / torch types.  All matrices are column-major doubles (Armadillo's
 * layout), all index vectors int64 and 0-based unless stated, rows are in the order R hands them to C++
 * (sorted by coordinates, /root/reference/R/spamtree_fit.R:267-269).  Pointers are borrowed for the call only;
 * the handle owns every device allocation.  One host thread per handle; the handle is not re-entrant.
 *
 * Return value of every function: 0 = ok; 1/2/3 = Cholesky failed in phase A at the root / a reference block /
 * a non-reference row (the reference's `errtype`, spamtree_model.cpp:876, 919, 958); 10/11 = Cholesky failed in
 * the w sweep (spamtree_model.cpp:1056, 1135); negative = usage / HIP error (st_last_error() has the text).
 * No exception crosses this boundary.  tests/test_gpu_failure_routes.py pins these codes against the oracle with every
 * phase-A and sweep kernel as the one that fails, on every path the failure word takes back to the caller.
 */
#ifndef SPAMTREE_HIP_H
#define SPAMTREE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ST_OK 0
#define ST_ERR_CHOL_ROOT 1
#define ST_ERR_CHOL_REF 2
#define ST_ERR_CHOL_LEAF 3
#define ST_ERR_CHOL_SAMPLE_REF 10
#define ST_ERR_CHOL_SAMPLE_LEAF 11
#define ST_ERR_USAGE (-1)
#define ST_ERR_HIP (-2)
#define ST_ERR_TOPOLOGY (-3)
#define ST_ERR_UNSUPPORTED (-4)

#define ST_MAX_Q 6          /* outcomes (theta has 3q + (q>2?3:1) + q(q-1)/2 <= 39 entries) */
#define ST_MAX_P 64         /* regressors: st_create refuses a problem with more (one pass of eight columns each through the statistics kernel) */
#define ST_MAX_ANCESTORS 24 /* tree depth - 1 */

typedef struct st_handle_s *st_handle;

/* Inputs of the SpamTreeMV constructor (spamtree_model.cpp:8-37) that the hot path needs.
 * Topologies beyond the tree builder's regular ones are supported (tests/tree_mutations.py builds them): a block may hang from
 * any shallower reference level, as long as parents(u) = parents(last parent) + [last parent], so the blocks of one level may
 * have chains of different lengths; blocks of one level may have any widths; a block may be empty or hold NA rows only (a
 * prediction block: it needs a parent, has no cache -- st_get_block refuses it with "block has no observations, hence no
 * cache" -- and its entries of st_get_comps are 0); a reference block may have from none to 64 direct child groups.  Sharded
 * handles (world > 1) need every block below the cut level to descend from a block on it, and a rank's blocks contiguous in
 * every level: st_create refuses a level-skipping tree there by name. */
typedef struct st_problem {
  int64_t n_all;               /* rows (observed + NA)                                   coords.n_rows            */
  int32_t d;                   /* coordinate columns, must be 2                           coords.n_cols            */
  int32_t q;                   /* outcomes                                                unique(mv_id)            */
  int32_t p;                   /* regressors, 1 .. ST_MAX_P                               X.n_cols                 */
  int32_t n_groups;            /* length of res_is_ref                                                             */
  int64_t n_blocks;            /*                                                         block_names.n_elem       */
  const double *y;             /* n_all, NaN = NA                                         y_in                     */
  const double *X;             /* n_all x p column-major                                  X_in                     */
  const double *coords;        /* n_all x d column-major                                  coords_in                */
  const int64_t *mv_id;        /* n_all, 1-based outcome id                               mv_id_in                 */
  const int64_t *res_is_ref;   /* n_groups flags, indexed by level rank                   res_is_ref_in            */
  const int64_t *block_names;  /* n_blocks, 1-based ids                                   block_names_in           */
  const int64_t *block_groups; /* n_blocks, level ("res") of block id-1                   block_groups_in          */
  const int64_t *indexing_ptr; /* n_blocks+1 CSR offsets                                  indexing_in (field)      */
  const int64_t *indexing_idx; /* row ids of each block, ascending                                                 */
  const int64_t *parents_ptr;  /* n_blocks+1                                              parents_in (field)       */
  const int64_t *parents_idx;  /* ancestor block ids, ascending (root first)                                       */
  const int64_t *children_ptr; /* n_blocks+1, may be NULL (derived from parents)          children_in (field)      */
  const int64_t *children_idx; /* all non-empty descendants, ascending; may be NULL                                */
} st_problem;

typedef struct st_options {
  int32_t device;              /* HIP device ordinal                                                               */
  int32_t reference_quirks;    /* 1 = reproduce spamtree_model.cpp:1375 (Q3: beta uses subset positions on full w) */
  int32_t rank;                /* multi-GPU: this process' rank ...                                                */
  int32_t world;               /* ... of `world` processes sharing one problem (1 = single GPU); see the end of this file */
  int32_t force_generic;       /* 1 = use the global-scratch kernels even where the LDS kernels fit (testing)      */
  int32_t reserved;            /* bit 0: recompute the theta-only Gram part of the messages on every sweep, as the
                                  reference does (need_update is always true, spamtree_fit.cpp:184); default 0 caches it
                                  per accepted theta -- identical values
                                  bit 1: limited_tree = TRUE (spamtree_fit.cpp:20, spamtree_model.cpp:901-903, 1275-1278):
                                  parents(u) is the single parent of make_edges_limited (tree_dep.cpp:133-186), children(u)
                                  the direct children, and Kxx_inv(u) = inv_sympd(K_uu); sharded like full trees since round 3
                                  bit 2: st_factor_enqueue(1, ...) factorises the quad leaf levels in full; default 0 defers
                                  their panels' T to the first reader of the slot (see st_factor_enqueue) -- identical results */
} st_options;

/* ---- lifetime: SpamTreeMV::SpamTreeMV (spamtree_model.cpp:8-192) incl. init_indexing/init_finalize/init_model_data */
int st_create(const st_problem *pb, const st_options *opt, st_handle *out);
int st_destroy(st_handle h);
const char *st_last_error(st_handle h); /* h may be NULL: error text of the last failed st_create */

/* ---- state the driver reads / writes directly in the reference (public fields w, Bcoeff, tausq_inv) */
int st_set_w(st_handle h, const double *w);                /* n_all, model row order */
int st_get_w(st_handle h, double *w);
int st_set_beta(st_handle h, const double *Bcoeff);        /* p x q column-major; recomputes XB (spamtree_model.cpp:127, 1382) */
int st_set_tausq_inv(st_handle h, const double *tausq_inv);/* q (spamtree_model.cpp:118, 1405-1407) */
int st_get_xb(st_handle h, double *xb);                    /* n_all */
/* inspection: the whitened residuals e = Ri (w_u - H_u w_pa) of the reference blocks, as the last st_factor / st_factor_local /
 * st_factor_enqueue (either slot) stored them for the leaf levels below; n = n_all, model row order, 0 at other rows.
 * limited_tree: chol(K_uu)^{-1} w_u of the blocks that have children. */
int st_get_resid(st_handle h, double *out, int64_t n);

/* ---- phase A: theta_update + get_loglik_comps_w(data) (spamtree_model.cpp:834-998, 1420-1422).
 * slot 0 = param_data, 1 = alter_data.  Returns 0 (the reference's `true`) or 1/2/3 (`false`, errtype);
 * *loglik = data.loglik_w (undefined on failure).  theta has ntheta = 3q + (q>2?3:1) + q(q-1)/2 entries. */
int st_factor(st_handle h, int slot, const double *theta, int ntheta, double *loglik);
/* st_factor in two halves: _enqueue starts the work (one GPU: every launch and the copy of the results; with a communicator
 * attached: nothing yet), _finish waits and returns what st_factor returns.  In between the caller may issue calls that do not
 * touch the slot -- the C++ driver draws tausq / beta from the sweep's statistics and uploads them (st_tausq_stats, st_beta_stats,
 * st_set_tausq_inv, st_set_beta: none of them waits for the main stream), so that the Metropolis step's host round trip
 * (src/spamtree_fit.cpp:232-262, then :308-330) is the only one of the iteration.  No st_swap / st_sample_w* in between.
 *
 * The contract of the two split operations, as the library enforces it (tests/protocol_model.py restates it and replays random
 * call sequences against it).  "open" = between st_factor_enqueue(s, .) and st_factor_finish; "pending" = between
 * st_sample_w_loglik_begin and _end; both may hold at once (the driver: _begin, _enqueue, statistics, setters, _finish, _end).
 * refused = ST_ERR_USAGE, a text in st_last_error() that names the call, the handle unchanged.
 *
 *   call                                         | while open (slot s)        | while pending
 *   ---------------------------------------------+----------------------------+---------------------------
 *   st_factor_finish                             | legal (closes it)          | legal
 *   st_sample_w_loglik_end                       | legal                      | legal (closes it)
 *   st_beta_stats, st_tausq_stats                | legal                      | legal (of the sweep's w)
 *   st_set_beta, st_set_tausq_inv                | legal                      | legal (the pending sweep does not see them)
 *   st_get_resid, st_get_xb, st_xtx              | legal                      | legal
 *   st_factor_ahead_enable                       | legal                      | legal
 *   st_get_block, st_get_comps (slot t)          | refused for t == s         | legal
 *   st_loglik_w (slot t)                         | refused for t == s         | refused
 *   st_set_w, st_get_w, st_yhat                  | legal (queued behind it)   | refused
 *   st_factor, st_factor_local, st_factor_enqueue| refused                    | legal
 *   st_factor_begin                              | refused                    | legal
 *   st_sample_w, st_sample_w_loglik, _begin      | refused                    | refused
 *   st_swap, st_predict                          | refused                    | refused
 *
 * A st_factor_enqueue that is itself refused or fails (a negative code) opens nothing; one that returns 0 is open even when the
 * factorisation fails: its code (1 / 2 / 3) comes from st_factor_finish.  A st_sample_w_loglik_begin with a negative code leaves
 * nothing pending.  The multi-GPU building blocks (st_*_local, st_mg_*) are the caller's protocol and are not checked. */
/* On slot 1 (one GPU, st_options.reserved bit 2 clear) the quad leaf levels compute V = Linv_pa K_pa,j and the log-density
 * only; their panel rows [-r_j T_j | r_j] are finished from the stored V by the first call that reads the slot's panels --
 * st_swap (before it swaps), st_get_block, st_loglik_w / st_loglik_local, st_sample_w_loglik(_begin) -- on the launch
 * stream, bit-identical to st_factor's.  Re-factorising the slot (st_factor*, st_factor_begin) drops the deferred half. */
int st_factor_enqueue(st_handle h, int slot, const double *theta, int ntheta);
int st_factor_is_async(st_handle h);   /* 1: _enqueue really starts the work (one GPU, no communicator) */
int st_factor_finish(st_handle h, double *loglik);
/* optional: start phase A of the latency-bound top levels ahead of time -- they depend on theta only (their blocks'
 * quadratic forms are redone with the current w afterwards) -- on a second stream, e.g. before the sweep; the next
 * st_factor / st_factor_local / st_factor_enqueue for the same slot and theta picks the result up.  Identical results; a no-op when the tree
 * does not qualify (column-group levels above a k_factor_quad level) or SPAMTREE_ASYNC_TOP=0.  (The proposal of spamtree_fit.cpp:211-229 does not depend on the sweep.) */
/* Contract: between st_factor_begin(slot, theta) and the st_factor / st_factor_local that picks its result up, st_swap is
 * refused (ST_ERR_USAGE: the arena being written would become the accepted slot); readers of the slot (st_get_block,
 * st_get_comps, st_loglik_w(1), st_mg_pack_comps) are ordered behind the launches in flight.
 * From st_factor_begin(slot, theta) on, the slot's caches are those of no theta (its top levels are theta's, the rest what was
 * there) until a factorisation of that slot succeeds.  The next factorisation of EITHER slot ends the ahead-of-time state: for
 * the same slot and a theta equal in every entry it continues from the result; for another theta or the other slot the result
 * is dropped and every level runs in full, as if st_factor_begin had not been called (the dropped launches are waited for, so
 * nothing overlaps them).  A st_factor_begin after another one replaces it. */
int st_factor_begin(st_handle h, int slot, const double *theta, int ntheta);
int st_factor_ahead_levels(st_handle h);   /* how many leading levels st_factor_begin runs ahead (0: none) */
/* measurement only: 0 switches the ahead-of-time path off (st_factor_begin becomes a no-op, every level runs inside
 * st_factor on the launch stream), 1 back on.  Results are identical either way. */
int st_factor_ahead_enable(st_handle h, int enable);

/* ---- accept_make_change (spamtree_model.cpp:1432-1435): swap the two cache slots */
int st_swap(st_handle h);

/* ---- phase B: gibbs_sample_w_std(true) on param_data (spamtree_model.cpp:1011-1226).
 * z = the reference's bigrnorm (n_all standard normals, model row order).  z == NULL: generate on device,
 * z_i = normal(Philox4x32-10; key=seed, counter=(row, row>>32, iter, 0)) -- identical for any GPU count. */
int st_sample_w(st_handle h, const double *z, uint64_t seed, uint32_t iter);

/* ---- phase C: get_loglik_w_std(data) (spamtree_model.cpp:781-826) */
int st_loglik_w(st_handle h, int slot, double *loglik);

/* st_sample_w followed by st_loglik_w(slot), same results and return codes (the sweep's 10 / 11 first), with a single
 * host synchronisation: what the MCMC driver calls once per iteration (spamtree_fit.cpp:182-185). */
int st_sample_w_loglik(st_handle h, const double *z, uint64_t seed, uint32_t iter, int slot, double *loglik);
/* The same pair without its host synchronisation (spamtree_fit.cpp:182-185 then :211-289: the sweep's log-density is not read
 * before the Metropolis step): _begin enqueues sweep + phase C and returns; any later synchronising call (st_factor) brings the
 * results along; _end returns what st_sample_w_loglik would have (0 and *loglik, or the sweep's failure code 10 / 11).  One
 * _end per _begin, before the next sweep.  Multi-GPU handles run the synchronous protocol inside _begin.
 * While a sweep is pending the handle's w is the sweep's (stream order) but no call that reads or replaces it on the host, runs
 * another sweep, predicts or swaps is accepted: the table next to st_factor_enqueue lists what is legal and what is refused. */
int st_sample_w_loglik_begin(st_handle h, const double *z, uint64_t seed, uint32_t iter, int slot);
int st_sample_w_loglik_end(st_handle h, double *loglik);

/* ---- phase P: predict_std(true, theta_changed) on param_data (spamtree_model.cpp:1234-1358); uses the last sweep's z */
int st_predict(st_handle h, int theta_changed);

/* ---- reductions for gibbs_sample_beta / gibbs_sample_tausq (spamtree_model.cpp:1374-1375, 1397-1400).
 * xty: p x q column-major, column j = X_avail_j' (y_avail_j - w[...]);  ssq: q, sum (y - XB - w)^2 over observed rows.
 * n_obs_by_q: q (may be NULL).  The draws themselves (R::rgamma, arma::randn) stay with the host driver.
 * One reduction serves both (and is kept until w or XB changes); its order of additions depends on n_all only, not on p or q,
 * so every statistic is reproducible bit for bit and identical on every rank of a sharded run. */
int st_beta_stats(st_handle h, double *xty);
int st_tausq_stats(st_handle h, double *ssq, int64_t *n_obs_by_q);
/* XtX(j) = X_avail_j' X_avail_j over the observed rows of outcome j (spamtree_model.cpp:151-155), p x p x q, formed once by
 * st_create: for p <= 8 by a serial host sum in row order, for p > 8 on the device by the statistics reduction with a column of X
 * as the row weight (fixed shape, deterministic, XtX(j) symmetric to the bit). */
int st_xtx(st_handle h, double *xtx);

/* ---- yhat = XB + w + tausq^{1/2} * normal (spamtree_fit.cpp:384); noise==NULL: device stream 5 */
int st_yhat(st_handle h, const double *noise, uint64_t seed, uint32_t iter, double *yhat);

/* ---- inspection (parity tests): per-block caches of a slot.
 * For block u (0-based id) with m rows and P ancestor rows the build keeps the inverse-Cholesky row panel
 * [ -Ri*H | Ri ] (tree_utils.cpp:204-206) instead of H, Kxx_inv, Kxx_invchol separately.
 * st_block_dims: *m, *P, *is_ref.  st_get_block: negRiH (m x P, column-major) and Ri (m x m column-major for a
 * reference block, m diagonal entries for a non-reference block). */
int st_block_dims(st_handle h, int64_t u, int64_t *m, int64_t *P, int32_t *is_ref, int32_t *n_obs);
int st_get_block(st_handle h, int slot, int64_t u, double *negRiH, double *Ri);
int st_get_comps(st_handle h, int slot, double *logdetCi_comps, double *loglik_w_comps); /* n_blocks each */

/* ---- measurement: algorithmic bytes of one iteration (SURVEY.md section 8d operand-streaming model)
 * out[0..4] = phase A, B, C, messages, S1+S2;  flops[0..2] = A, B, C (may be NULL). */
int st_algorithmic_bytes(st_handle h, double *out5, double *flops3);
/* box-measured peaks for the roofline report (csrc/probe.hip; no handle needed): out3[0] = stream-copy GB/s (read + written
 * bytes, `bytes` per buffer, best of `reps`), out3[1] = FP64 MFMA TFLOP/s (v_mfma_f64_16x16x4_f64), out3[2] = FP64 FMA TFLOP/s
 * (v_fma_f64).  About 0.15 s. */
int st_probe_peaks(int device, int64_t bytes, int reps, double *out3);
/* the covariance kernels' elementary functions (csrc/st_device.hpp), evaluated on the device through the same inlined helpers
 * (csrc/probe.hip; no handle needed): out[i] = f(x[i]), f = cov_sqrt (fn 0), cov_exp (1), cov_exp_tab (2). */
int st_probe_math(int32_t fn, const double *x, int64_t n, int32_t device, double *out);
/* the leaf factor kernel's sum over groups of ns (8 or 16) consecutive lanes of a wave (csrc/st_device.hpp: group_xor_sum, DPP
 * moves; dpp = 0: the __shfl_xor butterfly with the same partners and order), one value per lane: out[i] = the sum of x over
 * lane i's group.  n: a multiple of 64 (one wave per 64 values). */
int st_probe_group_sum(int32_t ns, int32_t dpp, const double *x, int64_t n, int32_t device, double *out);
/* per-kernel-family device time from HIP events recorded on the launch stream around every launch (enable=1), or around
 * the phase-A launches only (enable=2: the roofline measurement at a third of the event traffic; ~60 event records per
 * iteration cost 4-6 % of the iteration at n = 1e6).  Events are harvested lazily: no host synchronisation is added.
 * families: 0 factor(A) 1 sample(B) 2 loglik(C) 3 reduce 4 stats/xb 5 rng 6 predict 7 comm (the library's RCCL collectives
 * on the launch stream: device time between the events, i.e. including the wait for the slowest rank) */
#define ST_N_KERNEL_FAMILIES 8
int st_profile_enable(st_handle h, int enable);
int st_profile_get(st_handle h, double *ms_total, int64_t *launches); /* ST_N_KERNEL_FAMILIES each; resets */
/* phase-A launches by tree level since the last call: mean ms per launch, algorithmic bytes per launch; resets */
int st_profile_levels(st_handle h, int32_t *n_levels, double *ms_by_level, double *bytes_by_level, int32_t cap);
/* which phase-A kernel each observed level takes (same dispatch as st_factor: a function of the tree only) and the sizes
 * that decide it: per level g < *n_levels (at most cap entries written): kernel[g] = one of ST_KERNEL_*, max_m[g], max_P[g]
 * (largest block / ancestor-row count), n_blocks[g].  Any output pointer but n_levels may be NULL. */
#define ST_KERNEL_GENERIC_LDS 0
#define ST_KERNEL_GENERIC_SCRATCH 1
#define ST_KERNEL_MFMA 2
#define ST_KERNEL_QUAD 3
#define ST_KERNEL_BIGMFMA 4
#define ST_KERNEL_WIDE 5
#define ST_KERNEL_LCHAIN 6
#define ST_KERNEL_LCHAIN_REF 7   /* reference level: k_factor_lchain for the chain pass + k_factor_ref_finish per block */
int st_level_info(st_handle h, int32_t *n_levels, int32_t *kernel, int32_t *max_m, int32_t *max_P, int32_t *n_blocks, int32_t cap);
/* what the launch sites actually ran the last time each phase ran, as route codes written at the launch (not a recomputed
 * dispatch): per level g < *n_levels (at most cap levels written) phase_a[ST_ROUTE_A_SLOTS g + i] = phase A's kernels in
 * launch order (the limited tree's chain pre-pass is on level 0), phase_b[2 g] = the Gram kernel of the level's last sweep,
 * phase_b[2 g + 1] = its sweep kernel; *phase_p = the kernel of the last st_predict.  ST_ROUTE_NONE: nothing launched.
 * Any output pointer but n_levels may be NULL.  st_route_name spells a code as the template instantiation in the source
 * ("k_factor_quad<4, 44, 11, true, true>"); NULL for a code out of range.  Needs no device. */
#define ST_ROUTE_NONE 0
#define ST_ROUTE_A_SLOTS 3
int st_route_info(st_handle h, int32_t *n_levels, int32_t *phase_a, int32_t *phase_b, int32_t *phase_p, int32_t cap);
const char *st_route_name(int32_t code);
int st_synchronize(st_handle h);
void *st_stream(st_handle h);                              /* the hipStream_t every kernel is launched on */

/* ---- SURVEY.md section 8f "next" rows -------------------------------------------------------------------------------
 * CrossCovarianceAG10 (/root/reference/src/covariance_functions.cpp:301-355, exported to R, NAMESPACE:14): dense
 * n1 x n2 Apanasovich-Genton cross-covariance, column-major; coords n x 2 column-major, mv 1-based, Dmat q x q.
 * Needs no handle.  q < 2 is refused like the reference ("Invalid Dmat for multivariate data"). */
int st_cross_covariance_ag10(const double *coords1, const int64_t *mv1, int64_t n1, const double *coords2, const int64_t *mv2,
                             int64_t n2, const double *ai1, const double *ai2, const double *phi_i, const double *thetamv,
                             const double *Dmat, int32_t q, int32_t device, double *out);
/* Running posterior means of w and yhat on the device (what list_mean, /root/reference/src/list_mean.cpp:10-40, computes
 * after the fact from `keep` stored copies): accumulate on every saved iteration, read the means once. */
int st_summary_reset(st_handle h);
int st_summary_accumulate(st_handle h, uint64_t seed, uint32_t iter);
int st_summary_get(st_handle h, double *w_mean, double *yhat_mean, int64_t *n_accumulated);
/* Posterior quantiles on the device (list_qtile / prctile_stl, /root/reference/src/list_mean.cpp:62-137: per row, the order
 * statistics around q * keep of the `keep` saved draws, interpolated by the reference's rule).  st_summary_reserve(keep) keeps
 * the draws of the next `keep` st_summary_accumulate calls in HBM (2 x keep x n_all doubles: w and yhat; keep <= 16384;
 * keep = 0 frees them); st_summary_quantile sorts every row's draws in LDS.  Either output may be NULL. */
int st_summary_reserve(st_handle h, int64_t keep);
int st_summary_quantile(st_handle h, double q, double *w_q, double *yhat_q);

/* ---- convergence diagnostics of the stored draws, on the device: per series x_0 .. x_{K-1} of K >= ST_DIAG_MIN_DRAWS stored draws
 * (a row's w or yhat, a new point's w* or yhat*, a functional's F_w or F_y) the effective sample size, the Monte-Carlo standard
 * error of the posterior mean, the posterior sd of the draws and the split-R-hat of the one chain.  The definition (the kernel,
 * spamtree_amd.diagnostics.series_diagnostics and the tests' reference restate it):
 *   moments     m = (1/K) sum x_s;  d_s = x_s - m;  gamma_t = (1/K) sum_{s=0}^{K-1-t} d_s d_{s+t};
 *               sd = sqrt(K/(K-1) gamma_0);  rho_t = gamma_t / gamma_0
 *   lag cap     L = min(max_lag, K - 2), max_lag = 0 meaning ST_DIAG_DEFAULT_MAX_LAG (a design constant that bounds the worst-case
 *               cost per series, not a measurement);  k_max = (L - 1) / 2 (integer division)
 *   tau         Geyer's initial positive sequence, made monotone: for k = 0 .. k_max, Gamma_k = rho_2k + rho_2k+1; stop at the
 *               first k with !(Gamma_k > 0) (that Gamma_k is not added; a NaN stops too); otherwise Gamma_k <- min(Gamma_k,
 *               Gamma_k-1);  tau = -1 + 2 sum Gamma_k, floored at 1 / log10(K) (which caps ess at K log10 K)
 *   outputs     ess = K / tau;  mcse = sd / sqrt(ess);  lags = 2 x (number of pairs added).  A series is TRUNCATED when the loop
 *               ends at k_max without meeting a non-positive pair, lags == 2 (k_max + 1): its ess is then an overestimate.
 *               The monotone rule makes ess continuous in the data: a pair that changes sign in its last bit moves tau by no
 *               more than the pairs behind it can add, each of them at most that bit.
 *   split-R-hat h = K / 2 (integer division); halves x_0 .. x_{h-1} and x_{K-h} .. x_{K-1} (K odd: the middle draw is dropped);
 *               half means m_1, m_2; half sample variances s_1^2, s_2^2 with divisor h - 1;  W = (s_1^2 + s_2^2) / 2;
 *               B = h ((m_1 - mb)^2 + (m_2 - mb)^2), mb = (m_1 + m_2) / 2;  rhat = sqrt(((h-1)/h W + B/h) / W)
 *   degenerate  gamma_0 == 0: ess = NaN, mcse = 0, sd = 0, rhat = NaN, lags = 0.  W == 0 with gamma_0 > 0: rhat = NaN only.
 * One pass over a store gives all five outputs of its series; every sum is taken in an order that depends on K, max_lag and the
 * lane geometry only (spamtree_amd/csrc/diag_kernels.hpp), so the outputs of a series are bitwise a function of its K values and
 * max_lag, wherever it is stored.  Each call works on the draws stored so far, changes no state and consumes no Philox draw.
 * st_summary_diagnostics: the stores of st_summary_reserve; n_all values per array, model row order; limited_tree handles included.
 * st_points_summary_diagnostics: the point set's stores; n_new values, caller order; st_points_summary_quantile's refusals.
 * st_points_functionals_diagnostics: the functionals' stores; n_fun values; st_points_functionals_quantile's refusals.
 * Either struct, and any pointer in it, may be NULL.  ST_ERR_USAGE with a text: fewer than ST_DIAG_MIN_DRAWS stored draws (no
 * reservation included), max_lag < 0, a yhat request on a point set without X.  A point or functional set of size 0: ST_OK. */
#define ST_DIAG_MIN_DRAWS 4
#define ST_DIAG_DEFAULT_MAX_LAG 1024
typedef struct st_series_diag { double *ess, *mcse, *sd, *rhat; int32_t *lags; } st_series_diag;   /* any pointer may be NULL */
int st_summary_diagnostics(st_handle h, int32_t max_lag, const st_series_diag *w, const st_series_diag *yhat);
int st_points_summary_diagnostics(st_handle h, int32_t max_lag, const st_series_diag *w, const st_series_diag *yhat);
int st_points_functionals_diagnostics(st_handle h, int32_t max_lag, const st_series_diag *w, const st_series_diag *yhat);

/* ---- exceedance probabilities, excursion functions and simultaneous bands of the stored draws, on the device.  One store
 * X[d][i] has draws d < K (1 <= K <= 16384) and series i < n (a row's w or yhat, a new point's w* or yhat*, a functional's F_w or
 * F_y).  The definition (the kernel file, spamtree_amd.excursions and the tests' reference restate it):
 *   domain      every series has g(i) in {-1, 0 .. G-1}: rows and new points g(i) = outcome (mv - 1), G = q; functionals G = 1.
 *               mask (n bytes in the order of the outputs, 0 = out, NULL = all in) sets g(i) = -1: such a series still gets its
 *               marginal outputs (count, prob, mean, sd) and takes part in no joint one.
 *   thresholds  T = n_thr of them, 1 <= T <= ST_EXC_MAX_THRESHOLDS, each with a side s_t in {+1, -1} (side NULL: all +1) and the
 *               values c_t(i) = thr[t q + outcome(i)] for rows and points, thr[t n_fun + i] for functionals.
 *   event       E_t(d,i): X[d][i] > c_t(i) for side +1, X[d][i] < c_t(i) for side -1, both strict; a NaN draw makes it false.
 *   exceedance  count_t(i) = #{d : E_t(d,i)} (int32);  prob_t(i) = count_t(i) / K, one double division.
 *   excursion   the nested family is the level sets of the marginal count, D_{t,g}(c) = {i : g(i) = g, count_t(i) >= c}; whole
 *               tie classes enter together, no order among ties is invented.  Per draw
 *                 m_{t,g}(d) = max{count_t(i) : g(i) = g, not E_t(d,i)}, -1 if no series of the domain fails;
 *               draw d satisfies D(c) exactly when m(d) < c, so
 *                 excur_t(i) = #{d : m_{t,g(i)}(d) < count_t(i)} / K for g(i) >= 0, NaN for g(i) = -1;
 *                 joint_all[t][g] = #{d : m_{t,g}(d) < 0} / K, the share of draws with the event on the whole domain (an empty
 *               domain gives 1).  The level-alpha excursion set of a domain is {i : excur_t(i) >= 1 - alpha}.  excur <= prob, and
 *               excur does not decrease as count grows within a domain.  Integer comparisons, integer max and one division:
 *               bitwise defined, whatever the order of the reductions.
 *   band        (want_band, or any of mean / sd / maxdev / n_flat asked for; K >= 2)  per series Welford over ascending d in one
 *               chain: delta = x - m; m <- fma(delta, r_d, m) with r_d = 1 / (d + 1) rounded once; M2 <- fma(delta, x - m, M2);
 *               mean = m, sd = sqrt(M2 / (K - 1)).  Per draw and domain
 *                 maxdev[g][d] = max{|X[d][i] - mean_i| / sd_i : g(i) = g, sd_i > 0 and finite}, 0 if there is no such series;
 *               the series of a domain with sd_i = 0 or NaN are left out and counted in n_flat[g].  The band factor is not a
 *               device output: it is the ceil((1 - alpha) K)-th smallest maxdev[g][.] (an order statistic, not interpolated;
 *               spamtree_amd.excursions.band_factor), and the band is mean +- factor sd.
 * No reduction over series depends on the launch geometry in its value (integer max, max of non-negative doubles, integer sums);
 * the outputs of a store are a function of its contents, the thresholds and the mask only.
 * Any pointer of st_excursion_out may be NULL: only what is asked for is computed and copied.  count, prob, excur: n_thr x n,
 * threshold-major; joint_all: n_thr x G; mean, sd: n; maxdev: G x K; n_flat: G; n_draws: the K the call worked on.
 * st_summary_excursions: the stores of st_summary_reserve; n = n_all, model row order; limited_tree handles included.
 * st_points_summary_excursions: the point set's stores, caller order; st_points_summary_quantile's refusals.
 * st_points_functionals_excursions: the functionals' stores; st_points_functionals_quantile's refusals.
 * Each call works on the draws stored so far, changes no state and consumes no Philox draw; either out may be NULL.
 * ST_ERR_USAGE with a text: no stored draw; n_thr outside 1 .. 8 when thr is given; a NaN or infinite threshold; a side other
 * than +-1; a band request with K < 2; count / prob / excur / joint_all without thr; yhat on a point set without X; a spec with
 * neither thresholds nor band.  A point or functional set of size 0: ST_OK, nothing written.  A refusal leaves the handle usable. */
#define ST_EXC_MAX_THRESHOLDS 8
typedef struct st_excursion_spec { int32_t n_thr; const double *thr; const int32_t *side; const uint8_t *mask; int32_t want_band; } st_excursion_spec;
typedef struct st_excursion_out {      /* any pointer may be NULL; only what is asked for is computed and copied */
  int32_t *count; double *prob, *excur;        /* n_thr x n, threshold-major */
  double *joint_all;                           /* n_thr x G */
  double *mean, *sd;                           /* n */
  double *maxdev; int64_t *n_flat;             /* G x K; G */
  int64_t *n_draws;
} st_excursion_out;
int st_summary_excursions(st_handle h, const st_excursion_spec *spec, const st_excursion_out *w, const st_excursion_out *yhat);
int st_points_summary_excursions(st_handle h, const st_excursion_spec *spec, const st_excursion_out *w, const st_excursion_out *yhat);
int st_points_functionals_excursions(st_handle h, const st_excursion_spec *spec, const st_excursion_out *w, const st_excursion_out *yhat);

/* ---- rank-normalised R-hat, bulk, tail, quantile and exceedance ESS of the stored draws, on the device (Vehtari, Gelman, Simpson,
 * Carpenter, Buerkner 2021, for the one chain the stores hold).  st_*_diagnostics above gives the ESS of the MEAN and a plain
 * split-R-hat; these say how far a quantile, a tail or an exceedance probability of the same store can be trusted.  One series is
 * x_0 .. x_{K-1}, ST_DIAG_MIN_DRAWS <= K <= 16384; xs is its ascending sort.  "the diagnostics on a series" are ess, rhat, lags and
 * the truncated state of st_*_diagnostics, in that definition's order of operations and with its max_lag rule (one text:
 * spamtree_amd/csrc/diag_kernels.hpp).  The definition (spamtree_amd/csrc/rank_kernels.hpp, spamtree_amd.diagnostics.
 * rank_series_diagnostics and tests/rank_reference.py restate it):
 *   ranks       lo_s = #{u : x_u < x_s}, hi_s = #{u : x_u <= x_s};  r2_s = lo_s + hi_s + 1, twice the average 1-based rank, an
 *               integer; ties share it.
 *   scores      p_s = (4 r2_s - 3) / (8 K + 2), one double division of two exact integers (= (r - 3/8) / (K + 1/4));
 *               z_s = Phi^-1(p_s), Phi^-1 being st_norm_quantile_f of spamtree_amd/csrc/norm_quantile.hpp (Wichura's AS 241), the
 *               same text on the host (st_norm_quantile), on the device and in the CPU check.
 *   bulk        rhat_bulk = the diagnostics' rhat on z;  ess_bulk, lags_bulk = their ess and lags on z.  ess_bulk is NOT split
 *               into half chains (posterior::ess_bulk is): the split check is R-hat's job here.
 *   folded      med = xs[(K-1)/2] for odd K, 0.5 (xs[K/2-1] + xs[K/2]) for even K;  f_s = |x_s - med|;  zf = the scores of f;
 *               rhat_fold = the diagnostics' rhat on zf;  rhat_rank = fmax(rhat_bulk, rhat_fold) (NaN only if both are).
 *   indicator   for a 0/1 series I with c = sum I_s: c == 0 or c == K gives ess = NaN, lags = 0.  Otherwise, in 64-bit integers,
 *               n11_t = sum_{s<K-t} I_s I_{s+t}, head_t = sum_{s<K-t} I_s, tail_t = sum_{s>=t} I_s,
 *               A_t = K^2 n11_t - K c (head_t + tail_t) + (K - t) c^2  (= K^2 sum (I_s - c/K)(I_{s+t} - c/K); |A_t| <= 2^42;
 *               A_0 = K c (K - c));  rho_t = A_t / A_0.  From rho_t on, the pairs, the stop rule, the monotone rule, tau, its
 *               floor and ess = K / tau are the diagnostics', evaluated on the integer numerators: Gamma_k = N_k / A_0 with
 *               N_k = A_2k + A_2k+1; stop at the first !(N_k > 0); N_k <- min(N_k, N_k-1); (|N_k| <= 2^43, at most 2^13 pairs)
 *               tau = max((double)(2 sum N_k - A_0) / (double)A_0, 1 / log10 K): one quotient of integers (2 sum N_k - A_0 can
 *               reach 2^57, so each conversion rounds once, as does the quotient), the same on any machine and in any
 *               reduction order.  (With every rho_t rounded to double and the pairs summed in double, a
 *               slowly mixing indicator of 8192 draws came out 1.3e-14 from the exact rational: more than the 1e-14 its test allows.)
 *   quantile    n_prob <= ST_RANK_MAX_PROBS probabilities strictly inside (0, 1):  j = min(max(ceil(prob K), 1), K - 1) - 1
 *               (one multiplication, then ceil);  I_s = [x_s <= xs[j]];  ess_q[k][i] = the indicator ESS.
 *               ess_tail = fmin(indicator ESS at 0.05, at 0.95), whatever prob holds.
 *   exceedance  thresholds and sides as in st_excursion_spec: thr[t q + outcome] for rows and points, thr[t n_fun + i] for
 *               functionals, side +-1 (NULL: all +1), strict inequalities, at most ST_EXC_MAX_THRESHOLDS.  I_s = E_t(s, i);
 *               ess_exc[t][i] = its indicator ESS;  prob = c / K (bit for bit the prob of st_*_excursions on the same store);
 *               mcse_prob = sqrt(prob (1 - prob) / ess_exc), 0 where c is 0 or K.
 *   degenerate  a series with a NaN draw: NaN in every double output, 0 in lags_bulk.  A constant series: all ranks tied, z = 0,
 *               gamma_0 == 0 on z and the diagnostics' degenerate outputs follow (rhat NaN, ess NaN, lags 0).
 * The outputs of a series are bitwise a function of its K values and the spec, wherever it is stored.  Any pointer of
 * st_rank_out may be NULL: only what is asked for is computed and copied.  ess_q: n_prob x n; ess_exc, mcse_prob, prob: n_thr x n;
 * the others n.  Each call accepts exactly the handles its *_diagnostics sibling accepts, works on the draws stored so far, changes
 * no state and consumes no Philox draw.  ST_ERR_USAGE with a text: fewer than ST_DIAG_MIN_DRAWS stored draws; max_lag < 0; n_prob
 * or n_thr outside 0 .. 8; a prob not strictly inside (0, 1); a NaN or infinite threshold; a side other than +-1; ess_q without
 * prob; ess_exc, mcse_prob or prob without thr; yhat on a point set without X.  A set of size 0: ST_OK, nothing written.  A
 * refusal leaves the handle usable. */
#define ST_RANK_MAX_PROBS 8
typedef struct st_rank_spec {
  int32_t max_lag;                                       /* 0: ST_DIAG_DEFAULT_MAX_LAG */
  int32_t n_prob; const double *prob;
  int32_t n_thr; const double *thr; const int32_t *side;
} st_rank_spec;
typedef struct st_rank_out {          /* any pointer may be NULL; only what is asked for is computed and copied */
  double *rhat_rank, *rhat_bulk, *rhat_fold, *ess_bulk, *ess_tail;   /* n */
  int32_t *lags_bulk;                                                /* n */
  double *ess_q;                                                     /* n_prob x n */
  double *ess_exc, *mcse_prob, *prob;                                /* n_thr x n */
} st_rank_out;
int st_summary_rank_diagnostics(st_handle h, const st_rank_spec *spec, const st_rank_out *w, const st_rank_out *yhat);
int st_points_summary_rank_diagnostics(st_handle h, const st_rank_spec *spec, const st_rank_out *w, const st_rank_out *yhat);
int st_points_functionals_rank_diagnostics(st_handle h, const st_rank_spec *spec, const st_rank_out *w, const st_rank_out *yhat);
/* z[i] = Phi^-1(p[i]) by the text the device runs (norm_quantile.hpp); needs no device.  Returns ST_OK. */
int st_norm_quantile(const double *p, double *z, int64_t n);

/* ---- the same diagnostics of several chains in one store: between-chain R-hat and the ESS of the combined chains, on the device.
 * A store of K = M N draws, M = n_chains, is read as M chains of N draws laid end to end: x_{c,s} = x_{cN+s}, c < M, s < N (what a
 * driver leaves that runs M chains one after another into one set of stores).  The definition (spamtree_amd/csrc/diag_kernels.hpp,
 * rank_kernels.hpp, spamtree_amd.diagnostics.multichain_* and tests/multichain_reference.py restate it):
 *   limits      1 <= M <= ST_DIAG_MAX_CHAINS = 16 (a design constant: a wave keeps one value per half chain in a lane of its own; not
 *               a measurement);  N >= ST_DIAG_MIN_DRAWS;  K <= 16384.
 *   M = 1       the single-chain definitions above and their results, bit for bit.
 *   lag cap     L = min(max_lag, N - 2), max_lag = 0 meaning ST_DIAG_DEFAULT_MAX_LAG;  k_max = (L - 1) / 2.
 *   within and  mu_c = the mean of chain c;  d_{c,s} = x_{c,s} - mu_c;  gamma_{c,t} = (1/N) sum_{s<N-t} d_{c,s} d_{c,s+t} (no product
 *   between     crosses a chain boundary);  gbar_t = (1/M) sum_c gamma_{c,t};  mubar = (1/M) sum_c mu_c;
 *               B' = sum_c (mu_c - mubar)^2 / (M - 1).
 *   rho, ess    rho_t = (B' + gbar_t) / (B' + gbar_0): Stan's combined estimator with the divisor-N variance throughout, so that it
 *               is gamma_t / gamma_0 at M = 1; it differs from the `posterior` package's, which takes the divisor N - 1 in the
 *               within-chain variance, by O(1/N).  From rho_t on the text above holds: Geyer's pairs, the stop rule, the monotone
 *               rule, tau = -1 + 2 sum Gamma_k floored at 1 / log10 K, ess = K / tau, lags and the truncated state.
 *   sd, mcse    sd = the pooled sd of all K draws about the pooled mean, divisor K - 1: the sd of st_*_diagnostics on the same
 *               store;  mcse = sd / sqrt(ess).
 *   rhat        every chain is split: h = N / 2, halves x_{c,0..h-1} and x_{c,N-h..N-1} (N odd: the middle draw is dropped),
 *               S = 2M segments with means m_j and sample variances s_j^2 (divisor h - 1);  W = (1/S) sum s_j^2;
 *               B = h / (S - 1) sum (m_j - mbar)^2, mbar = (1/S) sum m_j;  rhat = sqrt(((h-1)/h W + B/h) / W).
 *   degenerate  B' + gbar_0 == 0: ess = NaN, mcse = 0, sd = 0, rhat = NaN, lags = 0.  W == 0 otherwise: rhat = NaN only.
 *   rank family ranks, scores z, the median, the folded series and the order statistics xs[j] are those of the pooled K draws,
 *               exactly as above.  rhat_bulk, ess_bulk, lags_bulk = the multi-chain diagnostics on z;  rhat_fold = the multi-chain
 *               rhat on zf;  rhat_rank = fmax of the two.  The quantile, tail and exceedance indicators are built as above; their
 *               ESS is the multi-chain indicator ESS;  prob = C / K and mcse_prob as above.
 *   indicator   in 64-bit integers, M >= 2: per chain c_c = sum_s I_{c,s} and A_{c,t} = the A_t above with K -> N on that chain's
 *               draws alone;  C = sum c_c;  D = sum_c (M c_c - C)^2;  S_t = sum_c A_{c,t};
 *               Num_t = N D + M (M - 1) S_t  (= (M - 1) M^2 N^3 (B' + gbar_t));  rho_t = Num_t / Num_0;  the pairs, the stop and
 *               the monotone rule on the integers N_k = Num_2k + Num_2k+1;
 *               tau = max((double)(2 sum N_k - Num_0) / (double)Num_0, 1 / log10 K);  ess = K / tau.  C == 0 or C == K: ess = NaN,
 *               lags = 0.  Bound: sum_c (c_c - C/M)^2 <= M N^2 / 4 gives N D <= M^3 N^3 / 4 = K^3 / 4;  |A_{c,t}| = N^2 |sum_{s<N-t}
 *               (I_s - p)(I_{s+t} - p)| <= N^2 N p (1 - p) <= N^3 / 4 (Cauchy-Schwarz) gives |M (M - 1) S_t| < M^3 N^3 / 4 = K^3 / 4;
 *               so |Num_t| < K^3 / 2 <= 2^41, |N_k| < 2^42, and with at most 2^13 pairs |2 sum N_k - Num_0| < 2^57.
 * Every sum is taken in an order that depends on K, M, max_lag and the lane geometry only: the outputs of a series are bitwise a
 * function of its K values, n_chains and the spec, wherever it is stored.  Each call accepts exactly the handles, structs and specs
 * of its single-chain sibling, works on the draws stored so far, changes no state and consumes no Philox draw.  ST_ERR_USAGE with a
 * text and the numbers, beside the count of stored draws in the sibling's order of refusals: n_chains outside 1 .. 16; K not a
 * multiple of n_chains; K / n_chains < ST_DIAG_MIN_DRAWS.  A refusal leaves the handle usable. */
#define ST_DIAG_MAX_CHAINS 16
int st_summary_chain_diagnostics(st_handle h, int32_t n_chains, int32_t max_lag, const st_series_diag *w, const st_series_diag *yhat);
int st_points_summary_chain_diagnostics(st_handle h, int32_t n_chains, int32_t max_lag, const st_series_diag *w, const st_series_diag *yhat);
int st_points_functionals_chain_diagnostics(st_handle h, int32_t n_chains, int32_t max_lag, const st_series_diag *w, const st_series_diag *yhat);
int st_summary_chain_rank_diagnostics(st_handle h, int32_t n_chains, const st_rank_spec *spec, const st_rank_out *w, const st_rank_out *yhat);
int st_points_summary_chain_rank_diagnostics(st_handle h, int32_t n_chains, const st_rank_spec *spec, const st_rank_out *w,
                                             const st_rank_out *yhat);
int st_points_functionals_chain_rank_diagnostics(st_handle h, int32_t n_chains, const st_rank_spec *spec, const st_rank_out *w,
                                                 const st_rank_out *yhat);

/* ---- new-point prediction from a fitted state: the predictive at locations that are not rows of the problem, the way the model
 * treats an NA row (make_tree's missing level, predict_std spamtree_model.cpp:1234-1358) without rebuilding the tree.
 * A point of margin j anchored at block b (the block of its nearest deepest-knot-level row, same margin if cherrypick_same_margin,
 * ties to the lowest row: spamtree_amd.predict.locate) conditions on S = parents(b), plus b itself when b is a reference block:
 * with k = K(S, x*), v = Linv_S k, mean = v' Linv_S w_S, var = max(K(x*, x*) - v'v, 0), draw = mean + sqrt(var) z,
 * yhat = x' beta_j + draw + sqrt(tausq_j) e.  Not for limited_tree or world > 1 handles (ST_ERR_UNSUPPORTED).
 * st_points_set: coords n_new x 2 column-major, mv 1-based, anchor 0-based block ids with observed rows, X n_new x p column-major
 *   or NULL (then no yhat).  Replaces the previous point set.  A point set of size 0 has no X, whatever is passed.
 * st_points_predict: on slot 0 (refused before st_factor(0, ...)) and the current w / beta / tausq_inv.  mode 0 = draw, 1 =
 *   conditional mean only (w_new = cond_mean, no noise in yhat).  z: n_new normals in the caller's order, or NULL = Philox stream 6,
 *   counter (i, i >> 32, iter, 6), i = index in the caller's order; yhat noise: stream 7, same counter.  Any output may be NULL.
 *   Outputs are in the caller's order; mean, var and draws from a given z do not depend on the order or grouping of the points.
 * st_points_info: of the last st_points_predict -- route = bit set, bit (code - 1) set when the kernel of that code ran
 *   (st_points_route_name spells it; NULL out of range); n_groups = conditioning chains of the point set; the algorithmic bytes and
 *   flops of the call (from shapes).  Any output may be NULL.  Needs no device. */
int st_points_set(st_handle h, int64_t n_new, const double *coords, const int64_t *mv, const int64_t *anchor, const double *X);
int st_points_predict(st_handle h, int mode, const double *z, uint64_t seed, uint32_t iter, double *w_new, double *cond_mean,
                      double *cond_var, double *yhat_new);
int st_points_info(st_handle h, int32_t *route, int64_t *n_groups, double *alg_bytes, double *flops);
const char *st_points_route_name(int32_t code);

/* ---- predictive summaries of the point set over saved iterations, kept on the device (the st_summary_* of the new points).
 * st_points_accumulate: st_points_predict's draw (mode 0, Philox streams 6 / 7 with counter `iter`) into device buffers, then one
 *   element-wise update per point, in call order: Welford mean and M2 of the conditional mean, running sums of the conditional
 *   variance, of w* and of yhat* (with X).  With a reservation it also stores w* and yhat* as the next row of [keep][n_new] while
 *   fewer than `keep` are stored: the store holds the first `keep` draws since the latest of st_points_set, st_points_summary_reset
 *   and st_points_summary_reserve (its row count starts again there; n_accumulated runs on over a reservation).
 *   Outputs (caller order, n_new each) may be NULL: then nothing is copied to the host and nothing is synchronised.  Changes no
 *   state of the handle but the point set's.
 * st_points_summary_reset: zero the summaries and the stored draws (st_points_set starts a new set with none of either).
 * st_points_summary_reserve: room for the first `keep` draws (at most 16384, else ST_ERR_UNSUPPORTED); 0 releases it.  Resets
 *   the stored draws.
 * st_points_summary_get: mean = mean of the conditional means; var = mean of the conditional variances + population variance of the
 *   conditional means (st_points_predict's Rao-Blackwellised moments); w_mean, yhat_mean = means of the draws.  Any may be NULL.
 *   ST_ERR_USAGE before the first accumulated iteration (n_accumulated is still written), as st_points_summary_get_cov.
 * st_points_summary_quantile: k_qtile over the stored draws (the rule and limit of st_summary_quantile); ST_ERR_USAGE without a
 *   stored draw or q outside [0, 1].
 * All refuse limited_tree and world > 1 handles (ST_ERR_UNSUPPORTED) and need st_points_set (ST_ERR_USAGE). */
int st_points_accumulate(st_handle h, uint64_t seed, uint32_t iter, double *w_new, double *cond_mean, double *cond_var, double *yhat_new);
int st_points_summary_reset(st_handle h);
int st_points_summary_reserve(st_handle h, int64_t keep);
int st_points_summary_get(st_handle h, double *mean, double *var, double *w_mean, double *yhat_mean, int64_t *n_accumulated);
int st_points_summary_quantile(st_handle h, double q, double *w_q, double *yhat_q);

/* ---- joint prediction of groups of new points.  A joint group is 1..ST_POINTS_MAX_JOINT points of the set that share one
 * conditioning chain S (the "groups" of st_points_info are those chains) and are predicted together, e.g. the q outcomes at a site
 * or a few neighbouring cells.  For a group G with members in the caller's order, V = Linv_S K(S, G) and u = Linv_S w_S:
 *   cond_mean = V'u (per point, as st_points_predict),  cond_cov Sigma = K(G, G) - V'V,  cond_chol L = lower Cholesky factor of Sigma,
 *   w_G = cond_mean + L z_G,  yhat as st_points_predict;  z and the yhat noise: the same streams 6 / 7 and per-point counters.
 * A pivot d_j of the factorisation that is not above (P + g) 2^-52 K(x_j, x_j) (P rows of S, g members) counts as zero: L_jj and the
 * column below it are zero, z_j is not used, and row j keeps what the earlier members explain -- a duplicate of an earlier member
 * repeats its draw, a point on a conditioning row gets its w to rounding.  Sigma is not clamped; nothing is NaN.
 * st_points_set_joint: st_points_set plus one label per point (any int64, members need not be adjacent); joint_id NULL is exactly
 *   st_points_set.  ST_ERR_USAGE (naming the group) when a group's members do not end in the same chain -- give them one anchor --
 *   and ST_ERR_UNSUPPORTED beyond ST_POINTS_MAX_JOINT members; both leave the previous point set in place.
 * st_points_joint_layout: n_joint groups ordered by first appearance in the caller's order; group k's g_k x g_k column-major block of
 *   cond_cov / cond_chol / st_points_summary_get_cov starts at offsets[k] (offsets: n_joint + 1, the last = the packed length); its
 *   members, in the caller's order, are members[member_ptr[k] .. member_ptr[k + 1]) (member_ptr: n_joint + 1, members: n_new point
 *   indices).  Any output may be NULL; call once for n_joint, then with buffers.
 * st_points_predict_joint: st_points_predict on a joint set; cond_cov and cond_chol packed as above.  Any output may be NULL.  A
 *   group's cond_mean, cond_cov, cond_chol and draws from a given z depend on its chain and its own members only, not on the other
 *   groups, their order or the labels.  st_points_predict on a joint set still gives the per-point predictive.
 * st_points_accumulate on a joint set draws jointly and also updates, per group and pair a >= b in call order, the running sum of
 *   Sigma_ab and the Welford co-moment of the conditional means; st_points_accumulate_joint is the same call returning cond_cov /
 *   cond_chol in place of cond_var (= max(Sigma_aa, 0) in the per-point summaries).  st_points_summary_get_cov: the packed
 *   mean_s(Sigma_s) + cov_s(cond_mean_s), the joint form of st_points_summary_get's var; st_points_summary_reset clears it too.
 * st_points_info reports the joint kernels under route codes of their own.  Refusals as st_points_predict. */
#define ST_POINTS_MAX_JOINT 16
int st_points_set_joint(st_handle h, int64_t n_new, const double *coords, const int64_t *mv, const int64_t *anchor, const double *X,
                        const int64_t *joint_id);
int st_points_joint_layout(st_handle h, int64_t *n_joint, int64_t *offsets, int64_t *member_ptr, int64_t *members);
int st_points_predict_joint(st_handle h, int mode, const double *z, uint64_t seed, uint32_t iter, double *w_new, double *cond_mean,
                            double *cond_cov, double *cond_chol, double *yhat_new);
int st_points_accumulate_joint(st_handle h, uint64_t seed, uint32_t iter, double *w_new, double *cond_mean, double *cond_cov,
                               double *cond_chol, double *yhat_new);
int st_points_summary_get_cov(st_handle h, double *cov);

/* ---- linear functionals of the new-point predictions: F_f = sum_{k in [ptr[f], ptr[f+1])} wt[k] value[idx[k]], e.g. the mean of
 * the field over a region, a total, a contrast of two outcomes at a site.  Every new point (joint group) is a leaf block of its
 * own, so given w_S and theta distinct points (groups) are independent and for one saved draw
 *   Var(a'w* | w, theta) = sum_groups a_g' Sigma_g a_g   (= sum_i a_i^2 cond_var_i on a plain set),
 * which gives F the Rao-Blackwellised moments st_points_summary_get / _get_cov give points and groups.
 * st_points_functionals_set: n_fun functionals in CSR form on the current point set (needs one, ST_ERR_USAGE); idx 0-based in the
 *   caller's order of the points; an empty row is the functional 0; n_fun = 0 removes them.  Replaces the previous functionals and
 *   zeroes their accumulators and stored draws; the per-point and pair summaries are left alone.  ST_ERR_USAGE, naming the
 *   functional and entry, when ptr[0] != 0, ptr decreases, an index is outside 0..n_new-1, a weight is not finite or a point
 *   occurs twice in one functional; the previous functionals then stay.  st_points_set / st_points_set_joint drop them.
 * With functionals set, st_points_accumulate(_joint) also forms per functional F_w = a'w*, F_m = a'cond_mean, F_y = a'yhat (with X)
 *   and F_v = Var(a'w* | w, theta) (a plain set: from the clamped cond_var; a joint set: from the packed Sigma, the sum clamped at
 *   0) and updates the Welford mean and M2 of F_m, the running sums of F_v, F_w, F_y and, within st_points_summary_reserve's room,
 *   the stored draws F_w, F_y, with a row count of their own: the first `keep` draws since the latest of st_points_functionals_set,
 *   st_points_summary_reserve and _reset.  st_points_summary_reserve / _reset size and clear these along with their own.  (A point set of
 *   size 0 reserves nothing, as for its points: its functionals, all 0, store no draw and have no quantile.)  The summation order
 *   is fixed (spamtree_amd/csrc/points_fun.hpp): a functional's values depend on its own terms only, bit for bit.
 * st_points_functionals_last: the four values of the last accumulated iteration.
 * st_points_functionals_get: mean = mean of F_m; var = mean of F_v + population variance of F_m; w_mean, yhat_mean = means of
 *   the draws; refusals as st_points_summary_get.  st_points_functionals_quantile: k_qtile over the stored F_w / F_y, rules as
 *   st_points_summary_quantile.  Outputs hold n_fun doubles; any may be NULL.
 * st_points_functionals_info: the counts of the term lists (nnz linear terms, n_var_terms variance terms, n_chunks chunks of both
 *   lists) and the algorithmic bytes of the functional step of one saved iteration; zeros without functionals.
 * All but _info refuse limited_tree and world > 1 handles (ST_ERR_UNSUPPORTED). */
int st_points_functionals_set(st_handle h, int64_t n_fun, const int64_t *ptr, const int64_t *idx, const double *wt);
int st_points_functionals_last(st_handle h, double *f_w, double *f_cond_mean, double *f_cond_var, double *f_yhat);
int st_points_functionals_get(st_handle h, double *mean, double *var, double *w_mean, double *yhat_mean, int64_t *n_accumulated);
int st_points_functionals_quantile(st_handle h, double q, double *w_q, double *yhat_q);
int st_points_functionals_info(st_handle h, int64_t *n_fun, int64_t *nnz, int64_t *n_chunks, int64_t *n_var_terms, double *alg_bytes);

/* ---- scores of held-out observations at the new points.  A scored point i of margin j has an observed y_i; saved draw s gives it
 * the Gaussian predictive mu_s = x_i'beta_j + cond_mean_s(i), sigma2_s = cond_var_s(i) + tau2_j (cond_var as st_points_accumulate
 * forms it, clamped at 0; tau2_j = 1 / tausq_inv_j).  With r_s = (y_i - mu_s) / sigma_s, l_s = -r_s^2 / 2 - log sigma_s - log(2 pi) / 2
 * and the S draws accumulated since the scores were set:
 *   lpd_i  = log((1 / S) sum_s exp l_s), a streaming log-sum-exp (two doubles of state per point; finite when every exp l_s underflows)
 *   pit_i  = (1 / S) sum_s Phi(r_s)
 *   crps_i = (1 / K) sum_k |d_(k)| - (1 / K^2) sum_k (2 k - K - 1) d_(k), d_k = yhat*_k - y_i sorted ascending: the CRPS of the
 *            empirical distribution of the K stored yhat* draws of the point (st_points_summary_reserve)
 * and, on a joint set, per group G with observed members o (in member order, g_o >= 1)
 *   lpd_joint_G = log((1 / S) sum_s N_{g_o}(y_o; mu_o, Sigma_oo + diag tau2)), Sigma the draw's cond_cov (lower triangle, not clamped),
 *            factorised by an unpivoted Cholesky.  A pivot that is not > 0 gives that draw density 0 for that group and adds one
 *            to n_degenerate.
 * st_points_score_set: y_new holds n_new values in the caller's order; NaN: the point is predicted as before and not scored.  NULL
 *   removes the scores.  Needs a point set with X (ST_ERR_USAGE); an infinite value is ST_ERR_USAGE naming the index, and the
 *   previous scores then stay.  Replaces the previous scores and zeroes their state; the point, pair and functional summaries are
 *   left alone.  st_points_set / st_points_set_joint drop the scores, st_points_summary_reset clears their state.
 * With scores set, st_points_accumulate(_joint) also runs the score step after its summaries, on the same stream: it reads this
 *   iteration's outputs, X, beta and tausq_inv, consumes no draw of any stream and writes nothing another step reads, so every
 *   other output is the same bit for bit; with NULL outputs it still copies nothing and synchronises nothing.  The order of every
 *   operation is fixed (spamtree_amd/csrc/points_score.hpp): a point's or group's scores depend on its own inputs only, bit for bit.
 * st_points_score_get: lpd, pit, crps (n_new each; NaN where y_new is), lpd_joint (one per joint group in st_points_joint_layout's
 *   order; NaN for a group without an observed member; -inf when no draw had a positive density), n_scored, n_degenerate.  Any may
 *   be NULL.  ST_ERR_USAGE: before st_points_score_set, no scored point (n_scored is still written), no iteration accumulated,
 *   crps without a stored draw, lpd_joint on a plain set.
 * Both refuse limited_tree and world > 1 handles (ST_ERR_UNSUPPORTED). */
int st_points_score_set(st_handle h, const double *y_new);
int st_points_score_get(st_handle h, double *lpd, double *pit, double *crps, double *lpd_joint, int64_t *n_scored, int64_t *n_degenerate);

/* ---- Rao-Blackwellised exceedance probabilities at the new points: the mean over the saved draws of the exact conditional
 * probability, not a count over stored draws -- no reservation, no steps of 1 / K, no Monte-Carlo noise of the indicator.
 * n_thr <= ST_EXC_MAX_THRESHOLDS thresholds, each with a side s_t in {+1, -1}; the value is per outcome, c = thr[t q + j] for a point
 * of margin j, and thr_fun[t n_fun + f] for functional f.  Saved draw s gives (spamtree_amd/csrc/points_exceed.hpp has every
 * operation's order):
 *   point, target w:    m = cond_mean_s(i), v = cond_var_s(i) (clamped at 0; on a joint set max(Sigma_aa, 0)).  v > 0:
 *                       p_s = Phi(s_t (m - c) / sqrt(v)), Phi(z) = erfc(-z / sqrt 2) / 2.  v == 0: p_s = 1 if s_t (m - c) > 0, else 0
 *                       (strict, as the event of st_*_excursions).
 *   point, target yhat: (needs X) mu = x_i'beta_j + m, sigma2 = v + 1 / tausq_inv_j, p_s = Phi(s_t (mu - c) / sigma).
 *   functional, target w only: m = F_m, v = F_v of st_points_functionals_last, the same two rules.
 * Over the S draws accumulated since the thresholds were set: prob = mean_s p_s (Welford, in call order) and prob_var = the
 * population variance of p_s over the draws (the caller's MCSE is sqrt(prob_var / ESS)).  Nothing is NaN for a finite threshold.
 * st_points_exceed_set: side NULL: all +1.  thr_fun NULL: no functional part; thr_fun needs functionals set.  n_thr = 0 or thr NULL
 *   removes the thresholds.  ST_ERR_USAGE naming the index: n_thr outside 1 .. ST_EXC_MAX_THRESHOLDS, a threshold that is not
 *   finite, a side other than +-1; the previous thresholds then stay.  Replaces the previous thresholds and zeroes their state
 *   (16 n_thr B per point and target, nothing per draw); every other summary is left alone.  st_points_set / st_points_set_joint
 *   drop the thresholds, st_points_summary_reset clears their state, st_points_functionals_set drops the functional part only.
 * With thresholds set, st_points_accumulate(_joint) also runs the exceedance step after its functionals, on the same stream: it
 *   consumes no draw of any stream and writes nothing another step reads, so every other output is the same bit for bit; with
 *   NULL outputs it still copies nothing and synchronises nothing.  Without thresholds nothing is launched or allocated.
 * st_points_exceed_get: w, yhat (n_thr x n_new, threshold-major, caller order), fun_w (n_thr x n_fun); any struct and either member
 *   may be NULL.  ST_ERR_USAGE: before st_points_exceed_set, no iteration accumulated (n_accumulated is still written), yhat on
 *   a set without X, fun_w without functional thresholds.  An empty point set returns ST_OK with nothing written.
 * Both refuse limited_tree and world > 1 handles (ST_ERR_UNSUPPORTED). */
typedef struct st_rb_out { double *prob, *prob_var; } st_rb_out;   /* n_thr x n, threshold-major; either may be NULL */
int st_points_exceed_set(st_handle h, int32_t n_thr, const double *thr, const int32_t *side, const double *thr_fun);
int st_points_exceed_get(st_handle h, const st_rb_out *w, const st_rb_out *yhat, const st_rb_out *fun_w, int64_t *n_accumulated);

/* ---- quantiles and the exact CRPS of the mixture predictive at the new points.  Every saved draw s gives a point the exact
 * conditional law of the targets above: w* ~ N(m_s, v_s) and, with X, yhat* ~ N(mu_s, sigma2_s), sigma2_s = v_s + 1 / tausq_inv_j; a
 * functional's w ~ N(F_m, F_v).  The predictive is the equal-weight mixture of the K stored components (spamtree_amd/csrc/
 * points_mixture.hpp has every operation's order and the rounding bounds, spamtree_amd.mixture the definition in float64):
 *   CDF       F(x) = (1 / K) sum_s Phi((x - m_s) / sd_s); a component with v_s == 0 is the right-continuous step 1(x >= m_s).
 *   quantile  inf{x : F(x) >= p}, p strictly inside (0, 1): a safeguarded Newton iteration inside the bracket
 *             [min_s, max_s] of m_s + z_p sd_s, stopped at the width 2^-50 max(|bracket ends|).
 *   CRPS at y A(d, s2) = d erf(d / (s sqrt 2)) + s sqrt(2 / pi) exp(-d^2 / (2 s2)), A(d, 0) = |d|;
 *             crps = (1 / K) sum_s A(y - mu_s, sigma2_s) - spread,  spread = (1 / (2 K^2)) sum_s sum_t A(mu_s - mu_t, sigma2_s + sigma2_t)
 *             (Grimit et al. 2006): O(K^2) per scored point.  spread does not depend on y.
 * st_points_mixture_reserve: room for the first `keep` saved draws' moments: m, v and with X mu per point (24 B per point and draw,
 *   16 B without X), tau2 per outcome, F_m and F_v per functional.  keep > ST_MIX_MAX_DRAWS: ST_ERR_UNSUPPORTED (one series' pairs of
 *   doubles must fit one workgroup's LDS).  keep = 0 releases the store.  Replaces a previous store.  st_points_set(_joint) drops
 *   the store, st_points_summary_reset clears its count, st_points_functionals_set drops (and, when functionals are given,
 *   re-reserves empty) the functional part only.  A functional column is written only on an iteration that writes a point column:
 *   functionals set when the point columns are full get none, and st_points_mixture_quantiles' fun_w then has no stored draw.
 * With a store, st_points_accumulate(_joint) also writes one column after its exceedance step, on the same stream, while fewer
 *   than `keep` are stored: it consumes no draw of any stream and writes nothing another step reads, so every other output is the
 *   same bit for bit; with NULL outputs it still copies nothing and synchronises nothing.  Without a store nothing is launched
 *   or allocated.
 * st_points_mixture_draws: the stored columns in caller order, n_stored x n_new each (m, v, mu) and n_stored x q (tau2); any may be
 *   NULL; n_stored is written first.  ST_ERR_USAGE: no store reserved, mu on a set without X.
 * st_points_mixture_quantiles: 1 <= n_probs <= ST_MIX_MAX_PROBS probabilities strictly inside (0, 1) in any order, otherwise
 *   ST_ERR_USAGE naming the index.  q is n_probs x n (n_new, or n_fun for fun_w), probability-major, caller order; n_unconverged
 *   counts the series that hit the cap on passes (0 in every case known).  Any struct and either member may be NULL.  The
 *   quantiles of a series never decrease in p.  ST_ERR_USAGE: no stored draw, yhat on a set without X, fun_w without functionals.
 * st_points_mixture_crps: crps and spread at every scored point (n_new each, NaN where y_new of st_points_score_set is; either may
 *   be NULL), from the stored mu, v and tau2; needs nothing of st_points_summary_reserve.  Unscored points cost nothing.
 *   ST_ERR_USAGE: before st_points_score_set, no scored point, no stored draw.
 * An empty point set returns ST_OK with nothing written.  All four refuse limited_tree and world > 1 handles (ST_ERR_UNSUPPORTED). */
#define ST_MIX_MAX_DRAWS 8192
#define ST_MIX_MAX_PROBS 8
typedef struct st_mix_out { double *q; int64_t *n_unconverged; } st_mix_out;       /* q: n_probs x n, probability-major */
int st_points_mixture_reserve(st_handle h, int64_t keep);
int st_points_mixture_draws(st_handle h, double *m, double *v, double *mu, double *tau2, int64_t *n_stored);
int st_points_mixture_quantiles(st_handle h, int32_t n_probs, const double *probs,
                                const st_mix_out *w, const st_mix_out *yhat, const st_mix_out *fun_w);
int st_points_mixture_crps(st_handle h, double *crps, double *spread, int64_t *n_scored);   /* n_new each; NaN where y_new is */
/* The store's room (keep), the components it holds, its bytes on the device, and of the last st_points_mixture_quantiles the
 * quantiles solved (series x probabilities over the targets asked for) and the evaluations of F they took together: the passes per
 * quantile are n_passes / n_solved.  Zeros without a store; any pointer may be NULL. */
int st_points_mixture_info(st_handle h, int64_t *keep, int64_t *n_stored, double *store_bytes, int64_t *n_solved, int64_t *n_passes);

/* ---- criteria over the fit's own rows, on the device: WAIC and DIC over the observed rows, and the scores of held-out values at
 * NA rows of the problem (the reference's hold-out workflow: set part of y to NA, fit, compare yhat there with the truth).  All of
 * it is CONDITIONAL ON w: saved draw s gives row i of margin j the Gaussian N(mu_s, tau2_j), mu_s = XB_i + w_i, tau2_j = 1 / tausq_inv_j,
 * and nothing integrates the latent field out -- the WAIC penalty therefore counts the effective dimension of w as well.
 * Row i has a target t_i: y_i when observed; y_holdout_i at an NA row with a finite held-out value; none otherwise (outputs NaN).
 * With r_s = (t_i - mu_s) / sqrt(tau2_j), l_s = -r_s^2 / 2 - log(tau2_j) / 2 - log(2 pi) / 2 and the S draws accumulated since _set:
 *   lppd_i = log((1 / S) sum_s exp l_s)   (the streaming log-sum-exp of st_points_score_*),   mean_ll_i = mean_s l_s,
 *   p_waic_i = the sample variance of l_s (0 when S = 1),   mu_mean_i = mean_s mu_s,   pit_i = mean_s Phi(r_s) (held-out rows),
 *   crps_i (held-out rows) = st_points_score_get's formula over the K yhat draws of the row that st_summary_reserve stored.
 * Per outcome j (spamtree_amd/csrc/rows_score.hpp has every operation's order; tau2bar_j = mean_s tau2_j):
 *   observed rows: lppd, p_waic, waic = -2 (lppd - p_waic), Dbar = -2 sum mean_ll, Dhat = -2 sum log N(y_i; mu_mean_i, tau2bar_j),
 *                  p_D = Dbar - Dhat, dic = Dbar + p_D;      held-out rows: the sums of lppd, pit, crps and (t_i - mu_mean_i)^2.
 * st_rows_score_set: y_holdout holds n_all values in model row order, NaN = none; NULL: criteria over the observed rows only.  A
 *   finite value at an observed row, or an infinite value anywhere, is ST_ERR_USAGE naming the row, and the previous state stays.
 *   Allocates and zeroes the state (6 doubles per row, 6 more for the outputs and the CRPS).  st_rows_score_clear frees it.
 * st_rows_score_accumulate: one draw from the current w, XB and tausq_inv, on the handle's stream.  It consumes no draw of any
 *   Philox stream, copies nothing to the host, synchronises nothing and writes nothing another step reads.
 * st_rows_score_get: n_all values each, model row order, NaN where a row has no target (pit, crps: off the held-out rows); any
 *   output may be NULL.  crps without a stored draw (st_summary_reserve before the st_summary_accumulate calls) is ST_ERR_USAGE.
 * st_rows_score_totals: obs is ST_ROWS_OBS_N x q and held ST_ROWS_HELD_N x q, column-major (column j = outcome j), rows as the
 *   macros below; n_obs and n_held hold q counts.  An outcome without rows reports count 0 and zeros.  The crps sums are 0 without
 *   a stored draw.  Any output may be NULL.  Sums, not means: the caller divides by the counts.  The CRPS is sorted once per state
 *   of the stored draws, and only for a call that returns it (crps of _get, held of _totals); the outputs and sums once per state.
 * st_rows_score_info: the algorithmic bytes of one st_rows_score_accumulate, from shapes; needs no device (0 before _set).
 * limited_tree handles are supported (nothing here depends on the tree); world > 1 handles are refused (ST_ERR_UNSUPPORTED).
 * ST_ERR_USAGE with a text: any call before _set; _get / _totals before the first accumulate.
 * A draw whose l_s is not finite (tausq_inv_j of 0 or infinity: a density of 0) leaves the row's log-sum-exp alone and enters the
 * moments of l at their running mean: lppd stays the log of the mean density, but mean_ll and p_waic (hence Dbar, p_D, dic) are then
 * not the moments of the draws, and tau2bar_j, Dhat, p_D and dic may be infinite.  Nothing is NaN. */
#define ST_ROWS_OBS_LPPD 0
#define ST_ROWS_OBS_P_WAIC 1
#define ST_ROWS_OBS_WAIC 2
#define ST_ROWS_OBS_DBAR 3
#define ST_ROWS_OBS_DHAT 4
#define ST_ROWS_OBS_P_D 5
#define ST_ROWS_OBS_DIC 6
#define ST_ROWS_OBS_N 7
#define ST_ROWS_HELD_LPPD 0
#define ST_ROWS_HELD_PIT 1
#define ST_ROWS_HELD_CRPS 2
#define ST_ROWS_HELD_SQERR 3
#define ST_ROWS_HELD_N 4
int st_rows_score_set(st_handle h, const double *y_holdout);
int st_rows_score_clear(st_handle h);
int st_rows_score_accumulate(st_handle h);
int st_rows_score_get(st_handle h, double *lppd, double *p_waic, double *mean_ll, double *mu_mean, double *pit, double *crps,
                      int64_t *n_accumulated);
int st_rows_score_totals(st_handle h, double *obs, double *held, int64_t *n_obs, int64_t *n_held);
int st_rows_score_info(st_handle h, double *alg_bytes);

/* ---- leave-one-out criteria with the latent field integrated out, on the device.  Unlike st_rows_score_*, which is conditional
 * on w, saved draw s gives an observed row i of margin j the density of y_i with its own w_i integrated out against the prior
 * full conditional w_i | w_-i, theta ~ N(m_i, v_i) of the tree's DAG:  v_i = 1 / Q_ii,  m_i = w_i - (Qw)_i / Q_ii,  Q = sum_u L_u' L_u
 * over slot 0's panels of the blocks with observed rows (prediction blocks take no part; spamtree_amd/csrc/loo_kernels.hpp has the
 * definition, the order of every sum and the rounding bound).  mu_s = XB_i + m_i, sigma2_s = v_i + 1 / tausq_inv_j,
 * l_s = log N(y_i; mu_s, sigma2_s), Phi_s = Phi((y_i - mu_s) / sigma_s), and over the S accumulated draws, r_s = exp(-l_s):
 *   elpd_loo_i = -log((1 / S) sum r_s)   (estimates log p(y_i | y_-i): E_post[1 / p(y_i | w_-i, theta, beta, tau2)] = 1 / p(y_i | y_-i)),
 *   pit_loo_i = sum r_s Phi_s / sum r_s,   mu_loo_i = sum r_s mu_s / sum r_s,   weight_ess_i = (sum r_s)^2 / sum r_s^2.
 * These are the raw weights, with weight_ess as their diagnostic; Pareto smoothing and k-hat are st_rows_loo_reserve / st_rows_loo_psis
 * below.  No leave-one-out for NA rows (pass them as new points).
 * st_rows_loo_set: allocates and zeroes the state; st_rows_loo_clear frees it.
 * st_rows_loo_accumulate: one draw from the current w, XB, tausq_inv and slot 0 (a deferred leaf half is finished first, as
 *   st_simulate does): one launch per level from the deepest to the root.  It consumes no Philox draw, copies nothing to the host,
 *   synchronises nothing and changes no state but its own.  A draw whose l_s is not finite at a row is skipped there and counted.
 * st_rows_loo_last: Q_ii, (Qw)_i, m_i and v_i of the last accumulate, n_all values each in model row order, for every row of a
 *   block of the density (NA rows of such a block included); NaN at the rows of prediction blocks.
 * st_rows_loo_get: n_all values each, model row order, NaN where a row has no observed y (or every draw was skipped); n_skipped is
 *   the number of (row, draw) pairs skipped.  A row's sums run over the draws not skipped at that row.
 * st_rows_loo_totals: tot is ST_ROWS_LOO_N x q column-major (column j = outcome j) over the outcome's observed rows; n_obs: q counts.
 * st_rows_loo_info: the bit set of routes of one accumulate (bit code - 1), its algorithmic bytes and flops, from shapes.
 * st_rows_loo_route_name: the kernel behind a route code (NULL outside the table).
 * Any output may be NULL.  Refused with a text, the handle stays usable: limited_tree and world > 1 handles (ST_ERR_UNSUPPORTED);
 * any call before _set, _accumulate before slot 0 was factorised, _get / _totals / _last before the first accumulate (ST_ERR_USAGE). */
#define ST_ROWS_LOO_ELPD 0
#define ST_ROWS_LOO_LOOIC 1
#define ST_ROWS_LOO_SQERR 2
#define ST_ROWS_LOO_PIT 3
#define ST_ROWS_LOO_MIN_ESS 4
#define ST_ROWS_LOO_COUNT 5
#define ST_ROWS_LOO_N 6
int st_rows_loo_set(st_handle h);
int st_rows_loo_clear(st_handle h);
int st_rows_loo_accumulate(st_handle h);
int st_rows_loo_last(st_handle h, double *q_diag, double *qw, double *cond_mean, double *cond_var);
int st_rows_loo_get(st_handle h, double *elpd_loo, double *pit_loo, double *mu_loo, double *weight_ess, int64_t *n_accumulated,
                    int64_t *n_skipped);
int st_rows_loo_totals(st_handle h, double *tot, int64_t *n_obs);
int st_rows_loo_info(st_handle h, int32_t *route_mask, double *alg_bytes, double *flops);
const char *st_rows_loo_route_name(int32_t code);

/* ---- leave-group-out criteria: a group of rows (a site's outcomes, a small spatial block) left out together, its rows of the
 * latent field integrated out jointly.  Saved draw s gives group G, with o its members with an observed y,
 *   A = Q_GG,  V = A^-1,  m_G = w_G - V (Qw)_G,  mu_o = XB_o + m_o,  Sigma = V_oo + diag(1 / tausq_inv_{j(a)}),
 *   l_s = log N(y_o; mu_o, Sigma),  Phi_a = Phi((y_a - mu_a) / sqrt(Sigma_aa)),
 * and over the S accumulated draws, r_s = exp(-l_s): elpd_lgo_G = -log((1 / S) sum r_s), which estimates log p(y_G | y_-G),
 * weight_ess_G = (sum r_s)^2 / sum r_s^2, and per observed member mu_lgo and pit_lgo weighted by r_s
 * (spamtree_amd/csrc/lgo_kernels.hpp has the definition, the order of every operation and the rounding bound).  The off-diagonal
 * entries of Q_GG are column-pair sums over the panels the sweep of st_rows_loo_accumulate reads anyway: with groups set that one
 * sweep serves rows and groups, and everything st_rows_loo_* reports stays bit for bit what it is without groups.
 * st_rows_loo_groups_set: labels, n_all values in model row order, negative = in no group.  A group is the set of rows with one label
 *   that lie in a block of the density (labelled rows of prediction blocks are ignored; a member without an observed y is
 *   integrated out with the group and not scored).  Groups are numbered by ascending label, members stand in ascending model row.
 *   After st_rows_loo_set and before the first accumulate.  Refused with a text, the previous state kept: a group of more than
 *   ST_ROWS_LGO_MAX_MEMBERS members (ST_ERR_UNSUPPORTED, with both numbers), a group without an observed member, no
 *   st_rows_loo_set, an accumulated iteration (ST_ERR_USAGE); limited_tree and world > 1 handles as st_rows_loo_set.
 * st_rows_loo_groups_clear: the groups leave (before the first accumulate, or after st_rows_loo_set anew); st_rows_loo_set and
 *   st_rows_loo_clear drop them too.
 * st_rows_loo_groups_count: the groups, their members in all, the non-structural member pairs, and the doubles of one of _last's
 *   matrix arguments (sum of g^2).
 * st_rows_loo_groups_index: CSR from group to member rows: label (n_groups), ptr (n_groups + 1), rows (n_members, model rows).
 * st_rows_loo_groups_last: of the last accumulate, group after group: Q_GG and cond_cov = V (g x g row-major each), (Qw)_G and
 *   cond_mean = m_G (n_members each).
 * st_rows_loo_groups_get: per group elpd_lgo, weight_ess (NaN when every draw was skipped) and the draws skipped; per row, n_all
 *   values in model row order, mu_lgo and pit_lgo, NaN off the observed members.
 * st_rows_loo_groups_totals: tot, ST_ROWS_LGO_N values over the groups with a value: sum elpd_lgo, the criterion -2 sum, its
 *   standard error sqrt(G var) (var with divisor G - 1; NaN below two groups), min weight_ess, the count; by_outcome,
 *   ST_ROWS_LGO_OUT_N x q column-major over the outcome's observed members: sum (y - mu_lgo)^2, sum pit_lgo, the count.
 * With a store (st_rows_loo_reserve below, called before or after the groups are set) every draw's group log ratio t_s = -l_s is
 * kept too, 8 B per group and draw, NaN where the draw is skipped for the group; the streaming outputs do not change.
 * st_rows_loo_groups_draws: the stored ratios, [n_accumulated][n_groups].
 * st_rows_loo_groups_psis: st_psis' kernel over them, one series per group without companions: khat, elpd_psis, weight_ess_psis,
 *   tail_len and n_draws per group.  Both need a store and one accumulate (ST_ERR_USAGE).
 * Any output may be NULL.  Before the first accumulate _last, _get and _totals are ST_ERR_USAGE. */
#define ST_ROWS_LGO_MAX_MEMBERS 16
#define ST_ROWS_LGO_ELPD 0
#define ST_ROWS_LGO_IC 1
#define ST_ROWS_LGO_SE 2
#define ST_ROWS_LGO_MIN_ESS 3
#define ST_ROWS_LGO_COUNT 4
#define ST_ROWS_LGO_N 5
#define ST_ROWS_LGO_OUT_SQERR 0
#define ST_ROWS_LGO_OUT_PIT 1
#define ST_ROWS_LGO_OUT_COUNT 2
#define ST_ROWS_LGO_OUT_N 3
int st_rows_loo_groups_set(st_handle h, const int64_t *labels);
int st_rows_loo_groups_clear(st_handle h);
int st_rows_loo_groups_count(st_handle h, int64_t *n_groups, int64_t *n_members, int64_t *n_pairs, int64_t *n_matrix);
int st_rows_loo_groups_index(st_handle h, int64_t *label, int64_t *ptr, int64_t *rows);
int st_rows_loo_groups_last(st_handle h, double *q_gg, double *qw, double *cond_mean, double *cond_cov);
int st_rows_loo_groups_get(st_handle h, double *elpd_lgo, double *weight_ess, int64_t *n_skipped, double *mu_lgo, double *pit_lgo,
                           int64_t *n_accumulated);
int st_rows_loo_groups_totals(st_handle h, double *tot, double *by_outcome);
int st_rows_loo_groups_draws(st_handle h, double *t);
int st_rows_loo_groups_psis(st_handle h, double *khat, double *elpd_psis, double *weight_ess_psis, int32_t *tail_len, int32_t *n_draws);

/* ---- Pareto-smoothed importance sampling of the leave-one-out weights, on the device (Vehtari, Simpson, Gelman, Yao, Gabry,
 * "Pareto smoothed importance sampling"; the generalised Pareto fit of Zhang and Stephens with the weakly informative prior of
 * loo::gpdfit; r_eff = 1).  spamtree_amd/psis.py has the definition, spamtree_amd/csrc/psis_kernels.hpp the order the kernel
 * evaluates it in.  A series is K log ratios t_s (the rows' own: t_s = -l_s) with optional companions Phi_s, mu_s; a draw whose t_s
 * is not finite is skipped, S = the finite ones.  Per series: khat, the Pareto shape of the largest M = min(S / 5, ceil(3 sqrt S))
 * ratios (+inf where nothing is smoothed: M < 5, a constant tail, a quarter of the tail tied with the cut, a fit that is not
 * finite; the estimates are then the raw ones), and with the smoothed log weights lw'_s
 *   elpd_psis = log(sum w_s p_s / sum w_s),  pit_psis = sum w_s Phi_s / sum w_s,  mu_psis = sum w_s mu_s / sum w_s,
 *   weight_ess_psis = (sum w_s)^2 / sum w_s^2,  tail_len = M (0: not smoothed),  n_draws = S  (S = 0: NaN, 0, 0).
 * st_rows_loo_reserve: after st_rows_loo_set and before the first accumulate; three [keep][n_all] device arrays (t, Phi, mu: 24 B
 *   per row and draw), NaN until written.  Every st_rows_loo_accumulate then also writes its draw's column (NaN in all three where
 *   the draw is skipped at a row; nothing at rows without an observed y); the streaming outputs are bit for bit the same with and
 *   without a store.  keep = 0 releases the store.  keep outside 0 .. ST_PSIS_MAX_DRAWS: ST_ERR_UNSUPPORTED; a failed allocation
 *   is refused with its size and leaves the handle as it was; an accumulate beyond keep is refused (ST_ERR_USAGE) before any launch.
 * st_rows_loo_draws: the stored columns, [n_accumulated][n_all] each, model row order (the pointwise matrix).
 * st_rows_loo_psis: the outputs of every row, n_all values each in model row order, NaN (0 for the integers) where a row has no
 *   observed y.  st_rows_loo_psis_totals: tot is ST_ROWS_PSIS_N x q column-major over the outcome's observed rows with n_draws > 0;
 *   N_ABOVE counts khat > min(1 - 1 / log10(n_accumulated), 0.7), N_BAD khat > 0.7 (se of elpd_psis = sqrt(n var), formed by the
 *   caller from ELPD and ELPD_SQ).  Both need a store and one accumulate, repeat the refusals of st_rows_loo_get, are repeatable
 *   and leave the streaming state, the store and the chain untouched.
 * st_psis: the same kernel on the caller's host arrays t, phi, mu [K][n] (phi, mu may be NULL: pit_psis, mu_psis are then not
 *   written), 1 <= K <= ST_PSIS_MAX_DRAWS (else ST_ERR_UNSUPPORTED); n = 0 is ST_OK with nothing written.  The handle lends its
 *   device, stream and LDS limit only: any handle will do, limited_tree included.
 * st_psis_info: R (series per tile), the padded length, the dynamic LDS and the algorithmic bytes (every log ratio twice, every
 *   companion value and the outputs once) of a pass over an n x K store with n_comp companions under the handle's LDS limit.
 * Any output pointer may be NULL. */
#define ST_PSIS_MAX_DRAWS 16384
#define ST_ROWS_PSIS_COUNT 0
#define ST_ROWS_PSIS_ELPD 1
#define ST_ROWS_PSIS_ELPD_SQ 2
#define ST_ROWS_PSIS_SQERR 3
#define ST_ROWS_PSIS_PIT 4
#define ST_ROWS_PSIS_MIN_ESS 5
#define ST_ROWS_PSIS_MAX_KHAT 6
#define ST_ROWS_PSIS_N_BAD 7
#define ST_ROWS_PSIS_N_ABOVE 8
#define ST_ROWS_PSIS_N 9
typedef struct st_psis_out {
  double *khat, *elpd_psis, *pit_psis, *mu_psis, *weight_ess_psis;
  int32_t *tail_len, *n_draws;
} st_psis_out;
int st_rows_loo_reserve(st_handle h, int64_t keep);
int st_rows_loo_draws(st_handle h, double *t, double *phi, double *mu);
int st_rows_loo_psis(st_handle h, const st_psis_out *out);
int st_rows_loo_psis_totals(st_handle h, double *tot, int64_t *n_obs);
int st_psis(st_handle h, int64_t n, int64_t K, const double *t, const double *phi, const double *mu, const st_psis_out *out);
int st_psis_info(st_handle h, int64_t n, int64_t K, int32_t n_comp, int32_t *R, int32_t *Kpad, int64_t *lds_bytes, double *alg_bytes);

/* ---- prior simulation from slot 0: exact draws w ~ N(0, C_DAG) of the tree's own model and y = XB + w + sqrt(tau^2_j) eps.
 * st_simulate: a root-to-leaf sweep over slot 0 as the last st_factor(h, 0, theta) left it (a deferred leaf half is finished
 *   first), Ri_u w_u = z_u - N_u w_pa(u) per block, with the handle's current beta (XB) and tau^-2.  nd draws (1..16) in one
 *   sweep; draw d uses Philox counter (row in model order, iter0 + d, stream 8) for z and stream 9 for eps, or the caller's z /
 *   eps (n_all x nd column-major, model row order; NULL: Philox).  w_out, y_out: n_all x nd column-major, model row order; either
 *   may be NULL (y_out NULL: no outcomes; w_out NULL: the draws stay on the device).  A draw does not depend on nd (bitwise).
 *   Changes no state of the handle: w, XB, both slots, the records and the chain's streams stay as they are.  Refused before any
 *   launch: NA rows or world > 1 (ST_ERR_UNSUPPORTED), nd outside 1..16 or slot 0 never factorised (ST_ERR_USAGE).
 * st_simulate_info: the bit set of routes the sweep takes (bit code - 1; a function of the tree only), the algorithmic bytes
 *   (every panel once + 8 nd B per row for z, eps, w, y and the ancestor gathers + 8 B per row for XB) and flops of an nd-draw call.
 * st_simulate_route_name: the kernel behind a route code (NULL outside the table). */
int st_simulate(st_handle h, int nd, const double *z, const double *eps, uint64_t seed, uint32_t iter0, double *w_out, double *y_out);
int st_simulate_info(st_handle h, int nd, int32_t *route_mask, double *alg_bytes, double *flops);
const char *st_simulate_route_name(int32_t code);

int st_set_stream(st_handle h, void *stream);              /* launch on the caller's stream (the one its collectives use) */

/* ---- multi-GPU (st_options.world > 1): one process per GPU shares ONE problem.
 * Ownership: whole subtrees below a cut level belong to one rank, levels above the cut are replicated
 * (st_shard_plan is pure host code: owner[u] = rank or -1 for replicated; no GPU needed).
 * Every exchange is an all-reduce(sum) in which each entry is contributed by exactly one rank and is zero on the
 * others, so the result is bit-identical to the single-GPU arrays for any number of ranks.  The caller owns the
 * collective (RCCL through torch.distributed on the stream given to st_set_stream); the single-call forms
 * (st_factor, st_sample_w, st_loglik_w) are the world == 1 composition of the same steps.
 *   phase A : st_factor_local -> st_mg_pack_comps -> all-reduce(buf) -> st_mg_finish        (code 0/1/2/3, loglik)
 *   phase C : st_loglik_local -> st_mg_pack_comps -> all-reduce(buf) -> st_mg_finish
 *   phase B : st_sample_w_local -> all-reduce(st_mg_top_region) -> st_sample_w_top
 *             -> st_mg_pack_w -> all-reduce(buf) -> st_mg_unpack_w                           (code 0/10/11) */
/* native exchange: rank 0 creates a 128-byte RCCL unique id (returns its size), every rank passes it to st_comm_init;
 * afterwards the single-call forms run the steps above with ncclAllReduce on the library's stream */
int st_comm_unique_id(void *out, int32_t cap);
int st_comm_init(st_handle h, const void *unique_id);
int st_shard_plan(const st_problem *pb, int32_t world, int64_t *owner /* n_blocks */, int32_t *cut_level);
/* the same with options (needed for limited_tree problems, whose single-parent lists only parse with reserved bit 1 set) */
int st_shard_plan_opt(const st_problem *pb, const st_options *opt, int32_t world, int64_t *owner /* n_blocks */, int32_t *cut_level);
int st_shard_info(st_handle h, int32_t *rank, int32_t *world, int32_t *cut_level, int64_t *owned_blocks, int64_t *owned_rows);
int st_factor_local(st_handle h, int slot, const double *theta, int ntheta);
int st_loglik_local(st_handle h, int slot);
int st_mg_pack_comps(st_handle h, int slot, void **dev_ptr, int64_t *len);
int st_mg_finish(st_handle h, double *loglik);
int st_sample_w_local(st_handle h, const double *z, uint64_t seed, uint32_t iter);
int st_mg_top_region(st_handle h, void **dev_ptr, int64_t *len);
int st_sample_w_top(st_handle h);
int st_mg_pack_w(st_handle h, void **dev_ptr, int64_t *len);
int st_mg_unpack_w(st_handle h);
/* all-gather form of the last step of phase B (half the traffic of the all-reduce of n doubles; what the native path uses):
 * every rank's slice of the receive buffer holds its owned rows in device order + its failure word, `count_per_rank`
 * doubles each (the same on all ranks); the replicated top is sampled identically everywhere and does not travel.
 *   st_mg_gather_w_pack -> all-gather(send = recv + rank * count, recv) -> st_mg_gather_w_unpack      (code 0/10/11) */
int st_mg_gather_w_pack(st_handle h, void **send_ptr, void **recv_ptr, int64_t *count_per_rank);
int st_mg_gather_w_unpack(st_handle h);

#ifdef __cplusplus
}
#endif
#endif /* SPAMTREE_HIP_H */

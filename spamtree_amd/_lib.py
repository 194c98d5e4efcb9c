"""ctypes binding of include/spamtree_hip.h.  No fallback: a missing library or GPU is an error."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# SPAMTREE_LIB: an alternative build of the SAME library (A/B timing of kernel variants under profiles/micro); never a fallback
LIB_PATH = os.environ.get("SPAMTREE_LIB") or os.path.join(HERE, "libspamtree_hip.so")

ST_MAX_P = 64   # include/spamtree_hip.h: the most regressors st_create accepts

c_dp = C.POINTER(C.c_double)
c_ip = C.POINTER(C.c_int64)


class StProblem(C.Structure):
    _fields_ = [("n_all", C.c_int64), ("d", C.c_int32), ("q", C.c_int32), ("p", C.c_int32), ("n_groups", C.c_int32),
                ("n_blocks", C.c_int64), ("y", c_dp), ("X", c_dp), ("coords", c_dp), ("mv_id", c_ip),
                ("res_is_ref", c_ip), ("block_names", c_ip), ("block_groups", c_ip), ("indexing_ptr", c_ip),
                ("indexing_idx", c_ip), ("parents_ptr", c_ip), ("parents_idx", c_ip), ("children_ptr", c_ip),
                ("children_idx", c_ip)]


class StOptions(C.Structure):
    _fields_ = [("device", C.c_int32), ("reference_quirks", C.c_int32), ("rank", C.c_int32), ("world", C.c_int32),
                ("force_generic", C.c_int32), ("reserved", C.c_int32)]


class StSeriesDiag(C.Structure):   # include/spamtree_hip.h, st_series_diag: n values each, any may be NULL
    _fields_ = [("ess", c_dp), ("mcse", c_dp), ("sd", c_dp), ("rhat", c_dp), ("lags", C.POINTER(C.c_int32))]


class StExcursionSpec(C.Structure):   # include/spamtree_hip.h, st_excursion_spec
    _fields_ = [("n_thr", C.c_int32), ("thr", C.POINTER(C.c_double)), ("side", C.POINTER(C.c_int32)), ("mask", C.POINTER(C.c_uint8)),
                ("want_band", C.c_int32)]


class StExcursionOut(C.Structure):    # st_excursion_out: any pointer may be NULL
    _fields_ = [("count", C.POINTER(C.c_int32)), ("prob", C.POINTER(C.c_double)), ("excur", C.POINTER(C.c_double)),
                ("joint_all", C.POINTER(C.c_double)), ("mean", C.POINTER(C.c_double)), ("sd", C.POINTER(C.c_double)),
                ("maxdev", C.POINTER(C.c_double)), ("n_flat", C.POINTER(C.c_int64)), ("n_draws", C.POINTER(C.c_int64))]


class StRankSpec(C.Structure):        # include/spamtree_hip.h, st_rank_spec
    _fields_ = [("max_lag", C.c_int32), ("n_prob", C.c_int32), ("prob", C.POINTER(C.c_double)), ("n_thr", C.c_int32),
                ("thr", C.POINTER(C.c_double)), ("side", C.POINTER(C.c_int32))]


class StRankOut(C.Structure):         # st_rank_out: any pointer may be NULL
    _fields_ = [("rhat_rank", C.POINTER(C.c_double)), ("rhat_bulk", C.POINTER(C.c_double)), ("rhat_fold", C.POINTER(C.c_double)),
                ("ess_bulk", C.POINTER(C.c_double)), ("ess_tail", C.POINTER(C.c_double)), ("lags_bulk", C.POINTER(C.c_int32)),
                ("ess_q", C.POINTER(C.c_double)), ("ess_exc", C.POINTER(C.c_double)), ("mcse_prob", C.POINTER(C.c_double)),
                ("prob", C.POINTER(C.c_double))]


class StRbOut(C.Structure):           # st_rb_out: n_thr x n, threshold-major; either may be NULL
    _fields_ = [("prob", C.POINTER(C.c_double)), ("prob_var", C.POINTER(C.c_double))]


class StMixOut(C.Structure):          # st_mix_out: q n_probs x n, probability-major; either may be NULL
    _fields_ = [("q", C.POINTER(C.c_double)), ("n_unconverged", C.POINTER(C.c_int64))]


class StPsisOut(C.Structure):         # st_psis_out: n values each, any pointer may be NULL
    _fields_ = [("khat", C.POINTER(C.c_double)), ("elpd_psis", C.POINTER(C.c_double)), ("pit_psis", C.POINTER(C.c_double)),
                ("mu_psis", C.POINTER(C.c_double)), ("weight_ess_psis", C.POINTER(C.c_double)), ("tail_len", C.POINTER(C.c_int32)),
                ("n_draws", C.POINTER(C.c_int32))]


ST_PSIS_MAX_DRAWS = 16384
ST_EXC_MAX_THRESHOLDS = 8
ST_RANK_MAX_PROBS = 8
ST_MIX_MAX_DRAWS = 8192
ST_MIX_MAX_PROBS = 8
ST_DIAG_MIN_DRAWS = 4
ST_DIAG_DEFAULT_MAX_LAG = 1024

# every symbol include/spamtree_hip.h declares: name -> (restype, argtypes)
H = C.c_void_p
c_sdp = C.POINTER(StSeriesDiag)
c_xsp, c_xop = C.POINTER(StExcursionSpec), C.POINTER(StExcursionOut)
c_rsp, c_rop = C.POINTER(StRankSpec), C.POINTER(StRankOut)
c_rbp = C.POINTER(StRbOut)
c_mxp = C.POINTER(StMixOut)
SIGNATURES = {
    "st_create": (C.c_int, [C.POINTER(StProblem), C.POINTER(StOptions), C.POINTER(H)]),
    "st_destroy": (C.c_int, [H]),
    "st_last_error": (C.c_char_p, [H]),
    "st_set_w": (C.c_int, [H, c_dp]),
    "st_get_w": (C.c_int, [H, c_dp]),
    "st_set_beta": (C.c_int, [H, c_dp]),
    "st_set_tausq_inv": (C.c_int, [H, c_dp]),
    "st_get_xb": (C.c_int, [H, c_dp]),
    "st_get_resid": (C.c_int, [H, c_dp, C.c_int64]),
    "st_factor": (C.c_int, [H, C.c_int, c_dp, C.c_int, c_dp]),
    "st_factor_begin": (C.c_int, [H, C.c_int, c_dp, C.c_int]),
    "st_factor_ahead_levels": (C.c_int, [H]),
    "st_swap": (C.c_int, [H]),
    "st_sample_w": (C.c_int, [H, c_dp, C.c_uint64, C.c_uint32]),
    "st_loglik_w": (C.c_int, [H, C.c_int, c_dp]),
    "st_sample_w_loglik": (C.c_int, [H, c_dp, C.c_uint64, C.c_uint32, C.c_int, c_dp]),
    "st_sample_w_loglik_begin": (C.c_int, [H, c_dp, C.c_uint64, C.c_uint32, C.c_int]),
    "st_sample_w_loglik_end": (C.c_int, [H, c_dp]),
    "st_predict": (C.c_int, [H, C.c_int]),
    "st_beta_stats": (C.c_int, [H, c_dp]),
    "st_tausq_stats": (C.c_int, [H, c_dp, c_ip]),
    "st_xtx": (C.c_int, [H, c_dp]),
    "st_yhat": (C.c_int, [H, c_dp, C.c_uint64, C.c_uint32, c_dp]),
    "st_block_dims": (C.c_int, [H, C.c_int64, c_ip, c_ip, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "st_get_block": (C.c_int, [H, C.c_int, C.c_int64, c_dp, c_dp]),
    "st_get_comps": (C.c_int, [H, C.c_int, c_dp, c_dp]),
    "st_algorithmic_bytes": (C.c_int, [H, c_dp, c_dp]),
    "st_factor_ahead_enable": (C.c_int, [H, C.c_int]),
    "st_probe_peaks": (C.c_int, [C.c_int, C.c_int64, C.c_int, c_dp]),
    "st_probe_math": (C.c_int, [C.c_int32, c_dp, C.c_int64, C.c_int32, c_dp]),
    "st_probe_group_sum": (C.c_int, [C.c_int32, C.c_int32, c_dp, C.c_int64, C.c_int32, c_dp]),
    "st_profile_enable": (C.c_int, [H, C.c_int]),
    "st_profile_get": (C.c_int, [H, c_dp, c_ip]),
    "st_profile_levels": (C.c_int, [H, C.POINTER(C.c_int32), c_dp, c_dp, C.c_int32]),
    "st_level_info": (C.c_int, [H, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                C.POINTER(C.c_int32), C.c_int32]),
    "st_route_info": (C.c_int, [H, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                C.c_int32]),
    "st_route_name": (C.c_char_p, [C.c_int32]),
    "st_synchronize": (C.c_int, [H]),
    "st_stream": (C.c_void_p, [H]),
    "st_set_stream": (C.c_int, [H, C.c_void_p]),
    "st_shard_plan": (C.c_int, [C.POINTER(StProblem), C.c_int32, c_ip, C.POINTER(C.c_int32)]),
    "st_shard_plan_opt": (C.c_int, [C.POINTER(StProblem), C.POINTER(StOptions), C.c_int32, c_ip, C.POINTER(C.c_int32)]),
    "st_shard_info": (C.c_int, [H, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), c_ip, c_ip]),
    "st_factor_local": (C.c_int, [H, C.c_int, c_dp, C.c_int]),
    "st_factor_enqueue": (C.c_int, [H, C.c_int, c_dp, C.c_int]),
    "st_factor_finish": (C.c_int, [H, c_dp]),
    "st_factor_is_async": (C.c_int, [H]),
    "st_loglik_local": (C.c_int, [H, C.c_int]),
    "st_mg_pack_comps": (C.c_int, [H, C.c_int, C.POINTER(C.c_void_p), c_ip]),
    "st_mg_finish": (C.c_int, [H, c_dp]),
    "st_sample_w_local": (C.c_int, [H, c_dp, C.c_uint64, C.c_uint32]),
    "st_mg_top_region": (C.c_int, [H, C.POINTER(C.c_void_p), c_ip]),
    "st_sample_w_top": (C.c_int, [H]),
    "st_mg_pack_w": (C.c_int, [H, C.POINTER(C.c_void_p), c_ip]),
    "st_mg_unpack_w": (C.c_int, [H]),
    "st_mg_gather_w_pack": (C.c_int, [H, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), c_ip]),
    "st_mg_gather_w_unpack": (C.c_int, [H]),
    "st_cross_covariance_ag10": (C.c_int, [c_dp, c_ip, C.c_int64, c_dp, c_ip, C.c_int64, c_dp, c_dp, c_dp, c_dp, c_dp, C.c_int32,
                                           C.c_int32, c_dp]),
    "st_summary_reset": (C.c_int, [H]),
    "st_summary_accumulate": (C.c_int, [H, C.c_uint64, C.c_uint32]),
    "st_summary_get": (C.c_int, [H, c_dp, c_dp, c_ip]),
    "st_summary_reserve": (C.c_int, [H, C.c_int64]),
    "st_summary_quantile": (C.c_int, [H, C.c_double, c_dp, c_dp]),
    "st_summary_diagnostics": (C.c_int, [H, C.c_int32, c_sdp, c_sdp]),
    "st_points_summary_diagnostics": (C.c_int, [H, C.c_int32, c_sdp, c_sdp]),
    "st_points_functionals_diagnostics": (C.c_int, [H, C.c_int32, c_sdp, c_sdp]),
    "st_summary_excursions": (C.c_int, [H, c_xsp, c_xop, c_xop]),
    "st_points_summary_excursions": (C.c_int, [H, c_xsp, c_xop, c_xop]),
    "st_points_functionals_excursions": (C.c_int, [H, c_xsp, c_xop, c_xop]),
    "st_summary_rank_diagnostics": (C.c_int, [H, c_rsp, c_rop, c_rop]),
    "st_points_summary_rank_diagnostics": (C.c_int, [H, c_rsp, c_rop, c_rop]),
    "st_points_functionals_rank_diagnostics": (C.c_int, [H, c_rsp, c_rop, c_rop]),
    "st_summary_chain_diagnostics": (C.c_int, [H, C.c_int32, C.c_int32, c_sdp, c_sdp]),
    "st_points_summary_chain_diagnostics": (C.c_int, [H, C.c_int32, C.c_int32, c_sdp, c_sdp]),
    "st_points_functionals_chain_diagnostics": (C.c_int, [H, C.c_int32, C.c_int32, c_sdp, c_sdp]),
    "st_summary_chain_rank_diagnostics": (C.c_int, [H, C.c_int32, c_rsp, c_rop, c_rop]),
    "st_points_summary_chain_rank_diagnostics": (C.c_int, [H, C.c_int32, c_rsp, c_rop, c_rop]),
    "st_points_functionals_chain_rank_diagnostics": (C.c_int, [H, C.c_int32, c_rsp, c_rop, c_rop]),
    "st_norm_quantile": (C.c_int, [c_dp, c_dp, C.c_int64]),
    "st_comm_unique_id": (C.c_int, [C.c_void_p, C.c_int32]),
    "st_comm_init": (C.c_int, [H, C.c_void_p]),
    "st_points_set": (C.c_int, [H, C.c_int64, c_dp, c_ip, c_ip, c_dp]),
    "st_points_predict": (C.c_int, [H, C.c_int, c_dp, C.c_uint64, C.c_uint32, c_dp, c_dp, c_dp, c_dp]),
    "st_points_info": (C.c_int, [H, C.POINTER(C.c_int32), c_ip, c_dp, c_dp]),
    "st_points_route_name": (C.c_char_p, [C.c_int32]),
    "st_points_accumulate": (C.c_int, [H, C.c_uint64, C.c_uint32, c_dp, c_dp, c_dp, c_dp]),
    "st_points_summary_reset": (C.c_int, [H]),
    "st_points_summary_reserve": (C.c_int, [H, C.c_int64]),
    "st_points_summary_get": (C.c_int, [H, c_dp, c_dp, c_dp, c_dp, c_ip]),
    "st_points_summary_quantile": (C.c_int, [H, C.c_double, c_dp, c_dp]),
    "st_points_set_joint": (C.c_int, [H, C.c_int64, c_dp, c_ip, c_ip, c_dp, c_ip]),
    "st_points_joint_layout": (C.c_int, [H, c_ip, c_ip, c_ip, c_ip]),
    "st_points_predict_joint": (C.c_int, [H, C.c_int, c_dp, C.c_uint64, C.c_uint32, c_dp, c_dp, c_dp, c_dp, c_dp]),
    "st_points_accumulate_joint": (C.c_int, [H, C.c_uint64, C.c_uint32, c_dp, c_dp, c_dp, c_dp, c_dp]),
    "st_points_summary_get_cov": (C.c_int, [H, c_dp]),
    "st_points_functionals_set": (C.c_int, [H, C.c_int64, c_ip, c_ip, c_dp]),
    "st_points_functionals_last": (C.c_int, [H, c_dp, c_dp, c_dp, c_dp]),
    "st_points_functionals_get": (C.c_int, [H, c_dp, c_dp, c_dp, c_dp, c_ip]),
    "st_points_functionals_quantile": (C.c_int, [H, C.c_double, c_dp, c_dp]),
    "st_points_functionals_info": (C.c_int, [H, c_ip, c_ip, c_ip, c_ip, c_dp]),
    "st_points_score_set": (C.c_int, [H, c_dp]),
    "st_points_score_get": (C.c_int, [H, c_dp, c_dp, c_dp, c_dp, c_ip, c_ip]),
    "st_points_exceed_set": (C.c_int, [H, C.c_int32, c_dp, C.POINTER(C.c_int32), c_dp]),
    "st_points_exceed_get": (C.c_int, [H, c_rbp, c_rbp, c_rbp, c_ip]),
    "st_points_mixture_reserve": (C.c_int, [H, C.c_int64]),
    "st_points_mixture_draws": (C.c_int, [H, c_dp, c_dp, c_dp, c_dp, c_ip]),
    "st_points_mixture_quantiles": (C.c_int, [H, C.c_int32, c_dp, c_mxp, c_mxp, c_mxp]),
    "st_points_mixture_crps": (C.c_int, [H, c_dp, c_dp, c_ip]),
    "st_points_mixture_info": (C.c_int, [H, c_ip, c_ip, c_dp, c_ip, c_ip]),
    "st_rows_score_set": (C.c_int, [H, c_dp]),
    "st_rows_score_clear": (C.c_int, [H]),
    "st_rows_score_accumulate": (C.c_int, [H]),
    "st_rows_score_get": (C.c_int, [H, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_ip]),
    "st_rows_score_totals": (C.c_int, [H, c_dp, c_dp, c_ip, c_ip]),
    "st_rows_score_info": (C.c_int, [H, c_dp]),
    "st_rows_loo_set": (C.c_int, [H]),
    "st_rows_loo_clear": (C.c_int, [H]),
    "st_rows_loo_accumulate": (C.c_int, [H]),
    "st_rows_loo_last": (C.c_int, [H, c_dp, c_dp, c_dp, c_dp]),
    "st_rows_loo_get": (C.c_int, [H, c_dp, c_dp, c_dp, c_dp, c_ip, c_ip]),
    "st_rows_loo_totals": (C.c_int, [H, c_dp, c_ip]),
    "st_rows_loo_info": (C.c_int, [H, C.POINTER(C.c_int32), c_dp, c_dp]),
    "st_rows_loo_route_name": (C.c_char_p, [C.c_int32]),
    "st_rows_loo_groups_set": (C.c_int, [H, c_ip]),
    "st_rows_loo_groups_clear": (C.c_int, [H]),
    "st_rows_loo_groups_count": (C.c_int, [H, c_ip, c_ip, c_ip, c_ip]),
    "st_rows_loo_groups_index": (C.c_int, [H, c_ip, c_ip, c_ip]),
    "st_rows_loo_groups_last": (C.c_int, [H, c_dp, c_dp, c_dp, c_dp]),
    "st_rows_loo_groups_get": (C.c_int, [H, c_dp, c_dp, c_ip, c_dp, c_dp, c_ip]),
    "st_rows_loo_groups_totals": (C.c_int, [H, c_dp, c_dp]),
    "st_rows_loo_groups_draws": (C.c_int, [H, c_dp]),
    "st_rows_loo_groups_psis": (C.c_int, [H, c_dp, c_dp, c_dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "st_rows_loo_reserve": (C.c_int, [H, C.c_int64]),
    "st_rows_loo_draws": (C.c_int, [H, c_dp, c_dp, c_dp]),
    "st_rows_loo_psis": (C.c_int, [H, C.POINTER(StPsisOut)]),
    "st_rows_loo_psis_totals": (C.c_int, [H, c_dp, c_ip]),
    "st_psis": (C.c_int, [H, C.c_int64, C.c_int64, c_dp, c_dp, c_dp, C.POINTER(StPsisOut)]),
    "st_psis_info": (C.c_int, [H, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), c_ip, c_dp]),
    "st_simulate": (C.c_int, [H, C.c_int, c_dp, c_dp, C.c_uint64, C.c_uint32, c_dp, c_dp]),
    "st_simulate_info": (C.c_int, [H, C.c_int, C.POINTER(C.c_int32), c_dp, c_dp]),
    "st_simulate_route_name": (C.c_char_p, [C.c_int32]),
}


class StmFlags(C.Structure):
    _fields_ = [("adapting", C.c_int32), ("sample_beta", C.c_int32), ("sample_tausq", C.c_int32),
                ("sample_theta", C.c_int32), ("sample_w", C.c_int32), ("sample_predicts", C.c_int32)]


class StmFunctionals(C.Structure):   # include/spamtree_fit.h, stm_functionals
    _fields_ = [("n_fun", C.c_int64), ("ptr", c_ip), ("idx", c_ip), ("wt", c_dp),
                ("fun_w", c_dp), ("fun_cond_mean", c_dp), ("fun_cond_var", c_dp), ("fun_yhat", c_dp),
                ("fun_mean", c_dp), ("fun_var", c_dp), ("fun_w_mean", c_dp), ("fun_yhat_mean", c_dp),
                ("fun_w_q", c_dp), ("fun_yhat_q", c_dp)]


class StmScores(C.Structure):   # include/spamtree_fit.h, stm_scores
    _fields_ = [("y_new", c_dp), ("lpd", c_dp), ("pit", c_dp), ("crps", c_dp), ("lpd_joint", c_dp),
                ("n_scored", c_ip), ("n_degenerate", c_ip)]


class StmCriteria(C.Structure):   # include/spamtree_fit.h, stm_criteria
    _fields_ = [("y_holdout", c_dp), ("want_crps", C.c_int32), ("lppd", c_dp), ("p_waic", c_dp), ("mean_ll", c_dp),
                ("mu_mean", c_dp), ("pit", c_dp), ("crps", c_dp), ("obs", c_dp), ("held", c_dp), ("n_obs", c_ip),
                ("n_held", c_ip), ("n_accumulated", c_ip)]


ST_ROWS_OBS = ("lppd", "p_waic", "waic", "Dbar", "Dhat", "p_D", "dic")   # include/spamtree_hip.h: ST_ROWS_OBS_*, ST_ROWS_HELD_*
ST_ROWS_HELD = ("lppd", "pit", "crps", "sqerr")
ST_ROWS_LOO = ("elpd_loo", "looic", "sqerr", "pit", "min_weight_ess", "count")   # ST_ROWS_LOO_*
ST_ROWS_LGO = ("elpd_lgo", "lgoic", "se", "min_weight_ess", "n_groups")          # ST_ROWS_LGO_*
ST_ROWS_LGO_OUT = ("sqerr", "pit", "count")                                      # ST_ROWS_LGO_OUT_*
ST_ROWS_LGO_MAX_MEMBERS = 16
ST_ROWS_PSIS = ("count", "elpd_psis", "elpd_psis_sq", "sqerr", "pit", "min_weight_ess", "max_khat", "n_khat_bad", "n_khat_above")   # ST_ROWS_PSIS_*


class StmLooPsis(C.Structure):   # include/spamtree_fit.h, stm_loo_psis
    _fields_ = [("out", StPsisOut), ("tot", c_dp), ("n_obs", c_ip), ("t", c_dp), ("phi", c_dp), ("mu", c_dp)]


class StmLooGroups(C.Structure):   # include/spamtree_fit.h, stm_loo_groups
    _fields_ = [("labels", c_ip), ("n_groups", c_ip), ("n_members", c_ip), ("n_pairs", c_ip), ("label", c_ip), ("ptr", c_ip), ("rows", c_ip),
                ("elpd_lgo", c_dp), ("weight_ess", c_dp), ("n_skipped", c_ip), ("mu_lgo", c_dp), ("pit_lgo", c_dp), ("tot", c_dp),
                ("by_outcome", c_dp), ("khat", c_dp), ("elpd_psis", c_dp), ("weight_ess_psis", c_dp)]


class StmLoo(C.Structure):   # include/spamtree_fit.h, stm_loo
    _fields_ = [("elpd_loo", c_dp), ("pit_loo", c_dp), ("mu_loo", c_dp), ("weight_ess", c_dp), ("tot", c_dp), ("n_obs", c_ip),
                ("n_accumulated", c_ip), ("n_skipped", c_ip), ("psis", C.POINTER(StmLooPsis)), ("groups", C.POINTER(StmLooGroups))]


class StmDiagnostics(C.Structure):   # include/spamtree_fit.h, stm_diagnostics
    _fields_ = [("max_lag", C.c_int32), ("want_rows", C.c_int32), ("rows_w", StSeriesDiag), ("rows_yhat", StSeriesDiag),
                ("new_w", StSeriesDiag), ("new_yhat", StSeriesDiag), ("fun_w", StSeriesDiag), ("fun_yhat", StSeriesDiag)]


class StmRbExceed(C.Structure):      # include/spamtree_fit.h, stm_rb_exceed
    _fields_ = [("n_thr", C.c_int32), ("thr", c_dp), ("side", C.POINTER(C.c_int32)), ("thr_fun", c_dp),
                ("new_w", StRbOut), ("new_yhat", StRbOut), ("fun_w", StRbOut), ("n_accumulated", c_ip)]


class StmExcursions(C.Structure):    # include/spamtree_fit.h, stm_excursions
    _fields_ = [("want_rows", C.c_int32), ("rows_spec", StExcursionSpec), ("new_spec", StExcursionSpec), ("fun_spec", StExcursionSpec),
                ("rows_w", StExcursionOut), ("rows_yhat", StExcursionOut), ("new_w", StExcursionOut), ("new_yhat", StExcursionOut),
                ("fun_w", StExcursionOut), ("fun_yhat", StExcursionOut), ("rb", C.POINTER(StmRbExceed))]


class StmRankDiagnostics(C.Structure):    # include/spamtree_fit.h, stm_rank_diagnostics
    _fields_ = [("want_rows", C.c_int32), ("rows_spec", StRankSpec), ("new_spec", StRankSpec), ("fun_spec", StRankSpec),
                ("rows_w", StRankOut), ("rows_yhat", StRankOut), ("new_w", StRankOut), ("new_yhat", StRankOut),
                ("fun_w", StRankOut), ("fun_yhat", StRankOut)]


class StmChains(C.Structure):             # include/spamtree_fit.h, stm_chains
    _fields_ = [("n_chains", C.c_int32), ("seeds", C.POINTER(C.c_uint64)), ("theta0", c_dp), ("paramsd", c_dp), ("chain_time", c_dp)]


class StmRun(C.Structure):                # include/spamtree_fit.h, stm_run: the twenty arguments of spamtree_mv_mcmc_c
    _fields_ = [("pb", C.POINTER(StProblem)), ("opt", C.POINTER(StOptions)), ("set_unif_bounds", c_dp), ("theta", c_dp),
                ("ntheta", C.c_int), ("beta", c_dp), ("tausq", C.c_double), ("mcmcsd", c_dp), ("mcmc_keep", C.c_int),
                ("mcmc_burn", C.c_int), ("mcmc_thin", C.c_int), ("seed", C.c_uint64), ("flags", C.POINTER(StmFlags)),
                ("w_mcmc", c_dp), ("yhat_mcmc", c_dp), ("beta_mcmc", c_dp), ("tausq_mcmc", c_dp), ("theta_mcmc", c_dp),
                ("paramsd", c_dp), ("mcmc_time", c_dp)]


class StmNewPoints(C.Structure):          # include/spamtree_fit.h, stm_new_points: the point arguments of stm_mcmc_points_joint
    _fields_ = [("n_new", C.c_int64), ("coords_new", c_dp), ("mv_new", c_ip), ("anchor_new", c_ip), ("X_new", c_dp),
                ("joint_id_new", c_ip), ("keep_draws", C.c_int64), ("quantiles", c_dp), ("n_quantiles", C.c_int32),
                ("new_w", c_dp), ("new_cond_mean", c_dp), ("new_cond_var", c_dp), ("new_yhat", c_dp), ("new_mean", c_dp),
                ("new_var", c_dp), ("new_w_mean", c_dp), ("new_yhat_mean", c_dp), ("new_w_q", c_dp), ("new_yhat_q", c_dp),
                ("new_route", C.POINTER(C.c_int32)), ("new_cond_cov", c_dp), ("new_cov", c_dp)]


class StmFit(C.Structure):                # include/spamtree_fit.h, stm_fit: the run and its optional parts (NULL: none)
    _fields_ = [("run", StmRun), ("pts", C.POINTER(StmNewPoints)), ("fun", C.POINTER(StmFunctionals)), ("scores", C.POINTER(StmScores)),
                ("diag", C.POINTER(StmDiagnostics)), ("exc", C.POINTER(StmExcursions)), ("rk", C.POINTER(StmRankDiagnostics)),
                ("ch", C.POINTER(StmChains)), ("criteria", C.POINTER(StmCriteria)), ("loo", C.POINTER(StmLoo))]


class StmMixture(C.Structure):            # include/spamtree_fit.h, stm_mixture
    _fields_ = [("probs", c_dp), ("n_probs", C.c_int32), ("new_w", StMixOut), ("new_yhat", StMixOut), ("fun_w", StMixOut),
                ("crps", c_dp), ("spread", c_dp), ("n_stored", c_ip)]


class StmFitMore(C.Structure):            # include/spamtree_fit.h, stm_fit_more: the parts that travel beside the request
    _fields_ = [("mix", C.POINTER(StmMixture))]


# include/spamtree_fit.h (C++ host driver).  The positional whole-fit entry points take the fields of the request in its order: the
# run's, then (the points family) the point set's and one pointer per further part.  JOINT_ONLY: what stm_mcmc_points leaves out.
JOINT_ONLY = ("joint_id_new", "new_cond_cov", "new_cov")
_run = [t for _, t in StmRun._fields_]
_points = [t for _, t in StmNewPoints._fields_]
_parts = dict(StmFit._fields_[2:])
SIGNATURES.update({
    "stm_create": (C.c_int, [C.POINTER(StProblem), C.POINTER(StOptions), c_dp, c_dp, c_dp, C.c_int, c_dp, C.c_double,
                             C.c_uint64, C.POINTER(StmFlags), C.POINTER(H)]),
    "stm_init": (C.c_int, [H]),
    "stm_destroy": (C.c_int, [H]),
    "stm_last_error": (C.c_char_p, [H]),
    "stm_handle": (C.c_void_p, [H]),
    "stm_step": (C.c_int, [H, C.c_int]),
    "stm_state": (C.c_int, [H, c_dp, c_dp, c_dp, c_dp, c_dp, c_ip, c_dp]),
    "stm_points_set": (C.c_int, [H, C.c_int64, c_dp, c_ip, c_ip, c_dp, C.c_int64]),
    "stm_points_set_joint": (C.c_int, [H, C.c_int64, c_dp, c_ip, c_ip, c_dp, c_ip, C.c_int64]),
    "stm_points_functionals_set": (C.c_int, [H, C.c_int64, c_ip, c_ip, c_dp]),
    "stm_points_score_set": (C.c_int, [H, c_dp]),
    "stm_rows_score_set": (C.c_int, [H, c_dp]),
    "stm_points_mixture_reserve": (C.c_int, [H, C.c_int64]),
    "stm_mcmc_fit": (C.c_int, [C.POINTER(StmFit)]),
    "stm_fit_run": (C.c_int, [C.POINTER(StmFit), C.POINTER(StmFitMore)]),
    "stm_mcmc_chains_last_error": (C.c_char_p, []),
    "spamtree_mv_mcmc_c": (C.c_int, _run),
    "stm_mcmc_points": (C.c_int, _run + [t for name, t in StmNewPoints._fields_ if name not in JOINT_ONLY]),
    "stm_mcmc_criteria": (C.c_int, _run + [_parts["criteria"]]),
    "stm_mcmc_loo": (C.c_int, _run + [_parts["criteria"], _parts["loo"]]),
})
# stm_mcmc_points_joint and then one more part each: fun, scores, diag, exc, rk, ch
for _i, _name in enumerate(("points_joint", "functionals", "scored", "diagnosed", "excursions", "ranked", "chains")):
    SIGNATURES["stm_mcmc_" + _name] = (C.c_int, _run + _points + [t for _, t in StmFit._fields_[2:2 + _i]])

# include/spamtree_tree.h (device parts of the tree builder)
c_i32p = C.POINTER(C.c_int32)
SIGNATURES.update({
    "st_tb_sort": (C.c_int, [c_dp, C.c_int64, C.c_int32, c_dp]),
    "st_tb_cell_argmin": (C.c_int, [c_ip, c_dp, c_ip, C.c_int64, C.c_int64, C.c_int32, c_ip]),
    "st_tb_nearest": (C.c_int, [c_dp, c_dp, c_i32p, C.c_int64, c_dp, c_dp, c_i32p, C.c_int64, C.c_int32, C.c_int32, c_ip]),
})

_lib = None


def load():
    """Load libspamtree_hip.so (built by spamtree_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -m spamtree_amd.build` (hipcc, gfx950). "
                           "There is no CPU fallback for the product path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib

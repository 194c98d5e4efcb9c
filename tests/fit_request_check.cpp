// fit_request_check -- a stand-alone host program: the layout of the whole-fit request of include/spamtree_fit.h as the C++
// compiler sees it.  It prints "<struct> <sizeof>" and "<struct>.<field> <offsetof>" for stm_run, stm_new_points and stm_fit, one per
// line; tests/test_fit_request_cpu.py compares them with the ctypes mirror in spamtree_amd/_lib.py.
#include "spamtree_fit.h"

#include <cstddef>
#include <cstdio>

#define SIZE(S) std::printf(#S " %zu\n", sizeof(S))
#define FIELD(S, f) std::printf(#S "." #f " %zu\n", offsetof(S, f))

int main() {
  SIZE(stm_run);
  FIELD(stm_run, pb); FIELD(stm_run, opt); FIELD(stm_run, set_unif_bounds); FIELD(stm_run, theta); FIELD(stm_run, ntheta);
  FIELD(stm_run, beta); FIELD(stm_run, tausq); FIELD(stm_run, mcmcsd); FIELD(stm_run, mcmc_keep); FIELD(stm_run, mcmc_burn);
  FIELD(stm_run, mcmc_thin); FIELD(stm_run, seed); FIELD(stm_run, flags); FIELD(stm_run, w_mcmc); FIELD(stm_run, yhat_mcmc);
  FIELD(stm_run, beta_mcmc); FIELD(stm_run, tausq_mcmc); FIELD(stm_run, theta_mcmc); FIELD(stm_run, paramsd); FIELD(stm_run, mcmc_time);
  SIZE(stm_new_points);
  FIELD(stm_new_points, n_new); FIELD(stm_new_points, coords_new); FIELD(stm_new_points, mv_new); FIELD(stm_new_points, anchor_new);
  FIELD(stm_new_points, X_new); FIELD(stm_new_points, joint_id_new); FIELD(stm_new_points, keep_draws); FIELD(stm_new_points, quantiles);
  FIELD(stm_new_points, n_quantiles); FIELD(stm_new_points, new_w); FIELD(stm_new_points, new_cond_mean);
  FIELD(stm_new_points, new_cond_var); FIELD(stm_new_points, new_yhat); FIELD(stm_new_points, new_mean); FIELD(stm_new_points, new_var);
  FIELD(stm_new_points, new_w_mean); FIELD(stm_new_points, new_yhat_mean); FIELD(stm_new_points, new_w_q); FIELD(stm_new_points, new_yhat_q);
  FIELD(stm_new_points, new_route); FIELD(stm_new_points, new_cond_cov); FIELD(stm_new_points, new_cov);
  SIZE(stm_fit);
  FIELD(stm_fit, run); FIELD(stm_fit, pts); FIELD(stm_fit, fun); FIELD(stm_fit, scores); FIELD(stm_fit, diag); FIELD(stm_fit, exc);
  FIELD(stm_fit, rk); FIELD(stm_fit, ch); FIELD(stm_fit, criteria); FIELD(stm_fit, loo);
  return 0;
}

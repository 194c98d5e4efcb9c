// spamtree_fit.cpp -- C++ host MCMC driver above the C-ABI: the counterpart of the reference's Rcpp-exported
// `spamtree_mv_mcmc` (/root/reference/src/spamtree_fit.cpp:5-430) and of the adaptive-Metropolis helpers in
// /root/reference/src/mh_adapt.h:20-239 and mh_adapt.cpp:3-15.  Everything here is host code (no kernels): the RNG,
// the Metropolis step, the conjugate draws of tausq and beta, the bookkeeping of saved iterations.  Each hot step is
// one call into include/spamtree_hip.h.
//
// R's generator (arma::randn / R::runif / R::rgamma through Rcpp) is not available outside R; the draws come from
// Philox4x32-10 counter streams with the contract documented in include/spamtree_fit.h (same per-iteration ORDER of
// draws as the reference).
#include "spamtree_fit.h"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

// ---- Philox4x32-10 (Salmon et al. 2011) ------------------------------------------------------------------------
struct HostRng {
  uint32_t k0, k1;
  explicit HostRng(uint64_t seed) : k0((uint32_t)seed), k1((uint32_t)(seed >> 32)) {}
  void block(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out[4]) const {
    uint32_t a = k0, b = k1;
    for (int r = 0; r < 10; ++r) {
      const uint64_t p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
      const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ a, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ b;
      c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
      a += 0x9E3779B9u; b += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
  }
  static double u01(uint32_t a, uint32_t b) {
    return ((double)(((uint64_t)(a >> 5) << 26) + (uint64_t)(b >> 6)) + 0.5) * (1.0 / 9007199254740992.0);
  }
  double normal(uint64_t idx, uint32_t hi, uint32_t it, uint32_t stream) const {
    uint32_t o[4];
    block((uint32_t)idx, hi, it, stream, o);
    return std::sqrt(-2.0 * std::log(u01(o[0], o[1]))) * std::cos(6.283185307179586476925286766559 * u01(o[2], o[3]));
  }
  double uniform(uint64_t idx, uint32_t hi, uint32_t it, uint32_t stream) const {
    uint32_t o[4];
    block((uint32_t)idx, hi, it, stream, o);
    return u01(o[0], o[1]);
  }
  // Marsaglia & Tsang (2000), shape >= 1; attempt t uses counters 2t (normal) and 2t+1 (uniform) of stream 3
  double gamma(uint32_t it, uint32_t j, double shape, double scale) const {
    const double d = shape - 1.0 / 3.0, c = 1.0 / std::sqrt(9.0 * d);
    for (uint64_t t = 0;; ++t) {
      const double x = normal(2 * t, j, it, 3), u = uniform(2 * t + 1, j, it, 3);
      double v = 1.0 + c * x;
      if (v <= 0.0) continue;
      v = v * v * v;
      if (std::log(u) < 0.5 * x * x + d - d * v + d * std::log(v)) return d * v * scale;
    }
  }
};

// ---- small dense helpers (column-major k x k, k <= 39) -----------------------------------------------------------
typedef std::vector<double> Mat;
bool chol_lower(const Mat &A, int n, Mat &L) {
  L.assign((size_t)n * n, 0.0);
  for (int j = 0; j < n; ++j) {
    double d = A[(size_t)j * n + j];
    for (int k = 0; k < j; ++k) d -= L[(size_t)k * n + j] * L[(size_t)k * n + j];
    if (!(d > 0.0)) return false;
    d = std::sqrt(d);
    L[(size_t)j * n + j] = d;
    for (int i = j + 1; i < n; ++i) {
      double s = A[(size_t)j * n + i];
      for (int k = 0; k < j; ++k) s -= L[(size_t)k * n + i] * L[(size_t)k * n + j];
      L[(size_t)j * n + i] = s / d;
    }
  }
  return true;
}
Mat inv_lower(const Mat &L, int n) {
  Mat X((size_t)n * n, 0.0);
  for (int j = 0; j < n; ++j)
    for (int i = j; i < n; ++i) {
      double s = (i == j) ? 1.0 : 0.0;
      for (int k = j; k < i; ++k) s -= L[(size_t)k * n + i] * X[(size_t)j * n + k];
      X[(size_t)j * n + i] = s / L[(size_t)i * n + i];
    }
  return X;
}

inline double logit(double x, double l, double u) { return -std::log((u - l) / (x - l) - 1.0); }
inline double logistic(double x, double l, double u) { return l + (u - l) / (1.0 + std::exp(-x)); }

// ---- RAMAdapt (mh_adapt.h:40-135; the member g0 = 50 shadows the file-level 500) -------------------------------
struct RAMAdapt {
  int p = 0, g0 = 50, c = 0;
  double alpha_star = 0.234, gamma = 0.5 + 1e-6;
  Mat S, paramsd, prodparam;
  bool started = false, flag_accepted = false;
  double propos_count = 0, accept_count = 0, accept_ratio = 0;
  std::vector<double> history = std::vector<double>(200, 0.0);
  bool init(int npars, const double *sd) {
    p = npars;
    S.assign(sd, sd + (size_t)p * p);
    if (!chol_lower(S, p, paramsd)) return false;
    prodparam = paramsd;
    for (auto &v : prodparam) v /= (g0 + 1.0);
    return true;
  }
  void count_proposal() { propos_count += 1; c += 1; flag_accepted = false; }
  void count_accepted() { accept_count += 1; history[c % 200] = 1; flag_accepted = true; }
  void update_ratios() { accept_ratio = accept_count / propos_count; if (!flag_accepted) history[c % 200] = 0; }
  void adapt(const std::vector<double> &U, double alpha, int mc) {
    if (mc < g0) {
      for (int j = 0; j < p; ++j)
        for (int i = 0; i < p; ++i) prodparam[(size_t)j * p + i] += U[i] * U[j] / (mc + 1.0);
      return;
    }
    if (!started) { paramsd = prodparam; started = true; }
    const double eta = std::min(1.0, p * std::pow(mc - g0 + 1.0, -gamma));
    alpha = std::isnan(alpha) ? 1.0 : std::min(1.0, alpha);   // std::min(1.0, NaN) == 1.0 in the reference
    double uu = 0;
    for (int i = 0; i < p; ++i) uu += U[i] * U[i];
    Mat Sigma((size_t)p * p, 0.0), T((size_t)p * p, 0.0);
    for (int j = 0; j < p; ++j)
      for (int i = 0; i < p; ++i) Sigma[(size_t)j * p + i] = (i == j ? 1.0 : 0.0) + eta * (alpha - alpha_star) * U[i] * U[j] / uu;
    for (int j = 0; j < p; ++j)          // T = paramsd * Sigma
      for (int i = 0; i < p; ++i) {
        double s = 0;
        for (int k = 0; k < p; ++k) s += paramsd[(size_t)k * p + i] * Sigma[(size_t)j * p + k];
        T[(size_t)j * p + i] = s;
      }
    for (int j = 0; j < p; ++j)          // S = T * paramsd'
      for (int i = 0; i < p; ++i) {
        double s = 0;
        for (int k = 0; k < p; ++k) s += T[(size_t)k * p + i] * paramsd[(size_t)k * p + j];
        S[(size_t)j * p + i] = s;
      }
    Mat L;
    if (chol_lower(S, p, L)) paramsd = L;   // arma::chol throws otherwise; the reference would abort the chain
  }
};

}  // namespace

struct stm_chain_s {
  st_handle h = nullptr;
  std::string err;
  int q = 1, p = 1, k = 0;
  long long n_all = 0;
  uint64_t seed = 0;
  HostRng rng{0};
  RAMAdapt am;
  std::vector<double> bounds;         // k x 2 column-major
  std::vector<double> param, theta_alt, Bcoeff, tausq_inv, xtx, Vi, Vim;
  std::vector<long long> n_obs_q;
  double loglik[2] = {0, 0}, current_loglik = 0;
  int adapting = 1, sample_beta = 1, sample_tausq = 1, sample_theta = 1, sample_w = 1;
  long long m = 0;
  int last_accepted = 0, last_acceptable = 1;
  bool tb_drawn = false;   // this iteration's tausq / beta were drawn under the proposal's factorisation already
  bool defer_sync = true, early_beta = true;   // SPAMTREE_DEFER_SYNC / SPAMTREE_EARLY_BETA, read by stm_create
  double last_logaccept = 0;
  bool initialised = false;
  std::vector<double> beta0, mcmcsd0;   // the caller's beta, tausq and mcmcsd: what stm_restart starts the next chain from
  double tausq0 = 1.0;
};

extern "C" const char *stm_last_error(stm_chain c) { return c ? c->err.c_str() : "null chain"; }

extern "C" int stm_destroy(stm_chain c) {
  if (!c) return 0;
  if (c->h) st_destroy(c->h);
  delete c;
  return 0;
}
extern "C" st_handle stm_handle(stm_chain c) { return c ? c->h : nullptr; }

// SpamTreeMV construction + the two initial factorisations of spamtree_fit.cpp:93-120, RAMAdapt of :151
extern "C" int stm_create(const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *mcmcsd,
                          const double *theta, int ntheta, const double *beta, double tausq, uint64_t seed, const stm_flags *flags,
                          stm_chain *out) {
  if (!pb || !out || !theta || !beta || !set_unif_bounds || !mcmcsd) return ST_ERR_USAGE;
  *out = nullptr;
  stm_chain c = new stm_chain_s();
  int rc = st_create(pb, opt, &c->h);
  if (rc != 0) { delete c; return rc; }
  const char *e;
  c->defer_sync = !((e = getenv("SPAMTREE_DEFER_SYNC")) && e[0] == '0');
  c->early_beta = !((e = getenv("SPAMTREE_EARLY_BETA")) && e[0] == '0');
  c->q = pb->q; c->p = pb->p; c->k = ntheta; c->n_all = pb->n_all; c->seed = seed; c->rng = HostRng(seed);
  if (flags) { c->adapting = flags->adapting; c->sample_beta = flags->sample_beta; c->sample_tausq = flags->sample_tausq;
               c->sample_theta = flags->sample_theta; c->sample_w = flags->sample_w; }
  c->bounds.assign(set_unif_bounds, set_unif_bounds + (size_t)ntheta * 2);
  c->beta0.assign(beta, beta + c->p); c->tausq0 = tausq; c->mcmcsd0.assign(mcmcsd, mcmcsd + (size_t)ntheta * ntheta);
  c->param.assign(theta, theta + ntheta);
  c->Bcoeff.assign((size_t)c->p * c->q, 0.0);
  for (int j = 0; j < c->q; ++j) for (int i = 0; i < c->p; ++i) c->Bcoeff[(size_t)j * c->p + i] = beta[i];   // :124-129
  c->tausq_inv.assign(c->q, 1.0 / tausq);
  c->xtx.assign((size_t)c->p * c->p * c->q, 0.0);
  c->Vi.assign((size_t)c->p * c->p, 0.0);
  for (int i = 0; i < c->p; ++i) c->Vi[(size_t)i * c->p + i] = 0.01;                                           // :157-159
  c->Vim.assign(c->p, 0.0);
  c->n_obs_q.assign(c->q, 0);
  auto fail = [&](int code, const std::string &msg) { c->err = msg; *out = c; return code; };
  *out = c;
  if ((rc = st_set_beta(c->h, c->Bcoeff.data())) != 0) return fail(rc, st_last_error(c->h));
  if ((rc = st_set_tausq_inv(c->h, c->tausq_inv.data())) != 0) return fail(rc, st_last_error(c->h));
  if ((rc = st_xtx(c->h, c->xtx.data())) != 0) return fail(rc, st_last_error(c->h));
  std::vector<double> ssq(c->q);
  std::vector<int64_t> nq(c->q);
  if ((rc = st_tausq_stats(c->h, ssq.data(), nq.data())) != 0) return fail(rc, st_last_error(c->h));
  for (int j = 0; j < c->q; ++j) c->n_obs_q[j] = nq[j];
  c->theta_alt = c->param;
  if (!c->am.init(ntheta, mcmcsd)) return fail(ST_ERR_USAGE, "mcmcsd is not positive definite");
  return ST_OK;
}

// w starts at zero (start_w is ignored, :95); both cache slots are factorised at the starting theta (:110-111).
// Separate from stm_create so that a multi-GPU caller can attach the communicator (st_comm_init on stm_handle) first.
extern "C" int stm_init(stm_chain c) {
  if (!c || !c->h) return ST_ERR_USAGE;
  if (c->initialised) return ST_OK;
  for (int slot = 0; slot < 2; ++slot) {
    const int rc = st_factor(c->h, slot, c->param.data(), c->k, &c->loglik[slot]);
    if (rc < 0) { c->err = st_last_error(c->h); return rc; }
    if (rc > 0) { c->err = "starting theta is not positive definite"; return ST_ERR_USAGE; }
  }
  c->current_loglik = c->loglik[0];
  c->initialised = true;
  return ST_OK;
}

// The next chain of stm_mcmc_chains on the same handle, from scratch as stm_create + stm_init start one: w = 0, the caller's beta
// and tausq, theta, the RAM adaptation restarted from mcmcsd, the host streams of `seed`, the iteration counter at 0, then both
// slots factorised at theta (st_factor on slot 0 voids the handle's theta-only caches).  The tree, the point set, the stores and
// every running sum of the summaries stay as they are.
static int stm_restart(stm_chain c, const double *theta, uint64_t seed) {
  int rc;
  c->seed = seed; c->rng = HostRng(seed);
  c->param.assign(theta, theta + c->k);
  c->theta_alt = c->param;
  for (int j = 0; j < c->q; ++j) for (int i = 0; i < c->p; ++i) c->Bcoeff[(size_t)j * c->p + i] = c->beta0[i];
  c->tausq_inv.assign(c->q, 1.0 / c->tausq0);
  c->am = RAMAdapt();
  if (!c->am.init(c->k, c->mcmcsd0.data())) { c->err = "mcmcsd is not positive definite"; return ST_ERR_USAGE; }
  c->m = 0; c->tb_drawn = false;
  c->last_accepted = 0; c->last_acceptable = 1; c->last_logaccept = 0;
  c->loglik[0] = c->loglik[1] = c->current_loglik = 0;
  const std::vector<double> w0((size_t)c->n_all, 0.0);
  if ((rc = st_set_w(c->h, w0.data())) != 0 || (rc = st_set_beta(c->h, c->Bcoeff.data())) != 0 ||
      (rc = st_set_tausq_inv(c->h, c->tausq_inv.data())) != 0) { c->err = st_last_error(c->h); return rc; }
  c->initialised = false;
  return stm_init(c);
}

// spamtree_fit.cpp:183-289 : w sweep, its log-density, Metropolis step for theta
static int draw_tausq_beta(stm_chain c);
// early_ok: nothing that changes w (a prediction on a saved iteration: :300-306) will run between this step and the tausq / beta draws
static int step_w_theta(stm_chain c, bool early_ok = true) {
  const uint32_t m = (uint32_t)c->m;
  int rc;
  const int k = c->k;
  RAMAdapt &am = c->am;
  std::vector<double> U(k), np(k);
  if (c->sample_theta) {
    // The proposal (:211-229) needs only theta, the adaptation state and its own normals (counter-based streams: drawing
    // them before the sweep's changes no value) -- so the factorisation of the latency-bound top levels for it can start
    // now and run under the sweep (st_factor_begin; results identical)
    am.count_proposal();
    for (int i = 0; i < k; ++i) U[i] = c->rng.normal(i, 0, m, 1);
    for (int j = 0; j < k; ++j) {                       // par_huvtransf_back(par_huvtransf_fwd(param) + paramsd * U)
      double f = logit(c->param[j], c->bounds[j], c->bounds[k + j]);
      for (int i = 0; i < k; ++i) f += am.paramsd[(size_t)i * k + j] * U[i];
      np[j] = logistic(f, c->bounds[j], c->bounds[k + j]);
    }
    for (int j = 0; j < k; ++j) {                       // unif_bounds (mh_adapt.h:188-202)
      if (np[j] < c->bounds[j]) np[j] = c->bounds[j] + 1e-10;
      if (np[j] > c->bounds[k + j]) np[j] = c->bounds[k + j] - 1e-10;
    }
    if (c->sample_w) {
      rc = st_factor_begin(c->h, 1, np.data(), k);
      if (rc < 0) { c->err = st_last_error(c->h); return rc; }
    }
  }
  // deal_with_w + get_loglik_w (:182-185).  The sweep's log-density is first read in the Metropolis step below: when a
  // proposal follows, sweep and phase C are only ENQUEUED here and their results come along with the synchronisation at the end
  // of the proposal's factorisation (one host round trip and one idle gap of the GPU less per iteration)
  bool sweep_open = false;
  auto finish_sweep = [&]() -> int {
    const int r2 = st_sample_w_loglik_end(c->h, &c->loglik[0]);
    if (r2 > 0) { c->err = "Error at gibbs_sample_w"; return r2; }
    if (r2 < 0) { c->err = st_last_error(c->h); return r2; }
    c->current_loglik = c->loglik[0];
    return 0;
  };
  if (c->sample_w) {
    rc = st_sample_w_loglik_begin(c->h, nullptr, c->seed, m, 0);
    if (rc) { c->err = st_last_error(c->h); return rc; }
    if ((!c->sample_theta || !c->defer_sync) && (rc = finish_sweep()) != 0) return rc;   // SPAMTREE_DEFER_SYNC=0: read the sweep's results at once
    sweep_open = c->sample_theta && c->defer_sync;
  }
  if (c->sample_theta) {
    c->theta_alt = np;
    double new_ll = c->loglik[1];
    // The tausq / beta draws of this iteration (:308-330) need the sweep's statistics only -- not the Metropolis outcome -- and
    // their streams are counter-based: they are made HERE, while the GPU factorises the proposal (the statistics ran on the
    // second stream at its start), and their uploads and the XB update queue behind phase A.  After the Metropolis step the
    // next sweep can be enqueued at once; before, two more host round trips (statistics -> draw -> upload, twice) stood between
    // the end of phase A and the next kernel: ~50 us of idle GPU per iteration (SPAMTREE_EARLY_BETA=0: the old order; same chain).
    // Not on iterations whose prediction step runs in between: with quirk Q3 the beta statistics pair y with w of ALL rows
    // (spamtree_model.cpp:1375), i.e. they see the predicted values.
    if (c->early_beta && early_ok && c->sample_w && st_factor_is_async(c->h)) {
      rc = st_factor_enqueue(c->h, 1, np.data(), k);
      if (rc == 0) {
        const int r3 = draw_tausq_beta(c);
        c->tb_drawn = true;
        rc = st_factor_finish(c->h, &new_ll);
        if (r3) return r3;
      }
    } else
    rc = st_factor(c->h, 1, np.data(), k, &new_ll);
    if (sweep_open) {
      const int r2 = finish_sweep();   // (a failed sweep outranks whatever the factorisation of the proposal made of its w)
      if (r2) return r2;
    }
    if (rc < 0) { c->err = st_last_error(c->h); return rc; }
    const bool acceptable = rc == 0;
    if (acceptable) c->loglik[1] = new_ll;
    c->current_loglik = c->loglik[0];
    if (std::isnan(c->current_loglik)) { c->err = "At nan loglik: error."; return STM_ERR_NAN; }   // throw 1 (:234-237)
    double jac = 0;                                      // calc_jacobian (mh_adapt.h:210-239)
    for (int j = 0; j < k; ++j) {
      const double l = c->bounds[j], u = c->bounds[k + j];
      jac += (-std::log(u - c->param[j]) - std::log(c->param[j] - l)) - (-std::log(u - np[j]) - std::log(np[j] - l));
    }
    const double logaccept = c->loglik[1] - c->current_loglik + jac;
    double acceptj = 1.0;                                // do_I_accept (mh_adapt.h:20-36); the uniform is always drawn
    if (!std::isfinite(logaccept)) acceptj = 0.0;
    else if (logaccept < 0) acceptj = std::exp(logaccept);
    const double u = c->rng.uniform(0, 0, m, 2);
    const bool accepted = (u < acceptj) && acceptable;
    if (accepted) {
      // accept_make_change first: it finishes the proposal's leaf panels (a launch, which can fail) -- an error leaves the
      // chain's own state as it was before the step's Metropolis outcome
      if ((rc = st_swap(c->h)) != 0) { c->err = st_last_error(c->h); return rc; }
      am.count_accepted();
      c->current_loglik = c->loglik[1];
      std::swap(c->loglik[0], c->loglik[1]);
      std::swap(c->param, c->theta_alt);
    }
    am.update_ratios();
    if (c->adapting) am.adapt(U, (acceptable ? 1.0 : 0.0) * std::exp(logaccept), (int)c->m);
    c->last_accepted = accepted; c->last_acceptable = acceptable; c->last_logaccept = logaccept;
  }
  return ST_OK;
}

// spamtree_fit.cpp:308-330 with the host parts of gibbs_sample_tausq (:1393-1417) and gibbs_sample_beta (:1364-1391)
static int draw_tausq_beta(stm_chain c) {
  const uint32_t m = (uint32_t)c->m;
  const int p = c->p, q = c->q;
  int rc;
  if (c->sample_tausq) {
    std::vector<double> ssq(q);
    if ((rc = st_tausq_stats(c->h, ssq.data(), nullptr)) != 0) { c->err = st_last_error(c->h); return rc; }
    for (int j = 0; j < q; ++j) {
      const double aparam = 2.01 + c->n_obs_q[j] / 2.0, bparam = 1.0 / (1.0 + 0.5 * ssq[j]);
      c->tausq_inv[j] = c->rng.gamma(m, j, aparam, bparam);
    }
    if ((rc = st_set_tausq_inv(c->h, c->tausq_inv.data())) != 0) { c->err = st_last_error(c->h); return rc; }
  }
  if (c->sample_beta) {
    std::vector<double> xty((size_t)p * q);
    if ((rc = st_beta_stats(c->h, xty.data())) != 0) { c->err = st_last_error(c->h); return rc; }
    for (int j = 0; j < q; ++j) {
      Mat Si((size_t)p * p), L;
      for (int i = 0; i < p * p; ++i) Si[i] = c->tausq_inv[j] * c->xtx[(size_t)j * p * p + i] + c->Vi[i];
      if (!chol_lower(Si, p, L)) { c->err = "beta posterior precision is not positive definite"; return ST_ERR_USAGE; }
      const Mat Sc = inv_lower(L, p);
      std::vector<double> b(p), t(p, 0.0), zn(p);
      for (int i = 0; i < p; ++i) { b[i] = c->Vim[i] + c->tausq_inv[j] * xty[(size_t)j * p + i]; zn[i] = c->rng.normal(i, j, m, 4); }
      for (int i = 0; i < p; ++i) { double s = 0; for (int kk = 0; kk <= i; ++kk) s += Sc[(size_t)kk * p + i] * b[kk]; t[i] = s + zn[i]; }
      for (int i = 0; i < p; ++i) {                      // Sc' (Sc b) + Sc' z  =  Sc' (Sc b + z)
        double s = 0;
        for (int kk = i; kk < p; ++kk) s += Sc[(size_t)i * p + kk] * t[kk];
        c->Bcoeff[(size_t)j * p + i] = s;
      }
    }
    if ((rc = st_set_beta(c->h, c->Bcoeff.data())) != 0) { c->err = st_last_error(c->h); return rc; }
  }
  return ST_OK;
}
static int step_tausq_beta(stm_chain c) {
  if (!c->tb_drawn) { const int rc = draw_tausq_beta(c); if (rc) return rc; }   // (else: drawn under the proposal's factorisation, step_w_theta)
  c->tb_drawn = false;
  c->m += 1;
  return ST_OK;
}

extern "C" int stm_step(stm_chain c, int n_iters) {
  if (!c || !c->h) return ST_ERR_USAGE;
  if (!c->initialised) { const int rc0 = stm_init(c); if (rc0) return rc0; }
  for (int it = 0; it < n_iters; ++it) {
    int rc = step_w_theta(c);
    if (rc) return rc;
    rc = step_tausq_beta(c);
    if (rc) return rc;
  }
  return ST_OK;
}

extern "C" int stm_state(stm_chain c, double *theta, double *Bcoeff, double *tausq_inv, double *loglik, double *accept_ratio,
                         int64_t *iteration, double *paramsd) {
  if (!c) return ST_ERR_USAGE;
  if (theta) std::memcpy(theta, c->param.data(), c->param.size() * sizeof(double));
  if (Bcoeff) std::memcpy(Bcoeff, c->Bcoeff.data(), c->Bcoeff.size() * sizeof(double));
  if (tausq_inv) std::memcpy(tausq_inv, c->tausq_inv.data(), c->tausq_inv.size() * sizeof(double));
  if (loglik) *loglik = c->current_loglik;
  if (accept_ratio) *accept_ratio = c->am.accept_ratio;
  if (iteration) *iteration = c->m;
  if (paramsd) std::memcpy(paramsd, c->am.paramsd.data(), c->am.paramsd.size() * sizeof(double));
  return ST_OK;
}

// New locations predicted during the fit (st_points_*): the point set and the summaries' reservation, before any iteration
extern "C" int stm_points_set(stm_chain c, int64_t n_new, const double *coords, const int64_t *mv, const int64_t *anchor, const double *X,
                              int64_t keep_draws) {
  if (!c || !c->h) return ST_ERR_USAGE;
  return stm_points_set_joint(c, n_new, coords, mv, anchor, X, nullptr, keep_draws);
}

extern "C" int stm_points_set_joint(stm_chain c, int64_t n_new, const double *coords, const int64_t *mv, const int64_t *anchor, const double *X,
                                    const int64_t *joint_id, int64_t keep_draws) {
  if (!c || !c->h) return ST_ERR_USAGE;
  int rc = st_points_set_joint(c->h, n_new, coords, mv, anchor, X, joint_id);
  if (rc == 0) rc = st_points_summary_reset(c->h);
  if (rc == 0) rc = st_points_summary_reserve(c->h, keep_draws);
  if (rc != 0) { c->err = st_last_error(c->h); return rc; }
  return ST_OK;
}

extern "C" int stm_points_functionals_set(stm_chain c, int64_t n_fun, const int64_t *ptr, const int64_t *idx, const double *wt) {
  if (!c || !c->h) return ST_ERR_USAGE;
  const int rc = st_points_functionals_set(c->h, n_fun, ptr, idx, wt);
  if (rc != 0) { c->err = st_last_error(c->h); return rc; }
  return ST_OK;
}

extern "C" int stm_points_score_set(stm_chain c, const double *y_new) {
  if (!c || !c->h) return ST_ERR_USAGE;
  const int rc = st_points_score_set(c->h, y_new);
  if (rc != 0) { c->err = st_last_error(c->h); return rc; }
  return ST_OK;
}

extern "C" int stm_points_mixture_reserve(stm_chain c, int64_t keep) {
  if (!c || !c->h) return ST_ERR_USAGE;
  const int rc = st_points_mixture_reserve(c->h, keep);
  if (rc != 0) { c->err = st_last_error(c->h); return rc; }
  return ST_OK;
}

extern "C" int stm_rows_score_set(stm_chain c, const double *y_holdout) {
  if (!c || !c->h) return ST_ERR_USAGE;
  const int rc = st_rows_score_set(c->h, y_holdout);
  if (rc != 0) { c->err = st_last_error(c->h); return rc; }
  return ST_OK;
}

// ---- the whole fit: one request (include/spamtree_fit.h, stm_fit) ------------------------------------------------------------------
#include "draw_store.hpp"   // any_out: what an output struct asks for
#include "fit_plan.hpp"     // FitPlan: the request as it is run, worked out without a device

namespace {
// What stm_mcmc_fit refuses before a chain exists to carry the text: the calling thread's last such refusal
thread_local std::string g_chains_error;

struct FitChain {          // one chain of a request: its saved draw s goes to column col0 + s of per-draw outputs with ncols columns
  uint64_t seed;
  int col0, ncols;
};
struct JointBlocks {       // st_points_joint_layout's groups, and the packed blocks of every draw when only new_cond_var is wanted of them
  int64_t nj = 0;
  std::vector<int64_t> off, ptr, mem;
  std::vector<double> scratch;
};
uint64_t chain_seed(const stm_fit &f, int cn) { return f.ch ? f.ch->seeds[cn] : f.run.seed; }
const double *chain_theta(const stm_fit &f, int cn) { return f.ch && f.ch->theta0 ? f.ch->theta0 + (size_t)cn * f.run.ntheta : f.run.theta; }
}  // namespace

extern "C" const char *stm_mcmc_chains_last_error(void) { return g_chains_error.c_str(); }

// The whole of spamtree_mv_mcmc (spamtree_fit.cpp:5-430) for one chain of a request, on a created chain.  Every Philox counter is the
// chain's own: the iteration m for the rows (st_yhat and st_summary_accumulate draw the same stream 5 values), the saved index for
// the points (streams 6 / 7 only), so the chain itself is the same draw for draw whatever parts the request has.
static int run_fit(stm_chain c, const FitPlan &pl, const FitChain &ch, double *seconds) {
  const stm_run &r = pl.f.run;
  const stm_new_points *pts = pl.f.pts;
  const stm_functionals *fun = pl.f.fun;
  const stm_criteria *crit = pl.f.criteria;
  int rc = 0;
  const int sample_predicts = r.flags ? r.flags->sample_predicts : 1;
  const auto t0 = std::chrono::steady_clock::now();
  const long long mcmc = (long long)r.mcmc_thin * r.mcmc_keep + r.mcmc_burn;
  std::vector<double> predict_param = c->param;
  int msaved = 0;
  const int p = c->p, q = c->q, k = c->k;
  const long long n = c->n_all;
  for (long long m = 0; m < mcmc && rc == 0; ++m) {
    const long long mx = m - r.mcmc_burn;
    const bool saving = mx >= 0 && (mx % r.mcmc_thin == 0);
    rc = step_w_theta(c, !(saving && sample_predicts && c->sample_w));
    if (rc) break;
    if (saving && sample_predicts && c->sample_w) {                    // :300-306
      int need_update = 0;
      for (int j = 0; j < k; ++j) need_update += std::fabs(c->param[j] - predict_param[j]) > 1e-05;
      rc = st_predict(c->h, need_update);
      if (rc) break;
      predict_param = c->param;
    }
    rc = step_tausq_beta(c);
    if (rc) break;
    if (saving && msaved < r.mcmc_keep) {                               // :376-389
      const size_t col_s = (size_t)ch.col0 + msaved;   // the draw's column in the per-draw outputs
      if (r.tausq_mcmc) for (int j = 0; j < q; ++j) r.tausq_mcmc[col_s * q + j] = 1.0 / c->tausq_inv[j];
      if (r.beta_mcmc) for (int j = 0; j < q; ++j) for (int i = 0; i < p; ++i)
        r.beta_mcmc[(size_t)j * p * ch.ncols + col_s * p + i] = c->Bcoeff[(size_t)j * p + i];
      if (r.theta_mcmc) std::memcpy(r.theta_mcmc + col_s * k, c->param.data(), k * sizeof(double));
      if (r.w_mcmc) rc = st_get_w(c->h, r.w_mcmc + col_s * n);
      if (!rc && r.yhat_mcmc) rc = st_yhat(c->h, nullptr, ch.seed, (uint32_t)m, r.yhat_mcmc + col_s * n);
      if (!rc && pts) {   // the saved theta's factor in slot 0, the saved w, beta and tausq
        const size_t o = col_s * pts->n_new;
        auto col = [&](double *a) { return a ? a + o : nullptr; };
        if (pts->new_cond_cov) {   // cond_var = max(diag, 0), from the packed blocks after the last chain
          rc = st_points_accumulate_joint(c->h, ch.seed, (uint32_t)msaved, col(pts->new_w), col(pts->new_cond_mean),
                                          pts->new_cond_cov + col_s * pl.cov_len, nullptr, col(pts->new_yhat));
        } else {
          rc = st_points_accumulate(c->h, ch.seed, (uint32_t)msaved, col(pts->new_w), col(pts->new_cond_mean), col(pts->new_cond_var),
                                    col(pts->new_yhat));
        }
        if (!rc && fun && (fun->fun_w || fun->fun_cond_mean || fun->fun_cond_var || fun->fun_yhat)) {
          const size_t of = col_s * fun->n_fun;
          auto fcol = [&](double *a) { return a ? a + of : nullptr; };
          rc = st_points_functionals_last(c->h, fcol(fun->fun_w), fcol(fun->fun_cond_mean), fcol(fun->fun_cond_var), fcol(fun->fun_yhat));
        }
      }
      if (!rc && crit) {         // the criteria over the fit's own rows and, when their CRPS is wanted, the iteration's yhat
        rc = st_rows_score_accumulate(c->h);
        if (!rc && crit->want_crps && crit->y_holdout) rc = st_summary_accumulate(c->h, ch.seed, (uint32_t)m);
      }
      if (!rc && pl.f.loo) rc = st_rows_loo_accumulate(c->h);   // reads w, XB, tausq_inv and slot 0, draws nothing
      if (!rc && pl.store_rows) rc = st_summary_accumulate(c->h, ch.seed, (uint32_t)m);   // the draws diag, exc and rk read
      if (rc) c->err = st_last_error(c->h);
      ++msaved;
    }
  }
  if (rc == 0) {
    if (r.paramsd) std::memcpy(r.paramsd, c->am.paramsd.data(), (size_t)k * k * sizeof(double));
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  return rc;
}

// Step 1 after the plan: the chain and what it is given before its first factorisation, so every refusal of these comes before
// stm_init.  Fills pl.cov_len and jb and points p.new_cond_cov at the scratch where only new_cond_var is wanted; no chain is left
// behind a refusal.
static int fit_setup(FitPlan &pl, JointBlocks &jb, stm_chain *out) {
  const stm_fit &f = pl.f;
  const stm_run &r = f.run;
  stm_new_points &p = pl.p;
  const stm_functionals *const fun = f.fun;
  const stm_loo *const loo = f.loo;
  stm_chain c = nullptr;
  int rc = stm_create(r.pb, r.opt, r.set_unif_bounds, r.mcmcsd, chain_theta(f, 0), r.ntheta, r.beta, r.tausq, chain_seed(f, 0), r.flags, &c);
  if (rc == 0 && f.pts)
    rc = stm_points_set_joint(c, p.n_new, p.coords_new, p.mv_new, p.anchor_new, p.X_new, p.joint_id_new, p.keep_draws);
  if (rc == 0 && (pl.store_rows || (pl.crps && r.mcmc_keep > 0))) {
    rc = st_summary_reset(c->h);
    if (rc == 0) rc = st_summary_reserve(c->h, pl.total);
  }
  if (rc == 0 && fun) rc = stm_points_functionals_set(c, fun->n_fun, fun->ptr, fun->idx, fun->wt);
  if (rc == 0 && f.scores) rc = stm_points_score_set(c, f.scores->y_new);
  if (rc == 0 && pl.rb && (rc = st_points_exceed_set(c->h, pl.rb->n_thr, pl.rb->thr, pl.rb->side, pl.rb->thr_fun)) != 0) c->err = st_last_error(c->h);
  if (rc == 0 && pl.mix) rc = stm_points_mixture_reserve(c, pl.total);
  if (rc == 0 && p.joint_id_new) {
    rc = st_points_joint_layout(c->h, &jb.nj, nullptr, nullptr, nullptr);
    jb.off.resize(jb.nj + 1); jb.ptr.resize(jb.nj + 1); jb.mem.resize(p.n_new);
    if (rc == 0) rc = st_points_joint_layout(c->h, &jb.nj, jb.off.data(), jb.ptr.data(), jb.mem.data());
    if (rc == 0 && !p.new_cond_cov && p.new_cond_var) jb.scratch.resize((size_t)jb.off[jb.nj] * std::max<long long>(pl.total, 0));
  }
  if (rc == 0 && f.criteria) rc = stm_rows_score_set(c, f.criteria->y_holdout);
  if (rc == 0 && loo) rc = st_rows_loo_set(c->h);   // (limited_tree is refused)
  if (rc == 0 && loo && loo->psis) rc = st_rows_loo_reserve(c->h, r.mcmc_keep);
  if (rc == 0 && loo && loo->groups) rc = st_rows_loo_groups_set(c->h, loo->groups->labels);   // (oversized groups, groups without an observed member)
  if (rc == 0) rc = stm_init(c);
  if (rc != 0) { stm_destroy(c); return rc; }
  if (p.joint_id_new) {
    pl.cov_len = jb.off[jb.nj];
    if (!p.new_cond_cov && !jb.scratch.empty()) p.new_cond_cov = jb.scratch.data();
  } else p.new_cond_cov = nullptr;
  *out = c;
  return ST_OK;
}

// Step 3: the read-outs after the last chain, in the order the header states
static int fit_read_out(stm_chain c, const FitPlan &pl, const JointBlocks &jb) {
  const stm_fit &f = pl.f;
  const stm_new_points &p = pl.p;
  const stm_functionals *const fun = f.fun;
  const stm_scores *const scores = f.scores;
  const stm_diagnostics *const diag = f.diag;
  const stm_excursions *const exc = f.exc;
  const stm_rank_diagnostics *const rk = f.rk;
  const stm_rb_exceed *const rb = pl.rb;
  const stm_criteria *const cr = f.criteria;
  const stm_loo *const loo = f.loo;
  const stm_loo_psis *const psis = loo ? loo->psis : nullptr;
  const stm_loo_groups *const lgo = loo ? loo->groups : nullptr;
  const Wanted &d = pl.d, &e = pl.e, &k = pl.k;
  const int M = pl.M;   // (diag and rk: the stored draws are M chains laid end to end)
  const bool have_pts = f.pts != nullptr, saved = f.run.mcmc_keep > 0;
  int rc = 0;
  if (have_pts && p.new_cond_cov && p.new_cond_var)
    for (long long s = 0; s < pl.total; ++s)
      for (int64_t g = 0; g < jb.nj; ++g) {
        const int64_t sz = jb.ptr[g + 1] - jb.ptr[g];
        for (int64_t a = 0; a < sz; ++a)
          p.new_cond_var[(size_t)s * p.n_new + jb.mem[jb.ptr[g] + a]] = std::max(p.new_cond_cov[(size_t)s * pl.cov_len + jb.off[g] + a * (sz + 1)], 0.0);
      }
  if (rc == 0 && have_pts && saved && (p.new_mean || p.new_var || p.new_w_mean || p.new_yhat_mean))
    rc = st_points_summary_get(c->h, p.new_mean, p.new_var, p.new_w_mean, p.new_yhat_mean, nullptr);
  if (rc == 0 && have_pts && saved && p.new_cov) rc = st_points_summary_get_cov(c->h, p.new_cov);
  for (int32_t i = 0; rc == 0 && have_pts && i < p.n_quantiles && (p.new_w_q || p.new_yhat_q); ++i)
    rc = st_points_summary_quantile(c->h, p.quantiles[i], p.new_w_q ? p.new_w_q + (size_t)i * p.n_new : nullptr,
                                    p.new_yhat_q ? p.new_yhat_q + (size_t)i * p.n_new : nullptr);
  if (rc == 0 && have_pts && p.new_route) rc = st_points_info(c->h, p.new_route, nullptr, nullptr, nullptr);
  if (rc == 0 && fun && saved && (fun->fun_mean || fun->fun_var || fun->fun_w_mean || fun->fun_yhat_mean))
    rc = st_points_functionals_get(c->h, fun->fun_mean, fun->fun_var, fun->fun_w_mean, fun->fun_yhat_mean, nullptr);
  for (int32_t i = 0; rc == 0 && fun && i < p.n_quantiles && (fun->fun_w_q || fun->fun_yhat_q); ++i)
    rc = st_points_functionals_quantile(c->h, p.quantiles[i], fun->fun_w_q ? fun->fun_w_q + (size_t)i * fun->n_fun : nullptr,
                                        fun->fun_yhat_q ? fun->fun_yhat_q + (size_t)i * fun->n_fun : nullptr);
  if (rc == 0 && scores && saved)
    rc = st_points_score_get(c->h, scores->lpd, scores->pit, scores->crps, scores->lpd_joint, scores->n_scored, scores->n_degenerate);
  // a yhat (rb: fun_w too) struct that asks for nothing goes as NULL: its store need not exist
  const auto opt = [](const auto &o) { return any_out(&o) ? &o : nullptr; };
  if (rc == 0 && rb && saved) rc = st_points_exceed_get(c->h, &rb->new_w, opt(rb->new_yhat), opt(rb->fun_w), rb->n_accumulated);
  if (const stm_mixture *const mix = pl.mix; mix && saved) {
    if (rc == 0 && pl.mix_q) rc = st_points_mixture_quantiles(c->h, mix->n_probs, mix->probs, opt(mix->new_w), opt(mix->new_yhat), opt(mix->fun_w));
    if (rc == 0 && pl.mix_crps) rc = st_points_mixture_crps(c->h, mix->crps, mix->spread, nullptr);
    if (rc == 0 && mix->n_stored) rc = st_points_mixture_draws(c->h, nullptr, nullptr, nullptr, nullptr, mix->n_stored);
  }
  if (rc == 0 && d.rows) rc = st_summary_chain_diagnostics(c->h, M, diag->max_lag, &diag->rows_w, &diag->rows_yhat);
  if (rc == 0 && d.pts) rc = st_points_summary_chain_diagnostics(c->h, M, diag->max_lag, &diag->new_w, opt(diag->new_yhat));
  if (rc == 0 && d.fun) rc = st_points_functionals_chain_diagnostics(c->h, M, diag->max_lag, &diag->fun_w, opt(diag->fun_yhat));
  if (rc == 0 && e.rows) rc = st_summary_excursions(c->h, &exc->rows_spec, &exc->rows_w, &exc->rows_yhat);
  if (rc == 0 && e.pts) rc = st_points_summary_excursions(c->h, &exc->new_spec, &exc->new_w, opt(exc->new_yhat));
  if (rc == 0 && e.fun) rc = st_points_functionals_excursions(c->h, &exc->fun_spec, &exc->fun_w, opt(exc->fun_yhat));
  if (rc == 0 && k.rows) rc = st_summary_chain_rank_diagnostics(c->h, M, &rk->rows_spec, &rk->rows_w, &rk->rows_yhat);
  if (rc == 0 && k.pts) rc = st_points_summary_chain_rank_diagnostics(c->h, M, &rk->new_spec, &rk->new_w, opt(rk->new_yhat));
  if (rc == 0 && k.fun) rc = st_points_functionals_chain_rank_diagnostics(c->h, M, &rk->fun_spec, &rk->fun_w, opt(rk->fun_yhat));
  if (rc == 0 && cr && saved) {
    rc = st_rows_score_get(c->h, cr->lppd, cr->p_waic, cr->mean_ll, cr->mu_mean, cr->pit, cr->crps, cr->n_accumulated);
    if (rc == 0) rc = st_rows_score_totals(c->h, cr->obs, cr->held, cr->n_obs, cr->n_held);
  }
  if (rc == 0 && loo && saved) {
    rc = st_rows_loo_get(c->h, loo->elpd_loo, loo->pit_loo, loo->mu_loo, loo->weight_ess, loo->n_accumulated, loo->n_skipped);
    if (rc == 0) rc = st_rows_loo_totals(c->h, loo->tot, loo->n_obs);
  }
  if (rc == 0 && psis && saved) {
    rc = st_rows_loo_psis(c->h, &psis->out);
    if (rc == 0) rc = st_rows_loo_psis_totals(c->h, psis->tot, psis->n_obs);
    if (rc == 0 && (psis->t || psis->phi || psis->mu)) rc = st_rows_loo_draws(c->h, psis->t, psis->phi, psis->mu);
  }
  if (rc == 0 && lgo) {
    rc = st_rows_loo_groups_count(c->h, lgo->n_groups, lgo->n_members, lgo->n_pairs, nullptr);
    if (rc == 0) rc = st_rows_loo_groups_index(c->h, lgo->label, lgo->ptr, lgo->rows);
  }
  if (rc == 0 && lgo && saved) {
    rc = st_rows_loo_groups_get(c->h, lgo->elpd_lgo, lgo->weight_ess, lgo->n_skipped, lgo->mu_lgo, lgo->pit_lgo, nullptr);
    if (rc == 0) rc = st_rows_loo_groups_totals(c->h, lgo->tot, lgo->by_outcome);
    if (rc == 0 && psis) rc = st_rows_loo_groups_psis(c->h, lgo->khat, lgo->elpd_psis, lgo->weight_ess_psis, nullptr, nullptr);
  }
  return rc;
}

// The request in four steps: the plan (fit_plan.cpp: every refusal that needs no device), the setup, chain after chain, the read-outs
extern "C" int stm_mcmc_fit(const stm_fit *fit) { return stm_fit_run(fit, nullptr); }

extern "C" int stm_fit_run(const stm_fit *fit, const stm_fit_more *more) {
  g_chains_error.clear();
  if (!fit) return ST_ERR_USAGE;
  FitPlan pl;
  JointBlocks jb;
  stm_chain c = nullptr;
  std::string which;   // the failing check of every refusal: the plan's own tests read it, no caller does
  int rc = fit_plan(*fit, pl, g_chains_error, which, more);
  if (rc == 0) rc = fit_setup(pl, jb, &c);
  if (rc != 0) return rc;
  const stm_run &r = pl.f.run;
  const stm_chains *const ch = pl.f.ch;
  const size_t kk = (size_t)r.ntheta * r.ntheta;
  // M chains one after another on one handle; chain cn's saved draws are columns cn keep .. (cn + 1) keep - 1 of every per-draw
  // output and of the stores
  double time_all = 0;
  for (int cn = 0; cn < pl.M && rc == 0; ++cn) {
    if (cn > 0) rc = stm_restart(c, chain_theta(pl.f, cn), chain_seed(pl.f, cn));
    double time_c = 0;
    if (rc == 0) rc = run_fit(c, pl, FitChain{chain_seed(pl.f, cn), cn * r.mcmc_keep, (int)pl.total}, &time_c);
    if (rc == 0 && ch && ch->paramsd) std::memcpy(ch->paramsd + cn * kk, c->am.paramsd.data(), kk * sizeof(double));
    if (rc == 0 && ch && ch->chain_time) ch->chain_time[cn] = time_c;
    time_all += time_c;
  }
  if (rc == 0 && r.mcmc_time) *r.mcmc_time = time_all;   // (paramsd: the last chain's; every chain's in ch->paramsd)
  if (rc == 0) rc = fit_read_out(c, pl, jb);
  stm_destroy(c);
  return rc;
}


// ---- the positional entry points: each fills a request from its arguments and calls stm_mcmc_fit -------------------------------
// The two argument lists every one of them repeats, once: the run's twenty and the point set's twenty-two, in the structs' order
#define STM_RUN_ARGS                                                                                                                    \
  const st_problem *pb, const st_options *opt, const double *set_unif_bounds, const double *theta, int ntheta, const double *beta,     \
      double tausq, const double *mcmcsd, int mcmc_keep, int mcmc_burn, int mcmc_thin, uint64_t seed, const stm_flags *flags,          \
      double *w_mcmc, double *yhat_mcmc, double *beta_mcmc, double *tausq_mcmc, double *theta_mcmc, double *paramsd, double *mcmc_time
#define STM_RUN                                                                                                                         \
  { pb, opt, set_unif_bounds, theta, ntheta, beta, tausq, mcmcsd, mcmc_keep, mcmc_burn, mcmc_thin, seed, flags, w_mcmc, yhat_mcmc,      \
    beta_mcmc, tausq_mcmc, theta_mcmc, paramsd, mcmc_time }
#define STM_POINTS_ARGS                                                                                                                 \
  int64_t n_new, const double *coords_new, const int64_t *mv_new, const int64_t *anchor_new, const double *X_new,                      \
      const int64_t *joint_id_new, int64_t keep_draws, const double *quantiles, int32_t n_quantiles, double *new_w,                    \
      double *new_cond_mean, double *new_cond_var, double *new_yhat, double *new_mean, double *new_var, double *new_w_mean,             \
      double *new_yhat_mean, double *new_w_q, double *new_yhat_q, int32_t *new_route, double *new_cond_cov, double *new_cov
#define STM_POINTS                                                                                                                      \
  const stm_new_points pts {                                                                                                            \
    n_new, coords_new, mv_new, anchor_new, X_new, joint_id_new, keep_draws, quantiles, n_quantiles, new_w, new_cond_mean, new_cond_var, \
        new_yhat, new_mean, new_var, new_w_mean, new_yhat_mean, new_w_q, new_yhat_q, new_route, new_cond_cov, new_cov                   \
  }

extern "C" int spamtree_mv_mcmc_c(STM_RUN_ARGS) {
  const stm_fit f{STM_RUN};
  return stm_mcmc_fit(&f);
}
extern "C" int stm_mcmc_points(STM_RUN_ARGS, int64_t n_new, const double *coords_new, const int64_t *mv_new, const int64_t *anchor_new,
                               const double *X_new, int64_t keep_draws, const double *quantiles, int32_t n_quantiles, double *new_w,
                               double *new_cond_mean, double *new_cond_var, double *new_yhat, double *new_mean, double *new_var,
                               double *new_w_mean, double *new_yhat_mean, double *new_w_q, double *new_yhat_q, int32_t *new_route) {
  const int64_t *const joint_id_new = nullptr;
  double *const new_cond_cov = nullptr, *const new_cov = nullptr;
  STM_POINTS;
  const stm_fit f{STM_RUN, &pts};
  return stm_mcmc_fit(&f);
}
extern "C" int stm_mcmc_points_joint(STM_RUN_ARGS, STM_POINTS_ARGS) {
  STM_POINTS;
  const stm_fit f{STM_RUN, &pts};
  return stm_mcmc_fit(&f);
}
extern "C" int stm_mcmc_functionals(STM_RUN_ARGS, STM_POINTS_ARGS, const stm_functionals *fun) {
  STM_POINTS;
  const stm_fit f{STM_RUN, &pts, fun};
  return stm_mcmc_fit(&f);
}
extern "C" int stm_mcmc_scored(STM_RUN_ARGS, STM_POINTS_ARGS, const stm_functionals *fun, const stm_scores *scores) {
  STM_POINTS;
  const stm_fit f{STM_RUN, &pts, fun, scores};
  return stm_mcmc_fit(&f);
}
extern "C" int stm_mcmc_diagnosed(STM_RUN_ARGS, STM_POINTS_ARGS, const stm_functionals *fun, const stm_scores *scores,
                                  const stm_diagnostics *diag) {
  STM_POINTS;
  const stm_fit f{STM_RUN, &pts, fun, scores, diag};
  return stm_mcmc_fit(&f);
}
extern "C" int stm_mcmc_excursions(STM_RUN_ARGS, STM_POINTS_ARGS, const stm_functionals *fun, const stm_scores *scores,
                                   const stm_diagnostics *diag, const stm_excursions *exc) {
  STM_POINTS;
  const stm_fit f{STM_RUN, &pts, fun, scores, diag, exc};
  return stm_mcmc_fit(&f);
}
extern "C" int stm_mcmc_ranked(STM_RUN_ARGS, STM_POINTS_ARGS, const stm_functionals *fun, const stm_scores *scores,
                               const stm_diagnostics *diag, const stm_excursions *exc, const stm_rank_diagnostics *rk) {
  STM_POINTS;
  const stm_fit f{STM_RUN, &pts, fun, scores, diag, exc, rk};
  return stm_mcmc_fit(&f);
}
extern "C" int stm_mcmc_chains(STM_RUN_ARGS, STM_POINTS_ARGS, const stm_functionals *fun, const stm_scores *scores,
                               const stm_diagnostics *diag, const stm_excursions *exc, const stm_rank_diagnostics *rk,
                               const stm_chains *ch) {
  STM_POINTS;
  const stm_fit f{STM_RUN, &pts, fun, scores, diag, exc, rk, ch};
  return stm_mcmc_fit(&f);
}
extern "C" int stm_mcmc_criteria(STM_RUN_ARGS, const stm_criteria *criteria) {
  stm_fit f{STM_RUN};
  f.criteria = criteria;
  return stm_mcmc_fit(&f);
}
extern "C" int stm_mcmc_loo(STM_RUN_ARGS, const stm_criteria *criteria, const stm_loo *loo) {
  stm_fit f{STM_RUN};
  f.criteria = criteria;
  f.loo = loo;
  return stm_mcmc_fit(&f);
}

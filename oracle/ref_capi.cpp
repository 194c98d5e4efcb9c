// C entry points over the reference's own covariance_functions.cpp, mh_adapt.{h,cpp}, list_mean.cpp and find_nan.cpp, which
// oracle/Makefile compiles unchanged from the reference tree against oracle/refshim/RcppArmadillo.h into
// _ref/libspamtree_ref.so.  Test infrastructure only: oracle/reflib.py loads it, tests/test_reference_binary.py compares the
// restatements (oracle/, spamtree_amd/mcmc.py) with it, tests/golden/make_reference_golden.py records fixtures from it.
// This file includes the reference's headers by name at build time; it holds none of their text.
//
// All arrays are flat and column-major.  Index arrays are 0-based int64 unless stated.  Every function that can throw
// returns 0 on success and a negative code otherwise (-1: the reference threw or stopped, -2: the uniform queue was empty).
#include <cstdint>
#include <deque>

#include "covariance_functions.h"
#include "find_nan.h"
#include "mh_adapt.h"

arma::mat list_mean(const arma::field<arma::mat>& x);                       // list_mean.cpp declares these in no header
arma::mat list_qtile(const arma::field<arma::mat>& x, double q);

// ---- R::runif: the Metropolis uniform comes from a queue the caller fills -------------------------------------------------
static std::deque<double> g_uniforms;
struct EmptyUniformQueue {};

namespace R {
double runif(double, double) {
  if (g_uniforms.empty()) throw EmptyUniformQueue();
  const double u = g_uniforms.front();
  g_uniforms.pop_front();
  return u;
}
}  // namespace R

namespace {

arma::mat to_mat(const double* p, int r, int c) {
  arma::mat m(r, c);
  std::copy(p, p + (size_t)r * c, m.memptr());
  return m;
}
arma::vec to_vec(const double* p, int n) { return arma::vec(to_mat(p, n, 1)); }
arma::uvec to_uvec(const int64_t* p, int n) {
  arma::uvec u(n);
  for (int i = 0; i < n; i++) u(i) = (arma::uword)p[i];
  return u;
}
void put(const arma::mat& m, double* out) { std::copy(m.begin(), m.end(), out); }

template <class F>
int guarded(F f) {
  try {
    f();
    return 0;
  } catch (const EmptyUniformQueue&) {
    return -2;
  } catch (...) {
    return -1;
  }
}

}  // namespace

extern "C" {

// ---- covariance -------------------------------------------------------------------------------------------------------------
// CovarianceParams(dd = 2, q, -1).transform(theta) read back.  dims = {covariance_model, npars, n_cbase, Dmat.n_rows}; Dmat
// must hold max(1, q * q) doubles.
int ref_transform(int q, const double* theta, int ntheta, double* ai1, double* ai2, double* phi_i, double* thetamv,
                  double* Dmat, int* dims) {
  return guarded([&] {
    CovarianceParams cp(2, q, -1);
    cp.transform(to_vec(theta, ntheta));
    dims[0] = cp.covariance_model;
    dims[1] = cp.npars;
    dims[2] = cp.n_cbase;
    dims[3] = (int)cp.Dmat.n_rows;
    put(cp.ai1, ai1);
    put(cp.ai2, ai2);
    put(cp.phi_i, phi_i);
    put(cp.thetamv, thetamv);
    put(cp.Dmat, Dmat);
  });
}

int ref_vec_to_symmat(const double* x, int k, double* out, int* p) {
  return guarded([&] {
    arma::mat m = vec_to_symmat(to_vec(x, k));
    *p = (int)m.n_rows;
    put(m, out);
  });
}

// Covariancef (which = 0) or mvCovAG20107 (which = 1) of rows ind1 x ind2 of coords (n x 2), qv the 0-based outcome of each row.
int ref_covariancef(int which, int q, const double* theta, int ntheta, const double* coords, int n, const int64_t* qv,
                    const int64_t* ind1, int n1, const int64_t* ind2, int n2, int same, double* out) {
  return guarded([&] {
    CovarianceParams cp(2, q, -1);
    cp.transform(to_vec(theta, ntheta));
    arma::mat cx = to_mat(coords, n, 2);
    arma::uvec v = to_uvec(qv, n), i1 = to_uvec(ind1, n1), i2 = to_uvec(ind2, n2);
    put(which == 0 ? Covariancef(cx, v, i1, i2, cp, same != 0) : mvCovAG20107(cx, v, i1, i2, cp, same != 0), out);
  });
}

// CrossCovarianceAG10 as exported to R: mv1, mv2 are 1-based; Dmat is pd x pd, thetamv has ncb entries.
int ref_cross_covariance_ag10(const double* coords1, int n1, const int64_t* mv1, const double* coords2, int n2,
                              const int64_t* mv2, const double* ai1, const double* ai2, const double* phi_i, int q,
                              const double* thetamv, int ncb, const double* Dmat, int pd, double* out) {
  return guarded([&] {
    put(CrossCovarianceAG10(to_mat(coords1, n1, 2), to_uvec(mv1, n1), to_mat(coords2, n2, 2), to_uvec(mv2, n2),
                            to_vec(ai1, q), to_vec(ai2, q), to_vec(phi_i, q), to_vec(thetamv, ncb), to_mat(Dmat, pd, pd)),
        out);
  });
}

// ---- Metropolis helpers -----------------------------------------------------------------------------------------------------
int ref_par_huvtransf_fwd(const double* par, int n, const double* bounds, double* out) {
  return guarded([&] { put(par_huvtransf_fwd(to_vec(par, n), to_mat(bounds, n, 2)), out); });
}
int ref_par_huvtransf_back(const double* par, int n, const double* bounds, double* out) {
  return guarded([&] { put(par_huvtransf_back(to_vec(par, n), to_mat(bounds, n, 2)), out); });
}
// par is clamped in place; *flag receives the returned out_of_bounds
int ref_unif_bounds(double* par, int n, const double* bounds, int* flag) {
  return guarded([&] {
    arma::vec p = to_vec(par, n);
    *flag = unif_bounds(p, to_mat(bounds, n, 2)) ? 1 : 0;
    put(p, par);
  });
}
int ref_calc_jacobian(const double* new_param, const double* param, int n, const double* bounds, double* out) {
  return guarded([&] { *out = calc_jacobian(to_vec(new_param, n), to_vec(param, n), to_mat(bounds, n, 2)); });
}
void ref_runif_push(const double* u, int n) { g_uniforms.insert(g_uniforms.end(), u, u + n); }
int ref_runif_pending() { return (int)g_uniforms.size(); }
void ref_runif_clear() { g_uniforms.clear(); }
int ref_do_I_accept(double logaccept, int* accepted) {
  return guarded([&] { *accepted = do_I_accept(logaccept) ? 1 : 0; });
}

void* ref_ram_create(int p, const double* metropolis_sd) {
  try {
    return new RAMAdapt(p, to_mat(metropolis_sd, p, p));
  } catch (...) {
    return nullptr;
  }
}
void ref_ram_destroy(void* h) { delete static_cast<RAMAdapt*>(h); }
void ref_ram_count_proposal(void* h) { static_cast<RAMAdapt*>(h)->count_proposal(); }
void ref_ram_count_accepted(void* h) { static_cast<RAMAdapt*>(h)->count_accepted(); }
void ref_ram_update_ratios(void* h) { static_cast<RAMAdapt*>(h)->update_ratios(); }
int ref_ram_adapt(void* h, const double* U, double alpha, int mc) {
  RAMAdapt* r = static_cast<RAMAdapt*>(h);
  return guarded([&] { r->adapt(to_vec(U, r->p), alpha, mc); });
}
void ref_ram_paramsd(void* h, double* out) { put(static_cast<RAMAdapt*>(h)->paramsd, out); }
void ref_ram_S(void* h, double* out) { put(static_cast<RAMAdapt*>(h)->S, out); }
int ref_ram_started(void* h) { return static_cast<RAMAdapt*>(h)->started ? 1 : 0; }
double ref_ram_accept_ratio(void* h) { return static_cast<RAMAdapt*>(h)->accept_ratio; }
int ref_ram_g0(void* h) { return static_cast<RAMAdapt*>(h)->g0; }

// ---- summaries --------------------------------------------------------------------------------------------------------------
// draws: keep matrices of nrows x ncols, one after the other
static arma::field<arma::mat> to_field(const double* p, int count, int nrows, int ncols) {
  arma::field<arma::mat> f(count);
  for (int i = 0; i < count; i++) f(i) = to_mat(p + (size_t)i * nrows * ncols, nrows, ncols);
  return f;
}
int ref_list_mean(const double* draws, int keep, int nrows, int ncols, double* out) {
  return guarded([&] { put(list_mean(to_field(draws, keep, nrows, ncols)), out); });
}
int ref_list_qtile(const double* draws, int keep, int nrows, int ncols, double q, double* out) {
  return guarded([&] { put(list_qtile(to_field(draws, keep, nrows, ncols), q), out); });
}

// find_not_nan (finite != 0) / find_nan over count matrices of nrows x ncols, filtered by column 0 of count matrices of
// nrows x fcols.  out receives the kept matrices one after the other (at most count * nrows * ncols doubles), out_rows their
// row counts.
int ref_find_nan(int finite, const double* infield, const double* filtering, int count, int nrows, int ncols, int fcols,
                 double* out, int* out_rows) {
  return guarded([&] {
    arma::field<arma::mat> a = to_field(infield, count, nrows, ncols), f = to_field(filtering, count, nrows, fcols);
    arma::field<arma::mat> r = finite ? find_not_nan(a, f) : find_nan(a, f);
    for (int i = 0; i < count; i++) {
      out_rows[i] = (int)r(i).n_rows;
      put(r(i), out);
      out += r(i).n_elem;
    }
  });
}

}  // extern "C"

// Stand-in for the subset of Armadillo and Rcpp that the reference's covariance_functions.{h,cpp}, mh_adapt.{h,cpp},
// list_mean.cpp and find_nan.{h,cpp} use, so that those files compile unchanged without R, Rcpp, RcppArmadillo, BLAS or LAPACK
// (oracle/Makefile, target _ref/libspamtree_ref.so).  Test infrastructure only; written for this repository, nothing copied.
//
// Everything is eager (no expression templates), column-major and header-only.
//
// Arithmetic rules:
//   * every sum and product is plain left-to-right double arithmetic: accu, sum, mean and norm add their terms in memory
//     order starting from 0.0; mat * mat accumulates over the inner index k = 0, 1, ... starting from 0.0; chol(., "lower")
//     subtracts its inner products in column order before the square root or the division;
//   * scalar * mat and mat / scalar apply the scalar to every element once, in the order the expression is written (Armadillo
//     may fold a scalar into the following product; the two differ in the last bit only);
//   * the library is built with -O2 and without -march / -mfma, so the compiler cannot contract a product and a sum into an
//     FMA.  Real Armadillo hands mat * mat and chol to the BLAS / LAPACK R was built with; their last bits are not reproduced.
//
// tests/refshim_check.cpp checks this header against hand-written known answers.  tests/stubs/RcppArmadillo.h is a different
// thing (declarations only, for the syntax check of the Rcpp shim) and stays separate.
#ifndef SPAMTREE_REFSHIM_RCPPARMADILLO_H
#define SPAMTREE_REFSHIM_RCPPARMADILLO_H

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

namespace arma {

typedef unsigned long long uword;

[[noreturn]] inline void shim_fail(const char* what) { throw std::logic_error(std::string("refshim: ") + what); }

class vec;
class rowvec;

class uvec {
public:
  uword n_elem, n_rows, n_cols;
  std::vector<uword> mem;
  uvec() : n_elem(0), n_rows(0), n_cols(1) {}
  explicit uvec(uword n) : n_elem(n), n_rows(n), n_cols(1), mem(n, 0) {}
  uword& operator()(uword i) { if (i >= n_elem) shim_fail("uvec index out of bounds"); return mem[i]; }
  const uword& operator()(uword i) const { if (i >= n_elem) shim_fail("uvec index out of bounds"); return mem[i]; }
  uvec& operator-=(uword k) { for (uword& v : mem) v -= k; return *this; }
  uvec& operator+=(uword k) { for (uword& v : mem) v += k; return *this; }
};

class mat {
public:
  uword n_rows, n_cols, n_elem;
  std::vector<double> mem;

  mat() : n_rows(0), n_cols(0), n_elem(0) {}
  mat(uword r, uword c) : n_rows(r), n_cols(c), n_elem(r * c), mem(r * c, 0.0) {}

  double& operator()(uword i) { if (i >= n_elem) shim_fail("index out of bounds"); return mem[i]; }
  const double& operator()(uword i) const { if (i >= n_elem) shim_fail("index out of bounds"); return mem[i]; }
  double& operator()(uword i, uword j) {
    if (i >= n_rows || j >= n_cols) shim_fail("index out of bounds");
    return mem[i + j * n_rows];
  }
  const double& operator()(uword i, uword j) const {
    if (i >= n_rows || j >= n_cols) shim_fail("index out of bounds");
    return mem[i + j * n_rows];
  }
  double* memptr() { return mem.data(); }
  const double* memptr() const { return mem.data(); }
  double* begin() { return mem.data(); }
  double* end() { return mem.data() + n_elem; }
  const double* begin() const { return mem.data(); }
  const double* end() const { return mem.data() + n_elem; }

  // sub-views are copies; bounds are inclusive, as Armadillo's
  mat submat(uword r0, uword c0, uword r1, uword c1) const {
    if (r1 < r0 || c1 < c0 || r1 >= n_rows || c1 >= n_cols) shim_fail("submat out of bounds");
    mat out(r1 - r0 + 1, c1 - c0 + 1);
    for (uword j = c0; j <= c1; j++)
      for (uword i = r0; i <= r1; i++) out(i - r0, j - c0) = (*this)(i, j);
    return out;
  }
  mat subvec(uword a, uword b) const {
    if (n_cols == 1) return submat(a, 0, b, 0);
    if (n_rows == 1) return submat(0, a, 0, b);
    shim_fail("subvec of a matrix");
  }
  inline rowvec row(uword i) const;
  inline vec col(uword j) const;
  mat rows(const uvec& ix) const {
    mat out(ix.n_elem, n_cols);
    for (uword j = 0; j < n_cols; j++)
      for (uword i = 0; i < ix.n_elem; i++) out(i, j) = (*this)(ix(i), j);
    return out;
  }
  mat t() const {
    mat out(n_cols, n_rows);
    for (uword j = 0; j < n_cols; j++)
      for (uword i = 0; i < n_rows; i++) out(j, i) = (*this)(i, j);
    return out;
  }
  mat& operator+=(const mat& b) {
    if (b.n_rows != n_rows || b.n_cols != n_cols) shim_fail("+= of different sizes");
    for (uword i = 0; i < n_elem; i++) mem[i] += b.mem[i];
    return *this;
  }
  mat& operator-=(const mat& b) {
    if (b.n_rows != n_rows || b.n_cols != n_cols) shim_fail("-= of different sizes");
    for (uword i = 0; i < n_elem; i++) mem[i] -= b.mem[i];
    return *this;
  }
};

class vec : public mat {
public:
  vec() : mat(0, 1) {}
  explicit vec(uword n) : mat(n, 1) {}
  vec(const mat& m) : mat(m) { if (n_cols != 1 && n_elem != 0) shim_fail("vec from a matrix with several columns"); }
};

class rowvec : public mat {
public:
  rowvec() : mat(1, 0) {}
  explicit rowvec(uword n) : mat(1, n) {}
  rowvec(const mat& m) : mat(m) { if (n_rows != 1 && n_elem != 0) shim_fail("rowvec from a matrix with several rows"); }
};

inline rowvec mat::row(uword i) const { return rowvec(submat(i, 0, i, n_cols - 1)); }
inline vec mat::col(uword j) const { return vec(submat(0, j, n_rows - 1, j)); }

class cube {
public:
  uword n_rows, n_cols, n_slices;
  std::vector<mat> slices;
  cube() : n_rows(0), n_cols(0), n_slices(0) {}
  cube(uword r, uword c, uword s) : n_rows(r), n_cols(c), n_slices(s), slices(s, mat(r, c)) {}
  mat& slice(uword k) { if (k >= n_slices) shim_fail("slice out of bounds"); return slices[k]; }
  const mat& slice(uword k) const { if (k >= n_slices) shim_fail("slice out of bounds"); return slices[k]; }
};

template <class T>
class field {
public:
  uword n_elem;
  std::vector<T> mem;
  field() : n_elem(0) {}
  explicit field(uword n) : n_elem(n), mem(n) {}
  T& operator()(uword i) { if (i >= n_elem) shim_fail("field index out of bounds"); return mem[i]; }
  const T& operator()(uword i) const { if (i >= n_elem) shim_fail("field index out of bounds"); return mem[i]; }
};

// ---- generators
inline vec zeros(uword n) { return vec(n); }
inline mat zeros(uword r, uword c) { return mat(r, c); }
template <class T> inline T zeros(uword n) { return T(n); }
inline mat ones(uword r, uword c) { mat m(r, c); std::fill(m.mem.begin(), m.mem.end(), 1.0); return m; }
inline vec ones(uword n) { return vec(ones(n, 1)); }
template <class T> inline T ones(uword n) { T m(n); std::fill(m.mem.begin(), m.mem.end(), 1.0); return m; }
inline mat eye(uword r, uword c) { mat m(r, c); for (uword i = 0; i < std::min(r, c); i++) m(i, i) = 1.0; return m; }

// ---- elementwise arithmetic
inline mat operator+(const mat& a, const mat& b) {
  if (a.n_rows != b.n_rows || a.n_cols != b.n_cols) shim_fail("+ of different sizes");
  mat out(a.n_rows, a.n_cols);
  for (uword i = 0; i < a.n_elem; i++) out.mem[i] = a.mem[i] + b.mem[i];
  return out;
}
inline mat operator-(const mat& a, const mat& b) {
  if (a.n_rows != b.n_rows || a.n_cols != b.n_cols) shim_fail("- of different sizes");
  mat out(a.n_rows, a.n_cols);
  for (uword i = 0; i < a.n_elem; i++) out.mem[i] = a.mem[i] - b.mem[i];
  return out;
}
inline mat operator%(const mat& a, const mat& b) {
  if (a.n_rows != b.n_rows || a.n_cols != b.n_cols) shim_fail("% of different sizes");
  mat out(a.n_rows, a.n_cols);
  for (uword i = 0; i < a.n_elem; i++) out.mem[i] = a.mem[i] * b.mem[i];
  return out;
}
inline mat operator*(double s, const mat& a) { mat out(a); for (double& v : out.mem) v = s * v; return out; }
inline mat operator*(const mat& a, double s) { mat out(a); for (double& v : out.mem) v = v * s; return out; }
inline mat operator/(const mat& a, double s) { mat out(a); for (double& v : out.mem) v = v / s; return out; }
inline mat operator*(const mat& a, const mat& b) {
  if (a.n_cols != b.n_rows) shim_fail("* of incompatible sizes");
  mat out(a.n_rows, b.n_cols);
  for (uword j = 0; j < b.n_cols; j++)
    for (uword i = 0; i < a.n_rows; i++) {
      double acc = 0.0;
      for (uword k = 0; k < a.n_cols; k++) acc += a(i, k) * b(k, j);
      out(i, j) = acc;
    }
  return out;
}

// ---- elementwise functions
inline mat exp(const mat& a) { mat out(a); for (double& v : out.mem) v = std::exp(v); return out; }
inline mat sqrt(const mat& a) { mat out(a); for (double& v : out.mem) v = std::sqrt(v); return out; }
inline mat abs(const mat& a) { mat out(a); for (double& v : out.mem) v = std::fabs(v); return out; }
inline mat log(const mat& a) { mat out(a); for (double& v : out.mem) v = std::log(v); return out; }

// ---- reductions
inline double accu(const mat& a) { double s = 0.0; for (double v : a.mem) s += v; return s; }
inline double mean(const mat& a) { return accu(a) / (double)a.n_elem; }
inline double norm(const mat& a) { double s = 0.0; for (double v : a.mem) s += v * v; return std::sqrt(s); }
inline mat sum(const mat& a, uword dim) {
  if (dim == 0) {                                       // down each column: 1 x n_cols
    mat out(1, a.n_cols);
    for (uword j = 0; j < a.n_cols; j++) { double s = 0.0; for (uword i = 0; i < a.n_rows; i++) s += a(i, j); out(0, j) = s; }
    return out;
  }
  if (dim != 1) shim_fail("sum: dim must be 0 or 1");
  mat out(a.n_rows, 1);                                  // along each row: n_rows x 1
  for (uword i = 0; i < a.n_rows; i++) { double s = 0.0; for (uword j = 0; j < a.n_cols; j++) s += a(i, j); out(i, 0) = s; }
  return out;
}

// ---- structure
inline mat repmat(const mat& a, uword r, uword c) {
  mat out(a.n_rows * r, a.n_cols * c);
  for (uword j = 0; j < out.n_cols; j++)
    for (uword i = 0; i < out.n_rows; i++) out(i, j) = a(i % a.n_rows, j % a.n_cols);
  return out;
}
inline mat symmatl(const mat& a) {                       // the lower triangle, mirrored upwards
  if (a.n_rows != a.n_cols) shim_fail("symmatl of a non-square matrix");
  mat out(a);
  for (uword j = 0; j < a.n_cols; j++)
    for (uword i = j + 1; i < a.n_rows; i++) out(j, i) = a(i, j);
  return out;
}
inline mat symmatu(const mat& a) {                       // the upper triangle, mirrored downwards
  if (a.n_rows != a.n_cols) shim_fail("symmatu of a non-square matrix");
  mat out(a);
  for (uword j = 0; j < a.n_cols; j++)
    for (uword i = j + 1; i < a.n_rows; i++) out(i, j) = a(j, i);
  return out;
}

// ---- finiteness
inline bool is_finite(double x) { return std::isfinite(x); }
inline uvec find_finite(const mat& a) {
  uvec out;
  for (uword i = 0; i < a.n_elem; i++) if (std::isfinite(a.mem[i])) out.mem.push_back(i);
  out.n_elem = out.n_rows = out.mem.size();
  return out;
}
inline uvec find_nonfinite(const mat& a) {
  uvec out;
  for (uword i = 0; i < a.n_elem; i++) if (!std::isfinite(a.mem[i])) out.mem.push_back(i);
  out.n_elem = out.n_rows = out.mem.size();
  return out;
}

// ---- Cholesky: A = L L', reads the lower triangle; throws like Armadillo when A is not positive definite
inline mat chol(const mat& a, const char* layout) {
  if (std::strcmp(layout, "lower") != 0) shim_fail("chol: only \"lower\" is provided");
  if (a.n_rows != a.n_cols) shim_fail("chol of a non-square matrix");
  const uword n = a.n_rows;
  mat L(n, n);
  for (uword j = 0; j < n; j++) {
    double d = a(j, j);
    for (uword k = 0; k < j; k++) d -= L(j, k) * L(j, k);
    if (!(d > 0.0) || !std::isfinite(d)) throw std::runtime_error("chol(): decomposition failed");
    const double ljj = std::sqrt(d);
    L(j, j) = ljj;
    for (uword i = j + 1; i < n; i++) {
      double s = a(i, j);
      for (uword k = 0; k < j; k++) s -= L(i, k) * L(j, k);
      L(i, j) = s / ljj;
    }
  }
  return L;
}

}  // namespace arma

namespace Rcpp {
inline std::ostream& Rcout = std::cerr;
[[noreturn]] inline void stop(const std::string& msg) { throw std::runtime_error(msg); }
struct RNGScope {
  RNGScope() {}
  ~RNGScope() {}
};
}  // namespace Rcpp

namespace R {
double runif(double a, double b);                        // declared only: whoever links the reference's files defines it
}

inline void Rprintf(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vfprintf(stderr, fmt, ap);
  va_end(ap);
}

#endif

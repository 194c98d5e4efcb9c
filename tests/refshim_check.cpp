// Stand-alone check of oracle/refshim/RcppArmadillo.h (the Armadillo / Rcpp stand-in the reference's files are compiled against)
// with hand-written known answers.  Built and run by tests/test_refshim_cpu.py; host code only, so it may also be built with
// -fsanitize=address,undefined.  Prints the first failed check and exits 1; prints "refshim ok <count>" and exits 0 otherwise.
#include <cstdio>
#include <cstdlib>

#include "RcppArmadillo.h"

namespace R {
double runif(double, double) { return 0.25; }
}

static int checks = 0;
#define CHECK(cond)                                                           \
  do {                                                                        \
    checks++;                                                                 \
    if (!(cond)) {                                                            \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);                   \
      return 1;                                                               \
    }                                                                         \
  } while (0)

template <class F>
static bool throws(F f) {
  try {
    f();
  } catch (...) {
    return true;
  }
  return false;
}

int main() {
  using namespace arma;
  // ---- the column-major (i, j) mapping: A = [1 3 5; 2 4 6] filled through memptr in memory order
  mat A(2, 3);
  for (int k = 0; k < 6; k++) A.memptr()[k] = k + 1.0;
  CHECK(A.n_rows == 2 && A.n_cols == 3 && A.n_elem == 6);
  CHECK(A(0, 0) == 1 && A(1, 0) == 2 && A(0, 1) == 3 && A(1, 1) == 4 && A(0, 2) == 5 && A(1, 2) == 6);
  CHECK(A(3) == 4 && A(4) == 5);                                    // linear index = i + j * n_rows
  CHECK(*A.begin() == 1 && A.end() - A.begin() == 6);
  CHECK(throws([&] { (void)A(2, 0); }) && throws([&] { (void)A(6); }));
  mat At = A.t();
  CHECK(At.n_rows == 3 && At.n_cols == 2 && At(2, 0) == 5 && At(0, 1) == 2 && At(1, 1) == 4);

  // ---- inclusive subvec bounds, on a column and on a row
  vec v = zeros(6);
  for (int k = 0; k < 6; k++) v(k) = 10.0 * k;
  vec s = v.subvec(1, 3);
  CHECK(s.n_elem == 3 && s.n_rows == 3 && s.n_cols == 1 && s(0) == 10 && s(2) == 30);
  vec one = v.subvec(4, 4);
  CHECK(one.n_elem == 1 && one(0) == 40);
  rowvec r = v.t();
  rowvec rs = r.subvec(0, 1);
  CHECK(rs.n_rows == 1 && rs.n_cols == 2 && rs(1) == 10);
  CHECK(throws([&] { (void)v.subvec(3, 6); }));
  mat sm = A.submat(0, 1, 1, 2);
  CHECK(sm.n_rows == 2 && sm.n_cols == 2 && sm(0, 0) == 3 && sm(1, 1) == 6);
  CHECK(A.row(1).n_cols == 3 && A.row(1)(2) == 6 && A.col(2).n_rows == 2 && A.col(2)(0) == 5);

  // ---- rows(uvec): the order of the index vector, repeats included
  uvec ix(3);
  ix(0) = 2; ix(1) = 0; ix(2) = 2;
  mat R3 = At.rows(ix);                                             // At = [1 2; 3 4; 5 6]
  CHECK(R3.n_rows == 3 && R3.n_cols == 2);
  CHECK(R3(0, 0) == 5 && R3(0, 1) == 6 && R3(1, 0) == 1 && R3(1, 1) == 2 && R3(2, 0) == 5 && R3(2, 1) == 6);
  ix -= 1;                                                          // 1, wraps, 1: only the arithmetic is checked
  CHECK(ix(0) == 1 && ix(2) == 1);

  // ---- symmatl against symmatu on B = [1 2 3; 4 5 6; 7 8 9]
  mat B(3, 3);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) B(i, j) = 3 * i + j + 1.0;
  mat Lo = symmatl(B), Up = symmatu(B);
  CHECK(Lo(0, 1) == 4 && Lo(1, 0) == 4 && Lo(0, 2) == 7 && Lo(2, 0) == 7 && Lo(1, 2) == 8 && Lo(2, 1) == 8 && Lo(1, 1) == 5);
  CHECK(Up(0, 1) == 2 && Up(1, 0) == 2 && Up(0, 2) == 3 && Up(2, 0) == 3 && Up(1, 2) == 6 && Up(2, 1) == 6 && Up(2, 2) == 9);

  // ---- repmat tiling: of a column side by side, of a row downwards, of a matrix both ways
  vec c2 = zeros(2);
  c2(0) = 1; c2(1) = 2;
  mat T1 = repmat(c2, 1, 3);
  CHECK(T1.n_rows == 2 && T1.n_cols == 3 && T1(0, 2) == 1 && T1(1, 0) == 2 && T1(1, 2) == 2);
  mat T2 = repmat(c2.t(), 3, 1);
  CHECK(T2.n_rows == 3 && T2.n_cols == 2 && T2(2, 0) == 1 && T2(0, 1) == 2 && T2(2, 1) == 2);
  mat T3 = repmat(A, 2, 2);
  CHECK(T3.n_rows == 4 && T3.n_cols == 6 && T3(2, 0) == 1 && T3(3, 5) == 6 && T3(1, 4) == 4 && T3(2, 3) == 1);

  // ---- sum along both dimensions: dim 0 gives the column sums as a row, dim 1 the row sums as a column
  mat S0 = sum(A, 0), S1 = sum(A, 1);
  CHECK(S0.n_rows == 1 && S0.n_cols == 3 && S0(0) == 3 && S0(1) == 7 && S0(2) == 11);
  CHECK(S1.n_rows == 2 && S1.n_cols == 1 && S1(0) == 9 && S1(1) == 12);
  CHECK(accu(A) == 21 && mean(v) == 25 && norm(At.row(1)) == 5);    // |(3, 4)| = 5

  // ---- arithmetic
  mat P = A * At;                                                   // [35 44; 44 56]
  CHECK(P.n_rows == 2 && P.n_cols == 2 && P(0, 0) == 35 && P(0, 1) == 44 && P(1, 0) == 44 && P(1, 1) == 56);
  mat O = c2 * c2.t() / 2.0;                                        // outer product [0.5 1; 1 2]
  CHECK(O(0, 0) == 0.5 && O(1, 0) == 1 && O(0, 1) == 1 && O(1, 1) == 2);
  mat E = (A % A) + 2 * A - A;                                      // x^2 + x
  CHECK(E(1, 2) == 42 && E(0, 0) == 2);
  E -= A;
  E += ones(2, 3);
  CHECK(E(1, 2) == 37 && E(0, 1) == 10);
  CHECK(throws([&] { (void)(A + At); }) && throws([&] { (void)(A * A); }));
  mat F = sqrt(abs(-1.0 * (A % A)));
  CHECK(F(1, 1) == 4 && F(0, 2) == 5);
  CHECK(exp(zeros(2, 2))(1, 1) == 1 && log(ones(2, 2))(0, 1) == 0);
  CHECK(eye(3, 3)(1, 1) == 1 && eye(3, 3)(1, 2) == 0 && ones<rowvec>(3).n_cols == 3 && zeros<rowvec>(4).n_rows == 1);

  // ---- chol(., "lower"): A = L L' with L = [2 0 0; 6 1 0; -8 5 3] (all steps exact in binary); throws when indefinite
  mat L(3, 3);
  L(0, 0) = 2; L(1, 0) = 6; L(2, 0) = -8; L(1, 1) = 1; L(2, 1) = 5; L(2, 2) = 3;
  mat SPD = L * L.t();
  CHECK(SPD(0, 0) == 4 && SPD(1, 0) == 12 && SPD(2, 0) == -16 && SPD(1, 1) == 37 && SPD(2, 1) == -43 && SPD(2, 2) == 98);
  mat C = chol(SPD, "lower");
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) CHECK(C(i, j) == L(i, j));
  mat Ind = SPD;
  Ind(2, 2) = 89 - 1;                                               // 98 -> 88: the last pivot is 88 - 64 - 25 = -1
  CHECK(throws([&] { (void)chol(Ind, "lower"); }));
  mat Z = zeros(2, 2);
  CHECK(throws([&] { (void)chol(Z, "lower"); }));

  // ---- finiteness
  vec f = zeros(4);
  f(1) = NAN; f(3) = INFINITY;
  uvec fin = find_finite(f), non = find_nonfinite(f);
  CHECK(fin.n_elem == 2 && fin(0) == 0 && fin(1) == 2 && non.n_elem == 2 && non(0) == 1 && non(1) == 3);
  CHECK(is_finite(1.0) && !is_finite(NAN) && !is_finite(-INFINITY));

  // ---- field, cube, Rcpp
  field<mat> fl(2);
  fl(1) = A;
  CHECK(fl.n_elem == 2 && fl(1)(4) == 5 && fl(0).n_elem == 0);
  cube cb(2, 2, 3);
  cb.slice(2)(1, 1) = 7;
  CHECK(cb.n_slices == 3 && cb.slice(2)(3) == 7 && cb.slice(0)(3) == 0);
  CHECK(throws([] { Rcpp::stop("stop"); }));
  Rcpp::RNGScope scope;
  CHECK(R::runif(0, 1) == 0.25);

  std::printf("refshim ok %d\n", checks);
  return 0;
}

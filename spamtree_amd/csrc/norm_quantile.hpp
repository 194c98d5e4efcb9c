// The standard normal quantile function, one text for the host, the device and the CPU check (tests/rank_norm_check.cpp): plain C++
// that compiles with or without HIP.  Wichura's algorithm AS 241 (Applied Statistics 37, 1988), routine PPND16: three rational
// approximations of degree 7 / 7, in q = p - 1/2 for |q| <= 0.425 and in r = sqrt(-log(min(p, 1 - p))) for the tails (r <= 5 and
// r > 5).  Published accuracy about 1 part in 1e16; the error measured against 50-digit arithmetic on the arguments the rank
// normalisation uses is recorded in DESIGN.md section 23.  Horner's rule in the order written, one division: the only operations
// whose rounding may differ between the host's and the device's compiler are the contraction of a * b + c into an fma and log().
// 1 - p is exact for p >= 1/2 (Sterbenz), so the upper tail is as accurate as the lower.
// p = 0 gives -inf, p = 1 gives +inf, p outside [0, 1] or NaN gives NaN.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ST_NQ_HD __host__ __device__
#else
#define ST_NQ_HD
#endif

ST_NQ_HD inline double st_norm_quantile_f(double p) {
  if (!(p >= 0.0 && p <= 1.0)) return NAN;
  const double q = p - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    const double num = (((((((2509.0809287301226727 * r + 33430.575583588128105) * r + 67265.770927008700853) * r +
                            45921.953931549871457) * r + 13731.693765509461125) * r + 1971.5909503065514427) * r +
                         133.14166789178437745) * r + 3.387132872796366608);
    const double den = (((((((5226.495278852545925 * r + 28729.085735721942674) * r + 39307.89580009271061) * r +
                            21213.794301586595867) * r + 5394.1960214247511077) * r + 687.1870074920579083) * r +
                         42.313330701600911252) * r + 1.0);
    return q * num / den;
  }
  const double t = q < 0.0 ? p : 1.0 - p;
  if (t == 0.0) return q < 0.0 ? -INFINITY : INFINITY;
  double r = sqrt(-log(t));
  double num, den;
  if (r <= 5.0) {
    r -= 1.6;
    num = (((((((7.7454501427834140764e-4 * r + 0.0227238449892691845833) * r + 0.24178072517745061177) * r +
               1.27045825245236838258) * r + 3.64784832476320460504) * r + 5.7694972214606914055) * r +
            4.6303378461565452959) * r + 1.42343711074968357734);
    den = (((((((1.05075007164441684324e-9 * r + 5.475938084995344946e-4) * r + 0.0151986665636164571966) * r +
               0.14810397642748007459) * r + 0.68976733498510000455) * r + 1.6763848301838038494) * r +
            2.05319162663775882187) * r + 1.0);
  } else {
    r -= 5.0;
    num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 0.0012426609473880784386) * r +
               0.026532189526576123093) * r + 0.29656057182850489123) * r + 1.7848265399172913358) * r +
            5.4637849111641143699) * r + 6.6579046435011037772);
    den = (((((((2.04426310338993978564e-15 * r + 1.4215117583164458887e-7) * r + 1.8463183175100546818e-5) * r +
               7.868691311456132591e-4) * r + 0.0148753612908506148525) * r + 0.13692988092273580531) * r +
            0.59983220655588793769) * r + 1.0);
  }
  const double v = num / den;
  return q < 0.0 ? -v : v;
}

// The normal score of twice-the-average-rank r2 (an integer in 2 .. 2K) among K draws: p = (4 r2 - 3) / (8 K + 2), one double
// division of two exact integers, which is (r - 3/8) / (K + 1/4) for the average 1-based rank r = r2 / 2 (Blom's offset).
ST_NQ_HD inline double st_rank_score(int r2, int K) {
  return st_norm_quantile_f((double)(4 * r2 - 3) / (double)(8 * K + 2));
}

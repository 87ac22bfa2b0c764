// PIT, NLL and CRPS of the Student-t posterior predictive of the Normal-Inverse-Gamma heads at one pixel, in double from
// the fp32 heads (csrc/evidential.h: nig_head), rounded once into the three fp32 results.  Host and device: the kernel
// (score_evidential.hip) and a host program can run the same lines.
//
//   nu = 2 alpha,  sigma = sqrt(beta (1 + v) / (v alpha)),  z = (y - mu) / sigma,  x = nu / (nu + z^2)
//   PIT   u = F_nu(z) = I_x(alpha, 1/2) / 2  (z <= 0),  1 - I_x(alpha, 1/2) / 2  (z > 0)
//   NLL   -lgamma(alpha + 1/2) + lgamma(alpha) + ln(nu pi) / 2 + ln sigma + (alpha + 1/2) log1p(z^2 / nu)
//   CRPS  sigma [ z (2 F - 1) + 2 f (nu + z^2) / (nu - 1) - 2 sqrt(nu) / (nu - 1) B(1/2, nu - 1/2) / B(1/2, nu/2)^2 ]
//         (Jordan, Krueger, Lerch 2019; f the standard t density; valid for nu > 1, and nu >= 2 here)
//
// Why double: the modified-Lentz continued fraction of I_x(a, b) in fp32 loses up to 1e-3 relative at large nu with x near
// its branch limit (its first denominator 1 - (a + b) x / (a + 1) cancels), and log f is a difference of terms of size
// alpha log1p(z^2 / nu) and lgamma.
//
// Gamma ratios.  Both beta functions are half-offset ratios, B(1/2, a) = sqrt(pi) Gamma(a) / Gamma(a + 1/2), so with
//   R(a) = Gamma(a - 1/2) / Gamma(a)   (= 4 G(a) of csrc/evidential.h: nig_gamma, restated in double)
// B(1/2, nu/2) = sqrt(pi) R(alpha + 1/2) and B(1/2, nu - 1/2) = sqrt(pi) R(2 alpha).  R comes from the recurrence
// R(a) = R(a + 1) a / (a - 1/2) up to a >= 16 (at most 15 steps; numerator and denominator as two products, one division)
// and there from nig_gamma's six-term series of the difference of the two lgammas, whose truncation error shrinks like
// a^-7: 1.1e-9 at 8, under 1e-11 from 16 on — five orders below the fp32 ulp the results are rounded to.  No lgamma call.
//
// Incomplete beta.  I_x(a, b) = x^a (1 - x)^b / (a B(a, b)) h, h the continued fraction (Numerical Recipes betacf), which
// converges quickly for x < (a + 1) / (a + b + 2).  With b = 1/2:
//   x < (alpha + 1) / (alpha + 2.5):  I = I_x(alpha, 1/2) directly                          (the tails: |z| large)
//   otherwise:                        J = I_{1-x}(1/2, alpha) = 1 - I, with 1 - x formed as z^2 / (nu + z^2), never by
//                                     subtraction                                           (the centre: |z| small)
// Both share the factor x^alpha sqrt(1 - x) / (sqrt(pi) R(alpha + 1/2)) and differ in the divisor (alpha or 1/2), and
// x^alpha = exp(-alpha log1p(z^2 / nu)) also gives the density f: one exponential per pixel.  2 F - 1 = sign(z) J is exact
// at the centre (no 1 - 2 F), the lower tail u = I / 2 is formed directly, and z == 0 gives J = 0, u = 0.5 exactly.
//
// The iteration has a compile-time cap, kBetaCap, and leaves only by convergence (the last factor within kBetaEps = 2^-50 of
// 1) or at the cap; a pixel that reaches the cap keeps the value it has.  Counted on the host with this code over the test
// ranges (nu in [2, 6e4], |z| up to 1e6, and a scan of |z| from 1e-3 to 1e6 times its value at the branch limit): at most
// 107 iterations, on the direct branch right at the limit at the largest nu (8 on the other side of it; the random draws
// of the tests take 12 on average and at most 71); the cap is 160.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace mimo {
namespace score {

constexpr int kBetaCap = 160;
constexpr double kBetaEps = 0x1p-50;
constexpr double kSqrtPi = 1.7724538509055160273;
constexpr double kPi = 3.14159265358979323846;

// R(a) = Gamma(a - 1/2) / Gamma(a), a >= 1.5
__host__ __device__ inline double gamma_half_ratio(double a) {
  double num = 1.0, den = 1.0;
  for (int k = 0; k < 15 && a < 16.0; ++k) {
    num *= a;
    den *= a - 0.5;
    a += 1.0;
  }
  const double i = 1.0 / a;
  const double P = i * (0.375 + i * (0.125 + i * (3.0 / 64.0 + i * (1.0 / 64.0 + i * (3.0 / 640.0 + i * (1.0 / 384.0))))));
  return num * exp(P) / (den * sqrt(a));
}

// the continued fraction h of I_x(a, b), x < (a + 1) / (a + b + 2), by the modified Lentz recurrence, three divisions per
// half step.  (Folding the partial numerator n / e into the two updates — d <- e / (e + n d), c <- (e c + n) / (e c) —
// saves a division but leaves the last factor wandering 1e-13 around 1 at alpha = 3e4: it reaches the cap instead of
// converging after 19 iterations.)
__host__ __device__ inline double beta_fraction(double a, double b, double x, int& iterations) {
  constexpr double tiny = 1e-300;
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * x / qap;
  d = 1.0 / (fabs(d) < tiny ? tiny : d);
  double h = d;
  int m = 1;
  for (; m <= kBetaCap; ++m) {
    const double m2 = 2.0 * m;
    double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    c = 1.0 + aa / c;
    d = 1.0 / (fabs(d) < tiny ? tiny : d);
    c = fabs(c) < tiny ? tiny : c;
    h *= d * c;
    aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    c = 1.0 + aa / c;
    d = 1.0 / (fabs(d) < tiny ? tiny : d);
    c = fabs(c) < tiny ? tiny : c;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) < kBetaEps) break;
  }
  iterations = m < kBetaCap ? m : kBetaCap;
  return h;
}

// v > 0, beta > 0, alpha >= 1 and every input finite (the caller's skip rule)
__host__ __device__ inline void student_t_scores(float mu, float v, float alpha, float beta, float y, float& pit, float& nll,
                                                 float& crps, int& iterations) {
  const double a = (double)alpha, nu = 2.0 * a, vd = (double)v;
  const double s2 = (double)beta * (1.0 + vd) / (vd * a), sigma = sqrt(s2);
  const double z = ((double)y - (double)mu) / sigma, z2 = z * z;
  const double l1p = log1p(z2 / nu);            // -ln x
  const double x = nu / (nu + z2), xc = z2 / (nu + z2);
  const double R1 = gamma_half_ratio(a + 0.5);  // Gamma(alpha) / Gamma(alpha + 1/2)
  const double R2 = gamma_half_ratio(nu);       // Gamma(nu - 1/2) / Gamma(nu)
  const double xa = exp(-a * l1p);              // x^alpha
  const double front = xa * sqrt(xc) / (kSqrtPi * R1);
  const bool direct = x < (a + 1.0) / (a + 2.5);
  double I, J;  // P(|T| > |z|) and P(|T| <= |z|)
  if (direct) {
    I = front / a * beta_fraction(a, 0.5, x, iterations);
    J = 1.0 - I;
  } else {
    J = 2.0 * front * beta_fraction(0.5, a, xc, iterations);
    I = 1.0 - J;
  }
  const double u = z <= 0.0 ? 0.5 * I : (direct ? 1.0 - 0.5 * I : 0.5 + 0.5 * J);
  const double f = xa * sqrt(x) / (sqrt(nu) * kSqrtPi * R1);  // x^(alpha + 1/2) / (sqrt(nu) B(1/2, nu/2))
  const double c = sigma * (fabs(z) * J + 2.0 * f * (nu + z2) / (nu - 1.0) - 2.0 * sqrt(nu) / (nu - 1.0) * R2 / (kSqrtPi * R1 * R1));
  const double l = log(R1) + 0.5 * log(nu * kPi * s2) + (a + 0.5) * l1p;
  pit = (float)u;
  nll = (float)l;
  crps = (float)c;
}

}  // namespace score
}  // namespace mimo

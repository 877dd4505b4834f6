// svsdf_scale_host.hpp -- rigorous bounds of a scale schedule s_a(t) = c_a + sin(w_a t + phi_a) A_a (a = x, y) over a time
// interval, for the certified clearance under a schedule (svsdf_scale_bounds; DESIGN.md §4e "Under a scale schedule").
// Plain C++ with no HIP and no kernel header, like svsdf_traj_host.hpp: a host compiler builds it alone.
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>

#include "../../include/svsdf_c.h"

namespace svsdf_traj {

// What check_scale found: SVSDF_OK, or SVSDF_ERR_INVALID and a short reason.  The rules are svsdf_set_scale's.
struct ScaleCheck { int code; const char *reason; };
inline ScaleCheck check_scale(const svsdf_scale *s) {
  if (!s) return {SVSDF_OK, ""};
  if (s->struct_size != (int)sizeof(svsdf_scale)) return {SVSDF_ERR_INVALID, "struct_size is not sizeof(svsdf_scale)"};
  if (!s->enabled) return {SVSDF_OK, ""};
  for (int a = 0; a < 2; ++a) {
    const double v[4] = {s->c[a], s->amp[a], s->omega[a], s->phase[a]};
    for (double x : v)
      if (!std::isfinite(x)) return {SVSDF_ERR_INVALID, "non-finite parameter"};
    if (!(s->c[a] - std::fabs(s->amp[a]) > 0.0))
      return {SVSDF_ERR_INVALID, a ? "s_y(t) can reach 0 (c - |A| <= 0): S(t) would be singular"
                                   : "s_x(t) can reach 0 (c - |A| <= 0): S(t) would be singular"};
  }
  return {SVSDF_OK, ""};
}

// Ranges of sin and of |cos| over the argument interval [lo, hi] (lo <= hi, already widened by its own rounding): the
// endpoints' values, and the extrema the interval contains -- sin = +1 at pi/2 + 2 k pi, -1 at -pi/2 + 2 k pi; |cos| = 1
// at k pi, 0 at pi/2 + k pi.  "Contains" is decided with a margin `tol` that only ever widens a range.
struct TrigRange { double sin_lo, sin_hi, acos_lo, acos_hi; };
inline TrigRange trig_range(double lo, double hi, double tol) {
  constexpr double kPi = 3.14159265358979323846;
  TrigRange r;
  const double sa = std::sin(lo), sb = std::sin(hi), ca = std::fabs(std::cos(lo)), cb = std::fabs(std::cos(hi));
  r.sin_lo = std::min(sa, sb); r.sin_hi = std::max(sa, sb);
  r.acos_lo = std::min(ca, cb); r.acos_hi = std::max(ca, cb);
  // the first x0 + k * period at or after lo - tol lies at or before hi + tol
  auto contains = [&](double x0, double period) {
    const double k = std::ceil((lo - tol - x0) / period);
    return x0 + k * period <= hi + tol;
  };
  if (!(hi - lo < 2.0 * kPi) || contains(0.5 * kPi, 2.0 * kPi)) r.sin_hi = 1.0;
  if (!(hi - lo < 2.0 * kPi) || contains(-0.5 * kPi, 2.0 * kPi)) r.sin_lo = -1.0;
  if (!(hi - lo < kPi) || contains(0.0, kPi)) r.acos_hi = 1.0;
  if (!(hi - lo < kPi) || contains(0.5 * kPi, kPi)) r.acos_lo = 0.0;
  return r;
}

// out4 = { Smin, Smax, Imax, Q } over [ta, tb] (ta <= tb, the schedule valid by check_scale):
//   Smin = inf_t min_a s_a (rounded down)           Smax = sup_t max_a s_a (rounded up)
//   Imax = sup_t max_a 1 / s_a (rounded up)         Q = sup_t max_a |s_a'| / s_a^2 (rounded up), s_a' = A_a w_a cos(w_a t + phi_a)
// Per axis s_a ranges over exactly c + A [sin_lo, sin_hi]; Q_a <= |A w| sup|cos| / (inf s_a)^2, the product of the factors'
// suprema -- which exceeds the supremum of the product by at most (tb - ta) |A w^2| / (inf s_a)^2, the range of |cos| over
// the interval.  The argument interval is widened by the rounding of w t + phi (two operations on numbers of size
// |w t| + |phi|) and by as much again for the device's own evaluation of the same argument; the results by 1e-12, far above
// the last-bit errors of sin, cos, the divisions and the device's 1 / (s_x s_y) form of the inverse.
inline void scale_bounds(const svsdf_scale *s, double ta, double tb, double out4[4]) {
  out4[0] = out4[1] = out4[2] = 1.0;
  out4[3] = 0.0;
  if (!s || !s->enabled) return;
  double smin = std::numeric_limits<double>::infinity(), smax = 0.0, imax = 0.0, q = 0.0;
  for (int a = 0; a < 2; ++a) {
    const double c = s->c[a], A = s->amp[a], w = s->omega[a], ph = s->phase[a];
    if (A == 0.0) {   // s_a = c exactly, on the device too (c + sin(..) * 0); c = 1 inverts to exactly 1 there (scale_inv)
      smin = std::min(smin, c);
      smax = std::max(smax, c);
      imax = std::max(imax, c == 1.0 ? 1.0 : (1.0 / c) * (1.0 + 1e-12));
      continue;
    }
    const double xa = w * ta + ph, xb = w * tb + ph;
    const double mag = std::fabs(w) * std::max(std::fabs(ta), std::fabs(tb)) + std::fabs(ph);
    const double tol = 8.0 * std::numeric_limits<double>::epsilon() * mag + 1e-300;
    const double lo = std::min(xa, xb) - tol, hi = std::max(xa, xb) + tol;
    const TrigRange r = trig_range(lo, hi, tol + 1e-15 * (1.0 + std::fabs(lo) + std::fabs(hi)));
    const double v0 = A * r.sin_lo, v1 = A * r.sin_hi;
    // (never outside [c - |A|, c + |A|]: the range of s_a over all t, and c - |A| > 0)
    const double s_lo = std::max(c + std::min(v0, v1), c - std::fabs(A)) * (1.0 - 1e-12);
    const double s_hi = std::min(c + std::max(v0, v1), c + std::fabs(A)) * (1.0 + 1e-12);
    smin = std::min(smin, s_lo);
    smax = std::max(smax, s_hi);
    imax = std::max(imax, (1.0 / s_lo) * (1.0 + 1e-12));
    q = std::max(q, std::fabs(A * w) * std::min(1.0, r.acos_hi * (1.0 + 1e-12) + 1e-15) / (s_lo * s_lo));
  }
  out4[0] = smin;
  out4[1] = smax;
  out4[2] = imax;
  out4[3] = q * (1.0 + 1e-12);
}

}  // namespace svsdf_traj

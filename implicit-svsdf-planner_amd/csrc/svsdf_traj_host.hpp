// svsdf_traj_host.hpp -- the trajectory intake of every device entry point, on the host: the argument checks, the duration
// rule, the layer-1 time grid, the Bernstein velocity bound with its two users (the exact cull's table, svsdf_motion_bounds)
// and the piece-time mode.  upload_traj (svsdf_pipeline.hip) stages what these produce.  Plain C++
// with no HIP and no kernel header: a host compiler builds it alone (tests/cpp/traj_host.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <limits>
#include <vector>

#include "../../include/svsdf_c.h"

namespace svsdf_traj {

// What check_traj found: SVSDF_OK, or the code and a short reason; td = sum of T (Trajectory::getTotalDuration, TRJ:410-419).
struct TrajCheck { int code; const char *reason; double td; };

// The one order every entry reports a faulty trajectory in: N, the total duration, the piece durations, the coefficients.
// (forwardT, BEO:213-226, only produces positive durations and Trajectory asserts t_max > 0; the scan table needs one.)
inline TrajCheck check_traj(int N, const double *coeffs, const double *T) {
  if (N < 1 || N > SVSDF_MAX_PIECES) return {SVSDF_ERR_INVALID, "N out of range [1, 128]", 0.0};
  double td = 0.0;
  for (int i = 0; i < N; ++i) td += T[i];
  if (!std::isfinite(td)) return {SVSDF_ERR_NONFINITE, "non-finite duration", td};
  for (int i = 0; i < N; ++i)
    if (!(T[i] > 0.0)) return {SVSDF_ERR_INVALID, "piece durations must be positive", td};
  for (size_t i = 0; i < 18 * (size_t)N; ++i)
    if (!std::isfinite(coeffs[i])) return {SVSDF_ERR_NONFINITE, "non-finite trajectory input", td};
  return {SVSDF_OK, "", td};
}

// traj_duration as SweptVolumeManager::updateTraj keeps it (SWM:376-385): a total of 300 s or more leaves the previous one
// in force (the stale regime), except on the first trajectory.
inline void update_duration(double td, double &traj_duration, bool &have_duration) {
  if (td < 3 * 1e2 || !have_duration) { traj_duration = td; have_duration = true; }
}

// The layer-1 time grid, exactly the reference's accumulating loop (SWM:567).  Returns the count K; tk needs room for
// scan_times_room(dur) entries: t_k is k * 0.15 to a relative k * 2^-53, so K <= dur / 0.15 + 2 while that is below 2^20.
inline size_t scan_times_room(double dur) { return (size_t)(dur / 0.15) + 3; }
inline size_t scan_times(double dur, double *tk) {
  size_t k = 0;
  for (double t = 0.0; t <= dur; t += 0.15) tk[k++] = t;
  return k;
}

inline std::vector<double> prefix_sums(int N, const double *T) {
  std::vector<double> S(N + 1, 0.0);
  for (int i = 0; i < N; ++i) S[i + 1] = S[i] + T[i];
  return S;
}

// Bernstein coefficients of a polynomial given by its power coefficients a[0..n] on [0, 1]:
//   b_j = sum_{i <= j} C(j, i) / C(n, i) a_i     (the binomials are exact integers for n = 4 and n = 8)
template <int n>
void bernstein(const double *a, double *b) {
  double cn[n + 1];
  cn[0] = 1.0;
  for (int i = 0; i < n; ++i) cn[i + 1] = cn[i] * (n - i) / (i + 1);
  for (int j = 0; j <= n; ++j) {
    double bj = 0.0, cji = 1.0;
    for (int i = 0; i <= j; ++i) { bj += cji / cn[i] * a[i]; cji = cji * (j - i) / (i + 1); }
    b[j] = bj;
  }
}

// The core of both bounds: the velocity quartics of piece i (x, y, yaw) on the local interval [a, a + w], shifted and
// scaled to u in [0, 1] (pw: their power coefficients), and per axis the largest |Bernstein coefficient| -- the quartic
// lies in the convex hull of its Bernstein coefficients on the interval.  No rounding allowance: each caller adds its own.
inline void velocity_bernstein(int N, const double *coeffs, int i, double a, double w, double pw[3][5], double bmax[3]) {
  for (int d = 0; d < 3; ++d) {
    double *p = pw[d];   // velocity in s: p[k] = (k+1) c_{k+1}
    for (int k = 0; k < 5; ++k) p[k] = (k + 1) * coeffs[(size_t)d * 6 * N + 6 * i + k + 1];
    for (int j = 0; j < 4; ++j)          // Taylor shift s = a + s' (repeated synthetic division)
      for (int k = 3; k >= j; --k) p[k] += a * p[k + 1];
    double wp = 1.0;
    for (int k = 0; k < 5; ++k) { p[k] *= wp; wp *= w; }   // s' = w u, u in [0, 1]
    double bj[5];
    bernstein<4>(p, bj);
    bmax[d] = 0.0;
    for (int j = 0; j <= 4; ++j) bmax[d] = std::max(bmax[d], std::fabs(bj[j]));
  }
}

// Exact cull (k_solve, main points): a point is skipped when  min_c(|p - c_c| - rb_c - slack_c) > safety_hor.
// Chunk c holds the table times t_k0 .. t_k1 (`chunk` of them); every t of [t_k0 - h, t_k1 + h] lies within h of one of
// them (h = half the table spacing; the last chunk also covers (t_last, dur]), so |x(t) - x(t_k)| <= V_c * h with V_c a
// rigorous bound of the planar speed on that interval (velocity_bernstein).  Then sdf(t) >= |p - x(t)| - R_shape >=
// |p - c_c| - rb_c - V_c * h for every continuous t, whatever local minimum the reference's search returns, and
// smoothedL1 (BEO:316-340) is inactive.  rot[c] = W_c * h is the yaw-rate allowance of the value-based second cull
// (scan_layer1).  Only in the regular regime (td == dur: traj_duration not stale); otherwise every entry is infinite.
struct CullTable { double slack_max; bool ok; };   // slack_max: over the chunks' finite slack entries
inline CullTable cull_table(int N, const double *coeffs, const double *S, const double *tk, size_t K, double dur, double td,
                            size_t chunk, double *slack, double *rot) {
  CullTable out{0.0, (td == dur) && K >= 1};
  const size_t nch = (K + chunk - 1) / chunk;
  for (size_t c = 0; c < nch; ++c) {
    slack[c] = rot[c] = std::numeric_limits<double>::infinity();
    if (!out.ok) continue;
    const size_t k0 = c * chunk, k1 = std::min(k0 + chunk, K) - 1;
    const double h = (c + 1 == nch) ? std::max(0.0751, dur - tk[k1]) : 0.0751;
    const double ta = std::max(0.0, tk[k0] - h), tb = std::min(td, tk[k1] + h);
    double v2 = 0.0, wmax = 0.0;
    for (int i = 0; i < N; ++i) {
      const double a = std::max(ta, S[i]) - S[i], b = std::min(tb, S[i + 1]) - S[i];  // local times in piece i
      if (!(b >= a)) continue;
      double pw[3][5], bound[3];
      velocity_bernstein(N, coeffs, i, a, b - a, pw, bound);
      v2 = std::max(v2, std::hypot(bound[0], bound[1]));
      wmax = std::max(wmax, bound[2]);
    }
    const double sl = v2 * (1.0 + 1e-9) * h + 1e-9;
    if (std::isfinite(sl)) { slack[c] = sl; out.slack_max = std::max(out.slack_max, sl); }
    const double rl = wmax * (1.0 + 1e-9) * h + 1e-12;
    if (std::isfinite(rl)) rot[c] = rl;
  }
  return out;
}

// svsdf_motion_bounds: the same bound on [ta, tb] (clamped to [0, S[N]]), for the certified clearance.  The planar speed
// also has the degree-8 form vx^2 + vy^2, whose gap closes quadratically with the interval (the hypot of the two axes'
// maxima is first order only: the axes peak at different ends).  Every bound is rounded up by what the shift can have
// lost: `mag` bounds every intermediate of the shift, (k+1) |c_{k+1}| T^k summed.
inline void motion_bounds(int N, const double *coeffs, const double *S, double ta, double tb, double out2[2]) {
  const double td = S[N];
  ta = std::min(std::max(ta, 0.0), td);
  tb = std::min(std::max(tb, 0.0), td);
  double vmax = 0.0, wmax = 0.0;
  for (int i = 0; i < N; ++i) {
    const double a = std::max(ta, S[i]) - S[i], b = std::min(tb, S[i + 1]) - S[i];   // local times in piece i
    if (!(b >= a)) continue;
    const double Ti = S[i + 1] - S[i];
    double pw[3][5], bound[3], mag[3];
    velocity_bernstein(N, coeffs, i, a, b - a, pw, bound);
    for (int d = 0; d < 3; ++d) {
      mag[d] = 0.0;
      double tp = 1.0;
      for (int k = 0; k < 5; ++k) { mag[d] += std::fabs((k + 1) * coeffs[(size_t)d * 6 * N + 6 * i + k + 1]) * tp; tp *= Ti; }
      bound[d] += 1e-13 * mag[d];
    }
    double q[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bq[9];
    for (int k = 0; k < 5; ++k)
      for (int l = 0; l < 5; ++l) q[k + l] += pw[0][k] * pw[0][l] + pw[1][k] * pw[1][l];
    bernstein<8>(q, bq);
    double v2 = 0.0;
    for (int j = 0; j <= 8; ++j) v2 = std::max(v2, bq[j]);
    const double m2 = mag[0] + mag[1];
    const double v = std::min(std::hypot(bound[0], bound[1]), std::sqrt(v2 + 1e-12 * m2 * m2));
    vmax = std::max(vmax, v);
    wmax = std::max(wmax, bound[2]);
  }
  out2[0] = vmax * (1.0 + 1e-12);
  out2[1] = wmax * (1.0 + 1e-12);
}

// Piece-local time: the reference subtracts the durations one after the other from t (TRJ:498-516);
// t - (T_0 + ... + T_{i-1}) in one subtraction is the same number only when every operation involved is exact.  That is
// guaranteed when all durations are coarse dyadic numbers (multiples of 2^-20 below 2^20, e.g. the 2.5 s of every BASELINE
// config): then all partial sums and all differences with any t < 2^30 are exact in both forms.  Otherwise (an optimiser's
// durations are generic doubles) the faithful chain runs.  0: the single subtraction; 1, 2: the chain (2: a piece below 1e-6 s).
inline int piece_time_mode(int flags, int N, const double *T, double dur) {
  bool coarse = dur < 1073741824.0;
  double tmin = std::numeric_limits<double>::infinity();
  for (int i = 0; i < N; ++i) {
    const double v = std::ldexp(T[i], 20);
    coarse = coarse && T[i] < 1048576.0 && v == std::floor(v);
    tmin = std::min(tmin, T[i]);
  }
  int mode = (flags & SVSDF_FLAG_EXACT_PIECE_TIME) ? 1 : (flags & SVSDF_FLAG_FAST_PIECE_TIME) ? 0 : (coarse ? 0 : 1);
  if (mode == 1 && !(tmin >= 1e-6)) mode = 2;
  return mode;
}

}  // namespace svsdf_traj

// Host check of csrc/svsdf_traj_host.hpp, the trajectory intake of every device entry point.
//   cull_table      against the loop upload_traj carried before the header existed, written out literally here (memcmp);
//   motion_bounds   against values recorded from the library before the header existed (tests/golden/motion_bounds_parent.json,
//                   handed over as a text file of hex doubles by tests/test_traj_host.py), bit for bit;
//   piece_time_mode, scan_times, check_traj   on their tables.
// usage: traj_host <data file>.  Prints one line per case; exit code 1 on a mismatch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../implicit-svsdf-planner_amd/csrc/svsdf_traj_host.hpp"

using namespace svsdf_traj;

static int bad = 0;
static void fail(const char *what, int a = -1, int b = -1) {
  std::printf("MISMATCH %s (%d, %d)\n", what, a, b);
  ++bad;
}

constexpr size_t kChunk = 8;   // svsdf::kChunk

// upload_traj's cull loop as it stood (ctx->slack_max / ctx->cull_ok as references, the staging pointers as arguments)
static void literal_cull(int N, const double *coeffs, const double *T, const double *tk, size_t K, double dur, double td,
                         double *slack, double *rot, double &slack_max, bool &cull_ok) {
  const size_t nch = (K + kChunk - 1) / kChunk;
  slack_max = 0.0;
  cull_ok = (td == dur) && K >= 1;
  std::vector<double> S(N + 1, 0.0);
  for (int i = 0; i < N; ++i) S[i + 1] = S[i] + T[i];
  for (size_t c = 0; c < nch; ++c) {
    slack[c] = std::numeric_limits<double>::infinity();
    rot[c] = std::numeric_limits<double>::infinity();
    if (!cull_ok) continue;
    const size_t k0 = c * kChunk, k1 = std::min(k0 + kChunk, K) - 1;
    const double h = (c + 1 == nch) ? std::max(0.0751, dur - tk[k1]) : 0.0751;
    const double ta = std::max(0.0, tk[k0] - h), tb = std::min(td, tk[k1] + h);
    double v2 = 0.0, wmax = 0.0;
    for (int i = 0; i < N; ++i) {
      const double a = std::max(ta, S[i]) - S[i], b = std::min(tb, S[i + 1]) - S[i];  // local times in piece i
      if (!(b >= a)) continue;
      const double w = b - a;
      double bound[3] = {0.0, 0.0, 0.0};
      for (int d = 0; d < 3; ++d) {
        double p[5];  // velocity in s: p[k] = (k+1) c_{k+1}
        for (int k = 0; k < 5; ++k) p[k] = (k + 1) * coeffs[(size_t)d * 6 * N + 6 * i + k + 1];
        for (int j = 0; j < 4; ++j)          // Taylor shift s = a + s' (repeated synthetic division)
          for (int k = 3; k >= j; --k) p[k] += a * p[k + 1];
        double wp = 1.0;
        for (int k = 0; k < 5; ++k) { p[k] *= wp; wp *= w; }   // s' = w u, u in [0, 1]
        static const double binom4[5] = {1, 4, 6, 4, 1};
        for (int j = 0; j <= 4; ++j) {
          double bj = 0.0, cjq = 1.0;  // C(j, q)
          for (int q = 0; q <= j; ++q) { bj += cjq / binom4[q] * p[q]; cjq = cjq * (j - q) / (q + 1); }
          bound[d] = std::max(bound[d], std::fabs(bj));
        }
      }
      v2 = std::max(v2, std::hypot(bound[0], bound[1]));
      wmax = std::max(wmax, bound[2]);
    }
    const double sl = v2 * (1.0 + 1e-9) * h + 1e-9;
    if (std::isfinite(sl)) { slack[c] = sl; slack_max = std::max(slack_max, sl); }
    const double rl = wmax * (1.0 + 1e-9) * h + 1e-12;
    if (std::isfinite(rl)) rot[c] = rl;
  }
}

// the time grid as upload_traj built it: one loop to count, one to fill
static std::vector<double> literal_scan(double dur) {
  size_t K = 0;
  for (double t = 0.0; t <= dur; t += 0.15) ++K;
  std::vector<double> tk(K);
  size_t k = 0;
  for (double t = 0.0; t <= dur; t += 0.15) tk[k++] = t;
  return tk;
}

static std::vector<double> scan(double dur) {
  std::vector<double> tk(scan_times_room(dur));   // (exactly the room the header asks for: the sanitizer sees an overrun)
  tk.resize(scan_times(dur, tk.data()));
  return tk;
}

static void check_cull(int ti, int N, const std::vector<double> &coeffs, const std::vector<double> &T, double dur) {
  const std::vector<double> S = prefix_sums(N, T.data());
  const double td = S[N];
  const std::vector<double> tk = scan(dur);
  const size_t K = tk.size(), nch = (K + kChunk - 1) / kChunk;
  std::vector<double> s0(nch), r0(nch), s1(nch), r1(nch);
  double m0 = -1.0;
  bool ok0 = false;
  literal_cull(N, coeffs.data(), T.data(), tk.data(), K, dur, td, s0.data(), r0.data(), m0, ok0);
  const CullTable c = cull_table(N, coeffs.data(), S.data(), tk.data(), K, dur, td, kChunk, s1.data(), r1.data());
  if (std::memcmp(s0.data(), s1.data(), nch * sizeof(double))) fail("cull slack", ti);
  if (std::memcmp(r0.data(), r1.data(), nch * sizeof(double))) fail("cull rot", ti);
  if (std::memcmp(&m0, &c.slack_max, sizeof(double))) fail("cull slack_max", ti);
  if (ok0 != c.ok) fail("cull cull_ok", ti);
  size_t finite = 0;
  for (size_t i = 0; i < nch; ++i) finite += std::isfinite(s1[i]) && std::isfinite(r1[i]);
  std::printf("cull traj %d N %d K %zu chunks %zu ok %d tail %d finite %zu slack_max %a\n", ti, N, K, nch, (int)c.ok,
              (int)(dur - tk[K - 1] > 0.0751), finite, c.slack_max);
}

static void check_piece_time() {
  const double dyadic[5] = {2.5, 2.5, 0.75, 1.0, 3.25}, generic[5] = {2.5 * 1.1, 2.5 * 1.1, 0.7, 1.3, 2.9};
  const double tiny[5] = {2.5 * 1.1, 5e-7, 0.7, 1.3, 2.9};
  auto sum = [](const double *T) { double s = 0.0; for (int i = 0; i < 5; ++i) s += T[i]; return s; };
  struct { const char *name; int flags; const double *T; int want; } cases[] = {
      {"dyadic", 0, dyadic, 0},
      {"generic", 0, generic, 1},
      {"generic with a piece below 1e-6", 0, tiny, 2},
      {"dyadic, SVSDF_FLAG_EXACT_PIECE_TIME", SVSDF_FLAG_EXACT_PIECE_TIME, dyadic, 1},
      {"generic, SVSDF_FLAG_FAST_PIECE_TIME", SVSDF_FLAG_FAST_PIECE_TIME, generic, 0},
  };
  for (const auto &c : cases) {
    const int got = piece_time_mode(c.flags, 5, c.T, sum(c.T));
    if (got != c.want) fail("piece_time_mode", got, c.want);
    std::printf("piece_time %s: %d\n", c.name, got);
  }
}

static void check_scan() {
  for (double dur : {0.15, 12.5, 80.0}) {
    const std::vector<double> want = literal_scan(dur), got = scan(dur);
    if (got.size() != want.size() || std::memcmp(got.data(), want.data(), want.size() * sizeof(double))) fail("scan_times");
    std::printf("scan dur %g: K %zu\n", dur, got.size());
  }
}

static void check_checks() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const int N = 3;
  // which: 0 nothing, 1 T[1] = v, 2 coeffs[20] = v, 3 T = (-1, +inf, 1), 4 T[1] = -1 and coeffs[20] = NaN
  struct { const char *name; int N, which; double v; int want; } cases[] = {
      {"valid", N, 0, 0.0, SVSDF_OK},
      {"N = 0", 0, 0, 0.0, SVSDF_ERR_INVALID},
      {"N = 129", 129, 0, 0.0, SVSDF_ERR_INVALID},
      {"T = 0", N, 1, 0.0, SVSDF_ERR_INVALID},
      {"T < 0", N, 1, -1.0, SVSDF_ERR_INVALID},
      {"T NaN", N, 1, nan, SVSDF_ERR_NONFINITE},
      {"T +inf", N, 1, inf, SVSDF_ERR_NONFINITE},
      {"coefficient NaN", N, 2, nan, SVSDF_ERR_NONFINITE},
      {"coefficient inf", N, 2, inf, SVSDF_ERR_NONFINITE},
      {"T non-positive and T +inf", N, 3, 0.0, SVSDF_ERR_NONFINITE},
      {"T non-positive and coefficient NaN", N, 4, 0.0, SVSDF_ERR_INVALID},
  };
  for (const auto &c : cases) {
    std::vector<double> coeffs(18 * 129, 0.25), T(129, 1.5);
    if (c.which == 1) T[1] = c.v;
    if (c.which == 2) coeffs[20] = c.v;
    if (c.which == 3) { T[0] = -1.0; T[1] = inf; }
    if (c.which == 4) { T[1] = -1.0; coeffs[20] = nan; }
    const TrajCheck r = check_traj(c.N, coeffs.data(), T.data());
    if (r.code != c.want) fail("check_traj", r.code, c.want);
    if ((r.code == SVSDF_OK) != (r.reason[0] == 0)) fail("check_traj reason");
    if (r.code == SVSDF_OK && r.td != 4.5) fail("check_traj td");
    std::printf("check %s: %d %s\n", c.name, r.code, r.reason);
  }
  // the duration rule: the first trajectory always, later ones below 300 s
  double dur = 0.0;
  bool have = false;
  update_duration(400.0, dur, have);
  if (!(have && dur == 400.0)) fail("update_duration first");
  update_duration(300.0, dur, have);
  if (dur != 400.0) fail("update_duration stale");
  update_duration(299.5, dur, have);
  if (dur != 299.5) fail("update_duration regular");
  std::printf("duration rule: %g\n", dur);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  auto next = [&](double &v) {   // one hex (or decimal) double
    char tok[64];
    if (std::fscanf(f, "%63s", tok) != 1) return false;
    v = std::strtod(tok, nullptr);
    return true;
  };
  double v = 0.0;
  int ti = 0;
  while (next(v)) {   // per trajectory: N | T | coeffs | stale dur | n | n x (ta tb V W)
    const int N = (int)v;
    std::vector<double> T(N), coeffs(18 * (size_t)N);
    for (double &x : T) if (!next(x)) return 2;
    for (double &x : coeffs) if (!next(x)) return 2;
    double stale = 0.0, n = 0.0;
    if (!next(stale) || !next(n)) return 2;
    if (check_traj(N, coeffs.data(), T.data()).code) fail("golden trajectory refused", ti);
    const std::vector<double> S = prefix_sums(N, T.data());
    int same = 0;
    for (int k = 0; k < (int)n; ++k) {
      double ta, tb, want[2], got[2];
      if (!next(ta) || !next(tb) || !next(want[0]) || !next(want[1])) return 2;
      motion_bounds(N, coeffs.data(), S.data(), ta, tb, got);
      if (std::memcmp(got, want, sizeof(got))) {
        std::printf("MISMATCH motion_bounds traj %d [%a, %a]: %a %a, recorded %a %a\n", ti, ta, tb, got[0], got[1], want[0], want[1]);
        ++bad;
      } else ++same;
    }
    std::printf("bounds traj %d N %d: %d of %d intervals equal\n", ti, N, same, (int)n);
    check_cull(ti, N, coeffs, T, S[N]);
    if (stale > 0.0) check_cull(ti, N, coeffs, T, stale);   // td != dur: every entry infinite, cull_ok false
    ++ti;
  }
  std::fclose(f);
  check_piece_time();
  check_scan();
  check_checks();
  std::printf(bad ? "%d mismatches\n" : "all checks passed\n", bad);
  return bad ? 1 : 0;
}

// scale_host.cpp -- csrc/svsdf_scale_host.hpp compiled for the host alone (tests/test_scale_bounds_cpu.py builds this with
// -fsanitize=address,undefined and runs it once): check_scale's fault table, the special values, and scale_bounds against
// dense sampling of the schedule on random (schedule, interval) pairs from a fixed linear congruential sequence.
#include <cmath>
#include <cstdio>
#include <cstdint>

#include "../../implicit-svsdf-planner_amd/csrc/svsdf_scale_host.hpp"

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static double uniform(double lo, double hi) {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return lo + (hi - lo) * (double)(g_state >> 11) / 9007199254740992.0;
}

static int fails = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++fails; } \
  } while (0)

static svsdf_scale example() {
  svsdf_scale s{};
  s.struct_size = (int)sizeof(svsdf_scale);
  s.enabled = 1;
  s.c[0] = 0.8; s.amp[0] = 0.6; s.omega[0] = 1.5; s.phase[0] = -1.0;
  s.c[1] = 0.8; s.amp[1] = 0.4; s.omega[1] = 1.8; s.phase[1] = 0.0;
  return s;
}

int main() {
  using namespace svsdf_traj;
  double o[4];
  // special values
  scale_bounds(nullptr, 0.0, 5.0, o);
  CHECK(o[0] == 1.0 && o[1] == 1.0 && o[2] == 1.0 && o[3] == 0.0);
  svsdf_scale s = example();
  s.enabled = 0;
  scale_bounds(&s, 0.0, 5.0, o);
  CHECK(o[0] == 1.0 && o[1] == 1.0 && o[2] == 1.0 && o[3] == 0.0);
  s = example();
  s.c[0] = s.c[1] = 1.0; s.amp[0] = s.amp[1] = 0.0;
  scale_bounds(&s, 1.0, 9.0, o);
  CHECK(o[0] == 1.0 && o[1] == 1.0 && o[2] == 1.0 && o[3] == 0.0);
  // check_scale
  s = example();
  CHECK(check_scale(nullptr).code == SVSDF_OK && check_scale(&s).code == SVSDF_OK);
  s.struct_size = 8;
  CHECK(check_scale(&s).code == SVSDF_ERR_INVALID);
  s = example(); s.omega[1] = std::nan("");
  CHECK(check_scale(&s).code == SVSDF_ERR_INVALID);
  s = example(); s.phase[0] = INFINITY;
  CHECK(check_scale(&s).code == SVSDF_ERR_INVALID);
  s = example(); s.amp[0] = -0.8;
  CHECK(check_scale(&s).code == SVSDF_ERR_INVALID);
  s.enabled = 0;
  CHECK(check_scale(&s).code == SVSDF_OK);   // (a disabled schedule is not validated beyond its size)
  // domination on 400 random pairs, 501 samples each
  int pairs = 0;
  for (int i = 0; i < 400; ++i) {
    s = example();
    for (int a = 0; a < 2; ++a) {
      s.c[a] = uniform(0.3, 2.0);
      s.amp[a] = s.c[a] * uniform(-0.999, 0.999);
      s.omega[a] = (i % 7 == 0) ? 0.0 : uniform(-6.0, 6.0);
      s.phase[a] = uniform(-10.0, 10.0);
    }
    const double ta = uniform(0.0, 300.0), tb = ta + std::pow(10.0, uniform(-9.0, 1.3));
    scale_bounds(&s, ta, tb, o);
    bool ok = o[0] > 0.0;
    for (int k = 0; k <= 500 && ok; ++k) {
      const double t = ta + (tb - ta) * k / 500.0;
      for (int a = 0; a < 2; ++a) {
        const double arg = s.omega[a] * t + s.phase[a], v = s.c[a] + std::sin(arg) * s.amp[a];
        const double q = std::fabs(s.amp[a] * s.omega[a] * std::cos(arg)) / (v * v);
        ok = ok && v >= o[0] && v <= o[1] && 1.0 / v <= o[2] && q <= o[3];
      }
    }
    CHECK(ok);
    ++pairs;
  }
  std::printf("pairs %d\n", pairs);
  if (fails) return 1;
  std::printf("all checks passed\n");
  return 0;
}

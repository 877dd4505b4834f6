// The order-preserving key of svsdf_point_clearance's per-point minima (csrc/svsdf_ordkey.hpp), compiled for the host alone:
// key order equals < on random pairs of doubles and on the special values, -0.0 sorts below +0.0, and key -> double is exact.
// Built and run by tests/test_point_clearance_cpu.py with the address and undefined-behaviour sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../implicit-svsdf-planner_amd/csrc/svsdf_ordkey.hpp"

using svsdf::ord_key;
using svsdf::ord_unkey;

static uint64_t bits_of(double x) { uint64_t u; std::memcpy(&u, &x, sizeof u); return u; }
static double from_bits(uint64_t u) { double x; std::memcpy(&x, &u, sizeof x); return x; }

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t next_u64() {   // splitmix64
  uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// a double that is not a NaN: any bit pattern (every exponent, both signs, denormals, infinities), or a value near +-1
static double next_double() {
  for (;;) {
    const uint64_t u = next_u64();
    if (u & 1ull) return ((double)(int64_t)(next_u64() >> 11) / 9007199254740992.0 - 0.5) * 4.0;
    const double x = from_bits(u);
    if (x == x) return x;
  }
}

static long g_bad = 0;
static void check_pair(double a, double b) {
  const uint64_t ka = ord_key(a), kb = ord_key(b);
  bool ok = true;
  if (a < b) ok = ka < kb;
  else if (b < a) ok = kb < ka;
  else if (bits_of(a) == bits_of(b)) ok = ka == kb;
  else ok = std::signbit(a) ? ka < kb : kb < ka;   // the two zeros: -0.0 below +0.0
  if (!ok && g_bad++ < 10) std::printf("BAD pair %a %a keys %016llx %016llx\n", a, b, (unsigned long long)ka, (unsigned long long)kb);
}
static void check_round_trip(double a) {
  if (bits_of(ord_unkey(ord_key(a))) != bits_of(a) && g_bad++ < 10) std::printf("BAD round trip %a\n", a);
}

int main() {
  const long n = 1000000;
  for (long i = 0; i < n; ++i) {
    const double a = next_double(), b = next_double();
    check_pair(a, b);
    check_round_trip(a);
    check_round_trip(b);
  }
  std::printf("random pairs %ld\n", n);

  const double inf = std::numeric_limits<double>::infinity(), dmin = std::numeric_limits<double>::denorm_min(),
               nmin = std::numeric_limits<double>::min(), big = std::numeric_limits<double>::max();
  std::vector<double> sp = {-inf, -big, -1.0, -nmin, -dmin, -0.0, 0.0, dmin, nmin, 1.0, big, inf};
  for (double x : {-big, -1.0, -nmin, -2.0 * dmin, 1e-3, 1.0, 0.7, big, -0.7}) {   // adjacent ulps around these
    sp.push_back(std::nextafter(x, -inf));
    sp.push_back(x);
    sp.push_back(std::nextafter(x, inf));
  }
  for (double a : sp) {
    check_round_trip(a);
    for (double b : sp) check_pair(a, b);
  }
  std::printf("specials %zu\n", sp.size());
  // strictly increasing along the ordered prefix, both zeros included
  for (size_t i = 0; i + 1 < 12; ++i)
    if (!(ord_key(sp[i]) < ord_key(sp[i + 1])) && g_bad++ < 10) std::printf("BAD order at %zu\n", i);
  if (ord_key(inf) != svsdf::kOrdKeyPosInf) { ++g_bad; std::printf("BAD kOrdKeyPosInf\n"); }
  // a NaN round-trips too (callers keep NaNs out of the minima)
  check_round_trip(std::numeric_limits<double>::quiet_NaN());
  check_round_trip(-std::numeric_limits<double>::quiet_NaN());
  if (g_bad) { std::printf("%ld failures\n", g_bad); return 1; }
  std::printf("ordkey ok\n");
  return 0;
}

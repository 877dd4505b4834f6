// svsdf_ordkey.hpp -- an order-preserving map of doubles onto unsigned 64-bit integers, so that a minimum over doubles can be
// taken with an integer atomicMin (svsdf_point_clearance: the per-point state, svsdf_clearance.hpp).  A minimum does not
// depend on the order its operands arrive in, so results stay bit-reproducible without a floating-point atomic.
//   ord_key(a) < ord_key(b)  <=>  a < b     for all finite doubles and both infinities, except that -0.0 sorts below +0.0
//   ord_unkey(ord_key(a)) has a's bits      for every double, NaNs included
// A NaN with the sign bit clear sorts above +infinity, one with the sign bit set below -infinity: callers keep NaNs out.
// Free of HIP: a host compiler takes this header as it is (tests/cpp/ordkey_host.cpp).
#pragma once

#if defined(__HIPCC__)
#define SVSDF_ORDKEY_FN __host__ __device__ inline
#else
#define SVSDF_ORDKEY_FN inline
#endif

namespace svsdf {

constexpr unsigned long long kOrdSign = 0x8000000000000000ull;
constexpr unsigned long long kOrdKeyPosInf = 0xfff0000000000000ull;   // ord_key(+infinity)

SVSDF_ORDKEY_FN unsigned long long ord_key(double x) {
  unsigned long long u;
  __builtin_memcpy(&u, &x, sizeof u);
  return (u & kOrdSign) ? ~u : (u | kOrdSign);   // negative: larger magnitude -> smaller key; non-negative: above every negative
}
SVSDF_ORDKEY_FN double ord_unkey(unsigned long long k) {
  const unsigned long long u = (k & kOrdSign) ? (k & ~kOrdSign) : ~k;
  double x;
  __builtin_memcpy(&x, &u, sizeof x);
  return x;
}

}  // namespace svsdf

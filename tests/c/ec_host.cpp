/* The field and point arithmetic of bftkv_amd/csrc/ec_field.h compiled for the CPU (the same text the threshold-ECDSA kernels
 * compile for the GPU), so that tests/test_ec_reference.py can check it against the Python restatement of Go's generic curve
 * code in the CPU suite.  Test infrastructure only.
 *
 * ech_op(curve, fbytes, op, in, out): curve = P || N || B || Gx || Gy (fbytes each, big-endian); numbers in and out are
 * big-endian, fbytes each, plain (not Montgomery); points are affine with (0, 0) for infinity.
 *   0 a b -> a b mod p      1 a -> a^2 mod p      2 a -> a^-1 mod p (0 -> 0)      3 a b -> a b mod n
 *   4 P Q -> P + Q, then one byte: pt_add's case     5 P -> 2P     6 P k -> k P     7 x y -> 1 if Unmarshal's checks pass */
#include <stdint.h>
#include <string.h>
#include "../../bftkv_amd/csrc/ec_field.h"

namespace {

template <int L>
void to_jac(ecf::Jac<L>& P, const uint8_t* in, uint32_t f, const ecf::Curve<L>& C) {
  uint32_t x[L], y[L];
  ecf::fe_from_be<L>(x, in, f);
  ecf::fe_from_be<L>(y, in + f, f);
  if (ecf::fe_is_zero<L>(x) && ecf::fe_is_zero<L>(y)) { ecf::pt_set_inf<L>(P); return; }
  ecf::fp_mul<L>(P.x, x, C.rr_p, C);
  ecf::fp_mul<L>(P.y, y, C.rr_p, C);
  ecf::fe_copy<L>(P.z, C.one);
}

template <int L>
void from_jac(uint8_t* out, const ecf::Jac<L>& P, uint32_t f, const ecf::Curve<L>& C) {
  uint32_t x[L], y[L];
  ecf::pt_affine<L>(x, y, P, C);
  ecf::fe_to_be<L>(out, f, x);
  ecf::fe_to_be<L>(out + f, f, y);
}

template <int L>
int run(const uint8_t* curve, uint32_t f, int op, const uint8_t* in, uint8_t* out) {
  ecf::Curve<L> C;
  ecf::curve_setup<L>(C, curve, f);
  uint32_t a[L], b[L], am[L], bm[L], r[L], one[L];
  ecf::fe_zero<L>(one);
  one[0] = 1;
  ecf::Jac<L> P, Q;
  switch (op) {
    case 0: case 1: case 2:
      ecf::fe_from_be<L>(a, in, f);
      ecf::fe_from_be<L>(b, op == 0 ? in + f : in, f);
      ecf::fp_mul<L>(am, a, C.rr_p, C);
      ecf::fp_mul<L>(bm, b, C.rr_p, C);
      if (op == 2) ecf::fp_inv<L>(r, am, C);
      else ecf::fp_mul<L>(r, am, bm, C);
      ecf::fp_mul<L>(r, r, one, C);
      ecf::fe_to_be<L>(out, f, r);
      return 0;
    case 3:
      ecf::fe_from_be<L>(a, in, f);
      ecf::fe_from_be<L>(b, in + f, f);
      ecf::fn_mul<L>(r, a, b, C);
      ecf::fe_to_be<L>(out, f, r);
      return 0;
    case 4: {
      to_jac<L>(P, in, f, C);
      to_jac<L>(Q, in + 2 * f, f, C);
      const int code = ecf::pt_add<L>(P, P, Q, C);
      from_jac<L>(out, P, f, C);
      out[2 * f] = (uint8_t)code;
      return 0;
    }
    case 5:
      to_jac<L>(P, in, f, C);
      ecf::pt_dbl<L>(P, P, C);
      from_jac<L>(out, P, f, C);
      return 0;
    case 6:
      to_jac<L>(P, in, f, C);
      ecf::fe_from_be<L>(a, in + 2 * f, f);
      ecf::pt_mul<L>(Q, P, a, C);
      from_jac<L>(out, Q, f, C);
      return 0;
    case 7:
      ecf::fe_from_be<L>(a, in, f);
      ecf::fe_from_be<L>(b, in + f, f);
      out[0] = ecf::pt_check<L>(am, bm, a, b, C) ? 1 : 0;
      return 0;
  }
  return -1;
}

}  // namespace

extern "C" int ech_op(const uint8_t* curve, uint32_t fbytes, int op, const uint8_t* in, uint8_t* out) {
  switch (fbytes) {
    case 28: return run<7>(curve, fbytes, op, in, out);
    case 32: return run<8>(curve, fbytes, op, in, out);
    case 48: return run<12>(curve, fbytes, op, in, out);
    case 66: return run<17>(curve, fbytes, op, in, out);
  }
  return -1;
}

/* The ECDSA-verification pieces of bftkv_amd/csrc/ec_field.h compiled for the CPU (the same text the k_ecv_* kernels compile
 * for the GPU), so that tests/test_ecdsa_verify_reference.py can check them against the Python restatement in the CPU suite.
 * Test infrastructure only.
 *
 * evh_op(curve, fbytes, bits, op, arg, in, in_len, out): curve = P || N || B || Gx || Gy (fbytes each, big-endian); numbers are
 * big-endian, fbytes each, plain; affine points use (0, 0) for infinity.  A Jacobian operand is given as affine x, y and a
 * scale z: (x z^2, y z^3, z), z = 0 for infinity.
 *   0  x y z qx qy       -> P + Q by pt_add_affine as affine x y, then one byte: the case code
 *   1  k      (arg = w)  -> k G by fb_mul over the table of window width w, affine x y
 *   2  (arg = w | i << 8 | j << 20)  -> entry j of window i of that table, affine x y (plain)
 *   3  digest (in_len bytes)         -> hashToInt(digest) mod N
 *   4  x y z r           -> one byte: x_matches_r
 *   5  key (1 + 2 fbytes) sig (2 fbytes) w digest (the rest; arg = w of the table) -> valid, status: the kernels' sequence of the
 *      pieces above (k_ecv_prep, k_ecv_base, k_ecv_key of ec_kernels.hip) with w = s^-1 mod N handed in (the device takes it from
 *      k_modinv); status 0 = decided, 2 = fenced */
#include <stdint.h>
#include <string.h>
#include <map>
#include <vector>
#include "../../bftkv_amd/csrc/ec_field.h"

namespace {

template <int L>
void to_jac(ecf::Jac<L>& P, const uint8_t* in, uint32_t f, const ecf::Curve<L>& C) {
  uint32_t x[L], y[L], z[L], z2[L];
  ecf::fe_from_be<L>(x, in, f);
  ecf::fe_from_be<L>(y, in + f, f);
  ecf::fe_from_be<L>(z, in + 2 * f, f);
  if (ecf::fe_is_zero<L>(z)) { ecf::pt_set_inf<L>(P); return; }
  ecf::fp_mul<L>(x, x, C.rr_p, C);
  ecf::fp_mul<L>(y, y, C.rr_p, C);
  ecf::fp_mul<L>(P.z, z, C.rr_p, C);
  ecf::fp_sqr<L>(z2, P.z, C);
  ecf::fp_mul<L>(P.x, x, z2, C);
  ecf::fp_mul<L>(z2, z2, P.z, C);
  ecf::fp_mul<L>(P.y, y, z2, C);
}

template <int L>
void from_jac(uint8_t* out, const ecf::Jac<L>& P, uint32_t f, const ecf::Curve<L>& C) {
  uint32_t x[L], y[L];
  ecf::pt_affine<L>(x, y, P, C);
  ecf::fe_to_be<L>(out, f, x);
  ecf::fe_to_be<L>(out + f, f, y);
}

template <int L>
const std::vector<uint32_t>& table(const ecf::Curve<L>& C, uint32_t w) {
  static std::map<uint32_t, std::vector<uint32_t>> cache;
  auto it = cache.find(w);
  if (it == cache.end()) {
    const uint32_t nwin = ecf::fb_windows(C.fbytes, w);
    std::vector<uint32_t> t(ecf::fb_table_words<L>(w, nwin));
    ecf::fb_table_build<L>(t.data(), w, nwin, C);
    it = cache.emplace(w, std::move(t)).first;
  }
  return it->second;
}

template <int L>
int run(const uint8_t* curve, uint32_t f, uint32_t bits, int op, uint32_t arg, const uint8_t* in, uint32_t in_len, uint8_t* out) {
  ecf::Curve<L> C;
  ecf::curve_setup<L>(C, curve, f);
  uint32_t a[L], b[L], one[L];
  ecf::fe_zero<L>(one);
  one[0] = 1;
  ecf::Jac<L> P;
  switch (op) {
    case 0: {
      to_jac<L>(P, in, f, C);
      ecf::fe_from_be<L>(a, in + 3 * f, f);
      ecf::fe_from_be<L>(b, in + 4 * f, f);
      ecf::fp_mul<L>(a, a, C.rr_p, C);
      ecf::fp_mul<L>(b, b, C.rr_p, C);
      const int code = ecf::pt_add_affine<L>(P, P, a, b, C);
      from_jac<L>(out, P, f, C);
      out[2 * f] = (uint8_t)code;
      return 0;
    }
    case 1: {
      if (arg < 2 || arg > 8) return -1;
      ecf::fe_from_be<L>(a, in, f);
      ecf::fb_mul<L>(P, table<L>(C, arg).data(), arg, ecf::fb_windows(f, arg), a, C);
      from_jac<L>(out, P, f, C);
      return 0;
    }
    case 2: {
      const uint32_t w = arg & 0xFF, i = (arg >> 8) & 0xFFF, j = arg >> 20;
      if (w < 2 || w > 8 || i >= ecf::fb_windows(f, w) || j == 0 || j >= (1u << w)) return -1;
      const uint32_t* e = table<L>(C, w).data() + (((size_t)i * 2 * L) << w) + j;
      for (int k = 0; k < L; ++k) { a[k] = e[(size_t)k << w]; b[k] = e[(size_t)(L + k) << w]; }
      ecf::fp_mul<L>(a, a, one, C);
      ecf::fp_mul<L>(b, b, one, C);
      ecf::fe_to_be<L>(out, f, a);
      ecf::fe_to_be<L>(out + f, f, b);
      return 0;
    }
    case 3:
      ecf::hash_to_int<L>(a, in, in_len, bits, C);
      ecf::fe_to_be<L>(out, f, a);
      return 0;
    case 4:
      to_jac<L>(P, in, f, C);
      ecf::fe_from_be<L>(a, in + 3 * f, f);
      out[0] = ecf::x_matches_r<L>(P, a, C) ? 1 : 0;
      return 0;
    case 5: {
      const uint8_t *kb = in, *sig = in + 1 + 2 * f, *wb = sig + 2 * f, *dg = wb + f;
      if (in_len <= 1 + 5 * f) return -1;
      uint32_t r[L], s[L], e[L], w[L], u1[L], u2[L];
      ecf::Jac<L> Q, A, B;
      out[0] = 0;
      out[1] = 0;
      ecf::fe_from_be<L>(a, kb + 1, f);
      ecf::fe_from_be<L>(b, kb + 1 + f, f);
      if (kb[0] != 4 || !ecf::pt_check<L>(Q.x, Q.y, a, b, C)) { out[1] = 2; return 0; }
      ecf::fe_copy<L>(Q.z, C.one);
      ecf::fe_from_be<L>(r, sig, f);
      ecf::fe_from_be<L>(s, sig + f, f);
      if (ecf::fe_is_zero<L>(r) || ecf::fe_is_zero<L>(s) || !ecf::fe_lt<L>(r, C.n) || !ecf::fe_lt<L>(s, C.n)) return 0;
      ecf::hash_to_int<L>(e, dg, in_len - (1 + 5 * f), bits, C);
      if (ecf::fe_is_zero<L>(e)) { out[1] = 2; return 0; }
      ecf::fe_from_be<L>(w, wb, f);
      ecf::fn_mul<L>(u1, e, w, C);
      ecf::fn_mul<L>(u2, r, w, C);
      ecf::fb_mul<L>(B, table<L>(C, arg).data(), arg, ecf::fb_windows(f, arg), u1, C);
      ecf::pt_mul<L>(A, Q, u2, C);
      const int code = ecf::pt_add<L>(A, B, A, C);
      if (code == ecf::EC_ADD_EQUAL) out[1] = 2;
      else if (code == ecf::EC_ADD_GENERAL) out[0] = ecf::x_matches_r<L>(A, r, C) ? 1 : 0;
      return 0;
    }
  }
  return -1;
}

}  // namespace

extern "C" int evh_op(const uint8_t* curve, uint32_t fbytes, uint32_t bits, int op, uint32_t arg, const uint8_t* in, uint32_t in_len, uint8_t* out) {
  switch (fbytes) {
    case 28: return run<7>(curve, fbytes, bits, op, arg, in, in_len, out);
    case 32: return run<8>(curve, fbytes, bits, op, arg, in, in_len, out);
    case 48: return run<12>(curve, fbytes, bits, op, arg, in, in_len, out);
    case 66: return run<17>(curve, fbytes, bits, op, arg, in, in_len, out);
  }
  return -1;
}

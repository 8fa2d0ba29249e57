/* The key-set pieces of bftkv_amd/csrc/ec_field.h compiled for the CPU: fb_table_build over an arbitrary base point (the oracle
 * of the device build, k_ec_keytab_build), fb_mul over such a table, and the verification chain in the order of k_ecv_prep /
 * k_ecv_base / k_ecv_key_tab.  tests/test_ecdsa_keyset_reference.py checks them against the Python restatement in the CPU suite;
 * tests/test_gpu_ecdsa_keyset.py compares the device-built tables with ekh_table's word for word.  Test infrastructure only.
 *
 * curve = P || N || B || Gx || Gy (fbytes each, big-endian); numbers are big-endian, fbytes each, plain; an affine point is
 * x || y with (0, 0) for infinity.  Every function returns 0, or -1 for arguments it does not take. */
#include <stdint.h>
#include <string.h>
#include <map>
#include <string>
#include <vector>
#include "../../bftkv_amd/csrc/ec_field.h"

namespace {

/* the table of `base` (x || y, checked by pt_check) at width w, or -- base NULL -- of G through the overload that takes no base */
template <int L>
const std::vector<uint32_t>* table(const ecf::Curve<L>& C, uint32_t w, const uint8_t* base) {
  static std::map<std::string, std::vector<uint32_t>> cache;
  const uint32_t f = C.fbytes;
  std::string key(1, (char)w);
  if (base) key.append((const char*)base, 2 * (size_t)f);
  auto it = cache.find(key);
  if (it == cache.end()) {
    const uint32_t nwin = ecf::fb_windows(f, w);
    std::vector<uint32_t> t(ecf::fb_table_words<L>(w, nwin));
    if (base) {
      uint32_t x[L], y[L], xm[L], ym[L];
      ecf::fe_from_be<L>(x, base, f);
      ecf::fe_from_be<L>(y, base + f, f);
      if (!ecf::pt_check<L>(xm, ym, x, y, C)) return nullptr;
      ecf::fb_table_build<L>(t.data(), w, nwin, xm, ym, C);
    } else {
      ecf::fb_table_build<L>(t.data(), w, nwin, C);
    }
    it = cache.emplace(std::move(key), std::move(t)).first;
  }
  return &it->second;
}

template <int L>
void from_jac(uint8_t* out, const ecf::Jac<L>& P, uint32_t f, const ecf::Curve<L>& C) {
  uint32_t x[L], y[L];
  ecf::pt_affine<L>(x, y, P, C);
  ecf::fe_to_be<L>(out, f, x);
  ecf::fe_to_be<L>(out + f, f, y);
}

template <int L>
int run_table(const uint8_t* curve, uint32_t f, uint32_t w, const uint8_t* base, uint32_t* words, uint64_t cap) {
  ecf::Curve<L> C;
  ecf::curve_setup<L>(C, curve, f);
  const std::vector<uint32_t>* t = table<L>(C, w, base);
  if (!t || cap < t->size()) return -1;
  memcpy(words, t->data(), t->size() * 4);
  return 0;
}

template <int L>
int run_mul(const uint8_t* curve, uint32_t f, uint32_t w, const uint8_t* base, const uint8_t* k, uint8_t* out) {
  ecf::Curve<L> C;
  ecf::curve_setup<L>(C, curve, f);
  const std::vector<uint32_t>* t = table<L>(C, w, base);
  if (!t) return -1;
  uint32_t kw[L];
  ecf::Jac<L> P;
  ecf::fe_from_be<L>(kw, k, f);
  ecf::fb_mul<L>(P, t->data(), w, ecf::fb_windows(f, w), kw, C);
  from_jac<L>(out, P, f, C);
  return 0;
}

/* out[0] = valid, out[1] = status (0 decided, 2 fenced); winv = s^-1 mod N (the device takes it from k_modinv) */
template <int L>
int run_verify(const uint8_t* curve, uint32_t f, uint32_t bits, uint32_t w, const uint8_t* kb, const uint8_t* sig, const uint8_t* winv,
               const uint8_t* dg, uint32_t dlen, uint8_t* out) {
  ecf::Curve<L> C;
  ecf::curve_setup<L>(C, curve, f);
  const uint32_t nwin = ecf::fb_windows(f, w);
  out[0] = 0;
  out[1] = 0;
  /* registration: the refusal flag, or the key's table */
  uint32_t a[L], b[L], xm[L], ym[L];
  ecf::fe_from_be<L>(a, kb + 1, f);
  ecf::fe_from_be<L>(b, kb + 1 + f, f);
  const bool refused = kb[0] != 4 || !ecf::pt_check<L>(xm, ym, a, b, C);
  /* k_ecv_prep */
  uint32_t r[L], s[L], e[L], wv[L], u1[L], u2[L];
  ecf::fe_from_be<L>(r, sig, f);
  ecf::fe_from_be<L>(s, sig + f, f);
  ecf::hash_to_int<L>(e, dg, dlen, bits, C);
  int fl = 0;
  if (ecf::fe_is_zero<L>(r) || ecf::fe_is_zero<L>(s) || !ecf::fe_lt<L>(r, C.n) || !ecf::fe_lt<L>(s, C.n)) fl = 1;
  else if (ecf::fe_is_zero<L>(e)) fl = 2;
  /* k_ecv_base */
  ecf::Jac<L> B, A;
  if (!fl) {
    ecf::fe_from_be<L>(wv, winv, f);
    ecf::fn_mul<L>(u2, r, wv, C);
    ecf::fn_mul<L>(u1, e, wv, C);
    ecf::fb_mul<L>(B, table<L>(C, w, nullptr)->data(), w, nwin, u1, C);
  }
  /* k_ecv_key_tab */
  if (refused) { out[1] = 2; return 0; }
  if (fl == 2) { out[1] = 2; return 0; }
  if (fl) return 0;
  ecf::fb_mul<L>(A, table<L>(C, w, kb + 1)->data(), w, nwin, u2, C);
  const int code = ecf::pt_add<L>(A, B, A, C);
  if (code == ecf::EC_ADD_EQUAL) out[1] = 2;
  else if (code == ecf::EC_ADD_GENERAL) out[0] = ecf::x_matches_r<L>(A, r, C) ? 1 : 0;
  return 0;
}

}  // namespace

#define EKH_DISPATCH(fn, ...)                    \
  switch (fbytes) {                              \
    case 28: return fn<7>(__VA_ARGS__);          \
    case 32: return fn<8>(__VA_ARGS__);          \
    case 48: return fn<12>(__VA_ARGS__);         \
    case 66: return fn<17>(__VA_ARGS__);         \
  }                                              \
  return -1

/* words (cap of them) <- the table of base (x || y; NULL: G through the overload without a base point) at width w */
extern "C" int ekh_table(const uint8_t* curve, uint32_t fbytes, uint32_t w, const uint8_t* base, uint32_t* words, uint64_t cap) {
  if (w < 2 || w > 8) return -1;
  EKH_DISPATCH(run_table, curve, fbytes, w, base, words, cap);
}
/* out (x || y) <- k base by fb_mul over that table */
extern "C" int ekh_mul(const uint8_t* curve, uint32_t fbytes, uint32_t w, const uint8_t* base, const uint8_t* k, uint8_t* out) {
  if (w < 2 || w > 8) return -1;
  EKH_DISPATCH(run_mul, curve, fbytes, w, base, k, out);
}
extern "C" int ekh_verify(const uint8_t* curve, uint32_t fbytes, uint32_t bits, uint32_t w, const uint8_t* key, const uint8_t* sig,
                          const uint8_t* winv, const uint8_t* digest, uint32_t dlen, uint8_t* out) {
  if (w < 2 || w > 8) return -1;
  EKH_DISPATCH(run_verify, curve, fbytes, bits, w, key, sig, winv, digest, dlen, out);
}

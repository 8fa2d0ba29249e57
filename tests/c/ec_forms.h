/* One operation table over bftkv_amd/csrc/ec_field.h for tests/c/ec_forms_host.cpp (g++, the CPU suite) and tests/c/ec_forms.hip
 * (gfx950, one thread per record).  Every function takes one record of raw 32-bit words and writes one row of raw words: field
 * elements exactly as fe_mul takes them (Montgomery form where the header says so, L little-endian words), points as 3 L words
 * X, Y, Z.  Nothing is converted on the way in: choosing the words that reach the arithmetic is the point (tests/ec_form_cases.py).
 * Test infrastructure only.
 *
 * family          record in                                      row out
 *  0 FE           sub, a[L], b[L]                                r[L]        sub = op | mod << 4; mod 0: p, 1: n;
 *                                                                            op 0 fe_add  1 fe_sub  2 fe_mul  3 fe_mul(a, a, b)  4 fe_mul(b, a, b)
 *  1 INV          a[L]                                           r[L]        fp_inv
 *  2 FN           a[L], b[L] plain                               r[L] plain  fn_mul
 *  3 DBL          P[3L]                                          R[3L]       pt_dbl(P, P)
 *  4 ADD          form, P[3L], Q[3L]                             R[3L], code pt_add; form 0: R distinct  1: R is P  2: R is Q
 *  5 ADDA         form, P[3L], qx[L], qy[L]                      R[3L], code pt_add_affine; form 0: R distinct  1: R is P
 *  6 MUL          P[3L], k[L]                                    R[3L]       pt_mul
 *  7 FB           t, k[L]                                        R[3L]       fb_mul over table t of G (aux.tab[t], width aux.w[t])
 *  8 AFF          P[3L]                                          x[L], y[L]  pt_affine (plain)
 *  9 CHK          x[L], y[L] plain                               ok, xm[L], ym[L]   pt_check; xm, ym arrive zeroed
 * 10 H2I          dlen, digest (EC_FORM_DG_WORDS words of bytes) e[L]        hash_to_int
 * 11 XR           R[3L], r[L] plain                              ok          x_matches_r
 * 12 LIMBS        a[L]                                           lim[76], a'[L]     device program only (ec_kernels.hip)
 * A distinct R arrives filled with 0xA5A5A5A5. */
#pragma once
#include <stdint.h>
#include "../../bftkv_amd/csrc/ec_field.h"

namespace ecforms {

enum : uint32_t { FAM_FE = 0, FAM_INV, FAM_FN, FAM_DBL, FAM_ADD, FAM_ADDA, FAM_MUL, FAM_FB, FAM_AFF, FAM_CHK, FAM_H2I, FAM_XR, FAM_LIMBS, FAM_COUNT };
constexpr uint32_t EC_FORM_DG_WORDS = 33;      // digests of up to 132 bytes (2 f on P-521)
constexpr uint32_t EC_FORM_LIMBS = 76;
constexpr uint32_t EC_FORM_TABLES = 2;
constexpr uint32_t EC_FORM_W[EC_FORM_TABLES] = {4, 5};      // 4: the library's width on every curve (ec_capi.inc ec_fb_table)

constexpr uint32_t in_words(uint32_t L, uint32_t fam) {
  return fam == FAM_FE ? 1 + 2 * L : fam == FAM_INV ? L : fam == FAM_FN ? 2 * L : fam == FAM_DBL ? 3 * L : fam == FAM_ADD ? 1 + 6 * L
       : fam == FAM_ADDA ? 1 + 5 * L : fam == FAM_MUL ? 4 * L : fam == FAM_FB ? 1 + L : fam == FAM_AFF ? 3 * L : fam == FAM_CHK ? 2 * L
       : fam == FAM_H2I ? 1 + EC_FORM_DG_WORDS : fam == FAM_XR ? 4 * L : fam == FAM_LIMBS ? L : 0;
}
constexpr uint32_t out_words(uint32_t L, uint32_t fam) {
  return fam == FAM_FE || fam == FAM_INV || fam == FAM_FN || fam == FAM_H2I ? L : fam == FAM_DBL || fam == FAM_MUL || fam == FAM_FB ? 3 * L
       : fam == FAM_ADD || fam == FAM_ADDA ? 3 * L + 1 : fam == FAM_AFF ? 2 * L : fam == FAM_CHK ? 1 + 2 * L : fam == FAM_XR ? 1
       : fam == FAM_LIMBS ? EC_FORM_LIMBS + L : 0;
}

// what the table walk needs beside the curve
struct Aux {
  const uint32_t* tab[EC_FORM_TABLES];
  uint32_t w[EC_FORM_TABLES], nwin[EC_FORM_TABLES];
  uint32_t bits;                 // the curve's bit size (hash_to_int)
};

template <int L>
EC_HD void load_jac(ecf::Jac<L>& P, const uint32_t* s) {
  ecf::fe_copy<L>(P.x, s);
  ecf::fe_copy<L>(P.y, s + L);
  ecf::fe_copy<L>(P.z, s + 2 * L);
}
template <int L>
EC_HD void store_jac(uint32_t* d, const ecf::Jac<L>& P) {
  ecf::fe_copy<L>(d, P.x);
  ecf::fe_copy<L>(d + L, P.y);
  ecf::fe_copy<L>(d + 2 * L, P.z);
}
template <int L>
EC_HD void junk_jac(ecf::Jac<L>& P) {
#pragma unroll
  for (int i = 0; i < L; ++i) P.x[i] = P.y[i] = P.z[i] = 0xA5A5A5A5u;
}

template <int L>
EC_HD void form_fe(const ecf::Curve<L>& C, const uint32_t* in, uint32_t* out) {
  const uint32_t op = in[0] & 15u, mod = in[0] >> 4;
  const uint32_t* m = mod ? C.n : C.p;
  const uint32_t m0inv = mod ? C.n0inv : C.p0inv;
  uint32_t a[L], b[L], r[L];
  ecf::fe_copy<L>(a, in + 1);
  ecf::fe_copy<L>(b, in + 1 + L);
  ecf::fe_zero<L>(r);
  if (op == 0) ecf::fe_add<L>(r, a, b, m);
  else if (op == 1) ecf::fe_sub<L>(r, a, b, m);
  else if (op == 2) ecf::fe_mul<L>(r, a, b, m, m0inv);
  else if (op == 3) { ecf::fe_mul<L>(a, a, b, m, m0inv); ecf::fe_copy<L>(r, a); }
  else if (op == 4) { ecf::fe_mul<L>(b, a, b, m, m0inv); ecf::fe_copy<L>(r, b); }
  ecf::fe_copy<L>(out, r);
}

template <int L>
EC_HD void form_inv(const ecf::Curve<L>& C, const uint32_t* in, uint32_t* out) {
  uint32_t a[L], r[L];
  ecf::fe_copy<L>(a, in);
  ecf::fp_inv<L>(r, a, C);
  ecf::fe_copy<L>(out, r);
}

template <int L>
EC_HD void form_fn(const ecf::Curve<L>& C, const uint32_t* in, uint32_t* out) {
  uint32_t a[L], b[L], r[L];
  ecf::fe_copy<L>(a, in);
  ecf::fe_copy<L>(b, in + L);
  ecf::fn_mul<L>(r, a, b, C);
  ecf::fe_copy<L>(out, r);
}

template <int L>
EC_HD void form_dbl(const ecf::Curve<L>& C, const uint32_t* in, uint32_t* out) {
  ecf::Jac<L> P;
  load_jac<L>(P, in);
  ecf::pt_dbl<L>(P, P, C);
  store_jac<L>(out, P);
}

template <int L>
EC_HD void form_add(const ecf::Curve<L>& C, const uint32_t* in, uint32_t* out) {
  const uint32_t form = in[0];
  ecf::Jac<L> P, Q;
  load_jac<L>(P, in + 1);
  load_jac<L>(Q, in + 1 + 3 * L);
  int code;
  if (form == 1) { code = ecf::pt_add<L>(P, P, Q, C); store_jac<L>(out, P); }
  else if (form == 2) { code = ecf::pt_add<L>(Q, P, Q, C); store_jac<L>(out, Q); }
  else {
    ecf::Jac<L> R;
    junk_jac<L>(R);
    code = ecf::pt_add<L>(R, P, Q, C);
    store_jac<L>(out, R);
  }
  out[3 * L] = (uint32_t)code;
}

template <int L>
EC_HD void form_adda(const ecf::Curve<L>& C, const uint32_t* in, uint32_t* out) {
  const uint32_t form = in[0];
  ecf::Jac<L> P;
  uint32_t qx[L], qy[L];
  load_jac<L>(P, in + 1);
  ecf::fe_copy<L>(qx, in + 1 + 3 * L);
  ecf::fe_copy<L>(qy, in + 1 + 4 * L);
  int code;
  if (form == 1) { code = ecf::pt_add_affine<L>(P, P, qx, qy, C); store_jac<L>(out, P); }
  else {
    ecf::Jac<L> R;
    junk_jac<L>(R);
    code = ecf::pt_add_affine<L>(R, P, qx, qy, C);
    store_jac<L>(out, R);
  }
  out[3 * L] = (uint32_t)code;
}

template <int L>
EC_HD void form_mul(const ecf::Curve<L>& C, const uint32_t* in, uint32_t* out) {
  ecf::Jac<L> P, R;
  uint32_t k[L];
  load_jac<L>(P, in);
  ecf::fe_copy<L>(k, in + 3 * L);
  ecf::pt_mul<L>(R, P, k, C);
  store_jac<L>(out, R);
}

template <int L>
EC_HD void form_fb(const ecf::Curve<L>& C, const Aux& aux, const uint32_t* in, uint32_t* out) {
  const uint32_t t = in[0] < EC_FORM_TABLES ? in[0] : 0;
  ecf::Jac<L> R;
  uint32_t k[L];
  ecf::fe_copy<L>(k, in + 1);
  ecf::fb_mul<L>(R, aux.tab[t], aux.w[t], aux.nwin[t], k, C);
  store_jac<L>(out, R);
}

template <int L>
EC_HD void form_aff(const ecf::Curve<L>& C, const uint32_t* in, uint32_t* out) {
  ecf::Jac<L> P;
  uint32_t x[L], y[L];
  load_jac<L>(P, in);
  ecf::pt_affine<L>(x, y, P, C);
  ecf::fe_copy<L>(out, x);
  ecf::fe_copy<L>(out + L, y);
}

template <int L>
EC_HD void form_chk(const ecf::Curve<L>& C, const uint32_t* in, uint32_t* out) {
  uint32_t x[L], y[L], xm[L], ym[L];
  ecf::fe_copy<L>(x, in);
  ecf::fe_copy<L>(y, in + L);
  ecf::fe_zero<L>(xm);
  ecf::fe_zero<L>(ym);
  out[0] = ecf::pt_check<L>(xm, ym, x, y, C) ? 1u : 0u;
  ecf::fe_copy<L>(out + 1, xm);
  ecf::fe_copy<L>(out + 1 + L, ym);
}

template <int L>
EC_HD void form_h2i(const ecf::Curve<L>& C, const Aux& aux, const uint32_t* in, uint32_t* out) {
  const uint32_t dlen = in[0] <= 4 * EC_FORM_DG_WORDS ? in[0] : 4 * EC_FORM_DG_WORDS;
  uint32_t e[L];
  ecf::hash_to_int<L>(e, (const uint8_t*)(in + 1), dlen, aux.bits, C);
  ecf::fe_copy<L>(out, e);
}

template <int L>
EC_HD void form_xr(const ecf::Curve<L>& C, const uint32_t* in, uint32_t* out) {
  ecf::Jac<L> R;
  uint32_t r[L];
  load_jac<L>(R, in);
  ecf::fe_copy<L>(r, in + 3 * L);
  out[0] = ecf::x_matches_r<L>(R, r, C) ? 1u : 0u;
}

// every family but LIMBS
template <int L, uint32_t FAM>
EC_HD void form_run(const ecf::Curve<L>& C, const Aux& aux, const uint32_t* in, uint32_t* out) {
  if constexpr (FAM == FAM_FE) form_fe<L>(C, in, out);
  else if constexpr (FAM == FAM_INV) form_inv<L>(C, in, out);
  else if constexpr (FAM == FAM_FN) form_fn<L>(C, in, out);
  else if constexpr (FAM == FAM_DBL) form_dbl<L>(C, in, out);
  else if constexpr (FAM == FAM_ADD) form_add<L>(C, in, out);
  else if constexpr (FAM == FAM_ADDA) form_adda<L>(C, in, out);
  else if constexpr (FAM == FAM_MUL) form_mul<L>(C, in, out);
  else if constexpr (FAM == FAM_FB) form_fb<L>(C, aux, in, out);
  else if constexpr (FAM == FAM_AFF) form_aff<L>(C, in, out);
  else if constexpr (FAM == FAM_CHK) form_chk<L>(C, in, out);
  else if constexpr (FAM == FAM_H2I) form_h2i<L>(C, aux, in, out);
  else if constexpr (FAM == FAM_XR) form_xr<L>(C, in, out);
}

}  // namespace ecforms

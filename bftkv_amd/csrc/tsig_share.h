// The rules of a threshold DSA / ECDSA server's share answers (dsaContext.Sign, crypto/threshold/dsa/dsa_core.go:91-163; docs/parity.md,
// "Threshold DSA / ECDSA signing (dsaContext.Sign)") that need no 2048-bit multiplier: decrypt's fold of a share column mod q
// (:235-238), vi of phase 2 (:139-141), si of phase 3 (:150-155), and which row every window of the fixed walk over a DSA key set's
// table of g multiplies by.  The same text compiles for the host (tests/c/tsig_share_host.cpp checks it against the Python restatement
// in the CPU suite).
//
// Numbers mod q are L little-endian 32-bit words (L = 8 for a DSA order, 7 / 8 / 12 / 17 for a curve's N) under ec_field.h's CIOS
// product with R = 2^(32 L).  A value of ANY size below R goes into Montgomery form by one product with R^2 mod q, which reduces it as
// big.Int.Mod reduces a non-negative value: that is the whole of "a share in [q, 2^(8 width))", and a column of m shares is m such
// products and m additions mod q, so m shares of q - 1 wrap m - 1 times one subtraction at a time.  Every step is a product, an
// addition with one conditional subtraction by select, or a copy: nothing here branches on a share.
#pragma once
#include "dsa_verify.h"
#include "ec_field.h"

namespace bftkv {

constexpr uint32_t TSIG_MAX_M = 1024, TSIG_MAX_ROWS = 1u << 22;      // shares per request; n_reqs * m of a call
constexpr uint32_t TSIG_MAX_NBYTES = 66;                             // phase 3: a P-521 order's row

// an odd modulus q < 2^(32 L): q, R^2 mod q, -q^-1 mod 2^32
template <int L>
struct TsigMod {
  uint32_t q[L], rr[L];
  uint32_t q0inv;
};

// big-endian bytes (len <= 4 L) <-> words with every word index known at compile time: the number stays in registers
template <int L>
EC_HD void tsig_from_be(uint32_t* r, const uint8_t* s, uint32_t len) {
#pragma unroll
  for (int i = 0; i < L; ++i) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t k = 4u * i + b;           // byte index from the LSB
      if (k < len) v |= (uint32_t)s[len - 1 - k] << (8 * b);
    }
    r[i] = v;
  }
}
template <int L>
EC_HD void tsig_to_be(uint8_t* d, uint32_t len, const uint32_t* a) {      // a < 2^(8 len)
#pragma unroll
  for (int i = 0; i < L; ++i) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t k = 4u * i + b;
      if (k < len) d[len - 1 - k] = (uint8_t)(a[i] >> (8 * b));
    }
  }
}

// the constants of an odd q (q = 1 included: R^2 mod 1 = 0, and everything under it is 0), on the host
template <int L>
EC_HD void tsig_mod_setup(TsigMod<L>& M, const uint8_t* q_be, uint32_t qbytes) {
  tsig_from_be<L>(M.q, q_be, qbytes);
  M.q0inv = ecf::neg_inv32(M.q[0]);
  uint32_t t[L];
  ecf::fe_zero<L>(t);
  t[0] = 1;
  if (!ecf::fe_lt<L>(t, M.q)) t[0] = 0;        // q = 1
  for (int i = 0; i < 64 * L; ++i) ecf::fe_add<L>(t, t, t, M.q);
  ecf::fe_copy<L>(M.rr, t);
}

// x R mod q, fully reduced, for ANY x < 2^(32 L); and back (a < q)
template <int L>
EC_HD void tsig_to_mont(uint32_t* r, const uint32_t* x, const TsigMod<L>& M) { ecf::fe_mul<L>(r, x, M.rr, M.q, M.q0inv); }
template <int L>
EC_HD void tsig_from_mont(uint32_t* r, const uint32_t* a, const TsigMod<L>& M) {
  uint32_t one[L];
  ecf::fe_zero<L>(one);
  one[0] = 1;
  ecf::fe_mul<L>(r, a, one, M.q, M.q0inv);
}

// decrypt's fold of one column: (sum of m shares) mod q, in Montgomery form.  Share j's `width` big-endian bytes are at col + j stride.
template <int L>
EC_HD void tsig_fold_col(uint32_t* acc, const uint8_t* col, uint32_t m, size_t stride, uint32_t width, const TsigMod<L>& M) {
  uint32_t x[L];
  ecf::fe_zero<L>(acc);
  for (uint32_t j = 0; j < m; ++j) {
    tsig_from_be<L>(x, col + (size_t)j * stride, width);
    tsig_to_mont<L>(x, x, M);
    ecf::fe_add<L>(acc, acc, x, M.q);
  }
}

// phase 2: vi = ((ki ai mod q) + bi) mod q, Montgomery forms in, plain out
template <int L>
EC_HD void tsig_vi(uint32_t* vi, const uint32_t* ki_m, const uint32_t* ai_m, const uint32_t* bi_m, const TsigMod<L>& M) {
  uint32_t t[L];
  ecf::fe_mul<L>(t, ki_m, ai_m, M.q, M.q0inv);
  ecf::fe_add<L>(t, t, bi_m, M.q);
  tsig_from_mont<L>(vi, t, M);
}

// phase 3: si = ((((r y mod q) + m) mod q) k mod q + c) mod q; every operand plain and of any size below 2^(32 L), plain out
template <int L>
EC_HD void tsig_si(uint32_t* si, const uint32_t* r, const uint32_t* y, const uint32_t* mm, const uint32_t* k, const uint32_t* c, const TsigMod<L>& M) {
  uint32_t t[L], u[L];
  tsig_to_mont<L>(t, r, M);
  tsig_to_mont<L>(u, y, M);
  ecf::fe_mul<L>(t, t, u, M.q, M.q0inv);
  tsig_to_mont<L>(u, mm, M);
  ecf::fe_add<L>(t, t, u, M.q);
  tsig_to_mont<L>(u, k, M);
  ecf::fe_mul<L>(t, t, u, M.q, M.q0inv);
  tsig_to_mont<L>(u, c, M);
  ecf::fe_add<L>(t, t, u, M.q);
  tsig_from_mont<L>(si, t, M);
}

// ---- the fixed walk over a DSA key set's table of g (k_tsig_gpow) ---------------------------------------------------------------------
// Window i of ai (dsav_limbs10's ten limbs, dsav_comb_digit's digits) multiplies the running product by ONE row, for every window of the
// set: the entry of its digit d, or, for d = 0, the group's Montgomery one, which the table has no entry for and the call keeps in its
// scratch.  TSIG_ROW_ONE names that row.
constexpr uint64_t TSIG_ROW_ONE = ~0ull;
U256_HD uint64_t tsig_gpow_row(const uint32_t* limbs10, uint32_t group, uint32_t window, uint32_t windows, uint32_t w) {
  const uint32_t d = dsav_comb_digit(limbs10, window, w);
  const uint64_t e = dsav_comb_entry(group, window, d | (d == 0 ? 1u : 0u), windows, w);
  return d == 0 ? TSIG_ROW_ONE : e;
}

}  // namespace bftkv

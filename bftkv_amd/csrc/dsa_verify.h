// The per-signature rules of raw DSA verification (crypto/dsa.Verify of Go 1.13; docs/parity.md, "DSA verification"): what one
// thread of k_dsav_prep does with r, s, the digest and the order q before any exponentiation.  The same text compiles for the
// host (tests/c/dsa_verify_host.cpp checks it against the Python restatement in the CPU suite).
#pragma once
#include "u256.h"

namespace bftkv {

constexpr uint8_t DSAV_OK = 0, DSAV_NO_INVERSE = 1, DSAV_FENCED = 2;      // BFTKV_TH_OK / _NO_INVERSE / _FENCED
constexpr int DSAV_EXP_LIMBS = 10;                                        // 280 bits of radix-2^28 limbs hold a 256-bit exponent
constexpr int DSAV_ROW = 3 * DSAV_EXP_LIMBS;                              // u1, u2, r of one signature

struct DsavPrep {
  U256 u1, u2, r;
  uint8_t status;      // DSAV_*
  uint8_t decided;     // 1: the verdict is 0 whatever the exponentiation gives (u1 = u2 = 0 then)
};

U256_HD void dsav_limbs10(const U256& a, uint32_t* l) {
  for (int j = 0; j < DSAV_EXP_LIMBS; ++j) {
    const uint32_t bit = 28u * j, wi = bit >> 5, sh = bit & 31;
    uint64_t v = 0;
    if (wi < 8) v = a.w[wi];
    if (wi + 1 < 8) v |= (uint64_t)a.w[wi + 1] << 32;
    l[j] = (uint32_t)(v >> sh) & 0xFFFFFFFu;
  }
}

// big-endian bytes (len <= 32) -> U256 with every word index known at compile time: the number stays in registers
U256_HD U256 dsav_from_be(const uint8_t* p, uint32_t len) {
  U256 out;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t k = 4u * i + b;           // byte index from the LSB
      if (k < len) v |= (uint32_t)p[len - 1 - k] << (8 * b);
    }
    out.w[i] = v;
  }
  return out;
}

// sig = r || s (qbytes each), q_be [qbytes] (odd: the call refuses an even order), digest [dlen]; qbytes <= 32, dlen <= 64.
// The rows of the table in docs/parity.md, in its order.  Every caller reaches u256_modinv_odd (on the device it votes across
// the wave), a decided signature with 1 in the place of s.
U256_HD void dsav_prep_one(const uint8_t* sig, uint32_t qbytes, const uint8_t* q_be, const uint8_t* digest, uint32_t dlen, DsavPrep& o) {
  U256 w, one = u256_zero();
  one.w[0] = 1;
  const U256 r = dsav_from_be(sig, qbytes), s = dsav_from_be(sig + qbytes, qbytes), q = dsav_from_be(q_be, qbytes);
  const uint32_t qbits = (uint32_t)u256_bits(q);
  const bool range = !u256_is_zero(r) && u256_cmp(r, q) < 0 && !u256_is_zero(s) && u256_cmp(s, q) < 0;     // 0 < r, s < q
  const bool whole = (qbits & 7u) == 0;                          // Go returns false before it uses w
  const bool fenced = range && whole && dlen > (qbits >> 3);     // Go takes the whole digest: no answer claimed
  const bool live = range && whole && !fenced;
  const bool inv = u256_modinv_odd(u256_select(live, s, one), q, w);
  const bool go = live && inv;
  // z: the digest as an integer, below 2^bits(q) < 2q, so one subtraction reduces it
  U256 z = dsav_from_be(digest, live ? dlen : 0u);
  if (u256_cmp(z, q) >= 0) u256_sub(z, q);
  w = u256_select(go, w, u256_zero());
  o.u1 = u256_mulmod(w, z, q);
  o.u2 = u256_mulmod(w, r, q);
  o.r = r;
  o.decided = go ? 0 : 1;
  o.status = fenced ? DSAV_FENCED : ((live && !inv) ? DSAV_NO_INVERSE : DSAV_OK);
}

// ---- resident key sets (bftkv_gpu_dsa_keyset_*): fixed-base window tables, tab[base][window][d - 1][76 limbs] ----------------
// Window i of an exponent is its bits [w i, w i + w), w = 4 .. 16, read out of dsav_limbs10's ten limbs: at w = 4, 7 and 14 a
// window lies within one limb, at every other width some windows straddle two.  The top window is narrower when w does not
// divide the order's length (its high digits never occur; the table holds 2^w - 1 entries for it all the same).
constexpr uint32_t DSAV_COMB_WMIN = 4, DSAV_COMB_WMAX = 16, DSAV_COMB_WDEF = 8;
constexpr uint32_t DSAV_COMB_ENTRY_LIMBS = 76;                            // MONT_N of mont28.h: the <19, 4> form, R = 2^2128

U256_HD uint32_t dsav_comb_windows(uint32_t qbits, uint32_t w) { return (qbits + w - 1u) / w; }

U256_HD uint32_t dsav_comb_digit(const uint32_t* limbs10, uint32_t window, uint32_t w) {
  const uint32_t bit = window * w, li = bit / 28u, sh = bit % 28u;
  if (li >= (uint32_t)DSAV_EXP_LIMBS) return 0u;
  uint64_t v = limbs10[li];
  if (li + 1u < (uint32_t)DSAV_EXP_LIMBS) v |= (uint64_t)limbs10[li + 1u] << 28;
  return (uint32_t)(v >> sh) & ((1u << w) - 1u);
}

// the entry of digit d >= 1 in window `window` of base `base`, counted in entries (76 limbs each)
U256_HD uint64_t dsav_comb_entry(uint32_t base, uint32_t window, uint32_t d, uint32_t windows, uint32_t w) {
  return ((uint64_t)base * windows + window) * ((1u << w) - 1u) + (d - 1u);
}

}  // namespace bftkv

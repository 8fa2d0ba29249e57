// The rules of raw RSA PKCS#1 v1.5 signing (crypto/rsa.SignPKCS1v15 of Go 1.13 on its precomputed CRT branch; docs/parity.md, "RSA
// signing (rsa.SignPKCS1v15)") that need no multiplier: which keys a signer set refuses, what the length rule and the key's state decide
// before any arithmetic, the encoded message em (rsa_verify.h's, the verifier's own text) and any value of the row width as the 80
// radix-2^28 limbs k_rsas_crt splits into a low and a high half of 1120 bits, the window digits of dp and dq, and the status byte a
// signature leaves with.  The same text compiles for the host (tests/c/rsa_sign_host.cpp checks it against the Python restatement in
// the CPU suite).
#pragma once
#include <stdint.h>

#include "rsa_verify.h"

namespace bftkv {

constexpr uint8_t RSAS_OK = 0, RSAS_FENCED = 2, RSAS_INVALID_INPUT = 3, RSAS_CHECK_FAILED = 4;      // BFTKV_TH_OK / _FENCED / _INVALID_INPUT / _CHECK_FAILED
constexpr uint32_t RSAS_MAX_NBYTES = 256, RSAS_MAX_PBYTES = 128;
constexpr int RSAS_W = 28;
constexpr int RSAS_L = 10, RSAS_TPI = 4, RSAS_N = RSAS_L * RSAS_TPI;      // the 10 x 4 form: 40 limbs, R = 2^1120
constexpr int RSAS_VALUE_LIMBS = 2 * RSAS_N;                              // em, or any value of the row width: low half | high half

// A key is refused at registration (counted, no error) when n is even, or when p or q is even or below 3: the Montgomery rows need
// odd moduli, and 1 is none.  Rows are big-endian and may hold any value of their width.
RSAV_HD bool rsas_prime_refused(const uint8_t* m_be, uint32_t pbytes) {
  if (!(m_be[pbytes - 1u] & 1u)) return true;
  for (uint32_t i = 0; i + 1u < pbytes; ++i) if (m_be[i]) return false;
  return m_be[pbytes - 1u] < 3u;
}
RSAV_HD bool rsas_key_refused(const uint8_t* n_be, uint32_t nbytes, const uint8_t* p_be, const uint8_t* q_be, uint32_t pbytes) {
  return !(n_be[nbytes - 1u] & 1u) || rsas_prime_refused(p_be, pbytes) || rsas_prime_refused(q_be, pbytes);
}

// Rows 1 and 2 of the table, in its order: Go refuses k < tLen + 11 (ErrMessageTooLong) whatever the key's state; then a refused key
// is fenced.  0: the arithmetic rows decide.
RSAV_HD uint8_t rsas_rule(uint32_t k, uint32_t tlen, bool key_refused) {
  if (k < tlen + 11u) return RSAS_INVALID_INPUT;
  return key_refused ? RSAS_FENCED : RSAS_OK;
}

// limb j (of RSAS_VALUE_LIMBS) of em; zero where the length rule refuses
RSAV_HD uint32_t rsas_em_limb(uint32_t j, uint32_t k, uint32_t hash_id, const uint8_t* digest, uint32_t dlen) {
  if (k < dlen + (uint32_t)rsav_prefix_len(hash_id) + 11u) return 0u;
  return em_limb<RSAS_W>(j, k, hash_id, digest, dlen);
}
// limb j of a big-endian value of nbytes bytes (bftkv_gpu_selftest_rsa_crt's operand)
RSAV_HD uint32_t rsas_value_limb(uint32_t j, const uint8_t* v_be, uint32_t nbytes) {
  const uint32_t bit = (uint32_t)RSAS_W * j, b0 = bit >> 3, sh = bit & 7u;
  uint64_t v = 0;
  for (uint32_t t = 0; t < 5u; ++t) if (b0 + t < nbytes) v |= (uint64_t)v_be[nbytes - 1u - (b0 + t)] << (8u * t);
  return (uint32_t)(v >> sh) & ((1u << RSAS_W) - 1u);
}

// 4-bit window w (0 = least significant) of an exponent row of pbytes big-endian bytes; the chain walks w = 2 pbytes - 1 .. 0
RSAV_HD uint32_t rsas_digit(const uint8_t* d_be, uint32_t pbytes, uint32_t w) {
  return ((uint32_t)d_be[pbytes - 1u - (w >> 1)] >> ((w & 1u) * 4u)) & 15u;
}

// The status a signature leaves with: rows 1 and 2 were settled before the check and override it; then s must fit the row and pass
// the check (s^e mod n == em).  Every status but RSAS_OK leaves a row of zeroes.
RSAV_HD uint8_t rsas_status(uint8_t rule, bool fits, bool check_ok) {
  if (rule != RSAS_OK) return rule;
  return fits && check_ok ? RSAS_OK : RSAS_CHECK_FAILED;
}

}  // namespace bftkv

// The rules of raw RSA PKCS#1 v1.5 verification (crypto/rsa.VerifyPKCS1v15 of Go 1.13; docs/parity.md, "RSA verification") that need
// no multiplier: which hashes a call may name, what a key's shape decides before any arithmetic (rows 1 and 2 of the table), and
// the encoded message EM = 00 01 FF .. FF 00 || prefix || digest as the radix-2^W limbs k_rsav_verify compares with s^e mod n.
// The same text compiles for the host (tests/c/rsa_verify_host.cpp checks it against the Python restatement in the CPU suite).
#pragma once
#include <stdint.h>

#ifndef RSAV_HD
#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define RSAV_HD __host__ __device__ __forceinline__
#else
#define RSAV_HD static inline
#endif
#endif

namespace bftkv {

constexpr uint8_t RSAV_OK = 0, RSAV_FENCED = 2;                           // BFTKV_TH_OK / _FENCED
constexpr uint32_t RSAV_LIVE = 0, RSAV_REFUSED = 1, RSAV_EVEN = 2;        // what a key's shape decides: the arithmetic row, row 1, row 2
constexpr uint32_t RSAV_MAX_NBYTES = 256, RSAV_MAX_DLEN = 64;

// DigestInfo prefix length of an OpenPGP hash id (device_types.h HASH_*; hash id 0: no prefix), or -1 for an unknown id
RSAV_HD int rsav_prefix_len(uint32_t hash_id) {
  switch (hash_id) {
    case 0: return 0;
    case 1: return 18;
    case 2: return 15;
    case 3: return 14;
    case 8: case 9: case 10: case 11: return 19;
    default: return -1;
  }
}
// the digest length Go insists on ("input must be hashed message"); hash id 0 takes 1 .. 64 bytes as they stand
RSAV_HD bool rsav_dlen_ok(uint32_t hash_id, uint32_t dlen) {
  switch (hash_id) {
    case 0: return dlen >= 1 && dlen <= RSAV_MAX_DLEN;
    case 1: return dlen == 16;
    case 2: case 3: return dlen == 20;
    case 8: return dlen == 32;
    case 9: return dlen == 48;
    case 10: return dlen == 64;
    case 11: return dlen == 28;
    default: return false;
  }
}
// byte i (0 = first) of the prefix: Go's hashPrefixes (the reference's copy: crypto/threshold/rsa/rsa.go:345-354), so RIPEMD-160
// carries Go's identifier.  The SHA-2 prefixes differ in three bytes: total length, algorithm arc, digest length.
RSAV_HD uint32_t rsav_prefix_byte(uint32_t hash_id, uint32_t i) {
  // the prefixes as little-endian 64-bit words (byte j of the prefix is byte j & 7 of word j >> 3): immediates, no table in memory
  uint64_t w0, w1, w2 = 0;
  if (hash_id == 2) { w0 = 0x0e2b050609302130ull; w1 = 0x00140400051a0203ull; }                       // SHA-1, 15 bytes
  else if (hash_id == 1) { w0 = 0x862a08060c302030ull; w1 = 0x000505020df78648ull; w2 = 0x1004ull; }   // MD5, 18 bytes
  else if (hash_id == 3) { w0 = 0xcf28060608302030ull; w1 = 0x0000140431000306ull; }                   // RIPEMD-160, 14 bytes
  else {                                                                                               // SHA-2, 19 bytes
    const uint64_t dl = hash_id == 8 ? 0x20u : hash_id == 9 ? 0x30u : hash_id == 10 ? 0x40u : 0x1cu;
    const uint64_t arc = hash_id == 8 ? 1u : hash_id == 9 ? 2u : hash_id == 10 ? 3u : 4u;
    w0 = 0x866009060d300030ull | (0x11u + dl) << 8;
    w1 = 0x0500020403650148ull | arc << 48;
    w2 = 0x0400ull | dl << 16;
  }
  const uint64_t w = i < 8u ? w0 : i < 16u ? w1 : w2;
  return (uint32_t)(w >> (8u * (i & 7u))) & 0xFFu;
}

// k = ceil(bits(n) / 8) of a big-endian modulus (0 for n = 0)
RSAV_HD uint32_t rsav_kbytes(const uint8_t* n_be, uint32_t nbytes) {
  uint32_t z = 0;
  while (z < nbytes && n_be[z] == 0) ++z;
  return nbytes - z;
}

// Rows 1 and 2 of the table, in its order: Go refuses k < tLen + 11 before any arithmetic, whatever n's parity (n = 0 and n = 1
// included: k = 0, 1); an even modulus that passes has an answer from big.Int.Exp which the Montgomery rows cannot give.
RSAV_HD uint32_t rsav_rule(uint32_t k, uint32_t tlen, bool n_even) {
  if (k < tlen + 11u) return RSAV_REFUSED;
  return n_even ? RSAV_EVEN : RSAV_LIVE;
}
RSAV_HD uint8_t rsav_status(uint32_t rule) { return rule == RSAV_EVEN ? RSAV_FENCED : RSAV_OK; }

// byte i, counted from the least significant end, of the k-byte EM over (hash_id, digest[dlen]); k >= tLen + 11.  0 past the top.
RSAV_HD uint32_t rsav_em_byte(uint32_t i, uint32_t k, uint32_t hash_id, const uint8_t* digest, uint32_t dlen, uint32_t plen) {
  const uint32_t tl = dlen + plen;
  if (i < dlen) return digest[dlen - 1u - i];
  if (i < tl) return rsav_prefix_byte(hash_id, plen - 1u - (i - dlen));
  if (i == tl) return 0u;
  if (i + 2u < k) return 0xFFu;
  return i + 2u == k ? 1u : 0u;
}

// Radix-2^W limb gi of that EM (W + 7 <= 40: five bytes hold any limb).  A limb that lies wholly in the FF padding, as most do,
// or wholly above the 01 costs two comparisons.
template <int W>
RSAV_HD uint32_t em_limb(uint32_t gi, uint32_t k, uint32_t hash_id, const uint8_t* digest, uint32_t dlen) {
  const uint32_t plen = (uint32_t)rsav_prefix_len(hash_id), tl = dlen + plen;
  const uint32_t bit = (uint32_t)W * gi, b0 = bit >> 3, sh = bit & 7u;
  if (b0 > tl && b0 + 4u + 2u < k) return (1u << W) - 1u;
  if (b0 >= k) return 0u;
  uint64_t v = 0;
  for (uint32_t t = 0; t < 5u; ++t) v |= (uint64_t)rsav_em_byte(b0 + t, k, hash_id, digest, dlen, plen) << (8u * t);
  return (uint32_t)(v >> sh) & ((1u << W) - 1u);
}

}  // namespace bftkv

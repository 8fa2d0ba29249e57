// The rules of a threshold-RSA server's partial signatures (rsaContext.Sign, crypto/threshold/rsa/rsa.go:140-178; docs/parity.md,
// "Threshold RSA signing (rsaContext.Sign)") that need no multiplier: emlen of a modulus row, emsaEncode's refusal (:356-362), the
// encoded message em = 00 01 FF .. 00 || T as the radix-2^28 limbs k_psign_pow raises, which fragments count as negative (:164),
// and the status byte of a fragment.  The same text compiles for the host (tests/c/rsa_psign_host.cpp checks it against the Python
// restatement in the CPU suite).
//
// This is NOT the verifier's rule (rsa_verify.h): Sign refuses padlen < 3 where VerifyPKCS1v15 refuses k < tLen + 11, so em may
// hold no FF byte at all, and T is taken as it comes (prefix || digest of any bytes and any length: Sign does not look inside).
#pragma once
#include <stdint.h>

#ifndef PSIGN_HD
#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define PSIGN_HD __host__ __device__ __forceinline__
#else
#define PSIGN_HD static inline
#endif
#endif

namespace bftkv {

constexpr uint8_t PSIGN_OK = 0, PSIGN_NO_INVERSE = 1, PSIGN_INVALID_INPUT = 3;      // BFTKV_TH_OK / _NO_INVERSE / _INVALID_INPUT
constexpr uint32_t PSIGN_MAX_NBYTES = 256, PSIGN_MAX_EXP_LEN = 8200;                 // 8200: n - k <= 4 under a 2048-bit key
constexpr int PSIGN_W = 28;

// emlen = ceil(bits(N) / 8) of a big-endian modulus row (0 for N = 0)
PSIGN_HD uint32_t psign_emlen(const uint8_t* n_be, uint32_t nbytes) {
  uint32_t z = 0;
  while (z < nbytes && n_be[z] == 0) ++z;
  return nbytes - z;
}

// emsaEncode's only refusal: padlen = emlen - len(T) < 3 (N = 0 and N = 1 included: emlen 0 and 1)
PSIGN_HD bool psign_refused(uint32_t emlen, uint32_t t_len) { return emlen < t_len + 3u; }

// byte i, counted from the least significant end, of the emlen-byte em over T; not refused.  0 past the top.
//   em = 00 | 01 | FF x (padlen - 3) | 00 | T
PSIGN_HD uint32_t psign_em_byte(uint32_t i, uint32_t emlen, const uint8_t* t, uint32_t t_len) {
  if (i < t_len) return t[t_len - 1u - i];
  if (i == t_len) return 0u;
  if (i + 2u < emlen) return 0xFFu;
  return i + 2u == emlen ? 1u : 0u;
}

// radix-2^28 limb j of that em (five bytes hold any limb); a refused request's em is zero
PSIGN_HD uint32_t psign_em_limb(uint32_t j, uint32_t emlen, const uint8_t* t, uint32_t t_len) {
  if (psign_refused(emlen, t_len)) return 0u;
  const uint32_t bit = (uint32_t)PSIGN_W * j, b0 = bit >> 3, sh = bit & 7u;
  if (b0 >= emlen) return 0u;
  uint64_t v = 0;
  for (uint32_t k = 0; k < 5u; ++k) v |= (uint64_t)psign_em_byte(b0 + k, emlen, t, t_len) << (8u * k);
  return (uint32_t)(v >> sh) & ((1u << PSIGN_W) - 1u);
}

// parsePartialParam (:457-469): any non-zero sign byte negates the magnitude, and Neg(0) is not negative -- Sign's di.Sign() < 0
PSIGN_HD bool psign_negative(uint8_t sign_byte, bool magnitude_is_zero) { return sign_byte != 0 && !magnitude_is_zero; }

// The rows of the table in their order: a refused request fails all its fragments; a negative fragment needs m^-1.
PSIGN_HD uint8_t psign_status(bool refused, bool negative, bool m_has_no_inverse) {
  if (refused) return PSIGN_INVALID_INPUT;
  return negative && m_has_no_inverse ? PSIGN_NO_INVERSE : PSIGN_OK;
}

}  // namespace bftkv

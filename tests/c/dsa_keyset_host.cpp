/* The host-compilable pieces of resident DSA key sets, bftkv_amd/csrc/dsa_verify.h, compiled for the CPU (the same text
 * k_dsav_prep, k_dsav_comb_build and k_dsav_comb_exp compile for the GPU): the per-signature rules, the window count, the digit
 * extraction and the entry index, so that tests/test_dsa_keyset_reference.py walks its pow() tables with the kernels' own
 * arithmetic.  Test infrastructure only.
 *
 * dkh_prep(sig, qbytes, q, digest, dlen, flags, limbs): flags = status, decided; limbs = u1, u2 and r as the ten radix-2^28 limbs
 *     each that k_dsav_prep writes.
 * dkh_limbs10(be, len, limbs): a big-endian exponent of at most 32 bytes as its ten limbs.
 * dkh_windows / dkh_digit / dkh_entry: dsav_comb_windows / dsav_comb_digit / dsav_comb_entry. */
#include <stdint.h>
#include <string.h>
#include "../../bftkv_amd/csrc/dsa_verify.h"

extern "C" int dkh_prep(const uint8_t* sig, uint32_t qbytes, const uint8_t* q, const uint8_t* digest, uint32_t dlen, uint8_t* flags, uint32_t* limbs) {
  if (qbytes == 0 || qbytes > 32 || dlen == 0 || dlen > 64 || !(q[qbytes - 1] & 1)) return -1;
  bftkv::DsavPrep o;
  bftkv::dsav_prep_one(sig, qbytes, q, digest, dlen, o);
  flags[0] = o.status;
  flags[1] = o.decided;
  bftkv::dsav_limbs10(o.u1, limbs);
  bftkv::dsav_limbs10(o.u2, limbs + bftkv::DSAV_EXP_LIMBS);
  bftkv::dsav_limbs10(o.r, limbs + 2 * bftkv::DSAV_EXP_LIMBS);
  return 0;
}

extern "C" int dkh_limbs10(const uint8_t* be, uint32_t len, uint32_t* limbs) {
  if (len > 32) return -1;
  bftkv::dsav_limbs10(bftkv::dsav_from_be(be, len), limbs);
  return 0;
}

extern "C" uint32_t dkh_windows(uint32_t qbits, uint32_t w) { return bftkv::dsav_comb_windows(qbits, w); }
extern "C" uint32_t dkh_digit(const uint32_t* limbs10, uint32_t window, uint32_t w) { return bftkv::dsav_comb_digit(limbs10, window, w); }
extern "C" uint64_t dkh_entry(uint32_t base, uint32_t window, uint32_t d, uint32_t windows, uint32_t w) {
  return bftkv::dsav_comb_entry(base, window, d, windows, w);
}
extern "C" uint32_t dkh_entry_limbs(void) { return bftkv::DSAV_COMB_ENTRY_LIMBS; }

/* The per-signature rules of DSA verification, bftkv_amd/csrc/dsa_verify.h, compiled for the CPU (the same text k_dsav_prep
 * compiles for the GPU), so that tests/test_dsa_verify_reference.py can check them against the Python restatement in the CPU
 * suite.  Test infrastructure only.
 *
 * dvh_prep(sig, qbytes, q, digest, dlen, out): sig = r || s (qbytes each), q [qbytes], big-endian; out = status, decided, then
 * u1 and u2 as 32 big-endian bytes each, then u1, u2 and r as the ten radix-2^28 limbs the kernel writes (little-endian words). */
#include <stdint.h>
#include <string.h>
#include "../../bftkv_amd/csrc/dsa_verify.h"

static void be32(const bftkv::U256& a, uint8_t* out) {
  for (int i = 0; i < 32; ++i) out[i] = (uint8_t)(a.w[(31 - i) >> 2] >> (8 * ((31 - i) & 3)));
}

extern "C" int dvh_prep(const uint8_t* sig, uint32_t qbytes, const uint8_t* q, const uint8_t* digest, uint32_t dlen, uint8_t* out) {
  if (qbytes == 0 || qbytes > 32 || dlen == 0 || dlen > 64 || !(q[qbytes - 1] & 1)) return -1;
  bftkv::DsavPrep o;
  bftkv::dsav_prep_one(sig, qbytes, q, digest, dlen, o);
  out[0] = o.status;
  out[1] = o.decided;
  be32(o.u1, out + 2);
  be32(o.u2, out + 34);
  uint32_t limbs[bftkv::DSAV_ROW];
  bftkv::dsav_limbs10(o.u1, limbs);
  bftkv::dsav_limbs10(o.u2, limbs + bftkv::DSAV_EXP_LIMBS);
  bftkv::dsav_limbs10(o.r, limbs + 2 * bftkv::DSAV_EXP_LIMBS);
  memcpy(out + 66, limbs, sizeof(limbs));
  return 0;
}

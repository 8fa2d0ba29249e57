// Raw RSA PKCS#1 v1.5 verification (include/bftkv_gpu.h: bftkv_gpu_rsa_verify and its key-set forms; rsa_verify_capi.inc).
//   k_rsav_verify<L,TPI,W>  s^e mod n on mont_mul (mont28.h) and the comparison with the whole encoded message, in one kernel:
//                           fixed-width signatures and digests in, one verdict and one status byte out
// Included from capi.hip behind kernels.hip (OP_*, limb_of, value_limbs, RSA_BLOCK).
#pragma once
#include "rsa_verify.h"

namespace bftkv {

// The key rows of a call or of a resident set, in the form of the instantiation that reads them: <18, 4, 29> takes n and
// (2^2088)^2 mod n as 72 limbs of 29 bits, <10, 8> n and (2^2240)^2 mod n as 80 limbs of 28 bits.  meta[key] = { -n^-1 mod 2^29
// (its low 28 bits are -n^-1 mod 2^28), k = ceil(bits(n) / 8), e, 1 for an even n }.  A key without rows (even, 0) has zero limbs.
struct RsavKeys {
  const uint32_t* n_limbs;    // [n_keys][TPI * L]
  const uint32_t* r2_limbs;   // [n_keys][TPI * L]
  const uint4* meta;          // [n_keys]
};

// One lane group per signature.  The exponent schedule is k_rsa_modexp's: wave-uniform per (e, shortcut) class, looping over the
// classes present in the wave; waves never meet (wavefront fences only).  A signature whose key rows 1 or 2 of the table decide
// rides along on the value 1 under its key's exponent and leaves with verdict 0.
//   sigs [n_ops][nbytes], digests [n_ops][dlen], key_idx [n_ops] or null (key 0), clamped to n_keys - 1
//   xr_scratch [n_ops][TPI * L]: xR of a signature whose exponent multiplies by it again
template <int L, int TPI, int W>
__global__ void __launch_bounds__(RSA_BLOCK, 3) k_rsav_verify(uint32_t n_ops, const uint8_t* __restrict__ sigs, uint32_t nbytes,
                                                              const uint8_t* __restrict__ digests, uint32_t dlen, uint32_t hash_id,
                                                              const uint32_t* __restrict__ key_idx, uint32_t n_keys, RsavKeys keys,
                                                              uint32_t* __restrict__ xr_scratch, uint8_t* __restrict__ valid_out,
                                                              uint8_t* __restrict__ status_out) {
  static_assert((W == 29 && L == 18 && TPI == 4) || (W == MONT_W && L == 10 && TPI == 8), "18 x 4 limbs of 29 bits, or 10 x 8 of 28");
  constexpr int NL = TPI * L;
  constexpr int GROUPS = RSA_BLOCK / TPI;   // signatures per block
  __shared__ uint32_t a_sh[GROUPS * NL];
  __shared__ uint32_t x_sh[GROUPS * NL];
  if (blockIdx.x * GROUPS >= n_ops) return;
  const uint32_t grp = threadIdx.x / TPI;
  const int qlane = threadIdx.x % TPI;
  const uint32_t gq = blockIdx.x * GROUPS + grp;
  const bool active = gq < n_ops;
  const uint32_t op = active ? gq : (n_ops - 1);
  const uint32_t key = key_idx ? min(key_idx[op], n_keys - 1u) : 0u;
  const uint4 meta = keys.meta[key];
  const uint32_t n0inv = meta.x & ((1u << W) - 1u), kbytes = meta.y, e = meta.z;
  const uint32_t rule = rsav_rule(kbytes, dlen + (uint32_t)rsav_prefix_len(hash_id), meta.w != 0u);
  uint32_t* a_lds = a_sh + grp * NL + qlane * L;      // this lane's slice of the group's operand
  const uint32_t* a_rd = a_sh + grp * NL;
  uint32_t* x_lds = x_sh + grp * NL + qlane * L;

  uint32_t n[L], b[L], y[L];
  const uint32_t* np = keys.n_limbs + (uint64_t)key * NL + qlane * L;
  const uint32_t* rp = keys.r2_limbs + (uint64_t)key * NL + qlane * L;
  uint32_t* xrp = xr_scratch + (uint64_t)op * NL + qlane * L;
#pragma unroll
  for (int k = 0; k < L; ++k) n[k] = np[k];
  // signature value: nbytes big-endian bytes -> this lane's L limbs; what of it lies at or above bit 8k
  uint32_t high = 0;
  {
    const uint8_t* sp = sigs + (uint64_t)op * nbytes;
    auto sig_b = [&](uint32_t i) -> uint32_t { return i < nbytes ? sp[nbytes - 1 - i] : 0u; };
    uint32_t x[L];
    if constexpr (VALUE_LOAD_DWORDS)   // unaligned dwords, all in flight before the first is used (value_load.h)
      value_limbs<W, L, TPI>(x, nbytes, qlane,
                             [&](uint32_t o) -> uint32_t { uint32_t w; __builtin_memcpy(&w, sp + o, 4); return w; },
                             [&](uint32_t o) -> uint32_t { return sp[o]; });
#pragma unroll
    for (int k = 0; k < L; ++k) {
      const int32_t lo = (qlane * L + k) * W, cut = 8 * (int32_t)kbytes;
      uint32_t v = VALUE_LOAD_DWORDS ? x[k] : limb_of<W>(sig_b, qlane * L + k);
      if (lo + W > cut) high |= lo >= cut ? v : v >> (cut - lo);
      if (rule != RSAV_LIVE) v = (qlane == 0 && k == 0) ? 1u : 0u;
      x_lds[k] = v;
    }
    high = grp_or<TPI>(high);
  }
  // x-shortcut: the last multiplication of an odd exponent uses plain x instead of xR, which also leaves the Montgomery
  // domain.  Only when x < 2^(8k), so that the result stays below n(1 + 2^-39) (18 x 4 at 2^29, R = 2^2088; 10 x 8: R = 2^2240).
  const bool wide_x = rule == RSAV_LIVE && high != 0u;
  // (e is any 32-bit value: the class is the pair, not k_rsa_modexp's one word e << 1 | shortcut)
  const uint32_t sc = ((e & 1u) && e > 1u && !wide_x) ? 1u : 0u;

  uint64_t todo = __builtin_amdgcn_ballot_w64(true);
  while (todo) {
    const int lead = __builtin_ctzll(todo);
    const uint32_t e_u = (uint32_t)__builtin_amdgcn_readlane((int)e, lead);
    const bool sc_u = __builtin_amdgcn_readlane((int)sc, lead) != 0;
    const bool live = e == e_u && (sc != 0u) == sc_u;
    const int top = 31 - __builtin_clz(e_u | 1u);
    int kind = OP_TO_MONT, bitpos = top;
    while (true) {
      // ---- operands of this step
      if (kind == OP_TO_MONT) {
#pragma unroll
        for (int k = 0; k < L; ++k) { b[k] = rp[k]; a_lds[k] = x_lds[k]; }
      } else {
#pragma unroll
        for (int k = 0; k < L; ++k) b[k] = y[k];
        if (kind == OP_SQR) {
#pragma unroll
          for (int k = 0; k < L; ++k) a_lds[k] = y[k];
        } else if (kind == OP_MULX) {
#pragma unroll
          for (int k = 0; k < L; ++k) a_lds[k] = xrp[k];
        } else if (kind == OP_MULP) {
#pragma unroll
          for (int k = 0; k < L; ++k) a_lds[k] = x_lds[k];
        } else {
#pragma unroll
          for (int k = 0; k < L; ++k) a_lds[k] = (qlane == 0 && k == 0) ? 1u : 0u;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if (kind == OP_SQR) mont_mul<L, TPI, true, W>(y, a_rd, b, n, n0inv, qlane);
      else mont_mul<L, TPI, false, W>(y, a_rd, b, n, n0inv, qlane);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      // ---- next step (scalar control flow)
      if (kind == OP_TO_MONT && (e_u & (e_u - 1u)) != 0 && !(sc_u && __builtin_popcount(e_u) == 2)) {
#pragma unroll
        for (int k = 0; k < L; ++k) xrp[k] = y[k];   // xR is needed again by OP_MULX
      }
      if (kind == OP_MULP || kind == OP_MUL1) break;
      if (kind == OP_SQR && ((e_u >> bitpos) & 1u)) { kind = (bitpos == 0 && sc_u) ? OP_MULP : OP_MULX; continue; }
      --bitpos;
      kind = (bitpos >= 0) ? OP_SQR : OP_MUL1;
    }
    // y = t or t + n for the residue t = s^e mod n: the last product is by 1 (y < n + 1) or by the plain value x < 2^(8k)
    // (y < n(1 + 2^(8k+1)/R) <= n(1 + 2^-39)), so y = t + n is possible only for a tiny t < n * 2^-39.  An encoded message is
    // below 2^(8k-15) and at least 2^(8k-16), while n >= 2^(8k-8): such a t is no encoding, and t + n >= n is none either.
    // Comparing the unreduced y with the encoding therefore decides as comparing t would, without a final subtraction.
    canonicalize<L, TPI, W>(y, qlane);
    if (e_u == 0) {                            // x^0 = 1 (n = 1 is row 1's)
#pragma unroll
      for (int k = 0; k < L; ++k) y[k] = (qlane == 0 && k == 0) ? 1u : 0u;
    }
    // the whole encoded message against y, in registers: each lane builds the L expected limbs it owns, one at a time (y waits in
    // the lane's own LDS slice, free now, so that the loop need not be unrolled around 5 L byte fetches)
#pragma unroll
    for (int k = 0; k < L; ++k) a_lds[k] = y[k];
    uint32_t diff = 0;
    const uint8_t* dg = digests + (uint64_t)op * dlen;
#pragma unroll 1
    for (int k = 0; k < L; ++k) diff |= a_lds[k] ^ em_limb<W>((uint32_t)qlane * L + k, kbytes, hash_id, dg, dlen);
    diff = grp_or<TPI>(diff);
    if (live && active && qlane == 0) {
      valid_out[op] = (rule == RSAV_LIVE && diff == 0u) ? 1u : 0u;
      status_out[op] = rsav_status(rule);
    }
    todo &= ~__builtin_amdgcn_ballot_w64(live);
  }
}

}  // namespace bftkv

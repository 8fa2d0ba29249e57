// Threshold RSA signing, the server's side (rsaContext.Sign, crypto/threshold/rsa/rsa.go:140-178), gfx950: request bytes and stored
// key fragments in, the partial signatures of serializePartialSignature out, without a host step in between.
//   k_psign_em     em = 00 01 FF .. 00 | T of every request as radix-2^28 limbs, and its refusal byte (rsa_psign.h)
//   k_modinv       (threshold_kernels.hip, gated) m^-1 mod N and the no-inverse byte, ONCE per request that has a negative fragment
//   k_psign_pow    m^mag or (m^-1)^mag mod N, mag of up to 8200 bytes: window_chain's fixed 4-bit windows, a window count per WAVE
// The rules: docs/parity.md, "Threshold RSA signing (rsaContext.Sign)".
#pragma once
// (kernels.hip, threshold_kernels.hip, window_chain.h and tpa_kernels.hip are included before this file by capi.hip)
#include "rsa_psign.h"

namespace bftkv {

// One thread per limb of a request's em; the thread of limb 0 also writes the request's refusal byte (BFTKV_TH_INVALID_INPUT or 0).
__global__ void k_psign_em(uint32_t n_reqs, const uint8_t* __restrict__ t /*[n_reqs][t_cap]*/, uint32_t t_cap, const uint32_t* __restrict__ t_len,
                           const uint32_t* __restrict__ req_mod /*[n_reqs], below n_mods*/, const uint8_t* __restrict__ mods /*[n_mods][nbytes]*/,
                           uint32_t nbytes, uint32_t* __restrict__ em_limbs /*[n_reqs][76]*/, uint8_t* __restrict__ refused /*[n_reqs]*/) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_reqs * MONT_N) return;
  const uint32_t req = i / MONT_N, j = i % MONT_N;
  const uint32_t emlen = psign_emlen(mods + (uint64_t)req_mod[req] * nbytes, nbytes);
  const uint32_t tl = min(t_len[req], t_cap);
  em_limbs[i] = psign_em_limb(j, emlen, t + (uint64_t)req * t_cap, tl);
  if (j == 0) refused[req] = psign_refused(emlen, tl) ? PSIGN_INVALID_INPUT : PSIGN_OK;
}

// out[frag] = base ^ mag mod N for one CHAIN per quad.  Chain c of the call is fragment order[c]; the host hands the chains over
// longest first, so that the quads of a wave agree on their width, but no answer depends on that order.
//
// The chain is window_chain (window_chain.h, with what depends on a secret and what does not), as k_tpa_pow's.  Three things differ:
//   * the base row is m or m^-1 of the fragment's request, by the fragment's sign: an address, like the table row;
//   * the window count is the WAVE's: 2 x the widest exp_used among its 16 quads.  A narrower chain meets zero digits first, which is
//     what left-padding its magnitude to the wave's width gives: 1 * 1 = 1 in Montgomery form, so its answer is unchanged, and the
//     program counter stays wave-uniform.  A wave of empty magnitudes has no window: m^0 = 1;
//   * a refused request's chains, and the negative chains of a request whose m has no inverse, store zeroes and their status.
//   products: 1 (to Montgomery form) + 14 (table) + 1 (one) + 2 width * 5 + 1 (leave)        10 per byte of the wave's width
// The fragments and their signs are SECRET shares.  Beyond the table row's address, the address of the base row depends on one (the
// sign).  The widths follow from a fragment's depth in the key tree, which its index kid * n + id + 1 discloses to whoever sees the
// response.
// Padding quads (past the launch's chains) run the last chain again on a table of their own and store nothing.
struct PsignChain : TpaChain {
  uint32_t used;
  // (w >> 1: the digit's byte, counted from the row's end; past this chain's width: digit 0)
  __device__ __forceinline__ uint32_t digit(uint32_t w) const { return (w >> 1) < used ? TpaChain::digit(w) : 0u; }
};
__global__ void __launch_bounds__(RSA_BLOCK) k_psign_pow(uint32_t n_here /*chains of this launch*/, uint32_t first /*its first chain*/,
                                                         const uint32_t* __restrict__ order /*[chains] -> fragment*/,
                                                         const uint32_t* __restrict__ frag_req /*[n_frags], below n_reqs*/,
                                                         const uint32_t* __restrict__ exp_used /*[n_frags], <= exp_len*/,
                                                         const uint8_t* __restrict__ negative /*[n_frags] psign_negative*/,
                                                         const uint32_t* __restrict__ em_limbs /*[n_reqs][76]*/,
                                                         const uint32_t* __restrict__ inv_limbs /*[n_reqs][76]*/,
                                                         const uint8_t* __restrict__ refused /*[n_reqs]*/, const uint8_t* __restrict__ no_inverse /*[n_reqs]*/,
                                                         const uint8_t* __restrict__ exps /*[n_frags][exp_len] big-endian, right-aligned*/, uint32_t exp_len,
                                                         const uint32_t* __restrict__ req_mod /*[n_reqs], below the table's rows*/, ModTab mt,
                                                         uint32_t* __restrict__ scratch /*[quads of the launch][16][76]*/,
                                                         uint32_t* __restrict__ out_limbs /*[n_frags][76]*/, uint8_t* __restrict__ status /*[n_frags]*/) {
  __shared__ uint32_t a_sh[QUADS_PER_BLOCK * MONT_N];
  constexpr int L = MONT_L;
  const uint32_t quad = threadIdx.x >> 2;
  const int qlane = threadIdx.x & 3;
  const uint32_t lq = blockIdx.x * QUADS_PER_BLOCK + quad;
  const bool active = lq < n_here;
  const uint32_t frag = order[first + (active ? lq : n_here - 1)];
  const uint32_t req = frag_req[frag];
  const bool neg = negative[frag] != 0;
  const uint8_t st = psign_status(refused[req] != 0, neg, no_inverse[req] != 0);
  const uint32_t used = exp_used[frag];
  uint32_t* a_lds = a_sh + quad * MONT_N + qlane * L;
  const uint32_t* a_rd = a_sh + quad * MONT_N;
  const uint32_t mi = req_mod[req];
  const uint32_t* r2p = mt.r2_limbs + (uint64_t)mi * MONT_N + qlane * L;
  const uint32_t* brow = (neg ? inv_limbs : em_limbs) + (uint64_t)req * MONT_N + qlane * L;
  const uint8_t* erow = exps + (uint64_t)frag * exp_len;
  uint32_t* tab = scratch + (uint64_t)lq * CHAIN_ENT * MONT_N + qlane * L;    // this lane's limbs of row 0
  uint32_t n[L], t[L];
#pragma unroll
  for (int k = 0; k < L; ++k) n[k] = mt.n_limbs[(uint64_t)mi * MONT_N + qlane * L + k];
  const uint32_t n0inv = mt.n0inv[mi];
  // the wave's width: the widest chain among its quads, in a scalar register
  uint32_t wide = used;
#pragma unroll
  for (int off = 32; off >= 4; off >>= 1) wide = max(wide, (uint32_t)__shfl_xor((int)wide, off));
  wide = (uint32_t)__builtin_amdgcn_readfirstlane((int)wide);
  PsignChain pol{{brow, r2p, erow, exp_len}, used};
  window_chain<L, MONT_TPI>(pol, a_lds, a_rd, tab, r2p, n, n0inv, qlane, 2 * (int)wide, t);
  canonicalize(t, qlane);
  if (!active) return;
  uint32_t* o = out_limbs + (uint64_t)frag * MONT_N + qlane * L;
  if (st == PSIGN_OK) store_mod_result(o, t, n, qlane);
  else {
#pragma unroll
    for (int k = 0; k < L; ++k) o[k] = 0u;
  }
  if (qlane == 0) status[frag] = st;
}

}  // namespace bftkv

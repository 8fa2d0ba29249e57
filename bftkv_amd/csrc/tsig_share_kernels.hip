// Threshold DSA / ECDSA signing, a server's share answers (dsaContext.Sign, crypto/threshold/dsa/dsa_core.go:91-163), gfx950: from
// the request's decrypted shares to x's companions ri, vi (sent) and ki, ci (kept), then si, without a host step in between.
//   k_tsig_fold<L>   thread / request: decrypt's fold of the four share columns mod q, vi; ki, ci, vi as bytes, ai for the walk
//   k_tsig_ones      lane group / group of the set: R mod p, the row of a zero digit
//   k_tsig_gpow      lane group / request: ri = g^ai mod p from a DSA key set's table of g, one product per window of the set
//   k_tsig_gmul<L>   thread / request: ri = Marshal(ai G) from the context's table of G, one mixed addition per window (fb_mul_fixed)
//   k_tsig_s<L>      thread / request: si of the last phase
// ai is a share of the signing nonce's mask: no kernel here branches on it, skips for it or votes over it.  The rules: tsig_share.h
// and docs/parity.md, "Threshold DSA / ECDSA signing (dsaContext.Sign)".
#pragma once
// (kernels.hip, threshold_kernels.hip, ec_kernels.hip and dsa_verify_kernels.hip are included before this file by capi.hip)
#include "tsig_share.h"

namespace bftkv {

// shares [n_reqs][m][4][width]: k, a, b, c of every share, big-endian, any value of the width.  ai_out: dsav_limbs10's ten limbs per
// request (limbs10, L = 8: what dsav_comb_digit reads) or L words.  grp_out (may be null): the request's clamped group.
template <int L>
__global__ void __launch_bounds__(EC_BLOCK) k_tsig_fold(uint32_t n_reqs, uint32_t m, const uint8_t* __restrict__ shares, uint32_t width,
                                                        const uint32_t* __restrict__ group_idx /*[n_reqs] or null: group 0*/, uint32_t n_groups,
                                                        const TsigMod<L>* __restrict__ mods /*[n_groups]*/, uint8_t* __restrict__ vi_out,
                                                        uint8_t* __restrict__ ki_out, uint8_t* __restrict__ ci_out /*[n_reqs][width] each*/,
                                                        uint32_t* __restrict__ ai_out, uint32_t limbs10, uint32_t* __restrict__ grp_out) {
  const uint32_t req = blockIdx.x * blockDim.x + threadIdx.x;
  if (req >= n_reqs) return;
  const uint32_t gi = group_idx ? min(group_idx[req], n_groups - 1u) : 0u;
  const TsigMod<L> M = mods[gi];
  const uint8_t* row = shares + (uint64_t)req * m * 4u * width;
  const size_t stride = 4u * (size_t)width;
  uint32_t ki[L], ai[L], t[L];
  tsig_fold_col<L>(ki, row, m, stride, width, M);
  tsig_fold_col<L>(ai, row + width, m, stride, width, M);
  tsig_fold_col<L>(t, row + 2u * width, m, stride, width, M);      // bi
  tsig_vi<L>(t, ki, ai, t, M);
  tsig_to_be<L>(vi_out + (uint64_t)req * width, width, t);
  tsig_from_mont<L>(t, ki, M);
  tsig_to_be<L>(ki_out + (uint64_t)req * width, width, t);
  tsig_from_mont<L>(t, ai, M);
  if constexpr (L == 8) {
    if (limbs10) {
      U256 a;
#pragma unroll
      for (int i = 0; i < 8; ++i) a.w[i] = t[i];
      dsav_limbs10(a, ai_out + (uint64_t)req * DSAV_EXP_LIMBS);
    }
  }
  if (L != 8 || !limbs10) {
#pragma unroll
    for (int i = 0; i < L; ++i) ai_out[(uint64_t)req * L + i] = t[i];
  }
  tsig_fold_col<L>(t, row + 3u * width, m, stride, width, M);      // ci
  tsig_from_mont<L>(t, t, M);
  tsig_to_be<L>(ci_out + (uint64_t)req * width, width, t);
  if (grp_out) grp_out[req] = gi;
}

// R mod p of every group, fully reduced as the table's entries are (k_dsav_comb_build's B^0): the row a zero digit multiplies by
__global__ void __launch_bounds__(RSA_BLOCK) k_tsig_ones(uint32_t n_groups, ModTab mp, uint32_t* __restrict__ ones /*[n_groups][76]*/) {
  __shared__ uint32_t a_sh[QUADS_PER_BLOCK * MONT_N];
  constexpr int L = MONT_L;
  const uint32_t quad = threadIdx.x >> 2;
  const int qlane = threadIdx.x & 3;
  const uint32_t lq = blockIdx.x * QUADS_PER_BLOCK + quad;
  const bool active = lq < n_groups;
  const uint32_t gi = active ? lq : n_groups - 1u;
  uint32_t* a_lds = a_sh + quad * MONT_N + qlane * L;
  const uint32_t* a_rd = a_sh + quad * MONT_N;
  uint32_t n[L], y[L], t[L];
#pragma unroll
  for (int k = 0; k < L; ++k) {
    n[k] = mp.n_limbs[(uint64_t)gi * MONT_N + qlane * L + k];
    y[k] = mp.r2_limbs[(uint64_t)gi * MONT_N + qlane * L + k];
    a_lds[k] = (qlane == 0 && k == 0) ? 1u : 0u;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  mont_mul<L, MONT_TPI, false>(t, a_rd, y, n, mp.n0inv[gi], qlane);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  canonicalize<L, MONT_TPI>(t, qlane);
  reduce_once<L, MONT_TPI>(t, n, qlane);
  if (active) {
#pragma unroll
    for (int k = 0; k < L; ++k) ones[(uint64_t)gi * MONT_N + qlane * L + k] = t[k];
  }
}

// out = g^ai mod p for one request per quad, from the set's table of its group's g (dsav_comb_entry's layout, dsav_comb_digit's digits,
// at the set's width w).  The running product starts at the group's Montgomery one and EVERY window of the set multiplies it by one
// row: the entry of the window's digit, or the one row again for a zero digit (tsig_gpow_row).  No vote, no skip, no "first non-zero
// digit starts the chain": the sequence of products is a function of `windows` alone, the same in every lane, whatever the exponents.
// The ADDRESS of the row does depend on the digit.
//   products: windows + 1 (leave Montgomery form)        33 at a 256-bit q and w = 8, 65 at w = 4
// One loop with one multiplier call site.  Padding quads (past the call's requests) run the last request again and store nothing.
__global__ void __launch_bounds__(RSA_BLOCK) k_tsig_gpow(uint32_t n_reqs, const uint32_t* __restrict__ ai10 /*[n_reqs][10]*/,
                                                         const uint32_t* __restrict__ grp /*[n_reqs], below the set's groups*/, ModTab mp,
                                                         const uint32_t* __restrict__ tab, const uint32_t* __restrict__ ones /*[groups][76]*/,
                                                         uint32_t w, uint32_t windows, uint32_t* __restrict__ out_limbs /*[n_reqs][76]*/) {
  __shared__ uint32_t a_sh[QUADS_PER_BLOCK * MONT_N];
  constexpr int L = MONT_L;
  const uint32_t quad = threadIdx.x >> 2;
  const int qlane = threadIdx.x & 3;
  const uint32_t lq = blockIdx.x * QUADS_PER_BLOCK + quad;
  const bool active = lq < n_reqs;
  const uint32_t req = active ? lq : n_reqs - 1u;
  const uint32_t gi = grp[req];
  uint32_t* a_lds = a_sh + quad * MONT_N + qlane * L;
  const uint32_t* a_rd = a_sh + quad * MONT_N;
  const uint32_t* erow = ai10 + (uint64_t)req * DSAV_EXP_LIMBS;
  const uint32_t* one_row = ones + (uint64_t)gi * MONT_N;
  uint32_t n[L], y[L], t[L];
#pragma unroll
  for (int k = 0; k < L; ++k) { n[k] = mp.n_limbs[(uint64_t)gi * MONT_N + qlane * L + k]; y[k] = one_row[qlane * L + k]; }
  const uint32_t n0inv = mp.n0inv[gi];
#pragma unroll 1
  for (uint32_t i = 0; i <= windows; ++i) {
    if (i < windows) {
      const uint64_t e = tsig_gpow_row(erow, gi, i, windows, w);
      const uint32_t* row = (e == TSIG_ROW_ONE ? one_row : tab + e * MONT_N) + qlane * L;
#pragma unroll
      for (int k = 0; k < L; ++k) a_lds[k] = row[k];
    } else {                                        // leave: mont(y, 1)
#pragma unroll
      for (int k = 0; k < L; ++k) a_lds[k] = (qlane == 0 && k == 0) ? 1u : 0u;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    mont_mul<L, MONT_TPI, false>(t, a_rd, y, n, n0inv, qlane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int k = 0; k < L; ++k) y[k] = t[k];
  }
  canonicalize(t, qlane);
  if (active) store_mod_result(out_limbs + (uint64_t)req * MONT_N + qlane * L, t, n, qlane);
}

// out = Marshal(ai G): 04 || x || y, and 04 || 0 .. 0 for ai = 0 (infinity's Z = 0 inverts to 0, so the affine step needs no test)
template <int L>
__global__ void __launch_bounds__(EC_BLOCK) k_tsig_gmul(uint32_t n_reqs, const uint32_t* __restrict__ ai /*[n_reqs][L], below N*/, ecf::Curve<L> C,
                                                        const uint32_t* __restrict__ tab, uint32_t w, uint32_t nwin,
                                                        uint8_t* __restrict__ out /*[n_reqs][1 + 2 f]*/) {
  const uint32_t req = blockIdx.x * blockDim.x + threadIdx.x;
  if (req >= n_reqs) return;
  const uint32_t f = C.fbytes;
  uint8_t* o = out + (uint64_t)req * (1 + 2 * f);
  uint32_t s[L], zi[L], z2[L];
#pragma unroll
  for (int i = 0; i < L; ++i) s[i] = ai[(uint64_t)req * L + i];
  ecf::Jac<L> Q;
  ecf::fb_mul_fixed<L>(Q, tab, w, nwin, s, C);
  ecf::fp_inv<L>(zi, Q.z, C);
  ecf::fp_sqr<L>(z2, zi, C);
  ecf::fe_zero<L>(s);
  s[0] = 1;                                                  // (plain 1: a product with it leaves Montgomery form)
  ecf::fp_mul<L>(Q.x, Q.x, z2, C);
  ecf::fp_mul<L>(Q.x, Q.x, s, C);
  ecf::fp_mul<L>(z2, z2, zi, C);
  ecf::fp_mul<L>(Q.y, Q.y, z2, C);
  ecf::fp_mul<L>(Q.y, Q.y, s, C);
  o[0] = 4;
  tsig_to_be<L>(o + 1, f, Q.x);
  tsig_to_be<L>(o + 1 + f, f, Q.y);
}

// si = ((((r y mod q) + m) mod q) k mod q + c) mod q; rows of nbytes <= 4 L, any value of the width
template <int L>
__global__ void __launch_bounds__(EC_BLOCK) k_tsig_s(uint32_t n_reqs, const uint8_t* __restrict__ m_in, const uint8_t* __restrict__ r,
                                                     const uint8_t* __restrict__ y, const uint8_t* __restrict__ k, const uint8_t* __restrict__ c,
                                                     uint32_t nbytes, const uint32_t* __restrict__ mod_idx /*[n_reqs], clamped by the host*/,
                                                     const TsigMod<L>* __restrict__ mods, uint8_t* __restrict__ si_out) {
  const uint32_t req = blockIdx.x * blockDim.x + threadIdx.x;
  if (req >= n_reqs) return;
  const TsigMod<L> M = mods[mod_idx[req]];
  const uint64_t at = (uint64_t)req * nbytes;
  uint32_t rw[L], yw[L], mw[L], kw[L], cw[L];
  tsig_from_be<L>(rw, r + at, nbytes);
  tsig_from_be<L>(yw, y + at, nbytes);
  tsig_from_be<L>(mw, m_in + at, nbytes);
  tsig_from_be<L>(kw, k + at, nbytes);
  tsig_from_be<L>(cw, c + at, nbytes);
  tsig_si<L>(rw, rw, yw, mw, kw, cw, M);
  tsig_to_be<L>(si_out + at, nbytes, rw);
}

}  // namespace bftkv

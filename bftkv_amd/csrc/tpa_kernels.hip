// Threshold password authentication (crypto/auth/auth.go), gfx950: the phase computations of a server (makeYi :196-200, makeBi
// :202-223) and of the client (processBi :331-347), from request bytes to response fields without a host step in between.
//   k_tpa_bytes_to_limbs   big-endian rows, each with its own length, -> radix-2^28 limbs
//   k_tpa_pow              base ^ e mod p, e of up to 256 bytes: fixed 4-bit windows, a schedule that depends on exp_len alone
//   k_tpa_finish           keySched (HKDF-SHA256 over Ki.Bytes()) and the MAC (HMAC-SHA256 over Xi | Bi.Bytes())
// The rules: docs/parity.md, "Password authentication (crypto/auth)".
#pragma once
// (kernels.hip, threshold_kernels.hip and window_chain.h are included before this file by capi.hip)

namespace bftkv {

// Row r of `src` holds a number in its first min(lens[r], nbytes) bytes (lens == nullptr: in all nbytes of them), big-endian; what
// follows in the row is ignored (a request's Xi travels as received, auth.go:208).
__global__ void k_tpa_bytes_to_limbs(const uint8_t* __restrict__ src, uint32_t nbytes, const uint32_t* __restrict__ lens, uint32_t n_nums,
                                     uint32_t* __restrict__ dst) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_nums * MONT_N) return;
  const uint32_t num = i / MONT_N, j = i % MONT_N;
  const uint8_t* p = src + (uint64_t)num * nbytes;
  const uint32_t len = lens ? min(lens[num], nbytes) : nbytes;
  auto bf = [&](uint32_t k) -> uint32_t { return k < len ? p[len - 1 - k] : 0u; };
  dst[i] = limb_of(bf, (int)j);
}

// out = base ^ e mod p for one CHAIN per quad.  A call's chains are laid out [bases][n_ops]: chain c belongs to operation c % n_ops,
// whose exponent and modulus it takes -- makeBi's two powers v^b and Xi^b are two chains that share b, in different quads, so the
// registers of a quad are those of one chain.
//
// The chain is window_chain (window_chain.h, with what depends on a secret and what does not) over all 2 * exp_len digits of the
// exponent row: the schedule depends on exp_len alone, whatever the exponents (y of makeYi and b of makeBi are secrets).  The table
// is 4.75 KB per quad of the launch.
//   products: 1 (to Montgomery form) + 14 (table) + 1 (one) + 2 exp_len * 5 + 1 (leave)        2,577 at 256 exponent bytes
// Padding quads (past the launch's chains) run the last chain again on a table of their own and store no result.
struct TpaChain {
  static constexpr int PRE = 1, POST = 0;
  const uint32_t *brow, *r2p;         // this lane's limbs of the base and of R^2
  const uint8_t* erow;
  uint32_t exp_len;
  __device__ __forceinline__ void pre_load(int, uint32_t* a_lds, uint32_t (&y)[MONT_L]) const {      // b * R
#pragma unroll
    for (int k = 0; k < MONT_L; ++k) { a_lds[k] = brow[k]; y[k] = r2p[k]; }
  }
  __device__ __forceinline__ void pre_done(int, uint32_t (&)[MONT_L]) const {}
  __device__ __forceinline__ uint32_t digit(uint32_t w) const { return ((uint32_t)erow[exp_len - 1 - (w >> 1)] >> ((w & 1) * 4)) & 15u; }
};
__global__ void __launch_bounds__(RSA_BLOCK) k_tpa_pow(uint32_t n_here /*chains of this launch*/, uint32_t first /*its first chain*/, uint32_t n_ops,
                                                       const uint32_t* __restrict__ base_limbs /*[chains][76]*/,
                                                       const uint8_t* __restrict__ exps /*[n_ops][exp_len] big-endian*/, uint32_t exp_len,
                                                       const uint32_t* __restrict__ mod_idx /*[n_ops], below the table's rows*/, ModTab mt,
                                                       uint32_t* __restrict__ scratch /*[quads of the launch][16][76]*/,
                                                       uint32_t* __restrict__ out_limbs /*[chains][76]*/) {
  __shared__ uint32_t a_sh[QUADS_PER_BLOCK * MONT_N];
  constexpr int L = MONT_L;
  const uint32_t quad = threadIdx.x >> 2;
  const int qlane = threadIdx.x & 3;
  const uint32_t lq = blockIdx.x * QUADS_PER_BLOCK + quad;
  const bool active = lq < n_here;
  const uint32_t chain = first + (active ? lq : n_here - 1);
  const uint32_t op = chain % n_ops;
  uint32_t* a_lds = a_sh + quad * MONT_N + qlane * L;
  const uint32_t* a_rd = a_sh + quad * MONT_N;
  const uint32_t mi = mod_idx[op];
  const uint32_t* r2p = mt.r2_limbs + (uint64_t)mi * MONT_N + qlane * L;
  const uint32_t* brow = base_limbs + (uint64_t)chain * MONT_N + qlane * L;
  const uint8_t* erow = exps + (uint64_t)op * exp_len;
  uint32_t* tab = scratch + (uint64_t)lq * CHAIN_ENT * MONT_N + qlane * L;    // this lane's limbs of row 0
  uint32_t n[L], t[L];
#pragma unroll
  for (int k = 0; k < L; ++k) n[k] = mt.n_limbs[(uint64_t)mi * MONT_N + qlane * L + k];
  const uint32_t n0inv = mt.n0inv[mi];
  TpaChain pol{brow, r2p, erow, exp_len};
  window_chain<L, MONT_TPI>(pol, a_lds, a_rd, tab, r2p, n, n0inv, qlane, 2 * (int)exp_len, t);
  canonicalize(t, qlane);
  if (active) store_mod_result(out_limbs + (uint64_t)chain * MONT_N + qlane * L, t, n, qlane);
}

// ---- keySched and the MAC: HMAC-SHA256 with keys of at most 64 bytes, one thread per operation ------------------------------------
// SHA-256 of (a prefix of whole blocks already in s) | at(0) .. at(len - 1), finished.
template <class F>
__device__ __forceinline__ void tpa_sha256_tail(uint32_t (&s)[8], F at, uint32_t len, uint32_t prefix_bytes) {
  const uint32_t nblk = (len + 9 + 63) / 64;
#pragma unroll 1
  for (uint32_t b = 0; b < nblk; ++b) {
    uint32_t wd[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      uint32_t v = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t pos = b * 64 + i * 4 + j;
        const uint32_t by = pos < len ? (uint32_t)at(pos) : (pos == len ? 0x80u : 0u);
        v = (v << 8) | by;
      }
      wd[i] = v;
    }
    if (b == nblk - 1) wd[15] = (prefix_bytes + len) * 8;      // (the eight length bytes lie past the 0x80: they were zero)
    sha256_compress(s, wd);
  }
}
// out = HMAC-SHA256(key, at(0) .. at(len - 1)); key_word(i), i < 16: the key's big-endian words, zero-padded to 64 bytes
template <class K, class F>
__device__ __forceinline__ void tpa_hmac(K key_word, F at, uint32_t len, uint32_t (&out)[8]) {
  uint32_t wd[16], in[8];
#pragma unroll
  for (int i = 0; i < 16; ++i) wd[i] = key_word(i) ^ 0x36363636u;
  sha256_init(in);
  sha256_compress(in, wd);
  tpa_sha256_tail(in, at, len, 64);
#pragma unroll
  for (int i = 0; i < 16; ++i) wd[i] = key_word(i) ^ 0x5c5c5c5cu;
  sha256_init(out);
  sha256_compress(out, wd);
#pragma unroll
  for (int i = 0; i < 16; ++i) wd[i] = i < 8 ? in[i] : (i == 8 ? 0x80000000u : 0u);
  wd[15] = (64 + 32) * 8;
  sha256_compress(out, wd);
}

// ki, bi: fixed-width big-endian rows; Ki.Bytes() and Bi.Bytes() are what is left of them after the leading zero bytes (nothing for 0).
//   PRK = HMAC(salt, Ki.Bytes());  T1 = HMAC(PRK, 0x01) = km | ke  (hkdf with an empty info, auth.go:182-194)
//   mac = HMAC(km, Xi | Bi.Bytes()), Xi the xi_len[op] bytes as received
__global__ void __launch_bounds__(64) k_tpa_finish(uint32_t n_ops, const uint8_t* __restrict__ ki /*[n_ops][nbytes]*/,
                                                   const uint8_t* __restrict__ bi /*[n_ops][nbytes]*/, uint32_t nbytes,
                                                   const uint8_t* __restrict__ xi /*[n_ops][nbytes]*/, const uint32_t* __restrict__ xi_len,
                                                   const uint8_t* __restrict__ salt /*[n_ops][salt_len]*/, uint32_t salt_len,
                                                   uint8_t* __restrict__ keys_out /*[n_ops][32]*/, uint8_t* __restrict__ mac_out /*[n_ops][32]*/) {
  const uint32_t op = blockIdx.x * blockDim.x + threadIdx.x;
  if (op >= n_ops) return;
  const uint8_t* krow = ki + (uint64_t)op * nbytes;
  const uint8_t* brow = bi + (uint64_t)op * nbytes;
  const uint8_t* xrow = xi + (uint64_t)op * nbytes;
  const uint8_t* srow = salt + (uint64_t)op * salt_len;      // (never read when salt_len is 0)
  uint32_t kz = 0, bz = 0;
  while (kz < nbytes && krow[kz] == 0) ++kz;
  while (bz < nbytes && brow[bz] == 0) ++bz;
  const uint32_t xl = min(xi_len[op], nbytes);
  uint32_t prk[8], t1[8], mac[8];
  tpa_hmac([&](int i) -> uint32_t {
             uint32_t v = 0;
             for (int j = 0; j < 4; ++j) v = (v << 8) | ((uint32_t)(4 * i + j) < salt_len ? (uint32_t)srow[4 * i + j] : 0u);
             return v;
           },
           [&](uint32_t p) -> uint8_t { return krow[kz + p]; }, nbytes - kz, prk);
  tpa_hmac([&](int i) -> uint32_t { return i < 8 ? prk[i] : 0u; }, [](uint32_t) -> uint8_t { return 1; }, 1, t1);
  tpa_hmac([&](int i) -> uint32_t { return i < 4 ? t1[i] : 0u; },
           [&](uint32_t p) -> uint8_t { return p < xl ? xrow[p] : brow[bz + (p - xl)]; }, xl + (nbytes - bz), mac);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      keys_out[(uint64_t)op * 32 + 4 * i + j] = (uint8_t)(t1[i] >> (24 - 8 * j));
      mac_out[(uint64_t)op * 32 + 4 * i + j] = (uint8_t)(mac[i] >> (24 - 8 * j));
    }
  }
}

}  // namespace bftkv

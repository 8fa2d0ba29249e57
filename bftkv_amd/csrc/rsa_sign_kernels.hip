// Raw RSA PKCS#1 v1.5 signing under resident private key sets (include/bftkv_gpu.h: bftkv_gpu_rsa_sign_keyset, its _dev form and
// bftkv_gpu_selftest_rsa_crt; rsa_sign_capi.inc), gfx950: digests in, signature bytes out, by rsa.decrypt's precomputed CRT branch.
//   k_rsas_em          em = 00 01 FF .. 00 | prefix | digest as 80 limbs (low | high 1120 bits) and the rule byte of every signature
//   k_rsas_value       the same limbs of a caller's c (bftkv_gpu_selftest_rsa_crt), the rule byte by the key's state alone
//   k_rsas_crt         m1 = c^dp mod p and m2 = c^dq mod q in two quads of one wave, then h = (m1 - m2) qinv mod p
//   k_rsas_recombine   s = m2 + h q, a plain 40 x 40-limb product, and whether it fits the row
//   k_rsas_bytes       s as nbytes big-endian bytes -- which k_rsav_verify<18, 4, 29> (rsa_verify_kernels.hip) then checks as it stands
//   k_rsas_finish      the status of every signature; a row that is not BFTKV_TH_OK is zeroed
// The rules: rsa_sign.h and docs/parity.md, "RSA signing (rsa.SignPKCS1v15)".
#pragma once
// (kernels.hip, rsa_verify_kernels.hip and window_chain.h are included before this file by capi.hip)
#include "rsa_sign.h"

namespace bftkv {

// The rows of a signer set.  `prime` rows come in pairs, p's then q's: [n_keys][2][...].  A refused key has zero rows.
struct RsasKeys {
  const uint32_t* mod;        // [n_keys][2][40] p and q as plain limbs
  const uint32_t* r2;         // [n_keys][2][40] R^2 mod p, R^2 mod q  (R = 2^1120)
  const uint32_t* r3;         // [n_keys][2][40] R^3 mod p, R^3 mod q
  const uint32_t* n0inv;      // [n_keys][2]     -p^-1, -q^-1 mod 2^28
  const uint8_t* d;           // [n_keys][2][pbytes] dp, dq, big-endian
  const uint32_t* qinv_r;     // [n_keys][40]    qinv R mod p
  const uint8_t* refused;     // [n_keys]
  const uint4* meta;          // [n_keys]        the verifier's meta word (RsavKeys): .y = k = ceil(bits(n) / 8)
  uint32_t n_keys, pbytes;
};

constexpr int RSAS_SIGS_PER_BLOCK = QUADS_PER_BLOCK / 2;       // two quads per signature

__device__ __forceinline__ uint32_t rsas_key(const uint32_t* __restrict__ key_idx, uint32_t op, uint32_t n_keys) {
  return key_idx ? min(key_idx[op], n_keys - 1u) : 0u;
}

// One thread per limb; the thread of limb 0 also writes the rule byte (rsas_rule).
__global__ void k_rsas_em(uint32_t n_ops, const uint8_t* __restrict__ digests, uint32_t dlen, uint32_t hash_id, const uint32_t* __restrict__ key_idx,
                          RsasKeys ks, uint32_t* __restrict__ c_limbs /*[n_ops][80]*/, uint8_t* __restrict__ rule /*[n_ops]*/) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ops * RSAS_VALUE_LIMBS) return;
  const uint32_t op = i / RSAS_VALUE_LIMBS, j = i % RSAS_VALUE_LIMBS;
  const uint32_t key = rsas_key(key_idx, op, ks.n_keys), k = ks.meta[key].y;
  c_limbs[i] = rsas_em_limb(j, k, hash_id, digests + (uint64_t)op * dlen, dlen);
  if (j == 0) rule[op] = rsas_rule(k, dlen + (uint32_t)rsav_prefix_len(hash_id), ks.refused[key] != 0);
}
__global__ void k_rsas_value(uint32_t n_ops, const uint8_t* __restrict__ c /*[n_ops][nbytes]*/, uint32_t nbytes, const uint32_t* __restrict__ key_idx,
                             RsasKeys ks, uint32_t* __restrict__ c_limbs, uint8_t* __restrict__ rule) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ops * RSAS_VALUE_LIMBS) return;
  const uint32_t op = i / RSAS_VALUE_LIMBS, j = i % RSAS_VALUE_LIMBS;
  c_limbs[i] = rsas_value_limb(j, c + (uint64_t)op * nbytes, nbytes);
  if (j == 0) rule[op] = ks.refused[rsas_key(key_idx, op, ks.n_keys)] ? RSAS_FENCED : RSAS_OK;
}

// x = a + 2n - z for lazily normal a, z below 2n: limb-wise in two's complement, then the signed carries hop lane to lane as in
// reduce_once.  The value is positive and below 4n, so nothing leaves the top lane.
template <int L>
__device__ __forceinline__ void rsas_sub_2n(uint32_t (&x)[L], const uint32_t (&a)[L], const uint32_t (&n)[L], const uint32_t (&z)[L], int qlane) {
#pragma unroll
  for (int k = 0; k < L; ++k) x[k] = a[k] + 2u * n[k] - z[k];
  int32_t cout = 0;
#pragma unroll
  for (int step = 0; step < RSAS_TPI; ++step) {
    int32_t c = (int32_t)dpp_quad_shr1((uint32_t)cout);
    if (qlane == 0) c = 0;
#pragma unroll
    for (int k = 0; k < L; ++k) {
      const int32_t v = (int32_t)x[k] + c;
      x[k] = (uint32_t)v & MONT_MASK;
      c = v >> MONT_W;                                        // arithmetic shift: negative = borrow
    }
    cout = c;
  }
}

// One signature per PAIR of quads of one wave: the even quad raises c mod p to dp, the odd one c mod q to dq, on the 10 x 4 form
// (40 limbs of 28 bits, R = 2^1120 > 2^96 p: mont_mul<10, 4>'s ring path; the model's figures: tests/test_rsa_sign_reference.py).
//   base      c = hi 2^1120 + lo:  mont(hi, R^3) + mont(lo, R^2) = c R mod m, below 4m
//   chain     window_chain (window_chain.h, with what depends on a secret and what does not) over the set's 2 pbytes windows
//   leave     mont(y, 1), canonical and below m: the odd quad's is m2
//   meet      m2 crosses through the odd quad's LDS slice (one wave: wavefront fences);  z = mont(m2, R^2 mod p);
//             x = y1 + 2p - z;  u = mont(x, qinv R);  h = mont(u, 1), canonical and below p
// The odd quad runs the meeting's products too, on operands of its own that nobody reads: the program counter stays wave-uniform.
//   products: 2 (base) + 14 (table) + 1 (one) + 2 pbytes * 5 + 1 (leave) + 3 (meeting)        1,301 per half at 128 bytes
// p, q, dp, dq and qinv are SECRETS.  The sequence of products follows from the set's pbytes alone, and the entry and exit products
// add no address that depends on one: the table row's (the digit) is the only one.
// Padding pairs (past the launch's signatures) run the last signature again on tables of their own and store nothing.
struct RsasChain {
  static constexpr int PRE = 2, POST = 3, L = RSAS_L;
  const uint32_t (&n)[L];
  const uint32_t *crow, *r2p, *r3p, *qinvp;         // this lane's limbs of c (low | high), R^2, R^3 and qinv R
  const uint8_t* erow;
  uint32_t pbytes;
  const uint32_t* a_odd;                            // the LDS slice of the pair's odd quad: where m2 crosses
  uint32_t* m2row;                                  // this lane's limbs of m2 in m2h
  bool half, active;
  int qlane;
  uint32_t keep[L];                                 // the base's high part, then y1
  __device__ __forceinline__ void pre_load(int step, uint32_t* a_lds, uint32_t (&y)[L]) const {      // hi * R^3, then lo * R^2
    const uint32_t *r2 = r2p, *r3 = r3p;
    const uint32_t *src = step == 0 ? crow + RSAS_N : crow, *rr = step == 0 ? r3 : r2;
#pragma unroll
    for (int k = 0; k < L; ++k) { a_lds[k] = src[k]; y[k] = rr[k]; }
  }
  __device__ __forceinline__ void pre_done(int step, uint32_t (&t)[L]) {
    if (step == 0) {
#pragma unroll
      for (int k = 0; k < L; ++k) keep[k] = t[k];
    } else {                                        // c R mod m below 4m: canonical, the base of the powers and row 1
#pragma unroll
      for (int k = 0; k < L; ++k) t[k] += keep[k];
      canonicalize<L, RSAS_TPI>(t, qlane);
    }
  }
  __device__ __forceinline__ uint32_t digit(uint32_t w) const { return rsas_digit(erow, pbytes, w); }
  // y: the power in Montgomery form, kept; t: the power itself, at most m
  __device__ __forceinline__ void leave_done(uint32_t (&t)[L], const uint32_t (&y)[L], uint32_t* a_lds) {
#pragma unroll
    for (int k = 0; k < L; ++k) keep[k] = y[k];
    canonicalize<L, RSAS_TPI>(t, qlane);
    reduce_once<L, RSAS_TPI>(t, n, qlane);
    if (half) {
#pragma unroll
      for (int k = 0; k < L; ++k) a_lds[k] = t[k];
      if (active) {
#pragma unroll
        for (int k = 0; k < L; ++k) m2row[k] = t[k];
      }
    }
  }
  // step 0: a = m2 in the odd quad's slice (written behind the leave), b = R^2;  1: a = x (written behind step 0), b = qinv R;
  // 2: mont(y, 1).  The members are read ahead of the branches, so that the object is taken apart into registers.
  __device__ __forceinline__ const uint32_t* post_load(int step) const {
    const uint32_t *r2 = r2p, *qi = qinvp;
    return step == 0 ? r2 : step == 1 ? qi : nullptr;
  }
  __device__ __forceinline__ const uint32_t* post_slice(int step, const uint32_t* a_own) const { return step == 0 ? a_odd : a_own; }
  __device__ __forceinline__ void post_done(int step, const uint32_t (&t)[L], uint32_t* a_lds) const {
    if (step != 0) return;
    uint32_t x[L];                                  // x = y1 + 2p - m2 R, canonical, below 4p
    rsas_sub_2n<L>(x, keep, n, t, qlane);
#pragma unroll
    for (int k = 0; k < L; ++k) a_lds[k] = x[k];
  }
};
__global__ void __launch_bounds__(RSA_BLOCK) k_rsas_crt(uint32_t n_here /*signatures of this launch*/, uint32_t first /*its first signature*/,
                                                        const uint32_t* __restrict__ key_idx, RsasKeys ks,
                                                        const uint32_t* __restrict__ c_limbs /*[n_ops][80]*/,
                                                        uint32_t* __restrict__ scratch /*[quads of the launch][16][40]*/,
                                                        uint32_t* __restrict__ m2h /*[n_ops][80]: m2 | h*/) {
  __shared__ uint32_t a_sh[QUADS_PER_BLOCK * RSAS_N];
  constexpr int L = RSAS_L;
  const uint32_t quad = threadIdx.x >> 2, half = quad & 1u;
  const int qlane = threadIdx.x & 3;
  const uint32_t lq = blockIdx.x * QUADS_PER_BLOCK + quad, ls = lq >> 1;
  const bool active = ls < n_here;
  const uint32_t op = first + (active ? ls : n_here - 1);
  const uint32_t key = rsas_key(key_idx, op, ks.n_keys);
  const uint64_t prow = ((uint64_t)key * 2 + half) * RSAS_N + qlane * L;      // this lane's limbs of its prime's rows
  uint32_t* a_lds = a_sh + quad * RSAS_N + qlane * L;
  const uint32_t* a_own = a_sh + quad * RSAS_N;
  const uint32_t* a_odd = a_sh + (quad | 1u) * RSAS_N;                        // the pair's odd quad: where m2 crosses
  const uint32_t* r2p = ks.r2 + prow;
  const uint32_t* crow = c_limbs + (uint64_t)op * RSAS_VALUE_LIMBS + qlane * L;
  const uint8_t* erow = ks.d + ((uint64_t)key * 2 + half) * ks.pbytes;
  uint32_t* tab = scratch + (uint64_t)lq * CHAIN_ENT * RSAS_N + qlane * L;   // this lane's limbs of row 0
  uint32_t n[L], t[L];
#pragma unroll
  for (int k = 0; k < L; ++k) n[k] = ks.mod[prow + k];
  const uint32_t n0inv = ks.n0inv[key * 2 + half];
  RsasChain pol{n, crow, r2p, ks.r3 + prow, ks.qinv_r + (uint64_t)key * RSAS_N + qlane * L, erow, ks.pbytes, a_odd,
                m2h + (uint64_t)op * RSAS_VALUE_LIMBS + qlane * L, half != 0u, active, qlane};
  window_chain<L, RSAS_TPI>(pol, a_lds, a_own, tab, r2p, n, n0inv, qlane, 2 * (int)ks.pbytes, t);
  canonicalize<L, RSAS_TPI>(t, qlane);
  reduce_once<L, RSAS_TPI>(t, n, qlane);
  if (!active || half) return;
#pragma unroll
  for (int k = 0; k < L; ++k) m2h[(uint64_t)op * RSAS_VALUE_LIMBS + RSAS_N + qlane * L + k] = t[k];
}

// s = m2 + h q: one thread per signature, the columns of the 40 x 40 product in order with one running carry (at most 40 products of
// 2^56 and a carry in a column: below 2^62).  fits = s < 2^(8 nbytes).
__global__ void __launch_bounds__(64) k_rsas_recombine(uint32_t n_ops, const uint32_t* __restrict__ key_idx, RsasKeys ks,
                                                       const uint32_t* __restrict__ m2h /*[n_ops][80]*/, uint32_t nbytes,
                                                       uint32_t* __restrict__ s_limbs /*[n_ops][80]*/, uint8_t* __restrict__ fits /*[n_ops]*/) {
  const uint32_t op = blockIdx.x * blockDim.x + threadIdx.x;
  if (op >= n_ops) return;
  constexpr int N = RSAS_N;
  const uint32_t* qrow = ks.mod + ((uint64_t)rsas_key(key_idx, op, ks.n_keys) * 2 + 1) * N;
  const uint32_t* mrow = m2h + (uint64_t)op * RSAS_VALUE_LIMBS;
  uint32_t h[N], q[N];
#pragma unroll
  for (int k = 0; k < N; ++k) { h[k] = mrow[N + k]; q[k] = qrow[k]; }
  const int32_t cut = 8 * (int32_t)nbytes;
  uint64_t carry = 0;
  uint32_t high = 0;
#pragma unroll
  for (int j = 0; j < 2 * N; ++j) {
    uint64_t acc = carry;
    if (j < N) acc += mrow[j];
#pragma unroll
    for (int i = (j < N ? 0 : j - N + 1); i <= (j < N ? j : N - 1); ++i) acc = mad64(h[i], q[j - i], acc);
    const uint32_t limb = (uint32_t)acc & MONT_MASK;
    carry = acc >> MONT_W;
    s_limbs[(uint64_t)op * RSAS_VALUE_LIMBS + j] = limb;
    const int32_t lo = j * MONT_W;
    if (lo + MONT_W > cut) high |= lo >= cut ? limb : limb >> (cut - lo);
  }
  fits[op] = (high == 0u && carry == 0u) ? 1u : 0u;
}

// one thread per byte: s_limbs -> nbytes big-endian bytes (what of s lies above the row is fits' business)
__global__ void k_rsas_bytes(const uint32_t* __restrict__ s_limbs, uint32_t nbytes, uint32_t n_ops, uint8_t* __restrict__ dst) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ops * nbytes) return;
  const uint32_t op = i / nbytes, k = i % nbytes;      // k: byte index from the LSB
  const uint32_t bit = k * 8, j = bit / MONT_W, sh = bit % MONT_W;
  const uint32_t* l = s_limbs + (uint64_t)op * RSAS_VALUE_LIMBS;
  uint64_t v = l[j];
  if (j + 1 < (uint32_t)RSAS_VALUE_LIMBS) v |= (uint64_t)l[j + 1] << MONT_W;
  dst[(uint64_t)op * nbytes + (nbytes - 1 - k)] = (uint8_t)(v >> sh);
}

// one thread per byte: the row of a signature whose status is not BFTKV_TH_OK is zeroed; the thread of a row's first byte writes the
// status.  check == nullptr (bftkv_gpu_selftest_rsa_crt): no check was run.
__global__ void k_rsas_finish(uint32_t n_ops, uint32_t nbytes, const uint8_t* __restrict__ rule, const uint8_t* __restrict__ fits,
                              const uint8_t* __restrict__ check, uint8_t* __restrict__ sig, uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ops * nbytes) return;
  const uint32_t op = i / nbytes;
  const uint8_t st = rsas_status(rule[op], fits[op] != 0, check ? check[op] != 0 : true);
  if (st != RSAS_OK) sig[i] = 0;
  if (i % nbytes == 0) status[op] = st;
}

}  // namespace bftkv

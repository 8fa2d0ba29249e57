// Threshold-ECDSA kernels (crypto/threshold/ecdsa/ecdsa.go), gfx950.  Field and point arithmetic: ec_field.h, templated on
// the curve's word count L (7, 8, 12, 17 for P-224, P-256, P-384, P-521).
//   k_ec_terms      thread / (operation, term): Unmarshal's checks on R_j, s_j = l_j w mod N, T_j = s_j R_j   CalculateR
//   k_ec_fold       thread / operation: S = T_0 + ... + T_(k-1) in j order with the fence rules, r = x(S) mod N
//   k_ec_calc_r_op  thread / operation: both of the above in one lane (the split for calls with many terms per SIMD)
//   k_ec_base_mult  thread / scalar: Marshal(s G)                                                             CalculatePartialR
// w = v^-1 mod N is folded into the per-term scalars: the curves have prime order, so sum (l_j w) R_j = w sum l_j R_j and
// the scaled prefix sums meet +-T_j and infinity exactly where the reference's unscaled ones do.
// Status bytes: bit 2 = fenced (the reference decides), bit 1 = v has no inverse (k_modinv's); copy_status normalises.
#pragma once
#include "ec_field.h"
// (kernels.hip and threshold_kernels.hip are included before this file by capi.hip)

namespace bftkv {

constexpr int EC_BLOCK = 64;

// radix-2^28 limbs (the Lagrange kernels' layout, value < 2^(32 L)) -> L words
template <int L>
__device__ __forceinline__ void ec_from_limbs28(uint32_t* w, const uint32_t* lim) {
  ecf::fe_zero<L>(w);
#pragma unroll
  for (int k = 0; k < (32 * L + 27) / 28; ++k) {
    const int bit = 28 * k, wi = bit >> 5, sh = bit & 31;
    const uint32_t v = lim[k];
    w[wi] |= v << sh;
    if (sh > 4 && wi + 1 < L) w[wi + 1] |= v >> (32 - sh);
  }
}

__device__ __forceinline__ void ec_fence(uint8_t* status, uint32_t op) {
  atomicOr((unsigned int*)(status + (op & ~3u)), 2u << (8 * (op & 3u)));
}

// w = v^-1 mod N of an operation; 1 where v = 0 (k_modinv has flagged it: the fold still runs, on the unscaled sums, because the
// fences precede ModInverse in the reference)
template <int L>
__device__ __forceinline__ void ec_load_w(uint32_t* w, const uint32_t* winv28) {
  ec_from_limbs28<L>(w, winv28);
  if (ecf::fe_is_zero<L>(w)) w[0] = 1;
}

// One term: Unmarshal's checks on R_j (prefix 0x04, coordinates below P, on the curve), l_j != 0, T_j = (l_j w mod N) R_j.
// false: fenced.
template <int L>
__device__ __forceinline__ bool ec_term(ecf::Jac<L>& T, const uint8_t* rb, const uint32_t* lam28, const uint32_t* w, const ecf::Curve<L>& C) {
  const uint32_t f = C.fbytes;
  uint32_t x[L], y[L];
  ecf::Jac<L> R;
  if (rb[0] != 4) return false;
  ecf::fe_from_be<L>(x, rb + 1, f);
  ecf::fe_from_be<L>(y, rb + 1 + f, f);
  if (!ecf::pt_check<L>(R.x, R.y, x, y, C)) return false;
  ecf::fe_copy<L>(R.z, C.one);
  ec_from_limbs28<L>(x, lam28);
  if (ecf::fe_is_zero<L>(x)) return false;               // l_j = 0: the term (0, 0) goes into Add
  ecf::fn_mul<L>(y, x, w, C);
  ecf::pt_mul<L>(T, R, y, C);
  return true;
}

// r = x(S) mod N; x < P < 2N, so one conditional subtraction.  Infinity (the last fold met -T) gives 0.
template <int L>
__device__ __forceinline__ void ec_r_of(uint32_t* r, const ecf::Jac<L>& S, const ecf::Curve<L>& C) {
  uint32_t x[L], y[L];
  ecf::pt_affine<L>(x, y, S, C);
  if (!ecf::fe_lt<L>(x, C.n)) {
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < L; ++i) { const uint64_t v = (uint64_t)x[i] - C.n[i] - br; x[i] = (uint32_t)v; br = v >> 63; }
  }
  ecf::fe_copy<L>(r, x);
}

// One fold step S += T_j (j >= 1) under the fence rules: S_(j-1) = T_j (Add's doubling case) and a prefix sum at infinity
// before the last term are fenced; infinity after the last term is the answer r = 0.  false: fenced.
template <int L>
__device__ __forceinline__ bool ec_fold_step(ecf::Jac<L>& S, const ecf::Jac<L>& T, uint32_t j, uint32_t k, const ecf::Curve<L>& C) {
  const int code = ecf::pt_add<L>(S, S, T, C);
  return !(code == ecf::EC_ADD_EQUAL || code == ecf::EC_ADD_INF_OPERAND || (code == ecf::EC_ADD_OPPOSITE && j + 1 < k));
}

template <int L>
__device__ __forceinline__ void ec_store_jac(uint32_t* d, const ecf::Jac<L>& P) {
#pragma unroll
  for (int i = 0; i < L; ++i) { d[i] = P.x[i]; d[L + i] = P.y[i]; d[2 * L + i] = P.z[i]; }
}
template <int L>
__device__ __forceinline__ void ec_load_jac(ecf::Jac<L>& P, const uint32_t* s) {
#pragma unroll
  for (int i = 0; i < L; ++i) { P.x[i] = s[i]; P.y[i] = s[L + i]; P.z[i] = s[2 * L + i]; }
}

template <int L>
__global__ void __launch_bounds__(EC_BLOCK) k_ec_terms(uint32_t n_ops, uint32_t k, const uint8_t* __restrict__ ri /*[n_ops][k][1 + 2 f]*/,
                                                       const uint32_t* __restrict__ lam28 /*[n_ops][k][76]*/, const uint32_t* __restrict__ winv28 /*[n_ops][76]*/,
                                                       ecf::Curve<L> C, uint32_t* __restrict__ t_out /*[n_ops][k][3 L]*/, uint8_t* __restrict__ status) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_ops * k) return;
  const uint32_t op = t / k;
  uint32_t w[L];
  ec_load_w<L>(w, winv28 + (uint64_t)op * MONT_N);
  ecf::Jac<L> T;
  if (!ec_term<L>(T, ri + (uint64_t)t * (1 + 2 * C.fbytes), lam28 + (uint64_t)t * MONT_N, w, C)) {
    ecf::pt_set_inf<L>(T);
    ec_fence(status, op);
  }
  ec_store_jac<L>(t_out + (uint64_t)t * 3 * L, T);
}

// (runs behind k_ec_terms: a fenced term has already set its operation's bit 2)
template <int L>
__global__ void __launch_bounds__(EC_BLOCK) k_ec_fold(uint32_t n_ops, uint32_t k, const uint32_t* __restrict__ t_in, ecf::Curve<L> C,
                                                      uint8_t* __restrict__ status, uint8_t* __restrict__ r_out /*[n_ops][f]*/) {
  const uint32_t op = blockIdx.x * blockDim.x + threadIdx.x;
  if (op >= n_ops) return;
  uint32_t r[L];
  ecf::fe_zero<L>(r);
  uint8_t st = status[op];
  if (!(st & 2u)) {
    const uint32_t* tp = t_in + (uint64_t)op * k * 3 * L;
    ecf::Jac<L> S, T;
    ec_load_jac<L>(S, tp);
    bool ok = true;
    for (uint32_t j = 1; j < k && ok; ++j) {
      ec_load_jac<L>(T, tp + (uint64_t)j * 3 * L);
      ok = ec_fold_step<L>(S, T, j, k, C);
    }
    if (ok) ec_r_of<L>(r, S, C);
    else st |= 2u;
    status[op] = st;               // (this thread's byte alone: the term kernel's atomics are done)
  }
  if (st) ecf::fe_zero<L>(r);
  ecf::fe_to_be<L>(r_out + (uint64_t)op * C.fbytes, C.fbytes, r);
}

template <int L>
__global__ void __launch_bounds__(EC_BLOCK) k_ec_calc_r_op(uint32_t n_ops, uint32_t k, const uint8_t* __restrict__ ri, const uint32_t* __restrict__ lam28,
                                                           const uint32_t* __restrict__ winv28, ecf::Curve<L> C, uint8_t* __restrict__ status,
                                                           uint8_t* __restrict__ r_out) {
  const uint32_t op = blockIdx.x * blockDim.x + threadIdx.x;
  if (op >= n_ops) return;
  uint32_t r[L];
  ecf::fe_zero<L>(r);
  uint8_t st = status[op];
  if (!(st & 2u)) {
    uint32_t w[L];
    ec_load_w<L>(w, winv28 + (uint64_t)op * MONT_N);
    ecf::Jac<L> S, T;
    bool ok = true;
    for (uint32_t j = 0; j < k && ok; ++j) {
      const uint64_t t = (uint64_t)op * k + j;
      ok = ec_term<L>(j ? T : S, ri + t * (1 + 2 * C.fbytes), lam28 + t * MONT_N, w, C);
      if (ok && j) ok = ec_fold_step<L>(S, T, j, k, C);
    }
    if (ok) ec_r_of<L>(r, S, C);
    else st |= 2u;
    status[op] = st;
  }
  if (st) ecf::fe_zero<L>(r);
  ecf::fe_to_be<L>(r_out + (uint64_t)op * C.fbytes, C.fbytes, r);
}

// Marshal(ScalarBaseMult(s)) for s < N (big-endian, sbytes <= f); s >= N is fenced (never a share mod N) and left zero
template <int L>
__global__ void __launch_bounds__(EC_BLOCK) k_ec_base_mult(uint32_t n_ops, const uint8_t* __restrict__ sc, uint32_t sbytes, ecf::Curve<L> C,
                                                           uint8_t* __restrict__ out /*[n_ops][1 + 2 f]*/, uint8_t* __restrict__ status) {
  const uint32_t op = blockIdx.x * blockDim.x + threadIdx.x;
  if (op >= n_ops) return;
  const uint32_t f = C.fbytes;
  uint8_t* o = out + (uint64_t)op * (1 + 2 * f);
  uint32_t s[L], x[L], y[L];
  ecf::fe_from_be<L>(s, sc + (uint64_t)op * sbytes, sbytes);
  if (!ecf::fe_lt<L>(s, C.n)) {
    for (uint32_t i = 0; i < 1 + 2 * f; ++i) o[i] = 0;
    status[op] = BFTKV_TH_FENCED;
    return;
  }
  ecf::Jac<L> G, Q;
  ecf::fe_copy<L>(G.x, C.gx);
  ecf::fe_copy<L>(G.y, C.gy);
  ecf::fe_copy<L>(G.z, C.one);
  ecf::pt_mul<L>(Q, G, s, C);
  ecf::pt_affine<L>(x, y, Q, C);                            // s = 0: (0, 0), Marshal's 04 || 0...0
  o[0] = 4;
  ecf::fe_to_be<L>(o + 1, f, x);
  ecf::fe_to_be<L>(o + 1 + f, f, y);
  status[op] = BFTKV_TH_OK;
}

}  // namespace bftkv

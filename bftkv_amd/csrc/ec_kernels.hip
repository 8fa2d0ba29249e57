// Threshold-ECDSA kernels (crypto/threshold/ecdsa/ecdsa.go), gfx950.  Field and point arithmetic: ec_field.h, templated on
// the curve's word count L (7, 8, 12, 17 for P-224, P-256, P-384, P-521).
//   k_ec_terms      thread / (operation, term): Unmarshal's checks on R_j, s_j = l_j w mod N, T_j = s_j R_j   CalculateR
//   k_ec_fold       thread / operation: S = T_0 + ... + T_(k-1) in j order with the fence rules, r = x(S) mod N
//   k_ec_calc_r_op  thread / operation: both of the above in one lane (the split for calls with many terms per SIMD)
//   k_ec_base_mult  thread / scalar: Marshal(s G)                                                             CalculatePartialR
//   k_ecv_prep / k_ecv_base / k_ecv_key   thread / signature: ecdsa.Verify on raw r || s (further down)        Verify
//   k_ec_keytab_build / k_ecv_key_tab     resident key sets: a table per key, u2 Q from it (at the end)         Verify
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

// ---- ECDSA verification (crypto/ecdsa.Verify, Go 1.13): a thread per signature in three kernels around k_modinv -------------
//   k_ecv_prep   range checks on r and s, e = hashToInt(digest) mod N, r and e as words, s as radix-2^28 limbs for k_modinv
//   k_ecv_base   u1 = e w, u2 = r w mod N, u1 G from the curve's fixed-base table (fb_mul)          -> HBM
//   k_ecv_key    Unmarshal's checks on the key, u2 Q (pt_mul), ONE pt_add of the two multiples, the x comparison, the verdict
// The two multiples stay separate points until that last addition: its case code is the fence (u1 G = u2 Q is Add's doubling
// case) and the INVALID of a sum at infinity.  They meet through HBM because a P-521 lane cannot hold the finished u1 G (51
// words) beside pt_mul's working set without scratch.
// flag byte of an operation: 0 go on, 1 decided INVALID (r or s outside [1, N)), 2 fenced (e = 0 mod N)
enum { ECV_GO = 0, ECV_INVALID = 1, ECV_FENCED = 2 };

template <int L>
__device__ __forceinline__ void ec_to_limbs28(uint32_t* lim, const uint32_t* w) {
#pragma unroll
  for (int k = 0; k < MONT_N; ++k) {
    const int bit = 28 * k, wi = bit >> 5, sh = bit & 31;
    uint32_t v = 0;
    if (wi < L) v = w[wi] >> sh;
    if (sh > 4 && wi + 1 < L) v |= w[wi + 1] << (32 - sh);
    lim[k] = v & 0x0FFFFFFFu;
  }
}

template <int L>
__global__ void __launch_bounds__(EC_BLOCK) k_ecv_prep(uint32_t n_ops, const uint8_t* __restrict__ digests /*[n_ops][dlen]*/, uint32_t dlen, uint32_t bits,
                                                       const uint8_t* __restrict__ sigs /*[n_ops][2 f]*/, ecf::Curve<L> C,
                                                       uint32_t* __restrict__ s28 /*[n_ops][76]*/, uint32_t* __restrict__ e_out /*[n_ops][L]*/,
                                                       uint32_t* __restrict__ r_out /*[n_ops][L]*/, uint8_t* __restrict__ flag) {
  const uint32_t op = blockIdx.x * blockDim.x + threadIdx.x;
  if (op >= n_ops) return;
  const uint32_t f = C.fbytes;
  uint32_t r[L], s[L], e[L];
  ecf::fe_from_be<L>(r, sigs + (uint64_t)op * 2 * f, f);
  ecf::fe_from_be<L>(s, sigs + (uint64_t)op * 2 * f + f, f);
  ecf::hash_to_int<L>(e, digests + (uint64_t)op * dlen, dlen, bits, C);
  uint8_t fl = ECV_GO;
  if (ecf::fe_is_zero<L>(r) || ecf::fe_is_zero<L>(s) || !ecf::fe_lt<L>(r, C.n) || !ecf::fe_lt<L>(s, C.n)) fl = ECV_INVALID;
  else if (ecf::fe_is_zero<L>(e)) fl = ECV_FENCED;         // u1 = 0: the affine (0, 0) would go into Add
  if (fl) { ecf::fe_zero<L>(s); s[0] = 1; }               // (k_modinv still runs on the lane: give it an invertible number)
  ec_to_limbs28<L>(s28 + (uint64_t)op * MONT_N, s);
#pragma unroll
  for (int i = 0; i < L; ++i) { e_out[(uint64_t)op * L + i] = e[i]; r_out[(uint64_t)op * L + i] = r[i]; }
  flag[op] = fl;
}

template <int L>
__global__ void __launch_bounds__(EC_BLOCK) k_ecv_base(uint32_t n_ops, const uint32_t* __restrict__ r_in, const uint32_t* __restrict__ e_in,
                                                       const uint32_t* __restrict__ winv28, const uint8_t* __restrict__ flag, ecf::Curve<L> C,
                                                       const uint32_t* __restrict__ tab, uint32_t w, uint32_t nwin,
                                                       uint32_t* __restrict__ pt_out /*[n_ops][3 L]*/, uint32_t* __restrict__ u2_out /*[n_ops][L]*/) {
  const uint32_t op = blockIdx.x * blockDim.x + threadIdx.x;
  if (op >= n_ops || flag[op]) return;
  uint32_t wv[L], u[L], t[L];
  ec_from_limbs28<L>(wv, winv28 + (uint64_t)op * MONT_N);
#pragma unroll
  for (int i = 0; i < L; ++i) t[i] = r_in[(uint64_t)op * L + i];
  ecf::fn_mul<L>(u, t, wv, C);                              // u2 = r w
#pragma unroll
  for (int i = 0; i < L; ++i) u2_out[(uint64_t)op * L + i] = u[i];
#pragma unroll
  for (int i = 0; i < L; ++i) t[i] = e_in[(uint64_t)op * L + i];
  ecf::fn_mul<L>(u, t, wv, C);                              // u1 = e w  (not 0: e != 0 and N is prime)
  ecf::Jac<L> P;
  ecf::fb_mul<L>(P, tab, w, nwin, u, C);
  ec_store_jac<L>(pt_out + (uint64_t)op * 3 * L, P);
}

// (inv_bad: k_modinv's byte array, set only if s had no inverse -- N is prime, so never; such an operation stays BFTKV_TH_FAILED)
template <int L>
__global__ void __launch_bounds__(EC_BLOCK) k_ecv_key(uint32_t n_ops, const uint32_t* __restrict__ r_in, const uint8_t* __restrict__ keys /*[n_keys][1 + 2 f]*/,
                                                      const uint32_t* __restrict__ key_idx, uint32_t n_keys, const uint32_t* __restrict__ u2_in,
                                                      const uint32_t* __restrict__ pt_in, const uint8_t* __restrict__ flag,
                                                      const uint8_t* __restrict__ inv_bad, ecf::Curve<L> C, uint8_t* __restrict__ valid_out,
                                                      uint8_t* __restrict__ status_out) {
  const uint32_t op = blockIdx.x * blockDim.x + threadIdx.x;
  if (op >= n_ops) return;
  const uint32_t f = C.fbytes;
  const uint8_t* kb = keys + (uint64_t)(key_idx ? min(key_idx[op], n_keys - 1u) : 0u) * (1 + 2 * f);
  uint8_t valid = 0, st = BFTKV_TH_OK;
  const uint8_t fl = flag[op];
  uint32_t x[L], y[L];
  ecf::Jac<L> Q, A;
  ecf::fe_from_be<L>(x, kb + 1, f);
  ecf::fe_from_be<L>(y, kb + 1 + f, f);
  if (kb[0] != 4 || !ecf::pt_check<L>(Q.x, Q.y, x, y, C)) st = BFTKV_TH_FENCED;       // no reference key object holds this point
  else if (fl == ECV_FENCED) st = BFTKV_TH_FENCED;
  else if (inv_bad[op]) st = BFTKV_TH_FAILED;
  else if (fl == ECV_GO) {
    ecf::fe_copy<L>(Q.z, C.one);
#pragma unroll
    for (int i = 0; i < L; ++i) x[i] = u2_in[(uint64_t)op * L + i];
    ecf::pt_mul<L>(A, Q, x, C);                              // u2 Q: finite (0 < u2 < N, prime order)
    ec_load_jac<L>(Q, pt_in + (uint64_t)op * 3 * L);         // u1 G
    const int code = ecf::pt_add<L>(A, Q, A, C);
    if (code == ecf::EC_ADD_EQUAL) st = BFTKV_TH_FENCED;     // Add's doubling case on the generic path
    else if (code == ecf::EC_ADD_GENERAL) {                  // (opposite: the sum is infinity, INVALID)
#pragma unroll
      for (int i = 0; i < L; ++i) x[i] = r_in[(uint64_t)op * L + i];
      valid = ecf::x_matches_r<L>(A, x, C) ? 1 : 0;
    }
  }
  valid_out[op] = valid;
  status_out[op] = st;
}

// ---- resident key sets (bftkv_gpu_ecdsa_keyset_*): a fixed-base table per key, built once on the device ------------------------
// k_ec_keytab_build, a lane per (key, window i): Unmarshal's checks on the key (a refused key sets its byte and leaves its rows
// zero), B = 2^(w i) Q by w i doublings, the multiples j B (j = 1 .. 2^w - 1) by the exact pt_add, made affine with one inversion
// per lane (Montgomery's trick over the row; no Z is zero, ec_field.h fb_table_build).  The Jacobian X, Y wait in the row's own
// table slots, Z and the running products of Z in tmp ([2^w - 1][2 L][n_lanes] words: a wave's stores are contiguous).  The result
// is the table of fb_table_build with base Q, word for word: the affine Montgomery words are fully reduced, hence unique.
// The lanes of a wave double a different number of times; registration is off the hot path and the worst lane costs one ladder's
// doublings.  tab arrives zeroed (slot 0 of every run and the rows of refused keys stay zero).
template <int L>
__global__ void __launch_bounds__(EC_BLOCK) k_ec_keytab_build(uint32_t n_keys, const uint8_t* __restrict__ keys /*[n_keys][1 + 2 f]*/, ecf::Curve<L> C,
                                                              uint32_t w, uint32_t nwin, uint32_t* __restrict__ tmp,
                                                              uint32_t* __restrict__ tab /*[n_keys][fb_table_words]*/, uint8_t* __restrict__ refused) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, n_lanes = n_keys * nwin;
  if (t >= n_lanes) return;
  const uint32_t key = t / nwin, i = t % nwin, f = C.fbytes, per = (1u << w) - 1u;
  const uint8_t* kb = keys + (uint64_t)key * (1 + 2 * f);
  uint32_t a[L], b[L];
  ecf::Jac<L> B, P;
  ecf::fe_from_be<L>(a, kb + 1, f);
  ecf::fe_from_be<L>(b, kb + 1 + f, f);
  const bool ok = kb[0] == 4 && ecf::pt_check<L>(B.x, B.y, a, b, C);
  if (i == 0) refused[key] = ok ? 0 : 1;
  if (!ok) return;
  ecf::fe_copy<L>(B.z, C.one);
  for (uint32_t d = 0; d < w * i; ++d) ecf::pt_dbl<L>(B, B, C);
  uint32_t* row = tab + (uint64_t)key * ecf::fb_table_words<L>(w, nwin) + (((size_t)i * 2 * L) << w);
  uint32_t* zs = tmp + t;                                    // word k of Z_j: zs[(j 2L + k) n_lanes], of Z_0 .. Z_j: k + L
  P = B;
  ecf::fe_copy<L>(a, B.z);                                   // a: Z_0 ... Z_j
  for (uint32_t j = 0; j < per; ++j) {
    if (j) { ecf::pt_add<L>(P, P, B, C); ecf::fp_mul<L>(a, a, P.z, C); }
#pragma unroll
    for (int k = 0; k < L; ++k) {
      row[((size_t)k << w) + j + 1] = P.x[k];
      row[((size_t)(L + k) << w) + j + 1] = P.y[k];
      zs[((uint64_t)j * 2 * L + k) * n_lanes] = P.z[k];
      zs[((uint64_t)j * 2 * L + L + k) * n_lanes] = a[k];
    }
  }
  uint32_t inv[L], zi[L];
  ecf::fp_inv<L>(inv, a, C);                                 // 1 / (Z_0 ... Z_(per-1))
  for (uint32_t j = per; j-- > 0;) {
    if (j) {
#pragma unroll
      for (int k = 0; k < L; ++k) { a[k] = zs[((uint64_t)(j - 1) * 2 * L + L + k) * n_lanes]; b[k] = zs[((uint64_t)j * 2 * L + k) * n_lanes]; }
      ecf::fp_mul<L>(zi, inv, a, C);                         // 1 / Z_j
      ecf::fp_mul<L>(inv, inv, b, C);
    } else ecf::fe_copy<L>(zi, inv);
#pragma unroll
    for (int k = 0; k < L; ++k) { a[k] = row[((size_t)k << w) + j + 1]; b[k] = row[((size_t)(L + k) << w) + j + 1]; }
    ecf::fp_sqr<L>(P.z, zi, C);                              // (P is free in this pass: 1 / Z_j^2, then 1 / Z_j^3)
    ecf::fp_mul<L>(a, a, P.z, C);
    ecf::fp_mul<L>(P.z, P.z, zi, C);
    ecf::fp_mul<L>(b, b, P.z, C);
#pragma unroll
    for (int k = 0; k < L; ++k) { row[((size_t)k << w) + j + 1] = a[k]; row[((size_t)(L + k) << w) + j + 1] = b[k]; }
  }
}

// k_ecv_key with the key's table in place of the ladder: stands behind the same k_ecv_prep, k_modinv and k_ecv_base.  A key
// refused at registration fences every signature that names it, before any other rule; u2 Q comes from fb_mul over the key's
// table (set_tab + key * fb_table_words), and the two multiples still meet in ONE pt_add whose case code is the fence.
template <int L>
__global__ void __launch_bounds__(EC_BLOCK) k_ecv_key_tab(uint32_t n_ops, const uint32_t* __restrict__ r_in, const uint32_t* __restrict__ set_tab,
                                                          const uint8_t* __restrict__ refused /*[n_keys]*/, const uint32_t* __restrict__ key_idx,
                                                          uint32_t n_keys, uint32_t w, uint32_t nwin, const uint32_t* __restrict__ u2_in,
                                                          const uint32_t* __restrict__ pt_in, const uint8_t* __restrict__ flag,
                                                          const uint8_t* __restrict__ inv_bad, ecf::Curve<L> C, uint8_t* __restrict__ valid_out,
                                                          uint8_t* __restrict__ status_out) {
  const uint32_t op = blockIdx.x * blockDim.x + threadIdx.x;
  if (op >= n_ops) return;
  const uint32_t key = key_idx ? min(key_idx[op], n_keys - 1u) : 0u;
  uint8_t valid = 0, st = BFTKV_TH_OK;
  const uint8_t fl = flag[op];
  if (refused[key]) st = BFTKV_TH_FENCED;                    // no reference key object holds this point
  else if (fl == ECV_FENCED) st = BFTKV_TH_FENCED;
  else if (inv_bad[op]) st = BFTKV_TH_FAILED;
  else if (fl == ECV_GO) {
    uint32_t x[L];
    ecf::Jac<L> Q, A;
#pragma unroll
    for (int i = 0; i < L; ++i) x[i] = u2_in[(uint64_t)op * L + i];
    ecf::fb_mul<L>(A, set_tab + (uint64_t)key * ecf::fb_table_words<L>(w, nwin), w, nwin, x, C);      // u2 Q: finite (0 < u2 < N)
    ec_load_jac<L>(Q, pt_in + (uint64_t)op * 3 * L);         // u1 G
    const int code = ecf::pt_add<L>(A, Q, A, C);
    if (code == ecf::EC_ADD_EQUAL) st = BFTKV_TH_FENCED;     // Add's doubling case on the generic path
    else if (code == ecf::EC_ADD_GENERAL) {                  // (opposite: the sum is infinity, INVALID)
#pragma unroll
      for (int i = 0; i < L; ++i) x[i] = r_in[(uint64_t)op * L + i];
      valid = ecf::x_matches_r<L>(A, x, C) ? 1 : 0;
    }
  }
  valid_out[op] = valid;
  status_out[op] = st;
}

}  // namespace bftkv

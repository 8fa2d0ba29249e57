// Field and point arithmetic of the NIST prime curves (crypto/elliptic's P-224, P-256, P-384, P-521: a = -3, prime order,
// cofactor 1) for the threshold-ECDSA kernels of ec_kernels.hip.  The same text compiles for the host (tests/c/ec_host.cpp
// checks it against the Python restatement in the CPU suite), so everything here is plain C++ behind EC_HD.
//
// Field elements are L little-endian 32-bit words (L = 7, 8, 12, 17), kept fully reduced in [0, p) in Montgomery form
// (R = 2^(32 L)): one product is CIOS Montgomery, 2 L^2 32x32->64 multiply-adds (one v_mad_u64_u32 each), and a reduced
// representation makes "is zero" and "equal" plain word compares -- what the exceptional cases of point addition need.
// Points are Jacobian (X : Y : Z), Z = 0 is the point at infinity.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#ifndef EC_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define EC_HD __host__ __device__ __forceinline__
#else
#define EC_HD static inline
#endif
#endif

namespace ecf {

template <int L>
struct Curve {
  static constexpr int kWords = L;
  uint32_t p[L], n[L];        // field prime, group order
  uint32_t rr_p[L], rr_n[L];  // R^2 mod p, R^2 mod n
  uint32_t one[L];            // R mod p (1 in Montgomery form)
  uint32_t b[L];              // B R mod p
  uint32_t gx[L], gy[L];      // the base point, Montgomery form
  uint32_t pm2[L];            // p - 2 (Fermat's exponent)
  uint32_t p0inv, n0inv;      // -p^-1, -n^-1 mod 2^32
  uint32_t fbytes;            // (BitSize + 7) / 8
};

template <int L>
struct Jac {
  uint32_t x[L], y[L], z[L];
};

// ---- words -----------------------------------------------------------------------------------------------------------
template <int L>
EC_HD void fe_copy(uint32_t* r, const uint32_t* a) {
#pragma unroll
  for (int i = 0; i < L; ++i) r[i] = a[i];
}
template <int L>
EC_HD void fe_zero(uint32_t* r) {
#pragma unroll
  for (int i = 0; i < L; ++i) r[i] = 0;
}
template <int L>
EC_HD bool fe_is_zero(const uint32_t* a) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < L; ++i) o |= a[i];
  return o == 0;
}
template <int L>
EC_HD bool fe_eq(const uint32_t* a, const uint32_t* b) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < L; ++i) o |= a[i] ^ b[i];
  return o == 0;
}
template <int L>
EC_HD bool fe_lt(const uint32_t* a, const uint32_t* m) {        // a < m
  uint64_t br = 0;
#pragma unroll
  for (int i = 0; i < L; ++i) br = ((uint64_t)a[i] - m[i] - br) >> 63;
  return br != 0;
}
// big-endian bytes (len <= 4 L) -> words
template <int L>
EC_HD void fe_from_be(uint32_t* r, const uint8_t* s, uint32_t len) {
  fe_zero<L>(r);
  for (uint32_t i = 0; i < len; ++i) {
    const uint32_t bit = 8u * (len - 1u - i);
    r[bit >> 5] |= (uint32_t)s[i] << (bit & 31u);
  }
}
template <int L>
EC_HD void fe_to_be(uint8_t* d, uint32_t len, const uint32_t* a) {
  for (uint32_t i = 0; i < len; ++i) {
    const uint32_t bit = 8u * (len - 1u - i);
    d[i] = (uint8_t)(a[bit >> 5] >> (bit & 31u));
  }
}

// ---- arithmetic mod m (inputs in [0, m)) --------------------------------------------------------------------------
template <int L>
EC_HD void fe_add(uint32_t* r, const uint32_t* a, const uint32_t* b, const uint32_t* m) {
  uint32_t s[L], d[L];
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < L; ++i) { c += (uint64_t)a[i] + b[i]; s[i] = (uint32_t)c; c >>= 32; }
  uint64_t br = 0;
#pragma unroll
  for (int i = 0; i < L; ++i) { const uint64_t v = (uint64_t)s[i] - m[i] - br; d[i] = (uint32_t)v; br = v >> 63; }
  const bool use_d = c || !br;     // a + b >= m
#pragma unroll
  for (int i = 0; i < L; ++i) r[i] = use_d ? d[i] : s[i];
}
template <int L>
EC_HD void fe_sub(uint32_t* r, const uint32_t* a, const uint32_t* b, const uint32_t* m) {
  uint32_t d[L];
  uint64_t br = 0;
#pragma unroll
  for (int i = 0; i < L; ++i) { const uint64_t v = (uint64_t)a[i] - b[i] - br; d[i] = (uint32_t)v; br = v >> 63; }
  const uint32_t mask = br ? 0xFFFFFFFFu : 0u;
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < L; ++i) { c += (uint64_t)d[i] + (m[i] & mask); r[i] = (uint32_t)c; c >>= 32; }
}
// CIOS Montgomery product a b R^-1 mod m (a, b < m < 2^(32 L)); r may alias a or b.  The outer loop stays rolled (the
// product is inlined some forty times per kernel) and walks b by rotating a copy, so every index is a constant and nothing
// leaves registers.
template <int L>
EC_HD void fe_mul(uint32_t* r, const uint32_t* a, const uint32_t* b, const uint32_t* m, uint32_t m0inv) {
  uint32_t t[L + 2], bw[L];
#pragma unroll
  for (int j = 0; j < L + 2; ++j) t[j] = 0;
#pragma unroll
  for (int j = 0; j < L; ++j) bw[j] = b[j];
#pragma unroll 1
  for (int i = 0; i < L; ++i) {
    const uint32_t bi = bw[0];
#pragma unroll
    for (int j = 0; j + 1 < L; ++j) bw[j] = bw[j + 1];
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < L; ++j) { c = (uint64_t)a[j] * bi + t[j] + (c >> 32); t[j] = (uint32_t)c; }
    c = (uint64_t)t[L] + (c >> 32);
    t[L] = (uint32_t)c;
    t[L + 1] = (uint32_t)(c >> 32);
    const uint32_t q = t[0] * m0inv;
    c = (uint64_t)q * m[0] + t[0];
#pragma unroll
    for (int j = 1; j < L; ++j) { c = (uint64_t)q * m[j] + t[j] + (c >> 32); t[j - 1] = (uint32_t)c; }
    c = (uint64_t)t[L] + (c >> 32);
    t[L - 1] = (uint32_t)c;
    t[L] = t[L + 1] + (uint32_t)(c >> 32);
  }
  uint32_t d[L];       // t < 2m: one conditional subtraction
  uint64_t br = 0;
#pragma unroll
  for (int i = 0; i < L; ++i) { const uint64_t v = (uint64_t)t[i] - m[i] - br; d[i] = (uint32_t)v; br = v >> 63; }
  const bool use_d = t[L] || !br;
#pragma unroll
  for (int i = 0; i < L; ++i) r[i] = use_d ? d[i] : t[i];
}

template <int L> EC_HD void fp_mul(uint32_t* r, const uint32_t* a, const uint32_t* b, const Curve<L>& C) { fe_mul<L>(r, a, b, C.p, C.p0inv); }
template <int L> EC_HD void fp_sqr(uint32_t* r, const uint32_t* a, const Curve<L>& C) { fe_mul<L>(r, a, a, C.p, C.p0inv); }
template <int L> EC_HD void fp_add(uint32_t* r, const uint32_t* a, const uint32_t* b, const Curve<L>& C) { fe_add<L>(r, a, b, C.p); }
template <int L> EC_HD void fp_sub(uint32_t* r, const uint32_t* a, const uint32_t* b, const Curve<L>& C) { fe_sub<L>(r, a, b, C.p); }

// a^(p-2) = a^-1 (Montgomery form in and out; 0 -> 0): left-to-right square and multiply over the bits of p - 2
template <int L>
EC_HD void fp_inv(uint32_t* r, const uint32_t* a, const Curve<L>& C) {
  uint32_t acc[L];
  fe_copy<L>(acc, C.one);
  for (int i = 32 * L - 1; i >= 0; --i) {
    fp_sqr<L>(acc, acc, C);
    if ((C.pm2[i >> 5] >> (i & 31)) & 1u) fp_mul<L>(acc, acc, a, C);
  }
  fe_copy<L>(r, acc);
}

// ---- points --------------------------------------------------------------------------------------------------------
template <int L>
EC_HD bool pt_is_inf(const Jac<L>& P) { return fe_is_zero<L>(P.z); }
template <int L>
EC_HD void pt_set_inf(Jac<L>& P) { fe_zero<L>(P.x); fe_zero<L>(P.y); fe_zero<L>(P.z); }

// 2P with a = -3 (dbl-2001-b, the formula of Go's doubleJacobian); infinity stays infinity (Z3 = (Y+0)^2 - Y^2 = 0).  The
// curves have prime order, so no finite point has Y = 0.  R may alias P.
template <int L>
EC_HD void pt_dbl(Jac<L>& R, const Jac<L>& P, const Curve<L>& C) {
  uint32_t delta[L], gamma[L], beta[L], alpha[L], t[L], u[L];
  fp_sqr<L>(delta, P.z, C);
  fp_sqr<L>(gamma, P.y, C);
  fp_mul<L>(beta, P.x, gamma, C);
  fp_sub<L>(t, P.x, delta, C);
  fp_add<L>(u, P.x, delta, C);
  fp_mul<L>(alpha, t, u, C);
  fp_add<L>(t, alpha, alpha, C);
  fp_add<L>(alpha, alpha, t, C);                        // alpha = 3 (X - delta)(X + delta)
  fp_add<L>(u, P.y, P.z, C);
  fp_sqr<L>(u, u, C);
  fp_sub<L>(u, u, gamma, C);
  fp_sub<L>(R.z, u, delta, C);                          // Z3 = (Y + Z)^2 - gamma - delta   (P.z is dead from here)
  fp_add<L>(beta, beta, beta, C);
  fp_add<L>(beta, beta, beta, C);                       // 4 beta
  fp_sqr<L>(t, alpha, C);
  fp_add<L>(u, beta, beta, C);
  fp_sub<L>(R.x, t, u, C);                              // X3 = alpha^2 - 8 beta
  fp_sub<L>(t, beta, R.x, C);
  fp_mul<L>(t, alpha, t, C);
  fp_sqr<L>(gamma, gamma, C);
  fp_add<L>(gamma, gamma, gamma, C);
  fp_add<L>(gamma, gamma, gamma, C);
  fp_add<L>(gamma, gamma, gamma, C);                    // 8 gamma^2
  fp_sub<L>(R.y, t, gamma, C);                          // Y3 = alpha (4 beta - X3) - 8 gamma^2
}

// What pt_add met (the fold's fence rules need to know; the result is exact in every case)
enum { EC_ADD_GENERAL = 0, EC_ADD_EQUAL = 1, EC_ADD_OPPOSITE = 2, EC_ADD_INF_OPERAND = 3 };

// P + Q, exact for every input: an operand at infinity, P == Q (doubling), P == -Q (infinity).  R may alias P or Q.
template <int L>
EC_HD int pt_add(Jac<L>& R, const Jac<L>& P, const Jac<L>& Q, const Curve<L>& C) {
  if (pt_is_inf<L>(P)) { R = Q; return EC_ADD_INF_OPERAND; }
  if (pt_is_inf<L>(Q)) { R = P; return EC_ADD_INF_OPERAND; }
  uint32_t u1[L], s1[L], h[L], rr[L], t[L], v[L];
  fp_sqr<L>(t, Q.z, C);
  fp_mul<L>(u1, P.x, t, C);                             // U1 = X1 Z2^2
  fp_mul<L>(t, t, Q.z, C);
  fp_mul<L>(s1, P.y, t, C);                             // S1 = Y1 Z2^3
  fp_sqr<L>(t, P.z, C);
  fp_mul<L>(h, Q.x, t, C);                              // U2
  fp_sub<L>(h, h, u1, C);                               // H = U2 - U1
  fp_mul<L>(t, t, P.z, C);
  fp_mul<L>(rr, Q.y, t, C);                             // S2
  fp_sub<L>(rr, rr, s1, C);                             // r = S2 - S1
  if (fe_is_zero<L>(h)) {
    if (fe_is_zero<L>(rr)) { pt_dbl<L>(R, P, C); return EC_ADD_EQUAL; }
    pt_set_inf<L>(R);
    return EC_ADD_OPPOSITE;
  }
  fp_mul<L>(t, P.z, Q.z, C);
  fp_mul<L>(R.z, t, h, C);                              // Z3 = Z1 Z2 H
  fp_sqr<L>(t, h, C);                                   // H^2
  fp_mul<L>(v, u1, t, C);                               // V = U1 H^2
  fp_mul<L>(h, h, t, C);                                // H^3
  fp_mul<L>(s1, s1, h, C);                              // S1 H^3
  fp_sqr<L>(t, rr, C);
  fp_sub<L>(t, t, h, C);
  fp_sub<L>(t, t, v, C);
  fp_sub<L>(R.x, t, v, C);                              // X3 = r^2 - H^3 - 2 V
  fp_sub<L>(t, v, R.x, C);
  fp_mul<L>(t, rr, t, C);
  fp_sub<L>(R.y, t, s1, C);                             // Y3 = r (V - X3) - S1 H^3
  return EC_ADD_GENERAL;
}

// k P, left to right over the bits of k (L words), one doubling per bit and one addition per set bit.  Exact whatever k
// (k >= n included): every addition goes through pt_add.
template <int L>
EC_HD void pt_mul(Jac<L>& R, const Jac<L>& P, const uint32_t* k, const Curve<L>& C) {
  Jac<L> acc;
  pt_set_inf<L>(acc);
  int top = 32 * L - 1;
  while (top >= 0 && !((k[top >> 5] >> (top & 31)) & 1u)) --top;
  for (int i = top; i >= 0; --i) {
    pt_dbl<L>(acc, acc, C);
    if ((k[i >> 5] >> (i & 31)) & 1u) pt_add<L>(acc, acc, P, C);
  }
  R = acc;
}

// P + (qx, qy) for a finite affine point in Montgomery form (Z2 = 1): pt_add without the three products that Z2 costs, 8
// products and 3 squarings.  Exact for every input and the same case codes as pt_add.  R may alias P.  Every exit writes R.y
// last, as pt_dbl does: with exits that end on different words the compiler merges the final stores behind a pointer into
// private memory, and the table walk that inlines this gets 12 bytes of scratch.
template <int L>
EC_HD int pt_add_affine(Jac<L>& R, const Jac<L>& P, const uint32_t* qx, const uint32_t* qy, const Curve<L>& C) {
  if (pt_is_inf<L>(P)) {
    fe_copy<L>(R.z, C.one);
    fe_copy<L>(R.x, qx);
    fe_copy<L>(R.y, qy);
    return EC_ADD_INF_OPERAND;
  }
  uint32_t h[L], rr[L], t[L], v[L];
  fp_sqr<L>(t, P.z, C);
  fp_mul<L>(h, qx, t, C);                               // U2 = X2 Z1^2
  fp_sub<L>(h, h, P.x, C);                              // H = U2 - X1
  fp_mul<L>(t, t, P.z, C);
  fp_mul<L>(rr, qy, t, C);                              // S2 = Y2 Z1^3
  fp_sub<L>(rr, rr, P.y, C);                            // r = S2 - Y1
  if (fe_is_zero<L>(h)) {
    if (fe_is_zero<L>(rr)) { pt_dbl<L>(R, P, C); return EC_ADD_EQUAL; }
    fe_zero<L>(R.z);
    fe_zero<L>(R.x);
    fe_zero<L>(R.y);
    return EC_ADD_OPPOSITE;
  }
  fp_mul<L>(R.z, P.z, h, C);                            // Z3 = Z1 H
  fp_sqr<L>(t, h, C);                                   // H^2
  fp_mul<L>(v, P.x, t, C);                              // V = X1 H^2
  fp_mul<L>(h, h, t, C);                                // H^3
  fp_sqr<L>(t, rr, C);
  fp_sub<L>(t, t, h, C);
  fp_sub<L>(t, t, v, C);
  fp_sub<L>(R.x, t, v, C);                              // X3 = r^2 - H^3 - 2 V
  fp_mul<L>(h, P.y, h, C);                              // Y1 H^3
  fp_sub<L>(t, v, R.x, C);
  fp_mul<L>(t, rr, t, C);
  fp_sub<L>(R.y, t, h, C);                              // Y3 = r (V - X3) - Y1 H^3
  return EC_ADD_GENERAL;
}

// affine coordinates, plain (out of Montgomery form); infinity -> (0, 0) as Go's affineFromJacobian
template <int L>
EC_HD void pt_affine(uint32_t* x, uint32_t* y, const Jac<L>& P, const Curve<L>& C) {
  if (pt_is_inf<L>(P)) { fe_zero<L>(x); fe_zero<L>(y); return; }
  uint32_t zi[L], z2[L], t[L], one_plain[L];
  fp_inv<L>(zi, P.z, C);
  fp_sqr<L>(z2, zi, C);
  fe_zero<L>(one_plain);
  one_plain[0] = 1;
  fp_mul<L>(t, P.x, z2, C);
  fp_mul<L>(x, t, one_plain, C);
  fp_mul<L>(z2, z2, zi, C);
  fp_mul<L>(t, P.y, z2, C);
  fp_mul<L>(y, t, one_plain, C);
}

// Go's Unmarshal checks on plain coordinates x, y: both below p and y^2 = x^3 - 3 x + B.  On success xm / ym are the
// Montgomery forms.
template <int L>
EC_HD bool pt_check(uint32_t* xm, uint32_t* ym, const uint32_t* x, const uint32_t* y, const Curve<L>& C) {
  if (!fe_lt<L>(x, C.p) || !fe_lt<L>(y, C.p)) return false;
  uint32_t l[L], r[L], t[L];
  fp_mul<L>(xm, x, C.rr_p, C);
  fp_mul<L>(ym, y, C.rr_p, C);
  fp_sqr<L>(l, ym, C);
  fp_sqr<L>(r, xm, C);
  fp_mul<L>(r, r, xm, C);
  fp_add<L>(t, xm, xm, C);
  fp_add<L>(t, t, xm, C);
  fp_sub<L>(r, r, t, C);
  fp_add<L>(r, r, C.b, C);
  return fe_eq<L>(l, r);
}

// a b mod n for a, b < n (plain in, plain out): two Montgomery products under n
template <int L>
EC_HD void fn_mul(uint32_t* r, const uint32_t* a, const uint32_t* b, const Curve<L>& C) {
  uint32_t t[L];
  fe_mul<L>(t, a, b, C.n, C.n0inv);
  fe_mul<L>(r, t, C.rr_n, C.n, C.n0inv);
}

// ---- ECDSA verification (crypto/ecdsa.Verify of Go 1.13) ----------------------------------------------------------------
// hashToInt, then mod N: the leftmost fbytes bytes of a longer digest, shifted right by the bits beyond the order's length
// (bits = N.BitLen(), the curve's bit size on all four curves); a shorter digest whole.  e < 2^bits <= 2N before the subtraction.
template <int L>
EC_HD void hash_to_int(uint32_t* e, const uint8_t* dg, uint32_t dlen, uint32_t bits, const Curve<L>& C) {
  const uint32_t take = dlen > C.fbytes ? C.fbytes : dlen;
  fe_from_be<L>(e, dg, take);
  if (8u * take > bits) {
    const uint32_t sh = 8u * take - bits;                // 7 on P-521, nothing elsewhere
#pragma unroll
    for (int i = 0; i < L; ++i) e[i] = (e[i] >> sh) | (i + 1 < L ? e[i + 1] << (32u - sh) : 0u);
  }
  if (!fe_lt<L>(e, C.n)) fe_sub<L>(e, e, C.n, C.n);      // (e - N >= 0: no add-back)
}

// x(R) mod N == r for a finite R and 0 < r < N, without leaving Jacobian coordinates: x = X / Z^2 < p < 2N is r or r + N, so
// X == r Z^2 or, where r + N < p, X == (r + N) Z^2 (mod p).
template <int L>
EC_HD bool x_matches_r(const Jac<L>& R, const uint32_t* r, const Curve<L>& C) {
  uint32_t z2[L], t[L], u[L];
  fp_sqr<L>(z2, R.z, C);
  fp_mul<L>(t, r, C.rr_p, C);                             // (r < N < p)
  fp_mul<L>(t, t, z2, C);
  if (fe_eq<L>(t, R.x)) return true;
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < L; ++i) { c += (uint64_t)r[i] + C.n[i]; u[i] = (uint32_t)c; c >>= 32; }
  if (c || !fe_lt<L>(u, C.p)) return false;
  fp_mul<L>(t, u, C.rr_p, C);
  fp_mul<L>(t, t, z2, C);
  return fe_eq<L>(t, R.x);
}

// The fixed-base table of a point B (the curve's G, or a registered key): the affine points j 2^(w i) B in Montgomery form, windows
// i = 0 .. nwin - 1 of w bits (nwin w covers the scalar), digits j = 1 .. 2^w - 1.  Word-major inside a window: word k (k < L: x,
// k >= L: y) of digit j is
//   tab[((i 2L + k) << w) + j]       (slot j = 0 unused, zero)
// so the 64 lanes of a wave, which walk the same window with their own digits, read one word of their entries from one 2^w-word
// run (64 bytes at w = 4: one line per load instruction, whatever the digits).
EC_HD uint32_t fb_windows(uint32_t fbytes, uint32_t w) { return (8u * fbytes + w - 1u) / w; }
template <int L>
EC_HD size_t fb_table_words(uint32_t w, uint32_t nwin) { return ((size_t)nwin * 2 * L) << w; }

// k B for k < 2^(w nwin) (L words) from the table of B: one mixed addition per non-zero digit, no doubling.  The digits come off a
// copy of k that is shifted down, so that no register array is indexed by a variable.
template <int L>
EC_HD void fb_mul(Jac<L>& R, const uint32_t* tab, uint32_t w, uint32_t nwin, const uint32_t* k, const Curve<L>& C) {
  uint32_t kw[L], qx[L], qy[L];
  fe_copy<L>(kw, k);
  Jac<L> acc;
  pt_set_inf<L>(acc);
  const uint32_t mask = (1u << w) - 1u;
  for (uint32_t i = 0; i < nwin; ++i) {
    const uint32_t d = kw[0] & mask;
#pragma unroll
    for (int j = 0; j < L; ++j) kw[j] = (kw[j] >> w) | (j + 1 < L ? kw[j + 1] << (32u - w) : 0u);
    if (d == 0) continue;
    const uint32_t* e = tab + (((size_t)i * 2 * L) << w) + d;
#pragma unroll
    for (int j = 0; j < L; ++j) { qx[j] = e[(size_t)j << w]; qy[j] = e[(size_t)(L + j) << w]; }
    pt_add_affine<L>(acc, acc, qx, qy, C);
  }
  R = acc;
}

// One step of fb_mul_fixed: P <- P where `keep`, (qx, qy, 1) where `first`, P + (qx, qy) otherwise (the masks are all ones or zero,
// at most one of them set).  The sum is pt_add_affine's GENERAL case alone, whatever P is -- no test for infinity, equal or opposite
// operands -- and each coordinate is settled by a word-wise select as soon as the formulas have no more use for the old one, so the
// step holds one point, not two.  Where the masks discard the sum, its words are arithmetic on whatever P held (zeroes before the
// first digit): defined, and unused.
template <int L>
EC_HD void pt_add_affine_fixed(Jac<L>& P, const uint32_t* qx, const uint32_t* qy, uint32_t keep, uint32_t first, const Curve<L>& C) {
  const uint32_t take = ~(keep | first);
  uint32_t h[L], rr[L], t[L], v[L];
  fp_sqr<L>(t, P.z, C);
  fp_mul<L>(h, qx, t, C);
  fp_sub<L>(h, h, P.x, C);                              // H = X2 Z1^2 - X1
  fp_mul<L>(t, t, P.z, C);
  fp_mul<L>(rr, qy, t, C);
  fp_sub<L>(rr, rr, P.y, C);                            // r = Y2 Z1^3 - Y1
  fp_mul<L>(t, P.z, h, C);                              // Z3 = Z1 H
#pragma unroll
  for (int j = 0; j < L; ++j) P.z[j] = (P.z[j] & keep) | (t[j] & take) | (C.one[j] & first);
  fp_sqr<L>(t, h, C);                                   // H^2
  fp_mul<L>(v, P.x, t, C);                              // V = X1 H^2
  fp_mul<L>(h, h, t, C);                                // H^3
  fp_sqr<L>(t, rr, C);
  fp_sub<L>(t, t, h, C);
  fp_sub<L>(t, t, v, C);
  fp_sub<L>(t, t, v, C);                                // X3 = r^2 - H^3 - 2 V
  fp_mul<L>(h, P.y, h, C);                              // Y1 H^3
  fp_sub<L>(v, v, t, C);                                // V - X3
#pragma unroll
  for (int j = 0; j < L; ++j) P.x[j] = (P.x[j] & keep) | (t[j] & take) | (qx[j] & first);
  fp_mul<L>(t, rr, v, C);
  fp_sub<L>(t, t, h, C);                                // Y3 = r (V - X3) - Y1 H^3
#pragma unroll
  for (int j = 0; j < L; ++j) P.y[j] = (P.y[j] & keep) | (t[j] & take) | (qy[j] & first);
}

// k B for k < N from the table of B, with a sequence of operations that does not depend on k (a secret share's multiple of G,
// dsaContext.Sign): EVERY window loads an entry -- its digit's, or digit 1's where the digit is 0 -- and runs the general mixed
// addition; the digit decides only the entry's address and the masks of the select.  The general formulas suffice for k < N: before
// window i the accumulator is t B with t < 2^(w i), the entry is d 2^(w i) B with d >= 1, so t < d 2^(w i) <= k < N and the two are
// never equal, and they are opposite only if t + d 2^(w i), a prefix of k and at most k, were N.  k = 0 keeps
// the zeroes the accumulator starts with: infinity.  fb_mul stays the route of public scalars (it skips zero digits).
template <int L>
EC_HD void fb_mul_fixed(Jac<L>& R, const uint32_t* tab, uint32_t w, uint32_t nwin, const uint32_t* k, const Curve<L>& C) {
  uint32_t kw[L], qx[L], qy[L];
  fe_copy<L>(kw, k);
  Jac<L> acc;
  pt_set_inf<L>(acc);
  const uint32_t mask = (1u << w) - 1u;
  uint32_t started = 0;                                 // all ones from the first non-zero digit on
  for (uint32_t i = 0; i < nwin; ++i) {
    const uint32_t d = kw[0] & mask;
#pragma unroll
    for (int j = 0; j < L; ++j) kw[j] = (kw[j] >> w) | (j + 1 < L ? kw[j + 1] << (32u - w) : 0u);
    const uint32_t nz = 0u - (uint32_t)(d != 0);
    const uint32_t* e = tab + (((size_t)i * 2 * L) << w) + (d | (1u & ~nz));
#pragma unroll
    for (int j = 0; j < L; ++j) { qx[j] = e[(size_t)j << w]; qy[j] = e[(size_t)(L + j) << w]; }
    pt_add_affine_fixed<L>(acc, qx, qy, ~nz, nz & ~started, C);
    started |= nz;
  }
  R = acc;
}

// ---- constants, on the host (once per curve and context) -------------------------------------------------------------
EC_HD uint32_t neg_inv32(uint32_t m0) {      // -m0^-1 mod 2^32 (m0 odd), Newton
  uint32_t x = m0;
  for (int i = 0; i < 5; ++i) x *= 2u - m0 * x;
  return 0u - x;
}
template <int L>
EC_HD void r_powers(uint32_t* r1, uint32_t* r2, const uint32_t* m) {    // R mod m, R^2 mod m by doubling (odd m < R)
  uint32_t t[L];
  fe_zero<L>(t);
  t[0] = 1;
  for (int i = 0; i < 32 * L; ++i) fe_add<L>(t, t, t, m);
  fe_copy<L>(r1, t);
  for (int i = 0; i < 32 * L; ++i) fe_add<L>(t, t, t, m);
  fe_copy<L>(r2, t);
}
// P, N, B, Gx, Gy: big-endian, fbytes each
template <int L>
EC_HD void curve_setup(Curve<L>& C, const uint8_t* be, uint32_t fbytes) {
  uint32_t bb[L], g[L], r1n[L];
  C.fbytes = fbytes;
  fe_from_be<L>(C.p, be, fbytes);
  fe_from_be<L>(C.n, be + fbytes, fbytes);
  C.p0inv = neg_inv32(C.p[0]);
  C.n0inv = neg_inv32(C.n[0]);
  r_powers<L>(C.one, C.rr_p, C.p);
  r_powers<L>(r1n, C.rr_n, C.n);
  fe_from_be<L>(bb, be + 2 * fbytes, fbytes);
  fp_mul<L>(C.b, bb, C.rr_p, C);
  fe_from_be<L>(g, be + 3 * fbytes, fbytes);
  fp_mul<L>(C.gx, g, C.rr_p, C);
  fe_from_be<L>(g, be + 4 * fbytes, fbytes);
  fp_mul<L>(C.gy, g, C.rr_p, C);
  uint64_t br = 2;
  for (int i = 0; i < L; ++i) { const uint64_t v = (uint64_t)C.p[i] - br; C.pm2[i] = (uint32_t)v; br = v >> 63; }
}

// The fixed-base table of fb_mul (tab: fb_table_words<L>(w, nwin) words) for the base point (bx, by), affine in Montgomery form,
// host only.  Window i's points are sums of B_i = 2^(w i) B through the exact pt_add; all of them are made affine with ONE field
// inversion (Montgomery's trick: the curves have prime order N > 2^w and cofactor 1, so no j 2^(w i) B of a point B on the curve
// is infinity and every Z is non-zero).  Every word written is fully reduced, so the table of a base is unique: the device build
// of a key set (ec_kernels.hip k_ec_keytab_build) is checked against this one word for word.
template <int L>
inline void fb_table_build(uint32_t* tab, uint32_t w, uint32_t nwin, const uint32_t* bx, const uint32_t* by, const Curve<L>& C) {
  const uint32_t per = (1u << w) - 1u;
  const size_t n = (size_t)nwin * per;
  std::vector<Jac<L>> pts(n);
  std::vector<uint32_t> pre(n * L);
  Jac<L> base;
  fe_copy<L>(base.x, bx);
  fe_copy<L>(base.y, by);
  fe_copy<L>(base.z, C.one);
  for (uint32_t i = 0; i < nwin; ++i) {
    Jac<L>* row = &pts[(size_t)i * per];
    row[0] = base;
    for (uint32_t j = 1; j < per; ++j) pt_add<L>(row[j], row[j - 1], base, C);
    for (uint32_t b = 0; b < w; ++b) pt_dbl<L>(base, base, C);
  }
  for (size_t i = 0; i < n; ++i) {                        // pre[i] = Z_0 ... Z_i
    if (i == 0) fe_copy<L>(&pre[0], pts[0].z);
    else fp_mul<L>(&pre[i * L], &pre[(i - 1) * L], pts[i].z, C);
  }
  uint32_t inv[L], zi[L], z2[L];
  fp_inv<L>(inv, &pre[(n - 1) * L], C);
  for (size_t k = 0; k < fb_table_words<L>(w, nwin); ++k) tab[k] = 0;
  for (size_t i = n; i-- > 0;) {
    if (i) { fp_mul<L>(zi, inv, &pre[(i - 1) * L], C); fp_mul<L>(inv, inv, pts[i].z, C); }
    else fe_copy<L>(zi, inv);
    fp_sqr<L>(z2, zi, C);
    fp_mul<L>(pts[i].x, pts[i].x, z2, C);
    fp_mul<L>(z2, z2, zi, C);
    fp_mul<L>(pts[i].y, pts[i].y, z2, C);
    uint32_t* e = tab + (((size_t)(i / per) * 2 * L) << w) + (i % per + 1);
    for (int k = 0; k < L; ++k) { e[(size_t)k << w] = pts[i].x[k]; e[(size_t)(L + k) << w] = pts[i].y[k]; }
  }
}
// ... of the curve's own base point G
template <int L>
inline void fb_table_build(uint32_t* tab, uint32_t w, uint32_t nwin, const Curve<L>& C) {
  fb_table_build<L>(tab, w, nwin, C.gx, C.gy, C);
}

}  // namespace ecf

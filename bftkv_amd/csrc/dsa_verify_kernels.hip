// Raw DSA verification (crypto/dsa.Verify of Go 1.13 on a digest, r || s and a public key sent with the call), gfx950.
//   k_dsav_prep     thread / signature: the range, width, digest-length and inverse rules, u1 = z w and u2 = r w mod q
//   k_dsav_tables   lane group / distinct base (the groups' g, then the keys' y): b^1 .. b^15 in Montgomery form mod its p
//   k_dsav_exp      lane group / signature: v = g^u1 y^u2 mod p mod q by Straus' method over the two tables, compared with r
// and, for keys registered once as a resident set (bftkv_gpu_dsa_keyset_*), after the same k_dsav_prep:
//   k_dsav_comb_build  lane group / (base, window, part): the fixed-base table b^(d 2^(w i)), fully reduced, built at registration
//   k_dsav_comb_exp    lane group / signature: the same v as a chain of table products, no squarings
// k_multiexp rebuilds its window table for every operation; here g is shared by every signature of a group and y by every
// signature of a key, so a table is built once per distinct base and call.  All big-number work is the multiplier of mont28.h.
#pragma once
// (kernels.hip and threshold_kernels.hip are included before this file by capi.hip)
#include "dsa_verify.h"

namespace bftkv {

// e_limbs [n_ops][3][10]: u1, u2, r as radix-2^28 limbs; op_key / op_grp: the signature's (clamped) key and that key's group
__global__ void __launch_bounds__(64) k_dsav_prep(uint32_t n_ops, const uint8_t* __restrict__ digests, uint32_t dlen, const uint8_t* __restrict__ sigs,
                                                  uint32_t qbytes, const uint32_t* __restrict__ key_idx /*[n_ops] or null: key 0*/, uint32_t n_keys,
                                                  const uint32_t* __restrict__ key_group /*[n_keys], below n_groups*/,
                                                  const uint8_t* __restrict__ q_be /*[n_groups][qbytes]*/, uint32_t* __restrict__ e_limbs,
                                                  uint32_t* __restrict__ op_key, uint32_t* __restrict__ op_grp, uint8_t* __restrict__ decided,
                                                  uint8_t* __restrict__ status) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = t < n_ops;
  const uint32_t op = active ? t : (n_ops - 1);      // (the inverse votes across the wave: spare lanes repeat the last signature)
  const uint32_t ki = key_idx ? min(key_idx[op], n_keys - 1u) : 0u;
  const uint32_t gi = key_group[ki];
  DsavPrep o;
  dsav_prep_one(sigs + (uint64_t)op * 2 * qbytes, qbytes, q_be + (uint64_t)gi * qbytes, digests + (uint64_t)op * dlen, dlen, o);
  if (!active) return;
  uint32_t* row = e_limbs + (uint64_t)op * DSAV_ROW;
  dsav_limbs10(o.u1, row);
  dsav_limbs10(o.u2, row + DSAV_EXP_LIMBS);
  dsav_limbs10(o.r, row + 2 * DSAV_EXP_LIMBS);
  op_key[op] = ki;
  op_grp[op] = gi;
  decided[op] = o.decided;
  status[op] = o.status;
}

// <L, TPI> as k_multiexp: 19 limbs x 4 lanes (R = 2^2128) or 10 limbs x 8 lanes (R = 2^2240); a call uses ONE form for its
// tables and its exponentiation (the Montgomery factor is part of a table entry).  Rows in memory are MONT_N limbs either way.
#define DSAV_GROUP_SETUP(count)                                                                                          \
  constexpr int NL = L * TPI, GROUPS = RSA_BLOCK / TPI;                                                                  \
  static_assert(NL >= MONT_N, "a group holds a whole row");                                                              \
  __shared__ uint32_t a_sh[GROUPS * NL];                                                                                 \
  const uint32_t grp = threadIdx.x / TPI;                                                                                \
  const int qlane = threadIdx.x % TPI;                                                                                   \
  const uint32_t gq = blockIdx.x * GROUPS + grp;                                                                         \
  const bool active = gq < (count);                                                                                      \
  uint32_t* a_lds = a_sh + grp * NL + qlane * L;                                                                         \
  const uint32_t* a_rd = a_sh + grp * NL;                                                                                \
  auto ld = [&](const uint32_t* row, int k) -> uint32_t { const int gi_ = qlane * L + k; return (NL == MONT_N || gi_ < MONT_N) ? row[gi_] : 0u; };

template <int L, int TPI>
__global__ void __launch_bounds__(RSA_BLOCK) k_dsav_tables(uint32_t n_groups, uint32_t n_keys, const uint32_t* __restrict__ base_limbs /*[n_groups + n_keys][76]: g, then y*/,
                                                           const uint32_t* __restrict__ key_group, ModTab mp, uint32_t* __restrict__ tab /*[n_groups + n_keys][15][76]*/) {
  const uint32_t n_bases = n_groups + n_keys;
  DSAV_GROUP_SETUP(n_bases);
  const uint32_t b = active ? gq : (n_bases - 1);
  const uint32_t mi = b < n_groups ? b : key_group[b - n_groups];
  auto st = [&](uint32_t* row, int k, uint32_t v) { const int gi_ = qlane * L + k; if (NL == MONT_N || gi_ < MONT_N) row[gi_] = v; };
  uint32_t n[L], y[L], t[L];
  const uint32_t* r2p = (TPI == MONT_TPI ? mp.r2_limbs + (uint64_t)mi * MONT_N : mp.r2w_limbs + (uint64_t)mi * MONT_N_WIDE) + qlane * L;
  const uint32_t* nrow = mp.n_limbs + (uint64_t)mi * MONT_N;
  const uint32_t* brow = base_limbs + (uint64_t)b * MONT_N;
  uint32_t* trow = tab + (uint64_t)b * MULTIEXP_ENT * MONT_N;
#pragma unroll
  for (int k = 0; k < L; ++k) { n[k] = ld(nrow, k); a_lds[k] = ld(brow, k); y[k] = r2p[k]; }
  const uint32_t n0inv = mp.n0inv[mi];
  // d = 0: b R mod p (the product also reduces a base >= p: b < R, so the result is below 2p); d >= 1: b^(d+1) = b^d * b, with
  // a = b R kept in LDS
#pragma unroll 1
  for (int d = 0; d < MULTIEXP_ENT; ++d) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    mont_mul<L, TPI, false>(t, a_rd, y, n, n0inv, qlane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int k = 0; k < L; ++k) {
      y[k] = t[k];
      if (d == 0) a_lds[k] = t[k];
      if (active) st(trow + (uint64_t)d * MONT_N, k, t[k]);
    }
  }
}

// One loop with two multiplier call sites (general and squaring), as k_multiexp and for its reason (registers): the Montgomery
// one, `exp_windows` windows of four squarings and at most one table product per base (a digit that is zero in every signature of
// the wave is skipped by a vote), out of the domain, then v mod q by two products under q's own rows (k_limbs_mod_q's method).
// A decided signature has u1 = u2 = 0 and rides along on 1; its verdict stays 0.
template <int L, int TPI>
__global__ void __launch_bounds__(RSA_BLOCK) k_dsav_exp(uint32_t n_ops, const uint32_t* __restrict__ e_limbs, const uint32_t* __restrict__ op_key,
                                                        const uint32_t* __restrict__ op_grp, const uint8_t* __restrict__ decided, uint32_t n_groups,
                                                        ModTab mp, ModTab mq, const uint32_t* __restrict__ tab, uint32_t exp_windows,
                                                        uint8_t* __restrict__ valid_out) {
  DSAV_GROUP_SETUP(n_ops);
  const uint32_t op = active ? gq : (n_ops - 1);
  const uint32_t gi = op_grp[op];
  const uint32_t* erow = e_limbs + (uint64_t)op * DSAV_ROW;
  const uint32_t* tab_g = tab + (uint64_t)gi * MULTIEXP_ENT * MONT_N;
  const uint32_t* tab_y = tab + ((uint64_t)n_groups + op_key[op]) * MULTIEXP_ENT * MONT_N;
  uint32_t n[L], y[L], t[L];
  const uint32_t* r2p = (TPI == MONT_TPI ? mp.r2_limbs + (uint64_t)gi * MONT_N : mp.r2w_limbs + (uint64_t)gi * MONT_N_WIDE) + qlane * L;
  const uint32_t* r2q = (TPI == MONT_TPI ? mq.r2_limbs + (uint64_t)gi * MONT_N : mq.r2w_limbs + (uint64_t)gi * MONT_N_WIDE) + qlane * L;
  const uint32_t* prow = mp.n_limbs + (uint64_t)gi * MONT_N;
  const uint32_t* qrow = mq.n_limbs + (uint64_t)gi * MONT_N;
#pragma unroll
  for (int k = 0; k < L; ++k) n[k] = ld(prow, k);
  uint32_t n0inv = mp.n0inv[gi];
  // wave-uniform program counter
  enum : int { P_ONE = 0, P_SQR, P_TABMUL, P_LEAVE, P_QIN, P_QOUT };
  int phase = P_ONE, w = (int)exp_windows - 1, sq = 0;
  uint32_t j = 0, dig = 0;
  while (true) {
    // ---- operands: a through LDS, b in registers (y)
    if (phase == P_ONE) {                           // Montgomery one = mont(1, R^2)
#pragma unroll
      for (int k = 0; k < L; ++k) { a_lds[k] = (qlane == 0 && k == 0) ? 1u : 0u; y[k] = r2p[k]; }
    } else if (phase == P_SQR) {
#pragma unroll
      for (int k = 0; k < L; ++k) a_lds[k] = y[k];
    } else if (phase == P_TABMUL) {
      const uint32_t* row = (j ? tab_y : tab_g) + (uint64_t)(dig ? dig - 1 : 0) * MONT_N;
#pragma unroll
      for (int k = 0; k < L; ++k) a_lds[k] = ld(row, k);
    } else if (phase == P_QIN) {                    // v (canonical, below p < R) times q's R^2, under q
#pragma unroll
      for (int k = 0; k < L; ++k) { a_lds[k] = y[k]; y[k] = r2q[k]; n[k] = ld(qrow, k); }
      n0inv = mq.n0inv[gi];
    } else {                                        // P_LEAVE, P_QOUT: mont(y, 1)
#pragma unroll
      for (int k = 0; k < L; ++k) a_lds[k] = (qlane == 0 && k == 0) ? 1u : 0u;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (phase == P_SQR) mont_mul<L, TPI, true>(t, a_rd, y, n, n0inv, qlane);
    else mont_mul<L, TPI, false>(t, a_rd, y, n, n0inv, qlane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // ---- results and next step (scalar control flow)
    if (phase == P_QOUT) break;
    if (phase != P_TABMUL || dig) {
#pragma unroll
      for (int k = 0; k < L; ++k) y[k] = t[k];
    }
    if (phase == P_LEAVE) {
      // y <= p after mont(., 1); y == p only for 0
      canonicalize<L, TPI>(y, qlane);
      uint32_t diff = 0;
#pragma unroll
      for (int k = 0; k < L; ++k) diff |= y[k] ^ n[k];
      diff = grp_or<TPI>(diff);
#pragma unroll
      for (int k = 0; k < L; ++k) y[k] = (diff == 0) ? 0u : y[k];
      phase = P_QIN;
      continue;
    }
    if (phase == P_QIN) { phase = P_QOUT; continue; }
    // advance: 4 squarings per window, then one table product per base with a non-zero digit somewhere in the wave
    if (phase == P_ONE) { phase = P_SQR; sq = 0; continue; }
    if (phase == P_SQR) { if (++sq == MULTIEXP_WIN) { phase = P_TABMUL; j = 0; } else continue; }
    else ++j;
    while (phase == P_TABMUL) {
      if (j == 2) { j = 0; if (--w < 0) phase = P_LEAVE; else { phase = P_SQR; sq = 0; } break; }
      const int bit = w * MULTIEXP_WIN;
      dig = active ? ((erow[j * DSAV_EXP_LIMBS + bit / MONT_W] >> (bit % MONT_W)) & 15u) : 0u;
      if (__any(dig != 0)) break;
      ++j;
    }
  }
  canonicalize<L, TPI>(t, qlane);
  // t <= q after mont(., 1); t == q only for 0, which no r of an open verdict is (0 < r < q): a plain compare decides
  uint32_t neq = 0;
#pragma unroll
  for (int k = 0; k < L; ++k) {
    const int gi_ = qlane * L + k;
    const uint32_t rl = gi_ < DSAV_EXP_LIMBS ? erow[2 * DSAV_EXP_LIMBS + gi_] : 0u;
    neq |= t[k] ^ rl;
  }
  neq = grp_or<TPI>(neq);
  if (active && qlane == 0) valid_out[op] = (neq == 0 && !decided[op]) ? 1 : 0;
}

// ---- resident key sets (bftkv_gpu_dsa_keyset_*; dsa_verify.h for the digits and the table's layout) ----------------------------
// The table of a base b under its group's p: tab[base][window i][d - 1] = b^(d 2^(w i)) R mod p for d = 1 .. 2^w - 1, FULLY reduced
// (below p, every limb below 2^28), so that a table is a function of (b, p, w) alone and the exponentiation's products, which only
// need operands below 2p, take entries as they are.  One lane group per (base, window, part), the method of k_dsa_build_comb over
// the set's own arrays: B = b^(2^(w i)) by w i squarings (a uniform trip count: groups past their own count keep B), the part's
// first entry B^d0 by square-and-multiply over d0, then the part's entries by repeated products with B.  `parts` divides 2^w.
// A base >= p is reduced by the first product, as in k_dsav_tables.  Runs once per set, never on the verify path.
template <int L, int TPI>
__global__ void __launch_bounds__(RSA_BLOCK) k_dsav_comb_build(uint32_t n_groups, uint32_t n_keys, const uint32_t* __restrict__ base_limbs /*[n_groups + n_keys][76]: g, then y*/,
                                                               const uint32_t* __restrict__ key_group, ModTab mp, uint32_t w, uint32_t windows, uint32_t parts,
                                                               uint32_t* __restrict__ tab) {
  const uint32_t n_units = (n_groups + n_keys) * windows * parts;
  DSAV_GROUP_SETUP(n_units);
  const uint32_t unit = active ? gq : (n_units - 1);
  const uint32_t part = unit % parts, win = (unit / parts) % windows, bb = unit / parts / windows;
  const uint32_t mi = bb < n_groups ? bb : key_group[bb - n_groups];
  auto st = [&](uint32_t* row, int k, uint32_t v) { const int gi_ = qlane * L + k; if (NL == MONT_N || gi_ < MONT_N) row[gi_] = v; };
  uint32_t n[L], y[L], b[L], t[L];
  const uint32_t* r2p = mp.r2_limbs + (uint64_t)mi * MONT_N + qlane * L;
  const uint32_t* nrow = mp.n_limbs + (uint64_t)mi * MONT_N;
  const uint32_t* brow = base_limbs + (uint64_t)bb * MONT_N;
  const uint32_t n0inv = mp.n0inv[mi];
#define DSAV_MONT(SQR, bexpr)                                    \
  do {                                                           \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");       \
    mont_mul<L, TPI, SQR>(t, a_rd, bexpr, n, n0inv, qlane);      \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");       \
  } while (0)
  // y = b R mod p (b < R, so the product is below 2p whatever b is)
#pragma unroll
  for (int k = 0; k < L; ++k) { n[k] = ld(nrow, k); a_lds[k] = ld(brow, k); b[k] = r2p[k]; }
  DSAV_MONT(false, b);
#pragma unroll
  for (int k = 0; k < L; ++k) y[k] = t[k];
  const uint32_t nsq = w * win;
#pragma unroll 1
  for (uint32_t i = 0; i < w * (windows - 1u); ++i) {
#pragma unroll
    for (int k = 0; k < L; ++k) a_lds[k] = y[k];
    DSAV_MONT(true, y);
    if (i < nsq) {
#pragma unroll
      for (int k = 0; k < L; ++k) y[k] = t[k];
    }
  }
  // y = B.  The part's digits are d0 .. d0 + per - 1 (digit 0 has no entry); b = B^d0, starting from R mod p = mont(1, R^2)
  const uint32_t per = (1u << w) / parts, d0 = part * per;
#pragma unroll
  for (int k = 0; k < L; ++k) { a_lds[k] = (qlane == 0 && k == 0) ? 1u : 0u; b[k] = r2p[k]; }
  DSAV_MONT(false, b);
#pragma unroll
  for (int k = 0; k < L; ++k) b[k] = t[k];
  if (parts > 1) {                                    // (one part: d0 = 0 everywhere)
#pragma unroll 1
    for (int bit = (int)w - 1; bit >= 0; --bit) {      // left to right; a uniform trip count, a select per group
#pragma unroll
      for (int k = 0; k < L; ++k) a_lds[k] = b[k];
      DSAV_MONT(true, b);
#pragma unroll
      for (int k = 0; k < L; ++k) { b[k] = t[k]; a_lds[k] = y[k]; }
      DSAV_MONT(false, b);
      if ((d0 >> bit) & 1u) {
#pragma unroll
        for (int k = 0; k < L; ++k) b[k] = t[k];
      }
    }
  }
#pragma unroll 1
  for (uint32_t j = 0; j < per; ++j) {
    const uint32_t d = d0 + j;
    // the entry, fully reduced: b is below 2p with limbs up to 2^28
#pragma unroll
    for (int k = 0; k < L; ++k) t[k] = b[k];
    canonicalize<L, TPI>(t, qlane);
    reduce_once<L, TPI>(t, n, qlane);
    if (active && d >= 1u) {
      uint32_t* row = tab + dsav_comb_entry(bb, win, d, windows, w) * MONT_N;
#pragma unroll
      for (int k = 0; k < L; ++k) st(row, k, t[k]);
    }
    if (j + 1u == per) break;
#pragma unroll
    for (int k = 0; k < L; ++k) a_lds[k] = y[k];
    DSAV_MONT(false, b);
#pragma unroll
    for (int k = 0; k < L; ++k) b[k] = t[k];
  }
#undef DSAV_MONT
}

// v = g^u1 y^u2 mod p mod q from the set's tables, compared with r: no squarings, one product per non-zero digit.  One lane group
// per signature walks (g's table, u1's digits), then (y's table, u2's digits); a (base, window) step whose digit is zero in every
// signature of the wave is skipped by a vote, a signature's first non-zero digit takes its entry as the starting value, and a
// signature with no non-zero digit at all is 1 (u1 = u2 = 0 of a decided signature, whose verdict stays 0).  The tail is
// k_dsav_exp's.  Wave-uniform control flow, one multiplier call site.
template <int L, int TPI>
__global__ void __launch_bounds__(RSA_BLOCK) k_dsav_comb_exp(uint32_t n_ops, const uint32_t* __restrict__ e_limbs, const uint32_t* __restrict__ op_key,
                                                             const uint32_t* __restrict__ op_grp, const uint8_t* __restrict__ decided, uint32_t n_groups,
                                                             ModTab mp, ModTab mq, const uint32_t* __restrict__ tab, uint32_t w, uint32_t windows,
                                                             uint8_t* __restrict__ valid_out) {
  DSAV_GROUP_SETUP(n_ops);
  const uint32_t op = active ? gq : (n_ops - 1);
  const uint32_t gi = op_grp[op];
  const uint32_t* erow = e_limbs + (uint64_t)op * DSAV_ROW;
  const uint32_t base_y = n_groups + op_key[op];
  uint32_t n[L], y[L], t[L];
  const uint32_t* r2q = mq.r2_limbs + (uint64_t)gi * MONT_N + qlane * L;
  const uint32_t* prow = mp.n_limbs + (uint64_t)gi * MONT_N;
  const uint32_t* qrow = mq.n_limbs + (uint64_t)gi * MONT_N;
#pragma unroll
  for (int k = 0; k < L; ++k) { n[k] = ld(prow, k); y[k] = 0u; t[k] = 0u; a_lds[k] = 0u; }
  uint32_t n0inv = mp.n0inv[gi];
  enum : int { P_TAB = 0, P_LEAVE, P_QIN, P_QOUT };
  int phase = P_TAB;
  uint32_t step = 0, dig = 0;                       // step = j * windows + i: base j (0: g with u1, 1: y with u2), window i
  bool started = false;
  // the next step with a non-zero digit somewhere in the wave (spare lane groups hold none), or the end of the chain
  auto seek = [&]() {
    while (step < 2u * windows) {
      const uint32_t j = step >= windows ? 1u : 0u;
      dig = active ? dsav_comb_digit(erow + j * DSAV_EXP_LIMBS, step - j * windows, w) : 0u;
      if (__any(dig != 0)) return;
      ++step;
    }
    phase = P_LEAVE;
  };
  seek();
  while (true) {
    // ---- operands: a through LDS, b in registers (y)
    bool mul = true;
    if (phase == P_TAB) {
      if (dig) {                                    // the gather: one 304-byte row per product
        const uint32_t j = step >= windows ? 1u : 0u;
        const uint32_t* row = tab + dsav_comb_entry(j ? base_y : gi, step - j * windows, dig, windows, w) * MONT_N;
#pragma unroll
        for (int k = 0; k < L; ++k) a_lds[k] = ld(row, k);
      }
      mul = __any(dig != 0 && started);             // (every signature of the wave starts here: nothing to multiply)
    } else if (phase == P_QIN) {                    // v (canonical, below p < R) times q's R^2, under q
#pragma unroll
      for (int k = 0; k < L; ++k) { a_lds[k] = y[k]; y[k] = r2q[k]; n[k] = ld(qrow, k); }
      n0inv = mq.n0inv[gi];
    } else {                                        // P_LEAVE, P_QOUT: mont(y, 1)
#pragma unroll
      for (int k = 0; k < L; ++k) a_lds[k] = (qlane == 0 && k == 0) ? 1u : 0u;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (mul) mont_mul<L, TPI, false>(t, a_rd, y, n, n0inv, qlane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // ---- results and next step (scalar control flow)
    if (phase == P_QOUT) break;
    if (phase == P_TAB) {
      if (dig) {
#pragma unroll
        for (int k = 0; k < L; ++k) y[k] = started ? t[k] : a_lds[k];      // (a_lds: this lane's own limbs of the entry)
        started = true;
      }
      ++step;
      seek();
      continue;
    }
#pragma unroll
    for (int k = 0; k < L; ++k) y[k] = t[k];
    if (phase == P_LEAVE) {
      // y <= p after mont(., 1); y == p only for 0.  A signature that never started is 1 (0 under p = 1, by the same compare).
      canonicalize<L, TPI>(y, qlane);
      uint32_t diff = 0;
#pragma unroll
      for (int k = 0; k < L; ++k) {
        if (!started) y[k] = (qlane == 0 && k == 0) ? 1u : 0u;
        diff |= y[k] ^ n[k];
      }
      diff = grp_or<TPI>(diff);
#pragma unroll
      for (int k = 0; k < L; ++k) y[k] = (diff == 0) ? 0u : y[k];
      phase = P_QIN;
      continue;
    }
    phase = P_QOUT;                                  // P_QIN
  }
  canonicalize<L, TPI>(t, qlane);
  // t <= q after mont(., 1); t == q only for 0, which no r of an open verdict is (0 < r < q): a plain compare decides
  uint32_t neq = 0;
#pragma unroll
  for (int k = 0; k < L; ++k) {
    const int gi_ = qlane * L + k;
    const uint32_t rl = gi_ < DSAV_EXP_LIMBS ? erow[2 * DSAV_EXP_LIMBS + gi_] : 0u;
    neq |= t[k] ^ rl;
  }
  neq = grp_or<TPI>(neq);
  if (active && qlane == 0) valid_out[op] = (neq == 0 && !decided[op]) ? 1 : 0;
}

}  // namespace bftkv

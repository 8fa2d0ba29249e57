// The secret-exponent ladder of k_tpa_pow (tpa_kernels.hip), k_psign_pow (rsa_psign_kernels.hip) and k_rsas_crt (rsa_sign_kernels.hip):
// one chain per quad on mont_mul<L, TPI>, fixed 4-bit windows, one loop with a wave-uniform program counter.
//
// The table b^0 .. b^15 (Montgomery form, b^0 = R mod n) goes to global memory, written and re-read by the same lanes (rows of L * TPI
// limbs, CHAIN_ENT of them per quad), then every window is 4 squarings and ONE multiplication by the row its digit names, and
// mont(y, 1) leaves Montgomery form.  The row of a zero digit is the Montgomery one, so nothing is skipped and nothing selected.
//
// SECRETS.  The exponents are secrets in all three kernels (y and b of the password protocol, key fragments, dp and dq), and so is
// whatever a policy's entry and exit products touch.  What does not depend on them: the sequence of products, which is a function of
// `windows` and of the policy's two constants alone, the same in every lane of the wave.  What does: the ADDRESS of the table row
// (the digit) -- and, outside this body, only what a kernel says of its own policy.
//
// There are two multiplier call sites (general and squaring), as in k_multiexp and for its reason: mont_mul is inlined twice, and the
// registers of a wave hold one copy of its live ranges.  The program counter is scalar, so the two never run in one iteration.
//
// The policy P supplies what differs between the kernels; every hook receives the wave-uniform step it is called for:
//   PRE (1, 2)   entry products: pre_load(step, a_lds, y) sets both operands, pre_done(step, t) sees the product.  After the last one,
//                t is the base in Montgomery form: it becomes y, the broadcast operand of the powers and table row 1.
//   digit(w)     digit w of the exponent, 0 .. 15; w counts down from windows - 1
//   POST (0, 3)  exit products behind the leave: leave_done(t, y, a_lds) sees the power (t) and its Montgomery form (y);
//                post_load(step) returns this lane's limbs of the row that becomes y, or nullptr for mont(y, 1) once more;
//                post_slice(step, a_own) the slice the multiplier reads, a_own or another quad's of the same wave (it is asked at
//                every product, with step < 0 ahead of the exit steps); post_done(step, t, a_lds) sees the product of every step
//                but the last, which is left in out.  y is the product behind every step, as in the chain.
// The hooks never store to y and a_lds in two arms of one branch: a hook is compiled on its own before it is inlined, where the two
// are plain pointers and such stores are merged into one through a chosen address, and that keeps y out of the registers.
#pragma once
// (kernels.hip is included before this file by capi.hip)

namespace bftkv {

constexpr int CHAIN_ENT = 16;      // rows of a chain's table: b^0 .. b^15

// a_lds: this lane's L limbs of the quad's slice a_own; tab: this lane's limbs of row 0 of the quad's table; r2p: of R^2 mod n.
// windows == 0: from the table straight to the leave (b^0 = 1).  Leaves the last product in out, not canonical.
template <int L, int TPI, class P>
__device__ __forceinline__ void window_chain(P& p, uint32_t* a_lds, const uint32_t* a_own, uint32_t* tab, const uint32_t* r2p,
                                             const uint32_t (&n)[L], uint32_t n0inv, int qlane, int windows, uint32_t (&out)[L]) {
  constexpr int N = L * TPI;
  // wave-uniform program counter: the entry steps 0 .. PRE - 1, the chain, the exit steps P_LEAVE + 1 .. P_LAST
  enum : uint32_t { P_POWERS = P::PRE, P_ONE, P_SQR, P_TABMUL, P_LEAVE, P_LAST = P_LEAVE + P::POST };
  // The register operand of every product is y (R^2 is loaded into it where needed).  The product goes to an array of this function's
  // and out is written once: through the caller's array the multiplier's closing masks end up inside its block loop.
  uint32_t y[L], t[L];
  uint32_t phase = 0, d = 0;          // d: the table row being built in P_POWERS
  int w = windows - 1, sq = 0;
  for (;;) {
    // ---- operands: a through LDS, b in registers
    const uint32_t* a_rd = a_own;
    if (phase < P_POWERS) {
      p.pre_load((int)phase, a_lds, y);
    } else if (phase == P_POWERS) {                 // b^d = b^(d-1) * b; a = b R stays in LDS, y = the previous power
    } else if (phase == P_ONE) {                    // Montgomery one = mont(1, R^2)
#pragma unroll
      for (int k = 0; k < L; ++k) { a_lds[k] = (qlane == 0 && k == 0) ? 1u : 0u; y[k] = r2p[k]; }
    } else if (phase == P_SQR) {
#pragma unroll
      for (int k = 0; k < L; ++k) a_lds[k] = y[k];
    } else if (phase == P_TABMUL) {
      const uint32_t* row = tab + (uint64_t)p.digit((uint32_t)w) * N;
#pragma unroll
      for (int k = 0; k < L; ++k) a_lds[k] = row[k];
    } else if (P::POST == 0 || phase == P_LEAVE) {  // mont(y, 1)  (POST == 0: nothing else is left, and the compiler is told so)
#pragma unroll
      for (int k = 0; k < L; ++k) a_lds[k] = (qlane == 0 && k == 0) ? 1u : 0u;
    } else if constexpr (P::POST > 0) {
      const uint32_t* b = p.post_load((int)(phase - P_LEAVE) - 1);
      if (b) {
#pragma unroll
        for (int k = 0; k < L; ++k) y[k] = b[k];
      } else {
#pragma unroll
        for (int k = 0; k < L; ++k) a_lds[k] = (qlane == 0 && k == 0) ? 1u : 0u;
      }
    }
    // (asked at every product, without a branch: a select, through which the loads still see the slice's alignment)
    if constexpr (P::POST > 0) a_rd = p.post_slice((int)(phase - P_LEAVE) - 1, a_own);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (phase == P_SQR) mont_mul<L, TPI, true>(t, a_rd, y, n, n0inv, qlane);
    else mont_mul<L, TPI, false>(t, a_rd, y, n, n0inv, qlane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // ---- results and next step (scalar control flow)
    if (phase == P_LAST) break;
    if (phase < P_POWERS) p.pre_done((int)phase, t);
    if constexpr (P::POST > 0) {
      if (phase == P_LEAVE) p.leave_done(t, y, a_lds);
      else if (phase > P_LEAVE) p.post_done((int)(phase - P_LEAVE) - 1, t, a_lds);
    }
#pragma unroll
    for (int k = 0; k < L; ++k) y[k] = t[k];
    if (phase < P_POWERS) {
      if (++phase == P_POWERS) {
#pragma unroll
        for (int k = 0; k < L; ++k) { a_lds[k] = t[k]; tab[N + k] = t[k]; }      // a = b R for the powers
        d = 2;
      }
    } else if (phase == P_POWERS) {
#pragma unroll
      for (int k = 0; k < L; ++k) tab[(uint64_t)d * N + k] = t[k];
      if (++d == CHAIN_ENT) phase = P_ONE;
    } else if (phase == P_ONE) {
#pragma unroll
      for (int k = 0; k < L; ++k) tab[k] = t[k];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");      // own table rows are read back below
      if (w < 0) phase = P_LEAVE; else { phase = P_SQR; sq = 0; }
    } else if (phase == P_SQR) {
      if (++sq == 4) phase = P_TABMUL;
    } else if (P::POST == 0 || phase == P_TABMUL) {
      if (--w < 0) phase = P_LEAVE; else { phase = P_SQR; sq = 0; }
    } else ++phase;                                 // (POST > 0: the leave and the exit steps)
  }
#pragma unroll
  for (int k = 0; k < L; ++k) out[k] = t[k];
}

}  // namespace bftkv

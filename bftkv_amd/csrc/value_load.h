// A lane's L radix-2^W limbs of a big-endian value of nb bytes, without a branch per byte: the limbs limb_of (kernels.hip) cuts
// five guarded bytes at a time come out of ceil((L W + 7) / 32) unaligned dwords, every one of them loaded before the first is
// used.  k_rsa_modexp and k_rsav_verify start with it.  Memory is reached through the caller's functors only, so the same text
// compiles for the host (tests/c/value_load_host.cpp runs it under the sanitizers over buffers of exactly nb bytes).
#pragma once
#include <stdint.h>

#ifndef VLOAD_HD
#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define VLOAD_HD __host__ __device__ __forceinline__
#else
#define VLOAD_HD static inline
#endif
#endif

// -DBFTKV_VALUE_LOAD=bytes: the kernels fetch the value byte by byte through limb_of, as they did before this header -- the two
// loaders as two builds of one tree (the default is dwords; any other word does not compile)
#define BFTKV_VALUE_LOAD_bytes 0
#define BFTKV_VALUE_LOAD_dwords 1
#ifndef BFTKV_VALUE_LOAD
#define BFTKV_VALUE_LOAD dwords
#endif
#define BFTKV_VLOAD_CAT_(a, b) a##b
#define BFTKV_VLOAD_CAT(a, b) BFTKV_VLOAD_CAT_(a, b)

namespace bftkv {

constexpr bool VALUE_LOAD_DWORDS = BFTKV_VLOAD_CAT(BFTKV_VALUE_LOAD_, BFTKV_VALUE_LOAD) != 0;

// dwords that hold a lane's L W bits from the byte its first limb starts in
template <int W, int L>
constexpr int value_load_dwords() { return (L * W + 7 + 31) / 32; }

// bits sh .. sh + 31 of hi:lo, sh < 32 (v_alignbit_b32)
VLOAD_HD uint32_t vload_align(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (sh & 31u)); }
VLOAD_HD uint32_t vload_bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }

// x[k] = limb lane * L + k of the value whose nb bytes, most significant first, the functors read:
//   load4(o)  the four bytes at offsets o .. o + 3 as they lie in memory (a little-endian dword), 0 <= o <= nb - 4
//   load1(o)  the byte at offset o < nb
// No other offset is asked for, whatever nb is: bytes above the form's TPI L limbs are never touched, bytes the value does not
// have count as zero.  The dword that straddles the value's first byte is fetched from offset 0 and shifted down, and a dword
// wholly above it is a second fetch of offset 0 whose result is dropped -- so the loads of the nb >= 4 path are unconditional.
template <int W, int L, int TPI, typename F4, typename F1>
VLOAD_HD void value_limbs(uint32_t (&x)[L], uint32_t nb, int lane, F4 load4, F1 load1) {
  static_assert(W >= 1 && W <= 32 && L >= 1 && TPI >= 1, "limbs of at most 32 bits");
  static_assert((uint64_t)TPI * L * W < (1ull << 28), "bit offsets stay in an int32");
  constexpr int ND = value_load_dwords<W, L>();
  constexpr uint32_t MASK = W == 32 ? 0xFFFFFFFFu : (uint32_t)((1ull << W) - 1u);
  const uint32_t bit0 = (uint32_t)lane * (uint32_t)(L * W), b0 = bit0 >> 3, sh = bit0 & 7u;
  uint32_t d[ND + 1];
  if (nb >= 4u) {
    // little-endian dword i of the lane: the value's bytes b0 + 4i .. b0 + 4i + 3 counted from its end, which lie at o .. o + 3
    const int32_t top = (int32_t)nb - 4 - (int32_t)b0;
#pragma unroll
    for (int i = 0; i < ND; ++i) {
      const int32_t o = top - 4 * i;
      d[i] = load4((uint32_t)(o > 0 ? o : 0));
    }
#pragma unroll
    for (int i = 0; i < ND; ++i) {
      const int32_t o = top - 4 * i;
      const uint32_t v = vload_bswap(d[i]);
      d[i] = o >= 0 ? v : o > -4 ? v >> (8u * (uint32_t)(-o)) : 0u;
    }
  } else {
    // at most three bytes: all of them in dword 0 of the lane they fall to
#pragma unroll
    for (int i = 0; i < ND; ++i) d[i] = 0u;
    for (uint32_t t = 0; t < nb; ++t)
      if (t >= b0 && t < b0 + 4u) d[0] |= load1(nb - 1u - t) << (8u * (t - b0));
  }
  d[ND] = 0u;
  // down to the lane's first bit, then limbs at compile-time offsets
#pragma unroll
  for (int i = 0; i < ND; ++i) d[i] = vload_align(d[i + 1], d[i], sh);
#pragma unroll
  for (int k = 0; k < L; ++k) {
    const int w = (k * W) >> 5, s = (k * W) & 31;
    x[k] = (s + W > 32 ? vload_align(d[w + 1], d[w], (uint32_t)s) : d[w] >> s) & MASK;
  }
}

}  // namespace bftkv

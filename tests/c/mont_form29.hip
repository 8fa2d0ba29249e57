/* The 18 x 4 form of the library's Montgomery multiplier at radix 2^29 (bftkv_amd/csrc/mont28.h with W = 29: the form of
 * k_rsa_modexp<18,4,29>) behind a kernel that does nothing else, the way tests/c/mont_forms.hip holds the 28-bit forms:
 * tests/test_gpu_mont29.py hands it raw limb rows -- limbs of 2^29, operands up to 2n - 1, x = R - 1 -- and reads back the
 * lazy output limb for limb, then the same row after canonicalize and after reduce_once.  Test infrastructure only; a
 * program of its own:
 *
 *   mont_form29 <input> <output>
 *
 * input : sections, each  u32 L (18), u32 TPI (4), u32 G,  then G records of  u32 op, u32 k, u32 n0inv, a[72], b[72], n[72]
 * output: per section G records of  lazy[72], canonical[72], reduced[72]
 * op    : 0 MUL    mont_mul<18,4,false,29>(a, b)          (a is the broadcast operand)
 *         1 SQR    mont_mul<18,4,true,29>(a, a)
 *         2 CHAIN  k squarings, each fed the previous lazy output unchanged, then mont_mul<18,4,false,29>(b, that)
 * Sections run one after the other.  Every HIP call is checked; the first error is printed and ends the program with a
 * non-zero status before anything else is launched. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../bftkv_amd/csrc/mont28.h"

using namespace bftkv;

enum : uint32_t { OP_MUL = 0, OP_SQR = 1, OP_CHAIN = 2 };
constexpr int BLOCK = 256;

template <int L, int TPI, int W>
__global__ void __launch_bounds__(BLOCK) k_mont_form(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t count) {
  constexpr int N = L * TPI;
  constexpr int GROUPS = BLOCK / TPI;          // numbers per block
  constexpr int REC = 3 + 3 * N;
  __shared__ uint32_t a_sh[GROUPS * N];
  if (blockIdx.x * GROUPS >= count) return;    // whole block idle
  const uint32_t grp = threadIdx.x / TPI;
  const int qlane = threadIdx.x % TPI;
  const uint32_t g = blockIdx.x * GROUPS + grp;
  const bool active = g < count;
  const uint32_t pi = active ? g : (count - 1);   // idle groups of the last block repeat the last operation
  const uint32_t* rec = in + (uint64_t)pi * REC;
  uint32_t* a_lds = a_sh + grp * N + qlane * L;   // this lane's slice of the group's broadcast operand
  const uint32_t* a_rd = a_sh + grp * N;

  const uint32_t op = rec[0], kk = rec[1], n0inv = rec[2];
  uint32_t a[L], b[L], n[L], y[L], t[L];
#pragma unroll
  for (int k = 0; k < L; ++k) {
    a[k] = rec[3 + qlane * L + k];
    b[k] = rec[3 + N + qlane * L + k];
    n[k] = rec[3 + 2 * N + qlane * L + k];
    y[k] = 0;
  }

  // One schedule per (op, k) class of the wave, every lane executing it on its own operands (the multiplier's DPP moves
  // cross group boundaries, so the groups of a wave stay in step, as they do in k_rsa_modexp); a lane keeps the result of
  // its own class.
  const uint32_t cls = (op << 16) | (op == OP_CHAIN ? (kk & 0xFFFFu) : 0u);
  uint64_t todo = __builtin_amdgcn_ballot_w64(true);
  while (todo) {
    const int lead = __builtin_ctzll(todo);
    const uint32_t cls_u = (uint32_t)__builtin_amdgcn_readlane((int)cls, lead);
    const bool live = (cls == cls_u);
    const uint32_t op_u = cls_u >> 16, k_u = cls_u & 0xFFFFu;
    if (op_u == OP_CHAIN) {
#pragma unroll
      for (int k = 0; k < L; ++k) t[k] = a[k];
      for (uint32_t i = 0; i < k_u; ++i) {
        uint32_t s[L];
#pragma unroll
        for (int k = 0; k < L; ++k) { s[k] = t[k]; a_lds[k] = t[k]; }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        mont_mul<L, TPI, true, W>(t, a_rd, s, n, n0inv, qlane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      }
      uint32_t s[L];
#pragma unroll
      for (int k = 0; k < L; ++k) { s[k] = t[k]; a_lds[k] = b[k]; }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      mont_mul<L, TPI, false, W>(t, a_rd, s, n, n0inv, qlane);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    } else {
#pragma unroll
      for (int k = 0; k < L; ++k) a_lds[k] = a[k];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if (op_u == OP_SQR) mont_mul<L, TPI, true, W>(t, a_rd, a, n, n0inv, qlane);
      else mont_mul<L, TPI, false, W>(t, a_rd, b, n, n0inv, qlane);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    if (live) {
#pragma unroll
      for (int k = 0; k < L; ++k) y[k] = t[k];
    }
    todo &= ~__builtin_amdgcn_ballot_w64(live);
  }

  uint32_t* o = out + (uint64_t)pi * 3 * N + qlane * L;
  if (active) {
#pragma unroll
    for (int k = 0; k < L; ++k) o[k] = y[k];
  }
  canonicalize<L, TPI, W>(y, qlane);
  if (active) {
#pragma unroll
    for (int k = 0; k < L; ++k) o[N + k] = y[k];
  }
  reduce_once<L, TPI, W>(y, n, qlane);
  if (active) {
#pragma unroll
    for (int k = 0; k < L; ++k) o[2 * N + k] = y[k];
  }
}

#define HIP_OK(call)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (call);                                                                            \
    if (e_ != hipSuccess) {                                                                            \
      fprintf(stderr, "mont_form29: %s: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      exit(2);                                                                                         \
    }                                                                                                  \
  } while (0)

template <int L, int TPI, int W>
static void run_section(const std::vector<uint32_t>& in, uint32_t count, std::vector<uint32_t>& out) {
  constexpr int N = L * TPI;
  constexpr int GROUPS = BLOCK / TPI;
  out.assign((size_t)count * 3 * N, 0xEEEEEEEEu);
  uint32_t *d_in = nullptr, *d_out = nullptr;
  HIP_OK(hipMalloc(&d_in, in.size() * sizeof(uint32_t)));
  HIP_OK(hipMalloc(&d_out, out.size() * sizeof(uint32_t)));
  HIP_OK(hipMemcpy(d_in, in.data(), in.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_out, out.data(), out.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  k_mont_form<L, TPI, W><<<dim3((count + GROUPS - 1) / GROUPS), dim3(BLOCK)>>>(d_in, d_out, count);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(out.data(), d_out, out.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_OK(hipFree(d_in));
  HIP_OK(hipFree(d_out));
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: mont_form29 <input> <output>\n"); return 1; }
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) { perror(argv[1]); return 1; }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) { perror(argv[2]); return 1; }
  uint32_t hdr[3];
  int sections = 0;
  while (fread(hdr, sizeof(uint32_t), 3, fi) == 3) {
    const uint32_t L = hdr[0], TPI = hdr[1], count = hdr[2];
    if (count == 0 || count > (1u << 16) || L * TPI > (uint32_t)MONT_NMAX) { fprintf(stderr, "mont_form29: bad section header\n"); return 1; }
    std::vector<uint32_t> in((size_t)count * (3 + 3 * L * TPI)), out;
    if (fread(in.data(), sizeof(uint32_t), in.size(), fi) != in.size()) { fprintf(stderr, "mont_form29: short section\n"); return 1; }
    if (L == 18 && TPI == 4) run_section<18, 4, 29>(in, count, out);
    else { fprintf(stderr, "mont_form29: no form <%u,%u>\n", L, TPI); return 1; }
    if (fwrite(out.data(), sizeof(uint32_t), out.size(), fo) != out.size()) { perror(argv[2]); return 1; }
    ++sections;
  }
  if (fclose(fo) != 0) { perror(argv[2]); return 1; }
  fclose(fi);
  printf("mont_form29: %d sections\n", sections);
  return 0;
}

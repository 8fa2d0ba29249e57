/* value_limbs (bftkv_amd/csrc/value_load.h) behind a kernel that does nothing else, with the lane geometry and the memory
 * functors of k_rsa_modexp: one group of TPI lanes per value, each lane writing the L limbs it got.  tests/test_gpu_value_load.py
 * places the values inside one blob between guard bytes, at every start alignment, and compares with integer slicing.  Test
 * infrastructure only; a program of its own:
 *
 *   value_load <input> <output>
 *
 * input : sections, each  u32 L, u32 TPI, u32 W, u32 G, u32 blob_len,  then G records of  u32 offset, u32 nb,  then the blob
 * output: per section G rows of TPI * L limbs (u32), least significant first
 * Every (offset, nb) is checked against blob_len on the host before anything is launched.  Sections run one after the other.
 * Every HIP call is checked; the first error is printed and ends the program with a non-zero status before anything else is
 * launched. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../bftkv_amd/csrc/value_load.h"

using namespace bftkv;

constexpr int BLOCK = 256;

template <int L, int TPI, int W>
__global__ void __launch_bounds__(BLOCK) k_value_load(const uint8_t* __restrict__ blob, const uint32_t* __restrict__ recs,
                                                      uint32_t* __restrict__ out, uint32_t count) {
  constexpr int N = L * TPI;
  constexpr int GROUPS = BLOCK / TPI;          // values per block
  if (blockIdx.x * GROUPS >= count) return;    // whole block idle
  const uint32_t grp = threadIdx.x / TPI;
  const int qlane = threadIdx.x % TPI;
  const uint32_t g = blockIdx.x * GROUPS + grp;
  const bool active = g < count;
  const uint32_t pi = active ? g : (count - 1);   // idle groups of the last block repeat the last value
  const uint32_t nb = recs[2 * pi + 1];
  const uint8_t* mp = blob + recs[2 * pi];
  uint32_t x[L];
  value_limbs<W, L, TPI>(x, nb, qlane,
                         [&](uint32_t o) -> uint32_t { uint32_t v; __builtin_memcpy(&v, mp + o, 4); return v; },
                         [&](uint32_t o) -> uint32_t { return mp[o]; });
  if (active) {
    uint32_t* o = out + (uint64_t)pi * N + qlane * L;
#pragma unroll
    for (int k = 0; k < L; ++k) o[k] = x[k];
  }
}

#define HIP_OK(call)                                                                                  \
  do {                                                                                                \
    hipError_t e_ = (call);                                                                           \
    if (e_ != hipSuccess) {                                                                           \
      fprintf(stderr, "value_load: %s: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      exit(2);                                                                                        \
    }                                                                                                 \
  } while (0)

template <int L, int TPI, int W>
static void run_section(const std::vector<uint32_t>& recs, const std::vector<uint8_t>& blob, uint32_t count, std::vector<uint32_t>& out) {
  constexpr int N = L * TPI;
  constexpr int GROUPS = BLOCK / TPI;
  out.assign((size_t)count * N, 0xEEEEEEEEu);
  uint8_t* d_blob = nullptr;
  uint32_t *d_recs = nullptr, *d_out = nullptr;
  HIP_OK(hipMalloc(&d_blob, blob.size()));
  HIP_OK(hipMalloc(&d_recs, recs.size() * sizeof(uint32_t)));
  HIP_OK(hipMalloc(&d_out, out.size() * sizeof(uint32_t)));
  HIP_OK(hipMemcpy(d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_recs, recs.data(), recs.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_out, out.data(), out.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  k_value_load<L, TPI, W><<<dim3((count + GROUPS - 1) / GROUPS), dim3(BLOCK)>>>(d_blob, d_recs, d_out, count);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(out.data(), d_out, out.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_OK(hipFree(d_blob));
  HIP_OK(hipFree(d_recs));
  HIP_OK(hipFree(d_out));
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: value_load <input> <output>\n"); return 1; }
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) { perror(argv[1]); return 1; }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) { perror(argv[2]); return 1; }
  uint32_t hdr[5];
  int sections = 0;
  while (fread(hdr, sizeof(uint32_t), 5, fi) == 5) {
    const uint32_t L = hdr[0], TPI = hdr[1], W = hdr[2], count = hdr[3], blob_len = hdr[4];
    if (count == 0 || count > (1u << 16) || blob_len == 0 || blob_len > (1u << 26)) { fprintf(stderr, "value_load: bad section header\n"); return 1; }
    std::vector<uint32_t> recs((size_t)count * 2), out;
    std::vector<uint8_t> blob(blob_len);
    if (fread(recs.data(), sizeof(uint32_t), recs.size(), fi) != recs.size() || fread(blob.data(), 1, blob_len, fi) != blob_len) {
      fprintf(stderr, "value_load: short section\n");
      return 1;
    }
    for (uint32_t i = 0; i < count; ++i)
      if (recs[2 * i] > blob_len || recs[2 * i + 1] > blob_len - recs[2 * i]) { fprintf(stderr, "value_load: value %u leaves the blob\n", i); return 1; }
    if (L == 18 && TPI == 4 && W == 29) run_section<18, 4, 29>(recs, blob, count, out);
    else if (L == 19 && TPI == 4 && W == 28) run_section<19, 4, 28>(recs, blob, count, out);
    else if (L == 10 && TPI == 8 && W == 28) run_section<10, 8, 28>(recs, blob, count, out);
    else if (L == 14 && TPI == 8 && W == 28) run_section<14, 8, 28>(recs, blob, count, out);
    else if (L == 19 && TPI == 8 && W == 28) run_section<19, 8, 28>(recs, blob, count, out);
    else { fprintf(stderr, "value_load: no form <%u,%u,%u>\n", L, TPI, W); return 1; }
    if (fwrite(out.data(), sizeof(uint32_t), out.size(), fo) != out.size()) { perror(argv[2]); return 1; }
    ++sections;
  }
  if (fclose(fo) != 0) { perror(argv[2]); return 1; }
  fclose(fi);
  printf("value_load: %d sections\n", sections);
  return 0;
}

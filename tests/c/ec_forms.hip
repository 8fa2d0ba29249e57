/* The field and point arithmetic of bftkv_amd/csrc/ec_field.h behind kernels that do nothing else, so that
 * tests/test_gpu_ec_forms.py can hand it raw word rows -- the Montgomery-form words themselves, points under any Z, infinity with
 * X and Y left in place, scalars at and above the order, every aliasing form: what the header's contracts admit and the C ABI's
 * hashed, inverted and reduced operands cannot express -- and read the result rows back.  The operations are those of
 * tests/c/ec_forms.h (the text tests/c/ec_forms_host.cpp compiles for the CPU suite), plus the two limb conversions of
 * ec_kernels.hip, which exist on the device only.  Test infrastructure only; a program of its own:
 *
 *   ec_forms <input> <output>
 *
 * input : four curve blocks, each  u32 L, u32 fbytes, u32 bits,  then P || N || B || Gx || Gy (fbytes each, big-endian) padded
 *         to a whole word; then sections, each  u32 L, u32 family, u32 count,  then count records of in_words(L, family) words
 * output: per section count rows of out_words(L, family) words
 * One kernel per (L, family), one thread per record, EC_BLOCK threads per block.  The fixed-base tables of G come from the
 * header's host-side fb_table_build.  Sections run one after the other.  Every HIP call is checked; the first error is printed
 * and ends the program with a non-zero status before anything else is launched. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../include/bftkv_gpu.h"
#include "../../bftkv_amd/csrc/mont28.h"        // MONT_N: the limb rows of ec_to_limbs28
#include "../../bftkv_amd/csrc/ec_kernels.hip"
#include "ec_forms.h"

using namespace ecforms;
using bftkv::EC_BLOCK;
static_assert(EC_FORM_LIMBS == (uint32_t)bftkv::MONT_N, "the limb row of ec_to_limbs28");

template <int L, uint32_t FAM>
__global__ void __launch_bounds__(EC_BLOCK) k_ec_form(ecf::Curve<L> C, Aux aux, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t count) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const uint32_t* rec = in + (uint64_t)t * in_words(L, FAM);
  uint32_t* row = out + (uint64_t)t * out_words(L, FAM);
  if constexpr (FAM == FAM_LIMBS) {
    uint32_t a[L], lim[EC_FORM_LIMBS];
    ecf::fe_copy<L>(a, rec);
    bftkv::ec_to_limbs28<L>(lim, a);
#pragma unroll
    for (int k = 0; k < (int)EC_FORM_LIMBS; ++k) row[k] = lim[k];
    ecf::fe_zero<L>(a);
    bftkv::ec_from_limbs28<L>(a, lim);
    ecf::fe_copy<L>(row + EC_FORM_LIMBS, a);
  } else {
    form_run<L, FAM>(C, aux, rec, row);
  }
}

#define HIP_OK(call)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (call);                                                                            \
    if (e_ != hipSuccess) {                                                                            \
      fprintf(stderr, "ec_forms: %s: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      exit(2);                                                                                         \
    }                                                                                                  \
  } while (0)

constexpr uint32_t MAX_COUNT = 1u << 16;

template <int L>
struct CurveState {
  ecf::Curve<L> C;
  Aux aux;
  bool ready = false;
  uint32_t *d_in = nullptr, *d_out = nullptr;          // sized for MAX_COUNT records of the widest family

  void setup(const uint8_t* be, uint32_t fbytes, uint32_t bits) {
    ecf::curve_setup<L>(C, be, fbytes);
    aux.bits = bits;
    for (uint32_t t = 0; t < EC_FORM_TABLES; ++t) {
      const uint32_t w = EC_FORM_W[t], nwin = ecf::fb_windows(fbytes, w);
      std::vector<uint32_t> host(ecf::fb_table_words<L>(w, nwin));
      ecf::fb_table_build<L>(host.data(), w, nwin, C);
      uint32_t* d = nullptr;
      HIP_OK(hipMalloc(&d, host.size() * sizeof(uint32_t)));
      HIP_OK(hipMemcpy(d, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
      aux.tab[t] = d;
      aux.w[t] = w;
      aux.nwin[t] = nwin;
    }
    HIP_OK(hipMalloc(&d_in, (size_t)MAX_COUNT * (1 + 6 * L) * sizeof(uint32_t)));
    HIP_OK(hipMalloc(&d_out, (size_t)MAX_COUNT * (EC_FORM_LIMBS + L) * sizeof(uint32_t)));
    ready = true;
  }

  template <uint32_t FAM>
  void launch(uint32_t count) {
    k_ec_form<L, FAM><<<dim3((count + EC_BLOCK - 1) / EC_BLOCK), dim3(EC_BLOCK)>>>(C, aux, d_in, d_out, count);
  }

  int run(uint32_t fam, const std::vector<uint32_t>& in, uint32_t count, std::vector<uint32_t>& out) {
    static_assert(in_words(L, FAM_ADD) >= in_words(L, FAM_H2I) && out_words(L, FAM_LIMBS) >= out_words(L, FAM_ADD), "buffer sizes");
    out.assign((size_t)count * out_words(L, fam), 0xEEEEEEEEu);
    HIP_OK(hipMemcpy(d_in, in.data(), in.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_out, out.data(), out.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    switch (fam) {
      case FAM_FE: launch<FAM_FE>(count); break;
      case FAM_INV: launch<FAM_INV>(count); break;
      case FAM_FN: launch<FAM_FN>(count); break;
      case FAM_DBL: launch<FAM_DBL>(count); break;
      case FAM_ADD: launch<FAM_ADD>(count); break;
      case FAM_ADDA: launch<FAM_ADDA>(count); break;
      case FAM_MUL: launch<FAM_MUL>(count); break;
      case FAM_FB: launch<FAM_FB>(count); break;
      case FAM_AFF: launch<FAM_AFF>(count); break;
      case FAM_CHK: launch<FAM_CHK>(count); break;
      case FAM_H2I: launch<FAM_H2I>(count); break;
      case FAM_XR: launch<FAM_XR>(count); break;
      case FAM_LIMBS: launch<FAM_LIMBS>(count); break;
      default: return 1;
    }
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out.data(), d_out, out.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
  }

  void release() {
    if (!ready) return;
    for (uint32_t t = 0; t < EC_FORM_TABLES; ++t) HIP_OK(hipFree((void*)aux.tab[t]));
    HIP_OK(hipFree(d_in));
    HIP_OK(hipFree(d_out));
  }
};

// One curve's state behind plain functions.  The whole program compiles from this file with one command; with -DEC_FORMS_ONLY_L=7, 8,
// 12 or 17 (and -c) an object holds one curve's kernels alone and with -DEC_FORMS_ONLY_L=0 main alone, so that the test can
// compile the five side by side and link them.
#define EC_FORMS_DECLARE(L)                                                                                           \
  bool ec_forms_setup_##L(const uint8_t* be, uint32_t fbytes, uint32_t bits);                                         \
  int ec_forms_run_##L(uint32_t fam, const std::vector<uint32_t>& in, uint32_t count, std::vector<uint32_t>& out);    \
  void ec_forms_release_##L();
#define EC_FORMS_DEFINE(L)                                                                                            \
  static CurveState<L> g_state_##L;                                                                                   \
  bool ec_forms_setup_##L(const uint8_t* be, uint32_t fbytes, uint32_t bits) {                                        \
    if (g_state_##L.ready) return false;                                                                              \
    g_state_##L.setup(be, fbytes, bits);                                                                              \
    return true;                                                                                                      \
  }                                                                                                                   \
  int ec_forms_run_##L(uint32_t fam, const std::vector<uint32_t>& in, uint32_t count, std::vector<uint32_t>& out) {   \
    return g_state_##L.ready ? g_state_##L.run(fam, in, count, out) : 1;                                              \
  }                                                                                                                   \
  void ec_forms_release_##L() { g_state_##L.release(); }
EC_FORMS_DECLARE(7)
EC_FORMS_DECLARE(8)
EC_FORMS_DECLARE(12)
EC_FORMS_DECLARE(17)
#if !defined(EC_FORMS_ONLY_L) || EC_FORMS_ONLY_L == 7
EC_FORMS_DEFINE(7)
#endif
#if !defined(EC_FORMS_ONLY_L) || EC_FORMS_ONLY_L == 8
EC_FORMS_DEFINE(8)
#endif
#if !defined(EC_FORMS_ONLY_L) || EC_FORMS_ONLY_L == 12
EC_FORMS_DEFINE(12)
#endif
#if !defined(EC_FORMS_ONLY_L) || EC_FORMS_ONLY_L == 17
EC_FORMS_DEFINE(17)
#endif

#if !defined(EC_FORMS_ONLY_L) || EC_FORMS_ONLY_L == 0
int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: ec_forms <input> <output>\n"); return 1; }
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) { perror(argv[1]); return 1; }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) { perror(argv[2]); return 1; }
  uint32_t hdr[3];
  for (int i = 0; i < 4; ++i) {
    if (fread(hdr, sizeof(uint32_t), 3, fi) != 3) { fprintf(stderr, "ec_forms: short curve block\n"); return 1; }
    const uint32_t L = hdr[0], fbytes = hdr[1], bits = hdr[2];
    if (fbytes == 0 || fbytes > 4 * L || L > 17 || (bits + 7) / 8 != fbytes) { fprintf(stderr, "ec_forms: bad curve block\n"); return 1; }
    std::vector<uint32_t> be((5 * fbytes + 3) / 4);
    if (fread(be.data(), sizeof(uint32_t), be.size(), fi) != be.size()) { fprintf(stderr, "ec_forms: short curve block\n"); return 1; }
    const uint8_t* b = (const uint8_t*)be.data();
    const bool ok = L == 7 ? ec_forms_setup_7(b, fbytes, bits) : L == 8 ? ec_forms_setup_8(b, fbytes, bits)
                  : L == 12 ? ec_forms_setup_12(b, fbytes, bits) : L == 17 ? ec_forms_setup_17(b, fbytes, bits) : false;
    if (!ok) { fprintf(stderr, "ec_forms: no curve of %u words, or given twice\n", L); return 1; }
  }
  int sections = 0;
  while (fread(hdr, sizeof(uint32_t), 3, fi) == 3) {
    const uint32_t L = hdr[0], fam = hdr[1], count = hdr[2];
    if (count == 0 || count > MAX_COUNT || fam >= FAM_COUNT || (L != 7 && L != 8 && L != 12 && L != 17)) {
      fprintf(stderr, "ec_forms: bad section header\n");
      return 1;
    }
    std::vector<uint32_t> in((size_t)count * in_words(L, fam)), out;
    if (fread(in.data(), sizeof(uint32_t), in.size(), fi) != in.size()) { fprintf(stderr, "ec_forms: short section\n"); return 1; }
    const int rc = L == 7 ? ec_forms_run_7(fam, in, count, out) : L == 8 ? ec_forms_run_8(fam, in, count, out)
                 : L == 12 ? ec_forms_run_12(fam, in, count, out) : ec_forms_run_17(fam, in, count, out);
    if (rc) { fprintf(stderr, "ec_forms: no family %u on a curve of %u words\n", fam, L); return 1; }
    if (fwrite(out.data(), sizeof(uint32_t), out.size(), fo) != out.size()) { perror(argv[2]); return 1; }
    ++sections;
  }
  ec_forms_release_7();
  ec_forms_release_8();
  ec_forms_release_12();
  ec_forms_release_17();
  if (fclose(fo) != 0) { perror(argv[2]); return 1; }
  fclose(fi);
  printf("ec_forms: %d sections\n", sections);
  return 0;
}
#endif

/* The operation table of tests/c/ec_forms.h compiled for the CPU (the same text tests/c/ec_forms.hip runs on the GPU, one thread
 * per record), so that tests/test_ec_forms_reference.py can hold the table and the exact expectations of tests/ec_form_cases.py to
 * each other without a GPU.  Test infrastructure only.
 *
 * efh_run(curve, fbytes, bits, family, count, in, out): curve = P || N || B || Gx || Gy (fbytes each, big-endian); in is count
 * records of in_words(L, family) raw words, out count rows of out_words(L, family) words.  0, or -1 for a curve or a family that
 * does not exist here (LIMBS is the device program's alone). */
#include <stdint.h>
#include <vector>
#include "ec_forms.h"

namespace {

using namespace ecforms;

template <int L, uint32_t FAM>
void run_family(const ecf::Curve<L>& C, const Aux& aux, uint32_t count, const uint32_t* in, uint32_t* out) {
  for (uint32_t t = 0; t < count; ++t) form_run<L, FAM>(C, aux, in + (size_t)t * in_words(L, FAM), out + (size_t)t * out_words(L, FAM));
}

template <int L>
int run(const uint8_t* curve, uint32_t f, uint32_t bits, uint32_t fam, uint32_t count, const uint32_t* in, uint32_t* out) {
  ecf::Curve<L> C;
  ecf::curve_setup<L>(C, curve, f);
  Aux aux = {};
  aux.bits = bits;
  std::vector<uint32_t> tabs[EC_FORM_TABLES];
  if (fam == FAM_FB) {
    for (uint32_t t = 0; t < EC_FORM_TABLES; ++t) {
      aux.w[t] = EC_FORM_W[t];
      aux.nwin[t] = ecf::fb_windows(f, aux.w[t]);
      tabs[t].resize(ecf::fb_table_words<L>(aux.w[t], aux.nwin[t]));
      ecf::fb_table_build<L>(tabs[t].data(), aux.w[t], aux.nwin[t], C);
      aux.tab[t] = tabs[t].data();
    }
  }
  switch (fam) {
    case FAM_FE: run_family<L, FAM_FE>(C, aux, count, in, out); return 0;
    case FAM_INV: run_family<L, FAM_INV>(C, aux, count, in, out); return 0;
    case FAM_FN: run_family<L, FAM_FN>(C, aux, count, in, out); return 0;
    case FAM_DBL: run_family<L, FAM_DBL>(C, aux, count, in, out); return 0;
    case FAM_ADD: run_family<L, FAM_ADD>(C, aux, count, in, out); return 0;
    case FAM_ADDA: run_family<L, FAM_ADDA>(C, aux, count, in, out); return 0;
    case FAM_MUL: run_family<L, FAM_MUL>(C, aux, count, in, out); return 0;
    case FAM_FB: run_family<L, FAM_FB>(C, aux, count, in, out); return 0;
    case FAM_AFF: run_family<L, FAM_AFF>(C, aux, count, in, out); return 0;
    case FAM_CHK: run_family<L, FAM_CHK>(C, aux, count, in, out); return 0;
    case FAM_H2I: run_family<L, FAM_H2I>(C, aux, count, in, out); return 0;
    case FAM_XR: run_family<L, FAM_XR>(C, aux, count, in, out); return 0;
  }
  return -1;
}

}  // namespace

extern "C" int efh_run(const uint8_t* curve, uint32_t fbytes, uint32_t bits, uint32_t fam, uint32_t count, const uint32_t* in, uint32_t* out) {
  switch (fbytes) {
    case 28: return run<7>(curve, fbytes, bits, fam, count, in, out);
    case 32: return run<8>(curve, fbytes, bits, fam, count, in, out);
    case 48: return run<12>(curve, fbytes, bits, fam, count, in, out);
    case 66: return run<17>(curve, fbytes, bits, fam, count, in, out);
  }
  return -1;
}

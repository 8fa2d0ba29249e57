/* plan_report::decide (csrc/plan_report.h), the host function that sizes the launches of a resident big verify call from the
 * words the device reported, as a program of its own: built with -fsanitize=address,undefined by tests/test_plan_report_host.py.
 * Reads cases, writes what decide() returned for each (plan_report::flatten); the test holds the expectations.
 *   plan_report_host <input> <output>
 * input:  u32 count, then per case 13 u32: total, n_items, enabled, overflow_arrived, overflow_items, flags_word, len_word[4],
 *         ring bits (1 RSA-3072, 2 RSA-4096, 4 DSA <= 2048, 8 DSA 3072, 16 batched inverse enqueued, 32 single inverse enqueued),
 *         wide_form, numbers per block of the main modexp pass (Geometry::modexp_main)
 * output: per case plan_report::N_SLOTS u32, then phase 1's modexp (main, 3072, 4096) and inverse (batched, single) grids, which
 *         the getter does not report */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../bftkv_amd/csrc/plan_report.h"

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: plan_report_host <input> <output>\n"); return 1; }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) { fprintf(stderr, "plan_report_host: cannot open files\n"); return 1; }
  uint32_t count = 0;
  if (fread(&count, 4, 1, fi) != 1) { fprintf(stderr, "plan_report_host: no header\n"); return 1; }
  std::vector<uint32_t> out((size_t)plan_report::N_SLOTS + 5);
  for (uint32_t i = 0; i < count; ++i) {
    uint32_t w[13];
    if (fread(w, 4, 13, fi) != 13) { fprintf(stderr, "plan_report_host: short case %u\n", i); return 1; }
    plan_report::Input in;
    in.total = w[0]; in.n_items = w[1]; in.enabled = w[2] != 0; in.overflow_arrived = w[3] != 0; in.overflow_items = w[4];
    in.flags_word = w[5];
    for (int k = 0; k < plan_report::N_LISTS; ++k) in.len_word[k] = w[6 + k];
    in.have_rsa3072 = (w[10] & 1u) != 0; in.have_rsa4096 = (w[10] & 2u) != 0; in.have_dsa2048 = (w[10] & 4u) != 0;
    in.have_dsa3072 = (w[10] & 8u) != 0; in.dsa_inv_batched = (w[10] & 16u) != 0; in.dsa_inv_single = (w[10] & 32u) != 0;
    in.wide_form = w[11] != 0;
    plan_report::Geometry geo;
    geo.modexp_main = w[12];
    const plan_report::Decision d = plan_report::decide(in, geo);
    plan_report::flatten(d, in, out.data());
    uint32_t* p1 = out.data() + plan_report::N_SLOTS;
    p1[0] = d.p1.modexp; p1[1] = d.p1.modexp3072; p1[2] = d.p1.modexp4096; p1[3] = d.p1.dsa_inv_batched; p1[4] = d.p1.dsa_inv;
    if (fwrite(out.data(), 4, out.size(), fo) != out.size()) { fprintf(stderr, "plan_report_host: write failed\n"); return 1; }
  }
  fclose(fi);
  if (fclose(fo) != 0) return 1;
  printf("plan_report_host: %u cases, %d slots each\n", count, (int)plan_report::N_SLOTS);
  return 0;
}

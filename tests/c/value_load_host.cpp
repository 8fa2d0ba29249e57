/* value_limbs (bftkv_amd/csrc/value_load.h), the loader k_rsa_modexp and k_rsav_verify start with, compiled for the host and run
 * lane by lane over heap buffers of EXACTLY nb bytes: built with -fsanitize=address,undefined by tests/test_value_load_host.py, so
 * a read one byte before or behind a value is a report and a non-zero exit.  The functors also refuse every offset the header
 * does not promise to stay within.  Test infrastructure only; a program of its own:
 *
 *   value_load_host <input> <output>
 *
 * input : u32 count, then count values of  u32 nb, nb bytes (most significant first)
 * output: per value, for each of the five forms in the order of FORMS below, its TPI * L limbs (u32), least significant first */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../bftkv_amd/csrc/value_load.h"

using namespace bftkv;

/* FORMS: <L, TPI, W> = <18,4,29> <19,4,28> <10,8,28> <14,8,28> <19,8,28> */

static void die(const char* what, uint32_t o, uint32_t nb) {
  fprintf(stderr, "value_load_host: %s at offset %u of a value of %u bytes\n", what, o, nb);
  exit(3);
}

template <int L, int TPI, int W>
static void run_form(const uint8_t* v, uint32_t nb, std::vector<uint32_t>& out) {
  for (int lane = 0; lane < TPI; ++lane) {
    uint32_t x[L];
    value_limbs<W, L, TPI>(
        x, nb, lane,
        [&](uint32_t o) -> uint32_t {
          if (nb < 4u || o > nb - 4u) die("load4", o, nb);
          uint32_t w;
          memcpy(&w, v + o, 4);
          return w;
        },
        [&](uint32_t o) -> uint32_t {
          if (o >= nb) die("load1", o, nb);
          return v[o];
        });
    for (int k = 0; k < L; ++k) out.push_back(x[k]);
  }
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: value_load_host <input> <output>\n"); return 1; }
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) { perror(argv[1]); return 1; }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) { perror(argv[2]); return 1; }
  uint32_t count = 0;
  if (fread(&count, 4, 1, fi) != 1) { fprintf(stderr, "value_load_host: no header\n"); return 1; }
  std::vector<uint32_t> out;
  for (uint32_t i = 0; i < count; ++i) {
    uint32_t nb = 0;
    if (fread(&nb, 4, 1, fi) != 1 || nb > (1u << 16)) { fprintf(stderr, "value_load_host: bad value header\n"); return 1; }
    uint8_t* v = (uint8_t*)malloc(nb);                     // exactly nb bytes: the sanitizer's red zones start right at both ends
    if (nb && (!v || fread(v, 1, nb, fi) != nb)) { fprintf(stderr, "value_load_host: short value\n"); return 1; }
    out.clear();
    run_form<18, 4, 29>(v, nb, out);
    run_form<19, 4, 28>(v, nb, out);
    run_form<10, 8, 28>(v, nb, out);
    run_form<14, 8, 28>(v, nb, out);
    run_form<19, 8, 28>(v, nb, out);
    free(v);
    if (fwrite(out.data(), 4, out.size(), fo) != out.size()) { perror(argv[2]); return 1; }
  }
  if (fclose(fo) != 0) { perror(argv[2]); return 1; }
  fclose(fi);
  printf("value_load_host: %u values\n", count);
  return 0;
}

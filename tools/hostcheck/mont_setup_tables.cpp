// CPU: prints what hostbn::mont_setup and hostbn::mont_setup_by_doubling give for moduli named on the command line, at any limb
// width and count, so that a test can hold them against plain integers (tests/test_mont29_tables.py: the 72 x 29-bit tables of
// k_rsa_modexp<18,4,29>).   mont_setup_tables W nlimbs hex-modulus...
// One line per modulus and form:  <"fast"|"doubling"> <ok> <n0inv> <n limbs...> <r2 limbs...>   (all hex)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../bftkv_amd/csrc/host_bignum.h"
using namespace bftkv::hostbn;

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: mont_setup_tables W nlimbs hex-modulus...\n"); return 1; }
  const int W = atoi(argv[1]), nl = atoi(argv[2]);
  if (W < 8 || W > 31 || nl < 1 || nl > 1024) { fprintf(stderr, "bad width or limb count\n"); return 1; }
  for (int a = 3; a < argc; ++a) {
    const char* h = argv[a];
    const size_t hl = strlen(h);
    std::vector<uint8_t> be((hl + 1) / 2, 0);
    for (size_t i = 0; i < hl; ++i) {
      const char ch = h[hl - 1 - i];
      const int v = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : ch >= 'A' && ch <= 'F' ? ch - 'A' + 10 : -1;
      if (v < 0) { fprintf(stderr, "bad hex digit\n"); return 1; }
      be[be.size() - 1 - i / 2] |= (uint8_t)(v << (4 * (i & 1)));
    }
    for (int form = 0; form < 2; ++form) {
      std::vector<uint32_t> n(nl, 0xEEEEEEEEu), r2(nl, 0xEEEEEEEEu);
      uint32_t n0 = 0xEEEEEEEEu;
      const bool ok = form == 0 ? mont_setup(be.data(), (uint32_t)be.size(), nl, n.data(), r2.data(), &n0, W)
                                : mont_setup_by_doubling(be.data(), (uint32_t)be.size(), nl, n.data(), r2.data(), &n0, W);
      printf("%s %d %x", form == 0 ? "fast" : "doubling", (int)ok, n0);
      for (int j = 0; j < nl; ++j) printf(" %x", n[j]);
      for (int j = 0; j < nl; ++j) printf(" %x", r2[j]);
      printf("\n");
    }
  }
  return 0;
}

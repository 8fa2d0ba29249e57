/* The rules of raw RSA signing that need no multiplier, bftkv_amd/csrc/rsa_sign.h, compiled for the CPU (the same text k_rsas_em,
 * k_rsas_value, k_rsas_crt and k_rsas_finish compile for the GPU) into a stand-alone program, so that tests/test_rsa_sign_reference.py
 * can check them against the Python restatement in the CPU suite.  Test infrastructure only.
 *
 * One case per line of standard input, one answer per line of standard output:
 *   E <nbytes> <n row in hex> <hash id> <digest in hex> <key refused: 0|1>   ->  <rule byte> <limb 0> .. <limb 79> of em
 *   V <nbytes> <value row in hex>                                            ->  <limb 0> .. <limb 79>
 *   D <pbytes> <exponent row in hex>                                         ->  the 2 pbytes window digits, most significant first
 *   R <nbytes> <n row> <pbytes> <p row> <q row>                              ->  <refused: 0|1>
 *   S <rule byte> <fits: 0|1> <check: 0|1>                                   ->  <status byte> */
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../bftkv_amd/csrc/rsa_sign.h"

static int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }
static bool unhex(const char* s, std::vector<uint8_t>* out) {
  out->clear();
  const size_t n = strlen(s);
  if (n & 1) return false;
  for (size_t i = 0; i < n; i += 2) {
    const int a = hexval(s[i]), b = hexval(s[i + 1]);
    if (a < 0 || b < 0) return false;
    out->push_back((uint8_t)(a * 16 + b));
  }
  return true;
}

int main() {
  static char line[1 << 16], h1[1 << 12], h2[1 << 12], h3[1 << 12];
  std::vector<uint8_t> a, b, c;      // exact-size buffers: a read past any of them is the sanitizers' to find
  while (fgets(line, sizeof line, stdin)) {
    unsigned nbytes, pbytes, hash_id, refused, rule, fits, check;
    if (sscanf(line, "E %u %4095s %u %4095s %u", &nbytes, h1, &hash_id, h2, &refused) == 5) {
      if (!unhex(h1, &a) || !unhex(h2, &b) || a.size() != nbytes || nbytes == 0 || bftkv::rsav_prefix_len(hash_id) < 0 || b.empty()) { printf("bad line\n"); return 1; }
      const uint32_t k = bftkv::rsav_kbytes(a.data(), nbytes), dlen = (uint32_t)b.size();
      printf("%u", (unsigned)bftkv::rsas_rule(k, dlen + (uint32_t)bftkv::rsav_prefix_len(hash_id), refused != 0));
      for (uint32_t j = 0; j < (uint32_t)bftkv::RSAS_VALUE_LIMBS; ++j) printf(" %u", bftkv::rsas_em_limb(j, k, hash_id, b.data(), dlen));
      printf("\n");
    } else if (sscanf(line, "V %u %4095s", &nbytes, h1) == 2) {
      if (!unhex(h1, &a) || a.size() != nbytes || nbytes == 0) { printf("bad line\n"); return 1; }
      for (uint32_t j = 0; j < (uint32_t)bftkv::RSAS_VALUE_LIMBS; ++j) printf("%s%u", j ? " " : "", bftkv::rsas_value_limb(j, a.data(), nbytes));
      printf("\n");
    } else if (sscanf(line, "D %u %4095s", &pbytes, h1) == 2) {
      if (!unhex(h1, &a) || a.size() != pbytes || pbytes == 0) { printf("bad line\n"); return 1; }
      for (uint32_t w = 2 * pbytes; w-- > 0;) printf("%u%s", bftkv::rsas_digit(a.data(), pbytes, w), w ? " " : "");
      printf("\n");
    } else if (sscanf(line, "R %u %4095s %u %4095s %4095s", &nbytes, h1, &pbytes, h2, h3) == 5) {
      if (!unhex(h1, &a) || !unhex(h2, &b) || !unhex(h3, &c) || a.size() != nbytes || b.size() != pbytes || c.size() != pbytes || !nbytes || !pbytes) {
        printf("bad line\n");
        return 1;
      }
      printf("%u\n", bftkv::rsas_key_refused(a.data(), nbytes, b.data(), c.data(), pbytes) ? 1u : 0u);
    } else if (sscanf(line, "S %u %u %u", &rule, &fits, &check) == 3) {
      printf("%u\n", (unsigned)bftkv::rsas_status((uint8_t)rule, fits != 0, check != 0));
    } else {
      printf("bad line\n");
      return 1;
    }
  }
  return 0;
}

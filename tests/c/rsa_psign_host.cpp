/* The rules of threshold RSA signing that need no multiplier, bftkv_amd/csrc/rsa_psign.h, compiled for the CPU (the same text
 * k_psign_em and k_psign_pow compile for the GPU) into a stand-alone program, so that tests/test_rsa_psign_reference.py can check them
 * against the Python restatement in the CPU suite.  Test infrastructure only.
 *
 * One case per line of standard input, one answer per line of standard output:
 *   E <nbytes> <modulus row, 2 nbytes hex digits> <T in hex, or ->     ->  <emlen> <refusal byte> <limb 0> .. <limb 75>
 *   S <sign byte> <magnitude is zero: 0|1> <refused: 0|1> <m has no inverse: 0|1>     ->  <negative: 0|1> <status byte> */
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../bftkv_amd/csrc/rsa_psign.h"

static int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }
static bool unhex(const char* s, std::vector<uint8_t>* out) {
  out->clear();
  if (!strcmp(s, "-")) return true;
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
  static char line[1 << 16], mod_hex[1 << 12], t_hex[1 << 12];
  std::vector<uint8_t> mod, t;
  while (fgets(line, sizeof line, stdin)) {
    unsigned nbytes, sb, zero, refused, noinv;
    if (sscanf(line, "E %u %4095s %4095s", &nbytes, mod_hex, t_hex) == 3) {
      if (!unhex(mod_hex, &mod) || !unhex(t_hex, &t) || mod.size() != nbytes || nbytes == 0) { printf("bad line\n"); return 1; }
      // exact-size copies: a read past either buffer is the sanitizers' to find
      std::vector<uint8_t> mrow(mod), trow(t);
      const uint32_t emlen = bftkv::psign_emlen(mrow.data(), nbytes), tl = (uint32_t)trow.size();
      printf("%u %u", emlen, bftkv::psign_refused(emlen, tl) ? (unsigned)bftkv::PSIGN_INVALID_INPUT : (unsigned)bftkv::PSIGN_OK);
      for (uint32_t j = 0; j < 76; ++j) printf(" %u", bftkv::psign_em_limb(j, emlen, trow.data(), tl));
      printf("\n");
    } else if (sscanf(line, "S %u %u %u %u", &sb, &zero, &refused, &noinv) == 4) {
      const bool neg = bftkv::psign_negative((uint8_t)sb, zero != 0);
      printf("%u %u\n", neg ? 1u : 0u, (unsigned)bftkv::psign_status(refused != 0, neg, noinv != 0));
    } else {
      printf("bad line\n");
      return 1;
    }
  }
  return 0;
}

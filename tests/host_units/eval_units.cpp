// Stand-alone driver of the evaluation-form plans and host helpers (csrc/fr.hpp, csrc/plans.hpp: no
// GPU, no HIP header). tests/test_eval_units.py builds it plain and with
// -fsanitize=address,undefined, feeds it cases on stdin and compares every answer with Python
// integers; the program judges nothing.
//
// A 256-bit value travels as 64 hex digits, most significant first. Cases:
//   plan EXP T        eval_plan: the fields
//   open EXP FLAGS    open_evals_plan: the fields
//   tiles N T         batch_inverse_tiles
//   host EXP Z        fr_eval_setup for the domain of size 2^EXP and the point Z, canonical values on
//                     one line: z, z^n, 1/n, (z^n - 1)/n, then w^(2^k) for k < 26
//   inv A             fr_inv_binary and fr_inv of A mod r, canonical, on one line
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../kzg-setup-powersoftau_amd/csrc/fr.hpp"
#include "../../kzg-setup-powersoftau_amd/csrc/plans.hpp"

using namespace kzgpot;

static bool parse(const char* s, uint8_t le[32]) {  // a string that ends early fails at its terminator
  memset(le, 0, 32);
  for (int i = 0; i < 64; i++) {
    const char c = s[i];
    const int d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
    if (d < 0) return false;
    const int bit = 4 * (63 - i);
    le[bit >> 3] |= (uint8_t)(d << (bit & 7));
  }
  return true;
}
static void print_value(const fr& a, char end) {
  uint8_t be[32];
  fr_to_be32(be, a);
  for (int k = 0; k < 32; k++) printf("%02x", be[k]);
  putchar(end);
}
static void kv(const char* k, uint64_t v) { printf("%s=%" PRIu64 " ", k, v); }

static void print_plan(uint32_t exp, uint32_t t) {
  const EvalPlan p = eval_plan(exp, t);
  kv("bytes", p.bytes);
  if (p.bytes) {
    kv("exp", p.exp), kv("t", p.t), kv("n", p.n), kv("tiles", p.tiles), kv("inv", p.inv), kv("sums", p.sums);
    kv("qsums", p.qsums), kv("words", p.words), kv("value_at", kEvalValueAt);
    kv("ws", eval_workspace_bytes(exp, KZGPOT_POLY_TILE(t)));
  }
  putchar('\n');
}

static void print_open(uint32_t exp, uint32_t flags) {
  const OpenEvalsPlan p = open_evals_plan(exp, flags);
  kv("ok", p.ok), kv("bytes", p.bytes);
  if (p.ok) {
    kv("n", p.ev.n), kv("t", p.ev.t), kv("c", p.c), kv("rec", p.rec), kv("ev_bytes", p.ev.bytes), kv("quot", p.quot);
    kv("msm", p.msm), kv("msm_bytes", msm_workspace_bytes(false, p.ev.n, p.c));
  }
  putchar('\n');
}

static void print_host(uint32_t exp, const uint8_t z[32]) {
  fr_eval_scalars sc;
  fr_eval_setup(sc, exp, z);
  print_value(sc.z, ' ');
  print_value(fr_pow_2k(sc.z, exp), ' ');
  print_value(fr_inv_2k(exp), ' ');
  print_value(sc.scale, ' ');
  for (int k = 0; k < kEvalPowers; k++) print_value(sc.pw[k], k + 1 < kEvalPowers ? ' ' : '\n');
}

int main() {
  char* line = nullptr;
  size_t cap = 0;
  long at = 0;
  bool ok = true;
  while (ok && getline(&line, &cap, stdin) > 0) {
    at++;
    char op[16] = "", s1[80] = "";
    unsigned a = 0, b = 0;
    unsigned long long n = 0;
    uint8_t z[32];
    if (sscanf(line, "%15s", op) < 1) continue;
    if (!strcmp(op, "plan") && sscanf(line, "%*s %u %u", &a, &b) == 2) {
      print_plan(a, b);
    } else if (!strcmp(op, "open") && sscanf(line, "%*s %u %u", &a, &b) == 2) {
      print_open(a, b);
    } else if (!strcmp(op, "tiles") && sscanf(line, "%*s %llu %u", &n, &b) == 2) {
      kv("tiles", batch_inverse_tiles(n, b));
      putchar('\n');
    } else if (!strcmp(op, "host") && sscanf(line, "%*s %u %79s", &a, s1) == 2 && a <= kEvalMaxExp && parse(s1, z)) {
      print_host(a, z);
    } else if (!strcmp(op, "inv") && sscanf(line, "%*s %79s", s1) == 1 && parse(s1, z)) {
      const fr x = fr_from_le32(z);
      print_value(fr_inv_binary(x), ' ');
      print_value(fr_inv(x), '\n');
    } else {
      ok = false;
    }
  }
  free(line);
  if (!ok) {
    fprintf(stderr, "eval_units: bad case on line %ld\n", at);
    return 2;
  }
  printf("eval_units ok\n");
  return 0;
}

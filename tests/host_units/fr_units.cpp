// Stand-alone driver of the scalar field module (csrc/fr.hpp, included alone: no GPU, no HIP
// header). tests/test_fr_units.py builds it plain and with -fsanitize=address,undefined, feeds it one
// case per line on stdin and compares every answer with Python integers; the program itself judges
// nothing but the two compile-time constants.
//
// A 256-bit value travels as 64 hex digits, most significant first. Cases:
//   load A        A mod r                        mul A B / add A B   (A op B) mod r
//   pow A E       A^E mod r                      inv A               A^(r-2) mod r
//   rm1shr K      the integer (r - 1) >> K       rm2                 the integer r - 2
//   one           the Montgomery one, raw words  root K              7^((r-1) >> K) mod r
//   table A       A^(2^k) mod r, k < 64          bytes A             A mod r from A's 32 LE bytes,
//                                                                    as LE bytes then as BE bytes
#include <stdio.h>
#include <string.h>

#include "../../kzg-setup-powersoftau_amd/csrc/fr.hpp"

using namespace kzgpot;

// 2^256 mod r and 2^512 mod r (Python: pow(2, 256, r), pow(2, 512, r)), 8 LE words
constexpr uint32_t kR[8] = {0xfffffffeu, 0x00000001u, 0x00034802u, 0x5884b7fau,
                            0xecbc4ff5u, 0x998c4fefu, 0xacc5056fu, 0x1824b159u};
constexpr uint32_t kR2[8] = {0xf3f29c6du, 0xc999e990u, 0x87925c23u, 0x2b6cedcbu,
                             0x7254398fu, 0x05d31496u, 0x9f59ff11u, 0x0748d9d9u};
constexpr bool same_words(const uint32_t (&a)[8], const uint32_t (&b)[8]) {
  for (int i = 0; i < 8; i++)
    if (a[i] != b[i]) return false;
  return true;
}
static_assert(same_words(FR_RADIX.one, kR), "FR_RADIX.one is 2^256 mod r");
static_assert(same_words(FR_RADIX.r2, kR2), "FR_RADIX.r2 is 2^512 mod r");

// the plain integer of 64 hex digits; false: malformed
static bool parse(const char* s, fr& a) {
  if (!s || strlen(s) != 64) return false;
  a = fr{};
  for (int i = 0; i < 64; i++) {
    const char c = s[i];
    const int d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
    if (d < 0) return false;
    const int bit = 4 * (63 - i);
    a.v[bit >> 5] |= (uint32_t)d << (bit & 31);
  }
  return true;
}
static void print_words(const fr& a, char end = '\n') {  // the words as they are
  for (int k = 7; k >= 0; k--) printf("%08x", a.v[k]);
  putchar(end);
}
static void print_value(const fr& mont, char end = '\n') {  // an element's canonical value
  fr c;
  fr_store(c, mont);
  print_words(c, end);
}
static bool load(const char* s, fr& mont) {
  fr a;
  if (!parse(s, a)) return false;
  fr_load(mont, a);
  return true;
}

int main() {
  char line[256];
  long n = 0;
  while (fgets(line, sizeof line, stdin)) {
    n++;
    const char* op = strtok(line, " \n");
    const char* s1 = strtok(nullptr, " \n");
    const char* s2 = strtok(nullptr, " \n");
    if (!op) continue;
    fr a, b, o;
    bool ok = true;
    if (!strcmp(op, "load")) {
      if ((ok = load(s1, a))) print_value(a);
    } else if (!strcmp(op, "mul") || !strcmp(op, "add")) {
      if ((ok = load(s1, a) && load(s2, b))) {
        if (op[0] == 'm') fr_mul(o, a, b);
        else fr_add(o, a, b);
        print_value(o);
      }
    } else if (!strcmp(op, "pow")) {
      if ((ok = load(s1, a) && parse(s2, b))) print_value(fr_pow(a, b));
    } else if (!strcmp(op, "inv")) {
      if ((ok = load(s1, a))) print_value(fr_inv(a));
    } else if (!strcmp(op, "rm1shr") || !strcmp(op, "root")) {
      unsigned k = 0;
      if ((ok = s1 && sscanf(s1, "%u", &k) == 1 && k <= 32)) {
        if (op[1] == 'm') print_words(fr_rm1_shr(k));
        else print_value(fr_domain_root(k));
      }
    } else if (!strcmp(op, "rm2")) {
      print_words(fr_r_minus(2));
    } else if (!strcmp(op, "one")) {
      print_words(fr_one());
    } else if (!strcmp(op, "table")) {
      if ((ok = load(s1, a))) {
        fr_powers<64> t;
        fr_fill_powers(t.p, a);
        for (int k = 0; k < 64; k++) print_value(t.p[k], k < 63 ? ' ' : '\n');
      }
    } else if (!strcmp(op, "bytes")) {
      if ((ok = parse(s1, a))) {
        uint8_t in[32], le[32], be[32];
        for (int i = 0; i < 32; i++) in[i] = (uint8_t)(a.v[i >> 2] >> (8 * (i & 3)));
        const fr x = fr_from_le32(in);
        fr_to_le32(le, x);
        fr_to_be32(be, x);
        for (int i = 0; i < 32; i++) printf("%02x", le[i]);
        putchar(' ');
        for (int i = 0; i < 32; i++) printf("%02x", be[i]);
        putchar('\n');
      }
    } else {
      ok = false;
    }
    if (!ok) {
      fprintf(stderr, "fr_units: bad case on line %ld\n", n);
      return 2;
    }
  }
  printf("fr_units ok\n");
  return 0;
}

// Stand-alone driver of the Fr NTT's plan and index arithmetic (csrc/fr.hpp, csrc/plans.hpp,
// csrc/ntt_parts.hpp: no GPU, no HIP header). tests/test_ntt_units.py builds it plain and with
// -fsanitize=address,undefined, feeds it cases on stdin and compares every answer with Python
// integers; the program judges nothing.
//
// `ntt` executes ntt_plan sequentially the way ntt_kernels.hip does, through the same index
// functions: the two twiddle tables from the powers w^(2^k), then for each pass, for each block:
// stage the block's slots into an array, run the pass's stages on it, store the slots. Pass 0 reads
// the input and writes the output array, the later passes work on the output array in place.
//
// A 256-bit value travels as 64 hex digits, most significant first. Cases:
//   ntt EXP T INV      the next line holds the 2^EXP inputs; answer: the outputs on one line
//   sub A B            (A - B) mod r
//   plan EXP T         ntt_plan: the fields, then pass=q0,c,lb,stride,blocks per pass
//   bounds EXP T       per pass: max=load,store,twiddle_lo,twiddle_hi,slot, the largest element
//                      index loaded and stored, table index read and LDS slot touched, over
//                      every block (EXP <= 18) or over the blocks 0, 2^i, last, last - 2^i (the
//                      indices are ORs of disjoint bit fields, so those reach every field's maximum)
//   domain G2 EXP T    open_domain_plan: the fields
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../kzg-setup-powersoftau_amd/csrc/fr.hpp"
#include "../../kzg-setup-powersoftau_amd/csrc/ntt_parts.hpp"
#include "../../kzg-setup-powersoftau_amd/csrc/plans.hpp"

using namespace kzgpot;

static bool parse(const char* s, fr& a) {  // a string that ends early fails at its terminator
  if (!s) return false;
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
static void print_words(const fr& a, char end) {
  for (int k = 7; k >= 0; k--) printf("%08x", a.v[k]);
  putchar(end);
}
static void kv(const char* k, uint64_t v) { printf("%s=%" PRIu64 " ", k, v); }

// out = the transform of in (plain integers in, canonical values out)
static void run_ntt(const NttPlan& p, bool inverse, const std::vector<fr>& in, std::vector<fr>& out) {
  const uint64_t m = (uint64_t)1 << p.exp;
  fr w = fr_domain_root(p.exp);
  if (inverse) w = fr_pow(w, fr{{(uint32_t)(m - 1), 0, 0, 0, 0, 0, 0, 0}});
  fr pw[26];
  fr_fill_powers(pw, w);
  fr scale = {{1, 0, 0, 0, 0, 0, 0, 0}};
  if (inverse) fr_store(scale, fr_inv(fr_from_u64(m)));
  auto table = [&](uint32_t bits, uint32_t first) {
    std::vector<fr> t((size_t)1 << bits);
    for (uint32_t j = 0; j < t.size(); j++) {
      fr acc = fr_one();
      for (uint32_t k = 0; k < bits; k++)
        if ((j >> k) & 1) fr_mul(acc, acc, pw[first + k]);
      t[j] = acc;
    }
    return t;
  };
  const std::vector<fr> lo = table(p.lo_bits, 0), hi = table(p.hi_bits, p.lo_bits);
  out.assign(m, fr{});
  std::vector<fr> slots((size_t)1 << p.tl);
  for (uint32_t k = 0; k < p.npass; k++) {
    const NttPass& ps = p.pass[k];
    const bool first = k == 0, last = k + 1 == p.npass;
    const uint32_t n = 1u << (ps.c + ps.lb);
    for (uint64_t blk = 0; blk < ps.blocks; blk++) {
      for (uint32_t s = 0; s < n; s++) {
        const uint64_t g = ntt_load_index(ps, p.exp, blk, s);
        slots.at(s) = first ? in.at(g) : out.at(g);
        if (first) fr_load(slots[s], slots[s]);
      }
      for (uint32_t j = 0; j < ps.c; j++)
        for (uint32_t b = 0; b < n / 2; b++) {
          const uint32_t s0 = ntt_lower_slot(ps, j, b), s1 = s0 + ntt_slot_gap(ps, j);
          const uint64_t e = ntt_twiddle_exp(ps, p.exp, blk, j, b);
          fr tw, t;
          fr_mul(tw, lo.at(ntt_tw_lo(p.lo_bits, e)), hi.at(ntt_tw_hi(p.lo_bits, e)));
          const fr x = slots.at(s0);
          fr_mul(t, slots.at(s1), tw);
          fr_add(slots[s0], x, t);
          fr_sub(slots[s1], x, t);
        }
      for (uint32_t s = 0; s < n; s++) {
        fr a = slots[s];
        if (last) fr_mul(a, a, scale);
        out.at(ntt_store_index(ps, blk, s)) = a;
      }
    }
  }
}

static void print_plan(uint32_t exp, uint32_t t) {
  const NttPlan p = ntt_plan(exp, t);
  kv("bytes", p.bytes);
  if (p.bytes) {
    kv("exp", p.exp), kv("t", p.t), kv("tl", p.tl), kv("npass", p.npass), kv("lo_bits", p.lo_bits);
    kv("hi_bits", p.hi_bits), kv("tw_lo", p.tw_lo), kv("tw_hi", p.tw_hi), kv("tw_bytes", p.tw_bytes);
    kv("stage_bytes", p.stage_bytes);
    for (uint32_t k = 0; k < p.npass; k++) {
      const NttPass& s = p.pass[k];
      printf("pass=%u,%u,%u,%" PRIu64 ",%" PRIu64 " ", s.q0, s.c, s.lb, s.stride, s.blocks);
    }
  }
  putchar('\n');
}

static void print_bounds(uint32_t exp, uint32_t t) {
  const NttPlan p = ntt_plan(exp, t);
  kv("bytes", p.bytes);
  for (uint32_t k = 0; p.bytes && k < p.npass; k++) {
    const NttPass& ps = p.pass[k];
    std::vector<uint64_t> blocks;
    if (exp <= 18) {
      for (uint64_t b = 0; b < ps.blocks; b++) blocks.push_back(b);
    } else {
      blocks = {0, ps.blocks - 1};
      for (uint64_t bit = 1; bit < ps.blocks; bit <<= 1) blocks.push_back(bit), blocks.push_back(ps.blocks - 1 - bit);
    }
    const uint32_t n = 1u << (ps.c + ps.lb);
    uint64_t load = 0, store = 0, tlo = 0, thi = 0, slot = 0;
    auto up = [](uint64_t& m, uint64_t v) { m = v > m ? v : m; };
    for (const uint64_t blk : blocks) {
      for (uint32_t s = 0; s < n; s++) up(load, ntt_load_index(ps, exp, blk, s)), up(store, ntt_store_index(ps, blk, s));
      for (uint32_t j = 0; j < ps.c; j++)
        for (uint32_t b = 0; b < n / 2; b++) {
          const uint64_t e = ntt_twiddle_exp(ps, exp, blk, j, b);
          up(tlo, ntt_tw_lo(p.lo_bits, e)), up(thi, ntt_tw_hi(p.lo_bits, e));
          up(slot, ntt_lower_slot(ps, j, b) + ntt_slot_gap(ps, j));
        }
    }
    printf("max=%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 " ", load, store, tlo, thi, slot);
  }
  putchar('\n');
}

static void print_domain(bool g2, uint32_t exp, uint32_t t) {
  const OpenDomainPlan p = open_domain_plan(g2, exp, t);
  kv("ok", p.ok), kv("bytes", p.bytes);
  if (p.ok) {
    kv("n", p.n), kv("rec", p.rec), kv("rows", work_rows(g2)), kv("ntt_in", p.ntt_in), kv("scalars", p.scalars);
    kv("ntt_tw", p.ntt_tw), kv("rows_a", p.rows_a), kv("rows_b", p.rows_b), kv("tw_a", p.tw_a), kv("tw_b", p.tw_b);
    kv("ntt_tw_bytes", ntt_plan(exp + 1, t).tw_bytes), kv("ntt_tw_bytes_out", ntt_plan(exp, t).tw_bytes);
    kv("tw_a_bytes", fft_twiddle_bytes(exp + 1)), kv("tw_b_bytes", fft_twiddle_bytes(exp));
    kv("gather_src", p.gather_src), kv("gather_dst", p.gather_dst), kv("gather_cnt", p.gather_cnt);
    kv("table_ws", open_domain_table_workspace_bytes(g2, exp)), kv("ws", open_domain_workspace_bytes(g2, exp, KZGPOT_POLY_TILE(t)));
    for (uint32_t k = 0; k < kDomainSteps; k++) printf("step=%u ", (unsigned)p.step[k]);
  }
  putchar('\n');
}

int main() {
  char* line = nullptr;
  size_t cap = 0;
  long at = 0;
  bool ok = true;
  while (ok && getline(&line, &cap, stdin) > 0) {
    at++;
    char op[16] = "", s1[80] = "", s2[80] = "";
    unsigned a = 0, b = 0, c = 0;
    if (sscanf(line, "%15s", op) < 1) continue;
    if (!strcmp(op, "ntt")) {
      ok = sscanf(line, "%*s %u %u %u", &a, &b, &c) == 3 && ntt_plan(a, b).bytes && getline(&line, &cap, stdin) > 0;
      if (!ok) break;
      at++;
      const size_t m = (size_t)1 << a;
      std::vector<fr> in(m), out;
      ok = strlen(line) >= 65 * m - 1;
      for (size_t i = 0; ok && i < m; i++) ok = parse(line + 65 * i, in[i]);
      if (!ok) break;
      run_ntt(ntt_plan(a, b), c != 0, in, out);
      for (size_t i = 0; i < m; i++) print_words(out[i], i + 1 < m ? ' ' : '\n');
    } else if (!strcmp(op, "sub")) {
      fr x, y, o;
      ok = sscanf(line, "%*s %79s %79s", s1, s2) == 2 && parse(s1, x) && parse(s2, y);
      if (!ok) break;
      fr_load(x, x), fr_load(y, y);
      fr_sub(o, x, y);
      fr_store(o, o);
      print_words(o, '\n');
    } else if (!strcmp(op, "plan") && sscanf(line, "%*s %u %u", &a, &b) == 2) {
      print_plan(a, b);
    } else if (!strcmp(op, "bounds") && sscanf(line, "%*s %u %u", &a, &b) == 2) {
      print_bounds(a, b);
    } else if (!strcmp(op, "domain") && sscanf(line, "%*s %u %u %u", &a, &b, &c) == 3) {
      print_domain(a != 0, b, c);
    } else {
      ok = false;
    }
  }
  free(line);
  if (!ok) {
    fprintf(stderr, "ntt_units: bad case on line %ld\n", at);
    return 2;
  }
  printf("ntt_units ok\n");
  return 0;
}

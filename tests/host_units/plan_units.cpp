// Stand-alone driver of the launch plans (csrc/plans.hpp, included alone: no GPU, no HIP header).
// tests/test_plan_units.py builds it plain and with -fsanitize=address,undefined, feeds it one case per
// line on stdin and checks every printed region, stage, level and step; the program judges nothing.
//
// Every answer is one line of key=value tokens; a schedule entry is one token of comma-separated
// numbers (~0 prints as 18446744073709551615). Cases:
//   msm G2 N C         msm_plan: the fields, then step=mode,in_base,out_base,lanes,nseg,seg_len,
//                      seg_chunks,off_in,off_out per k_msm_sum launch
//   msmws G2 N FLAGS   bytes=msm_workspace_bytes for the MSM's flags (0: invalid), width=msm_window_bits(N)
//   poly N T           poly_plan: the fields, then level=cnt,off,tiles,pow0 per level
//   fft G2 EXP INV     fft_plan: the fields, then stage=lognb,logh,uniform per stage
//   open N NBLIND FLAGS  open_plan: the fields, and the sizes of what it stacks (poly_ws, msm_ws)
//   grid N BLOCK       grid_for
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "../../kzg-setup-powersoftau_amd/csrc/plans.hpp"

using namespace kzgpot;

static void kv(const char* k, uint64_t v) { printf("%s=%" PRIu64 " ", k, v); }

static void print_msm(bool g2, uint64_t n, uint32_t c) {
  const MsmPlan p = msm_plan(g2, n, c);
  kv("ok", p.ok), kv("bytes", p.bytes);
  if (p.ok) {
    kv("c", p.c), kv("nwin", p.nwin), kv("nb", p.nb), kv("levels", p.levels), kv("ntiles", p.ntiles);
    kv("nseg", p.nseg), kv("entries", p.entries), kv("cap", p.cap), kv("base_a", p.base_a), kv("base_b", p.base_b);
    kv("cnt", p.cnt), kv("off_a", p.off_a), kv("off_b", p.off_b), kv("sums", p.sums), kv("idx", p.idx);
    kv("pool", p.pool), kv("rows", work_rows(g2)), kv("scan_tile", kScanTile), kv("chunk", kMsmChunk);
    kv("nsteps", p.nsteps), kv("final_base", p.final_base);
    for (uint32_t k = 0; k < p.nsteps; k++) {
      const MsmStep& s = p.step[k];
      printf("step=%u,%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%u,%u,%u,%" PRIu64 ",%" PRIu64 " ", s.mode, s.in_base,
             s.out_base, s.lanes, s.nseg, s.seg_len, s.seg_chunks, s.off_in, s.off_out);
    }
  }
  putchar('\n');
}

static void print_poly(uint64_t n, uint32_t t) {
  const PolyPlan p = poly_plan(n, t);
  kv("bytes", p.bytes), kv("top", p.top), kv("powers", kPolyPowers), kv("reads", kPolyTileMax);
  if (p.bytes)
    for (uint32_t k = 0; k <= p.top; k++) {
      const PolyLevel& l = p.level[k];
      printf("level=%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%u ", l.cnt, l.off, l.tiles, l.pow0);
    }
  putchar('\n');
}

static void print_fft(bool g2, uint32_t exp, bool inverse) {
  const FftPlan p = fft_plan(g2, exp, inverse);
  kv("ok", p.ok), kv("bytes", p.bytes);
  if (p.ok) {
    kv("m", p.m), kv("half", p.half), kv("work", p.work), kv("rows", work_rows(g2)), kv("scale", p.scale);
    kv("twiddle_bytes", fft_twiddle_bytes(exp)), kv("workspace_bytes", fft_workspace_bytes(g2, exp));
    kv("nstages", p.nstages);
    for (uint32_t k = 0; k < p.nstages; k++)
      printf("stage=%u,%u,%d ", p.stage[k].lognb, p.stage[k].logh, (int)p.stage[k].uniform);
  }
  putchar('\n');
}

static void print_open(uint64_t n, uint64_t n_blind, uint32_t flags) {
  const OpenPlan p = open_plan(n, n_blind, flags);
  kv("ok", p.ok), kv("bytes", p.bytes);
  if (p.ok) {
    kv("t", p.t), kv("c", p.c), kv("nq", p.nq), kv("nb", p.nb), kv("rec", p.rec);
    kv("bases", p.bases), kv("scalars", p.scalars), kv("values", p.values), kv("poly", p.poly), kv("msm", p.msm);
    kv("poly_ws", poly_workspace_bytes(n > n_blind ? n : n_blind, p.t));
    kv("msm_ws", msm_workspace_bytes(false, p.nq + p.nb, p.c));
  }
  putchar('\n');
}

int main() {
  char line[256];
  long at = 0;
  while (fgets(line, sizeof line, stdin)) {
    at++;
    char op[16];
    uint64_t a = 0, b = 0, c = 0;
    const int got = sscanf(line, "%15s %" SCNu64 " %" SCNu64 " %" SCNu64, op, &a, &b, &c);
    if (got < 1) continue;
    if (!strcmp(op, "msm") && got == 4) {
      print_msm(a != 0, b, (uint32_t)c);
    } else if (!strcmp(op, "msmws") && got == 4) {
      uint32_t w;
      kv("bytes", msm_flags((uint32_t)c, w) ? msm_workspace_bytes(a != 0, b, w) : 0);
      kv("width", msm_window_bits(b));
      putchar('\n');
    } else if (!strcmp(op, "poly") && got == 3) {
      print_poly(a, (uint32_t)b);
    } else if (!strcmp(op, "fft") && got == 4) {
      print_fft(a != 0, (uint32_t)b, c != 0);
    } else if (!strcmp(op, "open") && got == 4) {
      print_open(a, b, (uint32_t)c);
    } else if (!strcmp(op, "grid") && got == 3) {
      kv("blocks", grid_for(a, (uint32_t)b));
      putchar('\n');
    } else {
      fprintf(stderr, "plan_units: bad case on line %ld\n", at);
      return 2;
    }
  }
  printf("plan_units ok\n");
  return 0;
}

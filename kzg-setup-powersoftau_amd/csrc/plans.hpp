// The launch plans of the group FFT (fft_kernels.hip), the multi-scalar multiplication
// (msm_kernels.hip), the polynomial division (poly_kernels.hip), KZG10 open (open.hip), the Fr NTT
// (ntt_kernels.hip), the amortized openings over a domain (domain.hip), the evaluation form
// (eval_kernels.hip, evals.hip), the pairing product (pairing_kernels.hip) and KZG10 check /
// batch_check (verify.hip), each stated once: where every kernel reads and writes inside the
// caller-supplied workspace, and the launch schedule as data (one entry per stage, level or step, in
// launch order). The launchers run the tables; nothing else decides an offset or a lane count.
//
// Plain C++17 with no HIP header, so a host program can include this file alone
// (tests/host_units/plan_units.cpp, built by g++ with and without sanitizers; tests/test_plan_units.py
// checks every launch's reads and writes against its regions; tests/host_units/ntt_units.cpp and
// tests/test_ntt_units.py do the same for the NTT's and the domain's plans,
// tests/host_units/eval_units.cpp and tests/test_eval_units.py for the evaluation form's,
// tests/host_units/verify_units.cpp and tests/test_verify_units.py for the pairing's and the check's).
#pragma once
#include <stdint.h>

#include "../../include/kzgpot.h"

namespace kzgpot {

constexpr uint64_t align256(uint64_t x) { return (x + 255) & ~(uint64_t)255; }  // every workspace region's size
// blocks of `block` lanes for n items; one block (whose lanes all leave) for none
inline unsigned grid_for(uint64_t n, uint32_t block) { return (unsigned)(n ? (n + block - 1) / block : 1); }

// ---------------------------------------------------------------- records and work rows
// rows of a work-row point (group_parts.hpp): x and y of NW = 14 (G1) or 28 (G2) words, the infinity mark
constexpr uint32_t kWorkRowsG1 = 2 * 14 + 1, kWorkRowsG2 = 2 * 28 + 1;
constexpr uint64_t work_rows(bool g2) { return g2 ? kWorkRowsG2 : kWorkRowsG1; }
// one ark-uncompressed point, and one base of an MSM: that, or (mont) the loaders' in-memory GroupAffine
constexpr uint64_t point_record(bool g2) { return g2 ? 192 : 96; }
constexpr uint64_t base_record(bool g2, bool mont) {
  return !mont ? point_record(g2) : g2 ? KZGPOT_G2_ARK_MONT_BYTES : KZGPOT_G1_ARK_MONT_BYTES;
}

// ---------------------------------------------------------------- group FFT
// d_work: the twiddle table (m/2 + 1 scalars of 32 B: w^(+-j) for j < m/2, then 1/m), then the work
// rows of m points. Stage st has half-block h = 2^logh = 2^st and nb = 2^lognb = m / 2h blocks; the
// uniform instantiation runs where the nb butterflies that share a twiddle fill whole waves.
constexpr uint32_t kFftMaxExp = 32;
struct FftStage {
  uint32_t lognb, logh;
  bool uniform;
};
struct FftPlan {
  uint64_t m, half;            // points; butterflies per stage
  uint64_t work, bytes;        // byte offset of the work rows (= the twiddle table's size); the total
  uint32_t nstages;
  FftStage stage[kFftMaxExp];
  bool scale;                  // the inverse's pass [1/m] over all m points (1/m = 1 at m = 1)
  bool ok;
};
inline FftPlan fft_plan(bool g2, uint32_t exp, bool inverse) {
  FftPlan p = {};
  if (exp > kFftMaxExp) return p;
  p.m = (uint64_t)1 << exp;
  p.half = p.m >> 1;
  p.work = align256((p.half + 1) * 32);
  p.bytes = p.work + p.m * work_rows(g2) * 4;
  p.nstages = exp;
  for (uint32_t st = 0; st < exp; st++) {
    const uint32_t lognb = exp - 1 - st;
    p.stage[st] = FftStage{lognb, st, lognb >= 6};
  }
  p.scale = inverse && exp > 0;
  p.ok = true;
  return p;
}
inline uint64_t fft_twiddle_bytes(uint32_t exp) { return fft_plan(false, exp, false).work; }
inline uint64_t fft_workspace_bytes(bool g2, uint32_t exp) { return fft_plan(g2, exp, false).bytes; }

// ---------------------------------------------------------------- multi-scalar multiplication
constexpr uint32_t kMsmChunk = 64;  // L: no lane sums more entries than this
constexpr uint64_t kMsmMaxN = 1ull << 26;
constexpr uint32_t kMsmWindowMax = 16;
constexpr uint32_t kMsmFlags = KZGPOT_MSM_BASES_MONT | KZGPOT_MSM_WINDOW(0x1f);
// KZGPOT_MSM_WINDOW(c) in the flags: c = 0 (the library chooses) or the width; false: above kMsmWindowMax
inline bool msm_window_flag(uint32_t flags, uint32_t& c) {
  c = (flags >> 8) & 0x1fu;
  return c <= kMsmWindowMax;
}
// the MSM's flags; false: an unknown bit or an invalid width
inline bool msm_flags(uint32_t flags, uint32_t& c) { return msm_window_flag(flags, c) && !(flags & ~kMsmFlags); }

// the exclusive scan of the NB bucket counts: tiles of kScanTile entries, then one block over the tile sums
constexpr int kScanItems = 8, kScanTile = 256 * kScanItems;
// bucket levels: L^levels >= n; bit-partial levels: 2^(c-1) entries per segment in chunks of L down to one
constexpr uint32_t kMsmMaxLevels = 6, kMsmMaxBitLevels = 3, kMsmMaxSteps = kMsmMaxLevels + kMsmMaxBitLevels;
constexpr uint64_t kMsmNoOffsets = ~0ull;  // MsmStep::off_out of a step that writes no chunk offsets
static_assert((uint64_t)kScanTile * kScanTile >= ((uint64_t)kMsmWindowMax << kMsmWindowMax),
              "NB <= 16 x 2^16 (c = 16): one block scans the tile sums");
static_assert((uint64_t)kMsmChunk * kMsmChunk * kMsmChunk * kMsmChunk * kMsmChunk * kMsmChunk >= kMsmMaxN,
              "step[] holds every bucket level of the largest n");
static_assert((1ull << (kMsmWindowMax - 1)) <= (uint64_t)kMsmChunk * kMsmChunk * kMsmChunk,
              "step[] holds every bit-partial level of the widest window");

// One k_msm_sum launch (msm_kernels.hip documents the modes). `lanes` lanes write the pool slots
// [out_base, out_base + lanes); they read below in_base + (the previous step's lanes), or for mode 0
// the n bases through idx. Modes 0, 1 (a bucket level): k_msm_chunks and the scan turn the entry
// offsets off_in into the chunk offsets off_out first. Modes 2, 3 (a bit-partial level): nseg
// segments of seg_len entries in seg_chunks chunks; mode 2 finds its entries through off_in.
struct MsmStep {
  uint32_t mode, nseg, seg_len, seg_chunks;
  uint64_t in_base, out_base, lanes;  // pool slots
  uint64_t off_in, off_out;           // byte offsets of the two offset arrays, or kMsmNoOffsets
};
// Workspace layout and schedule for (g2, n, c): W = ceil(256 / c) windows, NB = W 2^c buckets.
// Partial sums ping-pong between two regions A and B of the pool behind the n bases, the offsets
// between the arrays off_a and off_b. A level with `in` entries has at most min(in, in / L + NB)
// chunks (ceil(x / L) <= x, and <= x / L + 1 per non-empty bucket), so the regions are sized by
// U1 = min(E, E / L + NB) and U2 = min(U1, U1 / L + NB) for E = n W entries, and both hold the bit
// partials' first level, W c ceil(2^(c-1) / L) chunks.
struct MsmPlan {
  uint32_t c, nwin, nb, levels, ntiles;  // levels: the bucket levels, steps [0, levels)
  uint32_t nseg;                         // W c bit partials
  uint64_t entries;                      // n W: the sorted point indices
  uint64_t cap, base_a, base_b;          // pool slots: the total, and where A and B start
  uint64_t cnt, off_a, off_b, sums, idx, pool, bytes;  // byte offsets
  uint32_t nsteps;
  MsmStep step[kMsmMaxSteps];
  uint64_t final_base;  // k_msm_final reads the nseg slots from here
  bool ok;
};
inline MsmPlan msm_plan(bool g2, uint64_t n, uint32_t c) {
  constexpr uint64_t L = kMsmChunk;
  MsmPlan p = {};
  if (n > kMsmMaxN || c < 1 || c > kMsmWindowMax) return p;
  p.c = c;
  p.nwin = (256 + c - 1) / c;
  p.nb = p.nwin << c;
  p.nseg = p.nwin * c;
  p.entries = n * p.nwin;
  if (p.entries >= (1ull << 32)) return p;  // offsets and entry counts are 32-bit
  p.levels = 1;
  for (uint64_t r = L; r < n; r *= L) p.levels++;
  uint64_t upper[kMsmMaxLevels + 1] = {p.entries};  // upper[k]: entries of level k at most
  for (uint32_t k = 0; k < p.levels; k++) {
    const uint64_t in = upper[k], by_bucket = in / L + p.nb;
    upper[k + 1] = in < by_bucket ? in : by_bucket;
  }
  const uint64_t bits0 = (uint64_t)p.nseg * ((((uint64_t)1 << (c - 1)) + L - 1) / L);
  const uint64_t u1 = upper[1], u2 = p.levels > 1 ? upper[2] : 0;
  const uint64_t cap_a = u1 > bits0 ? u1 : bits0, cap_b = u2 > bits0 ? u2 : bits0;
  p.base_a = n;
  p.base_b = n + cap_a;
  p.cap = n + cap_a + cap_b;
  p.ntiles = (p.nb + kScanTile - 1) / kScanTile;
  uint64_t o = 0;
  p.cnt = o, o += align256((uint64_t)p.nb * 4);
  p.off_a = o, o += align256((uint64_t)(p.nb + 1) * 4);
  p.off_b = o, o += align256((uint64_t)(p.nb + 1) * 4);
  p.sums = o, o += align256((uint64_t)(p.ntiles + 1) * 4);
  p.idx = o, o += align256(p.entries * 4);
  p.pool = o, o += align256(p.cap * work_rows(g2) * 4);
  p.bytes = o;

  uint64_t in_base = 0, out_base = p.base_a;  // level 0 reads the bases and writes A
  uint64_t off_in = p.off_a, off_out = p.off_b;
  auto push = [&](MsmStep s) {
    s.in_base = in_base, s.out_base = out_base;
    p.step[p.nsteps++] = s;
    in_base = out_base;
    out_base = in_base == p.base_a ? p.base_b : p.base_a;
  };
  for (uint32_t k = 0; k < p.levels; k++) {
    push(MsmStep{k ? 1u : 0u, 0, 0, 0, 0, 0, upper[k + 1], off_in, off_out});
    const uint64_t t = off_in;
    off_in = off_out;
    off_out = t;
  }
  uint32_t seg_len = 1u << (c - 1), mode = 2;
  do {
    const uint32_t chunks = (seg_len + kMsmChunk - 1) / kMsmChunk;
    push(MsmStep{mode, p.nseg, seg_len, chunks, 0, 0, (uint64_t)p.nseg * chunks, off_in, kMsmNoOffsets});
    seg_len = chunks;
    mode = 3;
  } while (seg_len > 1);
  p.final_base = in_base;
  p.ok = true;
  return p;
}

// Width table: c = 8 below the first threshold, one more at each threshold n reaches. The
// thresholds are the smallest n at which the model
//   n W + B + 43 (W max(min(n, 2^c), n / L) + B / L),   W = ceil(256 / c), B = W c 2^(c-1)
// (bucket additions, bit-partial additions, and one inversion of about 43 additions' worth per
// level-0 partial) prefers c to c - 1 (tests/test_msm_model.py recomputes them). Narrower windows
// than 8 would win the model below n = 300 only, where the call is launch-bound; they are reachable
// by override.
constexpr uint64_t kWidthFrom[8] = {28416, 55872, 120384, 238720, 472064, 1114113, 2244609, 3669568};  // c = 9 .. 16
inline uint32_t msm_window_bits(uint64_t n) {
  uint32_t c = 8;
  for (uint64_t t : kWidthFrom)
    if (n >= t) c++;
  return c;
}
// 0 where (n, c) is not supported. c = 0: "the library's choice, msm_window_bits(n)". That width
// grows with n while the sorted-entry array (n W words) shrinks with the width, so the size for
// c = 0 is the largest over the widths 8 .. c(n): every term is monotone in n for a fixed width,
// hence so is this maximum.
inline uint64_t msm_workspace_bytes(bool g2, uint64_t n, uint32_t c) {
  if (c) return msm_plan(g2, n, c).bytes;  // 0 unless ok
  uint64_t bytes = 0;
  for (uint32_t w = 8; w <= msm_window_bits(n); w++) {
    const MsmPlan p = msm_plan(g2, n, w);
    if (!p.ok) return 0;
    if (p.bytes > bytes) bytes = p.bytes;
  }
  return bytes;
}

// ---------------------------------------------------------------- polynomial division
// t: tile width 2^t, kPolyTileMin .. kPolyTileMax. z_pow.p[k] = z^(2^k), kPolyPowers entries.
constexpr uint32_t kPolyTileMin = 8, kPolyTileMax = 12, kPolyTile = 11;
constexpr uint64_t kPolyMaxN = (1ull << 26) + 1;
constexpr int kPolyPowers = 64;
constexpr uint32_t kPolyMaxLevels = 4;
constexpr uint32_t kPolyFlags = KZGPOT_POLY_TILE(0xf);
// KZGPOT_POLY_TILE(t) in the flags: t, or the library's for 0; false: outside kPolyTileMin .. kPolyTileMax
inline bool poly_tile_flag(uint32_t flags, uint32_t& t) {
  t = (flags >> 16) & 0xfu;
  if (!t) t = kPolyTile;
  return t >= kPolyTileMin && t <= kPolyTileMax;
}
// the division's flags; false: an unknown bit or an invalid tile
inline bool poly_flags(uint32_t flags, uint32_t& t) { return poly_tile_flag(flags, t) && !(flags & ~kPolyFlags); }

// 2^26 + 1 entries in tiles of 2^8 leave 5 at level 3, and level k's multiplier is z^(S^k), whose
// powers y^(2^j), j < kPolyTileMax, are z_pow's entries k t + j
static_assert(((kPolyMaxN - 1) >> (3 * kPolyTileMin)) + 1 <= (1u << kPolyTileMin), "at most kPolyMaxLevels levels");
static_assert((kPolyMaxLevels - 1) * kPolyTileMax + kPolyTileMax <= (uint32_t)kPolyPowers,
              "z_pow holds the top level's powers");

// Level k has cnt entries of 32 B in `tiles` tiles; level 0 is the caller's array (off unused),
// levels 1 .. top live in the workspace at byte offset off, one entry per tile of the level below.
struct PolyLevel {
  uint64_t cnt, off, tiles;
  uint32_t pow0;  // the level reads z_pow.p[pow0 .. pow0 + kPolyTileMax)
};
struct PolyPlan {
  uint32_t top;
  PolyLevel level[kPolyMaxLevels];
  uint64_t bytes;  // 0: invalid arguments
};
inline PolyPlan poly_plan(uint64_t n, uint32_t t) {
  PolyPlan p = {};
  if (n > kPolyMaxN || t < kPolyTileMin || t > kPolyTileMax) return p;
  for (uint64_t cnt = n;; p.top++) {
    PolyLevel& l = p.level[p.top];
    l.cnt = cnt;
    l.tiles = (cnt + ((uint64_t)1 << t) - 1) >> t;
    l.pow0 = p.top * t;
    if (p.top) {
      l.off = p.bytes;
      p.bytes += align256(cnt * 32);
    }
    if (l.tiles <= 1) break;
    cnt = l.tiles;
  }
  if (!p.bytes) p.bytes = 256;  // a size of 0 means invalid arguments
  return p;
}
inline uint64_t poly_workspace_bytes(uint64_t n, uint32_t t) { return poly_plan(n, t).bytes; }

// ---------------------------------------------------------------- KZG10 open
// Workspace: the two base ranges end to end (what the one MSM reads), the two quotients end to
// end (its scalars), the two evaluations, the division's levels, the MSM's own workspace.
constexpr uint32_t kOpenFlags = kPolyFlags | kMsmFlags;
inline bool open_flags(uint32_t flags, uint32_t& t, uint32_t& c) {
  return poly_tile_flag(flags, t) && msm_window_flag(flags, c) && !(flags & ~kOpenFlags);
}
struct OpenPlan {
  uint32_t t, c;  // c: the width override, 0 for the library's
  uint64_t nq, nb, rec;
  uint64_t bases, scalars, values, poly, msm, bytes;  // byte offsets
  bool ok;
};
inline OpenPlan open_plan(uint64_t n, uint64_t n_blind, uint32_t flags) {
  OpenPlan p = {};
  if (!open_flags(flags, p.t, p.c) || n > kPolyMaxN || n_blind > kPolyMaxN) return p;
  p.nq = n ? n - 1 : 0;
  p.nb = n_blind ? n_blind - 1 : 0;
  p.rec = base_record(false, flags & KZGPOT_MSM_BASES_MONT);
  const uint64_t msm_bytes = msm_workspace_bytes(false, p.nq + p.nb, p.c);
  if (!msm_bytes) return p;
  uint64_t o = 0;
  p.bases = o, o += align256((p.nq + p.nb) * p.rec);
  p.scalars = o, o += align256((p.nq + p.nb) * 32);
  p.values = o, o += 256;
  p.poly = o, o += poly_workspace_bytes(n > n_blind ? n : n_blind, p.t);  // one division at a time
  p.msm = o, o += msm_bytes;
  p.bytes = o;
  p.ok = true;
  return p;
}

// ---------------------------------------------------------------- evaluation form (eval_kernels.hip)
// n = 2^exp evaluations in tiles of 2^t (the division's tiles and flag). Workspace of the division
// in evaluation form: inv (n entries of 32 B, 1 / (z - w^i) in Montgomery form), sums and qsums (one
// partial sum of 32 B per tile: the barycentric sum, and the sum behind the quotient's entry m when
// z = w^m), and 256 B of words: the index m at byte 0 (a 32-bit word, all ones unless z is on the
// domain) and the value at byte 32 (canonical).
constexpr uint32_t kEvalMaxExp = 26;
constexpr uint64_t kEvalMaxN = (uint64_t)1 << kEvalMaxExp;  // of the batch inversion too
constexpr uint32_t kEvalNoIndex = ~0u;
constexpr uint64_t kEvalValueAt = 32;  // inside the words region
struct EvalPlan {
  uint32_t exp, t;
  uint64_t n, tiles;
  uint64_t inv, sums, qsums, words, bytes;  // byte offsets; bytes = 0: invalid arguments
};
inline EvalPlan eval_plan(uint32_t exp, uint32_t t) {
  EvalPlan p = {};
  if (exp > kEvalMaxExp || t < kPolyTileMin || t > kPolyTileMax) return p;
  p.exp = exp, p.t = t;
  p.n = (uint64_t)1 << exp;
  p.tiles = (p.n + ((uint64_t)1 << t) - 1) >> t;
  uint64_t o = 0;
  p.inv = o, o += align256(p.n * 32);
  p.sums = o, o += align256(p.tiles * 32);
  p.qsums = o, o += align256(p.tiles * 32);
  p.words = o, o += 256;
  p.bytes = o;
  return p;
}
inline uint64_t eval_workspace_bytes(uint32_t exp, uint32_t flags) {
  uint32_t t;
  return poly_flags(flags, t) ? eval_plan(exp, t).bytes : 0;
}
// tiles of a batch inversion of n entries; 0: invalid arguments or nothing to do
inline uint64_t batch_inverse_tiles(uint64_t n, uint32_t t) {
  if (n > kEvalMaxN || t < kPolyTileMin || t > kPolyTileMax) return 0;
  return (n + ((uint64_t)1 << t) - 1) >> t;
}

// KZG10 open from evaluations: the division's workspace, the quotient's n evaluations (the one
// MSM's scalars; its bases are the caller's Lagrange records where they lie), the MSM's workspace.
struct OpenEvalsPlan {
  EvalPlan ev;
  uint32_t c;  // the width override, 0 for the library's
  uint64_t rec;
  uint64_t quot, msm, bytes;  // byte offsets (the division's workspace is at 0)
  bool ok;
};
inline OpenEvalsPlan open_evals_plan(uint32_t exp, uint32_t flags) {
  OpenEvalsPlan p = {};
  uint32_t t;
  if (!open_flags(flags, t, p.c)) return p;
  p.ev = eval_plan(exp, t);
  if (!p.ev.bytes) return p;
  const uint64_t msm_bytes = msm_workspace_bytes(false, p.ev.n, p.c);
  if (!msm_bytes) return p;
  p.rec = base_record(false, flags & KZGPOT_MSM_BASES_MONT);
  uint64_t o = p.ev.bytes;
  p.quot = o, o += align256(p.ev.n * 32);
  p.msm = o, o += msm_bytes;
  p.bytes = o;
  p.ok = true;
  return p;
}

// ---------------------------------------------------------------- pairing product (pairing_kernels.hip)
// One lane per pair. A lane's state is kPairLaneCells cells of one Fq2 (28 words) each, word-major
// across `stride` lanes (the pair count rounded up to the Miller kernel's block), followed by the
// kPairFinalCells cells of the one lane that runs the final exponentiation. The product tree is one
// k_pair_tree launch per level: `count` live values `step` lanes apart, 256 of them per block.
constexpr uint64_t kPairMaxK = KZGPOT_PAIRING_MAX_PAIRS;
constexpr uint32_t kPairMillerBlock = 64, kPairLaneCells = 29, kPairFinalCells = 56, kPairCellBytes = 112;
constexpr uint32_t kPairMaxLevels = 2;
static_assert(256ull * 256 >= kPairMaxK, "level[] holds every level of the largest product");
struct PairLevel {
  uint64_t count, step;
  uint32_t blocks;
};
struct PairingPlan {
  uint64_t k, stride;
  uint64_t lanes, final_cells, bytes;  // byte offsets; bytes = 0: invalid arguments
  uint32_t nlevels;
  PairLevel level[kPairMaxLevels];
  bool ok;
};
inline PairingPlan pairing_plan(uint64_t k) {
  PairingPlan p = {};
  if (k > kPairMaxK) return p;
  p.k = k;
  p.stride = (uint64_t)grid_for(k, kPairMillerBlock) * kPairMillerBlock;
  uint64_t o = 0;
  p.lanes = o, o += align256(p.stride * kPairLaneCells * kPairCellBytes);
  p.final_cells = o, o += align256((uint64_t)kPairFinalCells * kPairCellBytes);
  p.bytes = o;
  for (uint64_t count = k, step = 1; count > 1; count = (count + 255) / 256, step *= 256)
    p.level[p.nlevels++] = PairLevel{count, step, grid_for(count, 256)};
  p.ok = true;
  return p;
}
inline uint64_t pairing_workspace_bytes(uint64_t k) { return pairing_plan(k).bytes; }

// ---------------------------------------------------------------- KZG10 check and batch_check (verify.hip)
// n proofs. Workspace: the one MSM's bases end to end (commitments, proofs, g, gamma_g: 2 n + 2
// records), its scalars (rho_i, rho_i z_i, -sum rho_i v_i, -sum rho_i vbar_i), the Fr pass's partial
// sums (two per block of 256), the pairing product's two pairs (total_c and -total_w, then h and
// beta_h), a key of its own for the second MSM (over the proofs where they lie in `bases`; the first
// MSM has checked the same records under their indices), the MSMs' workspace, the pairing's.
constexpr uint64_t kCheckMaxN = (1ull << 25) - 1;
constexpr uint32_t kCheckFlags = KZGPOT_MSM_WINDOW(0x1f);
struct CheckPlan {
  uint64_t n, nbases, blocks;
  uint32_t c;  // the width override, 0 for the library's
  uint64_t bases, scalars, sums, pairs_g1, pairs_g2, key2, msm, pairing, bytes;  // byte offsets
  bool ok;
};
inline CheckPlan check_plan(uint64_t n, uint32_t flags) {
  CheckPlan p = {};
  if (n > kCheckMaxN || (flags & ~kCheckFlags) || !msm_window_flag(flags, p.c)) return p;
  p.n = n;
  p.nbases = 2 * n + 2;
  p.blocks = grid_for(n, 256);
  const uint64_t msm_bytes = msm_workspace_bytes(false, p.nbases, p.c);
  if (!msm_bytes) return p;
  uint64_t o = 0;
  p.bases = o, o += align256(p.nbases * point_record(false));
  p.scalars = o, o += align256(p.nbases * 32);
  p.sums = o, o += align256(2 * p.blocks * 32);
  p.pairs_g1 = o, o += align256(2 * point_record(false));
  p.pairs_g2 = o, o += align256(2 * point_record(true));
  p.key2 = o, o += 256;
  p.msm = o, o += msm_bytes;
  p.pairing = o, o += pairing_workspace_bytes(2);
  p.bytes = o;
  p.ok = true;
  return p;
}
inline uint64_t check_workspace_bytes(uint64_t n, uint32_t flags) { return check_plan(n, flags).bytes; }

// ---------------------------------------------------------------- Fr NTT
// A transform of m = 2^exp elements in passes (ntt_kernels.hip): a block of 256 lanes holds
// 2^tl = 2^min(t, exp) elements in LDS and runs the stages [q0, q0 + c) of the decimation-in-time
// schedule on them (stage q: half-block 2^q over the bit-reversed input), greedily c = min(t, what
// is left). A block's slot s = (k << lb) | l has k < 2^c along the pass's stages at element
// stride 2^q0 and l < 2^lb (lb = tl - c) consecutive elements; the other index bits are the
// block's (ntt_parts.hpp states the arithmetic). Pass 0 has lb = 0 and reads the caller's input
// bit-reversed; the other passes read and write the same elements.
//
// Workspace: two twiddle tables, lo[j] = w^j for j < 2^lo_bits and hi[j] = w^(j << lo_bits) for
// j < 2^hi_bits, lo_bits + hi_bits = exp - 1 split evenly (w^e = lo hi, one extra multiply; 384 KB
// at exp 26), and the staging array of m elements that pass 0 writes when the caller's output is
// its input and there is more than one pass (otherwise pass 0 writes the output itself).
// kNttTile: the tile that measured fastest at 2^22 (profiles/open_domain_timing.json)
constexpr uint32_t kNttMaxExp = 26, kNttTileMin = 8, kNttTileMax = 11, kNttTile = 9;
constexpr uint32_t kNttMaxPasses = 4;  // ceil(26 / 8)
constexpr uint32_t kNttFlags = KZGPOT_NTT_INVERSE | KZGPOT_POLY_TILE(0xf);
static_assert(kNttMaxPasses * kNttTileMin >= kNttMaxExp, "pass[] holds every pass of the largest transform");
static_assert((32u << kNttTileMax) <= 65536, "the largest tile is the 64 KB of LDS the kernel declares");
// the NTT's flags -> its tile (the library's for 0); false: an unknown bit or an unsupported tile
inline bool ntt_flags(uint32_t flags, uint32_t& t) {
  t = (flags >> 16) & 0xfu;
  if (!t) t = kNttTile;
  return t >= kNttTileMin && t <= kNttTileMax && !(flags & ~kNttFlags);
}
struct NttPass {
  uint32_t q0, c, lb;  // first stage, stages, log2 of the run of consecutive elements
  uint64_t stride;     // 2^q0: the element stride along the pass's stages
  uint64_t blocks;     // m >> tl
};
struct NttPlan {
  uint32_t exp, t, tl, npass;
  NttPass pass[kNttMaxPasses];
  uint32_t lo_bits, hi_bits;
  uint64_t tw_lo, tw_hi, tw_bytes;  // byte offsets of the tables; what both take (the staging array's offset)
  uint64_t stage_bytes, bytes;      // bytes = tw_bytes + stage_bytes; 0: invalid arguments
};
inline NttPlan ntt_plan(uint32_t exp, uint32_t t) {
  NttPlan p = {};
  if (exp > kNttMaxExp || t < kNttTileMin || t > kNttTileMax) return p;
  p.exp = exp, p.t = t, p.tl = exp < t ? exp : t;
  for (uint32_t q0 = 0; q0 < exp || !p.npass;) {
    const uint32_t c = exp - q0 < t ? exp - q0 : t;
    p.pass[p.npass++] = NttPass{q0, c, p.tl - c, (uint64_t)1 << q0, ((uint64_t)1 << exp) >> p.tl};
    q0 += c;
    if (!c) break;  // exp = 0: one pass without a stage
  }
  const uint32_t e = exp ? exp - 1 : 0;  // twiddle exponents are below m / 2
  p.lo_bits = (e + 1) / 2, p.hi_bits = e / 2;
  p.tw_lo = 0;
  p.tw_hi = align256((uint64_t)32 << p.lo_bits);
  p.tw_bytes = p.tw_hi + align256((uint64_t)32 << p.hi_bits);
  p.stage_bytes = p.npass > 1 ? (uint64_t)32 << exp : 0;
  p.bytes = p.tw_bytes + p.stage_bytes;
  return p;
}
inline uint64_t ntt_workspace_bytes(uint32_t exp, uint32_t t) { return ntt_plan(exp, t).bytes; }

// ---------------------------------------------------------------- amortized KZG10 opening (FK20)
// All n = 2^exp proofs of one polynomial from the table T of 2n points. Workspace:
// the NTT's input (2n elements: the shifted coefficients, later the coefficients themselves), its
// output (the 2n scalars of the per-point pass), its twiddle tables (sized for the size-2n transform; the
// size-n transform builds its own there afterwards; no staging array: neither runs in place), the work
// rows of the 2n-point and the n-point group transform, and their twiddle tables.
constexpr uint32_t kOpenDomainMaxExp = 24;
enum class DomainStep : uint32_t {
  ScalarsNtt,  // b -> v / 2n
  Load,        // k_fft_load of T into rows_a
  PointMul,    // rows_a[t] *= scalars[bitrev(t)]
  StagesWide,  // the 2n-point inverse stages, no scale pass
  Gather,      // rows_a[n - 1 + k] -> rows_b[bitrev_n(k)]
  StagesOut,   // the n-point forward stages
  Emit,        // rows_b -> proofs
  ValuesNtt,   // c -> values (skipped where the caller wants none)
};
constexpr uint32_t kDomainSteps = 8;
struct OpenDomainPlan {
  uint32_t exp, t;
  uint64_t n, rec;
  uint64_t ntt_in, scalars, ntt_tw, rows_a, rows_b, tw_a, tw_b, bytes;  // byte offsets
  uint64_t gather_src, gather_dst, gather_cnt;  // rows [src, src + cnt) of rows_a -> rows [dst, dst + cnt) of rows_b
  DomainStep step[kDomainSteps];
  bool ok;
};
inline OpenDomainPlan open_domain_plan(bool g2, uint32_t exp, uint32_t t) {
  OpenDomainPlan p = {};
  const NttPlan ntt = ntt_plan(exp + 1, t);
  if (exp > kOpenDomainMaxExp || !ntt.bytes) return p;
  p.exp = exp, p.t = t;
  p.n = (uint64_t)1 << exp;
  p.rec = point_record(g2);
  uint64_t o = 0;
  p.ntt_in = o, o += align256(2 * p.n * 32);
  p.scalars = o, o += align256(2 * p.n * 32);
  p.ntt_tw = o, o += ntt.tw_bytes;
  p.rows_a = o, o += align256(2 * p.n * work_rows(g2) * 4);
  p.rows_b = o, o += align256(p.n * work_rows(g2) * 4);
  p.tw_a = o, o += fft_twiddle_bytes(exp + 1);
  p.tw_b = o, o += fft_twiddle_bytes(exp);
  p.bytes = o;
  p.gather_src = p.n - 1, p.gather_dst = 0, p.gather_cnt = p.n;
  const DomainStep steps[kDomainSteps] = {DomainStep::ScalarsNtt, DomainStep::Load,      DomainStep::PointMul,
                                          DomainStep::StagesWide, DomainStep::Gather,    DomainStep::StagesOut,
                                          DomainStep::Emit,       DomainStep::ValuesNtt};
  for (uint32_t k = 0; k < kDomainSteps; k++) p.step[k] = steps[k];
  p.ok = true;
  return p;
}
// the opening's flags: KZGPOT_POLY_TILE alone, handed to the NTT
inline bool open_domain_flags(uint32_t flags, uint32_t& t) {
  return ntt_flags(flags, t) && !(flags & KZGPOT_NTT_INVERSE);
}
inline uint64_t open_domain_workspace_bytes(bool g2, uint32_t exp, uint32_t flags) {
  uint32_t t;
  return open_domain_flags(flags, t) ? open_domain_plan(g2, exp, t).bytes : 0;
}
// the table: the work rows and twiddles of one forward transform of 2n points
inline uint64_t open_domain_table_workspace_bytes(bool g2, uint32_t exp) {
  return exp > kOpenDomainMaxExp ? 0 : fft_workspace_bytes(g2, exp + 1);
}

}  // namespace kzgpot

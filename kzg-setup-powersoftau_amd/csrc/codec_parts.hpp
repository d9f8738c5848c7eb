// The decoding rules and LDS plumbing that the G1 and G2 codec kernels (g1_kernels.hip,
// codec_kernels.hip) share, each stated ONCE: a correction to one of DESIGN.md §2's rules is made
// in the function that names it here and reaches every kernel. All force-inlined; phases, layout
// and status codes are described at the top of codec_kernels.hip.
#pragma once
#include "codec.hpp"
#include "curve.hpp"
#include "records.hpp"

namespace kzgpot {

// ---------------------------------------------------------------- pairing compressed header
struct wire_head_t {
  int st;         // 0, or 1 / 2 / 7 / 3 in the order the reference decides them
  bool is_inf;    // accepted infinity encoding (unchecked streams only)
  bool greatest;  // bit 5: the sign rule's choice
};

// R1, R5: the flag byte is the top byte of the encoding's first word `top`; `rest` is the OR of
// every other word. Bit 7 must be set (1); bit 6 = infinity, well-formed only if the encoding is
// all zero once its top two bits are cleared (so bit 5 counts; else 2) — accepted on an unchecked
// stream, rejected (7) on a checked one, where read_g1 would see x >= p (R7); bit 5 = greatest.
// x is the encoding with its three flag bits cleared (wire_clear_flags, applied to `top`).
KZG_DEV void wire_clear_flags(uint32_t& top) { top &= 0x1fffffffu; }
KZG_DEV wire_head_t wire_head(uint32_t& top, uint32_t rest, bool reject_inf) {
  const uint32_t b0 = top >> 24;  // first byte on the wire
  const bool inf_clean = ((top & 0x3fffffffu) | rest) == 0;  // copy[0] &= 0x3f; all zero?
  wire_clear_flags(top);
  wire_head_t h;
  h.st = 0;
  if (!(b0 & 0x80u)) h.st = 1;
  else if (b0 & 0x40u) h.st = inf_clean ? (reject_inf ? 7 : 0) : 2;
  h.is_inf = (b0 & 0xc0u) == 0xc0u && h.st == 0;
  h.greatest = (b0 & 0x20u) != 0;
  return h;
}
// R2: x < p, decided after the flags (an accepted infinity has x = 0). In: x's words as on the
// wire; out: the canonical x.
KZG_DEV wire_head_t g1_head(words& w, bool reject_inf) {
  uint32_t rest = 0;
#pragma unroll
  for (int k = 0; k < 11; k++) rest |= w[k];
  wire_head_t h = wire_head(w[11], rest, reject_inf);
  if (h.st == 0 && words_geq_p(w)) h.st = 3;
  return h;
}
// G2: wire order x.c1 ‖ x.c0, the flags on x.c1
KZG_DEV wire_head_t g2_head(words& w1, words& w0, bool reject_inf) {
  uint32_t rest = w0[11];
#pragma unroll
  for (int k = 0; k < 11; k++) rest |= w1[k] | w0[k];
  wire_head_t h = wire_head(w1[11], rest, reject_inf);
  if (h.st == 0 && (words_geq_p(w0) || words_geq_p(w1))) h.st = 3;
  return h;
}

// ---------------------------------------------------------------- sign rule
// R4 (pairing get_point_from_x): keep y if (y < -y) XOR greatest, else -y, comparing canonical
// integers. In: a root y in Montgomery form; out: yc = the chosen root, canonical. Returns keep.
KZG_DEV bool sign_rule(fp& yc, const fp& y, bool greatest) {
  fp nyc;
  fp_from_mont(yc, y);
  fp_neg_canon(nyc, yc);
  const bool keep = fp_lt_canon(yc, nyc) ^ greatest;
  fp_select(yc, keep, yc, nyc);
  return keep;
}
// pairing Ord for Fq2: lexicographic, c1 first
KZG_DEV bool sign_rule(fp2& yc, const fp2& y, bool greatest) {
  fp2 nyc;
  fp_from_mont(yc.c0, y.c0);
  fp_from_mont(yc.c1, y.c1);
  fp_neg_canon(nyc.c0, yc.c0);
  fp_neg_canon(nyc.c1, yc.c1);
  bool c1eq = true;
#pragma unroll
  for (int k = 0; k < NL; k++) c1eq = c1eq && (yc.c1.v[k] == nyc.c1.v[k]);
  const bool keep = (c1eq ? fp_lt_canon(yc.c0, nyc.c0) : fp_lt_canon(yc.c1, nyc.c1)) ^ greatest;
  fp_select(yc.c0, keep, yc.c0, nyc.c0);
  fp_select(yc.c1, keep, yc.c1, nyc.c1);
  return keep;
}
// The chosen root in Montgomery form (for the fused kernels' ladders): y's representative made
// canonical, or p - y (0 -> 0), instead of converting the canonical bytes back (a multiply).
KZG_DEV void chosen_root_mont(fp& y, bool keep) {
  fp m;
  fp_reduce_once(y, y);
  fp_neg_canon(m, y);
  fp_select(y, keep, y, m);
}

// ---------------------------------------------------------------- LDS rows
// A lane's values live limb-major in a __shared__ uint32_t [rows][kBlock] array (the 64 lanes of a
// wave hit 64 consecutive dwords): value v occupies rows r .. r + N - 1 at column threadIdx.x.
using lds_rows = uint32_t (*)[kBlock];

template <int N>
KZG_DEV void lds_park(lds_rows rows, const uint32_t (&v)[N]) {
#pragma unroll
  for (int k = 0; k < N; k++) rows[k][threadIdx.x] = v[k];
}
// Loads go through an opaque lane index, so they are re-issued at every use and never hoisted:
// a parked value costs no VGPRs between its uses.
KZG_DEV uint32_t lds_lane() {
  uint32_t lane = threadIdx.x;
  asm volatile("" : "+v"(lane));
  return lane;
}
template <int N>
KZG_DEV void lds_load(uint32_t (&v)[N], const uint32_t (*rows)[kBlock], uint32_t lane) {
#pragma unroll
  for (int k = 0; k < N; k++) v[k] = rows[k][lane];
}

// ---------------------------------------------------------------- subgroup tests on a parked point
// G1: the ladders run on the 13 x 30 core (curve.hpp), so the point is parked in R30 = 2^390 form
// with w = 2y: x in rows 0.., w in rows N30.. of base; the fast test parks its second ladder's base
// Q1 = [|u|]P = (X : W : Z) in qpark (3 N30 rows): 65 rows per lane in all.
constexpr int kG1BaseRows = 2 * N30, kG1ParkRows = 3 * N30;
static_assert(kG1ParkRows >= 2 * NL, "the reference-ladder path parks the 14-limb point in qpark");

KZG_DEV void lds_park30(lds_rows rows, const f30& v) {
#pragma unroll
  for (int k = 0; k < N30; k++) rows[k][threadIdx.x] = (uint32_t)v.v[k];
}
KZG_DEV void lds_load30(f30& v, const uint32_t (*rows)[kBlock], uint32_t lane) {
#pragma unroll
  for (int k = 0; k < N30; k++) v.v[k] = (int32_t)rows[k][lane];
}
// In: the point in R = 2^392 Montgomery form, x normalized with value < 2 p, y canonical or < 2 p
KZG_DEV void g1_park_base(lds_rows base, const fp& x, const fp& y) {
  f30 t;
  f30_from_mont<2>(t, x);
  lds_park30(base, t);
  f30_from_mont<1>(t, y);  // w = 2y
  lds_park30(base + N30, t);
}
KZG_DEV void g1_load_base(f30& bx, f30& bw, const uint32_t (*base)[kBlock]) {
  const uint32_t lane = lds_lane();
  lds_load30(bx, base, lane);
  lds_load30(bw, base + N30, lane);
}
// ref: the reference's double-and-add by r (KZGPOT_SUBGROUP_REF, and every point off the curve),
// which stays on 14 x 28 limbs: the point goes back to R = 2^392 form once, parked in qpark
KZG_DEV bool g1_in_subgroup(const uint32_t (*base)[kBlock], lds_rows qpark, bool ref) {
  if (ref) {
    {
      f30 x30, w30;
      g1_load_base(x30, w30, base);
      fp t;
      fp_mont_from_f30<2>(t, x30);
      lds_park(qpark, t.v);
      fp_mont_from_f30<1>(t, w30);
      lds_park(qpark + NL, t.v);
    }
    return in_subgroup_ref<fp>([&](fp& bx, fp& by) {
      const uint32_t lane = lds_lane();
      lds_load(bx.v, qpark, lane);
      lds_load(by.v, qpark + NL, lane);
    });
  }
  auto park = [&](const jac<f30>& q) {
    lds_park30(qpark, q.x);
    lds_park30(qpark + N30, q.y);
    lds_park30(qpark + 2 * N30, q.z);
  };
  auto load_row = [&](int src, f30& bx, f30& bw) {  // src 0: P (base), 1: Q1 (qpark); wave-uniform
    g1_load_base(bx, bw, src ? qpark : base);
  };
  auto load_qz = [&](f30& qz) { lds_load30(qz, qpark + 2 * N30, lds_lane()); };
  return in_subgroup_fast_g1(load_row, park, load_qz);
}

// G2: base holds x.c0, x.c1, y.c0, y.c1 (Montgomery) in rows 0, NL, 2 NL, 3 NL
KZG_DEV void g2_load_base(fp2& bx, fp2& by, const uint32_t (*base)[kBlock]) {
  const uint32_t lane = lds_lane();
  lds_load(bx.c0.v, base, lane);
  lds_load(bx.c1.v, base + NL, lane);
  lds_load(by.c0.v, base + 2 * NL, lane);
  lds_load(by.c1.v, base + 3 * NL, lane);
}
KZG_DEV bool g2_in_subgroup(const uint32_t (*base)[kBlock], bool ref) {
  auto load = [&](fp2& bx, fp2& by) { g2_load_base(bx, by, base); };
  return ref ? in_subgroup_ref<fp2>(load) : in_subgroup_fast_g2(load);
}

// ---------------------------------------------------------------- ark records
constexpr uint32_t kArkInfinity = 0x40000000u;  // SWFlags::infinity(): bit 6 of the record's last byte

// R8: ark SWFlags live in the top byte of y (G2: of y.c1), the coordinate read last: bit 7
// PositiveY, bit 6 Infinity. Clears them from `ytop`; returns the infinity flag; `both` (both set)
// is UnexpectedFlags, status 6, which the caller ranks in ark's read order.
KZG_DEV bool ark_sw_flags(uint32_t& ytop, bool& both) {
  const uint32_t yb = ytop >> 24;
  const bool fpos = yb & 0x80u, finf = yb & 0x40u;
  ytop &= 0x3fffffffu;
  both = fpos && finf;
  return finf;
}
// R10: the last coordinate of an ark record carries the infinity flag and no other
// (GroupAffine::new(x, y, true) keeps x, y)
KZG_DEV void store_ark_last(uint4* dst, const words& y, bool finf) {
  words e;
#pragma unroll
  for (int k = 0; k < 12; k++) e[k] = y[k];
  if (finf) e[11] |= kArkInfinity;
  store_words(dst, e);
}
// R10, phase 1's record where no point is emitted: ark GroupAffine::zero() = (0, 1, inf) for an
// accepted infinity, zeros otherwise; `poison` marks a rejected point of a checked stream (phase 2
// zero-fills and skips it). NC coordinates per field element: G1 1, G2 2 (c0 first).
template <int NC>
KZG_DEV void emit_no_point(uint4* dst, bool is_inf, bool poison) {
#pragma unroll
  for (int c = 0; c < 2 * NC; c++) {
    words z;
    zero_words(z);
    if (c == 0 && poison) z[11] = kPoison;
    if (c == NC && is_inf) z[0] = 1;
    if (c == 2 * NC - 1 && is_inf) z[11] = kArkInfinity;
    store_words(dst + 3 * c, z);
  }
}

}  // namespace kzgpot

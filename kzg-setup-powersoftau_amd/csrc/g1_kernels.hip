// The G1 half of the hot path (the headline: 2^27 of the 2^27 + 2^16 points), in its own translation
// unit so that it can be compiled with its own scheduler (Makefile: -amdgpu-sched-strategy=
// iterative-ilp, -0.7 % time per G1 point on the same box; the G2 kernels measured +0.9 % with it,
// so codec_kernels.hip keeps the default). Kernels, phases, layout and status codes are described
// at the top of codec_kernels.hip; the rules the kernels share are stated in codec_parts.hpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec_parts.hpp"

namespace kzgpot {

// x^3 + 4, normalized
KZG_DEV void g1_rhs(fp& r, const fp& x) {
  fp four;
  fp_sqr(r, x);
  fp_mul(r, r, x);
  fp_set(four, FP_FOUR);
  fp_add(r, r, four);
}

// ================================================================================ phase 1: G1
__global__ void __launch_bounds__(kBlock) k_g1_decompress(const uint4* __restrict__ in, uint4* __restrict__ out,
                                                          uint64_t n, uint32_t flags,
                                                          unsigned long long* __restrict__ first_bad,
                                                          uint8_t* __restrict__ status) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const bool checked = !(flags & KZGPOT_NO_SUBGROUP_CHECK);
  wire_head_t h;
  fp a;
  {
    words w;
    load_be(w, in + i * 3);
    h = g1_head(w, checked);
    fp t;
    words_to_mont(t, w);  // x < 2^381 even when rejected: bounds hold (test_field_bounds.py)
    g1_rhs(a, t);
  }
  int st = h.st;
  // y = (x^3 + 4)^((p+1)/4); every lane runs the same chain (wave-uniform)
  fp y, t;
  fp_pow_pm3d4(t, a);
  fp_mul(y, t, a);
  fp_sqr(t, y);
  if (st == 0 && !h.is_inf && !fp_eq(t, a)) st = 4;
  fp yc;
  sign_rule(yc, y, h.greatest);

  uint4* dst = out + i * 6;
  if (st == 0 && !h.is_inf) {
    words w;  // re-read x rather than keep it live through the exponentiation
    load_be(w, opaque(in) + i * 3);
    wire_clear_flags(w[11]);
    store_words(dst, w);
    store_canon(dst + 3, yc);
  } else {
    emit_no_point<1>(dst, h.is_inf, st && checked);
  }
  report(i, st, first_bad, status);
}

// ================================================================================ fused G1 codec
// Both phases of a checked G1 point in one lane and one launch (the default for checked
// streams): x's canonical words and its Montgomery form are parked in LDS before the square root,
// the ark record (x, y) goes out after the sign rule and y's Montgomery form is parked next to x —
// so nothing but the ladder state is live across the subgroup test,
// and no record is read back from HBM (48 B in + 96 B out per point, against 48 + 96 + 96 + the
// x re-read of the split kernels). A rejected point's record is zero-filled (the split path's
// phase 2 does the same to its poison record). 65 KB of LDS per block (base point + the second
// ladder's base, as k_g1_check) holds the kernel at 2 waves per SIMD. x's Montgomery form waits in
// qpark's upper rows until the chosen root is known; the pair is then parked in the ladders' form.
__global__ void __launch_bounds__(kBlock) k_g1_codec(const uint4* __restrict__ in, uint4* __restrict__ out,
                                                     uint64_t n, uint32_t flags,
                                                     unsigned long long* __restrict__ first_bad,
                                                     uint8_t* __restrict__ status) {
  __shared__ uint32_t base[kG1BaseRows][kBlock];
  __shared__ uint32_t qpark[kG1ParkRows][kBlock];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  wire_head_t h;
  uint4* dst = out + i * 6;
  fp a;
  {
    words w;
    load_be(w, in + i * 3);
    h = g1_head(w, true);  // checked stream: infinity is rejected
    lds_park(qpark, w);    // ark x = the canonical x (qpark is free until the ladder)
    fp t;
    words_to_mont(t, w);
    lds_park(qpark + 12, t.v);
    g1_rhs(a, t);
  }
  int st = h.st;
  {
    fp y, t;
    fp_pow_pm3d4(t, a);
    fp_mul(y, t, a);
    fp_sqr(t, y);
    if (st == 0 && !fp_eq(t, a)) st = 4;
    fp yc;
    const bool keep = sign_rule(yc, y, h.greatest);
    if (st == 0) {
      words w;  // the whole 96-B record in one go: a 48-B half written long before the other costs
      lds_load(w, qpark, lds_lane());  // a partial 64-B write per half (PMC: 155 instead of 96 B/point)
      store_words(dst, w);
      store_canon(dst + 3, yc);
      chosen_root_mont(y, keep);
      fp x;
      lds_load(x.v, qpark + 12, lds_lane());
      g1_park_base(base, x, y);
    }
  }
  if (st == 0 && !g1_in_subgroup(base, qpark, flags & KZGPOT_SUBGROUP_REF)) st = 5;
  if (st) store_zero(dst, 6);
  report(i, st, first_bad, status);
}

template <Src S>
struct G1Rec {
  static KZG_DEV void load_xy(words& x, words& y, const uint4* rec) {
    if constexpr (S == Src::ArkInPlace) {
      load_le(x, rec);
      load_le(y, rec + 3);
    } else {
      load_be(x, rec);
      load_be(y, rec + 3);
    }
  }
};

template <Src S>
__global__ void __launch_bounds__(kBlock) k_g1_check(const uint4* __restrict__ in, uint4* __restrict__ out,
                                                     uint64_t n, uint32_t flags,
                                                     unsigned long long* __restrict__ first_bad,
                                                     uint8_t* __restrict__ status) {
  // The base point in the ladders' form (g1_park_base) is parked in LDS (digit-major, so the 64
  // lanes of a wave hit 64 consecutive dwords): each of the ~8 reloads in the ladders is 26 LDS
  // reads instead of two Montgomery conversions, and the point costs no VGPRs between reloads. The
  // fast test's second ladder base Q1 = [|u|]P = (X : W : Z) is parked beside it (qpark). 65 KB per
  // 256-lane block: 2 blocks per CU, the occupancy the VGPR count allows anyway.
  __shared__ uint32_t base[kG1BaseRows][kBlock];
  __shared__ uint32_t qpark[kG1ParkRows][kBlock];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint4* rec = (src_in_place(S) ? (const uint4*)out : in) + i * 6;
  uint4* dst = out + i * 6;
  int st = 0;
  bool finf, on_curve = true;
  {
    // The record is read ONCE: a transcode record that passes the flag and field checks is
    // emitted right away (as k_g1_codec emits before its subgroup test) and zero-filled if the
    // test rejects it, so nothing is re-read from HBM after the ladders (192 B/point moved).
    words x, y;
    G1Rec<S>::load_xy(x, y, rec);
    if (S == Src::ArkInPlace && x[11] == kPoison) {  // phase 1 already rejected (and reported) it
      store_zero(dst, 6);
      return;
    }
    bool both;
    finf = ark_sw_flags(y[11], both);
    if (words_geq_p(x)) st = 3;
    else if (both) st = 6;
    else if (words_geq_p(y)) st = 3;
    if (S != Src::ArkInPlace && st == 0) {
      store_words(dst, x);
      store_ark_last(dst + 3, y, finf);
    }
    if (st == 0 && !finf) {
      fp bx, by;
      words_to_mont(bx, x);
      words_to_mont(by, y);
      g1_park_base(base, bx, by);
      // Phase 1 emits only points with y^2 = x^3 + 4 (it rejects non-residues), so an in-place
      // record is on the curve; a transcode input may not be (the reference never checks).
      if (S != Src::ArkInPlace) {
        fp l, r;
        fp_sqr(l, by);
        g1_rhs(r, bx);
        on_curve = fp_eq(l, r);
      }
    }
  }

  if (st == 0 && !finf && !g1_in_subgroup(base, qpark, (flags & KZGPOT_SUBGROUP_REF) || !on_curve)) st = 5;
  if (st) store_zero(dst, 6);
  report(i, st, first_bad, status);
}

// ================================================================================ launcher
hipError_t launch_g1(CodecOp op, const uint4* in, uint4* out, uint64_t n, uint32_t flags,
                     unsigned long long* d_first_bad, uint8_t* d_status, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const dim3 grid(grid_for(n, kBlock)), block(kBlock);
  const bool checked = !(flags & KZGPOT_NO_SUBGROUP_CHECK);
  switch (op) {
    case CodecOp::G1Decompress:
      if (checked && !(flags & KZGPOT_SPLIT_PHASES)) {
        hipLaunchKernelGGL(k_g1_codec, grid, block, 0, stream, in, out, n, flags, d_first_bad, d_status);
        break;
      }
      hipLaunchKernelGGL(k_g1_decompress, grid, block, 0, stream, in, out, n, flags, d_first_bad, d_status);
      if (checked)
        hipLaunchKernelGGL(k_g1_check<Src::ArkInPlace>, grid, block, 0, stream, in, out, n, flags, d_first_bad,
                           d_status);
      break;
    case CodecOp::G1Transcode:
      hipLaunchKernelGGL(k_g1_check<Src::PairingBE>, grid, block, 0, stream, in, out, n, flags, d_first_bad,
                         d_status);
      break;
    case CodecOp::G1Phase1:
      hipLaunchKernelGGL(k_g1_check<Src::PairingBEInPlace>, grid, block, 0, stream, nullptr, out, n, flags,
                         d_first_bad, d_status);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace kzgpot

// Internal C++ interface between the C ABI (capi.hip, preprocess.hip, phase2.hip, msm.hip) and the kernels
// (codec_kernels.hip, g1_kernels.hip; the device functions those two share are in codec_parts.hpp, those of
// fft_kernels.hip and msm_kernels.hip in group_parts.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kzgpot.h"
#include "fr.hpp"

namespace kzgpot {

constexpr int kBlock = 256;  // 4 waves; one point per lane
inline unsigned grid_for(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }  // blocks for n points
constexpr uint64_t align256(uint64_t x) { return (x + 255) & ~(uint64_t)255; }  // every workspace region's size

// G1Phase1 / G2Phase1: read_g1 / read_g2 straight into the in-memory GroupAffine (load_phase1) —
// the transcode kernel in place on the input staging buffer, then the loader kernel. Host-buffer
// API only (run_host owns the staging it overwrites).
enum class CodecOp {
  G1Decompress, G2Decompress, G1Transcode, G2Transcode, G1Load, G2Load, Bn254G1Decompress, G1Phase1, G2Phase1
};

// record sizes on the wire
constexpr uint64_t in_record(CodecOp op) {
  switch (op) {
    case CodecOp::G1Decompress: return 48;
    case CodecOp::G2Decompress: return 96;
    case CodecOp::G1Transcode: return 96;
    case CodecOp::G2Transcode: return 192;
    case CodecOp::G1Load: return 96;
    case CodecOp::G2Load: return 192;
    case CodecOp::Bn254G1Decompress: return 32;
    case CodecOp::G1Phase1: return 96;
    case CodecOp::G2Phase1: return 192;
  }
  return 0;
}
constexpr uint64_t out_record(CodecOp op) {
  switch (op) {
    case CodecOp::G1Decompress: return 96;
    case CodecOp::G2Decompress: return 192;
    case CodecOp::G1Transcode: return 96;
    case CodecOp::G2Transcode: return 192;
    case CodecOp::G1Load: return KZGPOT_G1_ARK_MONT_BYTES;
    case CodecOp::G2Load: return KZGPOT_G2_ARK_MONT_BYTES;
    case CodecOp::Bn254G1Decompress: return 64;
    case CodecOp::G1Phase1: return KZGPOT_G1_ARK_MONT_BYTES;
    case CodecOp::G2Phase1: return KZGPOT_G2_ARK_MONT_BYTES;
  }
  return 0;
}

// phase 1 marks a rejected point's record with this value in x's top word (phase 2 then skips it)
constexpr uint32_t kPoison = 0xffffffffu;

// where phase 2 (k_g1_check / k_g2_check) reads its record (codec_kernels.hip "phase 2")
enum class Src { ArkInPlace, PairingBE, PairingBEInPlace };
constexpr bool src_in_place(Src s) { return s != Src::PairingBE; }

// G1 kernels (g1_kernels.hip, its own translation unit: compiled with the iterative ILP scheduler):
// G1Decompress (fused or split), G1Transcode, and G1Phase1's in-place transcode (in = nullptr)
hipError_t launch_g1(CodecOp op, const uint4* in, uint4* out, uint64_t n, uint32_t flags,
                     unsigned long long* d_first_bad, uint8_t* d_status, hipStream_t stream);

// loader kernels (load_kernels.hip)
hipError_t launch_load(bool g2, const void* d_in, void* d_out, uint64_t n, unsigned long long* d_first_bad,
                       uint8_t* d_status, hipStream_t stream);

// BN254 G1 codec (bn254_kernels.hip)
hipError_t launch_bn254(const void* d_in, void* d_out, uint64_t n, unsigned long long* d_first_bad,
                        uint8_t* d_status, hipStream_t stream);

hipError_t launch_codec(CodecOp op, const void* d_in, void* d_out, uint64_t n, uint32_t flags,
                        unsigned long long* d_first_bad, uint8_t* d_status, hipStream_t stream);

// group FFT (fft_kernels.hip). The scalars of one transform, computed on the host (phase2.hip) with
// csrc/fr.hpp and passed to k_fft_twiddles as they are. d_work: fft_workspace_bytes = the twiddle
// table (fft_twiddle_bytes), then the work buffer.
struct FftScalars {
  fr pw[31];  // w^(+-2^k) in Montgomery form, k < exp - 1 (the rest unused)
  fr one;     // Montgomery 1
  fr minv;    // 1/m, canonical
};
uint64_t fft_twiddle_bytes(uint32_t exp);
uint64_t fft_workspace_bytes(bool g2, uint32_t exp);
hipError_t launch_group_fft(bool g2, const void* d_in, uint32_t exp, void* d_out, bool inverse, bool pairing,
                            const FftScalars& sc, void* d_work, unsigned long long* d_key, hipStream_t stream);
// h[i] = tau_g1[m + i] - tau_g1[i], i < m - 1: ark G1 records in, pairing BE records out
hipError_t launch_h_bases(const void* d_tau_g1, uint64_t m, void* d_out, hipStream_t stream);

// multi-scalar multiplication (msm_kernels.hip): out = sum_i [s_i] P_i, one ark record. c: window
// width 1..16; msm_workspace_bytes is 0 where (n, c) is not supported, and takes c = 0 for "the
// library's choice, msm_window_bits(n)" (a size monotone in n; launch_msm wants the width itself).
// Bases are ark records or (mont) in-memory GroupAffine records; scalars 8 LE words each.
constexpr uint32_t kMsmChunk = 64;            // L: no lane sums more entries than this
constexpr uint64_t kMsmMaxN = 1ull << 26;
constexpr uint32_t kMsmWindowMax = 16;
// KZGPOT_MSM_WINDOW(c) in the flags: c = 0 (the library chooses) or the width; false: above kMsmWindowMax
inline bool msm_window_flag(uint32_t flags, uint32_t& c) {
  c = (flags >> 8) & 0x1fu;
  return c <= kMsmWindowMax;
}
uint32_t msm_window_bits(uint64_t n);
uint64_t msm_workspace_bytes(bool g2, uint64_t n, uint32_t c);
hipError_t launch_msm(bool g2, const void* d_bases, const void* d_scalars, uint64_t n, void* d_out, bool mont,
                      uint32_t c, void* d_work, unsigned long long* d_key, hipStream_t stream);

// polynomial division by (x - z) over Fr (poly_kernels.hip): value = p(z), and unless d_quotient
// is null the n - 1 coefficients of (p(x) - p(z)) / (x - z). t: tile width 2^t, kPolyTileMin ..
// kPolyTileMax. z_pow.p[k] = z^(2^k), computed on the host (open.hip) with csrc/fr.hpp.
constexpr uint32_t kPolyTileMin = 8, kPolyTileMax = 12, kPolyTile = 11;
// KZGPOT_POLY_TILE(t) in the flags: t, or the library's for 0; false: outside kPolyTileMin .. kPolyTileMax
inline bool poly_tile_flag(uint32_t flags, uint32_t& t) {
  t = (flags >> 16) & 0xfu;
  if (!t) t = kPolyTile;
  return t >= kPolyTileMin && t <= kPolyTileMax;
}
constexpr uint64_t kPolyMaxN = (1ull << 26) + 1;
constexpr int kPolyPowers = 64;  // entries of z_pow: the top level (at most the fourth) reads up to index 3 x 12 + 11
uint64_t poly_workspace_bytes(uint64_t n, uint32_t t);
hipError_t launch_poly_divide(const void* d_coeffs, uint64_t n, const fr_powers<kPolyPowers>& z_pow, void* d_quotient,
                              void* d_value, uint32_t t, void* d_work, hipStream_t stream);
// KZG10::open's last step: the two evaluations (64 B at d_values) behind the proof's point, unless
// the MSM's load rejected a base
hipError_t launch_open_emit(const void* d_values, void* d_out64, const unsigned long long* d_key, hipStream_t stream);

}  // namespace kzgpot

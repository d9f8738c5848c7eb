// Internal C++ interface between the C ABI (capi.hip, preprocess.hip, phase2.hip, msm.hip) and the kernels
// (codec_kernels.hip, g1_kernels.hip; the device functions those two share are in codec_parts.hpp, those of
// fft_kernels.hip and msm_kernels.hip in group_parts.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kzgpot.h"
#include "fr.hpp"
#include "plans.hpp"

namespace kzgpot {

constexpr int kBlock = 256;  // 4 waves; one point per lane

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
// csrc/fr.hpp and passed to k_fft_twiddles as they are. d_work: fft_workspace_bytes, laid out by
// fft_plan (plans.hpp).
struct FftScalars {
  fr pw[31];  // w^(+-2^k) in Montgomery form, k < exp - 1 (the rest unused)
  fr one;     // Montgomery 1
  fr minv;    // 1/m, canonical
};
// The scalars of one transform of size m = 2^exp <= 2^32: the powers w^(+-2^k) (the inverse uses
// w^-1 = w^(m-1)) and 1/m
inline fr fft_root(uint32_t exp, bool inverse) {
  const uint64_t m = (uint64_t)1 << exp;
  const fr w = fr_domain_root(exp);
  return inverse ? fr_pow(w, fr{{(uint32_t)(m - 1), 0, 0, 0, 0, 0, 0, 0}}) : w;  // m - 1 < 2^32
}
inline void fft_scalars(uint32_t exp, bool inverse, FftScalars& sc) {
  fr_fill_powers(sc.pw, fft_root(exp, inverse));
  sc.one = fr_one();
  fr_store(sc.minv, fr_inv(fr_from_u64((uint64_t)1 << exp)));
}
hipError_t launch_group_fft(bool g2, const void* d_in, uint32_t exp, void* d_out, bool inverse, bool pairing,
                            const FftScalars& sc, void* d_work, unsigned long long* d_key, hipStream_t stream);
// h[i] = tau_g1[m + i] - tau_g1[i], i < m - 1: ark G1 records in, pairing BE records out
hipError_t launch_h_bases(const void* d_tau_g1, uint64_t m, void* d_out, hipStream_t stream);

// multi-scalar multiplication (msm_kernels.hip): out = sum_i [s_i] P_i, one ark record. c: window
// width 1..16 (launch_msm wants the width itself); d_work: msm_workspace_bytes, laid out by msm_plan
// (plans.hpp). Bases are ark records or (mont) in-memory GroupAffine records; scalars 8 LE words each.
hipError_t launch_msm(bool g2, const void* d_bases, const void* d_scalars, uint64_t n, void* d_out, bool mont,
                      uint32_t c, void* d_work, unsigned long long* d_key, hipStream_t stream);

// polynomial division by (x - z) over Fr (poly_kernels.hip): value = p(z), and unless d_quotient
// is null the n - 1 coefficients of (p(x) - p(z)) / (x - z). t: tile width 2^t, kPolyTileMin ..
// kPolyTileMax. z_pow.p[k] = z^(2^k), computed on the host (open.hip) with csrc/fr.hpp. d_work:
// poly_workspace_bytes, laid out by poly_plan (plans.hpp).
hipError_t launch_poly_divide(const void* d_coeffs, uint64_t n, const fr_powers<kPolyPowers>& z_pow, void* d_quotient,
                              void* d_value, uint32_t t, void* d_work, hipStream_t stream);
// An open's last step: `words` <= 64 words from d_values behind the proof's point, unless the MSM's
// load rejected a base. KZG10::open emits its two evaluations (16 words), the open from evaluations
// (evals.hip) its value (8 words).
hipError_t launch_fr_emit(const void* d_values, void* d_out, uint32_t words, const unsigned long long* d_key,
                          hipStream_t stream);

// evaluation form (eval_kernels.hip). out[i] = in[i]^-1 mod r, 0 for a zero; n <= kEvalMaxN entries
// of 32 B (any 256-bit integers in, canonical values out), out may be in; t as for the division.
hipError_t launch_fr_batch_inverse(const void* d_in, uint64_t n, void* d_out, uint32_t t, hipStream_t stream);
// Division by (x - z) from the 2^exp evaluations of eval_plan p: value = p(z) (32 B, canonical) and,
// unless d_quotient is null, the quotient's 2^exp evaluations (canonical; not over d_evals). sc:
// fr_eval_setup's scalars for (p.exp, z), computed on the host (evals.hip). d_work: p.bytes.
hipError_t launch_evals_divide(const EvalPlan& p, const void* d_evals, const fr_eval_scalars& sc, void* d_quotient,
                               void* d_value, void* d_work, hipStream_t stream);

// pairing product (pairing_kernels.hip): d_out (576 B of GT, then one u32: 1 if it is one) =
// prod_{i < k} e(g1[i], g2[i])^KZGPOT_PAIRING_GT_POWER over ark records; k <= kPairMaxK. A malformed
// record lowers d_key to (key_bias + its index along g1 then g2) << 8 | status, and nothing is written
// once d_key reports a rejection, this call's or an earlier one's. d_work: pairing_workspace_bytes, laid
// out by pairing_plan (plans.hpp).
hipError_t launch_pairing_product(const void* d_g1, const void* d_g2, uint64_t k, void* d_out, void* d_work,
                                  unsigned long long* d_key, uint64_t key_bias, hipStream_t stream);

// KZG10 check (verify_kernels.hip). The Fr pass: the scalar rows rho_i, rho_i z_i and the two negated
// sums into the plan's `scalars` (d_random_vs may be null); and the negation of one ark G1 record in place.
hipError_t launch_check_scalars(const CheckPlan& p, const void* d_randomizers, const void* d_points, const void* d_values,
                                const void* d_random_vs, void* d_work, hipStream_t stream);
hipError_t launch_g1_negate(void* d_record, hipStream_t stream);

// Fr NTT (ntt_kernels.hip). The scalars of one transform, computed on the host (domain.hip) with
// csrc/fr.hpp. d_tw: the plan's twiddle tables (tw_bytes); d_stage: the plan's staging array
// (stage_bytes), needed only where d_out is d_in and the plan has more than one pass. d_key
// (optional): the bad key of the call the transform is part of; once it reports a rejection the
// passes write nothing.
struct NttScalars {
  fr pw[26];  // w^(+-2^k) in Montgomery form
  fr one;     // Montgomery 1
  fr scale;   // the plain integer every output is multiplied by: 1, 1/m, or another canonical factor
};
hipError_t launch_fr_ntt(const NttPlan& p, const void* d_in, void* d_out, const NttScalars& sc, void* d_tw, void* d_stage,
                         const unsigned long long* d_key, hipStream_t stream);

// amortized openings, the group side (fft_kernels.hip). The table: powers reversed and padded with
// n points at infinity, forward transform of 2n points (sc: its scalars); d_work:
// open_domain_table_workspace_bytes. The proofs: steps Load .. Emit of open_domain_plan over the 2n
// scalars the NTT left at the plan's `scalars` (wide: the scalars of the inverse transform of 2n
// points, out: of the forward transform of n points).
hipError_t launch_open_domain_table(bool g2, const void* d_powers, uint32_t exp, void* d_table, const FftScalars& sc,
                                    void* d_work, unsigned long long* d_key, hipStream_t stream);
hipError_t launch_open_domain_step(bool g2, const OpenDomainPlan& p, DomainStep step, const void* d_table, void* d_proofs,
                                   const FftScalars& wide, const FftScalars& out, void* d_work, unsigned long long* d_key,
                                   hipStream_t stream);

}  // namespace kzgpot

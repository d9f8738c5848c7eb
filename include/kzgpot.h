/*
 * kzgpot — MI355X-native Powers-of-Tau → arkworks KZG preprocessor: the C ABI.
 *
 * Drop-in boundary for the per-point hot path of heliaxdev/kzg-setup-powersoftau. The reference
 * is a Rust crate with no FFI; each entry point below names the reference code it replaces
 * (paths relative to the reference repo root). A Rust crate binds these with `extern "C"` (see
 * INTEGRATION.md); the Python package and the tests bind them with ctypes.
 *
 * Conventions
 *  - Plain pointers and sizes only. Host variants take host buffers and are synchronous. `_dev`
 *    variants take device pointers (HBM) and a hipStream_t passed as void*; they are
 *    asynchronous and report errors through a device-side key (see kzgpot_decode_bad_key).
 *  - Point formats: G1 compressed 48 B / uncompressed 96 B, G2 compressed 96 B / uncompressed
 *    192 B. "pairing" = zcash pairing 0.14.2 big-endian encodings as written by powersoftau;
 *    "ark" = ark-serialize 0.2 `serialize_uncompressed` (little-endian, SWFlags in the top byte).
 *  - Return value: 0 = every point accepted; -(status) of the FIRST rejected point (smallest
 *    index, deterministic) when a point is rejected; <= KZGPOT_E_INVALID_ARG on API/runtime errors.
 *    Rejected points' output records are zero-filled. The reference panics on the first bad point
 *    (`unwrap`, preprocess-kgz.rs:110,142); callers that want that behaviour abort on != 0.
 *  - Accept/reject and output bytes are bit-exact with the reference for every input; the error
 *    CLASS is informative (the reference's own class depends on which stage trips first).
 */
#ifndef KZGPOT_H
#define KZGPOT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- per-point status / errors */
#define KZGPOT_OK 0
#define KZGPOT_ST_COMPRESSION_MODE 1 /* pairing GroupDecodingError::UnexpectedCompressionMode */
#define KZGPOT_ST_UNEXPECTED_INFO 2  /* pairing GroupDecodingError::UnexpectedInformation */
#define KZGPOT_ST_NOT_IN_FIELD 3     /* pairing CoordinateDecodingError / ark InvalidData (coord >= p) */
#define KZGPOT_ST_NOT_ON_CURVE 4     /* pairing GroupDecodingError::NotOnCurve (x^3+b non-residue) */
#define KZGPOT_ST_NOT_IN_SUBGROUP 5  /* ark InvalidData from is_in_correct_subgroup_assuming_on_curve */
#define KZGPOT_ST_UNEXPECTED_FLAGS 6 /* ark SerializationError::UnexpectedFlags */
#define KZGPOT_ST_INFINITY 7         /* point at infinity reaching read_g1/read_g2: the reference panics */

#define KZGPOT_E_INVALID_ARG (-100)
#define KZGPOT_E_DEVICE (-101)  /* HIP runtime failure or no usable GPU: the product path never falls back to CPU */
#define KZGPOT_E_IO (-102)
#define KZGPOT_E_SIZE (-103)    /* transcript size != powersoftau CONTRIBUTION_BYTE_SIZE (preprocess-kgz.rs:83-91) */
#define KZGPOT_E_DIGEST (-104)  /* BLAKE2b-512 mismatch (preprocess-kgz.rs:51-61, src/lib.rs:147-157) */
#define KZGPOT_E_NETWORK (-105) /* download requested: this build has no network client */
#define KZGPOT_E_RANK_FAILED (-106) /* multi-GPU: a rank (maybe this one) could not decode its share */
#define KZGPOT_E_TIMEOUT (-107)     /* multi-GPU: kzgpot_comm_wait gave up; the communicator is aborted */
/* Host resources ran out: host memory (std::bad_alloc), the file path's 0.6-1.6 GB buffer mappings,
 * or a host thread (EAGAIN under a process or thread limit). The call has joined every thread it
 * started and removed its temporary output file; nothing crossed the C ABI as an exception. The
 * reference returns a Result here (Accumulator::deserialize, preprocess-kgz.rs:105-110). */
#define KZGPOT_E_OUT_OF_MEMORY (-108)

/* ---------------------------------------------------------------- flags */
/* Decompression only (powersoftau CheckForCorrectness::No with no read_g1 afterwards — the βτG1 /
 * βG2 sections in preprocess-kgz). The point at infinity is then legal and is emitted as ark
 * GroupAffine::zero(). Default (flag clear): the full reference chain of a point that is read
 * back by read_g1/read_g2 — infinity rejected, subgroup checked. */
#define KZGPOT_NO_SUBGROUP_CHECK 0x1u
/* Use the reference's own subgroup algorithm (ark mul_bits by r, 255-bit double-and-add) instead
 * of the endomorphism test. Same boolean for every point; ~3x slower. For cross-validation. */
#define KZGPOT_SUBGROUP_REF 0x2u
/* Checked G1 / G2 decompression as two launches (decompress, then the arkworks check in place on
 * its output — the split kernels) instead of the fused one-pass kernel. Same output and statuses;
 * for A/B measurement. */
#define KZGPOT_SPLIT_PHASES 0x4u

/* ---------------------------------------------------------------- hot path, host buffers */
/* Compressed G1 (48 B each, pairing) → ark uncompressed (96 B each).
 * Replaces, per point: pairing G1Compressed::into_affine_unchecked (via powersoftau
 * Accumulator::deserialize, src/bin/preprocess-kgz.rs:105-110) → G1Uncompressed (preprocess-kgz.rs:122)
 * → read_g1 (src/lib.rs:41-54, incl. ark subgroup check) → serialize_uncompressed (preprocess-kgz.rs:188-194). */
int kzgpot_g1_decompress(const uint8_t* in, size_t n, uint8_t* out, uint32_t flags, int64_t* first_bad);
/* Compressed G2 (96 B) → ark uncompressed (192 B). Same chain with read_g2 (src/lib.rs:56-80) and the
 * fastkgz G2 emit (src/bin/preprocess-fastkgz.rs:206-208). */
int kzgpot_g2_decompress(const uint8_t* in, size_t n, uint8_t* out, uint32_t flags, int64_t* first_bad);
/* Pairing-uncompressed G1 (96 B) → ark (96 B): the read_g1 loop alone (src/lib.rs:41-54;
 * preprocess-kgz.rs:140-153; load_phase1 src/lib.rs:92-110). flags: KZGPOT_SUBGROUP_REF only. */
int kzgpot_g1_transcode_uncompressed(const uint8_t* in, size_t n, uint8_t* out, uint32_t flags, int64_t* first_bad);
/* Pairing-uncompressed G2 (192 B) → ark (192 B): the read_g2 loop (src/lib.rs:56-80). */
int kzgpot_g2_transcode_uncompressed(const uint8_t* in, size_t n, uint8_t* out, uint32_t flags, int64_t* first_bad);

/* As above, also writing one status byte per point (KZGPOT_ST_*) into status[n] (may be NULL). */
int kzgpot_g1_decompress_ex(const uint8_t* in, size_t n, uint8_t* out, uint32_t flags, int64_t* first_bad, uint8_t* status);
int kzgpot_g2_decompress_ex(const uint8_t* in, size_t n, uint8_t* out, uint32_t flags, int64_t* first_bad, uint8_t* status);
int kzgpot_g1_transcode_uncompressed_ex(const uint8_t* in, size_t n, uint8_t* out, uint32_t flags, int64_t* first_bad, uint8_t* status);
int kzgpot_g2_transcode_uncompressed_ex(const uint8_t* in, size_t n, uint8_t* out, uint32_t flags, int64_t* first_bad, uint8_t* status);

/* ---------------------------------------------------------------- hot path, device buffers (async) */
/* d_bad_key: one device uint64 that the call resets to UINT64_MAX (on `stream`) and that the
 * kernel lowers with atomicMin((index << 8) | status). d_status may be NULL. */
int kzgpot_g1_decompress_dev(const void* d_in, size_t n, void* d_out, uint32_t flags, uint64_t* d_bad_key,
                             uint8_t* d_status, void* stream);
int kzgpot_g2_decompress_dev(const void* d_in, size_t n, void* d_out, uint32_t flags, uint64_t* d_bad_key,
                             uint8_t* d_status, void* stream);
int kzgpot_g1_transcode_uncompressed_dev(const void* d_in, size_t n, void* d_out, uint32_t flags,
                                         uint64_t* d_bad_key, uint8_t* d_status, void* stream);
int kzgpot_g2_transcode_uncompressed_dev(const void* d_in, size_t n, void* d_out, uint32_t flags,
                                         uint64_t* d_bad_key, uint8_t* d_status, void* stream);
/* Host-side decode of a bad key copied back from the device: returns 0 (none) or -(status) and
 * sets *first_bad to the index (or -1). The multi-rank key KZGPOT_KEY_RANK_FAILED (0) decodes to
 * KZGPOT_E_RANK_FAILED with *first_bad = -1: a gathered buffer with a failed peer is never "ok". */
int kzgpot_decode_bad_key(uint64_t key, int64_t* first_bad);

/* ---------------------------------------------------------------- file pipeline (next-row §8f) */
#define KZGPOT_MODE_KZG 0     /* src/bin/preprocess-kgz.rs: Powers + VerifierKey file */
#define KZGPOT_MODE_FASTKZG 1 /* src/bin/preprocess-fastkgz.rs: UniversalParams + powers_of_h file */
/* powersoftau CONTRIBUTION_BYTE_SIZE for 2^n_log2 powers (603,981,040 at n_log2 = 21). */
uint64_t kzgpot_contribution_size(uint32_t n_log2);
/* Output size of `mode` for 2^n_log2 powers (kgz 603,980,256 / fastkzg 1,006,633,248 at 21). */
uint64_t kzgpot_output_size(uint32_t n_log2, int mode);
/* preprocess-{kgz,fastkgz} main (preprocess-kgz.rs:162-199, preprocess-fastkgz.rs:180-213) minus the
 * download: reads the response transcript at `transcript_path`, checks its size, decompresses and
 * checks every section, writes `out_path`. No intermediate file.
 * n_gpus is a SHARD count (0 = one per visible GPU; at most 64): each section is split into n_gpus contiguous
 * shards, each driven by a host thread on GPU (current + k) mod device_count — more shards than
 * GPUs put several shards on one GPU. The caller's current device is restored on return.
 * File path: the transcript is pread() in 32 MiB pieces while the GPU decodes what has arrived;
 * the output is pwrite()n as it lands into a temporary file "<out_path>.kzgpot-tmp-XXXXXX"
 * (mkstemp: unique per call) in the same directory, renamed over out_path only on success and
 * removed on any error, so out_path is either the complete file or untouched.
 * Returns 0 or a negative error; on a rejected point *bad_section (0 τG1, 1 τG2, 2 ατG1, 3 βτG1,
 * 4 βG2) and *bad_index locate it (pointers may be NULL). */
int kzgpot_preprocess(const char* transcript_path, const char* out_path, int mode, uint32_t n_log2, int n_gpus,
                      int* bad_section, int64_t* bad_index);
/* Same, on in-memory buffers (out must hold kzgpot_output_size bytes). */
int kzgpot_preprocess_buffer(const uint8_t* transcript, size_t len, uint8_t* out, int mode, uint32_t n_log2,
                             int n_gpus, int* bad_section, int64_t* bad_index);
/* With the BLAKE2b-512 digests (src/lib.rs:129; the reference checks the transcript against
 * POWERSOFTAU_DIGEST, preprocess-kgz.rs:19,51-61, and publishes the outputs' digests,
 * src/lib.rs:21-22). Hashing runs on host threads beside the GPU pass: the transcript from the
 * start, the output section by section as the GPU finishes it. expect_transcript_digest (128 hex
 * chars, may be NULL): a mismatch returns KZGPOT_E_DIGEST (and no output file is written).
 * transcript_digest / output_digest (may be NULL): receive 128 hex chars + NUL. */
int kzgpot_preprocess_ex(const char* transcript_path, const char* out_path, int mode, uint32_t n_log2, int n_gpus,
                         const char* expect_transcript_digest, char* transcript_digest, char* output_digest,
                         int* bad_section, int64_t* bad_index);
int kzgpot_preprocess_buffer_ex(const uint8_t* transcript, size_t len, uint8_t* out, int mode, uint32_t n_log2,
                                int n_gpus, const char* expect_transcript_digest, char* transcript_digest,
                                char* output_digest, int* bad_section, int64_t* bad_index);
/* BLAKE2b-512 (unkeyed, 64-byte digest) of a host buffer — blake2b_simd::State::new() (src/lib.rs:129). */
int kzgpot_blake2b(const uint8_t* data, size_t len, uint8_t* digest64);

/* ---------------------------------------------------------------- loader mirror (next-row §8f 2) */
/* ark-ec 0.2 GroupAffine in memory (what `deserialize_unchecked` returns): each Fp as 6 LE u64 in
 * ark-ff Montgomery form (R = 2^384), then `infinity` (u8) and zero padding to 8 B:
 *   G1 104 B = x[48] y[48] inf[1] pad[7];  G2 200 B = x.c0 x.c1 y.c0 y.c1 [4 x 48] inf[1] pad[7].
 * A Rust caller reads these as #[repr(C)] mirrors of GroupAffine. */
#define KZGPOT_G1_ARK_MONT_BYTES 104
#define KZGPOT_G2_ARK_MONT_BYTES 200
/* ark-uncompressed G1 (96 B) → GroupAffine (104 B): ArkG1Affine::deserialize_unchecked (src/lib.rs:180,
 * 183) — coordinates < p and SWFlags checked, NO curve and NO subgroup check. */
int kzgpot_g1_deserialize_unchecked(const uint8_t* in, size_t n, uint8_t* out, int64_t* first_bad);
/* ark-uncompressed G2 (192 B) → GroupAffine (200 B): ArkG2Affine::deserialize_unchecked (src/lib.rs:209-215). */
int kzgpot_g2_deserialize_unchecked(const uint8_t* in, size_t n, uint8_t* out, int64_t* first_bad);
int kzgpot_g1_deserialize_unchecked_ex(const uint8_t* in, size_t n, uint8_t* out, int64_t* first_bad, uint8_t* status);
int kzgpot_g2_deserialize_unchecked_ex(const uint8_t* in, size_t n, uint8_t* out, int64_t* first_bad, uint8_t* status);
int kzgpot_g1_deserialize_unchecked_dev(const void* d_in, size_t n, void* d_out, uint64_t* d_bad_key,
                                        uint8_t* d_status, void* stream);
int kzgpot_g2_deserialize_unchecked_dev(const void* d_in, size_t n, void* d_out, uint64_t* d_bad_key,
                                        uint8_t* d_status, void* stream);
/* load_kzg_setup (src/lib.rs:174-195) for 2^n_log2 powers (the reference fixes n_log2 = 21):
 * powers_of_g (2N-1 G1), powers_of_gamma_g (N G1), vk = g, gamma_g (G1), h, beta_h (G2) =
 * 2 x 104 + 2 x 200 B (VerifierKey::deserialize_unchecked; prepared_h / prepared_beta_h are the
 * caller's `h.into()` / `beta_h.into()`). Output buffers in the layout above. Trailing bytes are
 * ignored, as by the reference's sequential reader; a short file is KZGPOT_E_SIZE. On a rejected
 * point *bad_section (0 powers_of_g, 1 powers_of_gamma_g, 2 vk/h-beta_h, 3 powers_of_h) and
 * *bad_index locate it. */
int kzgpot_load_kzg_setup(const char* path, uint32_t n_log2, uint8_t* powers_of_g, uint8_t* powers_of_gamma_g,
                          uint8_t* vk, int* bad_section, int64_t* bad_index);
int kzgpot_load_kzg_setup_buffer(const uint8_t* file, size_t len, uint32_t n_log2, uint8_t* powers_of_g,
                                 uint8_t* powers_of_gamma_g, uint8_t* vk, int* bad_section, int64_t* bad_index);
/* load_fastkzg_setup (src/lib.rs:197-228): powers_of_g, powers_of_gamma_g, h_beta_h = h, beta_h
 * (2 x 200 B, as read: prepared_beta_h = beta_h.into()), powers_of_h (N G2). UniversalParams.beta_h
 * is powers_of_h[1] in the reference (src/lib.rs:221), not the beta_h read from the file. NB: the
 * reference opens KZG_SETUP_FILE here (src/lib.rs:198); this entry point takes the path. */
int kzgpot_load_fastkzg_setup(const char* path, uint32_t n_log2, uint8_t* powers_of_g, uint8_t* powers_of_gamma_g,
                              uint8_t* h_beta_h, uint8_t* powers_of_h, int* bad_section, int64_t* bad_index);
int kzgpot_load_fastkzg_setup_buffer(const uint8_t* file, size_t len, uint32_t n_log2, uint8_t* powers_of_g,
                                     uint8_t* powers_of_gamma_g, uint8_t* h_beta_h, uint8_t* powers_of_h,
                                     int* bad_section, int64_t* bad_index);

/* load_phase1(exp) (src/lib.rs:82-121, Phase1Parameters src/lib.rs:30-39), next-row §8f 3: a
 * phase1radix2m{exp} file = alpha, beta_g1 (G1), beta_g2 (G2), then coeffs_g1, coeffs_g2,
 * alpha_coeffs_g1, beta_coeffs_g1 (2^exp points each), every point read by read_g1 / read_g2
 * (src/lib.rs:41-80: pairing uncompressed, byte reorder, ark deserialize_uncompressed with the
 * subgroup check) into the in-memory GroupAffine layout (104 / 200 B per point). The reference
 * hardcodes the path "../phase1radix2m{exp}" (src/lib.rs:84); here it is an argument. Trailing
 * bytes are ignored; a short file is KZGPOT_E_SIZE. *bad_section: 0 alpha, 1 beta_g1, 2 beta_g2,
 * 3 coeffs_g1, 4 coeffs_g2, 5 alpha_coeffs_g1, 6 beta_coeffs_g1. */
uint64_t kzgpot_phase1_size(uint32_t exp);
int kzgpot_load_phase1(const char* path, uint32_t exp, uint8_t* alpha, uint8_t* beta_g1, uint8_t* beta_g2,
                       uint8_t* coeffs_g1, uint8_t* coeffs_g2, uint8_t* alpha_coeffs_g1, uint8_t* beta_coeffs_g1,
                       int* bad_section, int64_t* bad_index);
int kzgpot_load_phase1_buffer(const uint8_t* file, size_t len, uint32_t exp, uint8_t* alpha, uint8_t* beta_g1,
                              uint8_t* beta_g2, uint8_t* coeffs_g1, uint8_t* coeffs_g2, uint8_t* alpha_coeffs_g1,
                              uint8_t* beta_coeffs_g1, int* bad_section, int64_t* bad_index);

/* ---------------------------------------------------------------- group FFT, phase1radix2m writer */
/* The radix-2 FFT in G1 / G2 over the domain of size m = 2^exp generated by
 * w_m = 7^((r-1)/m) mod r (r the group order): bellman EvaluationDomain<Point<G>>::fft / ifft as
 * powersoftau's verifier runs them on the first m powers of each section before it writes the
 * phase1radix2m{exp} file that load_phase1 (src/lib.rs:82-121) reads; also the Lagrange basis of
 * ark-poly's Radix2EvaluationDomain (same generator 7, same two-adicity 32).
 *   forward: out[i] = sum_j [w_m^(ij)] in[j];   KZGPOT_FFT_INVERSE: out[i] = [1/m] sum_j [w_m^(-ij)] in[j]
 * both in natural order. Input: 2^exp ark-uncompressed records (96 B G1 / 192 B G2, what the
 * codecs above emit; infinity records are legal). A malformed record (coordinate >= p: status 3;
 * both SWFlags: status 6) is rejected with the loaders' statuses and index, and no output is
 * written. Points are NOT checked for curve or subgroup membership: the result is defined, and
 * equals bellman's bytes, only for points of the prime-order subgroup — what a checked decode
 * guarantees. exp <= 32 (memory permitting). */
#define KZGPOT_FFT_INVERSE 0x1u     /* monomial -> Lagrange (bellman ifft, incl. the 1/m) */
#define KZGPOT_FFT_OUT_PAIRING 0x2u /* emit pairing-uncompressed BE records (infinity: 0x40, zeros) instead of ark LE */
/* w_m as 32 big-endian bytes: bellman's `omega` of EvaluationDomain::from_coeffs (Fr::root_of_unity
 * squared 32 - exp times). Host only; exp > 32 -> KZGPOT_E_INVALID_ARG. */
int kzgpot_fr_domain_root(uint32_t exp, uint8_t root_be32[32]);
/* Bytes of device memory (d_work) the _dev calls below need; 0 for exp > 32. */
uint64_t kzgpot_group_fft_workspace(int g2, uint32_t exp);
/* bellman fft / ifft of 2^exp points in HBM, asynchronous on `stream`; d_out may equal d_in.
 * d_bad_key as for the codecs' _dev calls (reset to all ones, lowered to (index << 8) | status). */
int kzgpot_g1_fft_dev(const void* d_in, uint32_t exp, void* d_out, uint32_t flags, void* d_work, uint64_t* d_bad_key,
                      void* stream);
int kzgpot_g2_fft_dev(const void* d_in, uint32_t exp, void* d_out, uint32_t flags, void* d_work, uint64_t* d_bad_key,
                      void* stream);
/* The same on host buffers, synchronous, on the current device. */
int kzgpot_g1_fft(const uint8_t* in, uint32_t exp, uint8_t* out, uint32_t flags, int64_t* first_bad);
int kzgpot_g2_fft(const uint8_t* in, uint32_t exp, uint8_t* out, uint32_t flags, int64_t* first_bad);

/* Size of a phase1radix2m{exp} file as powersoftau's verifier writes it: kzgpot_phase1_size(exp)
 * (what load_phase1 reads) + the 2^exp - 1 H bases (96 B each) that follow. */
uint64_t kzgpot_phase1radix_size(uint32_t exp);
/* Replaces the part of powersoftau's verifier (verify_transform_constrained's parameter
 * preparation) that produces phase1radix2m{exp} from a response transcript of 2^n_log2 powers
 * (exp <= n_log2). Argument and size checks first (KZGPOT_E_INVALID_ARG / KZGPOT_E_SIZE, no GPU
 * needed); then the slices tauG1[0, 2m-1), tauG2[0, m), alpha tauG1[0, m), beta tauG1[0, m), betaG2
 * (m = 2^exp) are decoded with the default checked flags (infinity rejected, subgroup tested —
 * beta tauG1 and betaG2 included); then, pairing-uncompressed: alpha tauG1[0], beta tauG1[0],
 * betaG2, ifft(tauG1[0..m)), ifft(tauG2[0..m)), ifft(alpha tauG1[0..m)), ifft(beta tauG1[0..m)),
 * h[i] = tauG1[m + i] - tauG1[i] for i < m - 1. One GPU (the current device, restored on return).
 * On a rejected point *bad_section / *bad_index as kzgpot_preprocess. */
int kzgpot_prepare_phase2_buffer(const uint8_t* transcript, size_t len, uint32_t n_log2, uint32_t exp, uint8_t* out,
                                 int* bad_section, int64_t* bad_index);
/* File to file: out_path is written through a temporary "<out_path>.kzgpot-tmp-XXXXXX" renamed over
 * it on success, so it is either the complete file or untouched. */
int kzgpot_prepare_phase2(const char* transcript_path, const char* out_path, uint32_t n_log2, uint32_t exp,
                          int* bad_section, int64_t* bad_index);

/* ---------------------------------------------------------------- multi-scalar multiplication (KZG10 commit) */
/* out = sum_{i<n} [s_i] P_i in G1 / G2: ark-ec VariableBaseMSM::multi_scalar_mul as ark-poly-commit
 * 0.2 KZG10::commit runs it over powers_of_g (and powers_of_gamma_g for the blinding polynomial) —
 * the one thing the reference's end_to_end_test_kzg (src/lib.rs:230-290) does with a loaded setup.
 * One ark-uncompressed record out (96 / 192 B; the infinity record for an empty or vanishing sum).
 *   scalars: n x 32 bytes, each a 256-bit unsigned integer, little-endian — the byte image of
 *     ark-ff BigInteger256 (4 LE u64), what `coeff.into_repr()` gives. Used as INTEGERS: no range
 *     check, no reduction mod r (2^256 - 1, r and 0 are legal); for points of the prime-order
 *     subgroup that is ark's result.
 *   bases: n packed ark-uncompressed records (what the codecs and the group FFT emit), range- and
 *     flag-checked as the loaders check them (coordinate >= p: status 3; both SWFlags: 6; smallest
 *     failing index; a rejected call writes nothing). An infinity record is legal and contributes
 *     nothing. Not re-checked for curve or subgroup membership: off the curve the result is undefined.
 *   KZGPOT_MSM_BASES_MONT: bases are the loaders' in-memory GroupAffine records instead
 *     (KZGPOT_G1_ARK_MONT_BYTES / KZGPOT_G2_ARK_MONT_BYTES), so rows of Powers.powers_of_g go in
 *     unchanged; a coordinate >= p gives status 3, a non-zero infinity byte is the point at infinity.
 *   KZGPOT_MSM_WINDOW(c): window width override, 1 <= c <= 16, in flag bits 8..12; 0: the library
 *     chooses (kzgpot_msm_window_bits).
 * n = 0 gives the infinity record; n > 2^26, an unknown flag, a width above 16, or an override
 * with n ceil(256 / c) >= 2^32 is KZGPOT_E_INVALID_ARG. */
#define KZGPOT_MSM_BASES_MONT 0x1u
#define KZGPOT_MSM_WINDOW(c) (((uint32_t)(c) & 0x1fu) << 8)
/* Host only. The width c the library chooses for n points, a table:
 *   n <  28416: 8    n <  55872: 9    n <  120384: 10   n <  238720: 11   n < 472064: 12
 *   n < 1114113: 13  n < 2244609: 14  n < 3669568: 15   otherwise: 16
 * Each threshold is the smallest n at which the cost model  n W + B + 43 (W max(min(n, 2^c), n / 64) + B / 64),
 * W = ceil(256 / c), B = W c 2^(c-1) — bucket additions, bit-partial additions and one inversion
 * (about 43 additions' worth) per 64-entry partial sum — prefers c to c - 1. */
uint32_t kzgpot_msm_window_bits(uint64_t n);
/* Host only. Bytes of device memory (d_work) the _dev calls below need for these flags; 0 for
 * invalid arguments. Without a width override the size is monotone in n. */
uint64_t kzgpot_msm_workspace(int g2, uint64_t n, uint32_t flags);
/* Asynchronous on `stream`: d_bases, d_scalars (4-byte aligned), d_out (one record, 16-byte
 * aligned) and d_work in HBM. d_bad_key as for kzgpot_g1_fft_dev (reset to all ones, lowered to
 * (index << 8) | status by a malformed base, after which d_out is not written). */
int kzgpot_g1_msm_dev(const void* d_bases, const void* d_scalars, uint64_t n, void* d_out, uint32_t flags, void* d_work,
                      uint64_t* d_bad_key, void* stream);
int kzgpot_g2_msm_dev(const void* d_bases, const void* d_scalars, uint64_t n, void* d_out, uint32_t flags, void* d_work,
                      uint64_t* d_bad_key, void* stream);
/* The same on host buffers, synchronous, on the current device. */
int kzgpot_g1_msm(const uint8_t* bases, const uint8_t* scalars, uint64_t n, uint8_t* out, uint32_t flags,
                  int64_t* first_bad);
int kzgpot_g2_msm(const uint8_t* bases, const uint8_t* scalars, uint64_t n, uint8_t* out, uint32_t flags,
                  int64_t* first_bad);

/* ---------------------------------------------------------------- polynomial division over Fr, KZG10 open */
/* For n coefficients c[0..n) of p, lowest degree first, and a point z: value = p(z) and the n - 1
 * coefficients of the witness polynomial (p(x) - p(z)) / (x - z), as a tiled scan of the Horner
 * recurrence H[j] = c[j] + z H[j+1] (value = H[0], quotient[j] = H[j+1]) on the GPU.
 *   coeffs, z: 32-byte little-endian 256-bit integers (the byte image of BigInteger256), any value:
 *     each is reduced mod r (2^256 - 1 is legal and means its residue).
 *   quotient: (n - 1) x 32 bytes, value: 32 bytes, little-endian, canonical (below r). quotient may be
 *     NULL: evaluate only. It must not overlap coeffs.
 *   KZGPOT_POLY_TILE(t): coefficients per 256-lane block, 2^t with 8 <= t <= 12, in flag bits
 *     16..19; 0: the library's tile (2^11). The result does not depend on it.
 * n = 0 gives value 0; n = 1 gives value c[0] mod r and an empty quotient. n > 2^26 + 1, an unknown
 * flag bit, a tile outside 8..12 or a NULL pointer where a count is non-zero is KZGPOT_E_INVALID_ARG. */
#define KZGPOT_POLY_TILE(t) (((uint32_t)(t) & 0xfu) << 16)
/* Host only. Bytes of device memory (d_work) the division needs (at least 256; monotone in n);
 * 0 for invalid arguments. */
uint64_t kzgpot_fr_poly_workspace(uint64_t n, uint32_t flags);
/* Asynchronous on `stream`: d_coeffs, d_quotient and d_value (16-byte aligned) and d_work in HBM;
 * z_le32 is read on the host before the call returns. */
int kzgpot_fr_poly_divide_dev(const void* d_coeffs, uint64_t n, const uint8_t z_le32[32], void* d_quotient,
                              void* d_value, uint32_t flags, void* d_work, void* stream);
/* The same on host buffers, synchronous, on the current device. */
int kzgpot_fr_poly_divide(const uint8_t* coeffs, uint64_t n, const uint8_t z_le32[32], uint8_t* quotient,
                          uint8_t value_le32[32], uint32_t flags);

/* ark-poly-commit 0.2 KZG10::open (compute_witness_polynomial, then open_with_witness_polynomial)
 * for a polynomial p of n coefficients and, when hiding, the blinding polynomial b of n_blind
 * coefficients that commit drew (n_blind = 0: ark's None). out, 160 bytes:
 *   [0, 96)    w, an ark-uncompressed G1 record:
 *              sum_{j<n-1} [q[j]] powers_of_g[j] + sum_{j<n_blind-1} [q_b[j]] powers_of_gamma_g[j],
 *              q and q_b the witness polynomials of p and b at z
 *   [96, 128)  value = p(z), little-endian, canonical
 *   [128, 160) random_v = b(z), little-endian, canonical; zeros when n_blind = 0
 * Both divisions run as above and w is ONE multi-scalar multiplication over the two base ranges and
 * the two quotients laid end to end in the workspace; the quotients never leave HBM.
 *   flags: KZGPOT_MSM_BASES_MONT and KZGPOT_MSM_WINDOW(c) as for the MSM (rows of
 *     Powers.powers_of_g go in unchanged with the first), KZGPOT_POLY_TILE(t) as above.
 *   bases: only the first n - 1 records of powers_of_g and n_blind - 1 of powers_of_gamma_g are read
 *     (supplying that many is the caller's contract), checked as the MSM checks them. A rejected call
 *     writes nothing; the index counts along the concatenation: i < n - 1 is in powers_of_g,
 *     otherwise i - (n - 1) is in powers_of_gamma_g.
 * n = 0 or 1 (and n_blind <= 1) gives the infinity record. Coefficients are used as given: ark
 * trims trailing zeros first, which changes no output byte. KZGPOT_E_INVALID_ARG, before any device
 * use: a NULL pointer where a count is non-zero, an unknown flag bit, a tile outside 8..12, n or
 * n_blind above 2^26 + 1, or n - 1 + n_blind - 1 bases above what the MSM takes at that width. */
/* Host only. Bytes of d_work for these arguments; 0 when they are invalid. Without a width
 * override the size is monotone in n and in n_blind. */
uint64_t kzgpot_kzg_open_workspace(uint64_t n, uint64_t n_blind, uint32_t flags);
/* Asynchronous on `stream`: every d_ pointer in HBM, d_coeffs, d_blinding, d_out (160 B) and d_work
 * 16-byte aligned. d_bad_key as for kzgpot_g1_msm_dev. */
int kzgpot_g1_kzg_open_dev(const void* d_powers_of_g, const void* d_coeffs, uint64_t n, const void* d_powers_of_gamma_g,
                           const void* d_blinding, uint64_t n_blind, const uint8_t z_le32[32], void* d_out,
                           uint32_t flags, void* d_work, uint64_t* d_bad_key, void* stream);
/* The same on host buffers, synchronous, on the current device. */
int kzgpot_g1_kzg_open(const uint8_t* powers_of_g, const uint8_t* coeffs, uint64_t n, const uint8_t* powers_of_gamma_g,
                       const uint8_t* blinding, uint64_t n_blind, const uint8_t z_le32[32], uint8_t out[160],
                       uint32_t flags, int64_t* first_bad);

/* ---------------------------------------------------------------- Fr NTT, amortized KZG10 openings (FK20) */
/* The number-theoretic transform over Fr on the domain of size m = 2^exp generated by
 * w = 7^((r-1)/m) (kzgpot_fr_domain_root), natural order in and out:
 *   forward               out[i] = sum_j in[j] w^(ij)          (coefficients -> evaluations p(w^i))
 *   KZGPOT_NTT_INVERSE    out[i] = 1/m sum_j in[j] w^(-ij)
 * in, out: 2^exp values of 32 little-endian bytes; inputs are any 256-bit integers, each reduced mod r,
 * outputs are canonical (below r). out may be in.
 *   KZGPOT_POLY_TILE(t): elements per 256-lane block, 2^t with 8 <= t <= 11 (the 64 KB of LDS), in the
 *     division's flag bits; 0: the library's tile (2^9). The result does not depend on it.
 * exp > 26, an unknown flag bit, a tile outside 8..11 or a NULL pointer is KZGPOT_E_INVALID_ARG
 * before any device use. */
#define KZGPOT_NTT_INVERSE 0x1u
/* Host only. Bytes of d_work for these arguments (at least 512); 0 when they are invalid. Two
 * twiddle tables of about 2^(exp/2) elements each and, where the transform takes more than one pass
 * (exp > t, t the tile), 32 x 2^exp bytes that only an in-place call uses. */
uint64_t kzgpot_fr_ntt_workspace(uint32_t exp, uint32_t flags);
/* Asynchronous on `stream`: d_in, d_out (16-byte aligned) and d_work in HBM. */
int kzgpot_fr_ntt_dev(const void* d_in, uint32_t exp, void* d_out, uint32_t flags, void* d_work, void* stream);
/* The same on host buffers, synchronous, on the current device. */
int kzgpot_fr_ntt(const uint8_t* in, uint32_t exp, uint8_t* out, uint32_t flags);

/* All n = 2^exp opening proofs of one polynomial p over the domain {w^i} at once (Feist and
 * Khovratovich's amortized KZG proofs, "FK20"), from a table that depends on the setup and exp only:
 *   table    T[i] = sum_{j<n} [x^(n-1-j)] powers[j], x = w_2n^i, i < 2n: the forward group FFT of size
 *            2n over powers[n-1], .., powers[0] followed by n points at infinity. 2n ark-uncompressed
 *            records (96 B in G1, 192 B in G2); powers: the first n records of powers_of_g (G1) or
 *            powers_of_h (G2, the fastkzg setup), ark-uncompressed.
 *   proofs   proofs[i] = [(p(tau) - p(w^i)) / (tau - w^i)] G, i < n, natural order: what KZG10::open
 *            returns as w at z = w^i, without hiding. n ark-uncompressed records.
 *   values   values[i] = p(w^i), n x 32 little-endian bytes, canonical. May be NULL: proofs only.
 *   coeffs   n_coeffs <= n values of 32 bytes, as for the division (reduced mod r, used as given).
 *   flags    KZGPOT_POLY_TILE(t) only, handed to the NTT.
 * One call is two NTTs, 2n scalar multiplications, a group FFT of 2n and one of n points
 * (O(n log n) group operations against the n multi-scalar multiplications of n openings); everything
 * between the table and the proofs stays in HBM. Records of powers and table are checked as the group
 * FFT checks its input: -3 / -6 with the smallest index, and a rejected call writes nothing.
 * n_coeffs <= 1 gives n infinity records and values all c[0] mod r (0 for none). exp > 24,
 * n_coeffs > 2^exp, an unknown flag bit, a tile outside 8..11 or a NULL pointer where a count is
 * non-zero is KZGPOT_E_INVALID_ARG before any device use; the workspace functions then return 0.
 * Hiding proofs are out of scope: they would need a second table over powers_of_gamma_g and the
 * blinding polynomial. */
/* Host only: bytes of d_work; monotone in exp. */
uint64_t kzgpot_open_domain_table_workspace(int g2, uint32_t exp);
uint64_t kzgpot_open_domain_workspace(int g2, uint32_t exp, uint32_t flags);
/* Asynchronous on `stream`: every d_ pointer in HBM and 16-byte aligned, d_bad_key as for
 * kzgpot_g1_fft_dev (an index along powers, or along table). */
int kzgpot_g1_open_domain_table_dev(const void* d_powers, uint32_t exp, void* d_table, void* d_work,
                                    uint64_t* d_bad_key, void* stream);
int kzgpot_g2_open_domain_table_dev(const void* d_powers, uint32_t exp, void* d_table, void* d_work,
                                    uint64_t* d_bad_key, void* stream);
int kzgpot_g1_open_domain_dev(const void* d_table, const void* d_coeffs, uint64_t n_coeffs, uint32_t exp,
                              void* d_proofs, void* d_values, uint32_t flags, void* d_work, uint64_t* d_bad_key,
                              void* stream);
int kzgpot_g2_open_domain_dev(const void* d_table, const void* d_coeffs, uint64_t n_coeffs, uint32_t exp,
                              void* d_proofs, void* d_values, uint32_t flags, void* d_work, uint64_t* d_bad_key,
                              void* stream);
/* The same on host buffers, synchronous, on the current device. */
int kzgpot_g1_open_domain_table(const uint8_t* powers, uint32_t exp, uint8_t* table, int64_t* first_bad);
int kzgpot_g2_open_domain_table(const uint8_t* powers, uint32_t exp, uint8_t* table, int64_t* first_bad);
int kzgpot_g1_open_domain(const uint8_t* table, const uint8_t* coeffs, uint64_t n_coeffs, uint32_t exp,
                          uint8_t* proofs, uint8_t* values, uint32_t flags, int64_t* first_bad);
int kzgpot_g2_open_domain(const uint8_t* table, const uint8_t* coeffs, uint64_t n_coeffs, uint32_t exp,
                          uint8_t* proofs, uint8_t* values, uint32_t flags, int64_t* first_bad);

/* ---------------------------------------------------------------- evaluation form: batch inversion, KZG10 open */
/* Scalars here are 32 little-endian bytes; an input is any 256-bit integer and is reduced mod r
 * (2^256 - 1 is legal and means its residue), an output is canonical (below r). Vectors over the
 * domain of size n = 2^exp generated by w = kzgpot_fr_domain_root(exp) are in natural order: entry i
 * belongs to w^i, the order of kzgpot_fr_ntt, of kzgpot_g1_fft's output and of
 * kzgpot_g1_open_domain's values.
 *   KZGPOT_POLY_TILE(t): entries per 256-lane block, 2^t with 8 <= t <= 12, as for the division; 0:
 *     the library's tile (2^11). No result depends on it.
 *
 * Batch inversion: out[i] = in[i]^-1 mod r, and out[i] = 0 where in[i] = 0 mod r (the convention of
 * ark-ff's batch_inversion). n <= 2^26 entries; out may be in. One field inversion per tile.
 * n > 2^26, an unknown flag bit, a tile outside 8..12 or a NULL pointer where n is non-zero is
 * KZGPOT_E_INVALID_ARG before any device use. */
/* Asynchronous on `stream`: d_in and d_out (16-byte aligned) in HBM; no workspace. */
int kzgpot_fr_batch_inverse_dev(const void* d_in, uint64_t n, void* d_out, uint32_t flags, void* stream);
/* The same on host buffers, synchronous, on the current device. */
int kzgpot_fr_batch_inverse(const uint8_t* in, uint64_t n, uint8_t* out, uint32_t flags);

/* Division by (x - z) in evaluation form. evals[i] = p(w^i), i < n = 2^exp, for a polynomial p of
 * degree below n; z any 256-bit integer.
 *   value      p(z)
 *   quotient   the n evaluations q_i of (p(x) - p(z)) / (x - z) on the same domain. May be NULL:
 *              evaluate only. It must not overlap evals.
 * z off the domain (z^n != 1):  value = (z^n - 1)/n sum_i e_i w^i / (z - w^i),  q_i = (value - e_i) / (z - w^i).
 * z = w^m:  value = e_m,  q_i = (value - e_i) / (z - w^i) for i != m,  q_m = - sum_{i != m} q_i w^(i-m).
 * n = 1: the domain is {1}; the value is e_0 and the quotient [0] for every z.
 * The n differences z - w^i are inverted by the batch inversion's tile routine. exp > 26, an unknown
 * flag bit, a tile outside 8..12 or a NULL pointer is KZGPOT_E_INVALID_ARG before any device use. */
/* Host only. Bytes of device memory (d_work) the division needs: 32 n for the inverted differences,
 * two partial sums per tile, 256 more; monotone in exp; 0 for invalid arguments. */
uint64_t kzgpot_fr_evals_workspace(uint32_t exp, uint32_t flags);
/* Asynchronous on `stream`: d_evals, d_quotient, d_value (16-byte aligned) and d_work in HBM; z_le32
 * is read on the host before the call returns. */
int kzgpot_fr_evals_divide_dev(const void* d_evals, uint32_t exp, const uint8_t z_le32[32], void* d_quotient,
                               void* d_value, uint32_t flags, void* d_work, void* stream);
/* The same on host buffers, synchronous, on the current device. */
int kzgpot_fr_evals_divide(const uint8_t* evals, uint32_t exp, const uint8_t z_le32[32], uint8_t* quotient,
                           uint8_t value_le32[32], uint32_t flags);

/* KZG10 open from evaluations: the proof that p(z) = value for the commitment
 * sum_i [e_i] lagrange[i] (kzgpot_g1_msm over the same basis), without the coefficients of p.
 * lagrange: the n = 2^exp records [L_i(tau)]G of the Lagrange basis, natural order: kzgpot_g1_fft
 * (inverse) of the first n records of powers_of_g. out, 128 bytes:
 *   [0, 96)    w = sum_i [q_i] lagrange[i], an ark-uncompressed G1 record; q the quotient above. For
 *              every z, on the domain or off it, it is the w of kzgpot_g1_kzg_open for the coefficients of p.
 *   [96, 128)  value = p(z), little-endian, canonical
 * The quotient stays in the workspace and w is ONE multi-scalar multiplication over the caller's
 * records where they lie (no staging copy: there is one base range).
 *   flags: KZGPOT_MSM_BASES_MONT and KZGPOT_MSM_WINDOW(c) as for the MSM, KZGPOT_POLY_TILE(t) as above.
 *   bases: all n records are read and checked as the MSM checks them: -(status) with the smallest
 *     index of a malformed record, and a rejected call writes nothing.
 * KZGPOT_E_INVALID_ARG, before any device use: a NULL pointer, an unknown flag bit, a tile outside
 * 8..12, exp > 26, or n bases above what the MSM takes at that width; the workspace function then
 * returns 0.
 * Hiding proofs are out of scope: the blinding quotient lives over powers_of_gamma_g, which the
 * loaders hold as 104-byte Montgomery rows while the Lagrange basis is 96-byte ark records, and one
 * MSM takes one record format. */
/* Host only. Bytes of d_work for these arguments; 0 when they are invalid. */
uint64_t kzgpot_kzg_open_evals_workspace(uint32_t exp, uint32_t flags);
/* Asynchronous on `stream`: every d_ pointer in HBM, d_evals, d_out (128 B) and d_work 16-byte
 * aligned. d_bad_key as for kzgpot_g1_msm_dev. */
int kzgpot_g1_kzg_open_evals_dev(const void* d_lagrange, const void* d_evals, uint32_t exp, const uint8_t z_le32[32],
                                 void* d_out, uint32_t flags, void* d_work, uint64_t* d_bad_key, void* stream);
/* The same on host buffers, synchronous, on the current device. */
int kzgpot_g1_kzg_open_evals(const uint8_t* lagrange, const uint8_t* evals, uint32_t exp, const uint8_t z_le32[32],
                             uint8_t out[128], uint32_t flags, int64_t* first_bad);

/* ---------------------------------------------------------------- pairing product, KZG10 check / batch_check */
/* The functions of this section that verify something return 1 (the product is one / the proofs are
 * accepted) or 0 (it is not / they are rejected) where the rest of the library returns 0 for success;
 * a negative value is an error as everywhere else: -(status) for a malformed record, with its index in
 * *first_bad, and <= KZGPOT_E_INVALID_ARG for argument and device errors.
 *
 * Pairing product: prod_{i < k} e(P_i, Q_i)^d over BLS12-381, e the optimal ate pairing and
 * d = KZGPOT_PAIRING_GT_POWER. The tower is ark-bls12-381's: Fq2 = Fq[u]/(u^2 + 1),
 * Fq6 = Fq2[v]/(v^3 - (u + 1)), Fq12 = Fq6[w]/(w^2 - v); the twist is of M type; the Miller loop runs
 * over |x| = 0xd201000000010000 and its value is conjugated for the negative x. One lane runs the
 * Miller loop of one pair, the lanes' values are multiplied by a tree, and ONE final exponentiation is
 * applied to the product.
 *   d          The hard part of the final exponentiation computes f^(3 (p^4 - p^2 + 1) / r), so the GT
 *              value is the CUBE of the reduced pairing f^((p^12 - 1) / r): d = 3. r is prime and not 3,
 *              so the product is one for d = 3 exactly when it is for d = 1, and the booleans of this
 *              section do not depend on d. The GT bytes do: they are e(P, Q)^3 by the mathematical
 *              definition. No byte equality with ark's Bls12_381::pairing is claimed.
 *   g1, g2     k ark-uncompressed G1 records (96 B) and G2 records (192 B). Both are range- and
 *              flag-checked as the MSM checks its bases (status 3 or 6), the index counting along g1
 *              then g2: i < k is g1[i], otherwise g2[i - k]; the smallest is reported and a rejected
 *              call writes nothing. A record with the infinity flag, on either side, is legal and its
 *              pair contributes 1. Points are NOT checked for curve or subgroup membership: as for the
 *              MSM, the result is defined for points of the prime-order subgroups (decode through
 *              the checked codecs).
 *   out_gt     KZGPOT_GT_BYTES bytes, or NULL: the product in ark's serialization order of Fq12,
 *              c0.c0.c0, c0.c0.c1, c0.c1.c0, .., c1.c2.c1, each 48 little-endian bytes, canonical.
 *   k          at most KZGPOT_PAIRING_MAX_PAIRS (the work is one lane per pair); k = 0 gives one.
 * k above the cap or a NULL pointer where k is non-zero is KZGPOT_E_INVALID_ARG before any device use,
 * and the workspace function then returns 0. */
#define KZGPOT_PAIRING_GT_POWER 3
#define KZGPOT_PAIRING_MAX_PAIRS 65536u
#define KZGPOT_GT_BYTES 576
/* Host only. Bytes of device memory (d_work) for k pairs: 3,248 per pair (a lane's 29 Fq2 cells), in
 * blocks of 64 pairs, and 6,400 for the final exponentiation; monotone in k; 0 for k above the cap. */
uint64_t kzgpot_pairing_workspace(uint64_t k);
/* Asynchronous on `stream`: every d_ pointer in HBM and 16-byte aligned. d_out: KZGPOT_GT_BYTES of GT,
 * then one u32 that is 1 if the product is one and 0 if not (580 bytes). d_bad_key as for
 * kzgpot_g1_msm_dev; d_out is written only if it reports no rejection. Returns 0 or an error. */
int kzgpot_pairing_product_dev(const void* d_g1, const void* d_g2, uint64_t k, void* d_out, void* d_work,
                               uint64_t* d_bad_key, void* stream);
/* The same on host buffers, synchronous, on the current device: 1 if the product is one, 0 if not. */
int kzgpot_pairing_product(const uint8_t* g1, const uint8_t* g2, uint64_t k, uint8_t* out_gt, int64_t* first_bad);

/* KZG10 batch_check: ark-poly-commit 0.2's KZG10::batch_check over n proofs with the randomizers rho_i
 * supplied by the caller (ark takes rho_0 = 1 and draws every later one as a u128 from the caller's
 * rng; this library never draws randomness itself):
 *   total_c = sum_i [rho_i] (C_i + [z_i] W_i) - [sum_i rho_i v_i] g - [sum_i rho_i vbar_i] gamma_g
 *   total_w = sum_i [rho_i] W_i
 *   accepted iff  e(total_c, h) e(-total_w, beta_h) = 1
 * An Fr pass writes the scalars rho_i, rho_i z_i and the two negated sums; total_c is ONE multi-scalar
 * multiplication over commitments, proofs, g, gamma_g (2 n + 2 bases, staged end to end), total_w a
 * second one over the proofs where they lie; the pairing product above runs over the two pairs. The
 * scalars and both sums never leave device memory.
 *   vk            g, gamma_g (96 B each), h, beta_h (192 B each), ark-uncompressed: 576 bytes
 *   commitments, proofs_w   n ark-uncompressed G1 records each
 *   points, values, random_vs, randomizers   n x 32 little-endian bytes each, every one any 256-bit
 *                 integer, reduced mod r. random_vs may be NULL: no proof is hiding (every vbar_i = 0).
 *   flags         KZGPOT_MSM_WINDOW(c) only
 *   first_bad     counts along commitments, proofs, then the four vk records: i < n is commitments[i],
 *                 i < 2 n is proofs_w[i - n], then g, gamma_g, h, beta_h. Records are checked as the
 *                 MSM and the pairing product check theirs; points are not checked for subgroup
 *                 membership.
 * n = 0 is accepted, as ark's empty product is. n <= 2^25 - 1, so that 2 n + 2 stays within what the
 * MSM takes; above that, a NULL pointer where n is non-zero (random_vs excepted), a NULL vk or an
 * unknown flag bit is KZGPOT_E_INVALID_ARG before any device use, and the workspace function returns 0.
 *
 * KZG10 check is the batch call with n = 1 and rho = 1: ark's equation
 * e(C - [v] g - [vbar] gamma_g, h) = e(W, beta_h - [z] h) with [z] W moved to the left-hand side,
 * e(C + [z] W - [v] g - [vbar] gamma_g, h) e(-W, beta_h) = 1, which needs no G2 scalar multiplication. */
/* Host only. Bytes of d_work for n proofs; monotone in n; 0 when the arguments are invalid. */
uint64_t kzgpot_kzg_batch_check_workspace(uint64_t n, uint32_t flags);
/* Asynchronous on `stream`: every d_ pointer in HBM and 16-byte aligned (d_vk: the 576 bytes above;
 * d_random_vs may be NULL). d_out as for kzgpot_pairing_product_dev: the GT value of the check's
 * product, then the u32 that is 1 if the proofs are accepted. d_bad_key as for kzgpot_g1_msm_dev.
 * Returns 0 or an error. */
int kzgpot_kzg_batch_check_dev(const void* d_vk, const void* d_commitments, const void* d_points, const void* d_values,
                               const void* d_proofs_w, const void* d_random_vs, const void* d_randomizers, uint64_t n,
                               void* d_out, uint32_t flags, void* d_work, uint64_t* d_bad_key, void* stream);
/* The same on host buffers, synchronous, on the current device: 1 accepted, 0 rejected. */
int kzgpot_kzg_batch_check(const uint8_t vk[576], const uint8_t* commitments, const uint8_t* points,
                           const uint8_t* values, const uint8_t* proofs_w, const uint8_t* random_vs,
                           const uint8_t* randomizers, uint64_t n, uint32_t flags, int64_t* first_bad);
/* One proof: random_v_le32 may be NULL (not hiding). first_bad: 0 the commitment, 1 w, 2 .. 5 the vk records. */
int kzgpot_kzg_check(const uint8_t vk[576], const uint8_t commitment[96], const uint8_t z_le32[32],
                     const uint8_t value_le32[32], const uint8_t w[96], const uint8_t* random_v_le32, int64_t* first_bad);

/* ---------------------------------------------------------------- BN254 (config 5, next-row §8f 4) */
/* No reference counterpart: the same path instantiated for ark-bn254 0.2 G1 (cofactor 1).
 * ark compressed (32 B: x LE, SWFlags bit7 PositiveY / bit6 Infinity in byte 31) → ark
 * uncompressed (64 B) = ark-ec 0.2 GroupAffine::deserialize + serialize_uncompressed. The point
 * at infinity is legal (→ ark zero()). Statuses: 3 NotInField, 4 NotOnCurve, 6 UnexpectedFlags. */
int kzgpot_bn254_g1_decompress(const uint8_t* in, size_t n, uint8_t* out, int64_t* first_bad);
int kzgpot_bn254_g1_decompress_ex(const uint8_t* in, size_t n, uint8_t* out, int64_t* first_bad, uint8_t* status);
int kzgpot_bn254_g1_decompress_dev(const void* d_in, size_t n, void* d_out, uint64_t* d_bad_key, uint8_t* d_status,
                                   void* stream);

/* ---------------------------------------------------------------- multi-GPU, RCCL inside */
/* north_star: "the τ^i array shards trivially across the 8 GPUs of one node with a final RCCL
 * all-gather over xGMI to produce one contiguous arkworks buffer". Replaces the reference's only
 * parallel stage, the chunked decompression of powersoftau's Accumulator::deserialize
 * (src/bin/preprocess-kgz.rs:105-110), whose workers fill disjoint slices of one Vec — here the
 * slices live on different GPUs and RCCL assembles them. One process (or thread) per GPU.
 *   rank 0: kzgpot_comm_unique_id(id); ship the 128 bytes to every rank (MPI, torch.distributed,
 *   a file, ...); every rank, with its GPU current: kzgpot_comm_init(&comm, id, nranks, rank).
 * RCCL is bound at first use with dlopen("librccl.so.1") (in a torch process: the RCCL torch has
 * already loaded). */
#define KZGPOT_COMM_ID_BYTES 128
int kzgpot_comm_unique_id(uint8_t* id);
int kzgpot_comm_init(void** comm, const uint8_t* id, int nranks, int rank); /* collective */
int kzgpot_comm_destroy(void* comm);
#define KZGPOT_OP_G1_DECOMPRESS 0
#define KZGPOT_OP_G2_DECOMPRESS 1
#define KZGPOT_OP_G1_TRANSCODE 2
#define KZGPOT_OP_G2_TRANSCODE 3
#define KZGPOT_OP_BN254_G1_DECOMPRESS 4
/* Block-cyclic layout of n points over nranks x chunks: *block = floor(n / (nranks chunks)) points
 * per block, *tail = the n - nranks chunks block points at the end. Rank k owns blocks
 * c nranks + k (global points [(c nranks + k) block, +block)), c = 0..chunks-1; every rank also
 * decodes the tail. */
int kzgpot_shard_layout(uint64_t n, int nranks, uint32_t chunks, uint64_t* block, uint64_t* tail);
/* Collective, asynchronous on `stream` (a hipStream_t of the communicator's GPU). d_in_local =
 * this rank's input records: its `chunks` owned blocks in chunk order, then the tail (chunks x
 * block + tail records). d_out = all n output records (HBM, every rank). Each chunk is decoded
 * on `stream` and then all-gathered in place (ncclAllGather on the communicator's own stream)
 * while the next chunk decodes. *d_bad_key = the first rejected point over ALL ranks as
 * (global index << 8) | status, or all ones (decode with kzgpot_decode_bad_key); rejected
 * records are zero-filled as in the single-GPU calls. `stream` waits for the gathers.
 * Collective contract: every rank calls with the same op, n, chunks and flags (the layout is
 * derived from them). Errors never desynchronise the ranks:
 *  - argument errors (identical on every rank, since the arguments are) return
 *    KZGPOT_E_INVALID_ARG before any collective is queued;
 *  - a local HIP failure (a decode launch, an event, the key buffer) stops this rank's decoding
 *    but every collective is still issued, so no peer waits forever; the all-reduced key is then
 *    KZGPOT_KEY_RANK_FAILED on every rank (kzgpot_comm_wait returns KZGPOT_E_RANK_FAILED) and
 *    this call returns KZGPOT_E_DEVICE. The communicator stays usable;
 *  - a failing RCCL call aborts the communicator (ncclCommAbort; later calls return
 *    KZGPOT_E_DEVICE) and returns KZGPOT_E_DEVICE. Peers then fail in their own RCCL calls or
 *    time out in kzgpot_comm_wait.
 * Calls on one communicator are ordered: each waits (on its `stream`) for the previous call's
 * collectives before touching the communicator's key buffers, whatever stream that call used. */
int kzgpot_decode_allgather_dev(void* comm, int op, const void* d_in_local, uint64_t n, uint32_t chunks, void* d_out,
                                uint32_t flags, uint64_t* d_bad_key, void* stream);
#define KZGPOT_KEY_RANK_FAILED 0ull /* the all-reduced key when some rank failed (no real key is 0: status >= 1) */
/* Host-side completion of kzgpot_decode_allgather_dev: waits for `stream` (polling, so that a
 * stuck collective cannot hang the caller), then decodes *d_bad_key. Returns 0 (every point
 * accepted), -(status) of the first rejected point (*first_bad = its global index),
 * KZGPOT_E_RANK_FAILED when a rank could not decode its share, KZGPOT_E_DEVICE on a device or
 * RCCL asynchronous error, or KZGPOT_E_TIMEOUT after timeout_ms (0 = no limit) — the last two
 * abort the communicator, which makes RCCL's kernels on this rank exit (the CUDA-style watchdog
 * a torch process group runs). first_bad may be NULL. */
int kzgpot_comm_wait(void* comm, const uint64_t* d_bad_key, int64_t* first_bad, uint32_t timeout_ms, void* stream);
/* What RCCL itself reports for the communicator (ncclCommCount / ncclCommUserRank /
 * ncclCommCuDevice): the rank count, this rank and its HIP device. Any pointer may be NULL.
 * KZGPOT_E_DEVICE once the communicator is aborted. bench.py puts these in its line, so an N-GPU
 * number carries RCCL's own proof of N. */
int kzgpot_comm_size(void* comm, int* nranks, int* rank, int* device);
/* Failure injection (kzgpot_comm_inject_fault, kzgpot_test_inject_host_fault) and the
 * KZGPOT_RCCL_LIB override exist only in the test build libkzgpot_test.so (tests/kzgpot_test_hooks.h); this library binds librccl.so.1. */

/* ---------------------------------------------------------------- misc */
const char* kzgpot_status_name(int status);  /* name of a KZGPOT_ST_* or KZGPOT_E_* code */
int kzgpot_device_count(void);               /* visible HIP devices (0 if none) */
const char* kzgpot_version(void);

#ifdef __cplusplus
}
#endif
#endif /* KZGPOT_H */

// C ABI (include/kzgpot.h): the G1 / G2 group FFT and the phase1radix2m (Lagrange-basis) writer.
// Each transform's scalars come from the host side of csrc/fr.hpp.
#include "accumulator.hpp"
#include "codec.hpp"
#include "device_rt.hpp"
#include "host_rt.hpp"

using namespace kzgpot;

namespace {

constexpr uint32_t kFftFlags = KZGPOT_FFT_INVERSE | KZGPOT_FFT_OUT_PAIRING;

// host_key (optional, prepare_phase2_run's): receives the bad key once the transform is done
int fft_dev(bool g2, const void* d_in, uint32_t exp, void* d_out, uint32_t flags, void* d_work, uint64_t* d_bad_key,
            void* stream, uint64_t* host_key = nullptr) {
  if (exp > 32 || !d_in || !d_out || !d_work || !d_bad_key || (flags & ~kFftFlags)) return KZGPOT_E_INVALID_ARG;
  FftScalars sc;
  fft_scalars(exp, flags & KZGPOT_FFT_INVERSE, sc);
  const hipStream_t s = (hipStream_t)stream;
  return launch_with_key(d_bad_key, s, [&](unsigned long long* key) {
    return launch_group_fft(g2, d_in, exp, d_out, flags & KZGPOT_FFT_INVERSE, flags & KZGPOT_FFT_OUT_PAIRING, sc,
                            d_work, key, s);
  }, host_key);
}

int fft_host(bool g2, const uint8_t* in, uint32_t exp, uint8_t* out, uint32_t flags, int64_t* first_bad) {
  if (first_bad) *first_bad = -1;
  if (exp > 32 || !in || !out || (flags & ~kFftFlags)) return KZGPOT_E_INVALID_ARG;
  const uint64_t bytes = ((uint64_t)1 << exp) * (g2 ? 192 : 96);
  StagedCall call;
  void *io, *work;
  if (call.begin() || call.in(io, in, bytes) || call.alloc(work, fft_workspace_bytes(g2, exp)) || call.key())
    return KZGPOT_E_DEVICE;
  return call.finish(fft_dev(g2, io, exp, io, flags, work, call.d_key, nullptr), first_bad,
                     [&] { return copy_out(out, io, bytes); });
}

// a finite ark-uncompressed record -> pairing uncompressed (A6): every 48-B coordinate byte-reversed,
// G2's c0 / c1 swapped
void ark_to_pairing(uint8_t* dst, const uint8_t* ark, bool g2) {
  const int nc = g2 ? 4 : 2;
  for (int c = 0; c < nc; c++) {
    const uint8_t* src = ark + 48 * (g2 ? (c ^ 1) : c);
    for (int b = 0; b < 48; b++) dst[48 * c + b] = src[47 - b];
  }
}

// powersoftau's verifier, the part that writes phase1radix2m{exp}: checked decode of the five
// slices, then alpha, beta_g1, beta_g2, the four inverse FFTs and the H bases, pairing-uncompressed
int prepare_phase2_run(const uint8_t* tr, uint32_t n_log2, uint32_t exp, uint8_t* out, int* bad_section,
                       int64_t* bad_index) {
  if (device_count() <= 0) return KZGPOT_E_DEVICE;
  DeviceGuard guard;
  const uint64_t m = 1ull << exp;
  const Accumulator in_file(1ull << n_log2), use(m);  // the first `use` points of each section are read
  hipStream_t s = nullptr;
  DevBuf comp, dec[Accumulator::kSections], tmp, work, key;
  if (comp.alloc(use.cnt[0] * 96) || tmp.alloc(m * 192) || work.alloc(fft_workspace_bytes(true, exp)) ||
      key.alloc(sizeof(uint64_t)))
    return KZGPOT_E_DEVICE;
  for (int sec = 0; sec < Accumulator::kSections; sec++) {
    const CodecOp op = Accumulator::g2(sec) ? CodecOp::G2Decompress : CodecOp::G1Decompress;
    const uint64_t rin = in_record(op), rout = out_record(op), cnt = use.cnt[sec];
    if (dec[sec].alloc(cnt * rout)) return KZGPOT_E_DEVICE;
    HIP_TRY(hipMemcpy(comp.p, tr + in_file.offset(sec), cnt * rin, hipMemcpyHostToDevice));
    uint64_t k;
    const int r = launch_with_key((uint64_t*)key.p, s, [&](unsigned long long* d_key) {
      return launch_codec(op, comp.p, dec[sec].p, cnt, 0, d_key, nullptr, s);
    }, &k);
    if (r) return r;
    if (k != kNoBad) {
      if (bad_section) *bad_section = sec;
      return decode_key(k, bad_index);
    }
  }
  uint8_t head[192];
  uint8_t* o = out;
  for (int sec = 2; sec < 5; sec++) {  // alpha = alpha tau^0 G1, beta_g1, beta_g2
    const size_t rec = Accumulator::g2(sec) ? 192 : 96;
    HIP_TRY(hipMemcpy(head, dec[sec].p, rec, hipMemcpyDeviceToHost));
    ark_to_pairing(o, head, Accumulator::g2(sec));
    o += rec;
  }
  uint8_t* const h_out = o + m * (3 * 96 + 192);
  HIP_TRY(launch_h_bases(dec[0].p, m, tmp.p, s));
  HIP_TRY(hipMemcpy(h_out, tmp.p, (m - 1) * 96, hipMemcpyDeviceToHost));
  for (int sec = 0; sec < 4; sec++) {  // coeffs_g1, coeffs_g2, alpha_coeffs_g1, beta_coeffs_g1
    const size_t bytes = m * (Accumulator::g2(sec) ? 192 : 96);
    uint64_t k;
    if (const int r = fft_dev(Accumulator::g2(sec), dec[sec].p, exp, tmp.p, kFftFlags, work.p, (uint64_t*)key.p, s, &k))
      return r;
    if (k != kNoBad) return KZGPOT_E_DEVICE;  // the records are the codec's own output
    HIP_TRY(hipMemcpy(o, tmp.p, bytes, hipMemcpyDeviceToHost));
    o += bytes;
  }
  return 0;
}

int prepare_phase2_args(const void* a, const void* b, uint32_t n_log2, uint32_t exp, int* bad_section,
                        int64_t* bad_index) {
  reset_bad(bad_section, bad_index);
  if (!a || !b || n_log2 < 1 || n_log2 > 30 || exp > n_log2) return KZGPOT_E_INVALID_ARG;
  return 0;
}

}  // namespace

extern "C" {

/* host only */
int kzgpot_fr_domain_root(uint32_t exp, uint8_t root_be32[32]) {
  if (exp > 32 || !root_be32) return KZGPOT_E_INVALID_ARG;
  return api_guard([&] {
    fr_to_be32(root_be32, fr_domain_root(exp));
    return 0;
  });
}
uint64_t kzgpot_group_fft_workspace(int g2, uint32_t exp) { return exp > 32 ? 0 : fft_workspace_bytes(g2 != 0, exp); }
int kzgpot_g1_fft_dev(const void* d_in, uint32_t exp, void* d_out, uint32_t flags, void* d_work, uint64_t* d_bad_key,
                      void* stream) {
  return api_guard([&] { return fft_dev(false, d_in, exp, d_out, flags, d_work, d_bad_key, stream); });
}
int kzgpot_g2_fft_dev(const void* d_in, uint32_t exp, void* d_out, uint32_t flags, void* d_work, uint64_t* d_bad_key,
                      void* stream) {
  return api_guard([&] { return fft_dev(true, d_in, exp, d_out, flags, d_work, d_bad_key, stream); });
}
int kzgpot_g1_fft(const uint8_t* in, uint32_t exp, uint8_t* out, uint32_t flags, int64_t* first_bad) {
  return api_guard([&] { return fft_host(false, in, exp, out, flags, first_bad); });
}
int kzgpot_g2_fft(const uint8_t* in, uint32_t exp, uint8_t* out, uint32_t flags, int64_t* first_bad) {
  return api_guard([&] { return fft_host(true, in, exp, out, flags, first_bad); });
}

uint64_t kzgpot_phase1radix_size(uint32_t exp) {
  if (exp > 30) return 0;
  return kzgpot_phase1_size(exp) + ((1ull << exp) - 1) * 96;
}
int kzgpot_prepare_phase2_buffer(const uint8_t* transcript, size_t len, uint32_t n_log2, uint32_t exp, uint8_t* out,
                                 int* bad_section, int64_t* bad_index) {
  if (const int r = prepare_phase2_args(transcript, out, n_log2, exp, bad_section, bad_index)) return r;
  if (len != kzgpot_contribution_size(n_log2)) return KZGPOT_E_SIZE;
  return api_guard([&] { return prepare_phase2_run(transcript, n_log2, exp, out, bad_section, bad_index); });
}
int kzgpot_prepare_phase2(const char* transcript_path, const char* out_path, uint32_t n_log2, uint32_t exp,
                          int* bad_section, int64_t* bad_index) {
  if (const int r = prepare_phase2_args(transcript_path, out_path, n_log2, exp, bad_section, bad_index)) return r;
  return api_guard([&]() -> int {
    std::vector<uint8_t> tr;
    if (const int r = read_file(transcript_path, tr, kzgpot_contribution_size(n_log2))) return r;
    std::vector<uint8_t> out(kzgpot_phase1radix_size(exp));
    if (const int r = prepare_phase2_run(tr.data(), n_log2, exp, out.data(), bad_section, bad_index)) return r;
    // the temporary exists only once the whole file is computed
    TempOutput tmp(out_path);
    if (tmp.fd() < 0 || !pwrite_all(tmp.fd(), out.data(), out.size(), 0) || !tmp.commit()) return KZGPOT_E_IO;
    return 0;
  });
}

}  // extern "C"

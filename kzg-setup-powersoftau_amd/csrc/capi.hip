// C ABI (include/kzgpot.h): host-buffer and device-buffer entry points for the point codec and the
// setup loaders, over run_host's two-slot staging pipeline. The kgz / fastkzg file pipeline is in
// preprocess.hip, the group FFT and the phase1radix2m writer in phase2.hip. No CPU fallback exists:
// without a GPU every entry point returns KZGPOT_E_DEVICE.
#include "accumulator.hpp"
#include "chunk_plan.hpp"  // ChunkPlan: the chunks of a host-buffer call
#include "device_rt.hpp"
#include "run_host.hpp"

using namespace kzgpot;

namespace {

// Per-device staging for the host-buffer API (grown on demand, reused across calls): two slots,
// each with its own stream, so chunk k's kernel runs while the host thread moves chunk k-1's
// output back and chunk k+1's input in (run_host).
struct Slot {
  hipStream_t stream = nullptr;
  void* d_in = nullptr;
  void* d_out = nullptr;
  uint8_t* d_status = nullptr;
  uint64_t* d_key = nullptr;
  uint64_t h_key = kNoBad;  // where the chunk's key is copied back to: outlives any frame that queues the copy
  size_t cap_in = 0, cap_out = 0, cap_status = 0;
};
struct DevCtx {
  std::mutex mu;
  Slot slot[2];
};
DevCtx g_ctx[64];

int ensure(void** p, size_t* cap, size_t need) {
  if (*cap >= need) return 0;
  if (*p) HIP_TRY(hipFree(*p));
  *p = nullptr;
  *cap = 0;
  HIP_TRY(hipMalloc(p, need));
  *cap = need;
  return 0;
}

// Leaves no copy or kernel of a run_host call in flight on the slots (they are reused, and the
// copies target the caller's buffers): waits for both streams on every exit but the successful
// one, where the last drain already has.
struct QuiesceOnExit {
  DevCtx& c;
  bool idle = false;
  ~QuiesceOnExit() {
    if (idle) return;
    for (Slot& sl : c.slot)
      if (sl.stream) (void)hipStreamSynchronize(sl.stream);
  }
};

int run_dev(CodecOp op, const void* d_in, size_t n, void* d_out, uint32_t flags, uint64_t* d_bad_key,
            uint8_t* d_status, void* stream) {
  if (!d_bad_key) return KZGPOT_E_INVALID_ARG;
  if (n && (!d_in || !d_out)) return KZGPOT_E_INVALID_ARG;
  const hipStream_t s = (hipStream_t)stream;
  return launch_with_key(d_bad_key, s, [&](unsigned long long* key) {
    return launch_codec(op, d_in, d_out, n, flags, key, d_status, s);
  });
}

int run_host_status(CodecOp op, const uint8_t* in, size_t n, uint8_t* out, uint32_t flags, int64_t* first_bad,
                    uint8_t* status) {
  return api_guard([&] {
    HostRunOpts o;
    o.status = status;
    return run_host(current_device(), op, in, n, out, flags, first_bad, o);
  });
}

// One sequential pass over a setup file: each section is `count` ark-uncompressed points read
// with deserialize_unchecked into `dst`. Mirrors the reference's BufReader loop (no size check
// beyond "enough bytes").
struct LoadSection {
  CodecOp op;
  uint64_t count;
  uint8_t* dst;
  int section;  // reported in *bad_section
};
int load_sections(const uint8_t* file, size_t len, const LoadSection* secs, int nsec, int* bad_section,
                  int64_t* bad_index) {
  reset_bad(bad_section, bad_index);
  if (!file) return KZGPOT_E_INVALID_ARG;
  uint64_t need = 0;
  for (int k = 0; k < nsec; k++) {
    if (!secs[k].dst) return KZGPOT_E_INVALID_ARG;
    need += secs[k].count * in_record(secs[k].op);
  }
  if (len < need) return KZGPOT_E_SIZE;
  if (device_count() <= 0) return KZGPOT_E_DEVICE;
  const uint8_t* p = file;
  for (int k = 0; k < nsec; k++) {
    int64_t fb = -1;
    const int r = run_host(current_device(), secs[k].op, p, secs[k].count, secs[k].dst, 0, &fb);
    if (r) {
      if (bad_section) *bad_section = secs[k].section;
      if (bad_index) *bad_index = fb;
      return r;
    }
    p += secs[k].count * in_record(secs[k].op);
  }
  return 0;
}

}  // namespace

// Run one op over host buffers on device `dev`, in chunks that bound the staging memory. Chunks
// alternate between two slots/streams: while the GPU decodes chunk k, this thread copies chunk
// k-1's output out and chunk k+1's input in (pageable copies block the host, not the other
// stream), so PCIe time hides behind the kernels except for the first input and last output.
// On any error exit no work of this call is left in flight (QuiesceOnExit).
int kzgpot::run_host(int dev, CodecOp op, const uint8_t* in, size_t n, uint8_t* out, uint32_t flags, int64_t* first_bad,
                     const HostRunOpts& opts) {
  const auto on_chunk = opts.on_chunk;
  const bool keep_out = opts.keep_out;
  uint8_t* const status = opts.status;
  if (first_bad) *first_bad = -1;
  if (n == 0) return 0;
  if (!in || (keep_out && !out)) return KZGPOT_E_INVALID_ARG;
  if (dev < 0 || dev >= device_count() || dev >= 64) return KZGPOT_E_DEVICE;
  DevCtx& c = g_ctx[dev];
  std::lock_guard<std::mutex> lock(c.mu);
  DeviceGuard guard;
  HIP_TRY(hipSetDevice(dev));
  const uint64_t rin = in_record(op), rout = out_record(op);
  // 2 x 2^21 x 288 B of staging at most. A call of up to 2^24 points is cut into at least 8 chunks
  // so that its PCIe copies overlap its kernels (2^20 G2 points in one chunk: 31 % over the
  // device-resident time, profiles/r04a_bench_n1.json); longer calls ramp their chunk sizes up and
  // down (ChunkPlan). A streaming consumer (on_chunk: the output digest of the e2e pipeline) can
  // only start on the first chunk's records, so an equal-chunk call gives it a 2^16-point first chunk.
  const ChunkPlan plan(n, on_chunk != nullptr);
  const size_t chunk = plan.max_chunk(), nchunks = plan.count();
  QuiesceOnExit quiesce{c};
  for (int k = 0; k < (nchunks > 1 ? 2 : 1); k++) {
    Slot& sl = c.slot[k];
    if (!sl.stream) HIP_TRY(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
    if (ensure(&sl.d_in, &sl.cap_in, chunk * rin)) return KZGPOT_E_DEVICE;
    if (ensure(&sl.d_out, &sl.cap_out, chunk * rout)) return KZGPOT_E_DEVICE;
    if (status && ensure((void**)&sl.d_status, &sl.cap_status, chunk)) return KZGPOT_E_DEVICE;
    if (!sl.d_key) HIP_TRY(hipMalloc(&sl.d_key, sizeof(uint64_t)));
  }
  uint64_t best = kNoBad;
  // drain chunk j: its output (and status, key) back to the host
  auto drain = [&](size_t j) -> int {
    TraceRange tr_("kzgpot.d2h");  // waits for chunk j's kernel, then its output copy
    Slot& sl = c.slot[j & 1];
    size_t off, m;
    plan.span(j, off, m);
    if (keep_out) HIP_TRY(hipMemcpyAsync(out + off * rout, sl.d_out, m * rout, hipMemcpyDeviceToHost, sl.stream));
    if (status) HIP_TRY(hipMemcpyAsync(status + off, sl.d_status, m, hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipMemcpyAsync(&sl.h_key, sl.d_key, sizeof sl.h_key, hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipStreamSynchronize(sl.stream));
    const uint64_t key = sl.h_key;
    if (key != kNoBad && best == kNoBad) best = ((uint64_t)(key >> 8) + off) << 8 | (key & 0xff);
    if (on_chunk && best == kNoBad) {
      TraceRange tc_("kzgpot.handoff");
      try {
        (*on_chunk)(off, m);
      } catch (...) {  // the consumer could not queue the range (std::bad_alloc)
        return KZGPOT_E_OUT_OF_MEMORY;
      }
    }
    return 0;
  };
  for (size_t j = 0; j < nchunks; j++) {
    Slot& sl = c.slot[j & 1];
    size_t off, m;
    plan.span(j, off, m);
    if (opts.in_wait) {
      TraceRange tw_("kzgpot.wait_input");  // the transcript still streaming in from disk
      if (!(*opts.in_wait)(in + (off + m) * rin)) return KZGPOT_E_IO;  // the transcript read failed
    }
    {
      TraceRange th_("kzgpot.h2d");  // a pageable copy: the host thread stages it
      HIP_TRY(hipMemcpyAsync(sl.d_in, in + off * rin, m * rin, hipMemcpyHostToDevice, sl.stream));
    }
    const int launched = launch_with_key(sl.d_key, sl.stream, [&](unsigned long long* key) {
      return launch_codec(op, sl.d_in, sl.d_out, m, flags, key, status ? sl.d_status : nullptr, sl.stream);
    });
    if (launched) return launched;
    if (j > 0)
      if (const int r = drain(j - 1)) return r;  // chunks finish in order: best stays the first
  }
  if (const int r = drain(nchunks - 1)) return r;
  // both streams are idle: chunk nchunks - 2 was drained before, chunk nchunks - 1 just now
  quiesce.idle = true;
  return decode_key(best, first_bad);
}

extern "C" {

int kzgpot_g1_decompress_ex(const uint8_t* in, size_t n, uint8_t* out, uint32_t flags, int64_t* first_bad,
                            uint8_t* status) {
  return run_host_status(CodecOp::G1Decompress, in, n, out, flags, first_bad, status);
}
int kzgpot_g2_decompress_ex(const uint8_t* in, size_t n, uint8_t* out, uint32_t flags, int64_t* first_bad,
                            uint8_t* status) {
  return run_host_status(CodecOp::G2Decompress, in, n, out, flags, first_bad, status);
}
int kzgpot_g1_transcode_uncompressed_ex(const uint8_t* in, size_t n, uint8_t* out, uint32_t flags,
                                        int64_t* first_bad, uint8_t* status) {
  return run_host_status(CodecOp::G1Transcode, in, n, out, flags & KZGPOT_SUBGROUP_REF, first_bad, status);
}
int kzgpot_g2_transcode_uncompressed_ex(const uint8_t* in, size_t n, uint8_t* out, uint32_t flags,
                                        int64_t* first_bad, uint8_t* status) {
  return run_host_status(CodecOp::G2Transcode, in, n, out, flags & KZGPOT_SUBGROUP_REF, first_bad, status);
}
int kzgpot_g1_decompress(const uint8_t* in, size_t n, uint8_t* out, uint32_t flags, int64_t* first_bad) {
  return kzgpot_g1_decompress_ex(in, n, out, flags, first_bad, nullptr);
}
int kzgpot_g2_decompress(const uint8_t* in, size_t n, uint8_t* out, uint32_t flags, int64_t* first_bad) {
  return kzgpot_g2_decompress_ex(in, n, out, flags, first_bad, nullptr);
}
int kzgpot_g1_transcode_uncompressed(const uint8_t* in, size_t n, uint8_t* out, uint32_t flags,
                                     int64_t* first_bad) {
  return kzgpot_g1_transcode_uncompressed_ex(in, n, out, flags, first_bad, nullptr);
}
int kzgpot_g2_transcode_uncompressed(const uint8_t* in, size_t n, uint8_t* out, uint32_t flags,
                                     int64_t* first_bad) {
  return kzgpot_g2_transcode_uncompressed_ex(in, n, out, flags, first_bad, nullptr);
}

int kzgpot_g1_decompress_dev(const void* d_in, size_t n, void* d_out, uint32_t flags, uint64_t* d_bad_key,
                             uint8_t* d_status, void* stream) {
  return run_dev(CodecOp::G1Decompress, d_in, n, d_out, flags, d_bad_key, d_status, stream);
}
int kzgpot_g2_decompress_dev(const void* d_in, size_t n, void* d_out, uint32_t flags, uint64_t* d_bad_key,
                             uint8_t* d_status, void* stream) {
  return run_dev(CodecOp::G2Decompress, d_in, n, d_out, flags, d_bad_key, d_status, stream);
}
int kzgpot_g1_transcode_uncompressed_dev(const void* d_in, size_t n, void* d_out, uint32_t flags,
                                         uint64_t* d_bad_key, uint8_t* d_status, void* stream) {
  return run_dev(CodecOp::G1Transcode, d_in, n, d_out, flags & KZGPOT_SUBGROUP_REF, d_bad_key, d_status, stream);
}
int kzgpot_g2_transcode_uncompressed_dev(const void* d_in, size_t n, void* d_out, uint32_t flags,
                                         uint64_t* d_bad_key, uint8_t* d_status, void* stream) {
  return run_dev(CodecOp::G2Transcode, d_in, n, d_out, flags & KZGPOT_SUBGROUP_REF, d_bad_key, d_status, stream);
}
int kzgpot_decode_bad_key(uint64_t key, int64_t* first_bad) { return decode_key(key, first_bad); }

// ------------------------------------------------------------------------------- loader mirror
int kzgpot_g1_deserialize_unchecked_ex(const uint8_t* in, size_t n, uint8_t* out, int64_t* first_bad,
                                       uint8_t* status) {
  return run_host_status(CodecOp::G1Load, in, n, out, 0, first_bad, status);
}
int kzgpot_g2_deserialize_unchecked_ex(const uint8_t* in, size_t n, uint8_t* out, int64_t* first_bad,
                                       uint8_t* status) {
  return run_host_status(CodecOp::G2Load, in, n, out, 0, first_bad, status);
}
int kzgpot_g1_deserialize_unchecked(const uint8_t* in, size_t n, uint8_t* out, int64_t* first_bad) {
  return kzgpot_g1_deserialize_unchecked_ex(in, n, out, first_bad, nullptr);
}
int kzgpot_g2_deserialize_unchecked(const uint8_t* in, size_t n, uint8_t* out, int64_t* first_bad) {
  return kzgpot_g2_deserialize_unchecked_ex(in, n, out, first_bad, nullptr);
}
int kzgpot_g1_deserialize_unchecked_dev(const void* d_in, size_t n, void* d_out, uint64_t* d_bad_key,
                                        uint8_t* d_status, void* stream) {
  return run_dev(CodecOp::G1Load, d_in, n, d_out, 0, d_bad_key, d_status, stream);
}
int kzgpot_g2_deserialize_unchecked_dev(const void* d_in, size_t n, void* d_out, uint64_t* d_bad_key,
                                        uint8_t* d_status, void* stream) {
  return run_dev(CodecOp::G2Load, d_in, n, d_out, 0, d_bad_key, d_status, stream);
}
int kzgpot_bn254_g1_decompress_ex(const uint8_t* in, size_t n, uint8_t* out, int64_t* first_bad, uint8_t* status) {
  return run_host_status(CodecOp::Bn254G1Decompress, in, n, out, 0, first_bad, status);
}
int kzgpot_bn254_g1_decompress(const uint8_t* in, size_t n, uint8_t* out, int64_t* first_bad) {
  return kzgpot_bn254_g1_decompress_ex(in, n, out, first_bad, nullptr);
}
int kzgpot_bn254_g1_decompress_dev(const void* d_in, size_t n, void* d_out, uint64_t* d_bad_key, uint8_t* d_status,
                                   void* stream) {
  return run_dev(CodecOp::Bn254G1Decompress, d_in, n, d_out, 0, d_bad_key, d_status, stream);
}

int kzgpot_load_kzg_setup_buffer(const uint8_t* file, size_t len, uint32_t n_log2, uint8_t* powers_of_g,
                                 uint8_t* powers_of_gamma_g, uint8_t* vk, int* bad_section, int64_t* bad_index) {
  if (n_log2 > 30 || !vk) return KZGPOT_E_INVALID_ARG;
  const uint64_t n = 1ull << n_log2;
  const uint64_t g1 = KZGPOT_G1_ARK_MONT_BYTES;
  const LoadSection secs[] = {
      {CodecOp::G1Load, tau_powers_g1_length(n), powers_of_g, 0},  // TAU_POWERS_G1_LENGTH (src/lib.rs:179-181)
      {CodecOp::G1Load, n, powers_of_gamma_g, 1},                  // TAU_POWERS_LENGTH (src/lib.rs:182-184)
      {CodecOp::G1Load, 2, vk, 2},                                 // VerifierKey g, gamma_g
      {CodecOp::G2Load, 2, vk + 2 * g1, 2},                        // VerifierKey h, beta_h
  };
  return api_guard([&] { return load_sections(file, len, secs, 4, bad_section, bad_index); });
}
int kzgpot_load_kzg_setup(const char* path, uint32_t n_log2, uint8_t* powers_of_g, uint8_t* powers_of_gamma_g,
                          uint8_t* vk, int* bad_section, int64_t* bad_index) {
  return api_guard([&] {
    std::vector<uint8_t> buf;
    const int r = read_file(path, buf);
    if (r) return r;
    return kzgpot_load_kzg_setup_buffer(buf.data(), buf.size(), n_log2, powers_of_g, powers_of_gamma_g, vk,
                                        bad_section, bad_index);
  });
}
uint64_t kzgpot_phase1_size(uint32_t exp) {
  if (exp > 30) return 0;
  const uint64_t m = 1ull << exp;
  return 2 * 96 + 192 + m * (3 * 96 + 192);
}
int kzgpot_load_phase1_buffer(const uint8_t* file, size_t len, uint32_t exp, uint8_t* alpha, uint8_t* beta_g1,
                              uint8_t* beta_g2, uint8_t* coeffs_g1, uint8_t* coeffs_g2, uint8_t* alpha_coeffs_g1,
                              uint8_t* beta_coeffs_g1, int* bad_section, int64_t* bad_index) {
  if (exp > 30) return KZGPOT_E_INVALID_ARG;
  const uint64_t m = 1ull << exp;
  const LoadSection secs[] = {
      {CodecOp::G1Phase1, 1, alpha, 0},            // src/lib.rs:92
      {CodecOp::G1Phase1, 1, beta_g1, 1},          // src/lib.rs:93
      {CodecOp::G2Phase1, 1, beta_g2, 2},          // src/lib.rs:94
      {CodecOp::G1Phase1, m, coeffs_g1, 3},        // src/lib.rs:95-98
      {CodecOp::G2Phase1, m, coeffs_g2, 4},        // src/lib.rs:99-102
      {CodecOp::G1Phase1, m, alpha_coeffs_g1, 5},  // src/lib.rs:103-106
      {CodecOp::G1Phase1, m, beta_coeffs_g1, 6},   // src/lib.rs:107-110
  };
  return api_guard([&] { return load_sections(file, len, secs, 7, bad_section, bad_index); });
}
int kzgpot_load_phase1(const char* path, uint32_t exp, uint8_t* alpha, uint8_t* beta_g1, uint8_t* beta_g2,
                       uint8_t* coeffs_g1, uint8_t* coeffs_g2, uint8_t* alpha_coeffs_g1, uint8_t* beta_coeffs_g1,
                       int* bad_section, int64_t* bad_index) {
  return api_guard([&] {
    std::vector<uint8_t> buf;
    const int r = read_file(path, buf);
    if (r) return r;
    return kzgpot_load_phase1_buffer(buf.data(), buf.size(), exp, alpha, beta_g1, beta_g2, coeffs_g1, coeffs_g2,
                                     alpha_coeffs_g1, beta_coeffs_g1, bad_section, bad_index);
  });
}
int kzgpot_load_fastkzg_setup_buffer(const uint8_t* file, size_t len, uint32_t n_log2, uint8_t* powers_of_g,
                                     uint8_t* powers_of_gamma_g, uint8_t* h_beta_h, uint8_t* powers_of_h,
                                     int* bad_section, int64_t* bad_index) {
  if (n_log2 > 30) return KZGPOT_E_INVALID_ARG;
  const uint64_t n = 1ull << n_log2;
  const LoadSection secs[] = {
      {CodecOp::G1Load, tau_powers_g1_length(n), powers_of_g, 0},  // src/lib.rs:204-206
      {CodecOp::G1Load, n, powers_of_gamma_g, 1},                  // src/lib.rs:207-209 (BTreeMap keys 0..N-1)
      {CodecOp::G2Load, 2, h_beta_h, 2},                           // h, beta_h (src/lib.rs:211-212)
      {CodecOp::G2Load, n, powers_of_h, 3},                        // src/lib.rs:214-217
  };
  return api_guard([&] { return load_sections(file, len, secs, 4, bad_section, bad_index); });
}
int kzgpot_load_fastkzg_setup(const char* path, uint32_t n_log2, uint8_t* powers_of_g, uint8_t* powers_of_gamma_g,
                              uint8_t* h_beta_h, uint8_t* powers_of_h, int* bad_section, int64_t* bad_index) {
  return api_guard([&] {
    std::vector<uint8_t> buf;
    const int r = read_file(path, buf);
    if (r) return r;
    return kzgpot_load_fastkzg_setup_buffer(buf.data(), buf.size(), n_log2, powers_of_g, powers_of_gamma_g,
                                            h_beta_h, powers_of_h, bad_section, bad_index);
  });
}

const char* kzgpot_status_name(int s) {
  switch (s < 0 && s > -100 ? -s : s) {
    case KZGPOT_OK: return "ok";
    case KZGPOT_ST_COMPRESSION_MODE: return "UnexpectedCompressionMode";
    case KZGPOT_ST_UNEXPECTED_INFO: return "UnexpectedInformation";
    case KZGPOT_ST_NOT_IN_FIELD: return "NotInField";
    case KZGPOT_ST_NOT_ON_CURVE: return "NotOnCurve";
    case KZGPOT_ST_NOT_IN_SUBGROUP: return "NotInSubgroup";
    case KZGPOT_ST_UNEXPECTED_FLAGS: return "UnexpectedFlags";
    case KZGPOT_ST_INFINITY: return "Infinity";
    case KZGPOT_E_INVALID_ARG: return "InvalidArgument";
    case KZGPOT_E_DEVICE: return "DeviceError";
    case KZGPOT_E_IO: return "IoError";
    case KZGPOT_E_SIZE: return "SizeMismatch";
    case KZGPOT_E_DIGEST: return "DigestMismatch";
    case KZGPOT_E_NETWORK: return "NetworkUnavailable";
    case KZGPOT_E_RANK_FAILED: return "RankFailed";
    case KZGPOT_E_TIMEOUT: return "Timeout";
    case KZGPOT_E_OUT_OF_MEMORY: return "OutOfMemory";
    default: return "unknown";
  }
}
int kzgpot_device_count(void) { return device_count(); }
const char* kzgpot_version(void) { return "kzgpot 0.1.0 (gfx950)"; }

#ifdef KZGPOT_TEST_HOOKS
// test build only (tests/kzgpot_test_hooks.h)
// The chunk plan of a host-buffer call of n points (run_host): writes up to cap (offset, count)
// pairs and returns the number of chunks (tests/test_host.py checks the tiling on the CPU).
long kzgpot_test_chunk_plan(uint64_t n, int streaming_consumer, uint64_t* spans, long cap) {
  if (n == 0) return 0;
  const ChunkPlan plan((size_t)n, streaming_consumer != 0);
  const long k = (long)plan.count();
  for (long j = 0; j < k && j < cap; j++) {
    size_t off, m;
    plan.span((size_t)j, off, m);
    spans[2 * j] = off;
    spans[2 * j + 1] = m;
  }
  return k;
}
int kzgpot_test_inject_host_fault(int site, long skip) {
  if (site < 0 || site > kFaultHostBuf || skip < 0) return KZGPOT_E_INVALID_ARG;
  inject_fault(site, skip);
  return 0;
}
#endif

}  // extern "C"

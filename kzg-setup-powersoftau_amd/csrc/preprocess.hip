// C ABI (include/kzgpot.h): the kgz / fastkzg file pipeline — kzgpot_preprocess[_buffer][_ex], its
// two size functions and kzgpot_blake2b. The host machinery it runs on is in host_rt.hpp; the
// decode of every section goes through run_host (capi.hip).
#include <string.h>
#include <strings.h>

#include "accumulator.hpp"
#include "blake2b.hpp"
#include "device_rt.hpp"
#include "run_host.hpp"

using namespace kzgpot;

namespace {

// Where the transcript comes from and where the output goes, besides the two buffers.
struct PipelineIo {
  Watermark* in_wm = nullptr;  // non-null: the transcript is still being read from disk
  int out_fd = -1;             // >= 0: output ranges are written here (file order offsets) as they land
};

int preprocess_run(const uint8_t* tr, size_t len, uint8_t* out, int mode, uint32_t n_log2, int n_shards,
                   const char* expect_in_hex, char* in_hex, char* out_hex, int* bad_section, int64_t* bad_index,
                   const PipelineIo& io) {
  // transcript digest (download_parameters' check, preprocess-kgz.rs:51-61) beside the GPU pass;
  // a transcript still streaming from disk is hashed as it arrives. It is the call's critical path
  // (one sequential BLAKE2b stream), so it starts before anything touches HIP: in a fresh process
  // (the CLI drop-ins) the runtime's initialisation then overlaps it instead of preceding it.
  uint8_t in_digest[64];
  bool in_ok = true;
  std::atomic<bool> abandon{false};  // set when the call fails: the hasher stops at its next piece
  std::thread in_hash;
  JoinOnExit in_hash_join{in_hash, [&abandon] { abandon = true; }};  // any early exit
  const bool want_in = expect_in_hex || in_hex;
  TraceRange call_("kzgpot.preprocess");
  if (want_in && !start_thread(in_hash, [&] {
        try {
          trace_thread("kzgpot.blake2b.transcript");
          TraceRange tr_("kzgpot.blake2b.transcript");
          Blake2b h;
          for (size_t off = 0; off < len;) {
            const size_t m = std::min<size_t>(len - off, (size_t)32 << 20);
            if (abandon.load(std::memory_order_relaxed) || (io.in_wm && !io.in_wm->wait(off + m))) {
              in_ok = false;
              return;
            }
            h.update(tr + off, m);
            off += m;
          }
          h.finalize(in_digest);
        } catch (...) {
          in_ok = false;
        }
      }))
    return KZGPOT_E_OUT_OF_MEMORY;
  const int ndev = device_count();
  if (ndev <= 0) return KZGPOT_E_DEVICE;
  if (n_shards <= 0) n_shards = ndev;
  n_shards = std::min(n_shards, 64);
  int dev0 = current_device();
  if (dev0 < 0 || dev0 >= ndev) dev0 = 0;
  const uint64_t n = 1ull << n_log2;
  const InputWait in_wait{io.in_wm, tr};
  // output consumers, fed the file's byte ranges in file order
  Blake2b out_h;
  std::unique_ptr<OrderedWorker> out_hash, out_write;
  if (out_hex) {
    out_hash.reset(new OrderedWorker("kzgpot.blake2b.output", [&](const uint8_t* p, size_t m) {
      out_h.update(p, m);
      return true;
    }));
    if (!out_hash->start()) return KZGPOT_E_OUT_OF_MEMORY;
  }
  if (io.out_fd >= 0) {
    out_write.reset(new OrderedWorker(
        "kzgpot.pwrite", [&](const uint8_t* p, size_t m) { return pwrite_all(io.out_fd, p, m, (uint64_t)(p - out)); }));
    if (!out_write->start()) return KZGPOT_E_OUT_OF_MEMORY;
  }
  const bool sink = out_hash || out_write;
  auto push = [&](const uint8_t* p, size_t m) {
    if (out_hash) out_hash->push(p, m);
    if (out_write) out_write->push(p, m);
  };

  const Accumulator acc(n);  // the section order, after the 64-B hash
  // read back by read_g1/read_g2 (checked) in each binary: kgz τG1, τG2, ατG1; fastkgz + βτG1
  const bool checked[5] = {true, true, true, mode == KZGPOT_MODE_FASTKZG, false};
  // output layout (A7): τG1 and ατG1 are decoded straight into their place in `out`; fastkzg's
  // powers_of_h (= τG2) too; sections the file does not hold (kgz τG2 beyond h, beta_h; βτG1;
  // βG2) are decoded and checked on the GPU but never copied back (dst = null)
  const uint64_t off_gamma = acc.cnt[0] * 96, off_tail = off_gamma + n * 96;
  uint8_t* dst[5] = {out, nullptr, out + off_gamma, nullptr, nullptr};
  if (mode == KZGPOT_MODE_FASTKZG) dst[1] = out + off_tail + 2 * 192;
  int ret = 0;
  for (int s = 0; s < Accumulator::kSections && !ret; s++) {
    const CodecOp op = Accumulator::g2(s) ? CodecOp::G2Decompress : CodecOp::G1Decompress;
    const uint64_t rin = in_record(op), rout = out_record(op), cnt = acc.cnt[s];
    const uint8_t* const p = tr + acc.offset(s);
    const uint32_t fl = checked[s] ? 0u : KZGPOT_NO_SUBGROUP_CHECK;
    // contiguous shards, one host thread each
    std::vector<int> rc(n_shards, 0);
    std::vector<int64_t> fb(n_shards, -1);
    const uint64_t per = (cnt + n_shards - 1) / n_shards;
    // The τG1 / ατG1 output (file order) is handed to the digest and writer threads chunk by chunk
    // as it lands, so hashing and writing overlap the GPU pass instead of following it
    // (ShardCursor puts the shards' chunks into file order).
    const bool stream = sink && (s == 0 || s == 2);
    ShardCursor cursor(cnt, per, n_shards);
    {
      // declared after everything the shards use, so it joins them first on any exit
      ThreadGroup th(n_shards);
      for (int g = 0; g < n_shards; g++) {
        const uint64_t lo = std::min(cnt, g * per), hi = std::min(cnt, lo + per);
        const bool started = th.start([&, g, lo, hi] {
          try {
            trace_thread("kzgpot.shard");
            TraceRange tr_(Accumulator::range_name(s));
            const std::function<void(size_t, size_t)> on_chunk = [&, g](size_t off, size_t m) {
              cursor.land(g, off, m, [&](uint64_t first, uint64_t k) { push(dst[s] + first * rout, k * rout); });
            };
            HostRunOpts o;
            o.on_chunk = stream ? &on_chunk : nullptr;
            o.keep_out = dst[s] != nullptr;
            o.in_wait = &in_wait;
            rc[g] = run_host((dev0 + g) % ndev, op, p + lo * rin, hi - lo, dst[s] ? dst[s] + lo * rout : nullptr,
                             fl, &fb[g], o);
          } catch (...) {
            rc[g] = KZGPOT_E_OUT_OF_MEMORY;
          }
          if (fb[g] >= 0) fb[g] += (int64_t)lo;
        });
        if (!started) {  // the shards already running finish their ranges; this one and the rest never run
          for (int k = g; k < n_shards; k++) rc[k] = KZGPOT_E_OUT_OF_MEMORY;
          break;
        }
      }
    }  // joined
    // shards are contiguous and in index order: the first failing shard holds the smallest index
    for (int g = 0; g < n_shards && !ret; g++)
      if (rc[g]) {
        ret = rc[g];
        if (bad_section) *bad_section = s;
        if (bad_index) *bad_index = fb[g];
      }
    if (!ret && stream && !cursor.done()) ret = KZGPOT_E_IO;  // cannot happen: every shard succeeded, so every chunk landed
  }
  uint8_t h_beta_h[2 * 192];  // kgz: τG2[0..1] for the VerifierKey (the section itself was checked)
  if (!ret && mode == KZGPOT_MODE_KZG) {
    int64_t fb2 = -1;
    HostRunOpts o;
    o.in_wait = &in_wait;
    ret = run_host(dev0, CodecOp::G2Decompress, tr + acc.offset(1), 2, h_beta_h, 0, &fb2, o);
  }
  if (!ret) {
    uint8_t* o = out + off_tail;
    const uint8_t* tau_g2 = mode == KZGPOT_MODE_FASTKZG ? dst[1] : h_beta_h;
    if (mode == KZGPOT_MODE_KZG) {  // VerifierKey{g, gamma_g, h, beta_h} (preprocess-kgz.rs:177-194)
      memcpy(o, out, 96);
      memcpy(o + 96, out + off_gamma, 96);
      memcpy(o + 192, tau_g2, 384);
      if (sink) push(o, 576);
    } else {  // h, beta_h, neg_powers_of_h (empty), powers_of_h (preprocess-fastkgz.rs:200-208)
      memcpy(o, tau_g2, 384);
      if (sink) push(o, 384 + n * 192);
    }
  }
  if (out_write && !out_write->finish() && !ret) ret = KZGPOT_E_IO;
  if (out_hash) {
    out_hash->finish();
    if (!ret) {
      uint8_t d[64];
      out_h.finalize(d);
      to_hex(d, out_hex);
    }
  }
  if (want_in) {
    in_hash.join();
    if (!in_ok) {
      if (!ret) ret = KZGPOT_E_IO;
    } else {
      char hex[129];
      to_hex(in_digest, hex);
      if (in_hex) memcpy(in_hex, hex, 129);
      // The reference checks the digest before it decodes anything (download_parameters runs
      // first), so a wrong transcript is reported as such even if it also holds a bad point.
      if (expect_in_hex && strncasecmp(hex, expect_in_hex, 128) != 0) {
        ret = KZGPOT_E_DIGEST;
        reset_bad(bad_section, bad_index);
      }
    }
  }
  return ret;
}

// what both the buffer and the file entry points refuse before they touch anything
bool bad_preprocess_args(int mode, uint32_t n_log2, const char* expect_in_hex) {
  return n_log2 < 1 || n_log2 > 30 || (mode != KZGPOT_MODE_KZG && mode != KZGPOT_MODE_FASTKZG) ||
         (expect_in_hex && !is_hex128(expect_in_hex));
}

// The two `main`s (preprocess-kgz.rs:162-199, preprocess-fastkgz.rs:180-213) minus the download.
// n_shards host threads each decode a contiguous shard of every section; shard g runs on device
// (current + g) % device_count, so n_shards above the device count oversubscribes (the shards of
// one device then run one after another) — which is how the multi-shard path is tested on one GPU.
// Host resources that run out (memory, a thread) end the call with KZGPOT_E_OUT_OF_MEMORY after
// every thread it started has been joined.
int preprocess_impl(const uint8_t* tr, size_t len, uint8_t* out, int mode, uint32_t n_log2, int n_shards,
                    const char* expect_in_hex, char* in_hex, char* out_hex, int* bad_section, int64_t* bad_index,
                    const PipelineIo& io = PipelineIo()) noexcept {
  reset_bad(bad_section, bad_index);
  if (!tr || !out || bad_preprocess_args(mode, n_log2, expect_in_hex)) return KZGPOT_E_INVALID_ARG;
  if (len != kzgpot_contribution_size(n_log2)) return KZGPOT_E_SIZE;
  const int r = api_guard([&] {
    return preprocess_run(tr, len, out, mode, n_log2, n_shards, expect_in_hex, in_hex, out_hex, bad_section,
                          bad_index, io);
  });
  if (r == KZGPOT_E_OUT_OF_MEMORY) reset_bad(bad_section, bad_index);
  return r;
}

Releaser g_release;  // joined when the library is unloaded

}  // namespace

extern "C" {

uint64_t kzgpot_contribution_size(uint32_t n_log2) { return Accumulator(1ull << n_log2).size(); }
uint64_t kzgpot_output_size(uint32_t n_log2, int mode) {
  const uint64_t n = 1ull << n_log2, g1 = (tau_powers_g1_length(n) + n) * 96;  // powers_of_g, powers_of_gamma_g
  return mode == KZGPOT_MODE_FASTKZG ? g1 + 2 * 192 + n * 192 : g1 + 576;
}

int kzgpot_blake2b(const uint8_t* data, size_t len, uint8_t* digest64) {
  if ((!data && len) || !digest64) return KZGPOT_E_INVALID_ARG;
  blake2b_512(data, len, digest64);
  return 0;
}

int kzgpot_preprocess_buffer_ex(const uint8_t* tr, size_t len, uint8_t* out, int mode, uint32_t n_log2,
                                int n_gpus, const char* expect_transcript_digest, char* transcript_digest,
                                char* output_digest, int* bad_section, int64_t* bad_index) {
  return preprocess_impl(tr, len, out, mode, n_log2, n_gpus, expect_transcript_digest, transcript_digest,
                         output_digest, bad_section, bad_index);
}
int kzgpot_preprocess_buffer(const uint8_t* tr, size_t len, uint8_t* out, int mode, uint32_t n_log2, int n_gpus,
                             int* bad_section, int64_t* bad_index) {
  return preprocess_impl(tr, len, out, mode, n_log2, n_gpus, nullptr, nullptr, nullptr, bad_section, bad_index);
}

// File to file, as the reference runs (preprocess-kgz.rs:69-126,187-194): a reader thread streams
// the transcript in 32 MiB pread()s while the GPU decodes what has arrived; a writer thread
// pwrite()s each output range as it lands. The output goes to a temporary file in the same
// directory, renamed over `out_path` only on success (TempOutput).
int kzgpot_preprocess_ex(const char* transcript_path, const char* out_path, int mode, uint32_t n_log2, int n_gpus,
                         const char* expect_transcript_digest, char* transcript_digest, char* output_digest,
                         int* bad_section, int64_t* bad_index) {
  reset_bad(bad_section, bad_index);
  if (!transcript_path || !out_path || bad_preprocess_args(mode, n_log2, expect_transcript_digest))
    return KZGPOT_E_INVALID_ARG;
  TraceRange call_("kzgpot.preprocess_file");
  // Everything the call opens, creates or starts is undone on every exit path, including an
  // exception (std::bad_alloc) caught by api_guard below: the reader is joined, both descriptors
  // closed, and the temporary output removed unless it was renamed over out_path.
  struct InFile {
    int fd = -1;
    ~InFile() {
      if (fd >= 0) close(fd);
    }
  };
  std::unique_ptr<HostBuf> tr, out;
  const int ret = api_guard([&]() -> int {
    InFile f;
    f.fd = open(transcript_path, O_RDONLY | O_CLOEXEC);
    if (f.fd < 0) return KZGPOT_E_IO;
    const off_t flen = lseek(f.fd, 0, SEEK_END);
    if (flen < 0) return KZGPOT_E_IO;
    if ((uint64_t)flen != kzgpot_contribution_size(n_log2)) return KZGPOT_E_SIZE;
    const size_t len = (size_t)flen;
    (void)posix_fadvise(f.fd, 0, flen, POSIX_FADV_SEQUENTIAL);
    tr.reset(new HostBuf(len));
    out.reset(new HostBuf(kzgpot_output_size(n_log2, mode)));
    if (!tr->get() || !out->get()) return KZGPOT_E_OUT_OF_MEMORY;  // the 0.6-1.6 GB mappings
    TempOutput tmp(out_path);
    if (tmp.fd() < 0) return KZGPOT_E_IO;
    Watermark wm;
    std::thread reader;
    JoinOnExit reader_join{reader, [&wm] { wm.fail(); }};  // stops at its next piece, then joined
    uint8_t* const trp = tr->get();
    const int fd = f.fd;
    if (!start_thread(reader, [&wm, trp, fd, len]() noexcept {
          try {
            trace_thread("kzgpot.pread");
          } catch (...) {
          }
          // stops at the next piece once the pipeline failed
          for (size_t off = 0; off < len && !wm.failed();) {
            const ssize_t k = pread(fd, trp + off, std::min<size_t>(len - off, (size_t)32 << 20), (off_t)off);
            if (k < 0 && errno == EINTR) continue;
            if (k <= 0) return wm.fail();
            off += (size_t)k;
            wm.advance(off);
          }
        }))
      return KZGPOT_E_OUT_OF_MEMORY;
    PipelineIo io;
    io.in_wm = &wm;
    io.out_fd = tmp.fd();
    int r = preprocess_impl(trp, len, out->get(), mode, n_log2, n_gpus, expect_transcript_digest, transcript_digest,
                            output_digest, bad_section, bad_index, io);
    if (r) wm.fail();  // the reader finishes its current pread and stops; nothing waits on it
    reader.join();
    TraceRange fin_("kzgpot.file_finish");  // close and rename
    if (!r && !tmp.commit()) r = KZGPOT_E_IO;
    return r;
  });
  if (tr || out) g_release.release(std::move(tr), std::move(out));  // unmapped behind the return (Releaser)
  if (ret == KZGPOT_E_OUT_OF_MEMORY) reset_bad(bad_section, bad_index);
  return ret;
}
int kzgpot_preprocess(const char* transcript_path, const char* out_path, int mode, uint32_t n_log2, int n_gpus,
                      int* bad_section, int64_t* bad_index) {
  return kzgpot_preprocess_ex(transcript_path, out_path, mode, n_log2, n_gpus, nullptr, nullptr, nullptr,
                              bad_section, bad_index);
}

}  // extern "C"

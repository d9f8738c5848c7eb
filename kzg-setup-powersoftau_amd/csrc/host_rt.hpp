// Host runtime of the C ABI units (capi.hip, preprocess.hip, phase2.hip): thread and exception
// plumbing, the ordered consumers of the file pipeline, host buffers and files. Host only: it
// includes no HIP header, so the stand-alone host unit program (tests/host_units) compiles it with
// g++ and runs it under the thread and address sanitizers.
#pragma once
#include <ctype.h>
#include <errno.h>
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/kzgpot.h"
#include "trace.hpp"

namespace kzgpot {

// ---------------------------------------------------------------- host resources at the C ABI
// No exception may cross an extern "C" entry (it would std::terminate the caller's process, where
// the reference returns a Result, preprocess-kgz.rs:105-110). Host threads are started through
// start_thread, which reports a failed start (std::system_error EAGAIN under a process or thread
// limit, std::bad_alloc) as false; every thread body catches its own exceptions; every entry that
// allocates runs under api_guard; and the threads a call started are joined on every exit path
// (JoinOnExit, ThreadGroup) before it returns.

#ifdef KZGPOT_TEST_HOOKS
// Fault injection, test build only (tests/kzgpot_test_hooks.h, kzgpot_test_inject_host_fault):
// from the (skip + 1)-th event of `site` on, every such event fails until the site is cleared.
inline std::atomic<int> g_fault_site{0};
inline std::atomic<long> g_fault_skip{0};
inline bool injected(int site) {
  if (g_fault_site.load() != site) return false;
  return g_fault_skip.fetch_sub(1) <= 0;
}
inline void inject_fault(int site, long skip) {
  g_fault_site = 0;
  g_fault_skip = skip;
  g_fault_site = site;
}
#endif
enum { kFaultThread = 1, kFaultHostBuf = 2 };

template <class F>
bool start_thread(std::thread& t, F&& f) noexcept {
  try {
#ifdef KZGPOT_TEST_HOOKS
    if (injected(kFaultThread)) throw std::system_error(EAGAIN, std::generic_category(), "injected thread fault");
#endif
    t = std::thread(std::forward<F>(f));
    return true;
  } catch (...) {
    return false;
  }
}

template <class F>
int api_guard(F&& f) noexcept {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return KZGPOT_E_OUT_OF_MEMORY;
  } catch (const std::system_error&) {  // a host thread or lock could not be obtained
    return KZGPOT_E_OUT_OF_MEMORY;
  } catch (...) {
    return KZGPOT_E_DEVICE;
  }
}

// "no rejected point": what every entry point with these two outputs starts from
inline void reset_bad(int* bad_section, int64_t* bad_index) {
  if (bad_section) *bad_section = -1;
  if (bad_index) *bad_index = -1;
}

// Joins a thread on scope exit (after running `before`, e.g. telling it to stop), so that an
// early return or an exception never destroys a joinable std::thread.
struct JoinOnExit {
  std::thread& t;
  std::function<void()> before;
  ~JoinOnExit() {
    if (!t.joinable()) return;
    if (before) before();
    t.join();
  }
};

// The shard threads of one section: joined on destruction whatever path leaves the scope.
class ThreadGroup {
 public:
  explicit ThreadGroup(size_t n) { th_.reserve(n); }
  ~ThreadGroup() { join(); }
  template <class F>
  bool start(F&& f) noexcept {
    std::thread t;
    if (!start_thread(t, std::forward<F>(f))) return false;
    th_.push_back(std::move(t));  // no reallocation: reserved
    return true;
  }
  void join() {
    for (auto& t : th_)
      if (t.joinable()) t.join();
  }

 private:
  std::vector<std::thread> th_;
};

// Bytes [0, ready) of a transcript that is still being read from disk are valid; consumers (the
// GPU chunk loop, the transcript hasher) wait for the range they need.
class Watermark {
 public:
  void advance(size_t to) {
    std::lock_guard<std::mutex> l(mu_);
    ready_ = to;
    cv_.notify_all();
  }
  void fail() {
    std::lock_guard<std::mutex> l(mu_);
    failed_ = true;
    cv_.notify_all();
  }
  bool failed() {
    std::lock_guard<std::mutex> l(mu_);
    return failed_;
  }
  // false if the reader failed before `upto` bytes arrived
  bool wait(size_t upto) {
    std::unique_lock<std::mutex> l(mu_);
    cv_.wait(l, [&] { return failed_ || ready_ >= upto; });
    return ready_ >= upto;
  }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  size_t ready_ = 0;
  bool failed_ = false;
};

// Where a run_host input lives while the file is still being read: wait until `end` is readable.
struct InputWait {
  Watermark* wm;
  const uint8_t* base;
  bool operator()(const uint8_t* end) const { return !wm || wm->wait((size_t)(end - base)); }
};

// Consumes byte ranges in submission order on its own thread: the output digest (BLAKE2b is one
// sequential stream) and the output file writer, so both run while the GPU is still decoding
// later sections.
class OrderedWorker {
 public:
  OrderedWorker(const char* name, std::function<bool(const uint8_t*, size_t)> fn)
      : name_(name), fn_(std::move(fn)) {}
  ~OrderedWorker() { finish(); }
  // false if the thread could not be started (the worker is then unusable)
  bool start() { return start_thread(th_, [this] { run(); }); }
  // may throw std::bad_alloc (the queue)
  void push(const uint8_t* p, size_t n) {
    std::lock_guard<std::mutex> l(mu_);
    q_.emplace_back(p, n);
    cv_.notify_one();
  }
  // waits for every pushed range; false if any range failed
  bool finish() {
    {
      std::lock_guard<std::mutex> l(mu_);
      if (done_) return ok_;
      done_ = true;
      cv_.notify_one();
    }
    if (!th_.joinable()) return ok_ = false;
    th_.join();
    return ok_;
  }

 private:
  void run() {
    try {
      trace_thread(name_);
    } catch (...) {
    }
    for (;;) {
      std::pair<const uint8_t*, size_t> item;
      {
        std::unique_lock<std::mutex> l(mu_);
        cv_.wait(l, [this] { return done_ || !q_.empty(); });
        if (q_.empty()) return;
        item = q_.front();
        q_.pop_front();
      }
      try {
        TraceRange tr_(name_);
        if (ok_ && !fn_(item.first, item.second)) ok_ = false;
      } catch (...) {
        ok_ = false;
      }
    }
  }
  const char* name_;
  std::function<bool(const uint8_t*, size_t)> fn_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::pair<const uint8_t*, size_t>> q_;
  bool done_ = false;
  bool ok_ = true;
  std::thread th_;
};

// Re-orders the chunks that the shards of one section land into section order. Shard g owns points
// [g per, (g + 1) per) of `count` and reports its chunks in order; a point goes to the sink once
// every shard before it has landed up to it, so the consumers (the output digest and writer) see
// the file in order at any shard count.
class ShardCursor {
 public:
  ShardCursor(uint64_t count, uint64_t per, int n_shards) : count_(count), per_(per), landed_(n_shards, 0) {}
  // points [off, off + m) of `shard`'s own range are in place; sink(first point, count) gets each
  // newly contiguous range of the section, under the cursor's lock
  template <class Sink>
  void land(int shard, uint64_t off, uint64_t m, Sink&& sink) {
    std::lock_guard<std::mutex> l(mu_);
    landed_[shard] = off + m;
    while (cursor_ < count_) {
      const uint64_t h = cursor_ / per_, avail = h * per_ + landed_[h];
      if (avail <= cursor_) break;
      sink(cursor_, avail - cursor_);
      cursor_ = avail;
    }
  }
  bool done() {  // the whole section went to the sink
    std::lock_guard<std::mutex> l(mu_);
    return cursor_ == count_;
  }

 private:
  const uint64_t count_, per_;
  std::mutex mu_;
  std::vector<uint64_t> landed_;  // shard g: points [g per, g per + landed[g]) are in place
  uint64_t cursor_ = 0;           // section points [0, cursor) have gone to the sink
};

inline bool pwrite_all(int fd, const uint8_t* p, size_t n, uint64_t off) {
  while (n) {
    const ssize_t w = pwrite(fd, p, std::min<size_t>(n, (size_t)1 << 30), (off_t)off);
    if (w < 0 && errno == EINTR) continue;
    if (w <= 0) return false;
    p += w, n -= (size_t)w, off += (uint64_t)w;
  }
  return true;
}

// An output file that appears under its name only when it is whole: written to a temporary beside
// `out_path` (unique per call, so concurrent calls for one out_path never share one), renamed over
// it by commit(), and removed on every other exit (the reference's File::create leaves a truncated
// file behind on a panic).
class TempOutput {
 public:
  explicit TempOutput(const char* out_path) : out_(out_path), tmp_(out_ + ".kzgpot-tmp-XXXXXX") {
    fd_ = mkostemp(&tmp_[0], O_CLOEXEC);
    if (fd_ < 0) return;
    made_ = true;
    (void)fchmod(fd_, 0644);  // mkstemp creates 0600: a setup file is meant to be read by others
  }
  ~TempOutput() {
    if (fd_ >= 0) close(fd_);
    if (made_) unlink(tmp_.c_str());
  }
  TempOutput(const TempOutput&) = delete;
  TempOutput& operator=(const TempOutput&) = delete;
  int fd() const { return fd_; }  // < 0: the temporary could not be created
  // closes the file and renames it over out_path; on false nothing is left behind
  bool commit() {
    if (fd_ < 0) return false;
    const int fd = fd_;
    fd_ = -1;
    if (close(fd) != 0 || rename(tmp_.c_str(), out_.c_str()) != 0) return false;
    made_ = false;
    return true;
  }

 private:
  std::string out_, tmp_;
  int fd_ = -1;
  bool made_ = false;  // the temporary exists under tmp_
};

// A large host buffer of the file path (the 604 MB transcript, the 0.6-1.0 GB output): a 2 MiB
// aligned anonymous mapping with MADV_HUGEPAGE, so faulting it in (pread, the D2H copies) and
// unmapping it at the end costs one fault / one free per 2 MiB instead of per 4 KiB page (with
// transparent huge pages in "madvise" mode; elsewhere it is an ordinary mapping).
class HostBuf {
 public:
  explicit HostBuf(size_t n) {
    constexpr size_t kHuge = (size_t)2 << 20;
    map_ = n + kHuge;
#ifdef KZGPOT_TEST_HOOKS
    void* m = injected(kFaultHostBuf) ? MAP_FAILED
                                      : mmap(nullptr, map_, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
#else
    void* m = mmap(nullptr, map_, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
#endif
    if (m == MAP_FAILED) {
      map_ = 0;
      return;
    }
    base_ = (uint8_t*)m;
    p_ = (uint8_t*)(((uintptr_t)m + kHuge - 1) & ~(uintptr_t)(kHuge - 1));
    (void)madvise(p_, n, MADV_HUGEPAGE);
  }
  ~HostBuf() {
    if (map_) munmap(base_, map_);
  }
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  uint8_t* get() const { return p_; }

 private:
  size_t map_ = 0;
  uint8_t* base_ = nullptr;
  uint8_t* p_ = nullptr;
};

// Unmapping a file call's 1.2-1.6 GB of faulted-in pages takes ~77 ms of kernel time
// (profiles/r04e_e2e_stages.json, after_pipeline_ms) that the caller need not wait for, so it
// runs on a helper thread. At most one release is outstanding when a call returns: the next file
// call joins the previous helper when it hands over its own buffers (by then, ~300 ms into its
// pipeline, the helper has long finished — joining at entry instead cost back-to-back calls up to
// 67 ms, profiles/r05b_e2e_stages.json), so at most two calls' buffers ever coexist, and the
// library's unload joins the last one (the library's one Releaser is destroyed at exit / dlclose),
// so no helper outlives the library's code. The helper calls nothing but munmap (no roctx, no
// HIP). If no thread can be started the buffers are released on the calling thread.
class Releaser {
 public:
  ~Releaser() { join(); }
  void join() {
    std::lock_guard<std::mutex> l(mu_);
    if (th_.joinable()) th_.join();
  }
  void release(std::unique_ptr<HostBuf> a, std::unique_ptr<HostBuf> b) {
    std::lock_guard<std::mutex> l(mu_);
    if (th_.joinable()) th_.join();
    // if no thread starts, the callable (and the buffers it owns) is destroyed with the failed
    // start: released here, on the calling thread
    (void)start_thread(th_, [a = std::move(a), b = std::move(b)]() mutable noexcept {
      a.reset();
      b.reset();
    });
  }

 private:
  std::mutex mu_;
  std::thread th_;
};

// Reads a whole file. `expect`: the length the caller requires, checked before anything is read
// (KZGPOT_E_SIZE); kAnyLength takes the file as it is.
constexpr uint64_t kAnyLength = ~0ull;
inline int read_file(const char* path, std::vector<uint8_t>& buf, uint64_t expect = kAnyLength) {
  if (!path) return KZGPOT_E_INVALID_ARG;
  FILE* f = fopen(path, "rb");
  if (!f) return KZGPOT_E_IO;
  fseek(f, 0, SEEK_END);
  const long len = ftell(f);
  fseek(f, 0, SEEK_SET);
  int r = len < 0 ? KZGPOT_E_IO : (expect != kAnyLength && (uint64_t)len != expect) ? KZGPOT_E_SIZE : 0;
  if (!r) {
    try {
      buf.resize((size_t)len);
      if (fread(buf.data(), 1, buf.size(), f) != buf.size()) r = KZGPOT_E_IO;
    } catch (const std::bad_alloc&) {
      r = KZGPOT_E_OUT_OF_MEMORY;
    }
  }
  fclose(f);
  return r;
}

// 128 hex digits (either case): the form of expect_transcript_digest
inline bool is_hex128(const char* s) {
  for (int i = 0; i < 128; i++)
    if (!isxdigit((unsigned char)s[i])) return false;
  return s[128] == '\0';
}

}  // namespace kzgpot

// Stand-alone checks of the library's host machinery (csrc/host_rt.hpp, csrc/chunk_plan.hpp): no
// GPU, no HIP header. tests/test_host_units.py builds it plain, with -fsanitize=thread and with
// -fsanitize=address,undefined, and runs each binary; exit 0 and no sanitizer report is a pass.
#include <dirent.h>
#include <string.h>

#include <random>
#include <stdexcept>

#include "../../kzg-setup-powersoftau_amd/csrc/chunk_plan.hpp"
#include "../../kzg-setup-powersoftau_amd/csrc/host_rt.hpp"

using namespace kzgpot;

static int g_failed = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                       \
    }                                                                   \
  } while (0)

// clears the injected fault on scope exit, so a failed check cannot poison the next case
struct Inject {
  Inject(int site, long skip) { inject_fault(site, skip); }
  ~Inject() { inject_fault(0, 0); }
};

static void test_chunk_plan() {
  std::vector<size_t> sizes = {1, 255, 256, (size_t)1 << 16, ((size_t)1 << 17) + 1, (size_t)1 << 18,
                               ((size_t)1 << 18) + 1, ((size_t)1 << 20) + 12345, (size_t)1 << 21,
                               ((size_t)1 << 21) + 7, (size_t)3 << 20, ((size_t)1 << 22) + 999, (size_t)1 << 23,
                               ((size_t)1 << 24) + 3, (size_t)1 << 25, ((size_t)1 << 27) + 5, (size_t)1 << 28};
  for (size_t k : {1, 2, 4, 8, 16})
    for (size_t d : {(size_t)0, (size_t)2}) sizes.push_back(((size_t)k << 17) - 1 + d);
  for (size_t n : sizes)
    for (bool small_first : {false, true}) {
      const ChunkPlan plan(n, small_first);
      size_t next = 0;
      for (size_t j = 0; j < plan.count(); j++) {
        size_t off, m;
        plan.span(j, off, m);
        CHECK(off == next && m > 0 && m <= plan.max_chunk());
        next = off + m;
      }
      CHECK(next == n);
    }
}

static void test_watermark() {
  {
    Watermark wm;
    std::atomic<int> bad{0};
    auto consumer = [&](size_t step) {
      for (size_t mark = step; mark <= 100; mark += step)
        if (!wm.wait(mark)) bad++;
    };
    std::thread c1(consumer, 7), c2(consumer, 10);
    std::thread producer([&] {
      for (size_t i = 1; i <= 100; i++) wm.advance(i);
    });
    producer.join();
    c1.join();
    c2.join();
    CHECK(bad == 0 && !wm.failed());
  }
  {
    Watermark wm;
    wm.advance(10);
    bool got = true;
    std::thread waiter([&] { got = wm.wait(20); });
    wm.fail();
    waiter.join();
    CHECK(!got && wm.failed());
    CHECK(wm.wait(10));  // had arrived before the failure
    CHECK(!wm.wait(11));
  }
}

static void test_ordered_worker() {
  static const uint8_t base[1] = {0};
  {  // 1000 ranges in push order
    std::vector<size_t> seen;
    OrderedWorker w("order", [&](const uint8_t* p, size_t n) {
      seen.push_back((size_t)(p - base) * 1000003 + n);
      return true;
    });
    CHECK(w.start());
    for (size_t i = 0; i < 1000; i++) w.push(base + i, i + 1);
    CHECK(w.finish());
    CHECK(w.finish());
    CHECK(seen.size() == 1000);
    for (size_t i = 0; i < seen.size(); i++) CHECK(seen[i] == i * 1000003 + i + 1);
  }
  {  // false at item k: no later call
    size_t calls = 0;
    OrderedWorker w("stop", [&](const uint8_t*, size_t n) {
      calls++;
      return n != 5;
    });
    CHECK(w.start());
    for (size_t i = 0; i < 20; i++) w.push(base, i);
    CHECK(!w.finish());
    CHECK(!w.finish());
    CHECK(calls == 6);
  }
  {  // a throwing consumer
    OrderedWorker w("throw", [&](const uint8_t*, size_t) -> bool { throw std::runtime_error("consumer"); });
    CHECK(w.start());
    w.push(base, 1);
    CHECK(!w.finish());
  }
  {  // a refused start: push, finish, destructor
    OrderedWorker w("refused", [&](const uint8_t*, size_t) { return true; });
    {
      Inject fault(kFaultThread, 0);
      CHECK(!w.start());
    }
    w.push(base, 1);
    CHECK(!w.finish());
    CHECK(!w.finish());
  }
}

static void test_threads() {
  for (long skip : {0, 1, 2}) {
    std::atomic<int> ran{0};
    int started = 0;
    {
      ThreadGroup g(4);
      Inject fault(kFaultThread, skip);
      for (int i = 0; i < 4; i++)
        if (g.start([&] { ran++; })) started++;
    }  // joined
    CHECK(started == skip && ran == skip);
  }
  {
    int before = 0;
    std::thread idle;
    { JoinOnExit j{idle, [&] { before++; }}; }
    CHECK(before == 0);
    std::atomic<bool> stop{false};
    std::thread t;
    CHECK(start_thread(t, [&] {
      while (!stop) std::this_thread::yield();
    }));
    { JoinOnExit j{t, [&] { before++, stop = true; }}; }
    CHECK(before == 1 && !t.joinable());
  }
}

static void test_api_guard() {
  CHECK(api_guard([] { return 7; }) == 7);
  CHECK(api_guard([]() -> int { throw std::bad_alloc(); }) == -108);
  CHECK(api_guard([]() -> int { throw std::system_error(EAGAIN, std::generic_category()); }) == -108);
  CHECK(api_guard([]() -> int { throw std::runtime_error("x"); }) == -101);
  CHECK(api_guard([]() -> int { throw 3; }) == -101);
  CHECK(KZGPOT_E_OUT_OF_MEMORY == -108 && KZGPOT_E_DEVICE == -101);
}

static void test_hostbuf() {
  {
    HostBuf b(12345);
    CHECK(b.get() && ((uintptr_t)b.get() & (((size_t)2 << 20) - 1)) == 0);
    b.get()[0] = 1, b.get()[12344] = 2;
  }
  {
    Inject fault(kFaultHostBuf, 0);
    HostBuf b(12345);
    CHECK(b.get() == nullptr);
  }
  {
    Releaser r;
    r.release(std::make_unique<HostBuf>(1 << 20), std::make_unique<HostBuf>(1 << 20));
    r.release(std::make_unique<HostBuf>(1 << 20), nullptr);
  }  // joined by the destructor
  {
    Releaser r;
    Inject fault(kFaultThread, 0);
    r.release(std::make_unique<HostBuf>(1 << 20), std::make_unique<HostBuf>(1 << 20));  // freed here
    r.join();
  }
}

static int count_temporaries(const std::string& dir) {
  int k = 0;
  DIR* d = opendir(dir.c_str());
  if (!d) return -1;
  while (dirent* e = readdir(d))
    if (strstr(e->d_name, ".kzgpot-tmp-")) k++;
  closedir(d);
  return k;
}

static void test_temp_output(const std::string& root) {
  std::string dir_template = root + "/kzgpot-host-units-XXXXXX";
  const char* made = mkdtemp(&dir_template[0]);
  CHECK(made != nullptr);
  if (!made) return;
  const std::string dir = made, target = dir + "/out.bin";
  {
    TempOutput t(target.c_str());
    CHECK(t.fd() >= 0 && count_temporaries(dir) == 1);
  }  // abandoned
  CHECK(count_temporaries(dir) == 0 && access(target.c_str(), F_OK) != 0);
  {
    const uint8_t bytes[5] = {1, 2, 3, 4, 5};
    TempOutput t(target.c_str());
    CHECK(t.fd() >= 0 && pwrite_all(t.fd(), bytes, sizeof bytes, 0));
    CHECK(t.commit());
    CHECK(!t.commit());  // already committed: nothing to rename
  }
  CHECK(count_temporaries(dir) == 0);
  struct stat st;
  CHECK(stat(target.c_str(), &st) == 0 && (st.st_mode & 0777) == 0644 && st.st_size == 5);
  std::vector<uint8_t> back;
  CHECK(read_file(target.c_str(), back, 5) == 0 && back == std::vector<uint8_t>({1, 2, 3, 4, 5}));
  CHECK(read_file(target.c_str(), back, 6) == KZGPOT_E_SIZE);
  CHECK(read_file((dir + "/absent").c_str(), back) == KZGPOT_E_IO);
  {
    TempOutput t((dir + "/no-such-dir/out.bin").c_str());
    CHECK(t.fd() < 0 && !t.commit());
  }
  CHECK(count_temporaries(dir) == 0);
  unlink(target.c_str());
  rmdir(dir.c_str());
}

// the pieces (shard, off, m) that shard g lands, in order: its range cut in two or three
struct Piece {
  int shard;
  uint64_t off, m;
};
static std::vector<std::vector<Piece>> shard_pieces(uint64_t count, int shards) {
  const uint64_t per = (count + shards - 1) / shards;
  std::vector<std::vector<Piece>> out(shards);
  for (int g = 0; g < shards; g++) {
    const uint64_t lo = std::min<uint64_t>(count, g * per), hi = std::min(count, lo + per), len = hi - lo;
    if (len == 0) continue;  // a trailing empty shard never lands (run_host returns at n == 0)
    const uint64_t parts = len >= 3 && g % 2 ? 3 : len >= 2 ? 2 : 1;
    for (uint64_t k = 0, off = 0; k < parts; k++) {
      const uint64_t m = k + 1 == parts ? len - off : std::max<uint64_t>(1, len / parts);
      out[g].push_back({g, off, m});
      off += m;
    }
  }
  return out;
}
// what the sink must have seen: non-empty, contiguous, ascending from 0
struct Coverage {
  uint64_t next = 0;
  bool ok = true;
  void operator()(uint64_t first, uint64_t k) {
    if (first != next || k == 0) ok = false;
    next = first + k;
  }
};

static void test_shard_cursor() {
  const struct { uint64_t count; int shards; } cases[] = {{15, 4}, {15, 1}, {5, 7}, {16, 4}};
  for (const auto& c : cases) {
    const uint64_t per = (c.count + c.shards - 1) / c.shards;
    const auto pieces = shard_pieces(c.count, c.shards);
    // one thread, 200 seeded interleavings that keep each shard's own order
    std::mt19937 rng(12345);
    for (int round = 0; round < 200; round++) {
      std::vector<int> order;
      for (int g = 0; g < c.shards; g++) order.insert(order.end(), pieces[g].size(), g);
      std::shuffle(order.begin(), order.end(), rng);
      std::vector<size_t> at(c.shards, 0);
      ShardCursor cur(c.count, per, c.shards);
      Coverage cov;
      for (int g : order) {
        const Piece& p = pieces[g][at[g]++];
        CHECK(!cur.done());
        cur.land(p.shard, p.off, p.m, cov);
      }
      CHECK(cov.ok && cov.next == c.count && cur.done());
    }
    {  // one thread per shard
      ShardCursor cur(c.count, per, c.shards);
      Coverage cov;  // written under the cursor's lock only
      {
        ThreadGroup th(c.shards);
        for (int g = 0; g < c.shards; g++)
          CHECK(th.start([&, g] {
            for (const Piece& p : pieces[g]) cur.land(p.shard, p.off, p.m, cov);
          }));
      }
      CHECK(cov.ok && cov.next == c.count && cur.done());
    }
    if (c.shards > 1) {  // shard 1 never lands: the section is not whole
      ShardCursor cur(c.count, per, c.shards);
      Coverage cov;
      for (int g = 0; g < c.shards; g++)
        if (g != 1)
          for (const Piece& p : pieces[g]) cur.land(p.shard, p.off, p.m, cov);
      CHECK(cov.ok && cov.next == std::min(c.count, per) && !cur.done());
    }
  }
}

static void test_small_helpers() {
  int sec = 3;
  int64_t idx = 9;
  reset_bad(&sec, &idx);
  CHECK(sec == -1 && idx == -1);
  reset_bad(nullptr, nullptr);
  const std::string hex(128, 'a');
  CHECK(is_hex128(hex.c_str()) && is_hex128(std::string(128, 'F').c_str()));
  CHECK(!is_hex128((hex + "0").c_str()) && !is_hex128(hex.substr(1).c_str()) && !is_hex128((hex.substr(1) + "g").c_str()));
}

int main(int argc, char** argv) {  // argv[1]: a directory for the TempOutput files (default /tmp)
  test_chunk_plan();
  test_watermark();
  test_ordered_worker();
  test_threads();
  test_api_guard();
  test_hostbuf();
  test_temp_output(argc > 1 ? argv[1] : "/tmp");
  test_shard_cursor();
  test_small_helpers();
  if (g_failed) {
    fprintf(stderr, "host_units: %d check(s) failed\n", g_failed);
    return 1;
  }
  puts("host_units ok");
  return 0;
}

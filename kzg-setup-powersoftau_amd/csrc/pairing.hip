// C ABI (include/kzgpot.h): the product of pairings (kernels: pairing_kernels.hip; the workspace is
// pairing_plan's, plans.hpp).
#include "codec.hpp"
#include "device_rt.hpp"
#include "host_rt.hpp"

using namespace kzgpot;

namespace {

constexpr uint64_t kOutBytes = KZGPOT_GT_BYTES + 4;  // GT, then the u32 "is one"

int pairing_dev(const void* d_g1, const void* d_g2, uint64_t k, void* d_out, void* d_work, uint64_t* d_bad_key,
                void* stream) {
  if (!pairing_workspace_bytes(k) || !d_out || !d_work || !d_bad_key || (k && (!d_g1 || !d_g2))) return KZGPOT_E_INVALID_ARG;
  const hipStream_t s = (hipStream_t)stream;
  return launch_with_key(d_bad_key, s, [&](unsigned long long* key) {
    return launch_pairing_product(d_g1, d_g2, k, d_out, d_work, key, 0, s);
  });
}

int pairing_host(const uint8_t* g1, const uint8_t* g2, uint64_t k, uint8_t* out_gt, int64_t* first_bad) {
  if (first_bad) *first_bad = -1;
  const uint64_t work_bytes = pairing_workspace_bytes(k);
  if (!work_bytes || (k && (!g1 || !g2))) return KZGPOT_E_INVALID_ARG;
  StagedCall call;
  void *d_g1, *d_g2, *d_out, *work;
  if (call.begin() || call.in(d_g1, g1, k * point_record(false)) || call.in(d_g2, g2, k * point_record(true)) ||
      call.alloc(d_out, kOutBytes) || call.alloc(work, work_bytes) || call.key())
    return KZGPOT_E_DEVICE;
  return call.finish(pairing_dev(d_g1, d_g2, k, d_out, work, call.d_key, nullptr), first_bad, [&] {
    const int is_one = read_verdict(d_out);  // before the GT bytes: an error here leaves out_gt alone
    if (is_one >= 0 && out_gt && copy_out(out_gt, d_out, KZGPOT_GT_BYTES)) return KZGPOT_E_DEVICE;
    return is_one;
  });
}

}  // namespace

extern "C" {

/* host only */
uint64_t kzgpot_pairing_workspace(uint64_t k) { return pairing_workspace_bytes(k); }
int kzgpot_pairing_product_dev(const void* d_g1, const void* d_g2, uint64_t k, void* d_out, void* d_work,
                               uint64_t* d_bad_key, void* stream) {
  return api_guard([&] { return pairing_dev(d_g1, d_g2, k, d_out, d_work, d_bad_key, stream); });
}
int kzgpot_pairing_product(const uint8_t* g1, const uint8_t* g2, uint64_t k, uint8_t* out_gt, int64_t* first_bad) {
  return api_guard([&] { return pairing_host(g1, g2, k, out_gt, first_bad); });
}

}  // extern "C"

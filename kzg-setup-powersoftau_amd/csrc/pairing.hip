// C ABI (include/kzgpot.h): the product of pairings (kernels: pairing_kernels.hip; the workspace is
// pairing_plan's, plans.hpp).
#include <string.h>

#include "codec.hpp"
#include "device_rt.hpp"
#include "host_rt.hpp"

using namespace kzgpot;

namespace {

constexpr uint64_t kOutBytes = KZGPOT_GT_BYTES + 4;  // GT, then the u32 "is one"

// host_key (optional): receives the bad key once the product is done
int pairing_dev(const void* d_g1, const void* d_g2, uint64_t k, void* d_out, void* d_work, uint64_t* d_bad_key,
                void* stream, uint64_t* host_key = nullptr) {
  if (!pairing_workspace_bytes(k) || !d_out || !d_work || !d_bad_key || (k && (!d_g1 || !d_g2))) return KZGPOT_E_INVALID_ARG;
  const hipStream_t s = (hipStream_t)stream;
  return launch_with_key(d_bad_key, s, [&](unsigned long long* key) {
    return launch_pairing_product(d_g1, d_g2, k, d_out, d_work, key, 0, s);
  }, host_key);
}

int pairing_host(const uint8_t* g1, const uint8_t* g2, uint64_t k, uint8_t* out_gt, int64_t* first_bad) {
  if (first_bad) *first_bad = -1;
  const uint64_t work_bytes = pairing_workspace_bytes(k);
  if (!work_bytes || (k && (!g1 || !g2))) return KZGPOT_E_INVALID_ARG;
  if (device_count() <= 0) return KZGPOT_E_DEVICE;
  DeviceGuard guard;
  DevBuf d_g1, d_g2, d_out, work, key;
  if (d_g1.alloc(k * point_record(false)) || d_g2.alloc(k * point_record(true)) || d_out.alloc(kOutBytes) ||
      work.alloc(work_bytes) || key.alloc(sizeof(uint64_t)))
    return KZGPOT_E_DEVICE;
  if (k) {
    HIP_TRY(hipMemcpy(d_g1.p, g1, k * point_record(false), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_g2.p, g2, k * point_record(true), hipMemcpyHostToDevice));
  }
  uint64_t bad;
  if (const int r = pairing_dev(d_g1.p, d_g2.p, k, d_out.p, work.p, (uint64_t*)key.p, nullptr, &bad)) return r;
  if (bad != kNoBad) return decode_key(bad, first_bad);  // rejected: nothing is written
  uint8_t out[kOutBytes];
  HIP_TRY(hipMemcpy(out, d_out.p, kOutBytes, hipMemcpyDeviceToHost));
  if (out_gt) memcpy(out_gt, out, KZGPOT_GT_BYTES);
  uint32_t is_one;
  memcpy(&is_one, out + KZGPOT_GT_BYTES, 4);
  return is_one ? 1 : 0;
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

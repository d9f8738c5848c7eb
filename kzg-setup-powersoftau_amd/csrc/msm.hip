// C ABI (include/kzgpot.h): the G1 / G2 multi-scalar multiplication of KZG10::commit
// (kernels: msm_kernels.hip).
#include "codec.hpp"
#include "device_rt.hpp"
#include "host_rt.hpp"

using namespace kzgpot;

namespace {

int msm_dev(bool g2, const void* d_bases, const void* d_scalars, uint64_t n, void* d_out, uint32_t flags, void* d_work,
            uint64_t* d_bad_key, void* stream) {
  uint32_t c;
  if (!msm_flags(flags, c) || !msm_workspace_bytes(g2, n, c) || !d_out || !d_work || !d_bad_key || (n && (!d_bases || !d_scalars)))
    return KZGPOT_E_INVALID_ARG;
  const hipStream_t s = (hipStream_t)stream;
  return launch_with_key(d_bad_key, s, [&](unsigned long long* key) {
    return launch_msm(g2, d_bases, d_scalars, n, d_out, flags & KZGPOT_MSM_BASES_MONT, c ? c : msm_window_bits(n),
                      d_work, key, s);
  });
}

int msm_host(bool g2, const uint8_t* bases, const uint8_t* scalars, uint64_t n, uint8_t* out, uint32_t flags,
             int64_t* first_bad) {
  if (first_bad) *first_bad = -1;
  uint32_t c;
  const uint64_t work_bytes = msm_flags(flags, c) ? msm_workspace_bytes(g2, n, c) : 0;
  if (!work_bytes || !out || (n && (!bases || !scalars))) return KZGPOT_E_INVALID_ARG;
  const uint64_t rec = base_record(g2, flags & KZGPOT_MSM_BASES_MONT), out_bytes = point_record(g2);
  StagedCall call;
  void *d_bases, *d_scalars, *d_out, *work;
  if (call.begin() || call.in(d_bases, bases, n * rec) || call.in(d_scalars, scalars, n * 32) ||
      call.alloc(d_out, out_bytes) || call.alloc(work, work_bytes) || call.key())
    return KZGPOT_E_DEVICE;
  return call.finish(msm_dev(g2, d_bases, d_scalars, n, d_out, flags, work, call.d_key, nullptr), first_bad,
                     [&] { return copy_out(out, d_out, out_bytes); });
}

}  // namespace

extern "C" {

/* host only */
uint32_t kzgpot_msm_window_bits(uint64_t n) { return msm_window_bits(n); }
uint64_t kzgpot_msm_workspace(int g2, uint64_t n, uint32_t flags) {
  uint32_t c;
  return msm_flags(flags, c) ? msm_workspace_bytes(g2 != 0, n, c) : 0;
}
int kzgpot_g1_msm_dev(const void* d_bases, const void* d_scalars, uint64_t n, void* d_out, uint32_t flags, void* d_work,
                      uint64_t* d_bad_key, void* stream) {
  return api_guard([&] { return msm_dev(false, d_bases, d_scalars, n, d_out, flags, d_work, d_bad_key, stream); });
}
int kzgpot_g2_msm_dev(const void* d_bases, const void* d_scalars, uint64_t n, void* d_out, uint32_t flags, void* d_work,
                      uint64_t* d_bad_key, void* stream) {
  return api_guard([&] { return msm_dev(true, d_bases, d_scalars, n, d_out, flags, d_work, d_bad_key, stream); });
}
int kzgpot_g1_msm(const uint8_t* bases, const uint8_t* scalars, uint64_t n, uint8_t* out, uint32_t flags,
                  int64_t* first_bad) {
  return api_guard([&] { return msm_host(false, bases, scalars, n, out, flags, first_bad); });
}
int kzgpot_g2_msm(const uint8_t* bases, const uint8_t* scalars, uint64_t n, uint8_t* out, uint32_t flags,
                  int64_t* first_bad) {
  return api_guard([&] { return msm_host(true, bases, scalars, n, out, flags, first_bad); });
}

}  // extern "C"

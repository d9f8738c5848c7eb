// C ABI (include/kzgpot.h): ark-poly-commit's KZG10::check and KZG10::batch_check — the Fr pass and
// the negation by verify_kernels.hip, total_c and total_w by two launch_msm (msm_kernels.hip), the
// product of the two pairings by launch_pairing_product (pairing_kernels.hip). The scalars, both sums
// and both points never leave HBM. The workspace is check_plan's (plans.hpp).
#include "codec.hpp"
#include "device_rt.hpp"
#include "host_rt.hpp"

using namespace kzgpot;

namespace {

constexpr uint64_t kG1 = point_record(false), kG2 = point_record(true);
constexpr uint64_t kVkBytes = 2 * kG1 + 2 * kG2, kOutBytes = KZGPOT_GT_BYTES + 4;
static_assert(kVkBytes == 576, "g, gamma_g, h, beta_h");

int check_dev(const void* d_vk, const void* d_commitments, const void* d_points, const void* d_values,
              const void* d_proofs_w, const void* d_random_vs, const void* d_randomizers, uint64_t n, void* d_out,
              uint32_t flags, void* d_work, uint64_t* d_bad_key, void* stream) {
  const CheckPlan p = check_plan(n, flags);
  if (!p.ok || !d_vk || !d_out || !d_work || !d_bad_key ||
      (n && (!d_commitments || !d_points || !d_values || !d_proofs_w || !d_randomizers)))
    return KZGPOT_E_INVALID_ARG;
  const hipStream_t s = (hipStream_t)stream;
  uint8_t* w = (uint8_t*)d_work;
  uint8_t *bases = w + p.bases, *scalars = w + p.scalars, *total_c = w + p.pairs_g1, *total_w = total_c + kG1;
  const uint8_t* vk = (const uint8_t*)d_vk;
  auto width = [&](uint64_t m) { return p.c ? p.c : msm_window_bits(m); };
  return launch_with_key(d_bad_key, s, [&](unsigned long long* key) -> hipError_t {
    hipError_t e;
    if (n && (e = hipMemcpyAsync(bases, d_commitments, n * kG1, hipMemcpyDeviceToDevice, s))) return e;
    if (n && (e = hipMemcpyAsync(bases + n * kG1, d_proofs_w, n * kG1, hipMemcpyDeviceToDevice, s))) return e;
    if ((e = hipMemcpyAsync(bases + 2 * n * kG1, vk, 2 * kG1, hipMemcpyDeviceToDevice, s))) return e;  // g, gamma_g
    if ((e = hipMemcpyAsync(w + p.pairs_g2, vk + 2 * kG1, 2 * kG2, hipMemcpyDeviceToDevice, s))) return e;  // h, beta_h
    // an MSM that rejects a base writes no point: the pairing's load then reads these zeros, a well-formed record
    if ((e = hipMemsetAsync(total_c, 0, 2 * kG1, s))) return e;
    if ((e = hipMemsetAsync(w + p.key2, 0xff, sizeof(uint64_t), s))) return e;
    if ((e = launch_check_scalars(p, d_randomizers, d_points, d_values, d_random_vs, d_work, s))) return e;
    // total_w = sum [rho_i] W_i: the proofs where they lie, the first n scalar rows; its rejections (under
    // the proofs' own indices) go to a key of its own, the next MSM reports the same records under theirs
    if ((e = launch_msm(false, bases + n * kG1, scalars, n, total_w, false, width(n), w + p.msm,
                        (unsigned long long*)(w + p.key2), s)))
      return e;
    if ((e = launch_msm(false, bases, scalars, p.nbases, total_c, false, width(p.nbases), w + p.msm, key, s))) return e;
    if ((e = launch_g1_negate(total_w, s))) return e;
    // e(total_c, h) e(-total_w, beta_h); h and beta_h are records 2 n + 2 and 2 n + 3 of the call
    return launch_pairing_product(total_c, w + p.pairs_g2, 2, d_out, w + p.pairing, key, 2 * n, s);
  });
}

int check_host(const uint8_t* vk, const uint8_t* commitments, const uint8_t* points, const uint8_t* values,
               const uint8_t* proofs_w, const uint8_t* random_vs, const uint8_t* randomizers, uint64_t n, uint32_t flags,
               int64_t* first_bad) {
  if (first_bad) *first_bad = -1;
  const CheckPlan p = check_plan(n, flags);
  if (!p.ok || !vk || (n && (!commitments || !points || !values || !proofs_w || !randomizers))) return KZGPOT_E_INVALID_ARG;
  StagedCall call;
  // the G1 records end to end (commitments, proofs), the four scalar arrays end to end
  const uint64_t ns = random_vs ? 4 : 3, g = n * kG1, s = n * 32;
  void *d_vk, *d_out, *work;
  uint8_t *dp, *ds;
  if (call.begin() || call.in(d_vk, vk, kVkBytes) || call.alloc(dp, 2 * g) || call.alloc(ds, ns * s) ||
      call.alloc(d_out, kOutBytes) || call.alloc(work, p.bytes) || call.key() || call.copy_in(dp, commitments, g) ||
      call.copy_in(dp + g, proofs_w, g) || call.copy_in(ds, points, s) || call.copy_in(ds + s, values, s) ||
      call.copy_in(ds + 2 * s, randomizers, s) || (random_vs && call.copy_in(ds + 3 * s, random_vs, s)))
    return KZGPOT_E_DEVICE;
  return call.finish(check_dev(d_vk, dp, ds, ds + s, dp + g, random_vs ? ds + 3 * s : nullptr, ds + 2 * s, n, d_out,
                               flags, work, call.d_key, nullptr),
                     first_bad, [&] { return read_verdict(d_out); });
}

}  // namespace

extern "C" {

/* host only */
uint64_t kzgpot_kzg_batch_check_workspace(uint64_t n, uint32_t flags) { return check_workspace_bytes(n, flags); }
int kzgpot_kzg_batch_check_dev(const void* d_vk, const void* d_commitments, const void* d_points, const void* d_values,
                               const void* d_proofs_w, const void* d_random_vs, const void* d_randomizers, uint64_t n,
                               void* d_out, uint32_t flags, void* d_work, uint64_t* d_bad_key, void* stream) {
  return api_guard([&] {
    return check_dev(d_vk, d_commitments, d_points, d_values, d_proofs_w, d_random_vs, d_randomizers, n, d_out, flags,
                     d_work, d_bad_key, stream);
  });
}
int kzgpot_kzg_batch_check(const uint8_t vk[576], const uint8_t* commitments, const uint8_t* points,
                           const uint8_t* values, const uint8_t* proofs_w, const uint8_t* random_vs,
                           const uint8_t* randomizers, uint64_t n, uint32_t flags, int64_t* first_bad) {
  return api_guard([&] {
    return check_host(vk, commitments, points, values, proofs_w, random_vs, randomizers, n, flags, first_bad);
  });
}
int kzgpot_kzg_check(const uint8_t vk[576], const uint8_t commitment[96], const uint8_t z_le32[32],
                     const uint8_t value_le32[32], const uint8_t w[96], const uint8_t* random_v_le32, int64_t* first_bad) {
  const uint8_t one[32] = {1};  // rho = 1
  return api_guard([&] { return check_host(vk, commitment, z_le32, value_le32, w, random_v_le32, one, 1, 0, first_bad); });
}

}  // extern "C"

// C ABI (include/kzgpot.h): Fr vectors in evaluation form — the batch inversion, the division of a
// polynomial by (x - z) from its evaluations over a radix-2 domain and the KZG10 open on top of it
// (kernels: eval_kernels.hip; the proof's point by one launch_msm over the caller's Lagrange basis),
// DESIGN.md §13. What the kernels read about the domain and z comes from the host side of csrc/fr.hpp.
#include "codec.hpp"
#include "device_rt.hpp"
#include "host_rt.hpp"

using namespace kzgpot;

namespace {

constexpr uint64_t kPointBytes = point_record(false), kOutBytes = kPointBytes + 32;

// ---------------------------------------------------------------- batch inversion
// false: invalid arguments. t: the tile
bool inverse_args(uint64_t n, uint32_t flags, const void* in, const void* out, uint32_t& t) {
  return poly_flags(flags, t) && n <= kEvalMaxN && (!n || (in && out));
}

int batch_inverse_dev(const void* d_in, uint64_t n, void* d_out, uint32_t flags, void* stream) {
  uint32_t t;
  if (!inverse_args(n, flags, d_in, d_out, t)) return KZGPOT_E_INVALID_ARG;
  HIP_TRY(launch_fr_batch_inverse(d_in, n, d_out, t, (hipStream_t)stream));
  return 0;
}

int batch_inverse_host(const uint8_t* in, uint64_t n, uint8_t* out, uint32_t flags) {
  uint32_t t;
  if (!inverse_args(n, flags, in, out, t)) return KZGPOT_E_INVALID_ARG;
  if (!n) return 0;
  StagedCall call;
  void* io;
  if (call.begin() || call.in(io, in, n * 32)) return KZGPOT_E_DEVICE;
  return call.finish(batch_inverse_dev(io, n, io, flags, nullptr), nullptr, [&] { return copy_out(out, io, n * 32); });
}

// ---------------------------------------------------------------- division in evaluation form
int evals_divide_dev(const void* d_evals, uint32_t exp, const uint8_t* z, void* d_quotient, void* d_value, uint32_t flags,
                     void* d_work, void* stream) {
  uint32_t t;
  if (!poly_flags(flags, t) || exp > kEvalMaxExp || !d_evals || !z || !d_value || !d_work) return KZGPOT_E_INVALID_ARG;
  fr_eval_scalars sc;
  fr_eval_setup(sc, exp, z);
  HIP_TRY(launch_evals_divide(eval_plan(exp, t), d_evals, sc, d_quotient, d_value, d_work, (hipStream_t)stream));
  return 0;
}

int evals_divide_host(const uint8_t* evals, uint32_t exp, const uint8_t* z, uint8_t* quotient, uint8_t* value,
                      uint32_t flags) {
  const uint64_t work_bytes = eval_workspace_bytes(exp, flags);
  if (!work_bytes || !evals || !z || !value) return KZGPOT_E_INVALID_ARG;
  const uint64_t bytes = (uint64_t)32 << exp;
  StagedCall call;
  void *d_evals, *d_quot = nullptr, *d_value, *work;  // no quotient wanted: no buffer
  if (call.begin() || call.in(d_evals, evals, bytes) || (quotient && call.alloc(d_quot, bytes)) ||
      call.alloc(d_value, 32) || call.alloc(work, work_bytes))
    return KZGPOT_E_DEVICE;
  return call.finish(evals_divide_dev(d_evals, exp, z, d_quot, d_value, flags, work, nullptr), nullptr, [&] {
    if (const int r = copy_out(value, d_value, 32)) return r;
    return quotient ? copy_out(quotient, d_quot, bytes) : 0;
  });
}

// ---------------------------------------------------------------- open
// The workspace is open_evals_plan's (plans.hpp)
int open_evals_dev(const void* d_lagrange, const void* d_evals, uint32_t exp, const uint8_t* z, void* d_out, uint32_t flags,
                   void* d_work, uint64_t* d_bad_key, void* stream) {
  const OpenEvalsPlan p = open_evals_plan(exp, flags);
  if (!p.ok || !d_lagrange || !d_evals || !z || !d_out || !d_work || !d_bad_key) return KZGPOT_E_INVALID_ARG;
  fr_eval_scalars sc;
  fr_eval_setup(sc, exp, z);
  const hipStream_t s = (hipStream_t)stream;
  uint8_t* w = (uint8_t*)d_work;
  uint8_t *quot = w + p.quot, *value = w + p.ev.words + kEvalValueAt;
  return launch_with_key(d_bad_key, s, [&](unsigned long long* key) -> hipError_t {
    hipError_t e;
    if ((e = launch_evals_divide(p.ev, d_evals, sc, quot, value, w, s))) return e;
    if ((e = launch_msm(false, d_lagrange, quot, p.ev.n, d_out, flags & KZGPOT_MSM_BASES_MONT,
                        p.c ? p.c : msm_window_bits(p.ev.n), w + p.msm, key, s)))
      return e;
    return launch_fr_emit(value, (uint8_t*)d_out + kPointBytes, 8, key, s);  // the value
  });
}

int open_evals_host(const uint8_t* lagrange, const uint8_t* evals, uint32_t exp, const uint8_t* z, uint8_t* out,
                    uint32_t flags, int64_t* first_bad) {
  if (first_bad) *first_bad = -1;
  const OpenEvalsPlan p = open_evals_plan(exp, flags);
  if (!p.ok || !lagrange || !evals || !z || !out) return KZGPOT_E_INVALID_ARG;
  StagedCall call;
  void *d_bases, *d_evals, *d_out, *work;
  if (call.begin() || call.in(d_bases, lagrange, p.ev.n * p.rec) || call.in(d_evals, evals, p.ev.n * 32) ||
      call.alloc(d_out, kOutBytes) || call.alloc(work, p.bytes) || call.key())
    return KZGPOT_E_DEVICE;
  return call.finish(open_evals_dev(d_bases, d_evals, exp, z, d_out, flags, work, call.d_key, nullptr), first_bad,
                     [&] { return copy_out(out, d_out, kOutBytes); });
}

}  // namespace

extern "C" {

/* host only */
uint64_t kzgpot_fr_evals_workspace(uint32_t exp, uint32_t flags) { return eval_workspace_bytes(exp, flags); }
uint64_t kzgpot_kzg_open_evals_workspace(uint32_t exp, uint32_t flags) { return open_evals_plan(exp, flags).bytes; }

int kzgpot_fr_batch_inverse_dev(const void* d_in, uint64_t n, void* d_out, uint32_t flags, void* stream) {
  return api_guard([&] { return batch_inverse_dev(d_in, n, d_out, flags, stream); });
}
int kzgpot_fr_batch_inverse(const uint8_t* in, uint64_t n, uint8_t* out, uint32_t flags) {
  return api_guard([&] { return batch_inverse_host(in, n, out, flags); });
}
int kzgpot_fr_evals_divide_dev(const void* d_evals, uint32_t exp, const uint8_t z_le32[32], void* d_quotient, void* d_value,
                               uint32_t flags, void* d_work, void* stream) {
  return api_guard([&] { return evals_divide_dev(d_evals, exp, z_le32, d_quotient, d_value, flags, d_work, stream); });
}
int kzgpot_fr_evals_divide(const uint8_t* evals, uint32_t exp, const uint8_t z_le32[32], uint8_t* quotient,
                           uint8_t value_le32[32], uint32_t flags) {
  return api_guard([&] { return evals_divide_host(evals, exp, z_le32, quotient, value_le32, flags); });
}
int kzgpot_g1_kzg_open_evals_dev(const void* d_lagrange, const void* d_evals, uint32_t exp, const uint8_t z_le32[32],
                                 void* d_out, uint32_t flags, void* d_work, uint64_t* d_bad_key, void* stream) {
  return api_guard(
      [&] { return open_evals_dev(d_lagrange, d_evals, exp, z_le32, d_out, flags, d_work, d_bad_key, stream); });
}
int kzgpot_g1_kzg_open_evals(const uint8_t* lagrange, const uint8_t* evals, uint32_t exp, const uint8_t z_le32[32],
                             uint8_t out[128], uint32_t flags, int64_t* first_bad) {
  return api_guard([&] { return open_evals_host(lagrange, evals, exp, z_le32, out, flags, first_bad); });
}

}  // extern "C"

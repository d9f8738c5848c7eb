// C ABI (include/kzgpot.h): division of a polynomial over Fr by (x - z) and ark-poly-commit's
// KZG10::open on top of it — the witness polynomials by poly_kernels.hip, the proof's point by one
// launch_msm (msm_kernels.hip) over both quotients. The quotients never leave HBM. The powers of z
// that the division's kernels read come from the host side of csrc/fr.hpp.
#include "codec.hpp"
#include "device_rt.hpp"
#include "host_rt.hpp"

using namespace kzgpot;

namespace {

constexpr uint64_t kPointBytes = point_record(false), kOutBytes = kPointBytes + 64;

// z^(2^k) for k < kPolyPowers; z is any 256-bit integer
fr_powers<kPolyPowers> z_powers(const uint8_t z_le32[32]) {
  fr_powers<kPolyPowers> zp;
  fr_fill_powers(zp.p, fr_from_le32(z_le32));
  return zp;
}

// ---------------------------------------------------------------- division
int poly_divide_dev(const void* d_coeffs, uint64_t n, const uint8_t* z, void* d_quotient, void* d_value, uint32_t flags,
                    void* d_work, void* stream) {
  uint32_t t;
  if (!poly_flags(flags, t) || !poly_workspace_bytes(n, t) || !z || !d_value || !d_work || (n && !d_coeffs))
    return KZGPOT_E_INVALID_ARG;
  const fr_powers<kPolyPowers> zp = z_powers(z);
  HIP_TRY(launch_poly_divide(d_coeffs, n, zp, d_quotient, d_value, t, d_work, (hipStream_t)stream));
  return 0;
}

int poly_divide_host(const uint8_t* coeffs, uint64_t n, const uint8_t* z, uint8_t* quotient, uint8_t* value,
                     uint32_t flags) {
  uint32_t t;
  const uint64_t work_bytes = poly_flags(flags, t) ? poly_workspace_bytes(n, t) : 0;
  if (!work_bytes || !z || !value || (n && !coeffs)) return KZGPOT_E_INVALID_ARG;
  const uint64_t nq = n ? n - 1 : 0;
  StagedCall call;
  void *d_coeffs, *d_quot = nullptr, *d_value, *work;  // no quotient wanted: no buffer
  if (call.begin() || call.in(d_coeffs, coeffs, n * 32) || (quotient && call.alloc(d_quot, nq * 32)) ||
      call.alloc(d_value, 32) || call.alloc(work, work_bytes))
    return KZGPOT_E_DEVICE;
  return call.finish(poly_divide_dev(d_coeffs, n, z, d_quot, d_value, flags, work, nullptr), nullptr, [&] {
    if (const int r = copy_out(value, d_value, 32)) return r;
    return quotient && nq ? copy_out(quotient, d_quot, nq * 32) : 0;
  });
}

// ---------------------------------------------------------------- open
// The workspace is open_plan's (plans.hpp).
int open_dev(const void* d_powers_of_g, const void* d_coeffs, uint64_t n, const void* d_powers_of_gamma_g,
             const void* d_blinding, uint64_t n_blind, const uint8_t* z, void* d_out, uint32_t flags, void* d_work,
             uint64_t* d_bad_key, void* stream) {
  const OpenPlan p = open_plan(n, n_blind, flags);
  if (!p.ok || !z || !d_out || !d_work || !d_bad_key || (n && !d_coeffs) || (n_blind && !d_blinding) ||
      (p.nq && !d_powers_of_g) || (p.nb && !d_powers_of_gamma_g))
    return KZGPOT_E_INVALID_ARG;
  const fr_powers<kPolyPowers> zp = z_powers(z);
  const hipStream_t s = (hipStream_t)stream;
  uint8_t* w = (uint8_t*)d_work;
  uint8_t *bases = w + p.bases, *scalars = w + p.scalars, *values = w + p.values;
  const uint64_t total = p.nq + p.nb;
  return launch_with_key(d_bad_key, s, [&](unsigned long long* key) -> hipError_t {
    hipError_t e;
    if ((e = hipMemsetAsync(values, 0, 64, s))) return e;  // no blinding polynomial: random_v = 0
    if ((e = launch_poly_divide(d_coeffs, n, zp, scalars, values, p.t, w + p.poly, s))) return e;
    if (n_blind && (e = launch_poly_divide(d_blinding, n_blind, zp, scalars + p.nq * 32, values + 32, p.t, w + p.poly, s)))
      return e;
    if (p.nq && (e = hipMemcpyAsync(bases, d_powers_of_g, p.nq * p.rec, hipMemcpyDeviceToDevice, s))) return e;
    if (p.nb && (e = hipMemcpyAsync(bases + p.nq * p.rec, d_powers_of_gamma_g, p.nb * p.rec, hipMemcpyDeviceToDevice, s)))
      return e;
    if ((e = launch_msm(false, bases, scalars, total, d_out, flags & KZGPOT_MSM_BASES_MONT,
                        p.c ? p.c : msm_window_bits(total), w + p.msm, key, s)))
      return e;
    return launch_fr_emit(values, (uint8_t*)d_out + kPointBytes, 16, key, s);  // value, random_v
  });
}

int open_host(const uint8_t* powers_of_g, const uint8_t* coeffs, uint64_t n, const uint8_t* powers_of_gamma_g,
              const uint8_t* blinding, uint64_t n_blind, const uint8_t* z, uint8_t* out, uint32_t flags,
              int64_t* first_bad) {
  if (first_bad) *first_bad = -1;
  const OpenPlan p = open_plan(n, n_blind, flags);
  if (!p.ok || !z || !out || (n && !coeffs) || (n_blind && !blinding) || (p.nq && !powers_of_g) ||
      (p.nb && !powers_of_gamma_g))
    return KZGPOT_E_INVALID_ARG;
  StagedCall call;
  void *d_pg, *d_pgg, *d_coeffs, *d_blind, *d_out, *work;
  if (call.begin() || call.in(d_pg, powers_of_g, p.nq * p.rec) || call.in(d_pgg, powers_of_gamma_g, p.nb * p.rec) ||
      call.in(d_coeffs, coeffs, n * 32) || call.in(d_blind, blinding, n_blind * 32) || call.alloc(d_out, kOutBytes) ||
      call.alloc(work, p.bytes) || call.key())
    return KZGPOT_E_DEVICE;
  return call.finish(open_dev(d_pg, d_coeffs, n, d_pgg, d_blind, n_blind, z, d_out, flags, work, call.d_key, nullptr),
                     first_bad, [&] { return copy_out(out, d_out, kOutBytes); });
}

}  // namespace

extern "C" {

/* host only */
uint64_t kzgpot_fr_poly_workspace(uint64_t n, uint32_t flags) {
  uint32_t t;
  return poly_flags(flags, t) ? poly_workspace_bytes(n, t) : 0;
}
uint64_t kzgpot_kzg_open_workspace(uint64_t n, uint64_t n_blind, uint32_t flags) {
  return open_plan(n, n_blind, flags).bytes;
}
int kzgpot_fr_poly_divide_dev(const void* d_coeffs, uint64_t n, const uint8_t z_le32[32], void* d_quotient,
                              void* d_value, uint32_t flags, void* d_work, void* stream) {
  return api_guard([&] { return poly_divide_dev(d_coeffs, n, z_le32, d_quotient, d_value, flags, d_work, stream); });
}
int kzgpot_fr_poly_divide(const uint8_t* coeffs, uint64_t n, const uint8_t z_le32[32], uint8_t* quotient,
                          uint8_t value_le32[32], uint32_t flags) {
  return api_guard([&] { return poly_divide_host(coeffs, n, z_le32, quotient, value_le32, flags); });
}
int kzgpot_g1_kzg_open_dev(const void* d_powers_of_g, const void* d_coeffs, uint64_t n, const void* d_powers_of_gamma_g,
                           const void* d_blinding, uint64_t n_blind, const uint8_t z_le32[32], void* d_out,
                           uint32_t flags, void* d_work, uint64_t* d_bad_key, void* stream) {
  return api_guard([&] {
    return open_dev(d_powers_of_g, d_coeffs, n, d_powers_of_gamma_g, d_blinding, n_blind, z_le32, d_out, flags, d_work,
                    d_bad_key, stream);
  });
}
int kzgpot_g1_kzg_open(const uint8_t* powers_of_g, const uint8_t* coeffs, uint64_t n, const uint8_t* powers_of_gamma_g,
                       const uint8_t* blinding, uint64_t n_blind, const uint8_t z_le32[32], uint8_t out[160],
                       uint32_t flags, int64_t* first_bad) {
  return api_guard([&] {
    return open_host(powers_of_g, coeffs, n, powers_of_gamma_g, blinding, n_blind, z_le32, out, flags, first_bad);
  });
}

}  // extern "C"

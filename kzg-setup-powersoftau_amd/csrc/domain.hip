// C ABI (include/kzgpot.h): the NTT over Fr (ntt_kernels.hip) and the amortized KZG10 openings over
// a radix-2 domain on top of it and of the group FFT's pieces (fft_kernels.hip), DESIGN.md §12.
// Every transform's scalars come from the host side of csrc/fr.hpp.
#include "codec.hpp"
#include "device_rt.hpp"
#include "host_rt.hpp"

using namespace kzgpot;

namespace {

// The scalars of one NTT of size 2^exp; scale: the plain integer the outputs are multiplied by
NttScalars ntt_scalars(uint32_t exp, bool inverse, const fr& scale) {
  NttScalars sc;
  fr_fill_powers(sc.pw, fft_root(exp, inverse));
  sc.one = fr_one();
  sc.scale = scale;
  return sc;
}
constexpr fr kPlainOne = {{1, 0, 0, 0, 0, 0, 0, 0}};
fr plain_inverse_of_size(uint32_t exp) {  // 1 / 2^exp, canonical
  fr minv;
  fr_store(minv, fr_inv(fr_from_u64((uint64_t)1 << exp)));
  return minv;
}

// ---------------------------------------------------------------- NTT
int ntt_dev(const void* d_in, uint32_t exp, void* d_out, uint32_t flags, void* d_work, void* stream) {
  uint32_t t;
  if (!ntt_flags(flags, t) || exp > kNttMaxExp || !d_in || !d_out || !d_work) return KZGPOT_E_INVALID_ARG;
  const NttPlan p = ntt_plan(exp, t);
  const bool inverse = flags & KZGPOT_NTT_INVERSE;
  const NttScalars sc = ntt_scalars(exp, inverse, inverse ? plain_inverse_of_size(exp) : kPlainOne);
  uint8_t* w = (uint8_t*)d_work;
  HIP_TRY(launch_fr_ntt(p, d_in, d_out, sc, w, p.stage_bytes ? w + p.tw_bytes : nullptr, nullptr, (hipStream_t)stream));
  return 0;
}

int ntt_host(const uint8_t* in, uint32_t exp, uint8_t* out, uint32_t flags) {
  uint32_t t;
  if (!ntt_flags(flags, t) || exp > kNttMaxExp || !in || !out) return KZGPOT_E_INVALID_ARG;
  const uint64_t bytes = (uint64_t)32 << exp;
  StagedCall call;
  void *io, *work;
  if (call.begin() || call.in(io, in, bytes) || call.alloc(work, ntt_workspace_bytes(exp, t))) return KZGPOT_E_DEVICE;
  return call.finish(ntt_dev(io, exp, io, flags, work, nullptr), nullptr, [&] { return copy_out(out, io, bytes); });
}

// ---------------------------------------------------------------- the table
bool table_args(uint32_t exp, const void* powers, const void* table) { return exp <= kOpenDomainMaxExp && powers && table; }

int table_dev(bool g2, const void* d_powers, uint32_t exp, void* d_table, void* d_work, uint64_t* d_bad_key, void* stream) {
  if (!table_args(exp, d_powers, d_table) || !d_work || !d_bad_key) return KZGPOT_E_INVALID_ARG;
  FftScalars sc;
  fft_scalars(exp + 1, false, sc);
  const hipStream_t s = (hipStream_t)stream;
  return launch_with_key(d_bad_key, s, [&](unsigned long long* key) {
    return launch_open_domain_table(g2, d_powers, exp, d_table, sc, d_work, key, s);
  });
}

int table_host(bool g2, const uint8_t* powers, uint32_t exp, uint8_t* table, int64_t* first_bad) {
  if (first_bad) *first_bad = -1;
  if (!table_args(exp, powers, table)) return KZGPOT_E_INVALID_ARG;
  const uint64_t in_bytes = point_record(g2) << exp;
  StagedCall call;
  void *d_powers, *d_table, *work;
  if (call.begin() || call.in(d_powers, powers, in_bytes) || call.alloc(d_table, 2 * in_bytes) ||
      call.alloc(work, open_domain_table_workspace_bytes(g2, exp)) || call.key())
    return KZGPOT_E_DEVICE;
  return call.finish(table_dev(g2, d_powers, exp, d_table, work, call.d_key, nullptr), first_bad,
                     [&] { return copy_out(table, d_table, 2 * in_bytes); });
}

// ---------------------------------------------------------------- the openings
// false: invalid arguments. t: the NTT's tile
bool open_args(uint32_t flags, uint32_t exp, uint64_t n_coeffs, const void* table, const void* coeffs, const void* proofs,
               uint32_t& t) {
  return open_domain_flags(flags, t) && exp <= kOpenDomainMaxExp && n_coeffs <= (uint64_t)1 << exp && table && proofs &&
         (!n_coeffs || coeffs);
}

// The steps are open_domain_plan's (plans.hpp)
int open_dev(bool g2, const void* d_table, const void* d_coeffs, uint64_t nc, uint32_t exp, void* d_proofs,
             void* d_values, uint32_t flags, void* d_work, uint64_t* d_bad_key, void* stream) {
  uint32_t t;
  if (!open_args(flags, exp, nc, d_table, d_coeffs, d_proofs, t) || !d_work || !d_bad_key) return KZGPOT_E_INVALID_ARG;
  const OpenDomainPlan p = open_domain_plan(g2, exp, t);
  FftScalars wide, out;
  fft_scalars(exp + 1, true, wide);
  fft_scalars(exp, false, out);
  // v / 2n: the inverse transform's 1/m goes into the scalars, so it runs without its scale pass
  const NttScalars sc_wide = ntt_scalars(exp + 1, false, wide.minv), sc_out = ntt_scalars(exp, false, kPlainOne);
  const NttPlan ntt_wide = ntt_plan(exp + 1, t), ntt_out = ntt_plan(exp, t);
  const hipStream_t s = (hipStream_t)stream;
  uint8_t* w = (uint8_t*)d_work;
  uint8_t *ntt_in = w + p.ntt_in, *scalars = w + p.scalars, *ntt_tw = w + p.ntt_tw;
  const uint8_t* c = (const uint8_t*)d_coeffs;
  return launch_with_key(d_bad_key, s, [&](unsigned long long* key) -> hipError_t {
    hipError_t e = hipSuccess;
    for (uint32_t k = 0; k < kDomainSteps && !e; k++) switch (p.step[k]) {
        case DomainStep::ScalarsNtt:  // b = (c_1 .. c_{n-1}, 0 ..), 2n elements
          if ((e = hipMemsetAsync(ntt_in, 0, 2 * p.n * 32, s))) break;
          if (nc > 1 && (e = hipMemcpyAsync(ntt_in, c + 32, (nc - 1) * 32, hipMemcpyDeviceToDevice, s))) break;
          e = launch_fr_ntt(ntt_wide, ntt_in, scalars, sc_wide, ntt_tw, nullptr, nullptr, s);
          break;
        case DomainStep::ValuesNtt:  // (c_0 .. c_{n-1}); the last step, so it sees a rejection
          if (!d_values) break;
          if ((e = hipMemsetAsync(ntt_in, 0, p.n * 32, s))) break;
          if (nc && (e = hipMemcpyAsync(ntt_in, c, nc * 32, hipMemcpyDeviceToDevice, s))) break;
          e = launch_fr_ntt(ntt_out, ntt_in, d_values, sc_out, ntt_tw, nullptr, key, s);
          break;
        default:
          e = launch_open_domain_step(g2, p, p.step[k], d_table, d_proofs, wide, out, d_work, key, s);
      }
    return e;
  });
}

int open_host(bool g2, const uint8_t* table, const uint8_t* coeffs, uint64_t nc, uint32_t exp, uint8_t* proofs,
              uint8_t* values, uint32_t flags, int64_t* first_bad) {
  if (first_bad) *first_bad = -1;
  uint32_t t;
  if (!open_args(flags, exp, nc, table, coeffs, proofs, t)) return KZGPOT_E_INVALID_ARG;
  const uint64_t n = (uint64_t)1 << exp, rec = point_record(g2);
  StagedCall call;
  // no coefficients, no values wanted: no buffer (open_dev takes a null pointer for either)
  void *d_table, *d_coeffs = nullptr, *d_proofs, *d_values = nullptr, *work;
  if (call.begin() || call.in(d_table, table, 2 * n * rec) || (nc && call.in(d_coeffs, coeffs, nc * 32)) ||
      call.alloc(d_proofs, n * rec) || (values && call.alloc(d_values, n * 32)) ||
      call.alloc(work, open_domain_plan(g2, exp, t).bytes) || call.key())
    return KZGPOT_E_DEVICE;
  const auto out = [&] {
    if (const int r = copy_out(proofs, d_proofs, n * rec)) return r;
    return values ? copy_out(values, d_values, n * 32) : 0;
  };
  return call.finish(open_dev(g2, d_table, d_coeffs, nc, exp, d_proofs, d_values, flags, work, call.d_key, nullptr),
                     first_bad, out);
}

}  // namespace

extern "C" {

/* host only */
uint64_t kzgpot_fr_ntt_workspace(uint32_t exp, uint32_t flags) {
  uint32_t t;
  return ntt_flags(flags, t) ? ntt_workspace_bytes(exp, t) : 0;
}
uint64_t kzgpot_open_domain_table_workspace(int g2, uint32_t exp) { return open_domain_table_workspace_bytes(g2 != 0, exp); }
uint64_t kzgpot_open_domain_workspace(int g2, uint32_t exp, uint32_t flags) {
  return open_domain_workspace_bytes(g2 != 0, exp, flags);
}

int kzgpot_fr_ntt_dev(const void* d_in, uint32_t exp, void* d_out, uint32_t flags, void* d_work, void* stream) {
  return api_guard([&] { return ntt_dev(d_in, exp, d_out, flags, d_work, stream); });
}
int kzgpot_fr_ntt(const uint8_t* in, uint32_t exp, uint8_t* out, uint32_t flags) {
  return api_guard([&] { return ntt_host(in, exp, out, flags); });
}

int kzgpot_g1_open_domain_table_dev(const void* d_powers, uint32_t exp, void* d_table, void* d_work, uint64_t* d_bad_key,
                                    void* stream) {
  return api_guard([&] { return table_dev(false, d_powers, exp, d_table, d_work, d_bad_key, stream); });
}
int kzgpot_g2_open_domain_table_dev(const void* d_powers, uint32_t exp, void* d_table, void* d_work, uint64_t* d_bad_key,
                                    void* stream) {
  return api_guard([&] { return table_dev(true, d_powers, exp, d_table, d_work, d_bad_key, stream); });
}
int kzgpot_g1_open_domain_table(const uint8_t* powers, uint32_t exp, uint8_t* table, int64_t* first_bad) {
  return api_guard([&] { return table_host(false, powers, exp, table, first_bad); });
}
int kzgpot_g2_open_domain_table(const uint8_t* powers, uint32_t exp, uint8_t* table, int64_t* first_bad) {
  return api_guard([&] { return table_host(true, powers, exp, table, first_bad); });
}

int kzgpot_g1_open_domain_dev(const void* d_table, const void* d_coeffs, uint64_t n_coeffs, uint32_t exp, void* d_proofs,
                              void* d_values, uint32_t flags, void* d_work, uint64_t* d_bad_key, void* stream) {
  return api_guard(
      [&] { return open_dev(false, d_table, d_coeffs, n_coeffs, exp, d_proofs, d_values, flags, d_work, d_bad_key, stream); });
}
int kzgpot_g2_open_domain_dev(const void* d_table, const void* d_coeffs, uint64_t n_coeffs, uint32_t exp, void* d_proofs,
                              void* d_values, uint32_t flags, void* d_work, uint64_t* d_bad_key, void* stream) {
  return api_guard(
      [&] { return open_dev(true, d_table, d_coeffs, n_coeffs, exp, d_proofs, d_values, flags, d_work, d_bad_key, stream); });
}
int kzgpot_g1_open_domain(const uint8_t* table, const uint8_t* coeffs, uint64_t n_coeffs, uint32_t exp, uint8_t* proofs,
                          uint8_t* values, uint32_t flags, int64_t* first_bad) {
  return api_guard([&] { return open_host(false, table, coeffs, n_coeffs, exp, proofs, values, flags, first_bad); });
}
int kzgpot_g2_open_domain(const uint8_t* table, const uint8_t* coeffs, uint64_t n_coeffs, uint32_t exp, uint8_t* proofs,
                          uint8_t* values, uint32_t flags, int64_t* first_bad) {
  return api_guard([&] { return open_host(true, table, coeffs, n_coeffs, exp, proofs, values, flags, first_bad); });
}

}  // extern "C"

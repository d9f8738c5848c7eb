// The powersoftau Accumulator as a contribution file holds it: a 64-B hash, five sections of
// pairing-compressed points, then the contributor's public key. Stated once; the file pipeline
// (preprocess.hip), the phase1radix2m writer (phase2.hip) and the size functions read it. Host only.
#pragma once
#include <stdint.h>

namespace kzgpot {

// TAU_POWERS_G1_LENGTH for TAU_POWERS_LENGTH = n (src/lib.rs:179-184): the setup files' tau G1 count too
constexpr uint64_t tau_powers_g1_length(uint64_t n) { return 2 * n - 1; }

struct Accumulator {
  static constexpr int kSections = 5;  // tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2: file order
  static constexpr uint64_t kHashBytes = 64;                      // before the sections
  static constexpr uint64_t kPublicKeyBytes = 3 * 192 + 6 * 96;   // after them (uncompressed)
  uint64_t cnt[kSections];                                        // points per section
  explicit constexpr Accumulator(uint64_t n) : cnt{tau_powers_g1_length(n), n, n, n, 1} {}
  static constexpr bool g2(int s) { return s == 1 || s == 4; }
  static constexpr uint64_t record(int s) { return g2(s) ? 96 : 48; }  // compressed bytes per point
  static const char* range_name(int s) {                               // trace range of a section's decode
    static const char* const k[kSections] = {"kzgpot.section.tau_g1", "kzgpot.section.tau_g2",
                                             "kzgpot.section.alpha_tau_g1", "kzgpot.section.beta_tau_g1",
                                             "kzgpot.section.beta_g2"};
    return k[s];
  }
  // byte offset of section s in the contribution; offset(kSections) is where the public key starts
  constexpr uint64_t offset(int s) const {
    uint64_t o = kHashBytes;
    for (int k = 0; k < s; k++) o += cnt[k] * record(k);
    return o;
  }
  constexpr uint64_t size() const { return offset(kSections) + kPublicKeyBytes; }
};

}  // namespace kzgpot

// The index arithmetic of one pass of the Fr NTT (ntt_plan, plans.hpp), stated once for the kernel
// (ntt_kernels.hip) and for the CPU program that executes the same plan (tests/host_units/
// ntt_units.cpp): which element a block's slot loads and stores, which slots a butterfly joins and
// which power of w it multiplies by.
//
// The schedule is decimation in time over X[pos] = in[bitrev(pos)]: stage q joins X[pos] and
// X[pos + 2^q] for every pos with bit q clear, (a, b) -> (a + w^e b, a - w^e b) with
// e = (pos mod 2^q) 2^(exp - 1 - q), and after stage exp - 1 X is the transform in natural order.
//
// Plain C++17 unless the compiler is hipcc (as fr.hpp, which defines KZG_HD).
#pragma once
#include "fr.hpp"
#include "plans.hpp"

namespace kzgpot {

// the low `bits` bits of x reversed, bits <= 32
KZG_HD uint64_t ntt_bitrev(uint64_t x, uint32_t bits) {
  uint32_t v = (uint32_t)x;
  v = (v >> 16) | (v << 16);
  v = ((v & 0xff00ff00u) >> 8) | ((v & 0x00ff00ffu) << 8);
  v = ((v & 0xf0f0f0f0u) >> 4) | ((v & 0x0f0f0f0fu) << 4);
  v = ((v & 0xccccccccu) >> 2) | ((v & 0x33333333u) << 2);
  v = ((v & 0xaaaaaaaau) >> 1) | ((v & 0x55555555u) << 1);
  return bits ? v >> (32 - bits) : 0;
}

// the position in X of slot s = (k << lb) | l of block blk: l in the bits [0, lb), k in the bits
// [q0, q0 + c), the block's bits in the rest (pass 0 has lb = 0)
KZG_HD uint64_t ntt_pos(const NttPass& p, uint64_t blk, uint32_t s) {
  const uint64_t k = s >> p.lb, l = s & ((1u << p.lb) - 1);
  const uint32_t mid = p.q0 - p.lb;  // the block's bits below the stages
  const uint64_t blk_lo = blk & (((uint64_t)1 << mid) - 1), blk_hi = blk >> mid;
  return l | (blk_lo << p.lb) | (k << p.q0) | (blk_hi << (p.q0 + p.c));
}
// the element slot s loads (pass 0: of the caller's input) and the element it is stored to
KZG_HD uint64_t ntt_load_index(const NttPass& p, uint32_t exp, uint64_t blk, uint32_t s) {
  const uint64_t pos = ntt_pos(p, blk, s);
  return p.q0 == 0 ? ntt_bitrev(pos, exp) : pos;
}
KZG_HD uint64_t ntt_store_index(const NttPass& p, uint64_t blk, uint32_t s) { return ntt_pos(p, blk, s); }

// butterfly b < 2^(tl - 1) of the pass's stage j < c: its lower slot (the upper one is
// ntt_slot_gap above), and the exponent e < m / 2 of its twiddle w^e
KZG_HD uint32_t ntt_slot_gap(const NttPass& p, uint32_t j) { return 1u << (p.lb + j); }
KZG_HD uint32_t ntt_lower_slot(const NttPass& p, uint32_t j, uint32_t b) {
  const uint32_t bit = p.lb + j;
  return ((b >> bit) << (bit + 1)) | (b & ((1u << bit) - 1));
}
KZG_HD uint64_t ntt_twiddle_exp(const NttPass& p, uint32_t exp, uint64_t blk, uint32_t j, uint32_t b) {
  const uint32_t q = p.q0 + j;
  const uint64_t pos = ntt_pos(p, blk, ntt_lower_slot(p, j, b));
  return (pos & (((uint64_t)1 << q) - 1)) << (exp - 1 - q);
}
// w^e = lo[e mod 2^lo_bits] hi[e >> lo_bits]
KZG_HD uint32_t ntt_tw_lo(uint32_t lo_bits, uint64_t e) { return (uint32_t)(e & (((uint64_t)1 << lo_bits) - 1)); }
KZG_HD uint32_t ntt_tw_hi(uint32_t lo_bits, uint64_t e) { return (uint32_t)(e >> lo_bits); }

}  // namespace kzgpot

// Test build only (libkzgpot_test.so, -DKZGPOT_TEST_HOOKS; tests/kzgpot_test_pairing_hooks.h): one
// function of pairing_parts.hpp per lane on caller-supplied cells, so that
// tests/test_gpu_pairing_cells.py can compare every cell of every lane with tests/pairing_kernel_model.py
// — the whole-call tests see 576 GT bytes of a real pairing: they cannot hand a cell function the value
// forms 0, p, p + 1 or 2 p - 1, a structured element, or a lane whose neighbours hold other data.
#ifdef KZGPOT_TEST_HOOKS
#include "../../tests/kzgpot_test_pairing_hooks.h"
#include "device_rt.hpp"
#include "pairing_parts.hpp"

using namespace kzgpot;

namespace {

static_assert(KZGPOT_PAIR_CELLS == kPairFinalCells && KZGPOT_PAIR_CELL_WORDS == kCellWords, "the header's layout");
static_assert(kMillerCells <= KZGPOT_PAIR_CELLS && kFinalCells <= KZGPOT_PAIR_CELLS, "both layouts fit a lane");

// cells taken by arg[0], arg[1], arg[2] (0: the op does not take the argument)
struct Extent {
  int n[3];
};
constexpr Extent extent(int op) {
  switch (op) {
    case KZGPOT_PAIR_C_MUL:
    case KZGPOT_PAIR_C_ADD:
    case KZGPOT_PAIR_C_SUB:
    case KZGPOT_PAIR_C_MUL_FQ: return {{1, 1, 1}};
    case KZGPOT_PAIR_C_SQR:
    case KZGPOT_PAIR_C_NEG:
    case KZGPOT_PAIR_C_MUL_XI:
    case KZGPOT_PAIR_C_HALF:
    case KZGPOT_PAIR_C_INV: return {{1, 1, 0}};
    case KZGPOT_PAIR_X_MUL6: return {{6, 6, 6}};
    case KZGPOT_PAIR_X_MUL3: return {{3, 3, 3}};
    case KZGPOT_PAIR_X_SQR3: return {{3, 3, 0}};
    case KZGPOT_PAIR_X_MUL_LINE: return {{6, 6, 3}};
    case KZGPOT_PAIR_X6_INV: return {{3, 3, 5}};
    case KZGPOT_PAIR_X12_INV: return {{6, 6, 17}};
    case KZGPOT_PAIR_X_SQR6:
    case KZGPOT_PAIR_X_FROB:
    case KZGPOT_PAIR_X_CONJ:
    case KZGPOT_PAIR_X12_POW_X: return {{6, 6, 0}};
    default: return {{0, 0, 0}};
  }
}

__global__ void __launch_bounds__(kPairMillerBlock) k_pair_op(int op, int d, int a, int b, int w, uint64_t lanes,
                                                               uint32_t* cells, uint64_t stride) {
  const uint64_t i = (uint64_t)blockIdx.x * kPairMillerBlock + threadIdx.x;
  if (i >= lanes) return;
  const Cells m{cells + i, stride};
  switch (op) {
    case KZGPOT_PAIR_C_MUL: c_mul(m, d, a, b); break;
    case KZGPOT_PAIR_C_SQR: c_sqr(m, d, a); break;
    case KZGPOT_PAIR_C_ADD: c_add(m, d, a, b); break;
    case KZGPOT_PAIR_C_SUB: c_sub(m, d, a, b); break;
    case KZGPOT_PAIR_C_NEG: c_neg(m, d, a); break;
    case KZGPOT_PAIR_C_MUL_XI: c_mul_xi(m, d, a); break;
    case KZGPOT_PAIR_C_HALF: c_half(m, d, a); break;
    case KZGPOT_PAIR_C_MUL_FQ: c_mul_fq(m, d, a, b, w); break;
    case KZGPOT_PAIR_C_INV: c_inv(m, d, a); break;
    case KZGPOT_PAIR_X_MUL6: x_mul(m, d, m, a, m, b, 6, false); break;
    case KZGPOT_PAIR_X_SQR6: x_mul(m, d, m, a, m, a, 6, true); break;
    case KZGPOT_PAIR_X_MUL3: x_mul(m, d, m, a, m, b, 3, false); break;
    case KZGPOT_PAIR_X_SQR3: x_mul(m, d, m, a, m, a, 3, true); break;
    case KZGPOT_PAIR_X_MUL_LINE: x_mul_line(m, d, a, b); break;
    case KZGPOT_PAIR_X_FROB: x_frob(m, d, a, w); break;
    case KZGPOT_PAIR_X_CONJ: x_conj(m, d, a); break;
    case KZGPOT_PAIR_X6_INV: x6_inv(m, d, a, b); break;
    case KZGPOT_PAIR_X12_INV: x12_inv(m, d, a, b); break;
    case KZGPOT_PAIR_X12_POW_X: x12_pow_x(m, d, a); break;
    case KZGPOT_PAIR_MILLER_DOUBLE: miller_double(m); break;
    case KZGPOT_PAIR_MILLER_ADD: miller_add(m); break;
    default: break;
  }
}

}  // namespace

extern "C" int kzgpot_test_pairing_op(int op, const int32_t arg[4], long lanes, long stride, long count, uint32_t* cells) {
  if (op < 0 || op >= KZGPOT_PAIR_OP_COUNT || !cells || lanes <= 0 || stride < lanes || stride > KZGPOT_PAIR_MAX_STRIDE)
    return KZGPOT_E_INVALID_ARG;
  const Extent ext = extent(op);
  int32_t v[4] = {0, 0, 0, 0};
  for (int k = 0; k < 3; k++) {
    if (!ext.n[k]) continue;
    if (!arg || arg[k] < 0 || arg[k] + ext.n[k] > KZGPOT_PAIR_CELLS) return KZGPOT_E_INVALID_ARG;
    v[k] = arg[k];
  }
  if (op == KZGPOT_PAIR_C_MUL_FQ || op == KZGPOT_PAIR_X_FROB) {
    const int lo = op == KZGPOT_PAIR_X_FROB ? 1 : 0;
    if (!arg || arg[3] < lo || arg[3] > lo + 1) return KZGPOT_E_INVALID_ARG;
    v[3] = arg[3];
  }
  if (op == KZGPOT_PAIR_TREE && (count < 1 || count > lanes)) return KZGPOT_E_INVALID_ARG;
  if (device_count() <= 0) return KZGPOT_E_DEVICE;
  const size_t bytes = (size_t)KZGPOT_PAIR_CELLS * kPairCellBytes * (size_t)stride;
  DevBuf dev;
  if (dev.alloc(bytes)) return KZGPOT_E_DEVICE;
  HIP_TRY(hipMemcpy(dev.p, cells, bytes, hipMemcpyHostToDevice));
  if (op == KZGPOT_PAIR_TREE)
    launch_pair_tree(pairing_plan((uint64_t)count), (uint32_t*)dev.p, (uint64_t)stride, nullptr);
  else
    hipLaunchKernelGGL(k_pair_op, dim3(grid_for((uint64_t)lanes, kPairMillerBlock)), dim3(kPairMillerBlock), 0, nullptr, op,
                       v[0], v[1], v[2], v[3], (uint64_t)lanes, (uint32_t*)dev.p, (uint64_t)stride);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipMemcpy(cells, dev.p, bytes, hipMemcpyDeviceToHost));
  return 0;
}
#endif  // KZGPOT_TEST_HOOKS

// run_host (capi.hip): one codec op over host buffers through the two-slot staging pipeline. Declared
// here for the ABI units that call it (capi.hip, preprocess.hip).
#pragma once
#include <functional>

#include "codec.hpp"
#include "host_rt.hpp"

namespace kzgpot {

// What a run_host call may set beside its buffers.
struct HostRunOpts {
  // called with (first point, count) of each chunk once its output is in `out`, in order — the
  // end-to-end preprocess streams the output digest from it
  const std::function<void(size_t, size_t)>* on_chunk = nullptr;
  bool keep_out = true;               // false: the records are validated but not copied back (out may be null)
  const InputWait* in_wait = nullptr;  // called before each chunk's input is copied: inputs still streaming in from disk
  uint8_t* status = nullptr;           // one status byte per point
};

int run_host(int dev, CodecOp op, const uint8_t* in, size_t n, uint8_t* out, uint32_t flags, int64_t* first_bad,
             const HostRunOpts& opts = HostRunOpts());

}  // namespace kzgpot

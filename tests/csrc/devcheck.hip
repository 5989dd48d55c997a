// TEST INFRASTRUCTURE (not part of the product, never loaded by spartan_amd, not part of include/spartan_hip.h): one __global__
// microkernel per field / curve operation of spartan_amd/csrc/{field,curve,msm}.hpp, element i handled by thread i, so the DEVICE
// forms of the arithmetic (the hand-scheduled carry chains and column accumulators of field.hpp) can be compared lane by lane with
// integer models (tests/field_vectors.py, tests/test_gpu_field_lanes.py). The wrappers are the plain C++ of checkops.hpp.
//
// Built twice from this source: libdevcheck.so (the device forms under test) and libdevcheck_generic.so (-DSP_FIELD_ADD_GENERIC
// -DSP_FQ_MUL_GENERIC -DSP_FP_MUL_GENERIC: the compiler's code for the u128 forms, on the same device).
//
// mode 0: every lane below n runs the operation.
// mode 1: lanes whose bit of `pattern` (bit = lane within the 64-wide wavefront) is set run the operation, the others the ALT
//         operation of checkops.hpp on the same operands: the two run under complementary EXEC masks.
#include <hip/hip_runtime.h>

#include "checkops.hpp"

namespace {

template <class OP, class ALT>
__global__ void __launch_bounds__(256) k_check(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint8_t* __restrict__ out, size_t n, int mode,
                                               uint64_t pattern) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;  // n need not be a multiple of the wavefront or the block
  const uint8_t* pa = a + 32 * i;
  const uint8_t* pb = b + 32 * i;
  uint8_t* po = out + 32 * i;
  if (mode == 0 || ((pattern >> (threadIdx.x & 63)) & 1))
    OP::run(pa, pb, po);
  else
    ALT::run(pa, pb, po);
}

template <class OP, class ALT>
int run_check(const void* a, const void* b, void* out, size_t n, int mode, uint64_t pattern) {
  if (n == 0) return (int)hipSuccess;
  if (!a || !out || n > ((size_t)1 << 24) || (mode != 0 && mode != 1)) return (int)hipErrorInvalidValue;
  const size_t bytes = 32 * n;
  uint8_t *da = nullptr, *db = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc((void**)&da, bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&db, bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&dout, bytes);
  if (e == hipSuccess) e = hipMemcpy(da, a, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(db, b ? b : a, bytes, hipMemcpyHostToDevice);  // unary operations: b may be null
  if (e == hipSuccess) e = hipMemset(dout, 0xa5, bytes);
  if (e == hipSuccess) {
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL((k_check<OP, ALT>), dim3(blocks), dim3(256), 0, 0, da, db, dout, n, mode, pattern);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost);
  if (da) (void)hipFree(da);
  if (db) (void)hipFree(db);
  if (dout) (void)hipFree(dout);
  return (int)e;
}

}  // namespace

extern "C" {
#define DC_ENTRY(name, OP, ALT) \
  int dc_##name(const void* a, const void* b, void* out, size_t n, int mode, uint64_t pattern) { return run_check<chk::OP, chk::ALT>(a, b, out, n, mode, pattern); }
CHK_OPS(DC_ENTRY)
#undef DC_ENTRY

// which of the generic-form macros this library was compiled with: 1 SP_FIELD_ADD_GENERIC | 2 SP_FQ_MUL_GENERIC | 4 SP_FP_MUL_GENERIC
int dc_flags() {
  int f = 0;
#if defined(SP_FIELD_ADD_GENERIC)
  f |= 1;
#endif
#if defined(SP_FQ_MUL_GENERIC)
  f |= 2;
#endif
#if defined(SP_FP_MUL_GENERIC)
  f |= 4;
#endif
  return f;
}
}

// The two pieces of ray arithmetic of the sphere-tracing kernels (trace.hip over an atlas, hash_trace.hip over
// hash-indexed levels): each restates tensor ops of the reference loop with a rounding per op.
#pragma once
#include <hip/hip_runtime.h>

namespace miso {

// c + a b as the two tensor ops it restates: the product rounded, then the sum.  (HIP's __fmul_rn / __fadd_rn are plain
// operators that the compiler may contract into one v_fma_f32 -- see axis_from_norm in trilinear.hpp; the pragma is what
// keeps them apart.)
__device__ __forceinline__ float add_product(float c, float a, float b) {
#pragma clang fp contract(off)
  const float ab = a * b;
  return c + ab;
}

// |e|: three products, two sums and a root, each rounded.  torch.norm may sum in another order or in a wider type, so
// the far test agrees with the loop's wherever dist is not within rounding of max_dist.
__device__ __forceinline__ float norm3(float ex, float ey, float ez) {
#pragma clang fp contract(off)
  const float xx = ex * ex, yy = ey * ey, zz = ez * ez;
  const float sum = (xx + yy) + zz;
  return __fsqrt_rn(sum);
}

}  // namespace miso

// Where a vertex of a hash-indexed level lives (include/miso_hash.h): the rows of a level (host) and the row of a
// vertex (kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/miso_hash.h"

namespace miso {

constexpr uint32_t HASH_PRIME_Y = 2654435761u, HASH_PRIME_Z = 805459861u;      // Instant-NGP's (x is multiplied by 1)

// rows of an X x Y x Z level behind at most 2^log2 rows; *dense: the level is dense-indexed.  0 = refused.
inline int64_t hash_rows(int32_t X, int32_t Y, int32_t Z, int32_t log2, bool* dense) {
  if (X < 1 || Y < 1 || Z < 1 || log2 < MISO_HASH_LOG2_MIN || log2 > MISO_HASH_LOG2_MAX) return 0;
  const int64_t cap = (int64_t)1 << log2;
  // X Y < 2^62 and the comparison comes before the third factor: no int64 overflow for any int32 sizes
  const int64_t xy = (int64_t)X * Y;
  const bool fits = xy <= cap && xy * Z <= cap;
  if (dense) *dense = fits;
  return fits ? xy * Z : cap;
}

// mask = rows - 1 of a hashed level; 0 = dense-indexed (then i < X, j < Y, k < Z, and X Y Z <= 2^28 fits uint32)
__device__ __forceinline__ uint32_t hash_row(int i, int j, int k, int X, int Y, uint32_t mask) {
  if (mask == 0u) return ((uint32_t)k * (uint32_t)Y + (uint32_t)j) * (uint32_t)X + (uint32_t)i;
  return ((uint32_t)i ^ ((uint32_t)j * HASH_PRIME_Y) ^ ((uint32_t)k * HASH_PRIME_Z)) & mask;
}

}  // namespace miso

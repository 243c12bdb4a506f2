// A hash-indexed grid as the kernels take it (include/miso_hash.h): the kernel-side structs, the cell of a point in a
// level, the rows of its eight corners and the row load -- shared by hash_encode.hip (encode, its backward),
// hash_sdf.hip and hash_trace.hip (the gather in front of the fused decoder: hash_gather_row) -- and the host functions
// those files call across: the checks of a grid argument, of a (grid, decoder) pair, and the backward launches.
#pragma once
#include "common.hpp"
#include "hash_index.hpp"

namespace miso {

struct HashLevelK {
  const float* table;
  float* grad;
  int32_t X, Y, Z, C;
  uint32_t mask;    // rows - 1 of a hashed level, 0 = dense-indexed
  int32_t foff;     // first output column of this level
};

struct HashGridK {
  int32_t n_levels;
  uint32_t ignore_mask;
  uint32_t flags;
  int32_t F;
  float bmin[3], bmax[3];
  HashLevelK lv[MISO_MAX_LEVELS];
};

// The cell of a point in a hashed level: make_cell reads the three sizes of a LevelK and nothing else.
__device__ __forceinline__ Cell hash_cell(const HashGridK& g, const HashLevelK& lv, float px, float py, float pz,
                                          Axis (&a)[3]) {
  LevelK shape = {};
  shape.X = lv.X; shape.Y = lv.Y; shape.Z = lv.Z;
  return level_cell(g.bmin, g.bmax, g.flags, shape, px, py, pz, a);
}

// The rows of the eight corners.  A corner out of range is never hashed: as in encode.hip (reread_in_range) it re-reads
// an in-range corner of its own cell under its zero weight, so a non-finite table entry reaches the rows it reaches in
// the dense encode and no others.  false: no corner in range (outside the level, a NaN or inf coordinate).
__device__ __forceinline__ bool corner_rows(const Cell& c, const HashLevelK& lv, const bool (&inb)[8], uint32_t (&row)[8]) {
  uint32_t safe = 0;
  bool any_in = false;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    row[k] = inb[k] ? hash_row(c.i0 + (k & 1), c.j0 + ((k >> 1) & 1), c.k0 + (k >> 2), lv.X, lv.Y, lv.mask) : 0u;
    safe = inb[k] ? row[k] : safe;
    any_in = any_in || inb[k];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) row[k] = inb[k] ? row[k] : safe;
  return any_in;
}

// V consecutive floats of a row, as one load (V = 4: 16 bytes; the tables are 16-byte aligned and a row is C floats)
template <int V>
__device__ __forceinline__ void load_vec(const float* __restrict__ p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else if constexpr (V == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x; v[1] = t.y;
  } else {
    v[0] = *p;
  }
}

// The feature row of one point through the tables, as the fused kernels form it (hash_sdf.hip, hash_trace.hip): per live
// level hash_cell + the eight corner_weight<0> + corner_rows, then 16-byte row loads summed corner by corner with fma
// (the PIN_FMA form of decoder.hpp's gather_level).  f[l C + c] is added to: the caller zero-fills.  An ignored level and
// a level with no corner in range leave their columns alone, and the latter reads nothing.
template <int C, int L, int NF>
__device__ __forceinline__ void hash_gather_row(const HashGridK& g, float px, float py, float pz, float (&f)[NF]) {
#pragma unroll
  for (int l = 0; l < L; ++l) {
    if ((g.ignore_mask >> l) & 1u) continue;      // zeros
    const HashLevelK& lv = g.lv[l];
    Axis a[3];
    const Cell c = hash_cell(g, lv, px, py, pz, a);
    bool inb[8];
    float w[8];
    uint32_t row[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      inb[k] = corner_in(c, k);
      w[k] = corner_weight<0>(c, k, inb[k]).w;
    }
    if (!corner_rows(c, lv, inb, row)) continue;      // no corner in range: zeros, nothing is read
#pragma unroll
    for (int q = 0; q < C; q += 4) {
      float v[8][4];
#pragma unroll
      for (int k = 0; k < 8; ++k) load_vec<4>(lv.table + (size_t)row[k] * C + q, v[k]);
#pragma unroll
      for (int k = 0; k < 8; ++k)      // corner by corner, as gather_level sums
#pragma unroll
        for (int e = 0; e < 4; ++e) f[l * C + q + e] = __builtin_fmaf(v[k][e], w[k], f[l * C + q + e]);
    }
  }
}

// ---- hash_sdf.hip (host): what the C entries of the fused routes (hash_sdf.hip, hash_trace.hip) ask before a launch
// grid + decoder as the kernels take them: (C, L, H, NH) is the fused kernels' table key
struct HashSdfCall { HashGridK g; int C, L, H, NH; };
// every check of (grid, mlp): convert_hash_grid's code, MISO_E_UNSUPPORTED for mixed C or a shape outside the fused table
int hash_sdf_call(HashSdfCall* f, const miso_hash_grid_t* grid, const miso_mlp_t* m, bool need_table);
// the decoder arguments and the batch, before the grid is looked at
int hash_sdf_args(const float* packed, uint32_t decoder_flags, int64_t n);

// ---- hash_encode.hip (host)
// Every check of a grid argument, then the kernel-side copy.  need_table: the call reads the tables.
int convert_hash_grid(const miso_hash_grid_t* in, HashGridK* out, bool need_table);
// (the table-gradient launch has up to 8 lanes per point)
inline bool blocks_fit(int64_t n) { return n < ((int64_t)1 << 56) && (n * 8 + 255) / 256 < ((int64_t)1 << 31); }
// grad_x (gx != nullptr) and the table gradients of the levels that carry a buffer, from rows gf of pitch ld: one launch each
hipError_t launch_hash_bwd(const HashGridK& g, const float* x, int64_t n, const float* gf, int64_t ld, float* gx,
                           hipStream_t s);

}  // namespace miso

// The way d feats leave a decoder backward, shared by sdf_bwd_kernel (sdf_fused.hip), sdf_train_kernel (sdf_train.hip) and
// atlas_sdf_bwd_kernel (atlas_bwd.hip): the wavefront's LDS tile of d-feat rows, the per-(point, level) cell records
// beside it, and the row-major float-atomic scatter that reads both.  The fences and wave barriers around these steps
// stay with the kernels: each has its own order of tile, records, write-out and scatter.
#pragma once
#include <type_traits>

#include "decoder.hpp"

namespace miso {

// d-feat row pitch of the tile [64][pitch] in floats: 16-B aligned, conflict-free b128 writes
__host__ __device__ constexpr int dfeat_pitch(int F) { return ((F + 3) / 4) * 4 + 4; }
// ints per (point, level) cell record: {base offset, in-range bits (x0 x1 y0 y1 z0 z1), wx1, wy1}, {wz1, wx0, wy0, wz0}
constexpr int CELL_REC = 8;
constexpr int CELL_REC_FLAGS = 1;      // where the in-range bits sit: 0 there and the scatter passes the record over

// d feats in accumulator layout (lane (hi, row) holds, for tile t, point 32 t + row: C == 8: channels 4 hi .. 4 hi + 3 of
// level j >> 2, C == 4: channels 0 .. 3 of level 2 (j >> 2) + hi) -> rows 32 t + row of the tile, NT = 1 or 2 tiles
template <int F, int NT>
__device__ __forceinline__ void dfeat_to_tile(const f32x16 (&df)[2], float* dF, int row, int hi) {
  constexpr int FP = dfeat_pitch(F);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int gq = 0; gq < (F + 7) / 8; ++gq) {
      const int f0 = 8 * gq + 4 * hi;
      if (f0 < F)
        *reinterpret_cast<float4*>(dF + (32 * t + row) * FP + f0) =
            make_float4(df[t][4 * gq], df[t][4 * gq + 1], df[t][4 * gq + 2], df[t][4 * gq + 3]);
    }
}

// the tile's first PTS rows -> dst, PTS contiguous rows of an (N, F) buffer of which rows_left exist: coalesced 16-B stores
template <int F, int PTS>
__device__ __forceinline__ void tile_to_rows(const float* dF, float* dst, int64_t rows_left, int lane) {
  constexpr int FP = dfeat_pitch(F);
  for (int i = lane; i < PTS * F / 4; i += 64) {
    const int row = (i * 4) / F, col = (i * 4) % F;
    if (row < rows_left)
      *reinterpret_cast<float4*>(dst + row * F + col) = *reinterpret_cast<const float4*>(dF + row * FP + col);
  }
}

// the record of one (point, level); a point that is not live (past the batch, outside the submap) adds nothing
__device__ __forceinline__ void write_cell_record(int* r, const Cell& c, const LevelK& lv, bool live) {
  int flags = (c.inx[0] ? 1 : 0) | (c.inx[1] ? 2 : 0) | (c.iny[0] ? 4 : 0) | (c.iny[1] ? 8 : 0) |
              (c.inz[0] ? 16 : 0) | (c.inz[1] ? 32 : 0);
  if (!live) flags = 0;
  static_assert(CELL_REC_FLAGS == 1, "the in-range bits are the second int of the record");
  *reinterpret_cast<int4*>(r) = make_int4(c.k0 * lv.sZ + c.j0 * lv.sY + c.i0 * lv.sX, flags,
                                          __float_as_int(c.wx[1]), __float_as_int(c.wy[1]));
  *reinterpret_cast<int4*>(r + 4) = make_int4(__float_as_int(c.wz[1]), __float_as_int(c.wx[0]),
                                              __float_as_int(c.wy[0]), __float_as_int(c.wz[0]));
}

// Scatter of the tile's first `points` rows (64, or 32) into the gradients of the levels in `levels`.
// The L2 executes fp32 atomics per 64-byte request (~21 G requests/s on MI355X, tools/ubench/atomics.hip), however many
// of its 16 dwords carry data.  So the scatter runs "row-major": the 2*C consecutive lanes of a group cover the x-pair
// (i0, i0+1) x C channels = one contiguous run of 2*C floats, and one atomic instruction serves 64/(2C) (point, row)
// pairs; four (dy, dz) atomics per lane and level, the cell of every (point, level) broadcast from its record rec[point][l].
// TOUCH: mark the Adam chunks written to (touch_chunk).  no_atomics: sdf_bwd_kernel's retained dev bit, always false.
// MISO_ABL_NO_SCATTER (dev ablation, a define of the build): was the training kernel's alone; here it takes the atomics
// out of every kernel that scatters, sdf_bwd_kernel and atlas_sdf_bwd_kernel included.
// Grid: GridK where the grid is the kernel's own argument -- by value, so that its level table is still read from the
// kernel arguments (scalar loads, hoisted out of the loop) once this is inlined: through a reference the reads are
// generic loads that the atomics might alias, 2 .. 30 VGPRs more and scratch in one instantiation.  const GridK& where
// the grid lies in memory anyway (the atlas's submap table).
template <int C, int L, bool TOUCH, class Grid>
__device__ __forceinline__ void scatter_tile(Grid g, uint32_t levels, const float* dF, const int* rec, int points,
                                             int lane, bool no_atomics = false) {
  static_assert(std::is_same<Grid, GridK>::value || std::is_same<Grid, const GridK&>::value,
                "scatter_tile: Grid is GridK (a kernel argument) or const GridK& (a grid in memory)");
  constexpr int FP = dfeat_pitch(C * L), REC = CELL_REC;
  constexpr int LPR = 2 * C, SLOTS = 64 / LPR;
  const int slot = lane / LPR, dx = (lane / C) & 1, ch = lane % C;
#pragma unroll 1
  for (int pg = 0; pg < (levels ? points / SLOTS : 0); ++pg) {
    const int pt = pg * SLOTS + slot;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const LevelK& lv = g.lv[l];
      if (!((levels >> l) & 1u)) continue;
      const int* r = rec + (pt * L + l) * REC;
      const int4 r0 = *reinterpret_cast<const int4*>(r);
      const int4 r1 = *reinterpret_cast<const int4*>(r + 4);
      const int fl = r0.y;
      if (!((fl >> dx) & 1)) continue;
      const float v = dF[pt * FP + l * C + ch];
      const float wx = dx ? __int_as_float(r0.z) : __int_as_float(r1.y);
      const float wy[2] = {__int_as_float(r1.z), __int_as_float(r0.w)};
      const float wz[2] = {__int_as_float(r1.w), __int_as_float(r1.x)};
      float* base = lv.grad + r0.x + dx * lv.sX + ch;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int dy = q & 1, dz = q >> 1;
        if (((fl >> (2 + dy)) & 1) && ((fl >> (4 + dz)) & 1) && !no_atomics) {
#ifndef MISO_ABL_NO_SCATTER      // dev ablation (wrong results): everything of the scatter but the atomics
          atomic_add_f32(base + dy * lv.sY + dz * lv.sZ, v * ((wx * wy[dy]) * wz[dz]));
#else
          asm volatile("" ::"v"(base + dy * lv.sY + dz * lv.sZ), "v"(v * ((wx * wy[dy]) * wz[dz])));
#endif
          if (TOUCH && ch == 0) touch_chunk(lv, r0.x + dx * lv.sX + dy * lv.sY + dz * lv.sZ);   // C floats: one chunk
        }
      }
    }
  }
}

}  // namespace miso

// The nearest-neighbour index as its kernels read it (nn.hip, and the normals kernel of icp.hip), and what capi.hip
// calls: the plan itself is host logic and lives in capi.hip with the other argument checks.
#pragma once
#include "common.hpp"

namespace miso {

struct NnK {
  float lo[3];      // bound_min
  float cell;       // the cell actually used
  float mag;        // miso_nn_plan_t.coord_mag: the coordinate magnitude the stop test's slack scales with
  int dims[3];
  int max_rings;
  int64_t n_tgt;
};

// cell index along one axis, clamped as a float so that any input (a NaN too) indexes inside the table.  Every step is
// monotone in p: a coordinate that is not below another never gets a lower cell.
__device__ __forceinline__ int nn_cell_axis(float p, float lo, float cell, int dim) {
  const float c = floorf(__fdiv_rn(p - lo, cell));
  return (int)fminf(fmaxf(c, 0.0f), (float)(dim - 1));              // fmaxf(NaN, 0) = 0
}

__device__ __forceinline__ int nn_cell_of(const NnK& k, float x, float y, float z, int c[3]) {
  c[0] = nn_cell_axis(x, k.lo[0], k.cell, k.dims[0]);
  c[1] = nn_cell_axis(y, k.lo[1], k.cell, k.dims[1]);
  c[2] = nn_cell_axis(z, k.lo[2], k.cell, k.dims[2]);
  return (c[2] * k.dims[1] + c[1]) * k.dims[0] + c[0];
}

inline int64_t nn_a256(int64_t v) { return (v + 255) / 256 * 256; }

struct NnLayout {
  int64_t table, sums, counters, list, rows, total;
};

// byte offsets inside the workspace
inline NnLayout nn_layout(const miso_nn_plan_t& p) {
  NnLayout l;
  int64_t at = 0;
  l.table = at;    at += nn_a256((p.cells + 1) * 4);
  l.sums = at;     at += nn_a256(1024 * 4);
  l.counters = at; at += nn_a256((int64_t)MISO_NN_MAX_CHUNKS * 4);
  l.list = at;     at += nn_a256((int64_t)MISO_NN_CHUNK * 4);
  l.rows = at;     at += nn_a256(p.n_tgt * 16);
  l.total = at;
  return l;
}

inline NnK nn_k(const miso_nn_plan_t& p) {
  NnK k;
  for (int a = 0; a < 3; ++a) { k.lo[a] = p.bound_min[a]; k.dims[a] = p.dims[a]; }
  k.cell = p.cell; k.mag = p.coord_mag; k.max_rings = p.max_rings; k.n_tgt = p.n_tgt;
  return k;
}

}  // namespace miso

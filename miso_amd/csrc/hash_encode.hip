// Hash-indexed feature levels (include/miso_hash.h): multi-level trilinear encode whose corner ADDRESS goes through a
// table -- dense-indexed or hashed (hash_index.hpp) -- and everything else is the sampler of trilinear.hpp: level_cell,
// corner_in, corner_weight, the accumulation order of encode_fwd_kernel.  A table that lists a dense level's vertices
// therefore gives encode_fwd_kernel's bits.  Forward, and a first backward of one launch for grad_x and one for the table
// gradients (all levels in each); there is no second backward.  The C entry points are at the end of this file.
//
// The kernels are bound by gathers of 4 - 32 bytes at random rows (a 2^19 x 4 table is 8 MB: past an XCD's L2), so what
// counts is loads in flight: the forward runs one lane per (point, level) -- eight independent corner loads each, and
// levels x more wavefronts than a lane per point would give a small batch.  Registers (gfx950, hipcc -O3, from
// -Rpass-analysis=kernel-resource-usage): hash_fwd_kernel 66 VGPRs (7 wavefronts per SIMD), hash_bwd_tables_kernel 22 (8),
// hash_bwd_x_kernel 124 under __launch_bounds__(256, 4) (4 wavefronts; 132 and 3 without it, nothing spilled either way):
// 24 derivative weights beside 32 gathered values.
#include <string.h>

#include "hash_grid.hpp"

namespace miso {

// v w + acc with the product rounded before the sum (see fwd_level)
__device__ __forceinline__ float mul_then_add(float v, float w, float acc) {
#pragma clang fp contract(off)
  return acc + v * w;
}

// The bits of encode_fwd_kernel are the bits of its compiled form: hipcc builds its channel loops as fma chains over the
// corners -- the float4 kernel for C % 4 == 0, and the scalar kernel two channels at a time -- and the scalar kernel's
// last odd channel as eight rounded products added in turn.  Said here explicitly, so that this kernel does not depend on
// what the compiler chooses to contract: C = 1 rounds each product, every other C is an fma chain.
template <int C>
__device__ __forceinline__ void fwd_level(const float* __restrict__ table, const uint32_t (&row)[8], const float (&w)[8],
                                          float* __restrict__ o) {
  constexpr int V = C >= 4 ? 4 : C;
#pragma unroll
  for (int ch = 0; ch < C; ch += V) {
    float v[8][V];
#pragma unroll
    for (int k = 0; k < 8; ++k) load_vec<V>(table + (size_t)row[k] * C + ch, v[k]);
    float acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k)      // corner by corner, as encode_fwd_kernel sums
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] = C == 1 ? mul_then_add(v[k][e], w[k], acc[e]) : __builtin_fmaf(v[k][e], w[k], acc[e]);
#pragma unroll
    for (int e = 0; e < V; ++e) o[ch + e] = acc[e];
  }
}

// One lane per (point, level): blockIdx.y is the level.
__global__ __launch_bounds__(256) void hash_fwd_kernel(HashGridK g, const float* __restrict__ x, int64_t n,
                                                      float* __restrict__ out, int64_t ld) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int l = blockIdx.y;
  const HashLevelK& lv = g.lv[l];
  float* o = out + p * ld + lv.foff;
  bool live = !((g.ignore_mask >> l) & 1u);
  uint32_t row[8];
  float w[8];
  if (live) {
    const float px = x[p * 3 + 0], py = x[p * 3 + 1], pz = x[p * 3 + 2];
    Axis a[3];
    const Cell c = hash_cell(g, lv, px, py, pz, a);
    bool inb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      inb[k] = corner_in(c, k);
      w[k] = corner_weight<0>(c, k, inb[k]).w;
    }
    live = corner_rows(c, lv, inb, row);
  }
  if (!live) {
    for (int ch = 0; ch < lv.C; ++ch) o[ch] = 0.0f;
    return;
  }
  switch (lv.C) {
    case 1: fwd_level<1>(lv.table, row, w, o); break;
    case 2: fwd_level<2>(lv.table, row, w, o); break;
    case 4: fwd_level<4>(lv.table, row, w, o); break;
    default: fwd_level<8>(lv.table, row, w, o); break;
  }
}

// One level's share of grad_x for one point: sum_c gF[c] sum_k (dw_k / d ix) T[row_k, c], which the caller scales by
// Axis::mult -- the sums encode_bwd_kernel forms, from the first-derivative weights.
template <int C>
__device__ __forceinline__ void bwd_x_level(const float* __restrict__ table, const uint32_t (&row)[8],
                                            const float (&dwx)[8], const float (&dwy)[8], const float (&dwz)[8],
                                            const float* __restrict__ go, float& ax, float& ay, float& az) {
  constexpr int V = C >= 4 ? 4 : C;
#pragma unroll
  for (int ch = 0; ch < C; ch += V) {
    float gv[V];
#pragma unroll
    for (int e = 0; e < V; ++e) gv[e] = go[ch + e];
    float v[8][V];
#pragma unroll
    for (int k = 0; k < 8; ++k) load_vec<V>(table + (size_t)row[k] * C + ch, v[k]);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float d = gv[0] * v[k][0];
#pragma unroll
      for (int e = 1; e < V; ++e) d += gv[e] * v[k][e];
      ax += d * dwx[k]; ay += d * dwy[k]; az += d * dwz[k];
    }
  }
}

// grad_x: one lane per point, the levels in turn -- one sum per point, formed in level order.
__global__ __launch_bounds__(256, 4) void hash_bwd_x_kernel(HashGridK g, const float* __restrict__ x, int64_t n,
                                                        const float* __restrict__ gf, int64_t ld, float* __restrict__ gx) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const float px = x[p * 3 + 0], py = x[p * 3 + 1], pz = x[p * 3 + 2];
  const float* go = gf + p * ld;
  float gpx = 0.f, gpy = 0.f, gpz = 0.f;
  for (int l = 0; l < g.n_levels; ++l) {
    const HashLevelK& lv = g.lv[l];
    if ((g.ignore_mask >> l) & 1u) continue;
    Axis a[3];
    const Cell c = hash_cell(g, lv, px, py, pz, a);
    uint32_t row[8];
    float dwx[8], dwy[8], dwz[8];
    bool inb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      inb[k] = corner_in(c, k);
      const CornerW cw = corner_weight<1>(c, k, inb[k]);
      dwx[k] = cw.dx; dwy[k] = cw.dy; dwz[k] = cw.dz;
    }
    if (!corner_rows(c, lv, inb, row)) continue;      // +0 for grad_x
    float ax = 0.f, ay = 0.f, az = 0.f;
    switch (lv.C) {
      case 1: bwd_x_level<1>(lv.table, row, dwx, dwy, dwz, go + lv.foff, ax, ay, az); break;
      case 2: bwd_x_level<2>(lv.table, row, dwx, dwy, dwz, go + lv.foff, ax, ay, az); break;
      case 4: bwd_x_level<4>(lv.table, row, dwx, dwy, dwz, go + lv.foff, ax, ay, az); break;
      default: bwd_x_level<8>(lv.table, row, dwx, dwy, dwz, go + lv.foff, ax, ay, az); break;
    }
    gpx += ax * a[0].mult; gpy += ay * a[1].mult; gpz += az * a[2].mult;
  }
  gx[p * 3 + 0] = gpx; gx[p * 3 + 1] = gpy; gx[p * 3 + 2] = gpz;
}

// Table gradient: d table[row] += w gF with no-return float atomics (one global_atomic_add_f32 each).  One lane per
// (point, channel), blockIdx.y the level: the C lanes of a point add to the C consecutive floats of a row, so a
// wave-instruction is 64 / C segments of 4 C bytes -- one lane per point would make it 64 dwords in 64 rows, the slowest
// shape an atomic wave-instruction has.  Each lane forms its point's cell itself (a few dozen VALU operations beside
// eight atomics).  A level without a gradient buffer, an ignored level and lanes past n C return at once.
__global__ __launch_bounds__(256) void hash_bwd_tables_kernel(HashGridK g, const float* __restrict__ x, int64_t n,
                                                             const float* __restrict__ gf, int64_t ld) {
  const int l = blockIdx.y;
  const HashLevelK& lv = g.lv[l];
  if (!lv.grad || ((g.ignore_mask >> l) & 1u)) return;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int shift = lv.C == 8 ? 3 : (lv.C == 4 ? 2 : (lv.C == 2 ? 1 : 0));
  const int64_t p = t >> shift;
  const int e = (int)(t & (lv.C - 1));
  if (p >= n) return;
  const float px = x[p * 3 + 0], py = x[p * 3 + 1], pz = x[p * 3 + 2];
  const float gv = gf[p * ld + lv.foff + e];
  Axis a[3];
  const Cell c = hash_cell(g, lv, px, py, pz, a);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (!corner_in(c, k)) continue;      // never hashed, nothing added
    const uint32_t row = hash_row(c.i0 + (k & 1), c.j0 + ((k >> 1) & 1), c.k0 + (k >> 2), lv.X, lv.Y, lv.mask);
    atomic_add_f32(lv.grad + (size_t)row * lv.C + e, gv * corner_weight<0>(c, k, true).w);
  }
}

namespace {
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }      // NULL passes: optional pointers
}  // namespace

// Every check of a grid argument, then the kernel-side copy.  need_table: the call reads the tables.
int convert_hash_grid(const miso_hash_grid_t* in, HashGridK* out, bool need_table) {
  if (!in || in->n_levels < 1 || in->n_levels > MISO_MAX_LEVELS) return MISO_E_BADARG;
  if (in->flags & ~(MISO_F_ALIGN_CORNERS | MISO_F_PAD_BORDER | MISO_F_COORDS_NORMALIZED)) return MISO_E_BADARG;
  memset(out, 0, sizeof(*out));
  out->n_levels = in->n_levels;
  out->ignore_mask = in->ignore_mask;
  out->flags = in->flags;
  for (int a = 0; a < 3; ++a) { out->bmin[a] = in->bound_min[a]; out->bmax[a] = in->bound_max[a]; }
  int foff = 0;
  for (int l = 0; l < in->n_levels; ++l) {
    const miso_hash_level_t& s = in->level[l];
    if (s.C != 1 && s.C != 2 && s.C != 4 && s.C != 8) return MISO_E_BADARG;
    if (s.X < 1 || s.Y < 1 || s.Z < 1) return MISO_E_BADARG;
    if (s.log2_rows != 0 && (s.log2_rows < MISO_HASH_LOG2_MIN || s.log2_rows > MISO_HASH_LOG2_MAX)) return MISO_E_BADARG;
    // the rows this shape has behind a table of that size, and of that kind: a table of any other length is refused
    // (the kernels address rows < `rows` by construction of exactly these two cases)
    bool dense = false;
    const int64_t want = hash_rows(s.X, s.Y, s.Z, s.log2_rows ? s.log2_rows : MISO_HASH_LOG2_MAX, &dense);
    if (want == 0 || s.rows != want || dense != (s.log2_rows == 0)) return MISO_E_BADARG;
    if (need_table && !s.table) return MISO_E_BADARG;
    if (!aligned16(s.table) || !aligned16(s.grad)) return MISO_E_BADARG;
    HashLevelK& d = out->lv[l];
    d.table = s.table; d.grad = s.grad;
    d.X = s.X; d.Y = s.Y; d.Z = s.Z; d.C = s.C;
    d.mask = dense ? 0u : (uint32_t)(s.rows - 1);
    d.foff = foff;
    foff += s.C;
  }
  out->F = foff;
  return MISO_OK;
}

hipError_t launch_hash_bwd(const HashGridK& g, const float* x, int64_t n, const float* gf, int64_t ld, float* gx,
                           hipStream_t s) {
  if (gx) {
    hash_bwd_x_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(g, x, n, gf, ld, gx);
    if (hipError_t e = hipGetLastError()) return e;
  }
  int cmax = 0;      // the widest level that takes a gradient sizes the launch: n C lanes per level
  for (int l = 0; l < g.n_levels; ++l)
    if (g.lv[l].grad && !((g.ignore_mask >> l) & 1u) && g.lv[l].C > cmax) cmax = g.lv[l].C;
  if (cmax == 0) return hipSuccess;
  hash_bwd_tables_kernel<<<dim3((unsigned)((n * cmax + 255) / 256), (unsigned)g.n_levels), 256, 0, s>>>(g, x, n, gf, ld);
  return hipGetLastError();
}

}  // namespace miso

using namespace miso;

extern "C" {

int64_t miso_hash_rows(int32_t X, int32_t Y, int32_t Z, int32_t log2_hashmap_size) {
  return hash_rows(X, Y, Z, log2_hashmap_size, nullptr);
}

int miso_hash_encode_fwd(const miso_hash_grid_t* grid, const float* x, int64_t n, float* feats, int64_t ld_out,
                         void* stream) {
  if (n < 0 || (n > 0 && (!x || !feats))) return MISO_E_BADARG;
  HashGridK g;
  if (int rc = convert_hash_grid(grid, &g, true)) return rc;
  if (ld_out < g.F) return MISO_E_BADARG;
  if (!blocks_fit(n)) return MISO_E_TOOLARGE;
  if (n == 0) return MISO_OK;
  hash_fwd_kernel<<<dim3((unsigned)((n + 255) / 256), (unsigned)g.n_levels), 256, 0, (hipStream_t)stream>>>(g, x, n, feats,
                                                                                                         ld_out);
  return (int)hipGetLastError();
}

int miso_hash_encode_bwd(const miso_hash_grid_t* grid, const float* x, int64_t n, const float* grad_feats, int64_t ld_g,
                         float* grad_x, void* stream) {
  if (n < 0 || (n > 0 && (!x || !grad_feats))) return MISO_E_BADARG;
  HashGridK g;
  if (int rc = convert_hash_grid(grid, &g, grad_x != nullptr)) return rc;
  if (ld_g < g.F) return MISO_E_BADARG;
  if (!blocks_fit(n)) return MISO_E_TOOLARGE;
  if (n == 0) return MISO_OK;
  return (int)launch_hash_bwd(g, x, n, grad_feats, ld_g, grad_x, (hipStream_t)stream);
}

}  // extern "C"

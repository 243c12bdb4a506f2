// The nearest-neighbour index as its kernels read it (nn.hip, knn.hip, and the normals kernel of icp.hip), and what
// capi.hip calls: the plan itself is host logic and lives in capi.hip with the other argument checks.
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

// ---- what the query kernels share (nn.hip, knn.hip, the radius normals of icp.hip) ---------------------------------------
// Every function here forms its result with one rounding per operation whatever the including file has set.
__device__ __forceinline__ float nn_dist2(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

struct Best {
  float d2; int idx;
  // target t as a candidate of query q: the smallest (d2, idx); false for a NaN d2, and for +inf against the initial (+inf, -1)
  __device__ __forceinline__ void take(float qx, float qy, float qz, const float4& t, int) {
    const float n2 = nn_dist2(qx, qy, qz, t.x, t.y, t.z); const int ni = __float_as_int(t.w);
    if (n2 < d2 || (n2 == d2 && ni < idx)) { d2 = n2; idx = ni; }
  }
};

__device__ __forceinline__ bool nn_finite3(float x, float y, float z) {
  const float inf = __builtin_huge_valf();
  return fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf;       // false for NaN
}

// After ring r the examined box is [c - r, c + r] (clamped to the grid).  A target outside it lies beyond a face of the box
// that is not on the grid's edge, so in real arithmetic it is at least g away, g the smallest distance from the query to
// such a face; with every face on the edge nothing is left.  In fp32 three things move that bound:
//   * membership.  A target t is below the face of cell k when floor(fl(fl(t - lo) / cell)) < k, which allows
//     t - lo < k cell (1 + 2.1 u), u = 2^-24: it may sit up to 2.1 u (k cell) beyond the plane lo + k cell.
//   * the face.  fl(q - fl(lo + fl(k cell))) is off by at most u (k cell + |lo + k cell| + g).
//   * the distance.  A computed d2 is within 5.1 u (relative) of the true one.
// With A = the largest coordinate magnitude of the grid plus its largest extent (NnK.mag, from the host plan) the first two
// are below u (4.1 A + g); the test takes 8 u (A + g) = 2^-21 (A + g) off g, which also covers the roundings of the test
// itself, and 16 u = 2^-20 (relative) off its square.  The comparison is strict: a target left out has a computed d2
// above `best`, so it loses whatever its index.
// g of the text above for any grid struct with lo, cell and dims (NnK; mesh.hpp's MeshK): +inf when the box is the grid
template <class K>
__device__ __forceinline__ float ring_gap(const K& k, const float q[3], const int c[3], int r) {
#pragma clang fp contract(off)
  float g = __builtin_huge_valf();
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (c[a] - r > 0) g = fminf(g, q[a] - (k.lo[a] + (float)(c[a] - r) * k.cell));
    if (c[a] + r < k.dims[a] - 1) g = fminf(g, (k.lo[a] + (float)(c[a] + r + 1) * k.cell) - q[a]);
  }
  return g;
}

__device__ __forceinline__ bool ring_finished(const NnK& k, const float q[3], const int c[3], int r, float best) {
#pragma clang fp contract(off)
  const float g = ring_gap(k, q, c, r);
  if (g == __builtin_huge_valf()) return true;    // the box is the grid
  const float gs = g - 0x1p-21f * (k.mag + g);
  if (!(gs > 0.0f)) return false;
  return best < (gs * gs) * (1.0f - 0x1p-20f);
}

// The cells first_cell .. last_cell of one x run are one run of rows: f(t, row) for each, ascending.  The run is clamped
// to [0, n_rows), so that a table no build wrote (a plan lives in the caller's memory) never leads outside the rows.
template <class F>
__device__ __forceinline__ void nn_visit_run(const int* table, const float4* rows, int n_rows, int first_cell, int last_cell,
                                             const F& f) {
  const int s = table[first_cell], e = min(table[last_cell + 1], n_rows);
  for (int j = max(s, 0); j < e; ++j) f(rows[j], j);
}

// Shell r of cell c, the cells at Chebyshev distance r clamped to the grid: per (y, z) of lo .. hi either the whole x run
// or its two end cells (nn_visit_shell_row).  A rings kernel walks the shells r = 0 .. max_rings of a finite query's
// cell and after each asks ring_finished with the largest d2 its accumulator still admits: +inf while that is not full
// (a list shorter than k), which finishes only when the box is the grid.  The loops over r, z and y stay in the kernels,
// and the query goes down as three scalars (profiles/nn_shared_walk.json holds the reasons).
struct NnShell { int lo[3], hi[3]; };
template <class K>
__device__ __forceinline__ NnShell nn_shell(const K& k, const int c[3], int r) {
  return {{max(c[0] - r, 0), max(c[1] - r, 0), max(c[2] - r, 0)},
          {min(c[0] + r, k.dims[0] - 1), min(c[1] + r, k.dims[1] - 1), min(c[2] + r, k.dims[2] - 1)}};
}

// a run of cells offered to an accumulator
template <class A>
__device__ __forceinline__ void nn_offer_run(const int* table, const float4* rows, int n_rows, int first_cell, int last_cell,
                                             float qx, float qy, float qz, A& acc) {
  nn_visit_run(table, rows, n_rows, first_cell, last_cell, [&](const float4& t, int row) { acc.take(qx, qy, qz, t, row); });
}

template <class A>
__device__ __forceinline__ void nn_visit_shell_row(const NnK& k, const int* table, const float4* rows, const int c[3], int r,
                                                   const NnShell& s, int z, int y, const float q[3], A& acc) {
  const int row = (z * k.dims[1] + y) * k.dims[0];
  if (abs(z - c[2]) == r || abs(y - c[1]) == r) {                    // a whole x run of the shell
    nn_offer_run(table, rows, (int)k.n_tgt, row + s.lo[0], row + s.hi[0], q[0], q[1], q[2], acc);
  } else {                                                            // (r > 0 here) the two end cells of the run
    if (c[0] - r >= 0) nn_offer_run(table, rows, (int)k.n_tgt, row + c[0] - r, row + c[0] - r, q[0], q[1], q[2], acc);
    if (c[0] + r < k.dims[0]) nn_offer_run(table, rows, (int)k.n_tgt, row + c[0] + r, row + c[0] + r, q[0], q[1], q[2], acc);
  }
}

// What every lane of a rings block ends with: the chunk's unfinished queries append their position li to its list.  One
// atomic per wavefront and counter (stats = {finished, listed}, null only where allowed); a slot is written inside [0, count).
template <bool STATS_MAY_BE_NULL>
__device__ __forceinline__ void nn_defer(bool live, bool done, int li, int count, int* __restrict__ list, int* __restrict__ list_n,
                                         int* __restrict__ stats) {
  const uint64_t fin = __ballot(live && done), rest = __ballot(live && !done);
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == 0) {
    if (fin && (!STATS_MAY_BE_NULL || stats)) atomicAdd(&stats[0], __popcll(fin));
    if (rest) {
      if (!STATS_MAY_BE_NULL || stats) atomicAdd(&stats[1], __popcll(rest));
      base = atomicAdd(list_n, __popcll(rest));
    }
  }
  base = __shfl(base, 0);
  if (live && !done) {
    const int at = base + __popcll(rest & ((1ull << lane) - 1));
    if (at >= 0 && at < count) list[at] = li;
  }
}

// The listed queries of a chunk of n, as the kernels behind the rings read them: both values live in the caller's
// memory, so both are clamped.
__device__ __forceinline__ int64_t nn_listed_count(const int* __restrict__ list_n, int64_t n) {
  const int c = *list_n; return c < 0 ? 0 : (c > n ? n : c);
}
__device__ __forceinline__ int64_t nn_listed_query(const int* __restrict__ list, int64_t slot, int64_t first, int64_t n) {
  const int li = list[slot]; return first + (li < 0 ? 0 : (li >= n ? n - 1 : li));
}

// The query of a lane of an all-pairs block of LANES: slot `blockIdx.x LANES + lane` of the chunk's list (LISTED), or
// of its n queries.  false: the block has no query and leaves as a whole, before any barrier.
template <bool LISTED, int LANES>
__device__ __forceinline__ bool nn_block_query(const float* __restrict__ src, int64_t ld_s, int64_t first, int64_t n,
                                               const int* __restrict__ list, const int* __restrict__ list_n, bool& live, int64_t& i,
                                               float q[3]) {
  const int64_t count = LISTED ? nn_listed_count(list_n, n) : n;
  if ((int64_t)blockIdx.x * LANES >= count) return false;
  const int64_t slot = (int64_t)blockIdx.x * LANES + threadIdx.x;
  live = slot < count;
  i = 0; q[0] = q[1] = q[2] = 0.0f;
  if (live) {
    i = LISTED ? nn_listed_query(list, slot, first, n) : first + slot;
    q[0] = src[i * ld_s]; q[1] = src[i * ld_s + 1]; q[2] = src[i * ld_s + 2];
  }
  return true;
}

// tile[0 .. len) = targets t0 .. t0 + len, {x, y, z, original index bits}: the index's rows (LISTED), or built from the
// caller's (m, 3) cloud with row stride ld_t.  The first barrier waits for the readers of the previous tile.
template <bool LISTED, int LANES>
__device__ __forceinline__ void nn_stage_tile(float4* tile, int len, const float4* __restrict__ rows, const float* __restrict__ tgt,
                                              int64_t ld_t, int64_t t0) {
  __syncthreads();
  for (int j = threadIdx.x; j < len; j += LANES) {
    if (LISTED) tile[j] = rows[t0 + j];
    else tile[j] = make_float4(tgt[(t0 + j) * ld_t], tgt[(t0 + j) * ld_t + 1], tgt[(t0 + j) * ld_t + 2], __int_as_float((int)(t0 + j)));
  }
  __syncthreads();
}

// nn.hip: (+inf, -1) into `total` slots (no target: every slot is padding); stats = {a, b}
hipError_t launch_nn_fill(int64_t total, float* out_d2, int64_t* out_idx, hipStream_t s);
hipError_t launch_nn_set_stats(int32_t* stats, int a, int b, hipStream_t s);
// nn.hip: the exclusive scan of the build, in place over counts[0 .. n), n <= MISO_NN_MAX_CELLS (mesh.hip's build too)
hipError_t launch_nn_scan(int* counts, int n, int* sums, hipStream_t s);

// ---- normals from a neighbourhood's sums (icp.hip: radius; knn.hip: k nearest) -------------------------------------------
// 1, d and d d^T of a neighbourhood, d = t - q in float64, added in the order add() is called
struct NormalSums {
  double cnt, s[3], ss[6];
  __device__ __forceinline__ void clear() {
    cnt = 0.0;
    s[0] = s[1] = s[2] = 0.0;
    ss[0] = ss[1] = ss[2] = ss[3] = ss[4] = ss[5] = 0.0;
  }
  __device__ __forceinline__ void add(const double d[3]) {
#pragma clang fp contract(off)
    cnt += 1.0;
    s[0] += d[0]; s[1] += d[1]; s[2] += d[2];
    ss[0] += d[0] * d[0]; ss[1] += d[0] * d[1]; ss[2] += d[0] * d[2];
    ss[3] += d[1] * d[1]; ss[4] += d[1] * d[2]; ss[5] += d[2] * d[2];
  }
};

// unit eigenvector of the smallest eigenvalue of the symmetric matrix {c00 c01 c02; . c11 c12; . . c22}; false: none
__device__ __forceinline__ bool smallest_eigenvector(double c00, double c01, double c02, double c11, double c12, double c22,
                                                     double v[3]) {
#pragma clang fp contract(off)
  const double big = fmax(fmax(fmax(fabs(c00), fabs(c11)), fabs(c22)), fmax(fmax(fabs(c01), fabs(c02)), fabs(c12)));
  if (!(big > 0.0) || !(big < __builtin_huge_val())) return false;
  const double s = 1.0 / big;
  c00 *= s; c01 *= s; c02 *= s; c11 *= s; c12 *= s; c22 *= s;
  const double q = (c00 + c11 + c22) / 3.0;
  const double b00 = c00 - q, b11 = c11 - q, b22 = c22 - q;
  const double off = c01 * c01 + c02 * c02 + c12 * c12;
  const double p = sqrt((b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * off) / 6.0);
  if (!(p > 0.0)) return false;                                       // a multiple of I
  const double ip = 1.0 / p;
  const double a00 = b00 * ip, a11 = b11 * ip, a22 = b22 * ip, a01 = c01 * ip, a02 = c02 * ip, a12 = c12 * ip;
  const double det = a00 * (a11 * a22 - a12 * a12) - a01 * (a01 * a22 - a12 * a02) + a02 * (a01 * a12 - a11 * a02);
  const double h = fmin(fmax(0.5 * det, -1.0), 1.0);
  const double lam = q + 2.0 * p * cos(acos(h) / 3.0 + 2.0943951023931954923);      // the smallest root
  const double r0[3] = {c00 - lam, c01, c02}, r1[3] = {c01, c11 - lam, c12}, r2[3] = {c02, c12, c22 - lam};
  double best[3] = {0.0, 0.0, 0.0}, best2 = -1.0;
#pragma unroll
  for (int pair = 0; pair < 3; ++pair) {
    const double* a = pair == 2 ? r1 : r0;
    const double* b = pair == 0 ? r1 : r2;
    const double x[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const double n2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
    if (n2 > best2) { best2 = n2; best[0] = x[0]; best[1] = x[1]; best[2] = x[2]; }
  }
  if (!(best2 > 1e-24)) return false;
  const double inv = 1.0 / sqrt(best2);
  v[0] = best[0] * inv; v[1] = best[1] * inv; v[2] = best[2] * inv;
  return true;
}

// the normal of the sums' covariance C = S_dd / n - (S_d / n)(S_d / n)^T; (0, 0, 1) for fewer than three neighbours and
// for the degenerate cases of smallest_eigenvector
__device__ __forceinline__ void normal_from_sums(const NormalSums& a, double v[3]) {
#pragma clang fp contract(off)
  v[0] = 0.0; v[1] = 0.0; v[2] = 1.0;
  if (a.cnt >= 3.0) {
    const double inv = 1.0 / a.cnt;
    const double m[3] = {a.s[0] * inv, a.s[1] * inv, a.s[2] * inv};
    double e[3];
    if (smallest_eigenvector(a.ss[0] * inv - m[0] * m[0], a.ss[1] * inv - m[0] * m[1], a.ss[2] * inv - m[0] * m[2],
                             a.ss[3] * inv - m[1] * m[1], a.ss[4] * inv - m[1] * m[2], a.ss[5] * inv - m[2] * m[2], e)) {
      v[0] = e[0]; v[1] = e[1]; v[2] = e[2];
    }
  }
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

// the workspace as its kernels read and write it, const for a const workspace; all null without one (no target)
template <class I, class R>
struct NnViews { I *table, *sums, *counters, *list; R* rows; };
template <class I, class R, class B>
inline NnViews<I, R> nn_views_of(const miso_nn_plan_t& p, B* w) {
  if (!w) return {};
  const NnLayout l = nn_layout(p);
  return {reinterpret_cast<I*>(w + l.table), reinterpret_cast<I*>(w + l.sums), reinterpret_cast<I*>(w + l.counters),
          reinterpret_cast<I*>(w + l.list), reinterpret_cast<R*>(w + l.rows)};
}
inline auto nn_views(const miso_nn_plan_t& p, void* ws) { return nn_views_of<int, float4>(p, static_cast<char*>(ws)); }
inline auto nn_views(const miso_nn_plan_t& p, const void* ws) {
  return nn_views_of<const int, const float4>(p, static_cast<const char*>(ws));
}

// the chunks of n queries, in order: f(chunk, first, count)
inline int nn_chunks(int64_t n) { return (int)((n + MISO_NN_CHUNK - 1) / MISO_NN_CHUNK); }
template <class F>
inline void nn_for_chunks(int64_t n, const F& f) {
  for (int c = 0, chunks = nn_chunks(n); c < chunks; ++c) {
    const int64_t first = (int64_t)c * MISO_NN_CHUNK;
    f(c, first, (int)(n - first < MISO_NN_CHUNK ? n - first : MISO_NN_CHUNK));
  }
}

inline NnK nn_k(const miso_nn_plan_t& p) {
  NnK k;
  for (int a = 0; a < 3; ++a) { k.lo[a] = p.bound_min[a]; k.dims[a] = p.dims[a]; }
  k.cell = p.cell; k.mag = p.coord_mag; k.max_rings = p.max_rings; k.n_tgt = p.n_tgt;
  return k;
}

}  // namespace miso

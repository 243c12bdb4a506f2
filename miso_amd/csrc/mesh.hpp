// The triangle-mesh index as its kernels read it (mesh.hip) and what capi.hip calls: the plan itself is host logic and
// lives in capi.hip with the other argument checks.
#pragma once
#include "common.hpp"
#include "nn.hpp"

namespace miso {

struct MeshK {
  float lo[3];      // bound_min
  float cell;       // the cell actually used
  float mag;        // miso_mesh_plan_t.coord_mag
  float widen;      // miso_mesh_plan_t.widen: the rounding slack w of the lists
  int dims[3];
  int n_tri;
  int64_t capacity; // list entries the caller's `lists` holds
};

// A triangle as every kernel reads it: three dwordx4 {v0.x v0.y v0.z e1.x} {e1.y e1.z e2.x e2.y} {e2.z - - -}, e1 = v1 - v0 and
// e2 = v2 - v0 rounded once.  The triangle the kernels intersect and bin IS (v0, v0 + e1, v0 + e2).  A triangle that is
// never hit (a vertex index outside [0, n_vert), a non-finite coordinate, e1 x e2 == 0 in fp32) has v0.x = NaN.
struct MeshTri { float v0[3], e1[3], e2[3]; };

__device__ __forceinline__ void mesh_cross(const float a[3], const float b[3], float c[3]) {
#pragma clang fp contract(off)
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ float mesh_dot(const float a[3], const float b[3]) {
#pragma clang fp contract(off)
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

__device__ __forceinline__ MeshTri mesh_unpack(const float4& r0, const float4& r1, const float4& r2) {
  return {{r0.x, r0.y, r0.z}, {r0.w, r1.x, r1.y}, {r1.z, r1.w, r2.x}};
}

// rows[3 t .. 3 t + 3) of triangle t of the caller's arrays
__device__ __forceinline__ void mesh_make_row(const float* __restrict__ verts, int64_t ld_v, int64_t n_vert,
                                              const int64_t* __restrict__ tris, int64_t ld_t, int64_t t, float4* out) {
#pragma clang fp contract(off)
  const float nan = __builtin_nanf("");
  const int64_t i0 = tris[t * ld_t], i1 = tris[t * ld_t + 1], i2 = tris[t * ld_t + 2];
  float v0[3] = {nan, nan, nan}, e1[3] = {0.0f, 0.0f, 0.0f}, e2[3] = {0.0f, 0.0f, 0.0f};
  if (i0 >= 0 && i0 < n_vert && i1 >= 0 && i1 < n_vert && i2 >= 0 && i2 < n_vert) {
    const float a[3] = {verts[i0 * ld_v], verts[i0 * ld_v + 1], verts[i0 * ld_v + 2]};
    const float b[3] = {verts[i1 * ld_v], verts[i1 * ld_v + 1], verts[i1 * ld_v + 2]};
    const float c[3] = {verts[i2 * ld_v], verts[i2 * ld_v + 1], verts[i2 * ld_v + 2]};
    if (nn_finite3(a[0], a[1], a[2]) && nn_finite3(b[0], b[1], b[2]) && nn_finite3(c[0], c[1], c[2])) {
      float n[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) { e1[k] = b[k] - a[k]; e2[k] = c[k] - a[k]; }
      mesh_cross(e1, e2, n);
      if (nn_finite3(n[0], n[1], n[2]) && (n[0] != 0.0f || n[1] != 0.0f || n[2] != 0.0f)) { v0[0] = a[0]; v0[1] = a[1]; v0[2] = a[2]; }
    }
  }
  out[0] = make_float4(v0[0], v0[1], v0[2], e1[0]);
  out[1] = make_float4(e1[1], e1[2], e2[0], e2[1]);
  out[2] = make_float4(e2[2], 0.0f, 0.0f, 0.0f);
}

// THE intersection (Moller-Trumbore, two-sided), fp32 with one rounding per operation, the reciprocal by __fdiv_rn:
//   p = d x e2, det = (e1.x p.x + e1.y p.y) + e1.z p.z, inv = 1 / det, s = o - v0, u = ((s . p)) inv,
//   q = s x e1, v = (d . q) inv, t = (e2 . q) inv          (every cross component a b - c d, every dot (x + y) + z)
// a hit iff det != 0, u >= 0, v >= 0, u + v <= 1 and t_min <= t <= t_max; a NaN anywhere fails a comparison (a NaN det
// passes `!= 0` and then gives NaN u).  t is in units of |d|.
__device__ __forceinline__ bool mesh_ray_hit(const float o[3], const float d[3], float t_min, float t_max, const MeshTri& m, float& tt) {
#pragma clang fp contract(off)
  float p[3], q[3];
  mesh_cross(d, m.e2, p);
  const float det = mesh_dot(m.e1, p);
  if (!(det != 0.0f)) return false;
  const float inv = __fdiv_rn(1.0f, det);
  const float s[3] = {o[0] - m.v0[0], o[1] - m.v0[1], o[2] - m.v0[2]};
  const float u = mesh_dot(s, p) * inv;
  if (!(u >= 0.0f)) return false;
  mesh_cross(s, m.e1, q);
  const float v = mesh_dot(d, q) * inv;
  if (!(v >= 0.0f) || !(u + v <= 1.0f)) return false;
  tt = mesh_dot(m.e2, q) * inv;
  return tt >= t_min && tt <= t_max;
}

// What a ray keeps of the triangles offered to it.  offer(): a candidate of the stretch [t_in, t_out) of the ray (the
// stretch of the cell that lists it; (-inf, +inf) on the routes without cells); done(t_out): nothing beyond t_out can matter.
// RayBest: the first hit, the best (t, triangle) pair kept lexicographically.
struct RayBest {
  float t; int tri;
  __device__ __forceinline__ void take(const float o[3], const float d[3], float t_min, float t_max, const MeshTri& m, int index) {
    float tt;
    if (!mesh_ray_hit(o, d, t_min, t_max, m, tt)) return;
    if (tt < t || (tt == t && index < tri)) { t = tt; tri = index; }
  }
  __device__ __forceinline__ void offer(const float o[3], const float d[3], float t_min, float t_max, const MeshTri& m, int index, float,
                                        float) { take(o, d, t_min, t_max, m, index); }
  __device__ __forceinline__ bool done(float t_out) const { return t < t_out; }
};

// RayCount: the number of triangles that pass the hit test.  On the grid a triangle is listed in several cells: it counts in
// the one whose stretch holds its computed t (half-open, so exactly one of the stretches that tile the ray).
struct RayCount {
  int n;
  __device__ __forceinline__ void offer(const float o[3], const float d[3], float t_min, float t_max, const MeshTri& m, int, float t_in,
                                        float t_out) {
    float tt;
    if (mesh_ray_hit(o, d, t_min, t_max, m, tt) && tt >= t_in && tt < t_out) ++n;
  }
  __device__ __forceinline__ bool done(float) const { return false; }
};

__device__ __forceinline__ MeshTri mesh_load(const float4* __restrict__ rows, int tri) {
  const float4* r = rows + 3 * (int64_t)tri;
  return mesh_unpack(r[0], r[1], r[2]);
}

// The grid route of one ray for any of the accumulators above (mesh.hip: first hit; mesh_sdf.hip: crossing count): clip to
// the widened box, walk the cells by the 3-D DDA whose boundaries come from the cell index, offer every listed triangle of a
// cell with the cell's stretch of the ray, stop when acc.done(t_out) or the walk leaves [t0, t1] or the grid.  The
// stretches are [-inf, t_out(1)), [t_out(1), t_out(2)), ... [t_out(last - 1), +inf): the boundaries are a running maximum,
// so they tile the line whatever the roundings did, and the hit test itself bounds the two open ends by t_min and t_max.
// A ray outside the walk's guarantee reads ALL rows with the stretch (-inf, +inf); `all_rows` says so.
template <bool STATS, class A>
__device__ __forceinline__ void mesh_walk_ray(const MeshK& k, const int* __restrict__ table, const int* __restrict__ lists,
                                              const float4* __restrict__ rows, const float o[3], const float d[3], float t_min,
                                              float t_max, A& acc, unsigned& visited, unsigned& offered, bool& all_rows) {
#pragma clang fp contract(off)
  const float inf = __builtin_huge_valf();
  bool walk = nn_finite3(o[0], o[1], o[2]) && nn_finite3(d[0], d[1], d[2]), miss = false;
  float inv[3], t0 = t_min, t1 = t_max;
  int step[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float lo = k.lo[a] - k.widen, hi = (k.lo[a] + (float)k.dims[a] * k.cell) + k.widen;
    if (!(fabsf(o[a]) <= 4.0f * k.mag)) walk = false;
    inv[a] = 0.0f; step[a] = 0;
    if (d[a] == 0.0f) {
      if (o[a] < lo || o[a] > hi) miss = true;
    } else {
      inv[a] = __fdiv_rn(1.0f, d[a]);
      if (!(fabsf(inv[a]) < inf)) walk = false;
      step[a] = d[a] > 0.0f ? 1 : -1;
      const float ta = (lo - o[a]) * inv[a], tb = (hi - o[a]) * inv[a];
      t0 = fmaxf(t0, fminf(ta, tb)); t1 = fminf(t1, fmaxf(ta, tb));
    }
  }
  if ((step[0] | step[1] | step[2]) == 0) miss = true;             // a zero direction: det == 0 for every triangle
  if (!(fabsf(t0) < inf) || t1 != t1) walk = false;
  all_rows = !walk;
  if (!walk) {
    for (int t = 0; t < k.n_tri; ++t) acc.offer(o, d, t_min, t_max, mesh_load(rows, t), t, -inf, inf);
    if (STATS) offered = (unsigned)k.n_tri;
  } else if (!miss && t0 <= t1) {
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = nn_cell_axis(o[a] + t0 * d[a], k.lo[a], k.cell, k.dims[a]);
    const int cap = (int)(k.capacity < 0x7fffffff ? k.capacity : 0x7fffffff);
    const int max_steps = k.dims[0] + k.dims[1] + k.dims[2] + 3;
    float t_in = -inf;
    for (int it = 0; it < max_steps; ++it) {
      // where the ray leaves the cell: per axis the plane ahead, from the cell index (monotone in it, no running sum)
      float tm[3];
#pragma unroll
      for (int a = 0; a < 3; ++a)
        tm[a] = step[a] == 0 ? inf : ((k.lo[a] + (float)(c[a] + (step[a] > 0 ? 1 : 0)) * k.cell) - o[a]) * inv[a];
      const float t_out = fminf(tm[0], fminf(tm[1], tm[2]));
      const int ax = tm[0] == t_out ? 0 : (tm[1] == t_out ? 1 : 2);
      const int next = c[ax] + step[ax];
      const bool last = t_out > t1 || !(t_out < inf) || next < 0 || next >= k.dims[ax];
      const float t_end = last ? inf : fmaxf(t_in, t_out);
      const int cell = (c[2] * k.dims[1] + c[1]) * k.dims[0] + c[0];
      const int s = table[cell], e = min(table[cell + 1], cap);     // clamped: a table no build wrote stays inside the lists
      for (int j = max(s, 0); j < e; ++j) {
        const int tri = lists[j];
        if ((unsigned)tri < (unsigned)k.n_tri) acc.offer(o, d, t_min, t_max, mesh_load(rows, tri), tri, t_in, t_end);
      }
      if (STATS) { ++visited; offered += (unsigned)max(e - max(s, 0), 0); }
      if (acc.done(t_out) || last) break;
      c[ax] = next; t_in = t_end;
    }
  }
}

// The all-triangles routes (mesh.hip, mesh_sdf.hip): the caller's triangles through LDS, MESH_TILE at a time, built by
// mesh_make_row; f(MeshTri, index) for each in ascending order, by every lane of the block (one address per wavefront: a
// broadcast).  Every lane of the block calls this, a lane without a query too.
constexpr int MESH_TILE = 512;                                        // triangles per LDS tile (24 KB)
template <class F>
__device__ __forceinline__ void mesh_for_tiles(float4* tile, const float* __restrict__ verts, int64_t ld_v, int64_t n_vert,
                                               const int64_t* __restrict__ tris, int64_t ld_t, int n_tri, const F& f) {
  for (int t0 = 0; t0 < n_tri; t0 += MESH_TILE) {
    const int len = n_tri - t0 < MESH_TILE ? n_tri - t0 : MESH_TILE;
    __syncthreads();                                                  // the readers of the previous tile
    for (int j = threadIdx.x; j < len; j += 256) mesh_make_row(verts, ld_v, n_vert, tris, ld_t, (int64_t)t0 + j, tile + 3 * j);
    __syncthreads();
    for (int j = 0; j < len; ++j) f(mesh_unpack(tile[3 * j], tile[3 * j + 1], tile[3 * j + 2]), t0 + j);
  }
}

// THE closest point of a triangle (v0, v0 + e1, v0 + e2) to q, fp32 with one rounding per operation, divisions by __fdiv_rn:
// the region-classified form (Ericson, Real-Time Collision Detection 5.1.5: ClosestPtPointTriangle), as barycentrics (v, w)
// of e1 and e2.  With ap = q - v0, bp = ap - e1, cp = ap - e2, d1 = e1.ap, d2 = e2.ap, d3 = e1.bp, d4 = e2.bp, d5 = e1.cp,
// d6 = e2.cp, in this order:
//   d1 <= 0, d2 <= 0                                 (0, 0)                        vertex v0
//   d3 >= 0, d4 <= d3                                (1, 0)                        vertex v0 + e1
//   vc = d1 d4 - d3 d2 <= 0, d1 >= 0, d3 <= 0        (d1 / (d1 - d3), 0)           edge e1
//   d6 >= 0, d5 <= d6                                (0, 1)                        vertex v0 + e2
//   vb = d5 d2 - d1 d6 <= 0, d2 >= 0, d6 <= 0        (0, d2 / (d2 - d6))           edge e2
//   va = d3 d6 - d5 d4 <= 0, d4 - d3 >= 0, d5 - d6 >= 0   w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w    the far edge
//   else  den = 1 / ((va + vb) + vc), v = vb den, w = vc den, then v = min(max(v, 0), 1), w = min(max(w, 0), 1 - v)
// (the clamp of the last line does nothing in real arithmetic; in fp32 it keeps the point on the triangle when roundings
// let a point through the six tests that belongs to none of them).  Every branch leaves 0 <= v, w <= 1 and v + w <= 1 + 2^-24:
// a quotient a / (a + b) of non-negative floats rounds into [0, 1].  Then r = ap - (v e1 + w e2) and d2 = (r.x r.x + r.y r.y) +
// r.z r.z.  The smallest (d2, triangle index) pair is kept lexicographically with that winner's (v, w).  A NaN row or a NaN
// query gives a NaN ap, hence a NaN d2, which loses every comparison; +inf never beats the initial (+inf, -1).
struct TriBest {
  float d2; int tri; float v, w;
  __device__ __forceinline__ void take(const float q[3], const MeshTri& m, int index) {
#pragma clang fp contract(off)
    const float ap[3] = {q[0] - m.v0[0], q[1] - m.v0[1], q[2] - m.v0[2]};
    const float bp[3] = {ap[0] - m.e1[0], ap[1] - m.e1[1], ap[2] - m.e1[2]};
    const float cp[3] = {ap[0] - m.e2[0], ap[1] - m.e2[1], ap[2] - m.e2[2]};
    const float d1 = mesh_dot(m.e1, ap), d2_ = mesh_dot(m.e2, ap), d3 = mesh_dot(m.e1, bp), d4 = mesh_dot(m.e2, bp);
    const float d5 = mesh_dot(m.e1, cp), d6 = mesh_dot(m.e2, cp);
    const float vc = d1 * d4 - d3 * d2_, vb = d5 * d2_ - d1 * d6, va = d3 * d6 - d5 * d4;
    float pv, pw;
    if (d1 <= 0.0f && d2_ <= 0.0f) { pv = 0.0f; pw = 0.0f; }
    else if (d3 >= 0.0f && d4 <= d3) { pv = 1.0f; pw = 0.0f; }
    else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { pv = __fdiv_rn(d1, d1 - d3); pw = 0.0f; }
    else if (d6 >= 0.0f && d5 <= d6) { pv = 0.0f; pw = 1.0f; }
    else if (vb <= 0.0f && d2_ >= 0.0f && d6 <= 0.0f) { pv = 0.0f; pw = __fdiv_rn(d2_, d2_ - d6); }
    else if (va <= 0.0f && d4 - d3 >= 0.0f && d5 - d6 >= 0.0f) { pw = __fdiv_rn(d4 - d3, (d4 - d3) + (d5 - d6)); pv = 1.0f - pw; }
    else {
      const float den = __fdiv_rn(1.0f, (va + vb) + vc);
      pv = fminf(fmaxf(vb * den, 0.0f), 1.0f);
      pw = fminf(fmaxf(vc * den, 0.0f), 1.0f - pv);
    }
    const float r[3] = {ap[0] - (pv * m.e1[0] + pw * m.e2[0]), ap[1] - (pv * m.e1[1] + pw * m.e2[1]), ap[2] - (pv * m.e1[2] + pw * m.e2[2])};
    const float n2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
    if (n2 < d2 || (n2 == d2 && index < tri)) { d2 = n2; tri = index; v = pv; w = pw; }
  }
};

// The shell walk's stop test (mesh_sdf.hip), ring_finished's shape with the slack of the triangle distance.  After ring r
// every triangle not yet offered touches no cell of the examined box (the lists name a triangle in every cell it touches,
// with w to spare), so each of its points lies beyond a face of the box that is not on the grid's edge: at least g away,
// g = ring_gap.  In fp32 (u = 2^-24, A = MeshK.mag, |q_a| <= 4 A for a query that walks):
//   * the face.  fl(q - fl(lo + fl(k cell))) is off by at most 2 u A + u (5 A + g) < 8 u (A + g).
//   * the distance.  take() measures the distance to a point P(v, w) with 0 <= v, w <= 1, v + w <= 1 + u: a point within
//     u |e2| of the triangle WHATEVER region the roundings chose, so its computed distance is never far below the true one:
//     per component ap is off by u |ap| <= 5 u A, v e1 + w e2 by 2 u (|e1_a| + |e2_a|) <= 4 u A, r by u |r_a|, in norm
//     sqrt(3) 9 u A + u d < 16 u A + u d; the sum of squares and the square adds 3 u relative.  A misclassified region can
//     only make the computed d LARGER than the triangle's true distance, which the stop test does not rest on.
// Together a triangle left out has a computed d above g - 26 u A - 4 u g; the test takes 64 u (A + g) = 2^-18 (A + g) off g
// and 2^-20 (relative) off its square, and the comparison is strict: its computed d2 is above `best`, so it loses whatever
// its index.  (The lists' own slack w = 128 u A is not spent here.)
__device__ __forceinline__ bool mesh_ring_finished(const MeshK& k, const float q[3], const int c[3], int r, float best) {
#pragma clang fp contract(off)
  const float g = ring_gap(k, q, c, r);
  if (g == __builtin_huge_valf()) return true;    // the box is the grid
  const float gs = g - 0x1p-18f * (k.mag + g);
  if (!(gs > 0.0f)) return false;
  return best < (gs * gs) * (1.0f - 0x1p-20f);
}

inline int64_t mesh_a256(int64_t v) { return (v + 255) / 256 * 256; }

struct MeshLayout { int64_t table, sums, rows, total; };

// byte offsets inside the workspace (the lists are the caller's second buffer: their length is known after the count)
inline MeshLayout mesh_layout(const miso_mesh_plan_t& p) {
  MeshLayout l;
  int64_t at = 0;
  l.table = at; at += mesh_a256((p.cells + 1) * 4);
  l.sums = at;  at += mesh_a256(1024 * 4);
  l.rows = at;  at += mesh_a256(p.n_tri * 48);
  l.total = at;
  return l;
}

inline MeshK mesh_k(const miso_mesh_plan_t& p, int64_t capacity) {
  MeshK k;
  for (int a = 0; a < 3; ++a) { k.lo[a] = p.bound_min[a]; k.dims[a] = p.dims[a]; }
  k.cell = p.cell; k.mag = p.coord_mag; k.widen = p.widen; k.n_tri = (int)p.n_tri; k.capacity = capacity;
  return k;
}

}  // namespace miso

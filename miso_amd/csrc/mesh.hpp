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
// passes `!= 0` and then gives NaN u).  t is in units of |d|.  The best (t, triangle) pair is kept lexicographically.
struct RayBest {
  float t; int tri;
  __device__ __forceinline__ void take(const float o[3], const float d[3], float t_min, float t_max, const MeshTri& m, int index) {
#pragma clang fp contract(off)
    float p[3], q[3];
    mesh_cross(d, m.e2, p);
    const float det = mesh_dot(m.e1, p);
    if (!(det != 0.0f)) return;
    const float inv = __fdiv_rn(1.0f, det);
    const float s[3] = {o[0] - m.v0[0], o[1] - m.v0[1], o[2] - m.v0[2]};
    const float u = mesh_dot(s, p) * inv;
    if (!(u >= 0.0f)) return;
    mesh_cross(s, m.e1, q);
    const float v = mesh_dot(d, q) * inv;
    if (!(v >= 0.0f) || !(u + v <= 1.0f)) return;
    const float tt = mesh_dot(m.e2, q) * inv;
    if (!(tt >= t_min) || !(tt <= t_max)) return;
    if (tt < t || (tt == t && index < tri)) { t = tt; tri = index; }
  }
};

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

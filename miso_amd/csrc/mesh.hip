// Ray casting against a triangle mesh: what Open3D's RaycastingScene.cast_rays gives the reference's PosedSdf3D
// (grid_opt/datasets/sdf_3d.py:209-312), the first hit of every ray.  Two routes, one answer: both put every candidate
// through RayBest::take (mesh.hpp: Moller-Trumbore in fp32, one rounding per operation) and keep the smallest
// (t, triangle index) pair, compared lexicographically, (+inf, -1) for a miss.  The answer is a function of the mesh and the
// ray alone: not of the route, the visit order, or the order the build's atomics left inside a cell.
//
// Index (miso_mesh_count, miso_mesh_build; workspace layout in mesh_layout):
//   rows   three dwordx4 per triangle in the caller's order (MeshTri); a triangle that is never hit carries a NaN.
//   table  cells + 1 int32, as nn.hip's: count, exclusive scan (nn.hip's launch_nn_scan), fill by atomicAdd.
//   lists  the caller's second buffer: per cell the triangles that may touch it.  A triangle is listed in the cells of
//          its box, widened by w = plan.widen on every side, whose centre lies within (cell / 2 + 2 w) |n|_1 (+ a bound on
//          the rounding of n) of the triangle's plane: a plane-slab test, conservative.
//          A wavefront per triangle, its lanes striding over the box: a triangle with two million box cells keeps 64
//          lanes busy and no lane waits for another's loop.
// Query (miso_mesh_cast_rays), a lane per ray, the walk itself being mesh.hpp's mesh_walk_ray (mesh_sdf.hip counts
// crossings with it): clip to the widened box, walk the cells by a 3-D DDA whose boundaries
// are recomputed from the cell index at every step (no accumulated increment), offer every listed triangle of a cell
// wherever on the ray its hit lies, stop when best.t < the parameter at which the ray leaves the cell.  The rounding
// slack sits in the lists (w), not in the stop test: section 4.15 shows why that is enough for origins within 4 coord_mag
// of zero.  A ray outside that guarantee (a non-finite origin or direction, a far origin, a direction component whose
// reciprocal overflows) is answered by the same lane from ALL rows: the all-triangles answer by construction.
// miso_mesh_cast_rays_all is the second kernel over the caller's arrays, triangles staged through LDS, no index.
#include "common.hpp"
#include "launch.hpp"
#include "mesh.hpp"

#pragma clang fp contract(off)

namespace miso {
namespace {

__global__ __launch_bounds__(256) void mesh_rows_kernel(const float* __restrict__ verts, int64_t ld_v, int64_t n_vert,
                                                        const int64_t* __restrict__ tris, int64_t ld_t, int n_tri,
                                                        float4* __restrict__ rows) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n_tri) mesh_make_row(verts, ld_v, n_vert, tris, ld_t, t, rows + 3 * t);
}

// count (FILL = false: table[c + 1] += 1 per listed cell, *total += the triangle's entries) or fill
template <bool FILL>
__global__ __launch_bounds__(256) void mesh_bin_kernel(MeshK k, const float4* __restrict__ rows, int* __restrict__ table,
                                                       int* __restrict__ lists, unsigned long long* __restrict__ total) {
  const int tri = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (tri >= k.n_tri) return;
  const MeshTri m = mesh_unpack(rows[3 * (int64_t)tri], rows[3 * (int64_t)tri + 1], rows[3 * (int64_t)tri + 2]);
  if (!(m.v0[0] == m.v0[0])) return;                                // never hit: in no list
  int c0[3], ext[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float p1 = m.v0[a] + m.e1[a], p2 = m.v0[a] + m.e2[a];
    const float mn = fminf(m.v0[a], fminf(p1, p2)), mx = fmaxf(m.v0[a], fmaxf(p1, p2));
    c0[a] = nn_cell_axis(mn - k.widen, k.lo[a], k.cell, k.dims[a]);
    ext[a] = nn_cell_axis(mx + k.widen, k.lo[a], k.cell, k.dims[a]) - c0[a] + 1;
  }
  float n[3];
  mesh_cross(m.e1, m.e2, n);
  const float l1 = (fabsf(m.e1[0]) + fabsf(m.e1[1])) + fabsf(m.e1[2]), l2 = (fabsf(m.e2[0]) + fabsf(m.e2[1])) + fabsf(m.e2[2]);
  // |n . (centre - v0)| <= (cell / 2 + w) |n|_1 for a widened cell the plane meets; + w |n|_1 and 2^-10 relative for the
  // roundings of the test, + the last term for the rounding of n itself (|dn_a| <= 2^-23 |e1| |e2|)
  const float reach = (0.5f * k.cell + 2.0f * k.widen) * ((fabsf(n[0]) + fabsf(n[1])) + fabsf(n[2])) * (1.0f + 0x1p-10f) +
                      0x1p-20f * (l1 * l2) * ((l1 + l2) + 2.0f * k.cell);
  const int nbox = ext[0] * ext[1] * ext[2];                        // <= cells <= 2^24
  const int xy = ext[0] * ext[1];
  int mine = 0;
  for (int i = lane; i < nbox; i += 64) {
    const int z = i / xy, r = i - z * xy, y = r / ext[0], x = r - y * ext[0];
    const int c[3] = {c0[0] + x, c0[1] + y, c0[2] + z};
    const float rel[3] = {(k.lo[0] + ((float)c[0] + 0.5f) * k.cell) - m.v0[0], (k.lo[1] + ((float)c[1] + 0.5f) * k.cell) - m.v0[1],
                          (k.lo[2] + ((float)c[2] + 0.5f) * k.cell) - m.v0[2]};
    if (fabsf(mesh_dot(n, rel)) > reach) continue;                  // (a NaN stays listed)
    const int cell = (c[2] * k.dims[1] + c[1]) * k.dims[0] + c[0];
    const int at = atomicAdd(&table[cell + 1], 1);
    if (FILL && at >= 0 && (int64_t)at < k.capacity) lists[at] = tri;
    ++mine;
  }
  if (!FILL) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if (lane == 0 && mine) atomicAdd(total, (unsigned long long)mine);
  }
}

// stats (STATS): {cells visited, triangles offered, rays answered from all rows}
template <bool STATS>
__global__ __launch_bounds__(256) void mesh_cast_rays_kernel(MeshK k, const int* __restrict__ table, const int* __restrict__ lists,
                                                             const float4* __restrict__ rows, const float* __restrict__ org,
                                                             int64_t ld_o, const float* __restrict__ dir, int64_t ld_d, int64_t n,
                                                             float t_min, float t_max, float* __restrict__ out_t,
                                                             int64_t* __restrict__ out_tri, unsigned long long* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float o[3] = {org[i * ld_o], org[i * ld_o + 1], org[i * ld_o + 2]};
  const float d[3] = {dir[i * ld_d], dir[i * ld_d + 1], dir[i * ld_d + 2]};
  RayBest b = {__builtin_huge_valf(), -1};
  unsigned visited = 0, offered = 0;
  bool all_rows;
  mesh_walk_ray<STATS>(k, table, lists, rows, o, d, t_min, t_max, b, visited, offered, all_rows);
  out_t[i] = b.t; out_tri[i] = (int64_t)b.tri;
  if (STATS) {
    atomicAdd(&stats[0], (unsigned long long)visited); atomicAdd(&stats[1], (unsigned long long)offered);
    if (all_rows) atomicAdd(&stats[2], 1ull);
  }
}

__global__ __launch_bounds__(256) void mesh_cast_rays_all_kernel(const float* __restrict__ verts, int64_t ld_v, int64_t n_vert,
                                                                 const int64_t* __restrict__ tris, int64_t ld_t, int n_tri,
                                                                 const float* __restrict__ org, int64_t ld_o,
                                                                 const float* __restrict__ dir, int64_t ld_d, int64_t n, float t_min,
                                                                 float t_max, float* __restrict__ out_t, int64_t* __restrict__ out_tri) {
  __shared__ float4 tile[3 * MESH_TILE];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n;
  float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
  if (live) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { o[a] = org[i * ld_o + a]; d[a] = dir[i * ld_d + a]; }
  }
  RayBest b = {__builtin_huge_valf(), -1};
  mesh_for_tiles(tile, verts, ld_v, n_vert, tris, ld_t, n_tri, [&](const MeshTri& m, int t) { b.take(o, d, t_min, t_max, m, t); });
  if (live) { out_t[i] = b.t; out_tri[i] = (int64_t)b.tri; }
}

}  // namespace

int64_t mesh_workspace_bytes(const miso_mesh_plan_t& p) { return mesh_layout(p).total; }

hipError_t launch_mesh_count(const miso_mesh_plan_t& p, const float* verts, int64_t ld_v, int64_t n_vert, const int64_t* tris,
                             int64_t ld_t, void* ws, int64_t* entries, hipStream_t s) {
  hipError_t e = launch_zero_words(entries, 2, s);
  if (e != hipSuccess || p.n_tri == 0) return e;
  const MeshLayout l = mesh_layout(p);
  char* w = static_cast<char*>(ws);
  int* table = reinterpret_cast<int*>(w + l.table);
  float4* rows = reinterpret_cast<float4*>(w + l.rows);
  const MeshK k = mesh_k(p, 0);
  e = launch_zero_words(table, (int)p.cells + 1, s);
  if (e != hipSuccess) return e;
  mesh_rows_kernel<<<(unsigned)((p.n_tri + 255) / 256), 256, 0, s>>>(verts, ld_v, n_vert, tris, ld_t, k.n_tri, rows);
  mesh_bin_kernel<false><<<(unsigned)((p.n_tri + 3) / 4), 256, 0, s>>>(k, rows, table, nullptr,
                                                                      reinterpret_cast<unsigned long long*>(entries));
  e = hipGetLastError();
  return e != hipSuccess ? e : launch_nn_scan(table + 1, (int)p.cells, reinterpret_cast<int*>(w + l.sums), s);
}

hipError_t launch_mesh_build(const miso_mesh_plan_t& p, void* ws, int32_t* lists, int64_t capacity, hipStream_t s) {
  if (p.n_tri == 0) return hipSuccess;
  const MeshLayout l = mesh_layout(p);
  char* w = static_cast<char*>(ws);
  mesh_bin_kernel<true><<<(unsigned)((p.n_tri + 3) / 4), 256, 0, s>>>(mesh_k(p, capacity), reinterpret_cast<const float4*>(w + l.rows),
                                                                     reinterpret_cast<int*>(w + l.table), lists, nullptr);
  return hipGetLastError();
}

hipError_t launch_mesh_cast_rays(const miso_mesh_plan_t& p, const void* ws, const int32_t* lists, int64_t capacity,
                                 const float* org, int64_t ld_o, const float* dir, int64_t ld_d, int64_t n, float t_min, float t_max,
                                 float* out_t, int64_t* out_tri, int64_t* stats, hipStream_t s) {
  if (stats) {
    const hipError_t e = launch_zero_words(stats, 6, s);
    if (e != hipSuccess) return e;
  }
  if (n == 0) return hipSuccess;
  if (p.n_tri == 0) return launch_nn_fill(n, out_t, out_tri, s);
  const MeshLayout l = mesh_layout(p);
  const char* w = static_cast<const char*>(ws);
  const int* table = reinterpret_cast<const int*>(w + l.table);
  const float4* rows = reinterpret_cast<const float4*>(w + l.rows);
  const unsigned g = (unsigned)((n + 255) / 256);
  const MeshK k = mesh_k(p, capacity);
  if (stats)
    mesh_cast_rays_kernel<true><<<g, 256, 0, s>>>(k, table, lists, rows, org, ld_o, dir, ld_d, n, t_min, t_max, out_t, out_tri,
                                                  reinterpret_cast<unsigned long long*>(stats));
  else
    mesh_cast_rays_kernel<false><<<g, 256, 0, s>>>(k, table, lists, rows, org, ld_o, dir, ld_d, n, t_min, t_max, out_t, out_tri, nullptr);
  return hipGetLastError();
}

hipError_t launch_mesh_cast_rays_all(const float* verts, int64_t ld_v, int64_t n_vert, const int64_t* tris, int64_t ld_t,
                                     int64_t n_tri, const float* org, int64_t ld_o, const float* dir, int64_t ld_d, int64_t n,
                                     float t_min, float t_max, float* out_t, int64_t* out_tri, hipStream_t s) {
  if (n == 0) return hipSuccess;
  // (n_tri == 0: no tile is staged and every ray keeps (+inf, -1))
  mesh_cast_rays_all_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(verts, ld_v, n_vert, tris, ld_t, (int)n_tri, org, ld_o, dir, ld_d,
                                                                       n, t_min, t_max, out_t, out_tri);
  return hipGetLastError();
}

}  // namespace miso

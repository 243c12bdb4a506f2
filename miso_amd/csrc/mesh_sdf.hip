// The distance side of the triangle-mesh index (mesh.hip builds it): what pysdf gives the reference's Sdf3D and PosedSdf3D
// (grid_opt/datasets/sdf_3d.py:17-155, 193-199), the closest triangle of every point and, for the sign, how many triangles
// a ray crosses.  DESIGN.md section 4.16.
//
// Closest (miso_mesh_closest, miso_mesh_closest_all): every route puts every candidate through TriBest::take (mesh.hpp: the
// region-classified closest point in fp32, one rounding per operation) and keeps the smallest (d2, triangle index) pair,
// compared lexicographically, with that winner's barycentrics (v, w); (+inf, -1, 0, 0) without a triangle.  The answer is a
// function of the mesh and the query alone.
//   index   a lane per query walks the Chebyshev shells of cells around the query's clamped cell (nn.hpp: nn_shell) and after
//           each asks mesh_ring_finished (mesh.hpp): every triangle not yet offered touches no cell of the examined box, so
//           it is at least the gap to the box's nearest inner face away.  A triangle is offered once per listed cell: take()
//           is idempotent.  After `far_rings` unfinished shells the lane starts again at shell 0 of a SECOND, coarser index
//           of the same mesh (cell x MISO_MESH_FAR_FACTOR, the same build): a query metres from any surface would
//           otherwise walk millions of empty fine cells.  The coarse index is complete on its own, the same argument
//           holds for it, and its walk ends at the latest when the box is its whole grid.  The best pair found on the fine
//           shells is kept: it went through the same take().
//   all rows  a finite query with |q_a| > 4 coord_mag lies outside the stop test's rounding argument and is answered by the
//           same lane from ALL rows; a non-finite query is (+inf, -1) without a scan.
//   all     miso_mesh_closest_all: the caller's arrays through LDS (mesh.hpp: mesh_for_tiles), no index.
// Crossing counts (miso_mesh_count_hits, miso_mesh_count_hits_all): the ray walk of mesh.hip (mesh.hpp: mesh_walk_ray) with
// the RayCount accumulator: no early stop, a triangle counts in the cell whose half-open stretch holds its computed t.
#include "common.hpp"
#include "launch.hpp"
#include "mesh.hpp"

#pragma clang fp contract(off)

namespace miso {
namespace {

// the lists of the cells first .. last of one x run are one run of entries (clamped like mesh_walk_ray's)
__device__ __forceinline__ void mesh_offer_cells(const MeshK& k, const int* __restrict__ table, const int* __restrict__ lists,
                                                 const float4* __restrict__ rows, int first, int last, const float q[3], TriBest& b,
                                                 unsigned& cells, unsigned& offered) {
  const int cap = (int)(k.capacity < 0x7fffffff ? k.capacity : 0x7fffffff);
  const int s = max(table[first], 0), e = min(table[last + 1], cap);
  for (int j = s; j < e; ++j) {
    const int tri = lists[j];
    if ((unsigned)tri < (unsigned)k.n_tri) b.take(q, mesh_load(rows, tri), tri);
  }
  cells += (unsigned)(last - first + 1); offered += (unsigned)max(e - s, 0);
}

// shells 0 .. r_end - 1 of the query's cell in index k; true: the stop test held (or the box became the grid)
__device__ __forceinline__ bool mesh_walk_shells(const MeshK& k, const int* __restrict__ table, const int* __restrict__ lists,
                                                 const float4* __restrict__ rows, const float q[3], int r_end, TriBest& b,
                                                 unsigned& cells, unsigned& offered) {
  int c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = nn_cell_axis(q[a], k.lo[a], k.cell, k.dims[a]);
  const int r_grid = max(k.dims[0], max(k.dims[1], k.dims[2]));      // at r = r_grid - 1 the box is the grid
  for (int r = 0; r < r_end && r < r_grid; ++r) {
    const NnShell s = nn_shell(k, c, r);
    for (int z = s.lo[2]; z <= s.hi[2]; ++z)
      for (int y = s.lo[1]; y <= s.hi[1]; ++y) {
        const int row = (z * k.dims[1] + y) * k.dims[0];
        if (abs(z - c[2]) == r || abs(y - c[1]) == r) {               // a whole x run of the shell
          mesh_offer_cells(k, table, lists, rows, row + s.lo[0], row + s.hi[0], q, b, cells, offered);
        } else {                                                      // (r > 0 here) the two end cells of the run
          if (c[0] - r >= 0) mesh_offer_cells(k, table, lists, rows, row + c[0] - r, row + c[0] - r, q, b, cells, offered);
          if (c[0] + r < k.dims[0]) mesh_offer_cells(k, table, lists, rows, row + c[0] + r, row + c[0] + r, q, b, cells, offered);
        }
      }
    if (mesh_ring_finished(k, q, c, r, b.d2)) return true;
  }
  return false;
}

__device__ __forceinline__ bool mesh_covers(const MeshK& k, const float q[3]) {
  return fabsf(q[0]) <= 4.0f * k.mag && fabsf(q[1]) <= 4.0f * k.mag && fabsf(q[2]) <= 4.0f * k.mag;
}

// stats (STATS): {fine cells, coarse cells, triangles offered, queries that went coarse, queries answered from all rows}
template <bool STATS>
__global__ __launch_bounds__(256) void mesh_closest_kernel(MeshK k, const int* __restrict__ table, const int* __restrict__ lists,
                                                           const float4* __restrict__ rows, MeshK kf, const int* __restrict__ table_f,
                                                           const int* __restrict__ lists_f, int far_rings,
                                                           const float* __restrict__ pts, int64_t ld_p, int64_t n,
                                                           float* __restrict__ out_d2, int64_t* __restrict__ out_tri,
                                                           float2* __restrict__ out_vw, unsigned long long* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float q[3] = {pts[i * ld_p], pts[i * ld_p + 1], pts[i * ld_p + 2]};
  TriBest b = {__builtin_huge_valf(), -1, 0.0f, 0.0f};
  unsigned fine = 0, coarse = 0, offered = 0;
  bool went_coarse = false, all_rows = false;
  if (k.n_tri > 0 && nn_finite3(q[0], q[1], q[2])) {
    if (!mesh_covers(k, q)) {
      all_rows = true;
      for (int t = 0; t < k.n_tri; ++t) b.take(q, mesh_load(rows, t), t);
      offered = (unsigned)k.n_tri;
    } else {
      const bool far = table_f != nullptr && mesh_covers(kf, q);     // no far set: the fine shells to their end
      if (!mesh_walk_shells(k, table, lists, rows, q, far ? far_rings : 0x7fffffff, b, fine, offered) && far) {
        went_coarse = true;
        mesh_walk_shells(kf, table_f, lists_f, rows, q, 0x7fffffff, b, coarse, offered);
      }
    }
  }
  out_d2[i] = b.d2; out_tri[i] = (int64_t)b.tri;
  if (out_vw) out_vw[i] = make_float2(b.v, b.w);
  if (STATS) {
    atomicAdd(&stats[0], (unsigned long long)fine); atomicAdd(&stats[1], (unsigned long long)coarse);
    atomicAdd(&stats[2], (unsigned long long)offered);
    if (went_coarse) atomicAdd(&stats[3], 1ull);
    if (all_rows) atomicAdd(&stats[4], 1ull);
  }
}

__global__ __launch_bounds__(256) void mesh_closest_all_kernel(const float* __restrict__ verts, int64_t ld_v, int64_t n_vert,
                                                               const int64_t* __restrict__ tris, int64_t ld_t, int n_tri,
                                                               const float* __restrict__ pts, int64_t ld_p, int64_t n,
                                                               float* __restrict__ out_d2, int64_t* __restrict__ out_tri,
                                                               float2* __restrict__ out_vw) {
  __shared__ float4 tile[3 * MESH_TILE];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n;
  float q[3] = {0.0f, 0.0f, 0.0f};
  if (live) {
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = pts[i * ld_p + a];
  }
  TriBest b = {__builtin_huge_valf(), -1, 0.0f, 0.0f};
  mesh_for_tiles(tile, verts, ld_v, n_vert, tris, ld_t, n_tri, [&](const MeshTri& m, int t) { b.take(q, m, t); });
  if (live) {
    out_d2[i] = b.d2; out_tri[i] = (int64_t)b.tri;
    if (out_vw) out_vw[i] = make_float2(b.v, b.w);
  }
}

__global__ __launch_bounds__(256) void mesh_count_hits_kernel(MeshK k, const int* __restrict__ table, const int* __restrict__ lists,
                                                              const float4* __restrict__ rows, const float* __restrict__ org,
                                                              int64_t ld_o, const float* __restrict__ dir, int64_t ld_d, int64_t n,
                                                              float t_min, float t_max, int* __restrict__ out_count) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float o[3] = {org[i * ld_o], org[i * ld_o + 1], org[i * ld_o + 2]};
  const float d[3] = {dir[i * ld_d], dir[i * ld_d + 1], dir[i * ld_d + 2]};
  RayCount acc = {0};
  unsigned visited = 0, offered = 0;
  bool all_rows;
  if (k.n_tri > 0) mesh_walk_ray<false>(k, table, lists, rows, o, d, t_min, t_max, acc, visited, offered, all_rows);
  out_count[i] = acc.n;
}

__global__ __launch_bounds__(256) void mesh_count_hits_all_kernel(const float* __restrict__ verts, int64_t ld_v, int64_t n_vert,
                                                                  const int64_t* __restrict__ tris, int64_t ld_t, int n_tri,
                                                                  const float* __restrict__ org, int64_t ld_o,
                                                                  const float* __restrict__ dir, int64_t ld_d, int64_t n, float t_min,
                                                                  float t_max, int* __restrict__ out_count) {
  __shared__ float4 tile[3 * MESH_TILE];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n;
  float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
  if (live) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { o[a] = org[i * ld_o + a]; d[a] = dir[i * ld_d + a]; }
  }
  const float inf = __builtin_huge_valf();
  RayCount acc = {0};
  mesh_for_tiles(tile, verts, ld_v, n_vert, tris, ld_t, n_tri,
                 [&](const MeshTri& m, int t) { acc.offer(o, d, t_min, t_max, m, t, -inf, inf); });
  if (live) out_count[i] = acc.n;
}

struct MeshViews { const int* table; const float4* rows; };
MeshViews mesh_views(const miso_mesh_plan_t& p, const void* ws) {
  if (!ws) return {nullptr, nullptr};
  const MeshLayout l = mesh_layout(p);
  const char* w = static_cast<const char*>(ws);
  return {reinterpret_cast<const int*>(w + l.table), reinterpret_cast<const float4*>(w + l.rows)};
}

}  // namespace

hipError_t launch_mesh_closest(const miso_mesh_plan_t& p, const void* ws, const int32_t* lists, int64_t capacity,
                               const miso_mesh_plan_t* p_far, const void* ws_far, const int32_t* lists_far, int64_t capacity_far,
                               const float* pts, int64_t ld_p, int64_t n, float* out_d2, int64_t* out_tri, float* out_vw,
                               int64_t* stats, hipStream_t s) {
  if (stats) {
    const hipError_t e = launch_zero_words(stats, 10, s);
    if (e != hipSuccess) return e;
  }
  if (n == 0) return hipSuccess;
  const MeshViews v = mesh_views(p, p.n_tri > 0 ? ws : nullptr);
  const bool far = p_far && p.n_tri > 0;
  const MeshViews vf = far ? mesh_views(*p_far, ws_far) : MeshViews{nullptr, nullptr};
  const MeshK k = mesh_k(p, capacity), kf = far ? mesh_k(*p_far, capacity_far) : k;
  const int far_rings = far && p_far->reserved > 0 ? p_far->reserved : MISO_MESH_FAR_RINGS;
  const unsigned g = (unsigned)((n + 255) / 256);
  float2* vw = reinterpret_cast<float2*>(out_vw);
  if (stats)
    mesh_closest_kernel<true><<<g, 256, 0, s>>>(k, v.table, lists, v.rows, kf, vf.table, lists_far, far_rings, pts, ld_p, n, out_d2, out_tri,
                                                vw, reinterpret_cast<unsigned long long*>(stats));
  else
    mesh_closest_kernel<false><<<g, 256, 0, s>>>(k, v.table, lists, v.rows, kf, vf.table, lists_far, far_rings, pts, ld_p, n, out_d2,
                                                 out_tri, vw, nullptr);
  return hipGetLastError();
}

hipError_t launch_mesh_closest_all(const float* verts, int64_t ld_v, int64_t n_vert, const int64_t* tris, int64_t ld_t, int64_t n_tri,
                                   const float* pts, int64_t ld_p, int64_t n, float* out_d2, int64_t* out_tri, float* out_vw,
                                   hipStream_t s) {
  if (n == 0) return hipSuccess;
  mesh_closest_all_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(verts, ld_v, n_vert, tris, ld_t, (int)n_tri, pts, ld_p, n, out_d2,
                                                                     out_tri, reinterpret_cast<float2*>(out_vw));
  return hipGetLastError();
}

hipError_t launch_mesh_count_hits(const miso_mesh_plan_t& p, const void* ws, const int32_t* lists, int64_t capacity, const float* org,
                                  int64_t ld_o, const float* dir, int64_t ld_d, int64_t n, float t_min, float t_max,
                                  int32_t* out_count, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const MeshViews v = mesh_views(p, p.n_tri > 0 ? ws : nullptr);
  mesh_count_hits_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(mesh_k(p, capacity), v.table, lists, v.rows, org, ld_o, dir, ld_d, n,
                                                                    t_min, t_max, out_count);
  return hipGetLastError();
}

hipError_t launch_mesh_count_hits_all(const float* verts, int64_t ld_v, int64_t n_vert, const int64_t* tris, int64_t ld_t,
                                      int64_t n_tri, const float* org, int64_t ld_o, const float* dir, int64_t ld_d, int64_t n,
                                      float t_min, float t_max, int32_t* out_count, hipStream_t s) {
  if (n == 0) return hipSuccess;
  mesh_count_hits_all_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(verts, ld_v, n_vert, tris, ld_t, (int)n_tri, org, ld_o, dir,
                                                                        ld_d, n, t_min, t_max, out_count);
  return hipGetLastError();
}

}  // namespace miso

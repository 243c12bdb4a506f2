// The per-point work of an ICP iteration (Open3D's registration_icp, restated from its documented behaviour; users:
// grid_opt/utils/utils_registration.py, utils_scannet.align_mesh_to_ref, grid_opt/align/icp.py) and normals on the
// nearest-neighbour index.  One iteration is: transform the source, search (miso_nn_query on the transformed cloud),
// reduce the correspondences to MISO_ICP_SUMS doubles, which the host reads and solves in float64.
//
// Transform (miso_icp_transform).  p'_i = ((R_i0 x + R_i1 y) + R_i2 z) + t_i in fp32, one rounding per operation (five a
// component), no contraction: the search and the sums read the bits written here.
//
// Sums (miso_icp_sums).  Pair i is an inlier when 0 <= idx[i] < m and (double)d2[i] <= max_dist * max_dist (the product
// in float64): `<=`, as the normals' radius test below; a NaN d2 is no inlier.  Every term is formed in float64 from the
// fp32 inputs (exactly converted), one rounding per operation in the order written here:
//     out[0]  count                      out[1]  sum of (double)d2
//   point to plane (kind 1), q = tgt[idx], n = normals[idx], e = p' - q:
//     r  = (e_x n_x + e_y n_y) + e_z n_z
//     J  = [p'_y n_z - p'_z n_y,  p'_z n_x - p'_x n_z,  p'_x n_y - p'_y n_x,  n_x, n_y, n_z]
//     w  = 1 (loss 0), or with s = r / k: (1 - s s)^2 for |r| <= k and 0 beyond it (loss 1, Tukey)
//     out[2 .. 22]   (w J_a) J_b for a <= b, rows of the upper triangle one after the other
//     out[23 .. 28]  (w J_a) r           out[29]  (w r) r
//   point to point (kind 0), a = p' - origin, b = q - origin:
//     out[2 .. 4] a    out[5 .. 7] b    out[8 .. 16] b_i a_j (row i, column j)    the rest 0
// Summation: a lane adds its pairs (i = lane, lane + lanes, ..) in index order, the 64 lanes of a wavefront are added by a
// butterfly (xor 32, 16, .. 1), the four wavefronts of a block in order, one partial per block into the workspace; a second
// launch of one block adds the partials in block order.  The grid is a function of n alone and no atomic is used, so two
// calls on the same inputs return the same bits.  n == 0 launches the second kernel only, which writes zeros.
//
// Normals (miso_nn_normals).  A lane per query point q walks the cells of the index that the ball of `radius` around q
// touches, an x run of rows at a time (nn_visit_run, nn.hpp: the run visitor of the nearest-neighbour queries): per
// axis the cells of fl(q - rs) .. fl(q + rs), rs = radius + 2^-21 (|q| + radius), which covers the rounding of
// the two sums (the cell function itself is monotone, so a target within the radius along an axis never lies in a cell
// outside that range).  For every target t of those cells, d = t - q in float64 and d2 = (d_x d_x + d_y d_y) + d_z d_z;
// with d2 <= radius^2 it adds 1, d and d d^T to ten float64 accumulators.  C = S_dd / n - (S_d / n)(S_d / n)^T; the
// normal is the unit eigenvector of C's smallest eigenvalue, closed form: C scaled by its largest |entry|, the smallest
// root by the trigonometric formula (q = tr / 3, p = sqrt(tr((C - qI)^2) / 6), lambda = q + 2 p cos(acos(det((C - qI) / p)
// / 2) / 3 + 2 pi / 3)), then the largest of the three cross products of two rows of C - lambda I, normalised.  Fewer than
// three neighbours, C = 0, C a multiple of I, or a largest cross product of squared length <= 1e-24 (a neighbourhood on
// a line) give (0, 0, 1).  The sign of the normal is whatever the cross product gives.  The order in which a cell's
// targets are added is the order the build's atomics left, so the last bits of a normal can differ between two builds of
// the index (never the count).
#include "common.hpp"
#include "launch.hpp"
#include "nn.hpp"

#pragma clang fp contract(off)

namespace miso {
namespace {

struct IcpPose {
  float R[9];
  float t[3];
};

__global__ __launch_bounds__(256) void icp_transform_kernel(IcpPose T, const float* __restrict__ src, int64_t ld, int64_t n,
                                                            float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = src[i * ld], y = src[i * ld + 1], z = src[i * ld + 2];
#pragma unroll
  for (int a = 0; a < 3; ++a) out[i * 3 + a] = ((T.R[3 * a] * x + T.R[3 * a + 1] * y) + T.R[3 * a + 2] * z) + T.t[a];
}

struct IcpK {
  int64_t n, m;
  double max2, k;
  double origin[3];
};

constexpr int ICP_USED = 30;                       // entries a kernel accumulates; MISO_ICP_SUMS = 32 are written
static_assert(ICP_USED <= MISO_ICP_SUMS, "the block of sums");

template <int KIND, int LOSS>
__global__ __launch_bounds__(256) void icp_sums_kernel(IcpK k, const float* __restrict__ moved, const float* __restrict__ d2,
                                                       const int64_t* __restrict__ idx, const float* __restrict__ tgt, int64_t ld_t,
                                                       const float* __restrict__ nrm, int64_t ld_n, double* __restrict__ partials) {
  constexpr int USED = KIND == 1 ? 30 : 17;
  __shared__ double ws[4][MISO_ICP_SUMS];
  double acc[USED];
#pragma unroll
  for (int a = 0; a < USED; ++a) acc[a] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < k.n; i += stride) {
    const int64_t j = idx[i];
    const double dd = (double)d2[i];
    if (j < 0 || j >= k.m || !(dd <= k.max2)) continue;
    const double p[3] = {(double)moved[i * 3], (double)moved[i * 3 + 1], (double)moved[i * 3 + 2]};
    const double q[3] = {(double)tgt[j * ld_t], (double)tgt[j * ld_t + 1], (double)tgt[j * ld_t + 2]};
    acc[0] += 1.0;
    acc[1] += dd;
    if (KIND == 1) {
      const double nv[3] = {(double)nrm[j * ld_n], (double)nrm[j * ld_n + 1], (double)nrm[j * ld_n + 2]};
      const double e[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
      const double r = (e[0] * nv[0] + e[1] * nv[1]) + e[2] * nv[2];
      const double J[6] = {p[1] * nv[2] - p[2] * nv[1], p[2] * nv[0] - p[0] * nv[2], p[0] * nv[1] - p[1] * nv[0],
                           nv[0], nv[1], nv[2]};
      double w = 1.0;
      if (LOSS == 1) {
        const double s = r / k.k, u = 1.0 - s * s;
        w = fabs(r) <= k.k ? u * u : 0.0;
      }
      int at = 2;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const double wj = w * J[a];
#pragma unroll
        for (int b = a; b < 6; ++b) acc[at++] += wj * J[b];
      }
#pragma unroll
      for (int a = 0; a < 6; ++a) acc[23 + a] += (w * J[a]) * r;
      acc[29] += (w * r) * r;
    } else {
      const double a3[3] = {p[0] - k.origin[0], p[1] - k.origin[1], p[2] - k.origin[2]};
      const double b3[3] = {q[0] - k.origin[0], q[1] - k.origin[1], q[2] - k.origin[2]};
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        acc[2 + a] += a3[a];
        acc[5 + a] += b3[a];
#pragma unroll
        for (int b = 0; b < 3; ++b) acc[8 + 3 * a + b] += b3[a] * a3[b];
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < USED; ++a) {
    double v = acc[a];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) ws[wave][a] = v;
  }
  __syncthreads();
  if (threadIdx.x < MISO_ICP_SUMS) {
    const int a = threadIdx.x;
    partials[(int64_t)blockIdx.x * MISO_ICP_SUMS + a] = a < USED ? ((ws[0][a] + ws[1][a]) + ws[2][a]) + ws[3][a] : 0.0;
  }
}

__global__ __launch_bounds__(64) void icp_finish_kernel(const double* __restrict__ partials, int nb, double* __restrict__ out) {
  const int a = threadIdx.x;
  if (a >= MISO_ICP_SUMS) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += partials[(int64_t)b * MISO_ICP_SUMS + a];
  out[a] = s;
}

inline int icp_blocks(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (int)(b > MISO_ICP_MAX_BLOCKS ? MISO_ICP_MAX_BLOCKS : b);
}

// ---- normals -----------------------------------------------------------------------------------------------------------
// (smallest_eigenvector / NormalSums / normal_from_sums: nn.hpp, shared with the k-nearest normals of knn.hip)
__global__ __launch_bounds__(256) void nn_normals_kernel(NnK k, const int* __restrict__ table, const float4* __restrict__ rows,
                                                         const float* __restrict__ pts, int64_t ld, int64_t n, double radius,
                                                         float* __restrict__ normals, int32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float qf[3] = {pts[i * ld], pts[i * ld + 1], pts[i * ld + 2]};
  const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
  const double r2 = radius * radius;
  NormalSums acc;
  acc.clear();
  if (k.n_tgt > 0) {
    int clo[3], chi[3];
    const float rf = (float)radius;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float rs = rf + 0x1p-21f * (fabsf(qf[a]) + rf);
      clo[a] = nn_cell_axis(qf[a] - rs, k.lo[a], k.cell, k.dims[a]);
      chi[a] = nn_cell_axis(qf[a] + rs, k.lo[a], k.cell, k.dims[a]);
    }
    const auto add = [&](const float4& t, int) {
      const double d[3] = {(double)t.x - q[0], (double)t.y - q[1], (double)t.z - q[2]};
      const double d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
      if (d2 <= r2) acc.add(d);
    };
    // the box, z outer, y inner, one x run per (z, y): the order the sums are added in
    for (int z = clo[2]; z <= chi[2]; ++z)
      for (int y = clo[1]; y <= chi[1]; ++y) {
        const int row = (z * k.dims[1] + y) * k.dims[0];
        nn_visit_run(table, rows, (int)k.n_tgt, row + clo[0], row + chi[0], add);
      }
  }
  double v[3];
  normal_from_sums(acc, v);
  normals[i * 3] = (float)v[0]; normals[i * 3 + 1] = (float)v[1]; normals[i * 3 + 2] = (float)v[2];
  counts[i] = (int32_t)acc.cnt;
}

}  // namespace

hipError_t launch_icp_transform(const float* pose, const float* src, int64_t ld, int64_t n, float* out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  IcpPose T;
  for (int a = 0; a < 9; ++a) T.R[a] = pose[a];
  for (int a = 0; a < 3; ++a) T.t[a] = pose[9 + a];
  icp_transform_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(T, src, ld, n, out);
  return hipGetLastError();
}

int64_t icp_workspace_bytes(int64_t n) {
  const int b = icp_blocks(n);
  return (int64_t)(b < 1 ? 1 : b) * MISO_ICP_SUMS * 8;
}

hipError_t launch_icp_sums(const float* moved, const float* d2, const int64_t* idx, int64_t n, const float* tgt, int64_t ld_t,
                           int64_t m, const float* normals, int64_t ld_n, double max_dist, int kind, int loss, double tukey_k,
                           const double* origin, void* workspace, double* out, hipStream_t s) {
  IcpK k;
  k.n = n; k.m = m; k.max2 = max_dist * max_dist; k.k = tukey_k;
  for (int a = 0; a < 3; ++a) k.origin[a] = origin ? origin[a] : 0.0;
  double* partials = reinterpret_cast<double*>(workspace);
  const int nb = icp_blocks(n);
  if (nb > 0) {
    if (kind == 1 && loss == 1) icp_sums_kernel<1, 1><<<nb, 256, 0, s>>>(k, moved, d2, idx, tgt, ld_t, normals, ld_n, partials);
    else if (kind == 1) icp_sums_kernel<1, 0><<<nb, 256, 0, s>>>(k, moved, d2, idx, tgt, ld_t, normals, ld_n, partials);
    else icp_sums_kernel<0, 0><<<nb, 256, 0, s>>>(k, moved, d2, idx, tgt, ld_t, nullptr, 0, partials);
  }
  icp_finish_kernel<<<1, 64, 0, s>>>(partials, nb, out);
  return hipGetLastError();
}

hipError_t launch_nn_normals(const miso_nn_plan_t& p, const void* ws, const float* pts, int64_t ld, int64_t n, double radius,
                             float* normals, int32_t* counts, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const auto v = nn_views(p, p.n_tgt > 0 ? ws : nullptr);
  nn_normals_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(nn_k(p), v.table, v.rows, pts, ld, n, radius, normals, counts);
  return hipGetLastError();
}

}  // namespace miso

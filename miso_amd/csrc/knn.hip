// Exact k nearest neighbours of every query among the targets of the cell-list index (nn.hip), 1 <= k <= MISO_NN_KNN_MAX:
// what pytorch3d's knn_points(K = k) and Open3D's KDTreeSearchParamKNN (estimate_normals' default, k = 30) ask for.  The
// arithmetic and the order are those of nn.hip:
//     d2 = ((ax - bx)^2 + (ay - by)^2) + (az - bz)^2        fp32, one rounding per operation
// and the answer of a query is the k smallest (d2, original target index) pairs in lexicographic order, listed ascending.
// A NaN or +inf d2 is never a neighbour (both comparisons of KnnList::offer are false for it); a query with a non-finite
// coordinate, and the slots beyond the number of finite targets, get (+inf, -1).  The k smallest pairs of a set do not
// depend on the order in which the set is visited, so the answer depends neither on the visiting order, nor on the order
// the build's atomics left inside a cell, nor on the kernel.
//
// The list.  A lane holds its query's list in LDS, sorted ascending, laid out [slot][lane] (the 64 lanes of a wavefront
// touch consecutive words): KNN_LANES x 32 slots x (4 B d2 + 4 B payload) = 32 KB a block of 128 lanes.  The worst kept
// pair lives in registers as the admission threshold, (+inf, -1) while the list is short, so a candidate touches LDS
// only when it beats the threshold; it is then inserted by shifting the larger entries one slot up (the last one falls
// out of a full list).  No per-lane array is indexed at run time: nothing goes to scratch.
//   payload  the original target index (neighbour lists), or the target's ROW in the index (normals: the epilogue reads
//            the neighbours' coordinates from the rows, which hold the original index in .w; a tie on d2 reads it there).
//
// Rings (knn_rings_kernel), a lane per query: the walk of nn.hip's rings (nn_shell, nn_visit_shell_row; nn.hpp), with the
// list as its accumulator.  A query is finished after ring r when its list holds k entries and ring_finished(k, q, c, r,
// worst kept d2) holds, or when every face of the examined box is on the grid's edge (then with fewer than k entries:
// there are no more targets).  The argument of ring_finished (nn.hpp) carries over with `best` = the worst kept d2: a
// target outside the box has a computed d2 strictly above it, so it loses against every kept entry whatever its index.
// Unfinished queries append themselves to the chunk's list (nn_defer) and write nothing.
//
// All pairs (knn_all_pairs_kernel; queries and tiles as nn.hip's: nn_block_query, nn_stage_tile).  LISTED: the queries
// the rings left, over the index's rows; each starts from an EMPTY list (the scan meets every target, those the rings
// had taken too) and one block sees ALL targets, tile by tile: a list of k entries has no 64-bit atomicMin to merge
// segments with, and one segment per block needs no second buffer and is deterministic.  Blocks whose first slot is at
// or beyond the device-side count leave as a whole, before any barrier, so the launch is sized for the worst case and
// the host reads nothing.  Else: every query over the caller's arrays, the second route (miso_nn_knn_all_pairs).
//
// Epilogue (knn_finish).  Lists: the lane writes its row of out_d2 / out_idx (n, k), padded with (+inf, -1).  Normals:
// 1, d and d d^T, d = t - q in float64, are added in the list's order, ascending (d2, index): the order is a function of
// the clouds alone, so the bits of a normal do not change with the build.  Covariance and eigenvector: normal_from_sums
// (nn.hpp), the code of the radius normals.
#include "common.hpp"
#include "launch.hpp"
#include "nn.hpp"

#pragma clang fp contract(off)

namespace miso {
namespace {

constexpr int KNN_LANES = 128;                                     // queries a block
constexpr int KNN_TILE = 1024;                                     // targets per LDS tile of the all-pairs kernel (16 KB)
static_assert(KNN_LANES * MISO_NN_KNN_MAX * 8 + KNN_TILE * 16 <= 64 * 1024, "a block's LDS");

// A lane's view of its list: column `lane` of d[slot][lane] / p[slot][lane]
template <bool ROWPOS>
struct KnnList {
  float* d;
  int* p;
  const float4* rows;          // ROWPOS: the payload is a row of these
  int k, cnt;
  float wd;                    // the admission threshold: the worst kept (d2, original index) once cnt == k
  int wi;

  __device__ __forceinline__ void open(float* ld, int* lp, const float4* r, int k_) {
    d = ld + threadIdx.x; p = lp + threadIdx.x; rows = r; k = k_; cnt = 0;
    wd = __builtin_huge_valf(); wi = -1;
  }
  __device__ __forceinline__ int original(int payload) const { return ROWPOS ? __float_as_int(rows[payload].w) : payload; }

  // false for a NaN d2, and for d2 = +inf against the initial (+inf, -1)
  __device__ __forceinline__ void offer(float d2, int idx, int payload) {
    if (!(d2 < wd || (d2 == wd && idx < wi))) return;
    int s = cnt < k ? cnt : k - 1;                                 // the slot that opens: a full list drops its last entry
    while (s > 0) {
      const float pd = d[(s - 1) * KNN_LANES];
      const int pp = p[(s - 1) * KNN_LANES];
      if (pd < d2 || (pd == d2 && original(pp) < idx)) break;
      d[s * KNN_LANES] = pd; p[s * KNN_LANES] = pp;
      --s;
    }
    d[s * KNN_LANES] = d2; p[s * KNN_LANES] = payload;
    if (cnt < k) ++cnt;
    if (cnt == k) { wd = d[(k - 1) * KNN_LANES]; wi = original(p[(k - 1) * KNN_LANES]); }
  }
  // target t, row `row` of the index (ROWPOS only), as a candidate of query q
  __device__ __forceinline__ void take(float qx, float qy, float qz, const float4& t, int row) {
    const int idx = __float_as_int(t.w);
    offer(nn_dist2(qx, qy, qz, t.x, t.y, t.z), idx, ROWPOS ? row : idx);
  }
  // the stop test's `best`: the worst kept d2, and nothing is excluded while the list is short
  __device__ __forceinline__ float bound() const { return cnt == k ? wd : __builtin_huge_valf(); }
};

// what a finished query writes: its row of the lists, or its normal and count
template <bool NORMALS>
__device__ __forceinline__ void knn_finish(const KnnList<NORMALS>& l, int64_t i, const float qf[3],
                                           float* __restrict__ out_d2, int64_t* __restrict__ out_idx,
                                           float* __restrict__ normals, int32_t* __restrict__ counts) {
  if (!NORMALS) {
    for (int s = 0; s < l.k; ++s) {
      const bool has = s < l.cnt;
      out_d2[i * l.k + s] = has ? l.d[s * KNN_LANES] : __builtin_huge_valf();
      out_idx[i * l.k + s] = has ? (int64_t)l.p[s * KNN_LANES] : (int64_t)-1;
    }
  } else {
    const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
    NormalSums acc;
    acc.clear();
    for (int s = 0; s < l.cnt; ++s) {
      const float4 t = l.rows[l.p[s * KNN_LANES]];
      const double d[3] = {(double)t.x - q[0], (double)t.y - q[1], (double)t.z - q[2]};
      acc.add(d);
    }
    double v[3];
    normal_from_sums(acc, v);
    normals[i * 3] = (float)v[0]; normals[i * 3 + 1] = (float)v[1]; normals[i * 3 + 2] = (float)v[2];
    counts[i] = l.cnt;
  }
}

// ---- rings -------------------------------------------------------------------------------------------------------------
template <bool NORMALS>
__global__ __launch_bounds__(KNN_LANES) void knn_rings_kernel(NnK k, int kk, const int* __restrict__ table, const float4* __restrict__ rows,
                                                              const float* __restrict__ src, int64_t ld, int64_t first, int count,
                                                              float* __restrict__ out_d2, int64_t* __restrict__ out_idx,
                                                              float* __restrict__ normals, int32_t* __restrict__ counts,
                                                              int* __restrict__ list, int* __restrict__ list_n, int* __restrict__ stats) {
  __shared__ float list_d[MISO_NN_KNN_MAX * KNN_LANES];
  __shared__ int list_p[MISO_NN_KNN_MAX * KNN_LANES];
  const int li = blockIdx.x * KNN_LANES + threadIdx.x;
  const bool live = li < count;
  const int64_t i = first + li;
  bool done = true;
  if (live) {
    const float q[3] = {src[i * ld], src[i * ld + 1], src[i * ld + 2]};
    KnnList<NORMALS> l;
    l.open(list_d, list_p, rows, kk);
    if (nn_finite3(q[0], q[1], q[2])) {
      int c[3];
      nn_cell_of(k, q[0], q[1], q[2], c);
      done = false;
      for (int r = 0; r <= k.max_rings && !done; ++r) {
        const NnShell s = nn_shell(k, c, r);
        for (int z = s.lo[2]; z <= s.hi[2]; ++z)
          for (int y = s.lo[1]; y <= s.hi[1]; ++y) nn_visit_shell_row(k, table, rows, c, r, s, z, y, q, l);
        done = ring_finished(k, q, c, r, l.bound());
      }
    }
    if (done) knn_finish<NORMALS>(l, i, q, out_d2, out_idx, normals, counts);
  }
  nn_defer<true>(live, done, li, count, list, list_n, stats);
}

// ---- all pairs ---------------------------------------------------------------------------------------------------------
// LISTED: targets are the index's rows, queries list[slot] of the chunk for slot < *list_n.  Else: the caller's (m, 3)
// targets with row stride ld_t, query `slot` of n.  A block sees every target.
template <bool LISTED, bool NORMALS>
__global__ __launch_bounds__(KNN_LANES) void knn_all_pairs_kernel(int kk, const float4* __restrict__ rows, const float* __restrict__ tgt,
                                                                  int64_t ld_t, int64_t m, const float* __restrict__ src, int64_t ld_s,
                                                                  int64_t first, int64_t n, const int* __restrict__ list,
                                                                  const int* __restrict__ list_n, float* __restrict__ out_d2,
                                                                  int64_t* __restrict__ out_idx, float* __restrict__ normals,
                                                                  int32_t* __restrict__ counts) {
  static_assert(LISTED || !NORMALS, "normals read the neighbours from the index's rows");
  __shared__ float4 tile[KNN_TILE];
  __shared__ float list_d[MISO_NN_KNN_MAX * KNN_LANES];
  __shared__ int list_p[MISO_NN_KNN_MAX * KNN_LANES];
  bool live; int64_t i; float q[3];
  if (!nn_block_query<LISTED, KNN_LANES>(src, ld_s, first, n, list, list_n, live, i, q)) return;
  KnnList<NORMALS> l;
  l.open(list_d, list_p, rows, kk);                                   // empty: the scan meets every target once
  for (int64_t t0 = 0; t0 < m; t0 += KNN_TILE) {
    const int len = (int)(m - t0 < KNN_TILE ? m - t0 : KNN_TILE);
    nn_stage_tile<LISTED, KNN_LANES>(tile, len, rows, tgt, ld_t, t0);
    if (live)
      for (int j = 0; j < len; ++j) l.take(q[0], q[1], q[2], tile[j], (int)(t0 + j));   // one address per wavefront: a broadcast
  }
  if (live) knn_finish<NORMALS>(l, i, q, out_d2, out_idx, normals, counts);
}

__global__ __launch_bounds__(256) void knn_flat_normals_kernel(int64_t n, float* __restrict__ normals, int32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) { normals[i * 3] = 0.0f; normals[i * 3 + 1] = 0.0f; normals[i * 3 + 2] = 1.0f; counts[i] = 0; }
}

// the chunks of a query over the index: rings, then the all-pairs kernel for the queries they listed
template <bool NORMALS>
hipError_t knn_on_index(const miso_nn_plan_t& p, void* ws, const float* src, int64_t ld, int64_t n, int kk, float* out_d2,
                        int64_t* out_idx, float* normals, int32_t* counts, int32_t* stats, hipStream_t s) {
  const auto v = nn_views(p, ws);
  const NnK k = nn_k(p);
  const hipError_t e = launch_zero_words(v.counters, nn_chunks(n), s);
  if (e != hipSuccess) return e;
  nn_for_chunks(n, [&](int c, int64_t first, int count) {
    const unsigned g = (unsigned)((count + KNN_LANES - 1) / KNN_LANES);
    knn_rings_kernel<NORMALS><<<g, KNN_LANES, 0, s>>>(k, kk, v.table, v.rows, src, ld, first, count, out_d2, out_idx, normals, counts,
                                                      v.list, v.counters + c, stats);
    knn_all_pairs_kernel<true, NORMALS><<<g, KNN_LANES, 0, s>>>(kk, v.rows, nullptr, 0, p.n_tgt, src, ld, first, (int64_t)count, v.list,
                                                                v.counters + c, out_d2, out_idx, normals, counts);
  });
  return hipGetLastError();
}

}  // namespace

hipError_t launch_nn_knn(const miso_nn_plan_t& p, void* ws, const float* src, int64_t ld, int64_t n, int k, float* out_d2,
                         int64_t* out_idx, int32_t* stats, hipStream_t s) {
  if (p.n_tgt == 0) {
    const hipError_t e = launch_nn_set_stats(stats, (int)n, 0, s);
    return e != hipSuccess ? e : launch_nn_fill(n * k, out_d2, out_idx, s);
  }
  hipError_t e = launch_zero_words(stats, 2, s);
  if (e != hipSuccess || n == 0) return e;
  return knn_on_index<false>(p, ws, src, ld, n, k, out_d2, out_idx, nullptr, nullptr, stats, s);
}

hipError_t launch_nn_knn_all_pairs(const float* tgt, int64_t ld_t, int64_t m, const float* src, int64_t ld_s, int64_t n, int k,
                                   float* out_d2, int64_t* out_idx, hipStream_t s) {
  if (n == 0) return hipSuccess;
  // (m == 0: no tile is loaded and every list stays empty)
  nn_for_chunks(n, [&](int, int64_t first, int count) {
    knn_all_pairs_kernel<false, false><<<(unsigned)((count + KNN_LANES - 1) / KNN_LANES), KNN_LANES, 0, s>>>(
        k, nullptr, tgt, ld_t, m, src, ld_s, first, (int64_t)count, nullptr, nullptr, out_d2, out_idx, nullptr, nullptr);
  });
  return hipGetLastError();
}

hipError_t launch_nn_knn_normals(const miso_nn_plan_t& p, void* ws, const float* pts, int64_t ld, int64_t n, int k, float* normals,
                                 int32_t* counts, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (p.n_tgt == 0) {
    knn_flat_normals_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(n, normals, counts);
    return hipGetLastError();
  }
  return knn_on_index<true>(p, ws, pts, ld, n, k, nullptr, nullptr, normals, counts, nullptr, s);
}

}  // namespace miso

// Exact nearest neighbour of every query among a target cloud: what utils_eval.nn_correspondance (grid_opt/utils/
// utils_eval.py:14-36) asks of pytorch3d's knn_points with K = 1, an all-pairs search.  Here a uniform cell list over the
// targets' bounding box answers a query from the shells of cells around it, and the queries it cannot finish within
// max_rings shells go to an all-pairs kernel.  Both compute
//     d2 = ((ax - bx)^2 + (ay - by)^2) + (az - bz)^2        fp32, one rounding per operation
// and the winner is the smallest (d2, original target index) pair, compared lexicographically: the answer depends neither
// on the order in which candidates are visited, nor on the order atomics left inside a cell, nor on the kernel.  A NaN
// or +inf d2 never wins (both comparisons below are false for it), so a query or target with a non-finite coordinate gives
// or takes no match: (d2, idx) = (+inf, -1).
//
// Index (miso_nn_build; workspace layout in nn_layout):
//   table  cells + 1 int32.  count: table[c + 1] += 1 per target of cell c.  scan: table[c + 1] = targets in cells < c
//          (three launches: block sums of 16 384, a scan of up to 1024 sums, the blocks again).  scatter: a target takes
//          row atomicAdd(&table[c + 1], 1), which leaves table[c] = first row of cell c and table[c + 1] = one past its last.
//   rows   {x, y, z, original index bits} per target in cell order, 16 bytes: a candidate is one dwordx4 load.
//   cell   c_a = int(clamp(floor((p_a - min_a) / cell), 0, dims_a - 1)), clamped as a float (fmaxf / fminf drop a NaN), so
//          any input indexes inside the table; linear index (z dims_y + y) dims_x + x: the cells of an x run are one run
//          of rows.
// Query (miso_nn_query), a lane per query, chunks of NN_CHUNK queries (nn_for_chunks).  The walk, the deferral and the
// staging are nn.hpp's, shared with knn.hip; what is this file's is the accumulator, Best::take:
//   rings  shell r = 0, 1, .. max_rings around the query's (clamped) cell (nn_shell, nn_visit_shell_row), then the stop
//          test (ring_finished).  Unfinished queries append themselves to the chunk's list (nn_defer).
//   rest   blocks of 256 listed queries (nn_block_query) against the rows, staged through LDS in tiles (nn_stage_tile),
//          the rows split over grid.y and merged with a 64-bit atomicMin on the packed (d2, idx); a block whose first
//          list slot is at or beyond the device counter leaves, so the launch is sized for the worst case and the host
//          reads nothing.  Then the pairs are unpacked.
// miso_nn_all_pairs is the second kernel over the caller's arrays, every query, no index.
#include "common.hpp"
#include "launch.hpp"
#include "nn.hpp"

// plain operators, one rounding each (see voxel.hip on why not the __fmul_rn / __fadd_rn wrappers)
#pragma clang fp contract(off)

namespace miso {
namespace {

constexpr int NN_SCAN_THREADS = 1024;
constexpr int NN_SCAN_ITEMS = 16;
constexpr int NN_SCAN_TILE = NN_SCAN_THREADS * NN_SCAN_ITEMS;      // 16 384 table entries per block; 1024 blocks = the cap
static_assert((int64_t)NN_SCAN_TILE * 1024 >= MISO_NN_MAX_CELLS, "one block scans the block sums");
constexpr int NN_TILE = 1024;                                      // targets per LDS tile of the all-pairs kernel (16 KB)
constexpr int NN_SEG_TILES = 8;                                    // the listed queries' all-pairs: at least 8 tiles a segment,
constexpr int NN_SEGMENTS = 64;                                    // at most 64 segments (grid.y)

// (d2, idx) as one unsigned 64-bit key that orders like the pair: d2 >= +0 (floats then order like their bits), idx as
// uint32 (-1 = the largest: no match).  The all-pairs kernel behind the rings merges its target segments with atomicMin.
__device__ __forceinline__ unsigned long long nn_pack(const Best& b) {
  return ((unsigned long long)__float_as_uint(b.d2) << 32) | (unsigned long long)(uint32_t)b.idx;
}

// ---- build -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nn_count_kernel(NnK k, const float* __restrict__ tgt, int64_t ld, int* __restrict__ table) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= k.n_tgt) return;
  int c[3];
  const int cell = nn_cell_of(k, tgt[i * ld], tgt[i * ld + 1], tgt[i * ld + 2], c);
  atomicAdd(&table[cell + 1], 1);
}

// sums of the blocks' NN_SCAN_TILE entries of t[0 .. n)
__global__ __launch_bounds__(NN_SCAN_THREADS) void nn_scan_sums_kernel(const int* __restrict__ t, int n, int* __restrict__ sums) {
  __shared__ int ws[NN_SCAN_THREADS / 64];
  const int base = blockIdx.x * NN_SCAN_TILE + threadIdx.x * NN_SCAN_ITEMS;
  int s = 0;
#pragma unroll
  for (int j = 0; j < NN_SCAN_ITEMS; ++j) s += base + j < n ? t[base + j] : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int w = 0; w < NN_SCAN_THREADS / 64; ++w) tot += ws[w];
    sums[blockIdx.x] = tot;
  }
}

// exclusive scan of `v` over the block's 1024 threads; returns the prefix of this thread
__device__ __forceinline__ int nn_block_exclusive(int v, int* ws) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int w = __shfl_up(inc, o); if (lane >= o) inc += w; }
  if (lane == 63) ws[wave] = inc;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += ws[w];
  return base + inc - v;
}

__global__ __launch_bounds__(NN_SCAN_THREADS) void nn_scan_blocks_kernel(int* __restrict__ sums, int nb) {
  __shared__ int ws[NN_SCAN_THREADS / 64];
  const int v = (int)threadIdx.x < nb ? sums[threadIdx.x] : 0;
  const int pre = nn_block_exclusive(v, ws);
  if ((int)threadIdx.x < nb) sums[threadIdx.x] = pre;
}

__global__ __launch_bounds__(NN_SCAN_THREADS) void nn_scan_apply_kernel(int* __restrict__ t, int n, const int* __restrict__ sums) {
  __shared__ int ws[NN_SCAN_THREADS / 64];
  const int base = blockIdx.x * NN_SCAN_TILE + threadIdx.x * NN_SCAN_ITEMS;
  int v[NN_SCAN_ITEMS], s = 0;
#pragma unroll
  for (int j = 0; j < NN_SCAN_ITEMS; ++j) { v[j] = base + j < n ? t[base + j] : 0; s += v[j]; }
  int run = nn_block_exclusive(s, ws) + sums[blockIdx.x];
#pragma unroll
  for (int j = 0; j < NN_SCAN_ITEMS; ++j) {
    if (base + j < n) t[base + j] = run;
    run += v[j];
  }
}

__global__ __launch_bounds__(256) void nn_scatter_kernel(NnK k, const float* __restrict__ tgt, int64_t ld, int* __restrict__ table,
                                                         float4* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= k.n_tgt) return;
  const float x = tgt[i * ld], y = tgt[i * ld + 1], z = tgt[i * ld + 2];
  int c[3];
  const int cell = nn_cell_of(k, x, y, z, c);
  const int at = atomicAdd(&table[cell + 1], 1);
  if (at >= 0 && (int64_t)at < k.n_tgt) rows[at] = make_float4(x, y, z, __int_as_float((int)i));
}

// ---- query: rings ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nn_rings_kernel(NnK k, const int* __restrict__ table, const float4* __restrict__ rows,
                                                       const float* __restrict__ src, int64_t ld, int64_t first, int count,
                                                       float* __restrict__ out_d2, int64_t* __restrict__ out_idx,
                                                       int* __restrict__ list, int* __restrict__ list_n, int* __restrict__ stats) {
  const int li = blockIdx.x * 256 + threadIdx.x;
  const bool live = li < count;
  const int64_t i = first + li;
  bool done = true;
  if (live) {
    const float q[3] = {src[i * ld], src[i * ld + 1], src[i * ld + 2]};
    Best b = {__builtin_huge_valf(), -1};
    if (nn_finite3(q[0], q[1], q[2])) {
      int c[3];
      nn_cell_of(k, q[0], q[1], q[2], c);
      done = false;
      for (int r = 0; r <= k.max_rings && !done; ++r) {
        const NnShell s = nn_shell(k, c, r);
        for (int z = s.lo[2]; z <= s.hi[2]; ++z)
          for (int y = s.lo[1]; y <= s.hi[1]; ++y) nn_visit_shell_row(k, table, rows, c, r, s, z, y, q, b);
        done = ring_finished(k, q, c, r, b.d2);
      }
    }
    if (done) { out_d2[i] = b.d2; out_idx[i] = (int64_t)b.idx; }
    else out_idx[i] = (int64_t)nn_pack(b);        // the best of the rings so far: the accumulator of the all-pairs blocks
  }
  nn_defer<false>(live, done, li, count, list, list_n, stats);
}

// ---- all pairs ---------------------------------------------------------------------------------------------------------
// LISTED: the kernel behind the rings.  Targets are the index's rows (the original index in .w), queries list[slot] of the
// chunk for slot < *list_n, and blockIdx.y takes the targets [y seg_len, (y + 1) seg_len): a few hundred listed queries
// against all targets are a few blocks, each bound by its own latency, unless the targets are spread over the device.
// The segments merge with a 64-bit atomicMin on the packed pair in out_idx[i] (seeded by the rings kernel), which
// nn_unpack_kernel turns into (d2, idx).  Else: the caller's (m, 3) targets with row stride ld_t, query `slot` of n, one
// segment, results written directly.
template <bool LISTED>
__global__ __launch_bounds__(256) void nn_all_pairs_kernel(const float4* __restrict__ rows, const float* __restrict__ tgt, int64_t ld_t,
                                                           int64_t m, int64_t seg_len, const float* __restrict__ src, int64_t ld_s,
                                                           int64_t first, int64_t n, const int* __restrict__ list,
                                                           const int* __restrict__ list_n, float* __restrict__ out_d2,
                                                           int64_t* __restrict__ out_idx) {
  __shared__ float4 tile[NN_TILE];
  bool live; int64_t i; float q[3];
  if (!nn_block_query<LISTED, 256>(src, ld_s, first, n, list, list_n, live, i, q)) return;
  Best b = {__builtin_huge_valf(), -1};
  const int64_t t_begin = (int64_t)blockIdx.y * seg_len, t_end = t_begin + seg_len < m ? t_begin + seg_len : m;
  for (int64_t t0 = t_begin; t0 < t_end; t0 += NN_TILE) {
    const int len = (int)(t_end - t0 < NN_TILE ? t_end - t0 : NN_TILE);
    nn_stage_tile<LISTED, 256>(tile, len, rows, tgt, ld_t, t0);
#pragma unroll 4
    for (int j = 0; j < len; ++j) {                                   // (dead lanes too: the loop as it was measured)
      const float4 t = tile[j];                                       // one address per wavefront: a broadcast
      b.take(q[0], q[1], q[2], t, 0);
    }
  }
  if (!live) return;
  if (LISTED) {
    if (b.idx >= 0) atomicMin(reinterpret_cast<unsigned long long*>(out_idx + i), nn_pack(b));
  } else {
    out_d2[i] = b.d2; out_idx[i] = (int64_t)b.idx;
  }
}

// the merged pairs of the listed queries -> (d2, idx)
__global__ __launch_bounds__(256) void nn_unpack_kernel(int64_t first, int n, const int* __restrict__ list, const int* __restrict__ list_n,
                                                        float* __restrict__ out_d2, int64_t* __restrict__ out_idx) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= nn_listed_count(list_n, n)) return;
  const int64_t i = nn_listed_query(list, slot, first, n);
  const unsigned long long key = (unsigned long long)out_idx[i];
  out_d2[i] = __uint_as_float((uint32_t)(key >> 32));
  out_idx[i] = (int64_t)(int32_t)(uint32_t)key;
}

__global__ __launch_bounds__(256) void nn_fill_kernel(int64_t total, float* __restrict__ out_d2, int64_t* __restrict__ out_idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total) { out_d2[i] = __builtin_huge_valf(); out_idx[i] = -1; }
}

__global__ void nn_set_stats_kernel(int* __restrict__ stats, int a, int b) {
  if (threadIdx.x == 0 && blockIdx.x == 0) { stats[0] = a; stats[1] = b; }
}

}  // namespace

int64_t nn_workspace_bytes(const miso_nn_plan_t& p) { return nn_layout(p).total; }

hipError_t launch_nn_fill(int64_t total, float* out_d2, int64_t* out_idx, hipStream_t s) {
  if (total > 0) nn_fill_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(total, out_d2, out_idx);
  return hipGetLastError();
}

hipError_t launch_nn_set_stats(int32_t* stats, int a, int b, hipStream_t s) {
  nn_set_stats_kernel<<<1, 64, 0, s>>>(stats, a, b);
  return hipGetLastError();
}

// counts[0 .. n) -> their exclusive prefix sums, in place (n <= MISO_NN_MAX_CELLS; sums: 1024 ints of scratch)
hipError_t launch_nn_scan(int* counts, int n, int* sums, hipStream_t s) {
  const int nb = (n + NN_SCAN_TILE - 1) / NN_SCAN_TILE;
  nn_scan_sums_kernel<<<nb, NN_SCAN_THREADS, 0, s>>>(counts, n, sums);
  nn_scan_blocks_kernel<<<1, NN_SCAN_THREADS, 0, s>>>(sums, nb);
  nn_scan_apply_kernel<<<nb, NN_SCAN_THREADS, 0, s>>>(counts, n, sums);
  return hipGetLastError();
}

hipError_t launch_nn_build(const miso_nn_plan_t& p, const float* tgt, int64_t ld, void* ws, hipStream_t s) {
  if (p.n_tgt == 0) return hipSuccess;
  const auto v = nn_views(p, ws);
  const NnK k = nn_k(p);
  const int cells = (int)p.cells;
  const unsigned g = (unsigned)((p.n_tgt + 255) / 256);
  hipError_t e = launch_zero_words(v.table, cells + 1, s);
  if (e != hipSuccess) return e;
  nn_count_kernel<<<g, 256, 0, s>>>(k, tgt, ld, v.table);
  e = launch_nn_scan(v.table + 1, cells, v.sums, s);
  if (e != hipSuccess) return e;
  nn_scatter_kernel<<<g, 256, 0, s>>>(k, tgt, ld, v.table, v.rows);
  return hipGetLastError();
}

hipError_t launch_nn_query(const miso_nn_plan_t& p, void* ws, const float* src, int64_t ld, int64_t n, float* out_d2,
                           int64_t* out_idx, int32_t* stats, hipStream_t s) {
  if (p.n_tgt == 0) {
    const hipError_t e = launch_nn_set_stats(stats, (int)n, 0, s);
    return e != hipSuccess ? e : launch_nn_fill(n, out_d2, out_idx, s);
  }
  hipError_t e = launch_zero_words(stats, 2, s);
  if (e != hipSuccess || n == 0) return e;
  const auto v = nn_views(p, ws);
  const NnK k = nn_k(p);
  // the listed queries see the targets in up to NN_SEGMENTS segments of at least NN_SEG_TILES tiles
  const int64_t tiles = (p.n_tgt + NN_TILE - 1) / NN_TILE;
  const unsigned segs = (unsigned)(tiles / NN_SEG_TILES < 1 ? 1 : (tiles / NN_SEG_TILES > NN_SEGMENTS ? NN_SEGMENTS : tiles / NN_SEG_TILES));
  const int64_t seg_len = (tiles + segs - 1) / segs * NN_TILE;
  e = launch_zero_words(v.counters, nn_chunks(n), s);
  if (e != hipSuccess) return e;
  nn_for_chunks(n, [&](int c, int64_t first, int count) {
    const unsigned g = (unsigned)((count + 255) / 256);
    nn_rings_kernel<<<g, 256, 0, s>>>(k, v.table, v.rows, src, ld, first, count, out_d2, out_idx, v.list, v.counters + c, stats);
    nn_all_pairs_kernel<true><<<dim3(g, segs), 256, 0, s>>>(v.rows, nullptr, 0, p.n_tgt, seg_len, src, ld, first, (int64_t)count, v.list,
                                                            v.counters + c, out_d2, out_idx);
    nn_unpack_kernel<<<g, 256, 0, s>>>(first, count, v.list, v.counters + c, out_d2, out_idx);
  });
  return hipGetLastError();
}

hipError_t launch_nn_all_pairs(const float* tgt, int64_t ld_t, int64_t m, const float* src, int64_t ld_s, int64_t n,
                               float* out_d2, int64_t* out_idx, hipStream_t s) {
  if (n == 0) return hipSuccess;
  // (m == 0: no tile is loaded and every query keeps (+inf, -1))
  nn_for_chunks(n, [&](int, int64_t first, int count) {
    nn_all_pairs_kernel<false><<<(unsigned)((count + 255) / 256), 256, 0, s>>>(nullptr, tgt, ld_t, m, m, src, ld_s, first, (int64_t)count,
                                                                               nullptr, nullptr, out_d2, out_idx);
  });
  return hipGetLastError();
}

}  // namespace miso

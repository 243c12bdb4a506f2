// utils_geometry.voxel_down_sample_torch (grid_opt/utils/utils_geometry.py:292-335) as the reference's RGB-D dataset runs it
// inside every __getitem__ (grid_opt/datasets/sdf_rgbd.py:460-470: .cpu(), unique + scatter_reduce on the host, six indexed
// gathers) and its LiDAR dataset per loaded frame (grid_opt/datasets/sdf_3d_lidar.py:108-122): one point per occupied voxel,
// the one closest to the voxel centre after quantising the distance into 1000 steps, ties to the lowest index, in the order
// of the sorted voxel keys.  Here: no host round trip, no allocation, a device live count, the same index array bit for bit.
//
// The arithmetic is the reference's CPU arithmetic, every operation rounded once to fp32 (true division, no contraction):
//   cell = floor(p / v); d = p - (cell + 0.5) v; dist = sqrt((dx^2 + dy^2) + dz^2); rank = trunc(dist / max(dist) * 999)
//   ijk = cell - floor(min(p) / v); side = float(max ijk); key = (ix + iy side) + (iz side) side          -- an fp32 key
// and two of its properties are reproduced, not repaired: `side` is the largest index, not the extent, so a cell with
// ix == side shares its key with (0, iy + 1, iz); and above 2^24 the fp32 key drops low bits, so neighbouring voxels merge.
//
// Launches (all sized by the capacity; rows at or beyond the live count are never read):
//   bounds   per-axis min / max of p and max(dist): block partials (order-independent, any tree gives the same bits)
//   finish   one block: lo = floor(min / v), side, max(dist) -> params
//   keys     composite = key bits << 32 | rank << 22 | index (keys are >= 0: floats order like their bit patterns)
//   6 x { hist, scan, scatter }   stable LSD radix sort of bits [22, 64), 8-bit digits.  A block owns a contiguous tile of
//            4096 composites, a wavefront a contiguous quarter-K of it; ranks inside a wavefront come from 64-bit ballot
//            matching, bases from the exclusive scan over (digit, block), so the order is fixed by the data alone.  A
//            digit that is the same in every live composite is skipped (the scan sees one full bin; the buffer parity is
//            a device word, so the host never learns it).
//   heads    count the first elements of key runs per tile, scan the tile counts (-> out_count), write the winners'
//            indices in key order and -1 behind them.
//   rows     (miso_voxel_select_rows) one gather of a RayBatch-shaped table through the selection, neutral rows behind it.
#include "common.hpp"
#include "launch.hpp"

// Products and sums below are plain operators under this pragma: one rounding each.  (The __fmul_rn / __fadd_rn wrappers
// are inline functions of the runtime's headers, compiled under the headers' contraction mode: a product feeding a sum
// through them is fused into one FMA, which rounds the reference's key (iz side) side + ... once instead of twice.)
#pragma clang fp contract(off)

namespace miso {
namespace {

constexpr int VOX_THREADS = 1024;                       // 16 wavefronts
constexpr int VOX_WAVES = VOX_THREADS / 64;
constexpr int VOX_ITEMS = 4;                            // composites per thread
constexpr int VOX_TILE = VOX_THREADS * VOX_ITEMS;       // 4096 per block
constexpr int VOX_WAVE_SPAN = 64 * VOX_ITEMS;           // 256 contiguous composites per wavefront
constexpr int VOX_RED_BLOCKS = 256;
constexpr int VOX_PASSES = 6;
constexpr int VOX_INDEX_BITS = 22;

// params (ints): [0..2] lo, [3] side (float bits), [4] max dist (float bits), [8 + p] source buffer of pass p (0 = a, 1 = b;
// [8 + VOX_PASSES] holds the sorted one), [16 + p] pass p is skipped
constexpr int P_SIDE = 3, P_MAXD = 4, P_SEL = 8, P_SKIP = 16, P_WORDS = 32;

__host__ __device__ constexpr int pass_shift(int p) { return VOX_INDEX_BITS + 8 * p; }
__host__ __device__ constexpr unsigned pass_mask(int p) { return pass_shift(p) + 8 <= 64 ? 255u : (1u << (64 - pass_shift(p))) - 1u; }

__device__ __forceinline__ int live_of(const int32_t* n_live, int cap) {
  if (!n_live) return cap;
  const int n = *n_live;
  return n < 0 ? 0 : (n > cap ? cap : n);
}

// cell (as floats) and distance to the cell centre of one point
__device__ __forceinline__ float cell_dist(const float p[3], float v, float cell[3]) {
  float sq[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    cell[a] = floorf(__fdiv_rn(p[a], v));
    const float d = p[a] - (cell[a] + 0.5f) * v;
    sq[a] = d * d;
  }
  return __fsqrt_rn((sq[0] + sq[1]) + sq[2]);
}

__global__ __launch_bounds__(256) void vox_bounds_kernel(const float* __restrict__ pts, int64_t ld, int cap,
                                                         const int32_t* __restrict__ n_live, float v,
                                                         float* __restrict__ partial) {
  __shared__ float red[4][7];
  const int n = live_of(n_live, cap);
  const float inf = __builtin_huge_valf();
  float r[7] = {inf, inf, inf, -inf, -inf, -inf, 0.0f};      // min xyz, max xyz, max dist
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += VOX_RED_BLOCKS * 256) {
    const float p[3] = {pts[(int64_t)i * ld], pts[(int64_t)i * ld + 1], pts[(int64_t)i * ld + 2]};
    float cell[3];
    const float d = cell_dist(p, v, cell);
#pragma unroll
    for (int a = 0; a < 3; ++a) { r[a] = fminf(r[a], p[a]); r[3 + a] = fmaxf(r[3 + a], p[a]); }
    r[6] = fmaxf(r[6], d);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const float w = __shfl_xor(r[k], o);
      r[k] = k < 3 ? fminf(r[k], w) : fmaxf(r[k], w);
    }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 7; ++k) red[wave][k] = r[k];
  __syncthreads();
  if (threadIdx.x < 7) {
    const int k = threadIdx.x;
    float w = red[0][k];
    for (int j = 1; j < 4; ++j) w = k < 3 ? fminf(w, red[j][k]) : fmaxf(w, red[j][k]);
    partial[blockIdx.x * 8 + k] = w;
  }
}

__global__ __launch_bounds__(VOX_RED_BLOCKS) void vox_finish_kernel(const float* __restrict__ partial, int cap,
                                                                    const int32_t* __restrict__ n_live, float v,
                                                                    int* __restrict__ params) {
  __shared__ float red[VOX_RED_BLOCKS / 64][7];
  float r[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) r[k] = partial[threadIdx.x * 8 + k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const float w = __shfl_xor(r[k], o);
      r[k] = k < 3 ? fminf(r[k], w) : fmaxf(r[k], w);
    }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 7; ++k) red[wave][k] = r[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    const int n = live_of(n_live, cap);
    for (int k = 0; k < 7; ++k)
      for (int j = 1; j < VOX_RED_BLOCKS / 64; ++j) r[k] = k < 3 ? fminf(r[k], red[j][k]) : fmaxf(r[k], red[j][k]);
    int side = 0;
    for (int a = 0; a < 3; ++a) {
      const int lo = n > 0 ? (int)floorf(__fdiv_rn(r[a], v)) : 0;
      const int hi = n > 0 ? (int)floorf(__fdiv_rn(r[3 + a], v)) : 0;
      params[a] = lo;
      side = max(side, hi - lo);      // = max over points and axes of cell - lo: floor and / v are monotone
    }
    params[P_SIDE] = __float_as_int((float)side);
    params[P_MAXD] = __float_as_int(r[6]);
    params[P_SEL] = 0;
  }
}

__global__ __launch_bounds__(256) void vox_keys_kernel(const float* __restrict__ pts, int64_t ld, int cap,
                                                       const int32_t* __restrict__ n_live, float v,
                                                       const int* __restrict__ params, uint64_t* __restrict__ comp) {
  const int n = live_of(n_live, cap);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float side = __int_as_float(params[P_SIDE]), maxd = __int_as_float(params[P_MAXD]);
  const float p[3] = {pts[(int64_t)i * ld], pts[(int64_t)i * ld + 1], pts[(int64_t)i * ld + 2]};
  float cell[3];
  const float d = cell_dist(p, v, cell);
  int rank = (int)truncf(__fdiv_rn(d, maxd) * 999.0f);
  rank = rank < 0 ? 0 : (rank > 1023 ? 1023 : rank);
  const float ix = (float)((int)cell[0] - params[0]), iy = (float)((int)cell[1] - params[1]),
              iz = (float)((int)cell[2] - params[2]);
  const float key = (ix + iy * side) + (iz * side) * side;
  comp[i] = ((uint64_t)__float_as_uint(key) << 32) | ((uint64_t)rank << VOX_INDEX_BITS) | (uint64_t)i;
}

// ---- one radix pass -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VOX_THREADS) void vox_hist_kernel(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b,
                                                               int cap, const int32_t* __restrict__ n_live, int pass,
                                                               const int* __restrict__ params, int* __restrict__ hist) {
  __shared__ int h[256];
  const int n = live_of(n_live, cap);
  if (threadIdx.x < 256) h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t* src = params[P_SEL + pass] ? b : a;
  const int shift = pass_shift(pass);
  const unsigned mask = pass_mask(pass);
  const int t0 = blockIdx.x * VOX_TILE;
#pragma unroll
  for (int k = 0; k < VOX_ITEMS; ++k) {
    const int i = t0 + k * VOX_THREADS + threadIdx.x;
    if (i < n) atomicAdd(&h[(unsigned)(src[i] >> shift) & mask], 1);
  }
  __syncthreads();
  if (threadIdx.x < 256) hist[blockIdx.x * 256 + threadIdx.x] = h[threadIdx.x];
}

// hist[b][d] <- number of composites that precede block b's digit-d run in the sorted order of this digit; the pass is
// skipped, and the buffer parity kept, when one digit holds every live composite
__global__ __launch_bounds__(1024) void vox_scan_kernel(int* __restrict__ hist, int nb, int cap,
                                                        const int32_t* __restrict__ n_live, int pass,
                                                        int* __restrict__ params) {
  __shared__ int part[4][256];
  __shared__ int tot[256];
  __shared__ int constant;
  const int n = live_of(n_live, cap);
  const int d = threadIdx.x & 255, seg = threadIdx.x >> 8;
  const int per = (nb + 3) / 4, b0 = min(nb, seg * per), b1 = min(nb, b0 + per);
  if (threadIdx.x == 0) constant = 0;
  int sum = 0;
  for (int b = b0; b < b1; ++b) sum += hist[b * 256 + d];
  part[seg][d] = sum;
  __syncthreads();
  if (seg == 0) {
    const int t = part[0][d] + part[1][d] + part[2][d] + part[3][d];
    tot[d] = t;
    if (t == n) constant = 1;
  }
  __syncthreads();
  const int skip = constant;
  if (threadIdx.x == 0) {
    const int sel = params[P_SEL + pass];
    params[P_SEL + pass + 1] = skip ? sel : sel ^ 1;
    params[P_SKIP + pass] = skip;
  }
  if (skip) return;
  int run = 0;
  for (int k = 0; k < d; ++k) run += tot[k];
  for (int s = 0; s < seg; ++s) run += part[s][d];
  for (int b = b0; b < b1; ++b) {
    const int c = hist[b * 256 + d];
    hist[b * 256 + d] = run;
    run += c;
  }
}

__global__ __launch_bounds__(VOX_THREADS) void vox_scatter_kernel(uint64_t* __restrict__ a, uint64_t* __restrict__ b, int cap,
                                                                  const int32_t* __restrict__ n_live, int pass,
                                                                  const int* __restrict__ params,
                                                                  const int* __restrict__ hist) {
  __shared__ int wh[VOX_WAVES][256];      // per wavefront and digit: count, then the running output position
  if (params[P_SKIP + pass]) return;
  const int n = live_of(n_live, cap);
  const int sel = params[P_SEL + pass];
  const uint64_t* src = sel ? b : a;
  uint64_t* dst = sel ? a : b;
  const int shift = pass_shift(pass);
  const unsigned mask = pass_mask(pass);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = threadIdx.x; k < VOX_WAVES * 256; k += VOX_THREADS) (&wh[0][0])[k] = 0;
  __syncthreads();
  const int w0 = blockIdx.x * VOX_TILE + wave * VOX_WAVE_SPAN;
  uint64_t c[VOX_ITEMS], same[VOX_ITEMS];
  unsigned dig[VOX_ITEMS];
#pragma unroll
  for (int r = 0; r < VOX_ITEMS; ++r) {
    const int i = w0 + r * 64 + lane;
    const bool ok = i < n;
    c[r] = ok ? src[i] : 0;
    dig[r] = (unsigned)(c[r] >> shift) & mask;
    uint64_t m = __ballot(ok);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (dig[r] >> bit) & 1u;
      const uint64_t v = __ballot(on);
      m &= on ? v : ~v;
    }
    same[r] = ok ? m : 0;      // the live lanes of this round that hold my digit
    if (ok && (same[r] & ((1ull << lane) - 1)) == 0) wh[wave][dig[r]] += __popcll(same[r]);     // one lane per digit
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  if (threadIdx.x < 256) {
    int run = hist[blockIdx.x * 256 + threadIdx.x];
    for (int w = 0; w < VOX_WAVES; ++w) {
      const int cnt = wh[w][threadIdx.x];
      wh[w][threadIdx.x] = run;
      run += cnt;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < VOX_ITEMS; ++r) {
    const uint64_t below = same[r] & ((1ull << lane) - 1);
    int pos = 0;
    if (same[r]) pos = wh[wave][dig[r]] + __popcll(below);
    __builtin_amdgcn_wave_barrier();
    if (same[r] && below == 0) wh[wave][dig[r]] += __popcll(same[r]);
    __builtin_amdgcn_wave_barrier();
    if (same[r] && pos < n) dst[pos] = c[r];
  }
}

// ---- heads of key runs ----------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_head(const uint64_t* s, int i, int n) {
  return i < n && (i == 0 || (uint32_t)(s[i] >> 32) != (uint32_t)(s[i - 1] >> 32));
}

__global__ __launch_bounds__(VOX_THREADS) void vox_head_count_kernel(const uint64_t* __restrict__ a,
                                                                     const uint64_t* __restrict__ b, int cap,
                                                                     const int32_t* __restrict__ n_live,
                                                                     const int* __restrict__ params, int* __restrict__ cnt) {
  __shared__ int ws[VOX_WAVES];
  const int n = live_of(n_live, cap);
  const uint64_t* s = params[P_SEL + VOX_PASSES] ? b : a;
  const int t0 = blockIdx.x * VOX_TILE;
  int c = 0;
#pragma unroll
  for (int k = 0; k < VOX_ITEMS; ++k) c += is_head(s, t0 + k * VOX_THREADS + threadIdx.x, n) ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < VOX_WAVES; ++w) t += ws[w];
    cnt[blockIdx.x] = t;
  }
}

// exclusive scan of up to 1024 tile counts, the total -> out_count
__global__ __launch_bounds__(1024) void vox_head_scan_kernel(int* __restrict__ cnt, int nb, int32_t* __restrict__ out_count) {
  __shared__ int ws[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = (int)threadIdx.x < nb ? cnt[threadIdx.x] : 0;
  int inc = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int w = __shfl_up(inc, o); if (lane >= o) inc += w; }
  if (lane == 63) ws[wave] = inc;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += ws[w];
  if ((int)threadIdx.x < nb) cnt[threadIdx.x] = base + inc - c;
  if (threadIdx.x == 1023) *out_count = base + inc;
}

__global__ __launch_bounds__(VOX_THREADS) void vox_head_write_kernel(const uint64_t* __restrict__ a,
                                                                     const uint64_t* __restrict__ b, int cap,
                                                                     const int32_t* __restrict__ n_live,
                                                                     const int* __restrict__ params,
                                                                     const int* __restrict__ cnt,
                                                                     const int32_t* __restrict__ out_count,
                                                                     int64_t* __restrict__ out_idx) {
  __shared__ int ws[VOX_WAVES];
  const int n = live_of(n_live, cap);
  const uint64_t* s = params[P_SEL + VOX_PASSES] ? b : a;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int w0 = blockIdx.x * VOX_TILE + wave * VOX_WAVE_SPAN;
  const int m = *out_count;
  uint64_t heads[VOX_ITEMS];
  int total = 0;
#pragma unroll
  for (int r = 0; r < VOX_ITEMS; ++r) {
    heads[r] = __ballot(is_head(s, w0 + r * 64 + lane, n));
    total += __popcll(heads[r]);
  }
  if (lane == 0) ws[wave] = total;
  __syncthreads();
  int pos = cnt[blockIdx.x];
  for (int w = 0; w < wave; ++w) pos += ws[w];
#pragma unroll
  for (int r = 0; r < VOX_ITEMS; ++r) {
    const int i = w0 + r * 64 + lane;
    if ((heads[r] >> lane) & 1ull) {
      const int at = pos + __popcll(heads[r] & ((1ull << lane) - 1));
      if (at < cap) out_idx[at] = (int64_t)(s[i] & ((1ull << VOX_INDEX_BITS) - 1));
    }
    pos += __popcll(heads[r]);
    if (i < cap && i >= m) out_idx[i] = -1;
  }
}

__global__ __launch_bounds__(256) void vox_rows_kernel(const float* __restrict__ sc, const int64_t* __restrict__ si,
                                                       const float4* __restrict__ sa, const int64_t* __restrict__ idx,
                                                       const int32_t* __restrict__ count, int cap, float* __restrict__ dc,
                                                       int64_t* __restrict__ di, float4* __restrict__ da,
                                                       int32_t* __restrict__ live_rows) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  int m = *count;
  m = m < 0 ? 0 : (m > cap ? cap : m);
  if (i == 0) *live_rows = m;
  if (i >= cap) return;
  float x = 0.0f, y = 0.0f, z = 0.0f;
  int64_t id = 0;
  float4 aux = make_float4(0.0f, 0.0f, 0.0f, 0.0f);       // the neutral row: no loss, no gradient
  if (i < m) {
    const int64_t j = idx[i];
    if (j >= 0 && j < cap) { x = sc[j * 3]; y = sc[j * 3 + 1]; z = sc[j * 3 + 2]; id = si[j]; aux = sa[j]; }
  }
  dc[(int64_t)i * 3] = x; dc[(int64_t)i * 3 + 1] = y; dc[(int64_t)i * 3 + 2] = z;
  di[i] = id;
  da[i] = aux;
}

inline int64_t a256(int64_t v) { return (v + 255) / 256 * 256; }
inline int vox_blocks(int64_t cap) { return (int)((cap + VOX_TILE - 1) / VOX_TILE); }

}  // namespace

int64_t voxel_down_workspace_bytes(int64_t cap) {
  return 2 * a256(cap * 8) + a256((int64_t)vox_blocks(cap) * 256 * 4) + a256(VOX_RED_BLOCKS * 8 * 4) + a256(P_WORDS * 4);
}

hipError_t launch_voxel_down_sample(const float* pts, int64_t ld, int64_t capacity, const int32_t* n_live, float v, void* ws,
                                    int64_t* out_idx, int32_t* out_count, hipStream_t s) {
  const int cap = (int)capacity, nb = vox_blocks(capacity);
  char* w = reinterpret_cast<char*>(ws);
  uint64_t* a = reinterpret_cast<uint64_t*>(w);   w += a256(capacity * 8);
  uint64_t* b = reinterpret_cast<uint64_t*>(w);   w += a256(capacity * 8);
  int* hist = reinterpret_cast<int*>(w);          w += a256((int64_t)nb * 256 * 4);
  float* partial = reinterpret_cast<float*>(w);   w += a256(VOX_RED_BLOCKS * 8 * 4);
  int* params = reinterpret_cast<int*>(w);
  const unsigned g256 = (unsigned)((capacity + 255) / 256);
  vox_bounds_kernel<<<VOX_RED_BLOCKS, 256, 0, s>>>(pts, ld, cap, n_live, v, partial);
  vox_finish_kernel<<<1, VOX_RED_BLOCKS, 0, s>>>(partial, cap, n_live, v, params);
  vox_keys_kernel<<<g256, 256, 0, s>>>(pts, ld, cap, n_live, v, params, a);
  for (int p = 0; p < VOX_PASSES; ++p) {
    vox_hist_kernel<<<nb, VOX_THREADS, 0, s>>>(a, b, cap, n_live, p, params, hist);
    vox_scan_kernel<<<1, 1024, 0, s>>>(hist, nb, cap, n_live, p, params);
    vox_scatter_kernel<<<nb, VOX_THREADS, 0, s>>>(a, b, cap, n_live, p, params, hist);
  }
  vox_head_count_kernel<<<nb, VOX_THREADS, 0, s>>>(a, b, cap, n_live, params, hist);
  vox_head_scan_kernel<<<1, 1024, 0, s>>>(hist, nb, out_count);
  vox_head_write_kernel<<<nb, VOX_THREADS, 0, s>>>(a, b, cap, n_live, params, hist, out_count, out_idx);
  return hipGetLastError();
}

hipError_t launch_voxel_select_rows(const float* sc, const int64_t* si, const float* sa, const int64_t* idx,
                                    const int32_t* count, int64_t capacity, float* dc, int64_t* di, float* da,
                                    int32_t* live_rows, hipStream_t s) {
  const unsigned g = (unsigned)((capacity + 255) / 256);
  vox_rows_kernel<<<g < 1 ? 1 : g, 256, 0, s>>>(sc, si, reinterpret_cast<const float4*>(sa), idx, count, (int)capacity, dc, di,
                                                reinterpret_cast<float4*>(da), live_rows);
  return hipGetLastError();
}

}  // namespace miso

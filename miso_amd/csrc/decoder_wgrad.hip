// Decoder weight gradients for a trainable MLPNet on the fused path, for gfx950.
//
// The frozen-decoder kernels (sdf_fused.hip) give the forward, the ReLU sign bits, d sdf / d x and the grid gradients.
// What a trainable decoder needs on top is, for every nn.Linear l,
//   dW_l[out][in] = sum_p delta_l[p][out] a_{l-1}[p][in],   db_l[out] = sum_p delta_l[p][out]
// with a_{-1} the encoded feature row, a_l the ReLU outputs and delta_l the cotangent that reaches layer l's output, gated
// by the sign bits THE FORWARD WROTE (so this pass and sdf_bwd_kernel gate alike, whichever arithmetic the forward ran in).
//
// One wavefront owns a 64-point chunk, as in sdf_fused.hip.  It gathers the features (gather_level), recomputes the
// activations with the exact fp32 chains (v_mfma_f32_32x32x2_f32, accumulators of a layer = B operand of the next) and runs
// the cotangent back through the transposed weights the same way.  In those chains a lane holds a POINT and its registers
// hold ROWS; the products above contract over points, so both operands are transposed through a per-wave LDS tile, one
// layer and one 32-point tile at a time: written as [point][row] (16-B stores straight from the accumulator layout), read
// back as A(l) = delta[2s + (l>>5)][32r + (l&31)], B(l) = a[2s + (l>>5)][32r' + (l&31)] -- 32 consecutive dwords per lane
// group, conflict-free.  The bias gradient is the sum of the A operands a lane reads (lane <-> row).
//
// Determinism: no atomics.  A wavefront keeps dW / db in accumulators over its whole grid-stride loop; the four waves of a
// workgroup are summed in wave order through LDS (the weights are dead by then), one partial block per workgroup goes to
// the workspace, and wgrad_reduce_kernel adds the blocks in a fixed order.  The launch geometry depends on (shape, n) only.
#include "sdf_fused.hpp"

namespace miso {

// one partial block (and the order wgrad_reduce_kernel reads it in): every dW_l as nn.Linear.weight has it, (out, in)
// row-major with the true F columns, then every db_l
struct WgradLayout {
  int F, H, NH;
  int o_w[MISO_MAX_LINEAR], o_b[MISO_MAX_LINEAR], total;
  __host__ __device__ WgradLayout(int F_, int H_, int NH_) {
    F = F_; H = H_; NH = NH_;
    int o = 0;      // (fixed trip counts and constant indices: the arrays stay in registers)
#pragma unroll
    for (int l = 0; l < MISO_MAX_LINEAR; ++l) { o_w[l] = o; o += l <= NH + 1 ? w_size(l) : 0; }
#pragma unroll
    for (int l = 0; l < MISO_MAX_LINEAR; ++l) { o_b[l] = o; o += l <= NH + 1 ? b_size(l) : 0; }
    total = o;
  }
  __host__ __device__ int w_size(int l) const { return l == 0 ? H * F : l == NH + 1 ? H : H * H; }
  __host__ __device__ int b_size(int l) const { return l == NH + 1 ? 1 : H; }
};

// floats of LDS in front of the waves' tiles: the staged weights during the loop; after it the workgroup's partial block,
// with its bias sums behind it in float64
__host__ __device__ inline int wgrad_static_floats(const PackLayout& pl, const WgradLayout& wl) {
  const int a = pl.fwd_end + (pl.o_w0T - pl.o_whT), b = (wl.total + 1) / 2 * 2 + 2 * (wl.total - wl.o_b[0]);
  return ((a > b ? a : b) + 3) / 4 * 4;
}

#ifdef MISO_ABL_WGRAD_BIAS_F32      // dev A/B (less accurate db): what the float64 bias sums of the loop cost -- DESIGN 4.2b
typedef float bias_acc_t;
#else
typedef double bias_acc_t;
#endif

constexpr unsigned WGRAD_MAX_BLOCKS = 256;      // one workgroup per CU: <= 256 partial blocks of <= 6337 floats (6.5 MB)

static inline unsigned wgrad_blocks(int64_t n) {
  const int64_t nchunks = (n + 63) / 64, b = (nchunks + 3) / 4;
  return (unsigned)(b < (int64_t)WGRAD_MAX_BLOCKS ? b : (int64_t)WGRAD_MAX_BLOCKS);
}

// LDS writes of this wavefront -> visible to its other lanes (and reads done before the tile is written again)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// tile t of a value in accumulator layout (lane (hi, c), register j <-> point 32 t + c, row 32 r + row_of(j, hi)) ->
// T[c][row], pitch P: registers 4g .. 4g+3 are the four consecutive rows 32 r + 8 g + 4 hi ..
template <int RT, int P>
__device__ __forceinline__ void stage_tile(float* __restrict__ T, const f32x16 (&v)[RT][2], int t, int lane) {
  const int hi = lane >> 5, c = lane & 31;
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<float4*>(T + c * P + 32 * r + 8 * q + 4 * hi) =
          make_float4(v[r][t][4 * q], v[r][t][4 * q + 1], v[r][t][4 * q + 2], v[r][t][4 * q + 3]);
}

template <int C, int L, int H, int NH>
__global__ __launch_bounds__(256) void decoder_wgrad_kernel(GridK g, const float* __restrict__ packed,
                                                            const float* __restrict__ x, int64_t n,
                                                            const float* __restrict__ gsdf,
                                                            const uint32_t* __restrict__ mask,
                                                            const int* __restrict__ perm, int gsdf_sorted,
                                                            float* __restrict__ partial) {
  // perm != nullptr: x and mask are in the binned order, gsdf in the caller's unless gsdf_sorted
  constexpr int F = C * L, RT = H / 32, KS0 = (F + 1) / 2, KS1 = H / 2;
  constexpr int MW = (NH + 1) * RT;
  constexpr int P = H + 4, FP = F + 4;      // tile pitches: 16-B aligned rows, b128 stores of 8 lanes cover 32 banks
  constexpr int TA = (32 * P > 64 * FP) ? 32 * P : 64 * FP, TD = 32 * P;
  constexpr int NHA = NH > 0 ? NH : 1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const PackLayout pl(F, H, NH);
  const WgradLayout wl(F, H, NH);
  // LDS: the fp32 forward pack [0, fwd_end), then the transposed hidden weights [o_whT, o_w0T), then the waves' tiles
  const int n_fwd = pl.fwd_end, n_T = pl.o_w0T - pl.o_whT;
  for (int i = threadIdx.x * 4; i < n_fwd; i += blockDim.x * 4)
    *reinterpret_cast<float4*>(smem + i) = *reinterpret_cast<const float4*>(packed + i);
  for (int i = threadIdx.x * 4; i < n_T; i += blockDim.x * 4)
    *reinterpret_cast<float4*>(smem + n_fwd + i) = *reinterpret_cast<const float4*>(packed + pl.o_whT + i);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hi = lane >> 5, c = lane & 31;
  const float* w0p = smem + pl.o_w0;
  const float* whp = smem + pl.o_wh;
  const float* b0 = smem + pl.o_b0;
  const float* bh = smem + pl.o_bh;
  const float* wo = smem + pl.o_wo;
  const float* whT = smem + n_fwd;
  float* ta = smem + wgrad_static_floats(pl, wl) + wave * (TA + TD);      // a_{l-1} (or the feature rows [64][FP])
  float* td = ta + TA;                                            // delta_l
  const int64_t nchunks = (n + 63) / 64;

  // the wavefront's sums: dW_0 (columns >= F unused), dW_h, dW_out as lane-partial sums over this lane's points, db.
  // The bias sums are plain sums of up to n terms: carried in float64 down to the partial block, they are rounded once
  // per workgroup (a library reduction sums fp32 as a tree; an fp32 chain per lane lost three times as much).
  f32x16 aW0[RT], aWh[NHA][RT][RT], aWo[RT];
  bias_acc_t ab[NH + 1][RT], abo = 0;
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    aW0[r] = zero_block(); aWo[r] = zero_block();
#pragma unroll
    for (int l = 0; l <= NH; ++l) ab[l][r] = 0;
#pragma unroll
    for (int h = 0; h < NHA; ++h)
#pragma unroll
      for (int rp = 0; rp < RT; ++rp) aWh[h][r][rp] = zero_block();
  }

  ChunkSched sched(nchunks, wave, 4, perm != nullptr);
  for (int64_t chunk = sched.cur; chunk < sched.end; chunk += sched.step) {
    asm volatile("" ::: "memory");  // see sdf_fwd_kernel
    const int64_t p = chunk * 64 + lane;
    const bool valid = p < n;
    const int64_t pt[2] = {chunk * 64 + c, chunk * 64 + 32 + c};
    float ds[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
      ds[t] = (pt[t] < n) ? gsdf[(perm && !gsdf_sorted) ? (int64_t)perm[pt[t]] : pt[t]] : 0.0f;
    uint32_t mw[MW];
    {
      const uint32_t* mi = mask + (chunk * 64 + lane) * MW;
#pragma unroll
      for (int i = 0; i < MW; ++i) mw[i] = mi[i];
    }
    // ---- encode: lane = point, as sdf_fwd_kernel (ignored levels and points outside the grid give zeros) ----------------
    float f[2 * KS0];
#pragma unroll
    for (int i = 0; i < 2 * KS0; ++i) f[i] = 0.0f;
    if (valid) {
      float px, py, pz;
      load_point(g, x, p, px, py, pz);
#pragma unroll
      for (int l = 0; l < L; ++l) {
        const LevelK& lv = g.lv[l];
        if ((g.ignore_mask >> l) & 1u) continue;
        Axis ax = axis_coord(px, g.bmin[0], g.bmax[0], lv.X, g.flags);
        Axis ay = axis_coord(py, g.bmin[1], g.bmax[1], lv.Y, g.flags);
        Axis az = axis_coord(pz, g.bmin[2], g.bmax[2], lv.Z, g.flags);
        Cell cell = make_cell(ax, ay, az, lv);
        gather_level<C>(lv, cell, &f[l * C]);
      }
    }
    // ---- activations, exact fp32 chains (decoder_fwd_exact, every layer kept) --------------------------------------------
    f32x16 act[NH + 1][RT][2];
    {
      f32x16 bias[RT];
#pragma unroll
      for (int r = 0; r < RT; ++r) bias[r] = bias_block(b0, r, hi);
#pragma unroll
      for (int s = 0; s < KS0; ++s) {
        auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(f[2 * s]), __float_as_uint(f[2 * s + 1]), false, false);
        const float bt0 = __uint_as_float(sw[0]), bt1 = __uint_as_float(sw[1]);
#pragma unroll
        for (int r = 0; r < RT; ++r) {
          const float a = w0p[(s * 64 + lane) * RT + r];
          act[0][r][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bt0, s == 0 ? bias[r] : act[0][r][0], 0, 0, 0);
          act[0][r][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bt1, s == 0 ? bias[r] : act[0][r][1], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int h = 0; h <= NH; ++h) {
      if (h > 0) {
        f32x16 bias[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r) bias[r] = bias_block(bh + (h - 1) * H, r, hi);
#pragma unroll
        for (int rp = 0; rp < RT; ++rp)
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const int ks = rp * 16 + j;
#pragma unroll
            for (int r = 0; r < RT; ++r) {
              const float a = whp[(((h - 1) * KS1 + ks) * 64 + lane) * RT + r];
              act[h][r][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, act[h - 1][rp][0][j], ks == 0 ? bias[r] : act[h][r][0], 0, 0, 0);
              act[h][r][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, act[h - 1][rp][1][j], ks == 0 ? bias[r] : act[h][r][1], 0, 0, 0);
            }
          }
      }
#pragma unroll
      for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int j = 0; j < 16; ++j) act[h][r][t][j] = relu1(act[h][r][t][j]);
    }
    // ---- output layer: dW_out[m] += a_NH[p][m] d sdf[p] (this lane's two points), db_out += d sdf ------------------------
    abo += (bias_acc_t)ds[0] + (bias_acc_t)ds[1];
    f32x16 d[RT][2];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        aWo[r][j] = __builtin_fmaf(act[NH][r][0][j], ds[0], aWo[r][j]);
        aWo[r][j] = __builtin_fmaf(act[NH][r][1][j], ds[1], aWo[r][j]);
        const float wv = wo[32 * r + row_of(j, hi)];
#pragma unroll
        for (int t = 0; t < 2; ++t) d[r][t][j] = gate(wv * ds[t], mw[NH * RT + r], t, j);
      }
    // ---- hidden layers, last to first: d = delta_{h+1}; dW_{h+1} += d^T a_h; then delta_h = gate(Wh[h]^T d) -------------
#pragma unroll
    for (int hh = 0; hh < NH; ++hh) {
      const int h = NH - 1 - hh;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        stage_tile<RT, P>(td, d, t, lane);
        stage_tile<RT, P>(ta, act[h], t, lane);
        wave_sync();
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          float av[RT], bv[RT];
#pragma unroll
          for (int r = 0; r < RT; ++r) {
            av[r] = td[(2 * s + hi) * P + 32 * r + c];
            bv[r] = ta[(2 * s + hi) * P + 32 * r + c];
            ab[h + 1][r] += (bias_acc_t)av[r];
          }
#pragma unroll
          for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int rp = 0; rp < RT; ++rp)
              aWh[h][r][rp] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[r], bv[rp], aWh[h][r][rp], 0, 0, 0);
        }
        wave_sync();
      }
      f32x16 dn[RT][2];
#pragma unroll
      for (int r = 0; r < RT; ++r) { dn[r][0] = zero_block(); dn[r][1] = zero_block(); }
#pragma unroll
      for (int rp = 0; rp < RT; ++rp)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int ks = rp * 16 + j;
#pragma unroll
          for (int r = 0; r < RT; ++r) {
            const float a = whT[((h * KS1 + ks) * 64 + lane) * RT + r];
            dn[r][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, d[rp][0][j], dn[r][0], 0, 0, 0);
            dn[r][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, d[rp][1][j], dn[r][1], 0, 0, 0);
          }
        }
#pragma unroll
      for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int j = 0; j < 16; ++j) d[r][t][j] = gate(dn[r][t][j], mw[h * RT + r], t, j);
    }
    // ---- first layer: dW_0 += delta_0^T feats (feature rows staged lane = point; columns >= F read as zero) --------------
#pragma unroll
    for (int q = 0; q < F; q += 4)
      *reinterpret_cast<float4*>(ta + lane * FP + q) = make_float4(f[q], f[q + 1], f[q + 2], f[q + 3]);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      stage_tile<RT, P>(td, d, t, lane);
      wave_sync();
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const float fv = ta[(32 * t + 2 * s + hi) * FP + (c < F ? c : 0)];
        const float bv = c < F ? fv : 0.0f;
#pragma unroll
        for (int r = 0; r < RT; ++r) {
          const float av = td[(2 * s + hi) * P + 32 * r + c];
          ab[0][r] += (bias_acc_t)av;
          aW0[r] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, aW0[r], 0, 0, 0);
        }
      }
      wave_sync();
    }
  }

  // ---- the workgroup's partial block: waves added in wave order through LDS, then stored -------------------------------
  // lane-partial sums first: dW_out over the 32 lanes of a half (fixed butterfly), db over the two halves
#pragma unroll
  for (int r = 0; r < RT; ++r) {
#pragma unroll
    for (int j = 0; j < 16; ++j)
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) aWo[r][j] += __shfl_xor(aWo[r][j], o);
#pragma unroll
    for (int l = 0; l <= NH; ++l) ab[l][r] += __shfl_xor(ab[l][r], 32);
  }
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) abo += __shfl_xor(abo, o);      // both halves hold the same points: one half's sum
  float* S = smem;
  double* SB = reinterpret_cast<double*>(smem + (wl.total + 1) / 2 * 2);      // the bias sums, [o_b[0], total)
  for (int w = 0; w < 4; ++w) {
    __syncthreads();
    if (wave != w) continue;
    const bool first = w == 0;
    auto put = [&](int idx, float v) { S[idx] = first ? v : S[idx] + v; };
    auto put_b = [&](int idx, double v) { SB[idx - wl.o_b[0]] = first ? v : SB[idx - wl.o_b[0]] + v; };
#pragma unroll
    for (int r = 0; r < RT; ++r) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int row = 32 * r + row_of(j, hi);
        if (c < F) put(wl.o_w[0] + row * F + c, aW0[r][j]);
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
          for (int rp = 0; rp < RT; ++rp) put(wl.o_w[1 + h] + row * H + 32 * rp + c, aWh[h][r][rp][j]);
        if (c == 0) put(wl.o_w[NH + 1] + row, aWo[r][j]);
      }
      if (hi == 0) {
#pragma unroll
        for (int l = 0; l <= NH; ++l) put_b(wl.o_b[l] + 32 * r + c, ab[l][r]);
      }
    }
    if (lane == 0) put_b(wl.o_b[NH + 1], abo);
  }
  __syncthreads();
  float* dst = partial + (int64_t)blockIdx.x * wl.total;
  for (int i = threadIdx.x; i < wl.total; i += blockDim.x) dst[i] = i < wl.o_b[0] ? S[i] : (float)SB[i - wl.o_b[0]];
}

// out = sum of the partial blocks, block 0 first: four interleaved sums (b mod 4) combined in a fixed order, carried in
// float64 (up to 256 terms of one sign pattern per element -- db above all: an fp32 chain of 64 costs ~1e-6 of the sum,
// several times what a tree-shaped library reduction loses; the adds are free here).  n_parts == 0 (an empty batch)
// writes zeros.
__global__ void wgrad_reduce_kernel(const float* __restrict__ partial, int n_parts, int F, int H, int NH, WgradOutK out) {
  const WgradLayout wl(F, H, NH);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= wl.total) return;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  int b = 0;
  for (; b + 4 <= n_parts; b += 4) {
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] += (double)partial[(int64_t)(b + q) * wl.total + i];
  }
  for (int q = 0; b + q < n_parts; ++q) s[q] += (double)partial[(int64_t)(b + q) * wl.total + i];
  const float v = (float)((s[0] + s[1]) + (s[2] + s[3]));
#pragma unroll
  for (int l = 0; l < MISO_MAX_LINEAR; ++l) {
    if (l > NH + 1) break;
    if (i >= wl.o_w[l] && i < wl.o_w[l] + wl.w_size(l)) { if (out.w[l]) out.w[l][i - wl.o_w[l]] = v; }
    if (i >= wl.o_b[l] && i < wl.o_b[l] + wl.b_size(l)) { if (out.b[l]) out.b[l][i - wl.o_b[l]] = v; }
  }
}

template <int C, int L, int H, int NH>
static hipError_t launch_wgrad_t(FusedShape<C, L, H, NH>, const GridK& g, const float* packed, const float* x, int64_t n,
                                 const float* gsdf, const uint32_t* mask, const int* perm, bool gsdf_sorted,
                                 float* partial, hipStream_t s) {
  constexpr int F = C * L, P = H + 4, FP = F + 4;
  constexpr int TA = (32 * P > 64 * FP) ? 32 * P : 64 * FP, TD = 32 * P;
  const PackLayout pl(F, H, NH);
  const WgradLayout wl(F, H, NH);
  const size_t lds = (size_t)(wgrad_static_floats(pl, wl) + 4 * (TA + TD)) * sizeof(float);
  auto k = decoder_wgrad_kernel<C, L, H, NH>;
  hipError_t e = allow_lds((const void*)k, lds);
  if (e != hipSuccess) return e;
  k<<<wgrad_blocks(n), 256, lds, s>>>(g, packed, x, n, gsdf, mask, perm, gsdf_sorted ? 1 : 0, partial);
  return hipGetLastError();
}

int64_t sdf_wgrad_workspace_floats(int C, int L, int H, int NH, int64_t n) {
  if (!fused_shape_supported(C, L, H, NH) || n <= 0) return 0;
  return (int64_t)wgrad_blocks(n) * WgradLayout(C * L, H, NH).total;
}

hipError_t launch_sdf_wgrad(int C, int L, int H, int NH, const GridK& g, const float* packed, const float* x, int64_t n,
                            const float* gsdf, const uint32_t* mask, const int* perm, bool gsdf_sorted,
                            const WgradOutK& out, float* workspace, hipStream_t s) {
  if (n > 0) {
    hipError_t e = with_fused_shape(C, L, H, NH, hipErrorInvalidValue, [&](auto shape) {
      return launch_wgrad_t(shape, g, packed, x, n, gsdf, mask, perm, gsdf_sorted, workspace, s);
    });
    if (e != hipSuccess) return e;
  }
  const WgradLayout wl(C * L, H, NH);
  wgrad_reduce_kernel<<<(wl.total + 255) / 256, 256, 0, s>>>(workspace, n > 0 ? (int)wgrad_blocks(n) : 0, C * L, H, NH, out);
  return hipGetLastError();
}

}  // namespace miso

// The field of an atlas at one world point per lane -- "world point -> masked mean over the submaps -> decoder" -- shared
// by the two kernels that evaluate it: atlas_sdf_kernel (atlas.hip: one evaluation per point) and atlas_trace_kernel
// (trace.hip: one per ray per sphere-tracing step).  Both go through atlas_eval below, so a traced ray sees the bits
// miso_atlas_sdf_fwd returns at the same point.
#pragma once
#include "sdf_fused.hpp"

namespace miso {

// Decoder weights in LDS (the bf16x3 split image, or the fp32 pack behind MISO_F_EXACT_F32) and the decoder chain of
// sdf_fwd_kernel on one feature row per lane.  decode() holds matrix instructions and a cross-lane exchange: every lane
// of the wavefront must call it (full EXEC).  The gather and the output dot product are asked for with their
// multiply-adds fused outright (mul_acc in decoder.hpp): this code is inlined into two kernels at several places, and
// every copy has to give the bits of sdf_fwd_kernel, where the compiler fuses them all.
template <int C, int L, int H, int NH, bool SPLIT>
struct AtlasDecoder {
  static constexpr int F = C * L, RT = H / 32, KS0 = (F + 1) / 2, NF = 2 * KS0, MW = (NH + 1) * RT;
  const float* smem;
  const uint32_t* s_fwd;
  const float* s_bias;
  PackLayout pl;
  int lane, hi;
  float bo = 0.0f;
  float sdf_empty = 0.0f;      // the decoder's answer to an all-zero feature row (a point inside no submap)

  // stage: all threads of the block; ends in a barrier (a feature-only query stages nothing)
  __device__ __forceinline__ AtlasDecoder(float* smem_, const float* __restrict__ packed, bool want_sdf)
      : smem(smem_), pl(F, H, NH) {
    const int n_split = pl.s_fwd_end - pl.s_w0;
    if (want_sdf) {
      if (SPLIT) {
        for (int i = threadIdx.x * 4; i < n_split; i += blockDim.x * 4)
          *reinterpret_cast<float4*>(smem_ + i) = *reinterpret_cast<const float4*>(packed + pl.s_w0 + i);
        for (int i = threadIdx.x * 4; i < pl.n_bias(); i += blockDim.x * 4)
          *reinterpret_cast<float4*>(smem_ + n_split + i) = *reinterpret_cast<const float4*>(packed + pl.o_b0 + i);
      } else {
        for (int i = threadIdx.x * 4; i < pl.fwd_end; i += blockDim.x * 4)
          *reinterpret_cast<float4*>(smem_ + i) = *reinterpret_cast<const float4*>(packed + i);
      }
    }
    __syncthreads();
    lane = threadIdx.x & 63;
    hi = lane >> 5;
    s_fwd = reinterpret_cast<const uint32_t*>(smem_);
    s_bias = smem_ + n_split;
    if (want_sdf) {
      bo = SPLIT ? s_bias[pl.o_bo - pl.o_b0] : smem_[pl.o_bo];
      float z[NF];
#pragma unroll
      for (int i = 0; i < NF; ++i) z[i] = 0.0f;
      sdf_empty = decode(z);      // once per wavefront
    }
  }

  __device__ __forceinline__ float decode(const float (&f)[NF]) const {
    uint32_t mw[MW];
    float p0 = 0.0f, p1 = 0.0f, poison = 0.0f;
    if constexpr (SPLIT) {
      u32x4 no_mask[H / 16][2];
      decoder_fwd_split<F, H, NH, false, false, false, true>(s_fwd, s_bias, lane, f, mw, no_mask, p0, p1, poison);
    } else {
      decoder_fwd_exact<F, H, NH, true>(smem + pl.o_w0, smem + pl.o_wh, smem + pl.o_b0, smem + pl.o_bh, smem + pl.o_wo, lane, f,
                                  mw, p0, p1);
    }
    p0 += __shfl_xor(p0, 32);
    p1 += __shfl_xor(p1, 32);
    return SPLIT ? ((hi ? p1 : p0) + bo) + poison : (hi ? p1 : p0) + bo;
  }
};

// One evaluation for the wavefront: lane's world point (wx, wy, wz); `valid` lanes take part in the gathers, the others
// only in the decoder (their value is to be ignored).  Per submap (poses and bounds are wave-uniform) the frame change
// and the bound test; a submap that no lane is inside costs one ballot; inside lanes encode.  mean[] receives the mean
// feature row (zeros past F); the return value is the decoded SDF when want_sdf (the zero-row shortcut when no lane is
// inside any submap: wave-uniform), else 0.  Call with full EXEC.
template <int C, int L, int H, int NH, bool SPLIT>
__device__ __forceinline__ float atlas_eval(const AtlasK& a, const AtlasDecoder<C, L, H, NH, SPLIT>& dec, bool valid,
                                            float wx, float wy, float wz, bool want_sdf,
                                            float (&mean)[AtlasDecoder<C, L, H, NH, SPLIT>::NF]) {
  constexpr int F = C * L, NF = AtlasDecoder<C, L, H, NH, SPLIT>::NF;
  float sum[NF];
#pragma unroll
  for (int i = 0; i < NF; ++i) sum[i] = 0.0f;
  float cnt = 0.0f;
  bool any_inside = false;
  for (int s = 0; s < a.n_submaps; ++s) {
    const float* ps = a.poses + s * 12;
    const GridK& g = a.submaps[s];
    // transfrom_points_from (utils_geometry.py:227-240) = transform_points_to with (R^T, -R^T t), both formed by the
    // caller with the reference's own tensor ops; the row-times-matrix product in torch's order: ((x r0) + y r1) + z r2, + t
    float xl[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      float v = __fmul_rn(wx, ps[3 * j]);
      v = __fmaf_rn(wy, ps[3 * j + 1], v);
      v = __fmaf_rn(wz, ps[3 * j + 2], v);
      xl[j] = __fadd_rn(v, ps[9 + j]);
    }
    // coords_in_bound (utils_geometry.py:11-27): min <= x <= max on every axis
    const bool inside = valid && (a.no_bound || (xl[0] >= g.bmin[0] && xl[0] <= g.bmax[0] && xl[1] >= g.bmin[1] &&
                                                 xl[1] <= g.bmax[1] && xl[2] >= g.bmin[2] && xl[2] <= g.bmax[2]));
    if (!__any(inside)) continue;
    any_inside = true;
    if (inside) {
      cnt += 1.0f;
#pragma unroll
      for (int l = 0; l < L; ++l) {
        if ((g.ignore_mask >> l) & 1u) continue;      // (zeros: utils.py:160-163; the atlas queries never set it)
        const LevelK lv = g.lv[l];
        Axis ax[3];
        const Cell c = level_cell(g, lv, xl[0], xl[1], xl[2], ax);
        float fl[C];
        gather_level<C, true>(lv, c, fl);
#pragma unroll
        for (int q = 0; q < C; ++q) sum[l * C + q] += fl[q];      // sum_feats += mask * feats, submap by submap
      }
    }
  }
  // sum_weights[sum_weights == 0] = 1; mean = sum / weights
  const float den = cnt == 0.0f ? 1.0f : cnt;
#pragma unroll
  for (int i = 0; i < NF; ++i) mean[i] = (i < F) ? __fdiv_rn(sum[i], den) : 0.0f;
  if (!want_sdf) return 0.0f;
  return any_inside ? dec.decode(mean) : dec.sdf_empty;      // (wave-uniform choice)
}

// The lane's world point in submap s's frame (xl) and whether it counts as inside that submap (`ps`: the submap's row
// of the pose table, `g`: its grid; both wave-uniform).  The operations of atlas_eval's loop, in its order: the
// backward (atlas_bwd.hip) has to find the same lanes inside the same submaps.
__device__ __forceinline__ bool atlas_to_submap(const AtlasK& a, const float* ps, const GridK& g, bool valid, float wx,
                                                float wy, float wz, float (&xl)[3]) {
  // transfrom_points_from (utils_geometry.py:227-240) = transform_points_to with (R^T, -R^T t), both formed by the
  // caller with the reference's own tensor ops; the row-times-matrix product in torch's order: ((x r0) + y r1) + z r2, + t
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float v = __fmul_rn(wx, ps[3 * j]);
    v = __fmaf_rn(wy, ps[3 * j + 1], v);
    v = __fmaf_rn(wz, ps[3 * j + 2], v);
    xl[j] = __fadd_rn(v, ps[9 + j]);
  }
  // coords_in_bound (utils_geometry.py:11-27): min <= x <= max on every axis
  return valid && (a.no_bound || (xl[0] >= g.bmin[0] && xl[0] <= g.bmax[0] && xl[1] >= g.bmin[1] &&
                                  xl[1] <= g.bmax[1] && xl[2] >= g.bmin[2] && xl[2] <= g.bmax[2]));
}

// The first half of atlas_eval for a caller that runs the decoder itself (atlas_sdf_bwd_kernel keeps the ReLU signs):
// the masked mean over the submaps at one world point per lane, operation for operation the loop of atlas_eval above.
// A second copy on purpose.  atlas_eval = atlas_mean + decode was built and measured: atlas_sdf_kernel<8,3,32,1,exact>
// went 128 -> 130 VGPRs and ten atlas_trace_kernel instantiations took 1 - 4 more; apart, every kernel keeps its counts.
// mean[] receives the mean feature row (zeros past F), den the number of submaps the lane is inside (1 where it is
// inside none: the divisor of the mean); returns whether any lane of the wavefront is inside any submap (wave-uniform).
template <int C, int L, int NF>
__device__ __forceinline__ bool atlas_mean(const AtlasK& a, bool valid, float wx, float wy, float wz, float (&mean)[NF],
                                           float& den) {
  constexpr int F = C * L;
  float sum[NF];
#pragma unroll
  for (int i = 0; i < NF; ++i) sum[i] = 0.0f;
  float cnt = 0.0f;
  bool any_inside = false;
  for (int s = 0; s < a.n_submaps; ++s) {
    const GridK& g = a.submaps[s];
    float xl[3];
    const bool inside = atlas_to_submap(a, a.poses + s * 12, g, valid, wx, wy, wz, xl);
    if (!__any(inside)) continue;
    any_inside = true;
    if (inside) {
      cnt += 1.0f;
#pragma unroll
      for (int l = 0; l < L; ++l) {
        if ((g.ignore_mask >> l) & 1u) continue;      // (zeros: utils.py:160-163; the atlas queries never set it)
        const LevelK lv = g.lv[l];
        Axis ax[3];
        const Cell c = level_cell(g, lv, xl[0], xl[1], xl[2], ax);
        float fl[C];
        gather_level<C, true>(lv, c, fl);
#pragma unroll
        for (int q = 0; q < C; ++q) sum[l * C + q] += fl[q];      // sum_feats += mask * feats, submap by submap
      }
    }
  }
  // sum_weights[sum_weights == 0] = 1; mean = sum / weights
  den = cnt == 0.0f ? 1.0f : cnt;
#pragma unroll
  for (int i = 0; i < NF; ++i) mean[i] = (i < F) ? __fdiv_rn(sum[i], den) : 0.0f;
  return any_inside;
}

// Launch shape of the kernels that run atlas_eval: dynamic LDS for the decoder image (split or fp32 pack; `staged` =
// false for a feature-only query, which stages nothing) and a persistent grid of four wavefronts per block, one per 64
// points at a time.
struct AtlasLaunch {
  size_t lds;
  unsigned blocks;
  AtlasLaunch(int F, int H, int NH, bool split, bool staged, int64_t n) {
    PackLayout pl(F, H, NH);
    lds = (size_t)(split ? pl.s_fwd_end - pl.s_w0 + (pl.n_bias() + 3) / 4 * 4 : (pl.fwd_end + 3) / 4 * 4) * sizeof(float);
    if (!staged) lds = 16;
    const int64_t nchunks = (n + 63) / 64;
    blocks = (unsigned)((nchunks + 3) / 4);
    if (blocks > 2048u) blocks = 2048u;
  }
};

}  // namespace miso

// The field of an atlas at one world point per lane -- "world point -> masked mean over the submaps -> decoder" -- shared
// by the two kernels that evaluate it: atlas_sdf_kernel (atlas.hip: one evaluation per point) and atlas_trace_kernel
// (trace.hip: one per ray per sphere-tracing step).  Both go through atlas_eval below, so a traced ray sees the bits
// miso_atlas_sdf_fwd returns at the same point.
#pragma once
#include "sdf_fused.hpp"

namespace miso {

// FwdDecoder (decoder.hpp) for an atlas: sdf_fwd_kernel's chain with the multiply-adds of the output dot product fused
// outright (the gather asks for the same: gather_level<C, true>) -- this code is inlined into several kernels at several
// places, and every copy has to give the bits of sdf_fwd_kernel, where the compiler fuses them all -- and the decoder's
// answer to an all-zero feature row.
template <int C, int L, int H, int NH, bool SPLIT>
struct AtlasDecoder : FwdDecoder<C * L, H, NH, SPLIT, true> {
  using Base = FwdDecoder<C * L, H, NH, SPLIT, true>;
  using Base::NF;
  float sdf_empty = 0.0f;      // a point inside no submap

  // stage: all threads of the block; ends in a barrier (want_sdf = false: a feature-only query stages nothing)
  __device__ __forceinline__ AtlasDecoder(const float* __restrict__ packed, bool want_sdf) : Base(packed, want_sdf) {
    if (want_sdf) {
      float z[NF];
#pragma unroll
      for (int i = 0; i < NF; ++i) z[i] = 0.0f;
      sdf_empty = decode(z);      // once per wavefront
    }
  }

  __device__ __forceinline__ float decode(const float (&f)[NF]) const {
    uint32_t mw[Base::MW];
    return Base::template decode<false>(f, mw);
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

}  // namespace miso

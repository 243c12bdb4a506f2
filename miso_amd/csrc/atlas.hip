// GridAtlas.query_feature / GridAtlas.forward in ONE launch (round 6).
//
// Reference (grid_opt/models/grid_atlas.py:374-399): for every active submap s -- world points into the submap frame
// (utils_geometry.transfrom_points_from), coords_in_bound mask, a full multi-level grid_interp_regular of EVERY point
// (masked-out ones too), mask * feats added to an (N,F) running sum, the mask to an (N,1) count -- then count == 0 -> 1,
// sum / count, and submap 0's decoder on the mean (utils.grid_decode).  Every demo's final global mesh runs it at
// resolution 512 (134 M points x S submaps: demo/align_submaps.py:99, full_slam_scannet.py:116).
//
// Here: one wavefront per 64 points, lane = point.  Per submap (poses and bounds are wave-uniform: scalar registers) the
// frame change and the bound test; a submap that no point of the wavefront is inside costs nothing more (one ballot), and
// inside ones are encoded for the lanes that are inside only.  Sum, count and mean stay in registers, the mean feeds the
// decoder chain of sdf_fwd_kernel (decoder.hpp: bf16x3 split products, or the exact fp32 chains behind MISO_F_EXACT_F32)
// without touching HBM.  Lattice queries (utils_sdf.extract_fields: the points ARE a linspace^3 meshgrid) generate their
// coordinates from the point index and three short axis tables: no (N,3) tensor is ever formed.
// A chunk with no point inside any submap (the empty corners of a scene's bounding box) decodes the all-zero feature row:
// that value is computed once per wavefront and stored.
#include "atlas_eval.hpp"

namespace miso {

template <int C, int L, int H, int NH, bool SPLIT>
__global__ __launch_bounds__(256, 2) void atlas_sdf_kernel(AtlasK a, const float* __restrict__ packed) {
  using Dec = AtlasDecoder<C, L, H, NH, SPLIT>;
  constexpr int F = C * L;
  const Dec dec(packed, a.sdf != nullptr);      // weights to LDS, the zero row's value (atlas_eval.hpp)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  const int64_t nchunks = (a.n + 63) / 64;
  const uint32_t nyz = (uint32_t)a.dim[1] * (uint32_t)a.dim[2];
  for (int64_t chunk = (int64_t)blockIdx.x * 4 + wave; chunk < nchunks; chunk += (int64_t)gridDim.x * 4) {
    asm volatile("" ::: "memory");      // (keeps the LDS reads of weights / biases inside the loop: sdf_fwd_kernel)
    const int64_t p = chunk * 64 + lane;
    const bool valid = p < a.n;
    float wx = 0.f, wy = 0.f, wz = 0.f;
    if (valid) {
      if (a.x) {
        wx = a.x[p * 3 + 0]; wy = a.x[p * 3 + 1]; wz = a.x[p * 3 + 2];
      } else {      // (a lattice launch has n < 2^31: checked on the host)
        const uint32_t q = (uint32_t)p, i = q / nyz, r = q - i * nyz, j = r / (uint32_t)a.dim[2], k = r - j * (uint32_t)a.dim[2];
        wx = a.ax[0][i]; wy = a.ax[1][j]; wz = a.ax[2][k];
      }
    }
    float mean[Dec::NF];
    const float v = atlas_eval(a, dec, valid, wx, wy, wz, a.sdf != nullptr, mean);
    if (a.feats && valid) {
      float* dst = a.feats + p * a.ld;
#pragma unroll
      for (int i = 0; i < F; ++i) dst[i] = mean[i];
    }
    if (a.sdf && valid) a.sdf[p] = v;
  }
}

template <int C, int L, int H, int NH>
static hipError_t launch_atlas_t(FusedShape<C, L, H, NH>, const AtlasK& a, const float* packed, bool split, hipStream_t s) {
  const FwdLaunch dims(C * L, H, NH, split, a.n, 2048u, a.sdf != nullptr);
  auto k = split ? atlas_sdf_kernel<C, L, H, NH, true> : atlas_sdf_kernel<C, L, H, NH, false>;
  hipError_t e = allow_dynamic_lds((const void*)k, dims.lds);
  if (e != hipSuccess) return e;
  k<<<dims.blocks, 256, dims.lds, s>>>(a, packed);
  return hipGetLastError();
}

hipError_t launch_atlas_sdf(int C, int L, int H, int NH, const AtlasK& a, const float* packed, bool exact, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  const bool split = use_split(exact);
  return with_fused_shape(C, L, H, NH, hipErrorInvalidValue,
                          [&](auto shape) { return launch_atlas_t(shape, a, packed, split, s); });
}

}  // namespace miso

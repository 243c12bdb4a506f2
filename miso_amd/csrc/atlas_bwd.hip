// Backward of the fused atlas query (atlas.hip: world point -> masked mean over the submaps -> decoder) in ONE launch:
// d sdf -> d world point, d (submap pose table), d (every submap's level features).
//
// Reference (grid_opt/models/grid_atlas.py:374-399 under autograd): per submap the backward of mask * grid_interp_regular
// over ALL points and an (N,F) cotangent through HBM, the backward of the division by the count, op by op.  Here: one
// wavefront per 64 world points (lane = point), per chunk
//   1. the forward again (atlas_mean, atlas_eval.hpp: same frame change, bound test, sum, count and mean) and the
//      decoder forward with its ReLU signs kept -- nothing is saved between the two launches but the SDF itself;
//   2. the decoder backward (decoder.hpp): d sdf -> d mean in accumulator layout -> the wavefront's LDS tile
//      (dfeat_tile.hpp) -> one row per lane, divided by the lane's count: that row is d feats of EVERY submap the
//      point is inside (the count is a constant, and the bound mask is not differentiated: autograd sees
//      inside * interp with a boolean mask);
//   3. per submap that some lane is inside (poses and bounds are wave-uniform):
//        grid   the row-major float-atomic scatter (scatter_tile) into the submap's level gradients (levels whose
//               gradient pointer is NULL -- a locked submap -- are skipped);
//        x      d x_local by the corner loop (lane = point), d x_world += R_sw^T d x_local;
//        pose   the table row is x_local = R_sw x_world + t_sw: dR_sw[j][k] += d x_local[j] x_world[k],
//               dt_sw[j] += d x_local[j] -- summed over the wavefront, then added into the block's (S,12) LDS partial.
// Every block stores its partial into its own slot of the workspace and atlas_pose_reduce_kernel sums the slots in
// fp64: no global atomics on the 12 S addresses that every wavefront of the launch would otherwise hit.
// A wavefront with no lane inside any submap (the forward's sdf_empty shortcut) leaves the loop before the decoder:
// wave-uniform, and its points get a zero gradient.
#include "atlas_eval.hpp"

namespace miso {

struct AtlasBwdK {
  const float* gsdf;      // (N) d loss / d sdf
  float* gx;              // (N,3) d loss / d x_world (written), or nullptr
  float* pose_slots;      // workspace (gridDim.x, S, 12), or nullptr: no pose gradient
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <int C, int L, int H, int NH, bool SPLIT>
__global__ __launch_bounds__(512) void atlas_sdf_bwd_kernel(AtlasK a, AtlasBwdK b, const float* __restrict__ packed) {
  constexpr int F = C * L, RT = H / 32, KS0 = (F + 1) / 2, NF = 2 * KS0, MW = (NH + 1) * RT;
  constexpr int FP = dfeat_pitch(F), REC = CELL_REC;      // the d-feat tile and the cell records: dfeat_tile.hpp
  constexpr int WAVE_LDS = 64 * FP + 64 * L * REC;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const PackImage<SPLIT, true> img(F, H, NH);      // the whole pack (decoder.hpp)
  img.stage(packed);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hi = lane >> 5;
  const int nw = blockDim.x >> 6;
  float* s_pose = img.behind() + nw * WAVE_LDS;      // the block's (S,12) pose partial
  if (b.pose_slots)
    for (int i = threadIdx.x; i < a.n_submaps * 12; i += blockDim.x) s_pose[i] = 0.0f;
  __syncthreads();
  float* dF = img.behind() + wave * WAVE_LDS;                       // this wavefront's d-feat tile [64][FP]
  int* rec = reinterpret_cast<int*>(dF + 64 * FP);                  // ... and cell records [64][L][REC]
  const bool want_x = b.gx != nullptr || b.pose_slots != nullptr;

  const int64_t nchunks = (a.n + 63) / 64;
  for (int64_t chunk = (int64_t)blockIdx.x * nw + wave; chunk < nchunks; chunk += (int64_t)gridDim.x * nw) {
    asm volatile("" ::: "memory");      // (keeps the LDS reads of weights / biases inside the loop: sdf_fwd_kernel)
    const int64_t p = chunk * 64 + lane;
    const bool valid = p < a.n;
    float wx = 0.f, wy = 0.f, wz = 0.f;
    if (valid) { wx = a.x[p * 3 + 0]; wy = a.x[p * 3 + 1]; wz = a.x[p * 3 + 2]; }
    // ================================ forward again ================================================================
    float mean[NF], den;
    const bool any_inside = atlas_mean<C, L>(a, valid, wx, wy, wz, mean, den);
    if (!any_inside) {      // (wave-uniform) the forward answered sdf_empty, a constant
      if (b.gx && valid) { b.gx[p * 3 + 0] = 0.f; b.gx[p * 3 + 1] = 0.f; b.gx[p * 3 + 2] = 0.f; }
      continue;
    }
    uint32_t mw[MW];
    u32x4 maskB[H / 16][2];      // SPLIT: the last ReLU's mask as the first backward product's B operand
    {
      float p0 = 0.0f, p1 = 0.0f, poison = 0.0f;
      if constexpr (SPLIT) decoder_fwd_split<F, H, NH, false, false, true, true>(img.s_fwd(), img.s_bias(), lane, mean, mw, maskB, p0, p1, poison);
      else decoder_fwd_exact<F, H, NH, true>(img.w0p(), img.whp(), img.b0(), img.bh(), img.wo(), lane, mean, mw, p0, p1);
    }
    // ================================ decoder backward ==============================================================
    // two tiles of 32 points, lane (hi, c) on point 32 t + c of tile t
    const float gl = valid ? b.gsdf[p] : 0.0f;
    float ds[2];
    ds[0] = __shfl(gl, lane & 31);
    ds[1] = __shfl(gl, 32 + (lane & 31));
    f32x16 df[2];
    if constexpr (SPLIT) decoder_bwd_split<F, H, NH, false>(img.s_bwd(), lane, maskB, mw, ds, df);
    else decoder_bwd_exact<F, H, NH>(img.whT(), img.w0T(), img.wo(), lane, mw, ds, df);
    // ---- accumulator layout -> LDS tile -> one row per lane; d feats_s = d mean / count ------------------------------
    dfeat_to_tile<F, 2>(df, dF, lane & 31, hi);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float dfe[F];
#pragma unroll
    for (int i = 0; i < F; i += 4) {
      const float4 v = *reinterpret_cast<const float4*>(dF + lane * FP + i);
      dfe[i] = __fdiv_rn(v.x, den); dfe[i + 1] = __fdiv_rn(v.y, den);
      dfe[i + 2] = __fdiv_rn(v.z, den); dfe[i + 3] = __fdiv_rn(v.w, den);
      *reinterpret_cast<float4*>(dF + lane * FP + i) = make_float4(dfe[i], dfe[i + 1], dfe[i + 2], dfe[i + 3]);
    }
    // ================================ per submap =====================================================================
    float gxw[3] = {0.f, 0.f, 0.f};
    for (int s = 0; s < a.n_submaps; ++s) {
      const float* ps = a.poses + s * 12;
      const GridK& g = a.submaps[s];
      float xl[3];
      const bool inside = atlas_to_submap(a, ps, g, valid, wx, wy, wz, xl);
      if (!__any(inside)) continue;
      uint32_t scatter_mask = 0;
#pragma unroll
      for (int l = 0; l < L; ++l)
        if (g.lv[l].grad && !((g.ignore_mask >> l) & 1u)) scatter_mask |= 1u << l;
      if (!scatter_mask && !want_x) continue;
      float dxl[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int l = 0; l < L; ++l) {
        if ((g.ignore_mask >> l) & 1u) continue;
        const LevelK lv = g.lv[l];
        Axis ax = axis_coord(xl[0], g.bmin[0], g.bmax[0], lv.X, g.flags);
        Axis ay = axis_coord(xl[1], g.bmin[1], g.bmax[1], lv.Y, g.flags);
        Axis az = axis_coord(xl[2], g.bmin[2], g.bmax[2], lv.Z, g.flags);
        Cell c = make_cell(ax, ay, az, lv);
        if ((scatter_mask >> l) & 1u) write_cell_record(rec + (lane * L + l) * REC, c, lv, inside);
        if (want_x && inside) {      // d x_local of this level: the corner loop of sdf_bwd_kernel, lane = point
          float sx_ = 0.f, sy_ = 0.f, sz_ = 0.f;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
            if (!(c.inx[dx] && c.iny[dy] && c.inz[dz])) continue;
            const int off = (c.k0 + dz) * lv.sZ + (c.j0 + dy) * lv.sY + (c.i0 + dx) * lv.sX;
            float dot = 0.f;
#pragma unroll
            for (int q = 0; q < C; q += 4) {
              const float4 gv = *reinterpret_cast<const float4*>(lv.data + off + q);
              dot += gv.x * dfe[l * C + q] + gv.y * dfe[l * C + q + 1] + gv.z * dfe[l * C + q + 2] + gv.w * dfe[l * C + q + 3];
            }
            const float sx = dx ? 1.f : -1.f, sy = dy ? 1.f : -1.f, sz = dz ? 1.f : -1.f;
            sx_ += dot * sx * c.wy[dy] * c.wz[dz];
            sy_ += dot * sy * c.wx[dx] * c.wz[dz];
            sz_ += dot * sz * c.wx[dx] * c.wy[dy];
          }
          dxl[0] += sx_ * (g.gscale[0] * ax.mult);
          dxl[1] += sy_ * (g.gscale[1] * ay.mult);
          dxl[2] += sz_ * (g.gscale[2] * az.mult);
        }
      }
      if (want_x) {
        // x_local = R_sw x_world + t_sw (row j of the table row: ps[3j .. 3j+2], ps[9 + j])
#pragma unroll
        for (int k = 0; k < 3; ++k) gxw[k] += (ps[k] * dxl[0] + ps[3 + k] * dxl[1]) + ps[6 + k] * dxl[2];
        if (b.pose_slots) {
          // dxl is zero outside the submap, but 0 x inf and 0 x NaN are not: a lane that is not inside (a NaN or inf
          // world coordinate is inside nothing) takes part with a zero point
          const float xw[3] = {inside ? wx : 0.f, inside ? wy : 0.f, inside ? wz : 0.f};
          float mine = 0.0f;      // lane i < 12 keeps element i of the wavefront's sum
#pragma unroll
          for (int i = 0; i < 12; ++i) {
            const float v = wave_sum(i < 9 ? dxl[i / 3] * xw[i % 3] : dxl[i - 9]);
            if (lane == i) mine = v;
          }
          if (lane < 12) __hip_atomic_fetch_add(s_pose + s * 12 + lane, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
      if (scatter_mask) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        scatter_tile<C, L, false, const GridK&>(g, scatter_mask, dF, rec, 64, lane);      // (no touched flags: the atlas keeps none)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();      // the next submap overwrites the records
      }
    }
    if (b.gx && valid) { b.gx[p * 3 + 0] = gxw[0]; b.gx[p * 3 + 1] = gxw[1]; b.gx[p * 3 + 2] = gxw[2]; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();          // the next chunk overwrites the tile
  }
  if (b.pose_slots) {
    __syncthreads();
    float* slot = b.pose_slots + (int64_t)blockIdx.x * a.n_submaps * 12;
    for (int i = threadIdx.x; i < a.n_submaps * 12; i += blockDim.x) slot[i] = s_pose[i];
  }
}

// the blocks' (S,12) partials -> the (S,12) pose-table gradient, summed in fp64 in slot order
__global__ void atlas_pose_reduce_kernel(const float* __restrict__ slots, int n_slots, int count, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  double acc = 0.0;
  for (int s = 0; s < n_slots; ++s) acc += (double)slots[(int64_t)s * count + i];
  out[i] = (float)acc;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// the most blocks a launch over n points has (four wavefronts per block, two blocks per CU): what the workspace is sized for
static unsigned atlas_bwd_max_blocks(int64_t n) {
  const int64_t nchunks = (n + 63) / 64, blocks = (nchunks + 3) / 4;
  return (unsigned)(blocks < 512 ? blocks : 512);
}

int64_t atlas_bwd_workspace_bytes(int64_t n, int n_submaps) {
  if (n <= 0 || n_submaps < 1) return 0;
  return (int64_t)atlas_bwd_max_blocks(n) * n_submaps * 12 * (int64_t)sizeof(float);
}

// The launch shape of atlas_sdf_bwd_kernel, planned in one place: two wavefronts per SIMD either way -- ONE workgroup of
// eight per CU where eight tiles fit beside the pack (one copy of the pack out of L2 per CU, as sdf_train_kernel's plan),
// else workgroups of four, two per CU where two fit.  lds == 0: not even four wavefronts fit (the block's (S,12) pose
// partial sits in LDS beside the decoder images and the tiles).
struct AtlasBwdPlan {
  int wavefronts;
  size_t lds;
};
static AtlasBwdPlan plan_atlas_bwd(int C, int L, int H, int NH, bool split, int n_submaps, bool poses) {
  const PackLayout pl(C * L, H, NH);
  const int F = C * L, wave_lds = 64 * dfeat_pitch(F) + 64 * L * CELL_REC;
  const int pack = image_floats(pl, split, true);
  const int pose = poses ? (n_submaps * 12 + 3) / 4 * 4 : 0;
  const auto bytes = [&](int wavefronts) { return (size_t)(pack + wavefronts * wave_lds + pose) * sizeof(float); };
  const int nw = bytes(8) <= MISO_LDS_LIMIT ? 8 : 4;
  return {nw, bytes(nw) <= MISO_LDS_LIMIT ? bytes(nw) : 0};
}

// can miso_atlas_sdf_bwd serve this decoder shape over n_submaps submaps (with a pose gradient), in both arithmetic forms?
bool atlas_bwd_covered(int C, int L, int H, int NH, int n_submaps, bool poses) {
  if (!fused_shape_supported(C, L, H, NH) || n_submaps < 1 || (poses && n_submaps > MISO_ATLAS_BWD_MAX_SUBMAPS)) return false;
  return plan_atlas_bwd(C, L, H, NH, true, n_submaps, poses).lds && plan_atlas_bwd(C, L, H, NH, false, n_submaps, poses).lds;
}

template <int C, int L, int H, int NH>
static hipError_t launch_atlas_bwd_t(FusedShape<C, L, H, NH>, const AtlasK& a, const float* packed, const float* gsdf,
                                     float* gx, float* gposes, float* workspace, bool split, hipStream_t s) {
  const AtlasBwdPlan plan = plan_atlas_bwd(C, L, H, NH, split, a.n_submaps, gposes != nullptr);
  if (!plan.lds) return hipErrorInvalidValue;      // (miso_atlas_sdf_bwd has asked atlas_bwd_covered)
  const int nw = plan.wavefronts;
  const size_t lds = plan.lds;
  const int64_t nchunks = (a.n + 63) / 64;
  const unsigned cap = nw == 8 ? 256u : (2 * lds <= MISO_LDS_LIMIT ? 512u : 256u);
  unsigned blocks = (unsigned)((nchunks + nw - 1) / nw);
  if (blocks > cap) blocks = cap;      // (<= atlas_bwd_max_blocks(n))
  AtlasBwdK b = {gsdf, gx, gposes ? workspace : nullptr};
  auto k = split ? atlas_sdf_bwd_kernel<C, L, H, NH, true> : atlas_sdf_bwd_kernel<C, L, H, NH, false>;
  hipError_t e = allow_dynamic_lds((const void*)k, lds);
  if (e != hipSuccess) return e;
  k<<<blocks, 64 * nw, lds, s>>>(a, b, packed);
  e = hipGetLastError();
  if (e != hipSuccess || !gposes) return e;
  const int count = a.n_submaps * 12;
  atlas_pose_reduce_kernel<<<(count + 255) / 256, 256, 0, s>>>(workspace, (int)blocks, count, gposes);
  return hipGetLastError();
}

hipError_t launch_atlas_sdf_bwd(int C, int L, int H, int NH, const AtlasK& a, const float* packed, const float* gsdf,
                                float* gx, float* gposes, float* workspace, bool exact, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  const bool split = use_split(exact);
  return with_fused_shape(C, L, H, NH, hipErrorInvalidValue, [&](auto shape) {
    return launch_atlas_bwd_t(shape, a, packed, gsdf, gx, gposes, workspace, split, s);
  });
}

}  // namespace miso

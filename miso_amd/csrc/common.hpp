// Shared device helpers for libmiso_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <unordered_map>

#include "../../include/miso_hip.h"

namespace miso {

// Kernel-side view of one level (no grad/data split: the launcher picks).
struct LevelK {
  const float* data;
  float* grad;
  const float* gg;  // cotangent-of-grad grid (second order), or nullptr
  unsigned char* touched;  // miso_level_t.grad_touched: one byte per MISO_ADAM_CHUNK floats of `grad`, or nullptr
  int32_t C, Z, Y, X;
  int32_t sC, sZ, sY, sX;  // element strides, validated < 2^31 on the host
  int32_t foff;            // first output column of this level
};

// elements from a level's first to its last, + 1 (miso_level_t or LevelK)
template <class Level>
inline int64_t level_span(const Level& s) {
  return (int64_t)(s.C - 1) * s.sC + (int64_t)(s.X - 1) * s.sX + (int64_t)(s.Y - 1) * s.sY + (int64_t)(s.Z - 1) * s.sZ + 1;
}

// internal GridK::flags bit (not part of the ABI): the batch is binned, there is no perm[] and the original index of
// sorted point p is the integer in xn[p].w (miso_sort_points with perm == NULL; sdf_train_kernel)
constexpr uint32_t MISO_F_INDEX_IN_XN = 1u << 20;

// sdf_train_kernel<SCAT> may have a second block of cell records in LDS and request the next chunk's gathers in front
// of this chunk's atomics (its rotate_records argument, set by its launcher when the shape leaves room)
constexpr int MISO_ROTATE_MAX_F = 12;        // ... for feature rows up to 12 floats (wider rows: the rotated loop spills)
constexpr size_t MISO_LDS_LIMIT = 160 * 1024;      // LDS of a CDNA4 compute unit = the most one workgroup can have

struct GridK {
  int32_t n_levels;
  uint32_t ignore_mask;
  uint32_t flags;
  int32_t F;
  float bmin[3], bmax[3];
  // sorted batches hand the kernels pre-normalised float4 points (sort.hip): xstride = 4,
  // flags carry COORDS_NORMALIZED and gscale = 2/len restores d xn / d x for the pose gradient
  float gscale[3];
  int32_t xstride;
  uint32_t tune;   // always 0 (convert_grid): read by sdf_bwd_kernel alone, whose dev branches stay as they were
  LevelK lv[MISO_MAX_LEVELS];
};

// One fused atlas query (atlas.hip; miso_atlas_sdf_fwd)
struct AtlasK {
  const GridK* submaps;      // device, n_submaps entries (miso_atlas_plan_build)
  const float* poses;        // device, n_submaps x 12: R_submap_world row-major (9), t_submap_world (3)
  int32_t n_submaps;
  const float* x;            // (N,3) world points, or nullptr: lattice
  const float* ax[3];        // lattice axes (device): point p = (i ny + j) nz + k sits at (ax[0][i], ax[1][j], ax[2][k])
  int32_t dim[3];
  int64_t n;
  float* sdf;                // (N) or nullptr
  float* feats;              // (N, ld) mean features or nullptr
  int64_t ld;
  int32_t no_bound;          // MISO_F_ATLAS_NO_BOUND: no coords_in_bound test (one submap queried as GridNet.forward does)
};

// One sphere-tracing launch (trace.hip; miso_atlas_sphere_trace): the rays, the reference's loop constants, the outputs.
// The field is the AtlasK that goes with it (x, sdf, feats unused; n = n_rays).
struct TraceK {
  const float* origins;      // (N,3)
  const float* dirs;         // (N,3), unit length (the caller normalises)
  int64_t n;
  float min_dist, max_dist, epsilon;
  float fd_step;             // central-difference step of grad
  int32_t max_iters;
  float* points;             // (N,3)
  uint8_t* hit;              // (N): s < epsilon in the ray's last iteration
  float* sdf;                // (N) field value at points, or nullptr
  int32_t* steps;            // (N) iterations in which the ray moved, or nullptr
  float* grad;               // (N,3) central differences at points, or nullptr
};

// miso_sorted_t.tiles_per_axis: a plain count (1..16: cubic binning) or MISO_TILES_XYZ(tx, ty, tz), 1..32 per axis
inline bool tiles_xyz(int32_t code, int T[3]) {
  if (code >= 1 && code <= 16) { T[0] = T[1] = T[2] = code; return true; }
  if (code < 256 || (code >> 24) != 0) return false;
  T[0] = code & 255; T[1] = (code >> 8) & 255; T[2] = (code >> 16) & 255;
  for (int a = 0; a < 3; ++a)
    if (T[a] < 1 || T[a] > 32) return false;
  return true;
}
inline bool tiles_cubic16(int32_t code) { return code >= 1 && code <= 16; }

struct MlpK {
  const float* w[MISO_MAX_LINEAR];
  const float* b[MISO_MAX_LINEAR];
};
// where the decoder's weight gradients go (decoder_wgrad.hip): nn.Linear layout, nullptr = not wanted / no bias
struct WgradOutK {
  float* w[MISO_MAX_LINEAR];
  float* b[MISO_MAX_LINEAR];
};

__device__ __forceinline__ void atomic_add_f32(float* p, float v) {
  // hardware fp32 add at L2 (global_atomic_add_f32, no return value)
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One Levenberg-Marquardt step of the tracker on the device (lm.hip)
struct LmTrackK {
  const float* x;            // (N,3) samples in the keyframe frame
  const float* gt;           // (N) measured SDF, element stride s_gt
  const void* valid;         // (N) validity (float or bool), stride s_valid, or nullptr
  const int64_t* frame_ids;  // (N), stride s_fid, or nullptr
  int64_t s_gt, s_valid, s_fid;
  int valid_is_bool;
  int64_t n, kf;
  float trunc;
  const float* Rwk;          // 9: base rotation of the keyframe
  const float* twk;          // 3
  float* dr;                 // 3: rotation correction (axis-angle), updated by the solve
  float* dt;                 // 3
  float* pose;               // scratch 12: R (row-major), t
  float* xw;                 // scratch (N,3): samples in the submap frame
  float* sums;               // scratch 36: 32 of lm_normal_eq + {rows kept, in bound, wrong frame id, invalid}
  float* info;               // out 8: |dR| (rad), |dt|, |g|, in bound, kept, wrong frame id, invalid, 0
  float* clean;              // nullptr, or scratch 5N: torch.nan_to_num of x (3N), gt (N), valid (N, as floats) -- written
                             // by the transform kernel, read by everything after it (the caller repoints x / gt / valid)
  float bmin[3], bmax[3];
  float lm_lambda;
};

// miso_level_t.grad_touched: a non-zero went into grad[off] (element offset from lv.grad)
constexpr int ADAM_CHUNK_SHIFT = 6;
static_assert(MISO_ADAM_CHUNK == (1 << ADAM_CHUNK_SHIFT), "touch_chunk shifts by log2 of the chunk");
__device__ __forceinline__ void touch_chunk(const LevelK& lv, int64_t off) {
  if (lv.touched) lv.touched[off >> ADAM_CHUNK_SHIFT] = 1;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device, size): the call is ~5 us of host time, and a
// training step that issues its six launches on the stream makes it three times (the host's lead over the device is
// what protects such a step against a busy host).  The attribute only ever grows.
inline hipError_t allow_dynamic_lds(const void* kernel, size_t bytes) {
  if (bytes <= 48 * 1024) return hipSuccess;
  static std::mutex mu;
  static std::unordered_map<uint64_t, size_t> granted;      // (kernel address ^ device) -> bytes
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const uint64_t key = (uint64_t)(uintptr_t)kernel ^ ((uint64_t)(dev + 1) << 56);
  {
    std::lock_guard<std::mutex> lock(mu);
    auto it = granted.find(key);
    if (it != granted.end() && it->second >= bytes) return hipSuccess;
  }
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(mu);
  size_t& g = granted[key];
  if (g < bytes) g = bytes;
  return hipSuccess;
}

// One (src, dst) pair of a fused alignment iteration, as the batched kernels of pair_latent.hip read it from the
// device-resident plan (built on the host by miso_align_plan_build from miso_align_pair_t).
struct AlignPairK {
  GridK g;              // destination levels 0..level (data only) and bound
  const float* p;       // (n,3) source vertices in the source frame
  const float* fsrc;    // (n, ld) source features
  int64_t ld, n;
  const float* gate_p;  // (gate_n,3) finest-level source vertices for the overlap gate, or nullptr: always on
  int64_t gate_n;
  // the same vertices as a lattice (preferred: nothing to read but three short tables): vertex (i,j,k), index
  // (k ny + j) nx + i, sits at (gate_ax[0][i], gate_ax[1][j], gate_ax[2][k]); gate_n = nx ny nz
  const float* gate_ax[3];
  int32_t gate_dim[3];
  int32_t src, dst;
  float n_ch;           // channels compared (the L2 mean divides by count * n_ch)
  // axis-aligned boxes {min xyz, max xyz} (source frame) of every run of ALIGN_BOX_VERTS consecutive source vertices, or
  // nullptr: a run that cannot reach the destination bound under the current poses is not read
  const float* boxes;
};
constexpr int ALIGN_BOX_VERTS = 64;

// One torch.optim.Adam update (amsgrad=False, weight_decay=0) as torch forms it op by op; shared by adam.hip
// (dense grids) and align.hip (the 6(S-1) pose numbers of the alignment loop).
struct AdamScalars {
  float one_minus_b1, b2, one_minus_b2, neg_step_size, bc2_sqrt, eps;
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamScalars& a) {
#pragma clang fp contract(off)   // one rounding per torch op, and the same bits from every kernel that inlines this
  // exp_avg.lerp_(grad, 1 - beta1).  torch's lerp has two forms, chosen by the weight: with the first alone a
  // beta1 <= 0.5 loses a gradient below an ulp of m (beta1 = 0, m = 1, g = 1e-20: 0 where torch keeps g)
  const float w = a.one_minus_b1, d = g - m;
  m = w < 0.5f ? m + w * d : g - d * (1.0f - w);
  v = v * a.b2 + (a.one_minus_b2 * g) * g;          // mul_(beta2).addcmul_(grad, grad, 1 - beta2)
  float denom = sqrtf(v) / a.bc2_sqrt + a.eps;      // (sqrt / bias_correction2_sqrt).add_(eps)
  p = p + (a.neg_step_size * m) / denom;            // addcdiv_(exp_avg, denom, value=-step_size)
}

// One Adam iteration of the tracker's pose refinement on the device (lm.hip: miso_track_adam_step)
struct TrackAdamK {
  LmTrackK s;
  int loss_type;             // 1 L1, 2 L2, 3 GM
  float weight_sdf, gm_scale;
  float* gpred;              // scratch (N): d loss / d sdf
  const float* gx;           // (N,3): d loss / d x_world, from the fused coordinate backward
  const float* sdf;          // (N)
  const AdamScalars* table;  // step scalars of steps 1..table_len (miso_adam_scalars_table)
  int table_len;
  float* state;              // 12 floats m[6] v[6], then int32 {steps taken, skipped, iterations}
  float* ring;               // loss of iteration i at ring[i], i < ring_len
  int ring_len;
};

// Pointwise mapping loss (grid_opt/loss.py:594-635, :668-700) shared by loss.hip and the fused
// backward.  g / gf: d(w_sdf * sdf term) / ds and d(w_fs * free-space term) / ds BEFORE the 1/N of
// the mean; s_sdf / s_fs accumulate the unweighted term sums.
struct MapLossK {
  int loss_type;  // 1 = L1, 2 = L2
  float w_sdf, w_fs, trunc;
};

__device__ __forceinline__ void map_loss_one(const MapLossK& p, float s, float t, float w, bool v, bool fs,
                                             float& g, float& gf, float& s_sdf, float& s_fs) {
  g = 0.f; gf = 0.f;
  const float d = s - t;
  if (v) {
    if (p.loss_type == 1) {
      s_sdf += w * fabsf(d);
      g = p.w_sdf * w * ((d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f));
    } else {
      s_sdf += w * d * d;
      g = p.w_sdf * w * 2.f * d;
    }
  }
  if (fs) {
    const float up = fmaxf(d, 0.f), lo = fmaxf(p.trunc - s, 0.f);
    s_fs += fmaxf(up, lo);
    // d/ds max(relu(s-t), relu(trunc-s)); ties carry zero slope on both sides
    if (up > lo) gf = p.w_fs;
    else if (lo > up) gf = -p.w_fs;
  }
}

// The mapping loss folded into the fused forward (sdf_fwd_kernel): with loss_type != 0 the kernel
// forms d loss / d sdf for every point right after its SDF and writes it in the binned order.
struct LossInK {
  MapLossK p;          // p.loss_type 0 = not fused
  const float4* aux;   // (N) {target, valid, sign, weight} per point, caller order
  float* gsdf_sorted;  // (N) out: d loss / d sdf, binned order
  float* loss_out;     // (MISO_LOSS_SLOTS, 2): every slot written by the launch
  float inv_n;
  const int32_t* n_live;   // device count of live rows (the rest is neutral padding), or nullptr: the means divide by it
};

}  // namespace miso

#include "trilinear.hpp"      // the sampler (load_point, Axis, Cell, level_cell, corner table, lerp tree): needs the structs above

// utils_sdf.sphere_tracing over hash-indexed levels in ONE launch (include/miso_hash_trace.h): hash_trace_kernel is the ray
// loop of atlas_trace_kernel (trace.hip) with f = "hash gather, then decoder" -- hash_gather_row (hash_grid.hpp), the
// gather of hash_sdf_fwd_kernel, in front of AtlasDecoder::decode (atlas_eval.hpp), the decoder chain that
// atlas_trace_kernel already runs inside a ray loop with sdf_fwd_kernel's bits.  A ray therefore sees at every point the
// bits miso_hash_sdf_fwd gives there, in both decoder arithmetics, poison term included.
//
// The semantics are the reference loop's as trace.hip states them: p = o + min_dist d (add_product: a rounding each for
// the product and the sum), then per round dist = norm3(p - o), s = f(p), conv = s < epsilon, far = dist > max_dist; a
// ray where either holds is frozen, any other moves by p += s d.  One wavefront per 64 rays, lane = ray, the ray's state
// in registers, persistent workgroups of four wavefronts, the decoder's weights staged in LDS once per workgroup.  The loop
// is wave-uniform (it ends when no lane is live); frozen and out-of-range lanes are predicated out of the table loads and
// the update but run the decoder with the others (matrix instructions, a cross-lane exchange: full EXEC).  No lane reads
// another's state.  A NaN field value never stops a ray and leaves its mask false.
//
// Registers of hash_trace_kernel<C, L, H, NH, SPLIT> (gfx950, hipcc -O3, -Rpass-analysis=kernel-resource-usage): VGPRs
// and the wavefronts per SIMD they allow; no AGPRs, scratch 0 and no static LDS in every instantiation (the LDS is
// dynamic: FwdLaunch sizes it; the counts below are this build's, the same as before FwdDecoder).  The field is evaluated at ONE place of the kernel (see the stages in its body): with
// a call per stage every H = 64 shape spilled 180 - 800 bytes per lane.  The two exact L = 4 shapes sit at the cap.
//   shape            split: VGPRs (waves)   exact: VGPRs (waves)
//   <4, 1, 32, 1>     140 (3)                121 (4)
//   <4, 1, 64, 1>     200 (2)                197 (2)
//   <4, 2, 32, 1>     151 (3)                128 (4)
//   <4, 2, 64, 1>     213 (2)                206 (2)
//   <4, 3, 64, 1>     226 (2)                215 (2)
//   <4, 4, 64, 1>     235 (2)                256 (2)
//   <8, 1, 64, 1>     204 (2)                197 (2)
//   <8, 2, 64, 1>     235 (2)                209 (2)
//   <8, 3, 64, 1>     252 (2)                218 (2)
//   <8, 4, 64, 1>     251 (2)                256 (2)
//   <8, 3, 32, 1>     184 (2)                171 (2)
#include <float.h>
#include <string.h>

#include "checks.hpp"
#include "hash_grid.hpp"
#include "atlas_eval.hpp"      // AtlasDecoder
#include "trace_math.hpp"      // add_product, norm3
#include "../../include/miso_hash_trace.h"

namespace miso {

// One evaluation for the wavefront: `take` lanes gather their feature row at (px, py, pz), the others decode a zero row
// (their value is to be ignored).  Call with full EXEC.
template <int C, int L, int H, int NH, bool SPLIT>
__device__ __forceinline__ float hash_eval(const HashGridK& g, const AtlasDecoder<C, L, H, NH, SPLIT>& dec, bool take,
                                           float px, float py, float pz) {
  constexpr int NF = AtlasDecoder<C, L, H, NH, SPLIT>::NF;
  float f[NF];
#pragma unroll
  for (int i = 0; i < NF; ++i) f[i] = 0.0f;
  if (take) hash_gather_row<C, L>(g, px, py, pz, f);
  return dec.decode(f);
}

template <int C, int L, int H, int NH, bool SPLIT>
__global__ __launch_bounds__(256, 2) void hash_trace_kernel(HashGridK g, TraceK t, const float* __restrict__ packed) {
  using Dec = AtlasDecoder<C, L, H, NH, SPLIT>;
  const Dec dec(packed, true);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  const int64_t nchunks = (t.n + 63) / 64;
  for (int64_t chunk = (int64_t)blockIdx.x * 4 + wave; chunk < nchunks; chunk += (int64_t)gridDim.x * 4) {
    asm volatile("" ::: "memory");      // (keeps the LDS reads of weights / biases inside the loop: sdf_fwd_kernel)
    const int64_t r = chunk * 64 + lane;
    const bool valid = r < t.n;
    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
    if (valid) {
      ox = t.origins[r * 3 + 0]; oy = t.origins[r * 3 + 1]; oz = t.origins[r * 3 + 2];
      dx = t.dirs[r * 3 + 0]; dy = t.dirs[r * 3 + 1]; dz = t.dirs[r * 3 + 2];
    }
    // points = origins + min_dist * directions
    float px = add_product(ox, t.min_dist, dx);
    float py = add_product(oy, t.min_dist, dy);
    float pz = add_product(oz, t.min_dist, dz);
    bool live = valid, conv = false;
    float s = 0.0f;      // the field value of the ray's last evaluation; in the last stage f(p + h e_a)
    int moved = 0;
    // The three stages of atlas_trace_kernel -- the rounds, the closing evaluation for t.sdf, the six of the central
    // differences -- around ONE call of hash_eval: with a call in each stage the compiler keeps what the copies share in
    // registers across all of them and every H = 64 shape spills (180 - 800 bytes per lane).  stage, it and k are
    // wave-uniform.
    enum { ROUNDS, CLOSING, DIFFS };
    int stage = ROUNDS, it = 0, k = 0;
    for (;;) {
      if (stage == ROUNDS && (it == t.max_iters || !__any(live))) {
        if (valid) {
          t.points[r * 3 + 0] = px; t.points[r * 3 + 1] = py; t.points[r * 3 + 2] = pz;
          t.hit[r] = conv ? 1 : 0;
          if (t.steps) t.steps[r] = moved;
        }
        stage = CLOSING;
      }
      // f at the returned point: a frozen ray has it; one that still moved at the cut-off does not
      if (stage == CLOSING && !(t.sdf && __any(live))) {
        if (t.sdf && valid) t.sdf[r] = s;
        stage = DIFFS;
      }
      if (stage == DIFFS && (!t.grad || k == 6)) break;
      // diff.gradient3d(method='finitediff'): (f(p + h e_a) - f(p - h e_a)) / (2 h), a = x, y, z
      const int axis = stage == DIFFS ? k >> 1 : 3;
      const float sh = (k & 1) ? -t.fd_step : t.fd_step;
      const float qx = axis == 0 ? __fadd_rn(px, sh) : px;
      const float qy = axis == 1 ? __fadd_rn(py, sh) : py;
      const float qz = axis == 2 ? __fadd_rn(pz, sh) : pz;
      const float v = hash_eval(g, dec, stage == DIFFS ? valid : live, qx, qy, qz);
      if (stage == ROUNDS) {
        if (live) {
          s = v;
          conv = s < t.epsilon;
          const float dist = norm3(__fsub_rn(px, ox), __fsub_rn(py, oy), __fsub_rn(pz, oz));      // (p: this round's still)
          const bool far = dist > t.max_dist;
          if (conv || far) {
            live = false;
          } else {      // points + sdfs * directions
            px = add_product(px, s, dx);
            py = add_product(py, s, dy);
            pz = add_product(pz, s, dz);
            ++moved;
          }
        }
        ++it;
      } else if (stage == CLOSING) {
        if (live) s = v;
        live = false;      // (every ray now has f at its point: the stage ends at its next test)
      } else {
        if (k & 1) {
          if (valid) t.grad[r * 3 + axis] = __fdiv_rn(__fsub_rn(s, v), __fmul_rn(2.0f, t.fd_step));
        } else {
          s = v;
        }
        ++k;
      }
    }
  }
}

template <int C, int L, int H, int NH>
static hipError_t launch_hash_trace_t(FusedShape<C, L, H, NH>, const HashGridK& g, const TraceK& t, const float* packed,
                                      bool split, hipStream_t s) {
  const FwdLaunch dims(C * L, H, NH, split, t.n, 2048u);
  auto k = split ? hash_trace_kernel<C, L, H, NH, true> : hash_trace_kernel<C, L, H, NH, false>;
  hipError_t e = allow_dynamic_lds((const void*)k, dims.lds);
  if (e != hipSuccess) return e;
  k<<<dims.blocks, 256, dims.lds, s>>>(g, t, packed);
  return hipGetLastError();
}

}  // namespace miso

using namespace miso;

extern "C" {

int miso_hash_trace_supported(const miso_hash_grid_t* grid, const miso_mlp_t* mlp) {
  HashSdfCall f;      // every shape of the fused table fits its registers (the table above): miso_hash_sdf_supported's answer
  return hash_sdf_call(&f, grid, mlp, false) == MISO_OK ? 1 : 0;
}

int miso_hash_sphere_trace(const miso_hash_grid_t* grid, const miso_mlp_t* mlp, const float* packed,
                           uint32_t decoder_flags, const float* origins, const float* dirs, int64_t n, float min_dist,
                           float max_dist, int32_t max_iters, float epsilon, float fd_step, float* points, uint8_t* hit,
                           float* sdf_or_null, int32_t* steps_or_null, float* grad_or_null, void* stream) {
  if (int rc = hash_sdf_args(packed, decoder_flags, n)) return rc;
  if (!set_if(n, origins, dirs, points, hit)) return MISO_E_BADARG;
  if (max_iters < 1 || (grad_or_null && !(fd_step > 0.0f && fd_step <= FLT_MAX))) return MISO_E_BADARG;
  HashSdfCall f;
  if (int rc = hash_sdf_call(&f, grid, mlp, true)) return rc;
  if (!blocks_fit(n)) return MISO_E_TOOLARGE;
  if (n == 0) return MISO_OK;
  TraceK t;
  memset(&t, 0, sizeof(t));
  t.origins = origins; t.dirs = dirs; t.n = n;
  t.min_dist = min_dist; t.max_dist = max_dist; t.epsilon = epsilon; t.fd_step = fd_step; t.max_iters = max_iters;
  t.points = points; t.hit = hit; t.sdf = sdf_or_null; t.steps = steps_or_null; t.grad = grad_or_null;
  const bool split = use_split((decoder_flags & MISO_F_EXACT_F32) != 0);
  return (int)with_fused_shape(f.C, f.L, f.H, f.NH, hipErrorInvalidValue, [&](auto shape) {
    return launch_hash_trace_t(shape, f.g, t, packed, split, (hipStream_t)stream);
  });
}

}  // extern "C"

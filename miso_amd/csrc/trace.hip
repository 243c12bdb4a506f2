// utils_sdf.sphere_tracing in ONE launch: depth and normals rendered from the map.
//
// Reference (grid_opt/utils/utils_sdf.py:197-236): p = o + min_dist d, then up to max_iters rounds of
//   dist = |p - o|;  s = f(p);  converged = s < epsilon;  far = dist > max_dist;  p += s d where neither
// over ALL N rays -- per round one model call, an (N,3) round trip through HBM per elementwise op and a host sync
// (torch.sum(mask_stop) == n).  The work is one encode and one decode per live ray per round.
//
// Here: one wavefront per 64 rays, lane = ray, the ray's state in registers; f is atlas_eval (atlas_eval.hpp), the body
// of atlas_sdf_kernel, so a ray sees the bits miso_atlas_sdf_fwd gives at its point.  A ray that has converged or gone
// far is frozen: the reference would re-evaluate it at the same point, get the same s and leave it where it is.  The
// loop is wave-uniform (it ends when no lane is live); frozen lanes are predicated out of the gathers and the update but
// run the decoder with the others (matrix instructions, a cross-lane exchange: full EXEC).  No lane reads another's
// state, so a ray's result does not depend on which rays share its wavefront.
//
// o + min_dist d and p + s d are a product and a sum with a rounding each, as the two torch ops: no FMA (add_product).  The
// comparisons keep the reference's form (s < epsilon, dist > max_dist): a NaN field value never stops a ray and its
// mask stays false, as upstream.
#include "atlas_eval.hpp"
#include "trace_math.hpp"      // add_product, norm3

namespace miso {

template <int C, int L, int H, int NH, bool SPLIT>
__global__ __launch_bounds__(256, 2) void atlas_trace_kernel(AtlasK a, TraceK t, const float* __restrict__ packed) {
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
    float s = 0.0f;
    int moved = 0;
    float mean[Dec::NF];
    for (int it = 0; it < t.max_iters; ++it) {
      if (!__any(live)) break;
      const float dist = norm3(__fsub_rn(px, ox), __fsub_rn(py, oy), __fsub_rn(pz, oz));
      const float v = atlas_eval(a, dec, live, px, py, pz, true, mean);
      if (live) {
        s = v;
        conv = s < t.epsilon;
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
    }
    if (valid) {
      t.points[r * 3 + 0] = px; t.points[r * 3 + 1] = py; t.points[r * 3 + 2] = pz;
      t.hit[r] = conv ? 1 : 0;
      if (t.steps) t.steps[r] = moved;
    }
    if (t.sdf) {      // f at the returned point: a frozen ray has it; one that still moved at the cut-off does not
      if (__any(live)) {
        const float v = atlas_eval(a, dec, live, px, py, pz, true, mean);
        if (live) s = v;
      }
      if (valid) t.sdf[r] = s;
    }
    if (t.grad) {      // diff.gradient3d(method='finitediff'): (f(p + h e_a) - f(p - h e_a)) / (2 h), a = x, y, z
      const float two_h = __fmul_rn(2.0f, t.fd_step);
      float fplus = 0.0f;
#pragma unroll 1
      for (int k = 0; k < 6; ++k) {
        const int axis = k >> 1;
        const float sh = (k & 1) ? -t.fd_step : t.fd_step;
        const float qx = axis == 0 ? __fadd_rn(px, sh) : px;
        const float qy = axis == 1 ? __fadd_rn(py, sh) : py;
        const float qz = axis == 2 ? __fadd_rn(pz, sh) : pz;
        const float v = atlas_eval(a, dec, valid, qx, qy, qz, true, mean);
        if (k & 1) {
          if (valid) t.grad[r * 3 + axis] = __fdiv_rn(__fsub_rn(fplus, v), two_h);
        } else {
          fplus = v;
        }
      }
    }
  }
}

template <int C, int L, int H, int NH>
static hipError_t launch_trace_t(FusedShape<C, L, H, NH>, const AtlasK& a, const TraceK& t, const float* packed, bool split,
                                 hipStream_t s) {
  const FwdLaunch dims(C * L, H, NH, split, t.n, 2048u);
  auto k = split ? atlas_trace_kernel<C, L, H, NH, true> : atlas_trace_kernel<C, L, H, NH, false>;
  hipError_t e = allow_dynamic_lds((const void*)k, dims.lds);
  if (e != hipSuccess) return e;
  k<<<dims.blocks, 256, dims.lds, s>>>(a, t, packed);
  return hipGetLastError();
}

hipError_t launch_atlas_trace(int C, int L, int H, int NH, const AtlasK& a, const TraceK& t, const float* packed, bool exact,
                              hipStream_t s) {
  if (t.n == 0) return hipSuccess;
  const bool split = use_split(exact);
  return with_fused_shape(C, L, H, NH, hipErrorInvalidValue,
                          [&](auto shape) { return launch_trace_t(shape, a, t, packed, split, s); });
}

}  // namespace miso

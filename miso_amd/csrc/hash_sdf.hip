// Fused SDF query of hash-indexed levels (include/miso_hash_sdf.h): hash_sdf_fwd_kernel is sdf_fwd_kernel
// (sdf_fused.hip) with the corner rows looked up through the tables of hash_grid.hpp -- the same persistent wavefronts
// of 64 points, the same FwdDecoder (decoder.hpp: the forward image in LDS, the chains, the closing); only the
// gather differs: hash_cell + corner_rows + 16-byte row loads, summed corner by corner with fma (the PIN_FMA form of
// decoder.hpp's gather_level).  A table that lists a dense level's vertices therefore gives sdf_fwd_kernel's bits, sign
// words included.  Points arrive in the caller's order; there is no binned form and no loss.
//
// The backward is composed, not written: the decoder's backward chain depends on the grid through C and L alone, so
// launch_sdf_bwd in its lean form (no gradient buffer on any level, no grad_x: nothing of x or the grid is touched)
// writes the d-feat rows (n, F), and hash_encode.hip's two backward kernels consume them as their grad_feats.
//
// Registers of hash_sdf_fwd_kernel<C, L, H, NH, SPLIT> (gfx950, hipcc -O3, -Rpass-analysis=kernel-resource-usage): VGPRs
// and the wavefronts per SIMD they allow; no AGPRs, scratch 0 and no static LDS in every instantiation (the LDS is
// dynamic: FwdLaunch sizes it, as for sdf_fwd_kernel).  __launch_bounds__(256, 2) asks for the two workgroups
// per CU that the 512-block cap launches; the H = 32 decoders over C = 4 fit three or four.
//   shape            split: VGPRs (waves)   exact: VGPRs (waves)
//   <4, 1, 32, 1>     140 (3)                117 (4)
//   <4, 1, 64, 1>     206 (2)                192 (2)
//   <4, 2, 32, 1>     152 (3)                126 (4)
//   <4, 2, 64, 1>     216 (2)                208 (2)
//   <4, 3, 64, 1>     230 (2)                218 (2)
//   <4, 4, 64, 1>     242 (2)                228 (2)
//   <8, 1, 64, 1>     208 (2)                198 (2)
//   <8, 2, 64, 1>     226 (2)                212 (2)
//   <8, 3, 64, 1>     244 (2)                216 (2)
//   <8, 4, 64, 1>     256 (2)                227 (2)
//   <8, 3, 32, 1>     192 (2)                162 (3)
#include <string.h>

#include "checks.hpp"
#include "hash_grid.hpp"
#include "sdf_fused.hpp"
#include "../../include/miso_hash_sdf.h"

namespace miso {

template <int C, int L, int H, int NH, bool SPLIT>
__global__ __launch_bounds__(256, MISO_FWD_OCC) void hash_sdf_fwd_kernel(HashGridK g, const float* __restrict__ packed,
                                                                        const float* __restrict__ x, int64_t n,
                                                                        float* __restrict__ sdf,
                                                                        uint32_t* __restrict__ mask) {
  using Dec = FwdDecoder<C * L, H, NH, SPLIT, false>;      // sdf_fwd_kernel's
  constexpr int KS0 = Dec::KS0, MW = Dec::MW;               // MW: mask words per lane
  const Dec dec(packed);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nchunks = (n + 63) / 64;

  ChunkSched sched(nchunks, wave, 4, false);
  for (int64_t chunk = sched.cur; chunk < sched.end; chunk += sched.step) {
    asm volatile("" ::: "memory");  // see sdf_fwd_kernel: the LDS reads of biases / weights stay inside the loop
    const int64_t p = chunk * 64 + lane;
    const bool valid = p < n;
    float f[2 * KS0];
#pragma unroll
    for (int i = 0; i < 2 * KS0; ++i) f[i] = 0.0f;
    memory_phase(true);
    if (valid) {
      const float px = x[p * 3 + 0], py = x[p * 3 + 1], pz = x[p * 3 + 2];
      hash_gather_row<C, L>(g, px, py, pz, f);
    }
    memory_phase(false);
    uint32_t mw[MW];
    const float sdf_v = dec.template decode<true>(f, mw);
    if (valid) sdf[p] = sdf_v;
    if (mask) {
      uint32_t* mo = mask + (chunk * 64 + lane) * MW;
#pragma unroll
      for (int i = 0; i < MW; ++i) mo[i] = mw[i];
    }
  }
}

template <int C, int L, int H, int NH>
static hipError_t launch_hash_fwd_t(FusedShape<C, L, H, NH>, const HashGridK& g, const float* packed, bool exact,
                                    const float* x, int64_t n, float* sdf, uint32_t* mask, hipStream_t s) {
  const bool split = use_split(exact);
  const FwdLaunch dims(C * L, H, NH, split, n, 512u);      // persistent: two workgroups per CU
  auto k = split ? hash_sdf_fwd_kernel<C, L, H, NH, true> : hash_sdf_fwd_kernel<C, L, H, NH, false>;
  hipError_t e = allow_lds((const void*)k, dims.lds);
  if (e != hipSuccess) return e;
  k<<<dims.blocks, 256, dims.lds, s>>>(g, packed, x, n, sdf, mask);
  return hipGetLastError();
}

// (hash_grid.hpp declares the two checks below: hash_trace.hip states its own with them)
int hash_sdf_call(HashSdfCall* f, const miso_hash_grid_t* grid, const miso_mlp_t* m, bool need_table) {
  if (int rc = convert_hash_grid(grid, &f->g, need_table)) return rc;
  if (!m) return MISO_E_BADARG;
  if (m->n_linear < 2 || m->n_linear > MISO_MAX_LINEAR) return MISO_E_UNSUPPORTED;
  const HashGridK& g = f->g;
  for (int l = 0; l < g.n_levels; ++l)
    if (g.lv[l].C != g.lv[0].C) return MISO_E_UNSUPPORTED;
  if (m->in_dim != g.F || m->out_dim != 1) return MISO_E_UNSUPPORTED;
  f->C = g.lv[0].C; f->L = g.n_levels; f->H = m->hidden_dim; f->NH = m->n_linear - 2;
  return fused_shape_supported(f->C, f->L, f->H, f->NH) ? MISO_OK : MISO_E_UNSUPPORTED;      // (C in {4, 8}: the table's)
}

// what both launching entries ask of the decoder arguments and the batch, before the grid is looked at
int hash_sdf_args(const float* packed, uint32_t decoder_flags, int64_t n) {
  if (n < 0 || !set_if(n, packed) || !aligned(16, packed)) return MISO_E_BADARG;      // packed is read with 16-byte loads
  return (decoder_flags & ~MISO_F_EXACT_F32) ? MISO_E_BADARG : MISO_OK;
}

}  // namespace miso

using namespace miso;

extern "C" {

int miso_hash_sdf_supported(const miso_hash_grid_t* grid, const miso_mlp_t* mlp) {
  HashSdfCall f;
  return hash_sdf_call(&f, grid, mlp, false) == MISO_OK ? 1 : 0;
}

int64_t miso_hash_sdf_bwd_workspace_floats(const miso_hash_grid_t* grid, int64_t n) {
  HashGridK g;
  if (n <= 0 || !blocks_fit(n) || convert_hash_grid(grid, &g, false) != MISO_OK) return 0;
  return n * g.F;
}

int miso_hash_sdf_fwd(const miso_hash_grid_t* grid, const miso_mlp_t* mlp, const float* packed, uint32_t decoder_flags,
                      const float* x, int64_t n, float* sdf, uint32_t* relu_mask, void* stream) {
  if (int rc = hash_sdf_args(packed, decoder_flags, n)) return rc;
  if (!set_if(n, x, sdf)) return MISO_E_BADARG;
  HashSdfCall f;
  if (int rc = hash_sdf_call(&f, grid, mlp, true)) return rc;
  if (!blocks_fit(n)) return MISO_E_TOOLARGE;
  if (n == 0) return MISO_OK;
  const bool exact = (decoder_flags & MISO_F_EXACT_F32) != 0;
  return (int)with_fused_shape(f.C, f.L, f.H, f.NH, hipErrorInvalidValue, [&](auto shape) {
    return launch_hash_fwd_t(shape, f.g, packed, exact, x, n, sdf, relu_mask, (hipStream_t)stream);
  });
}

int miso_hash_sdf_bwd(const miso_hash_grid_t* grid, const miso_mlp_t* mlp, const float* packed, uint32_t decoder_flags,
                      const float* x, int64_t n, const float* grad_sdf, const uint32_t* relu_mask, float* grad_x,
                      float* workspace, void* stream) {
  if (int rc = hash_sdf_args(packed, decoder_flags, n)) return rc;
  if (!set_if(n, x, grad_sdf, relu_mask, workspace) || !aligned(16, workspace)) return MISO_E_BADARG;
  HashSdfCall f;
  if (int rc = hash_sdf_call(&f, grid, mlp, grad_x != nullptr)) return rc;
  if (!blocks_fit(n)) return MISO_E_TOOLARGE;
  if (n == 0) return MISO_OK;
  // The decoder's backward chain in its lean form: a grid of the same (C, L) whose levels carry no data and no gradient
  // buffer, no grad_x -- sdf_bwd_kernel then reads grad_sdf and the sign words, writes the d-feat rows, and touches
  // neither x nor a level.
  GridK stub;
  memset(&stub, 0, sizeof(stub));
  stub.n_levels = f.L;
  stub.ignore_mask = f.g.ignore_mask;
  stub.flags = decoder_flags & MISO_F_EXACT_F32;
  stub.xstride = 3;
  stub.F = f.g.F;
  for (int l = 0; l < f.L; ++l) { stub.lv[l].C = f.C; stub.lv[l].foff = l * f.C; }
  hipStream_t st = (hipStream_t)stream;
  if (hipError_t e = launch_sdf_bwd(f.C, f.L, f.H, f.NH, stub, packed, nullptr, n, grad_sdf, relu_mask, nullptr, true, nullptr,
                                    workspace, 0u, false, st))
    return (int)e;
  return (int)launch_hash_bwd(f.g, x, n, workspace, f.g.F, grad_x, st);
}

}  // extern "C"

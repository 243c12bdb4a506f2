// What the fused decoder kernels share across their translation units -- sdf_fused.hip (forward, backward, weight pack),
// sdf_train.hip (the one-launch training step) and atlas.hip (the atlas query, which uses the host part only): the
// decoder chains (decoder.hpp), the d-feat tile and scatter behind a backward chain (dfeat_tile.hpp), the wavefront
// priority of a memory phase, the chunk schedule of the persistent waves, the list of instantiated decoder shapes with
// its dispatcher, and the choice between the two decoder arithmetics.
#pragma once
#include <stdlib.h>

#include "decoder.hpp"
#include "dfeat_tile.hpp"
#include "launch.hpp"

namespace miso {

// Two wavefronts share a SIMD (and its MFMA pipe).  A wave raises its issue priority while it is in
// a memory phase (corner gathers, scatter) and drops it for the MFMA chain, so that its loads and
// address arithmetic slip in between the co-resident wave's matrix instructions instead of queueing
// behind them.  Measured: forward over unsorted points 80 -> 66 us; sorted 46 -> 45 us.  (Fixed
// per-slot priorities and start delays were tried first: no effect.)
__device__ __forceinline__ void memory_phase(bool on) {
  if (on) __builtin_amdgcn_s_setprio(3);
  else __builtin_amdgcn_s_setprio(0);
}
// sdf_bwd_kernel's form, with the ablation bits of rounds 2-6 (tune is always 0 now): kept so that the kernel compiles to
// the code it had -- without them its coordinate gradient came out wrong now and then
__device__ __forceinline__ void memory_phase(bool on, uint32_t tune, bool first = false) {
  if (tune & 16u) return;
  if (on) __builtin_amdgcn_s_setprio(3);
  else if ((tune & 64u) && first) __builtin_amdgcn_s_setprio(2);
  else __builtin_amdgcn_s_setprio(0);
}

#ifndef MISO_FWD_OCC
#define MISO_FWD_OCC 2
#endif

// Chunk schedule of the persistent waves.  Plain batches: chunk = global wave id,
// grid-strided.  Tile-sorted batches (perm != nullptr): the chunk range is cut into 8
// contiguous parts, one per XCD (blocks are dispatched round-robin over the XCDs,
// block b -> XCD b % 8; a different placement only costs speed).  Spatially
// neighbouring points then stay on one XCD, so its L2 keeps ownership of the grid
// lines they gather from and scatter into: on MI355X an fp32 atomic that misses L2
// costs ~50 ns of request slot (21 G requests/s chip-wide, tools/ubench/atomics.hip),
// and a line bouncing between XCD L2s is the worst case.
struct ChunkSched {
  int64_t cur, end, step;
  __device__ __forceinline__ ChunkSched(int64_t nchunks, int wave, int nw, bool xcd_local) {
    if (xcd_local && gridDim.x >= 8) {
      const int xcd = blockIdx.x & 7, lb = blockIdx.x >> 3;
      const int nlb = (gridDim.x - xcd + 7) >> 3;  // blocks that share this residue
      const int64_t per = (nchunks + 7) / 8;
      const int64_t lo = per * xcd;
      end = lo + per < nchunks ? lo + per : nchunks;
      cur = lo + (int64_t)lb * nw + wave;
      step = (int64_t)nlb * nw;
    } else {
      cur = (int64_t)blockIdx.x * nw + wave;
      end = nchunks;
      step = (int64_t)gridDim.x * nw;
    }
  }
};

// ---------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------
static inline hipError_t allow_lds(const void* k, size_t lds) { return allow_dynamic_lds(k, lds); }

// Decoder arithmetic of a launch: bf16x3 split products (default) or the exact fp32 chains (exact: MISO_F_EXACT_F32 in the
// call's flags; MISO_EXACT_F32=1 in the environment forces it for a whole process -- dev A/B)
static inline bool use_split(bool exact) {
  static const bool env_exact = [] { const char* e = getenv("MISO_EXACT_F32"); return e && atoi(e) != 0; }();
  return !exact && !env_exact;
}

// The decoder shapes (C, L, H, NH) the fused kernels are instantiated for.  The order is the order of the kernels in the
// code objects: append, do not sort.
#define MISO_FUSED_SHAPES(X) \
  X(4, 1, 32, 1) X(4, 1, 64, 1) X(4, 2, 32, 1) X(4, 2, 64, 1) X(4, 3, 64, 1) X(4, 4, 64, 1) \
  X(8, 1, 64, 1) X(8, 2, 64, 1) X(8, 3, 64, 1) X(8, 4, 64, 1) X(8, 3, 32, 1)

template <int C, int L, int H, int NH>
struct FusedShape {};

// fn(FusedShape<C, L, H, NH>()) for the instantiated shape that equals the run-time one, or not_covered
template <class R, class Fn>
static inline R with_fused_shape(int C, int L, int H, int NH, R not_covered, Fn&& fn) {
#define X(c, l, h, nh) \
  if (C == c && L == l && H == h && NH == nh) return fn(FusedShape<c, l, h, nh>());
  MISO_FUSED_SHAPES(X)
#undef X
  return not_covered;
}

}  // namespace miso

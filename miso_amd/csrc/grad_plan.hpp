// The grid gradient of one binned call, decided once: which levels are formed from the d-feat rows, which of
// those are pushed, which are scattered by the kernel or zero-filled first, and the one pull kernel that follows.  Host
// logic only, no HIP call: capi.hip builds a plan per entry point, launch_grad_pull(_mc) carry it out.
#pragma once
#include "grad_pull.hpp"

namespace miso {

enum GradCaller { GRAD_BWD, GRAD_TRAIN, GRAD_PULL };      // miso_sdf_bwd | miso_sdf_train | miso_grad_pull(_dx)
enum PullForm {
  PULL_NONE,       // nothing left to pull (no owned level, or all of them pushed)
  PULL_MC,         // grad_pull_mc_kernel
  PULL_WAVE,       // grad_pull_kernel, one wavefront per tile
  PULL_BLOCK,      // grad_pull_block_kernel, one workgroup per 2 x 2 x 2 tiles
  PULL_FILL,       // an empty batch under a per-axis binning: the gradient of nothing is zero, written under OVERWRITE
  PULL_INVALID     // a per-axis binning the matrix-core kernel does not take (MISO_PULL_MC=0, gg_x): hipErrorInvalidValue
};

// Environment knobs, read at every call: the tests toggle them within a process to reach kernels that other inputs
// reach too.
struct PullKnobs {
  bool mc_off, no_split;      // MISO_PULL_MC=0: vector kernels only; MISO_PULL_NO_SPLIT: heavy tiles are not cut
};
constexpr int PULL_DENSE_MIN = 100;      // samples per tile, on average, from which coarse levels are pushed
PullKnobs pull_knobs();

struct GradAsk {
  GradCaller caller;
  bool vec4;                  // convert_grid's: every level 16-byte addressable, channels contiguous
  uint32_t flags;             // miso_grid_t.flags: GRAD_OVERWRITE and GRAD_ZEROED (CROWDED is read from GridK::flags)
  int64_t n, ld;              // batch size; row pitch of the d-feat rows in floats
  bool ggx;                   // MODE 1: the rows are weighted by gg_x (miso_grad_pull_dx)
  bool workspace;             // a 16-byte-aligned d-feat workspace
  bool sorted, xn;            // a sorted batch (else the next two are 0); it has xn_sorted
  int32_t tiles;              // miso_sorted_t.tiles_per_axis
  int64_t queue_ints;         // ints of miso_sorted_t.pull_queue, 0 without one
};

struct GradPlan {
  bool valid, refuse;         // the tiles code decodes; MISO_E_UNSUPPORTED, before anything is launched
  int T[3];
  uint32_t want;              // levels whose gradient the call forms
  uint32_t owned;             // ... from the d-feat rows (pull or push): the kernel's defer mask, miso_grad_pull_levels
  uint32_t push;              // ... of those through grad_push_mfma_kernel
  uint32_t scatter;           // ... with float atomics from the backward / training kernel: want & ~owned
  uint32_t fill;              // levels to zero-fill before the first launch: those atomics add to, 0 when no fill is due
  PullForm form;              // what serves owned & ~push
  bool drain;                 // PULL_WAVE / PULL_BLOCK: the launch that works off the slice queue follows,
  int qcap;                   // ... and the queue's item capacity
  int overwrite;              // PullK's, McK's
  int64_t n, ld;              // GradAsk's
  int nl, lev[PULL_MAXL];     // the pulled levels, and per level and axis:
  int bdiv[PULL_MAXL][3];     // size / T where T divides the size, else 0
  float inv_size[PULL_MAXL][3];
  int blk_off[PULL_MAXL], blk_cap[PULL_MAXL];   // PULL_BLOCK: partition of a tile's list pool over the levels
};
GradPlan plan_grad(const GridK& g, const GradAsk& a, const PullKnobs& k);

// what a launch reads besides the plan (as PullK names them)
struct PullBatch { const int* tile_off; const float *xn, *dfeat; const int* perm; const float* ggx; int32_t* queue; };

}  // namespace miso

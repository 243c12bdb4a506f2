// plan_grad: see grad_plan.hpp.  Every fit condition of the pull, push and matrix-core kernels is stated here, once.
#include <stdlib.h>

#include "grad_plan.hpp"

namespace miso {

PullKnobs pull_knobs() {
  const char* mc = getenv("MISO_PULL_MC");
  return PullKnobs{mc && atoi(mc) == 0, getenv("MISO_PULL_NO_SPLIT") != nullptr};
}

// A tile's brick of the level is at most PULL_BMAX^3 vertices, and the kernels' tile arithmetic stays within an int.
// Levels with larger bricks (ScanNet's 200 x 100 x 200 over 16 tiles: 13 x 7 x 13) are scattered with float atomics:
// owner-computes was built for them four ways over two rounds (tools/experiments/README.md), never cheaper than those.
static bool brick_fits(const LevelK& lv, const int T[3]) {
  const int size[3] = {lv.X, lv.Y, lv.Z};
  for (int a = 0; a < 3; ++a)
    if ((size[a] + T[a] - 1) / T[a] > PULL_BMAX || (int64_t)size[a] * T[a] >= (1 << 28)) return false;
  return true;
}

// the matrix-core kernel's sweep covers <= 7 tile rows per axis (64 in all: its lane table): no cells much wider than tiles
static bool mc_reaches(const LevelK& lv, const int T[3]) {
  return 3 * lv.X >= 2 * T[0] && 3 * lv.Y >= 2 * T[1] && 3 * lv.Z >= 2 * T[2];
}
// every tile's region of the level is within PUSH_R vertices per axis (cubic binning)
static bool push_fits(const LevelK& lv, int T) {
  const int size[3] = {lv.X, lv.Y, lv.Z};
  for (int a = 0; a < 3; ++a)
    for (int t = 0; t < T; ++t)
      if (push_r1(t, size[a], T) - push_r0(t, size[a], T) + 1 > PUSH_R) return false;
  return true;
}

GradPlan plan_grad(const GridK& g, const GradAsk& a, const PullKnobs& k) {
  GradPlan p = {};
  p.valid = tiles_xyz(a.tiles, p.T);
  p.n = a.n; p.ld = a.ld;
  const bool cubic = tiles_cubic16(a.tiles);      // the vector kernels and the push: cubic binnings of <= 16 tiles only
  uint32_t have = 0;                              // levels with a gradient buffer
  for (int l = 0; l < g.n_levels; ++l)
    if (g.lv[l].grad) have |= 1u << l;

  // What differs between the callers (kept as found; a behaviour fix is its own change):
  //  * the backward forms EVERY level with a buffer, ignored ones included (so under OVERWRITE they are filled); the
  //    training step leaves ignored levels out of `want`: one that cannot be owned is neither filled nor scattered
  //    there.  Ignored levels that can be owned stay owned in both: the pull writes their zeros.
  //  * the backward plans a pull only with a sorted batch, its xn_sorted, an aligned workspace and a gradient buffer;
  //    the training step with a sorted batch and a workspace; a stand-alone pull always.
  //  * the backward honours OVERWRITE without a sorted batch too, the training step only with one.
  //  * a stand-alone pull pushes nothing, refuses unless every level with a buffer is owned, and with gg_x goes to the
  //    vector kernels without the 2 GB refusal.
  bool pulls = true;
  p.want = have;
  p.overwrite = (a.flags & MISO_F_GRAD_OVERWRITE) ? 1 : 0;
  if (a.caller == GRAD_BWD) pulls = a.sorted && a.xn && a.workspace && have;
  if (a.caller == GRAD_TRAIN) {
    pulls = a.sorted && a.workspace;
    p.want = have & ~g.ignore_mask;
    if (!a.sorted) p.overwrite = 0;
  }

  // ---- owned: default sampling convention, 4 or 8 contiguous channels (what the kernels are compiled for, one count
  // per grid), bricks that fit, at most PULL_MAXL levels; under a per-axis or finer-than-16 binning only what the
  // matrix-core kernel reaches, for nothing else serves such a binning
  const int C = g.lv[0].C;
  bool channels_ok = a.vec4 && (C == 4 || C == 8);
  for (int l = 0; l < g.n_levels; ++l) channels_ok = channels_ok && g.lv[l].C == C;
  if (pulls && p.valid && channels_ok && !(g.flags & (MISO_F_ALIGN_CORNERS | MISO_F_PAD_BORDER))) {
    int cnt = 0;
    for (int l = 0; l < g.n_levels; ++l) {
      if (!((have >> l) & 1u) || !brick_fits(g.lv[l], p.T) || (!cubic && !mc_reaches(g.lv[l], p.T))) continue;
      if (cnt++ < PULL_MAXL) p.owned |= 1u << l;
    }
  }

  // ---- push: coarse levels under a crowd -- an average of PULL_DENSE_MIN samples per tile, or MISO_F_CROWDED: the caller
  // knows the batch piles up on a few tiles (ray samples: a 54 000-sample batch of the synthetic RGB-D demo put 112 us of
  // pull + drain launches on the 40 x 20 x 40 level, the push 46 us); a uniform batch below the threshold is better off
  // pulled (cfg-2: 107 -> 180 us).  (A finer binning: the matrix-core pull takes crowded levels as they come.)
  const bool crowded = (g.flags & MISO_F_CROWDED) != 0 && a.n >= 4096;
  if (a.caller != GRAD_PULL && cubic && a.n < (1ll << 31) &&
      (crowded || a.n >= (int64_t)PULL_DENSE_MIN * p.T[0] * p.T[0] * p.T[0]))
    for (int l = 0; l < g.n_levels; ++l)
      if (((p.owned >> l) & 1u) && push_fits(g.lv[l], p.T[0])) p.push |= 1u << l;

  p.scatter = p.want & ~p.owned;
  // atomics (scatter, push) add to what is there: under OVERWRITE the caller's buffers are cleared first, unless it did
  if (p.overwrite && !(a.flags & MISO_F_GRAD_ZEROED) && a.caller != GRAD_PULL) p.fill = p.push | p.scatter;

  // ---- the pull of the rest
  const uint32_t pulled = p.owned & ~p.push;
  bool all_reached = true;
  for (int l = 0; l < g.n_levels; ++l) {
    if (!((pulled >> l) & 1u)) continue;
    const int size[3] = {g.lv[l].X, g.lv[l].Y, g.lv[l].Z};
    for (int x = 0; x < 3; ++x) {
      p.bdiv[p.nl][x] = (size[x] % p.T[x] == 0) ? size[x] / p.T[x] : 0;
      p.inv_size[p.nl][x] = 1.0f / (float)size[x];
    }
    all_reached = all_reached && mc_reaches(g.lv[l], p.T);
    p.lev[p.nl++] = l;
  }
  // the matrix-core kernel addresses the d-feat rows with 32-bit byte offsets: rows past 2 GB are not for it
  const bool rows_2gb = a.n * a.ld * 4 >= (1ll << 31);
  if (!pulled) {      // PULL_NONE
  } else if (!a.ggx && !k.mc_off && a.n > 0 && a.ld > 0 && !rows_2gb && all_reached) {
    p.form = PULL_MC;
  } else if (!cubic) {
    p.form = a.n > 0 ? PULL_INVALID : PULL_FILL;
  } else {
    // block kernel: an even binning, bricks of (size / T)^3 for every level, at most three of them (its instantiations)
    bool block_ok = p.T[0] % 2 == 0 && p.nl <= 3;
    for (int d = 0; d < p.nl; ++d)
      for (int x = 0; x < 3; ++x) block_ok = block_ok && p.bdiv[d][x] > 0;
    p.form = block_ok ? PULL_BLOCK : PULL_WAVE;
    if (block_ok) {      // a tile's list pool, split in proportion to the catchment volume ((B+1)/B)^3 of each level's brick
      double w[PULL_MAXL], wsum = 0.0;
      for (int d = 0; d < p.nl; ++d) {
        w[d] = 1.0;
        for (int x = 0; x < 3; ++x) w[d] *= (double)(p.bdiv[d][x] + 1) / (double)p.bdiv[d][x];
        wsum += w[d];
      }
      for (int d = 0, off = 0; d < p.nl; ++d) {
        p.blk_off[d] = off;
        p.blk_cap[d] = (d + 1 == p.nl) ? BLK_POOL - off : ((int)(BLK_POOL * w[d] / wsum) & ~1);
        off += p.blk_cap[d];
      }
    }
    // heavy tiles are cut into queued slices (a cubic binning has <= 16^3 tiles: the 12 bits of a queue item)
    p.drain = a.queue_ints > PULL_QHDR && !k.no_split;
    if (p.drain) p.qcap = (int)((a.queue_ints - PULL_QHDR) < (1 << 30) ? (a.queue_ints - PULL_QHDR) : (1 << 30));
  }

  // ---- refusals.  Under a per-axis binning rows past 2 GB cannot be pulled at all: said BEFORE the step's first kernel
  // is launched (the launch used to fail after the backward had already deferred the levels).
  if (p.owned && !cubic && rows_2gb && !(a.caller == GRAD_PULL && a.ggx)) p.refuse = true;
  if (a.caller == GRAD_PULL && (have & ~p.owned)) p.refuse = true;      // every requested level must be pullable
  return p;
}

}  // namespace miso

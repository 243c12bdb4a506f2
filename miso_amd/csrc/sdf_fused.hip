// Fused multi-level encode + frozen-decoder MLP, forward and backward, for gfx950.
//
// Replaces GridNet.forward (grid_opt/models/grid_net.py:306-325) and its autograd
// backward with a frozen decoder: features never touch HBM, the decoder runs on
// the matrix cores -- by default as bf16x3 split products on v_mfma_f32_32x32x16_bf16
// (decoder.hpp, mlp_split.hpp: error against float64 equal to exact fp32), behind
// MISO_F_EXACT_F32 as exact fp32 FMA chains on v_mfma_f32_32x32x2_f32 (described
// below; both forms chain the accumulators of one layer into the next) -- and the
// backward needs only the ReLU sign bits saved by the forward (2*H bits per point)
// because the decoder's weights take no gradient.
//
// Work decomposition: one 64-lane wavefront owns a chunk of 64 points and never
// synchronises with other waves (no __syncthreads in the loop), so on one SIMD
// the gather phase of one wave overlaps the MFMA phase of its neighbour.
//
// MFMA chaining.  With D = A(32x2) * B(2x32) + C, points are the N (column)
// dimension and neurons the M (row) dimension.  The accumulator layout of
// 32x32x2 (col = lane&31, row = (j&3) + 8*(j>>2) + 4*(lane>>5) for register j)
// is, register by register, already a legal B operand of the next layer for the
// k-pair {row(j), row(j)+4}: lanes 0-31 hold k=row(j,0), lanes 32-63 hold
// k=row(j,1).  So activations stay in the accumulator registers from layer to
// layer; only the A operands (weights, pre-permuted by mlp_pack_kernel) come
// from LDS.  The first layer's B operand is built from the lane-per-point
// features with one v_permlane32_swap per k-pair.
#include "sdf_fused.hpp"

namespace miso {

__global__ void mlp_pack_kernel(MlpK m, int F, int H, int NH, float* __restrict__ out) {
  PackLayout pl(F, H, NH);
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pl.total_all) return;
  if (i >= pl.total) {
    // ---- bf16x3 section (decoder.hpp): dword i holds elements 2e, 2e+1 of piece q of one lane's A operand -----------------
    const float* w0 = m.w[0];
    const float* wo = m.w[1 + NH];
    int e = i, rt_m = pl.RT, kind = 0, h = 0;      // kind 0: W0 fwd, 1: Wh[h] fwd, 2: first backward product, 3: Wh[h]^T, 4: W0^T
    if (i < pl.s_wh) { e -= pl.s_w0; kind = 0; }
    else if (i < pl.s_fwd_end) { e -= pl.s_wh; kind = 1; h = e / split_matrix_dwords(pl.KBH, pl.RT); e %= split_matrix_dwords(pl.KBH, pl.RT); }
    else if (i < pl.s_whT) { e -= pl.s_bfirst; kind = 2; if (NH == 0) rt_m = 1; }
    else if (i < pl.s_w0T) { e -= pl.s_whT; kind = 3; h = e / split_matrix_dwords(pl.KBH, pl.RT); e %= split_matrix_dwords(pl.KBH, pl.RT); }
    else { e -= pl.s_w0T; kind = 4; rt_m = 1; }
    const int d = e & 3, lane = (e >> 2) & 63, q = (e >> 8) % 3, kr = (e >> 8) / 3, r = kr % rt_m, kb = kr / rt_m;
    uint32_t word = 0;
    for (int half = 0; half < 2; ++half) {
      const int el = 2 * d + half, hi = lane >> 5, row = 32 * r + (lane & 31);
      float v = 0.0f;
      if (kind == 0) {
        const int k = split_k_feat(kb, hi, el);
        v = (k < F) ? w0[row * F + k] : 0.0f;
      } else if (kind == 1) {
        v = m.w[1 + h][row * H + split_k_acc(kb, hi, el)];
      } else if (kind == 2) {
        const int mm = split_k_acc(kb, hi, el);      // the neuron of the last ReLU this element multiplies
        if (NH >= 1) v = __fmul_rn(m.w[NH][mm * H + row], wo[mm]);
        else v = (row < F) ? __fmul_rn(w0[mm * F + row], wo[mm]) : 0.0f;
      } else if (kind == 3) {
        v = m.w[1 + h][split_k_acc(kb, hi, el) * H + row];
      } else {
        v = (row < F) ? w0[split_k_acc(kb, hi, el) * F + row] : 0.0f;
      }
      uint32_t pc[3];
      bf16_split3(v, pc);
      word |= pc[q] << (16 * half);
    }
    reinterpret_cast<uint32_t*>(out)[i] = word;
    return;
  }
  float v = 0.0f;
  const int RT = pl.RT;
  if (i < pl.o_wh) {  // W0p
    int e = i - pl.o_w0;
    int r = e % RT, l = (e / RT) % 64, s = e / (RT * 64);
    int row = 32 * r + (l & 31), col = 2 * s + (l >> 5);
    v = (col < F) ? m.w[0][row * F + col] : 0.0f;
  } else if (i < pl.o_b0) {  // Whp
    int e = i - pl.o_wh;
    int r = e % RT, l = (e / RT) % 64, ks = (e / (RT * 64)) % pl.KS1, h = e / (RT * 64 * pl.KS1);
    int rp = ks / 16, j = ks % 16;
    int row = 32 * r + (l & 31), col = 32 * rp + row_of(j, l >> 5);
    v = m.w[1 + h][row * H + col];
  } else if (i < pl.o_bh) {
    int e = i - pl.o_b0;
    v = m.b[0] ? m.b[0][e] : 0.0f;
  } else if (i < pl.o_wo) {
    int e = i - pl.o_bh;
    int h = e / H;
    v = m.b[1 + h] ? m.b[1 + h][e % H] : 0.0f;
  } else if (i < pl.o_bo) {
    v = m.w[1 + NH][i - pl.o_wo];
  } else if (i < pl.fwd_end) {
    v = (i == pl.o_bo && m.b[1 + NH]) ? m.b[1 + NH][0] : 0.0f;
  } else if (i < pl.o_w0T) {  // WhTp
    int e = i - pl.o_whT;
    int r = e % RT, l = (e / RT) % 64, ks = (e / (RT * 64)) % pl.KS1, h = e / (RT * 64 * pl.KS1);
    int rp = ks / 16, j = ks % 16;
    int k = 32 * rp + row_of(j, l >> 5), irow = 32 * r + (l & 31);
    v = m.w[1 + h][k * H + irow];
  } else {  // W0Tp
    int e = i - pl.o_w0T;
    int l = e % 64, ks = e / 64;
    int rp = ks / 16, j = ks % 16;
    int k = 32 * rp + row_of(j, l >> 5), f = l & 31;
    v = (f < F) ? m.w[0][k * F + f] : 0.0f;
  }
  out[i] = v;
}

// ---------------------------------------------------------------------------
template <int C, int L, int H, int NH, bool SPLIT>
__global__ __launch_bounds__(256, MISO_FWD_OCC) void sdf_fwd_kernel(GridK g, const float* __restrict__ packed,
                                                        const float* __restrict__ x, int64_t n,
                                                        float* __restrict__ sdf,
                                                        uint32_t* __restrict__ mask,
                                                        const int* __restrict__ perm, LossInK lin) {
  // perm != nullptr: x is the tile-sorted copy of the batch (sort.hip) and the
  // result is written back in the caller's order, sdf[perm[p]].
  // lin.p.loss_type != 0 (binned batches only): the mapping loss of loss.hip is evaluated on the
  // spot -- d loss / d sdf goes to lin.gsdf_sorted[p] (binned order: the backward reads it
  // coalesced), the two loss sums are accumulated into lin.loss_out; sdf may then be NULL.
  using Dec = FwdDecoder<C * L, H, NH, SPLIT, false>;
  constexpr int KS0 = Dec::KS0, MW = Dec::MW;      // MW: mask words per lane
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const Dec dec(packed);      // the forward image to LDS (decoder.hpp)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nchunks = (n + 63) / 64;

  float loss_sdf = 0.0f, loss_fs = 0.0f;
  float inv_n = lin.inv_n;   // mean over the batch rows -- or over the live rows of a padded batch
  if (lin.p.loss_type && lin.n_live) { const int live = *lin.n_live; inv_n = 1.0f / (float)(live > 1 ? live : 1); }
  ChunkSched sched(nchunks, wave, 4, perm != nullptr);
  for (int64_t chunk = sched.cur; chunk < sched.end; chunk += sched.step) {
    // keep the (chunk-invariant) LDS reads of biases / weights inside the loop:
    // hoisted, they cost ~100 VGPRs and spill
    asm volatile("" ::: "memory");
    const int64_t p = chunk * 64 + lane;
    const bool valid = p < n;
    // loss inputs of this lane's point ({target, valid, sign, weight}, one 16-B row in the
    // caller's order): issued now, consumed after the MLP
    const int64_t po = (valid && perm) ? (int64_t)perm[p] : p;
    float4 l_in = make_float4(0.f, 1.f, 0.f, 1.f);
    if (lin.p.loss_type && valid) l_in = lin.aux[po];
    float f[2 * KS0];
#pragma unroll
    for (int i = 0; i < 2 * KS0; ++i) f[i] = 0.0f;
    memory_phase(true);
    if (valid) {
      float px, py, pz;
      load_point(g, x, p, px, py, pz);
      float bmn[3] = {g.bmin[0], g.bmin[1], g.bmin[2]}, bmx[3] = {g.bmax[0], g.bmax[1], g.bmax[2]};
      asm volatile("" : "+s"(bmn[0]), "+s"(bmn[1]), "+s"(bmn[2]), "+s"(bmx[0]), "+s"(bmx[1]), "+s"(bmx[2]));
#pragma unroll
      for (int l = 0; l < L; ++l) {
        LevelK lv = g.lv[l];
        if ((g.ignore_mask >> l) & 1u) continue;
        // The level constants are wave-uniform (SGPRs), but everything derived from them in float
        // (sizes, bound) would be hoisted out of the chunk loop into VGPRs and stay live across the
        // MFMA chain; laundering the integers keeps the conversions inside the loop.
        asm volatile("" : "+s"(lv.X), "+s"(lv.Y), "+s"(lv.Z));
        Axis a[3];
        const Cell c = level_cell(bmn, bmx, g.flags, lv, px, py, pz, a);
        gather_level<C>(lv, c, &f[l * C]);
      }
    }
    memory_phase(false);
    uint32_t mw[MW];
    const float sdf_v = dec.template decode<true>(f, mw);
    if (valid && sdf) sdf[po] = sdf_v;
    if (lin.p.loss_type && valid) {
      float gsd, gfs;
      map_loss_one(lin.p, sdf_v, l_in.x, l_in.w, l_in.y == 1.0f, lin.p.w_fs > 0.f && l_in.z == 1.0f, gsd, gfs,
                   loss_sdf, loss_fs);
      lin.gsdf_sorted[p] = (gsd + gfs) * inv_n;
    }
    if (mask) {
      uint32_t* mo = mask + (chunk * 64 + lane) * MW;
#pragma unroll
      for (int i = 0; i < MW; ++i) mo[i] = mw[i];
    }
  }
  if (lin.p.loss_type) {
    // block reduction through LDS (the weights are dead by now), then every block STORES its pair
    // into its own slot (and clears the slots no block owns): no atomics -- 1024 of them on two
    // addresses would be a 13 us serialised tail -- and nothing for the caller to zero.
    for (int o = 32; o > 0; o >>= 1) { loss_sdf += __shfl_down(loss_sdf, o); loss_fs += __shfl_down(loss_fs, o); }
    __syncthreads();
    if (lane == 0) { smem[2 * wave] = loss_sdf; smem[2 * wave + 1] = loss_fs; }
    __syncthreads();
    if (threadIdx.x == 0) {
      const float a = (smem[0] + smem[2]) + (smem[4] + smem[6]), b = (smem[1] + smem[3]) + (smem[5] + smem[7]);
      float2* slots = reinterpret_cast<float2*>(lin.loss_out);
      slots[blockIdx.x] = make_float2(lin.p.w_sdf * a * inv_n, lin.p.w_fs * b * inv_n);
      for (int sl = blockIdx.x + gridDim.x; sl < MISO_LOSS_SLOTS; sl += gridDim.x) slots[sl] = make_float2(0.f, 0.f);
    }
  }
}

// ---------------------------------------------------------------------------
// Backward: grad_sdf -> (MFMA chain through the transposed weights, gated by the
// saved ReLU bits) -> d feats in accumulator layout -> scatter-add into the level
// gradients and/or grad_x.  Lane (hi, l&31) holds, for tile t, point 32t+(l&31):
//   C == 8: channels 4hi..4hi+3 of level j>>2      (registers j = 4*level + c)
//   C == 4: channels 0..3 of level 2*(j>>2) + hi   (registers j = 4*g + c)
constexpr int BWD_GSDF_SORTED = 16, BWD_LEAN = 32;      // sdf_bwd_kernel's `debug` bits in use
template <int C, int L, int H, int NH, bool WANT_GRID, bool WANT_X, bool SPLIT>
__global__ __launch_bounds__(256, 2) void sdf_bwd_kernel(GridK g, const float* __restrict__ packed,
                                                        const float* __restrict__ x, int64_t n,
                                                        const float* __restrict__ gsdf,
                                                        const uint32_t* __restrict__ mask,
                                                        float* __restrict__ gx,
                                                        const int* __restrict__ perm, int debug,
                                                        float* __restrict__ dfeat_out,
                                                        uint32_t defer_mask) {
  // perm != nullptr: x and mask are in tile-sorted order, gsdf / gx in the caller's.
  // dfeat_out != nullptr: rows of d(feats) (N,F, sorted order) are written out and the levels in
  // defer_mask are NOT scattered here: grad_pull_kernel (grad_pull.hip) forms their gradient owner-computes.
  // debug: BWD_GSDF_SORTED and BWD_LEAN, set by the launcher.  Bits 1 (no atomics) and 8 (no scatter) were ablation
  // switches and are never set; their branches, and g.tune (always 0), stay so that the kernel compiles to the code it
  // had: without them the coordinate gradient of <4, 2, 32, 1, true, true> came out wrong now and then.
  constexpr int F = C * L, RT = H / 32;
  constexpr int MW = (NH + 1) * RT;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const PackLayout pl(F, H, NH);
  // stage wo + the transposed weights: [o_wo, o_bo) and [o_whT, total); the split form its backward block
  // [s_bfirst, total_all) (the output weights are folded into its first matrix; the H floats behind it stay unused)
  const int nb = SPLIT ? pl.total_all - pl.s_bfirst : pl.total - pl.o_whT;
  for (int i = threadIdx.x * 4; i < nb; i += blockDim.x * 4)
    *reinterpret_cast<float4*>(smem + i) = *reinterpret_cast<const float4*>(packed + (SPLIT ? pl.s_bfirst : pl.o_whT) + i);
  for (int i = threadIdx.x; i < H; i += blockDim.x) smem[nb + i] = packed[pl.o_wo + i];
  __syncthreads();
  const float* whT = smem;
  const float* w0T = smem + (pl.o_w0T - pl.o_whT);
  const float* wo = smem + nb;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hi = lane >> 5;
  constexpr int FP = dfeat_pitch(F), REC = CELL_REC;      // the tile and the cell records: dfeat_tile.hpp
  constexpr int WAVE_LDS = 64 * FP + 64 * L * REC;
  // BWD_LEAN (debug bit 32, set by the launcher when nothing is scattered from here): only the d-feat tile is
  // allocated per wave -- 50 KB per workgroup instead of 74, i.e. three workgroups per CU
  float* wave_lds = smem + ((nb + H + 3) / 4) * 4 + wave * ((debug & 32) ? 64 * FP : WAVE_LDS);
  const int64_t nchunks = (n + 63) / 64;
  // levels whose gradient is scattered from this kernel (binned training defers all of them to the
  // pull: then no per-point cell records are formed at all)
  uint32_t scatter_mask = 0;
  if (WANT_GRID)
    for (int l = 0; l < L; ++l)
      if (g.lv[l].grad && !((g.ignore_mask >> l) & 1u) && !((defer_mask >> l) & 1u)) scatter_mask |= 1u << l;

  ChunkSched sched(nchunks, wave, 4, perm != nullptr);
  for (int64_t chunk = sched.cur; chunk < sched.end; chunk += sched.step) {
    asm volatile("" ::: "memory");  // see sdf_fwd_kernel
    const int64_t pt[2] = {chunk * 64 + (lane & 31), chunk * 64 + 32 + (lane & 31)};
    float ds[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
      ds[t] = (pt[t] < n) ? gsdf[(perm && !(debug & 16)) ? (int64_t)perm[pt[t]] : pt[t]] : 0.0f;   // 16 = BWD_GSDF_SORTED
    uint32_t mw[MW];
    {
      const uint32_t* mi = mask + (chunk * 64 + lane) * MW;
#pragma unroll
      for (int i = 0; i < MW; ++i) mw[i] = mi[i];
    }
    f32x16 df[2];
    if constexpr (SPLIT) {
      u32x4 maskB[H / 16][2];
      mask_operand_from_bits<H, NH, false>(mw, maskB);
      decoder_bwd_split<F, H, NH, false>(reinterpret_cast<const uint32_t*>(smem), lane, maskB, mw, ds, df);
    } else {
      decoder_bwd_exact<F, H, NH>(whT, w0T, wo, kept_in_loop(lane), mw, ds, df);
    }      // exact fp32 chains
    // ---- scatter into the level gradients (dfeat_tile.hpp) ------------------------
    // d feats move from the accumulator layout to the scatter's lane order through a per-wave LDS tile; the cell
    // of every (point, level) is computed once (lane = point) and broadcast from LDS.
    memory_phase(true, g.tune);
    if (WANT_GRID && !(debug & 8)) {
      float* dF = wave_lds;                         // [64][FP]
      int* rec = reinterpret_cast<int*>(wave_lds + 64 * FP);   // [64][L][REC]
      dfeat_to_tile<F, 2>(df, dF, lane & 31, hi);
      if (scatter_mask) {     // cell records only where a level is still scattered from here
        const int64_t p = chunk * 64 + lane;
        const bool valid = p < n;
        float px = 0.f, py = 0.f, pz = 0.f;
        if (valid) load_point(g, x, p, px, py, pz);
#pragma unroll
        for (int l = 0; l < L; ++l) {
          const LevelK& lv = g.lv[l];
          Axis a[3];
          const Cell c = level_cell(g, lv, px, py, pz, a);
          write_cell_record(rec + (lane * L + l) * REC, c, lv, valid);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (dfeat_out) tile_to_rows<F, 64>(dF, dfeat_out + chunk * 64 * F, n - chunk * 64, lane);
      scatter_tile<C, L, true, GridK>(g, scatter_mask, dF, rec, 64, lane, (debug & 1) != 0);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    // ---- coordinate gradient (pose path): lane = (point, channel half) -----------
    if (WANT_X) {
      float gacc[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const bool valid = pt[t] < n;
        float px = 0.f, py = 0.f, pz = 0.f;
        if (valid) load_point(g, x, pt[t], px, py, pz);
        constexpr int NG = (C == 8) ? L : (L + 1) / 2;  // register groups of 4
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
          const int l = (C == 8) ? gi : 2 * gi + hi;
          const int choff = (C == 8) ? 4 * hi : 0;
          if (l >= L || !valid) continue;
          if ((g.ignore_mask >> l) & 1u) continue;
          // C == 4: the two lane halves work on different levels; pick the level's
          // fields with per-lane selects (a lane-varying index into the kernel
          // arguments would be spilled to scratch).
          LevelK lv = g.lv[(C == 8) ? gi : 2 * gi];
          if (C == 4 && 2 * gi + 1 < L && hi) lv = g.lv[(2 * gi + 1 < L) ? 2 * gi + 1 : 0];
          Axis a[3];
          const Cell c = level_cell(g, lv, px, py, pz, a);
          const float v0 = df[t][4 * gi + 0], v1 = df[t][4 * gi + 1], v2 = df[t][4 * gi + 2],
                      v3 = df[t][4 * gi + 3];
          float sx_ = 0.f, sy_ = 0.f, sz_ = 0.f;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
            if (!corner_in(c, k)) continue;
            int off = corner_offset(c, lv, k) + choff;
            float4 gv = *reinterpret_cast<const float4*>(lv.data + off);
            float dot = gv.x * v0 + gv.y * v1 + gv.z * v2 + gv.w * v3;
            float sx = dx ? 1.f : -1.f, sy = dy ? 1.f : -1.f, sz = dz ? 1.f : -1.f;
            sx_ += dot * sx * c.wy[dy] * c.wz[dz];
            sy_ += dot * sy * c.wx[dx] * c.wz[dz];
            sz_ += dot * sz * c.wx[dx] * c.wy[dy];
          }
          gacc[t][0] += sx_ * (g.gscale[0] * a[0].mult);
          gacc[t][1] += sy_ * (g.gscale[1] * a[1].mult);
          gacc[t][2] += sz_ * (g.gscale[2] * a[2].mult);
        }
      }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int a = 0; a < 3; ++a) gacc[t][a] += __shfl_xor(gacc[t][a], 32);
      const int64_t p = chunk * 64 + lane;
      if (p < n) {
        const int64_t po = perm ? (int64_t)perm[p] : p;
        gx[po * 3 + 0] = hi ? gacc[1][0] : gacc[0][0];
        gx[po * 3 + 1] = hi ? gacc[1][1] : gacc[0][1];
        gx[po * 3 + 2] = hi ? gacc[1][2] : gacc[0][2];
      }
    }
    memory_phase(false, g.tune);
  }
}

// ---------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------
template <int C, int L, int H, int NH>
static hipError_t launch_fwd_t(FusedShape<C, L, H, NH>, const GridK& g, const float* packed, const float* x, int64_t n,
                               float* sdf, uint32_t* mask, const int* perm, const LossInK& lin, hipStream_t s) {
  const bool split = use_split(g.flags & MISO_F_EXACT_F32);
  FwdLaunch dims(C * L, H, NH, split, n, 512u);      // persistent: two workgroups per CU
  if (lin.p.loss_type && dims.blocks > MISO_LOSS_SLOTS) dims.blocks = MISO_LOSS_SLOTS;   // one loss slot per block
  auto k = split ? sdf_fwd_kernel<C, L, H, NH, true> : sdf_fwd_kernel<C, L, H, NH, false>;
  hipError_t e = allow_lds((const void*)k, dims.lds);
  if (e != hipSuccess) return e;
  k<<<dims.blocks, 256, dims.lds, s>>>(g, packed, x, n, sdf, mask, perm, lin);
  return hipGetLastError();
}

template <int C, int L, int H, int NH>
static hipError_t launch_bwd_t(FusedShape<C, L, H, NH>, const GridK& g, const float* packed, const float* x, int64_t n,
                               const float* gsdf, const uint32_t* mask, float* gx, bool want_grid,
                               const int* perm, float* dfeat_out, uint32_t defer_mask, bool gsdf_sorted,
                               hipStream_t s) {
  PackLayout pl(C * L, H, NH);
  constexpr int F = C * L, FP = dfeat_pitch(F), WAVE_LDS = 64 * FP + 64 * L * CELL_REC;
  bool lean = want_grid && !gx && dfeat_out != nullptr;      // every gradient level deferred to the pull?
  for (int l = 0; l < L && lean; ++l)
    if (g.lv[l].grad && !((g.ignore_mask >> l) & 1u) && !((defer_mask >> l) & 1u)) lean = false;
  const bool split = use_split(g.flags & MISO_F_EXACT_F32);
  const int nb = split ? pl.total_all - pl.s_bfirst : pl.total - pl.o_whT;
  size_t lds = (size_t)(((nb + H + 3) / 4) * 4 + (want_grid ? 4 * (lean ? 64 * FP : WAVE_LDS) : 0)) * sizeof(float);
  int64_t nchunks = (n + 63) / 64;
  unsigned blocks = (unsigned)((nchunks + 3) / 4);
  const unsigned use_cap = lean ? 768u : 512u;
  if (blocks > use_cap) blocks = use_cap;
  const int debug = (gsdf_sorted ? BWD_GSDF_SORTED : 0) | (lean ? BWD_LEAN : 0);
  void (*k)(GridK, const float*, const float*, int64_t, const float*, const uint32_t*, float*, const int*, int,
            float*, uint32_t) =
      split ? ((want_grid && gx) ? sdf_bwd_kernel<C, L, H, NH, true, true, true>
               : want_grid       ? sdf_bwd_kernel<C, L, H, NH, true, false, true>
                                 : sdf_bwd_kernel<C, L, H, NH, false, true, true>)
            : ((want_grid && gx) ? sdf_bwd_kernel<C, L, H, NH, true, true, false>
               : want_grid       ? sdf_bwd_kernel<C, L, H, NH, true, false, false>
                                 : sdf_bwd_kernel<C, L, H, NH, false, true, false>);
  hipError_t e = allow_lds((const void*)k, lds);
  if (e != hipSuccess) return e;
  k<<<blocks, 256, lds, s>>>(g, packed, x, n, gsdf, mask, gx, perm, debug, dfeat_out, defer_mask);
  return hipGetLastError();
}

bool fused_shape_supported(int C, int L, int H, int NH) {
  return with_fused_shape(C, L, H, NH, false, [](auto) { return true; });
}

hipError_t launch_sdf_fwd(int C, int L, int H, int NH, const GridK& g, const float* packed,
                          const float* x, int64_t n, float* sdf, uint32_t* mask, const int* perm,
                          const LossInK& lin, hipStream_t s) {
  if (n == 0) return hipSuccess;
  return with_fused_shape(C, L, H, NH, hipErrorInvalidValue, [&](auto shape) {
    return launch_fwd_t(shape, g, packed, x, n, sdf, mask, perm, lin, s);
  });
}

hipError_t launch_sdf_bwd(int C, int L, int H, int NH, const GridK& g, const float* packed,
                          const float* x, int64_t n, const float* gsdf, const uint32_t* mask,
                          float* gx, bool want_grid, const int* perm, float* dfeat_out,
                          uint32_t defer_mask, bool gsdf_sorted, hipStream_t s) {
  if (n == 0) return hipSuccess;
  return with_fused_shape(C, L, H, NH, hipErrorInvalidValue, [&](auto shape) {
    return launch_bwd_t(shape, g, packed, x, n, gsdf, mask, gx, want_grid, perm, dfeat_out, defer_mask, gsdf_sorted, s);
  });
}

hipError_t launch_mlp_pack(const MlpK& m, int F, int H, int NH, float* out, hipStream_t s) {
  PackLayout pl(F, H, NH);
  mlp_pack_kernel<<<(pl.total_all + 255) / 256, 256, 0, s>>>(m, F, H, NH, out);
  return hipGetLastError();
}

int64_t mlp_packed_floats(int F, int H, int NH) { return PackLayout(F, H, NH).total_all; }

}  // namespace miso

// Training step in ONE kernel (binned batches, frozen decoder, every level's grid gradient left to the pull / push):
// gather -> decoder forward -> mapping loss -> decoder backward -> d-feat rows, per 64-point chunk, per wavefront.
// What sdf_fwd_kernel + sdf_bwd_kernel<.., true, false> do as two launches, minus everything that only carried state
// from one to the other: the ReLU sign bits (16 B per point written and read back), d loss / d sdf (4 + 4 B), the second
// kernel's launch, ramp and tail, its own staging of the weights -- and, what matters most on gfx950, the two phases
// now share a SIMD: fp32 MFMA and VALU use one datapath (tools/ubench/mfma_valu.hip), so a kernel's floor is the SUM
// of its matrix and vector clocks, but a wavefront waiting for its corner gathers costs the neighbour's matrix chain
// nothing.  The backward pass is ~all matrix work (it reads 20 B per point), the forward has the long memory phase:
// with both in one kernel a wavefront's gathers hide behind TWICE the matrix work of its neighbour.
// The split decoder chains (decoder.hpp) and the d-feat tile, cell records and scatter (dfeat_tile.hpp) are those of
// sdf_fwd_kernel and sdf_bwd_kernel (sdf_fused.hip; the kernels stay separate: those two also serve inference, the
// unsorted path, the coordinate backward and levels scattered from the backward).  The exact fp32 chains are written out
// here, each tile-1 statement under `if (!HALF)`: through decoder_fwd_exact / decoder_bwd_exact this kernel's exact
// instantiations took more VGPRs and more time (decoder.hpp's header).  The sign bits stay in the registers they were
// formed in, d loss / d sdf moves between the point-per-lane layout of the loss and the two 32-point tiles of the
// backward with two lane reads.
// SCAT: levels with a gradient that are NOT in defer_mask (bricks beyond what the pull owns: cfg-3's fine level; or
// every level of an unbinned batch, perm == nullptr) are scattered from here with float atomics (scatter_tile) -- the
// per-point cell records are kept in LDS from the forward's gather.  dfeat_out may then be null (nothing deferred).
// HALF: 32 points per wavefront and trip instead of 64 -- lanes 32..63 mirror lanes 0..31 (the same point, the same gather),
// only the first of the two 32-point matrix tiles is computed.  For batches that are one chunk per wavefront anyway (a
// few thousand samples: Newer College's 6 144, the tracker's windows): the wavefront's chain of matrix instructions halves,
// twice as many wavefronts share the batch.  Same arithmetic per point.
#include "sdf_fused.hpp"

namespace miso {

#ifdef MISO_ABL_NO_GATHER     // dev ablation (wrong results): the cell arithmetic without the corner loads
#define MISO_TRAIN_GATHER_LEVEL(lv, c, fo) \
  for (int q = 0; q < C; ++q) (fo)[q] = c.wx[0] * (float)(c.i0 + q) + c.wy[1] * (float)c.j0 + c.wz[0] * (float)c.k0
#else
#define MISO_TRAIN_GATHER_LEVEL(lv, c, fo) gather_level<C>(lv, c, fo)
#endif
// A chunk's input side (sdf_train_kernel): its point, label row and corner gathers (-> f) and, scattering, its cell records
// (-> recw: write_cell_record).  A macro, not a lambda: the non-scattering instantiations must compile to the loop they
// had before the scattering ones learnt to request a chunk's gathers one chunk early.
#define MISO_TRAIN_GATHER(CHUNK_, RECW_, P_O_, PO_O_, VALID_O_, LIN_O_)                                        \
  {                                                                                                         \
    const int64_t gp_ = HALF ? (CHUNK_) * 32 + (lane & 31) : (CHUNK_) * 64 + lane; \
    const bool gvalid_ = gp_ < n; \
    int64_t gpo_ = gp_; \
    if (gvalid_ && perm) gpo_ = (int64_t)perm[gp_]; \
    else if (gvalid_ && (g.flags & MISO_F_INDEX_IN_XN)) gpo_ = (int64_t)__float_as_int(reinterpret_cast<const float4*>(x)[gp_].w); \
    float4 glin_ = make_float4(0.f, 1.f, 0.f, 1.f); \
    if (gvalid_) glin_ = lin.aux[gpo_]; \
_Pragma("unroll") \
    for (int i = 0; i < 2 * KS0; ++i) f[i] = 0.0f; \
    memory_phase(true); \
    if (gvalid_) { \
      float px, py, pz; \
      load_point(g, x, gp_, px, py, pz); \
      float bmn[3] = {g.bmin[0], g.bmin[1], g.bmin[2]}, bmx[3] = {g.bmax[0], g.bmax[1], g.bmax[2]}; \
      asm volatile("" : "+s"(bmn[0]), "+s"(bmn[1]), "+s"(bmn[2]), "+s"(bmx[0]), "+s"(bmx[1]), "+s"(bmx[2])); \
_Pragma("unroll") \
      for (int l = 0; l < L; ++l) { \
        LevelK lv = g.lv[l]; \
        if ((g.ignore_mask >> l) & 1u) continue; \
        asm volatile("" : "+s"(lv.X), "+s"(lv.Y), "+s"(lv.Z)); \
        Axis a[3]; \
        const Cell c = level_cell(bmn, bmx, g.flags, lv, px, py, pz, a); \
      MISO_TRAIN_GATHER_LEVEL(lv, c, &f[l * C]); \
        if (SCAT && ((scatter_mask >> l) & 1u)) { \
          write_cell_record((RECW_) + (row_l * L + l) * REC, c, lv, true); \
        } \
      } \
    } else if (SCAT) { \
_Pragma("unroll") \
      for (int l = 0; l < L; ++l) (RECW_)[(row_l * L + l) * REC + CELL_REC_FLAGS] = 0; \
    } \
    memory_phase(false); \
    P_O_ = gp_; PO_O_ = gpo_; VALID_O_ = gvalid_; LIN_O_ = glin_; \
  }
template <int C, int L, int H, int NH, bool SCAT, int NW = 4, bool HALF = false, bool SPLIT = false>
__global__ __launch_bounds__(64 * NW, 2) void sdf_train_kernel(GridK g, const float* __restrict__ packed,
                                                          const float* __restrict__ x, int64_t n,
                                                          float* __restrict__ sdf, const int* __restrict__ perm,
                                                          LossInK lin, float* __restrict__ dfeat_out,
                                                          uint32_t defer_mask, bool rotate_records) {
  constexpr int F = C * L, RT = H / 32, KS0 = (F + 1) / 2, KS1 = H / 2;
  constexpr int MW = (NH + 1) * RT;
  constexpr int FP = dfeat_pitch(F), REC = CELL_REC;      // the d-feat tile and (SCAT) the cell records: dfeat_tile.hpp
  // SCAT: the cell records are double-buffered when the launcher found room for a second block (rotate_records,
  // TrainPlan::rotate) -- the next chunk's gathers are then issued in FRONT of this chunk's atomics, see the loop
  const bool rotate = SCAT && C * L <= MISO_ROTATE_MAX_F && rotate_records;
  const int WAVE_LDS = 64 * FP + (SCAT ? (rotate ? 2 : 1) * 64 * L * REC : 0);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const PackImage<SPLIT, true> img(F, H, NH);      // the whole pack (decoder.hpp)
  img.stage(packed);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hi = lane >> 5;
  constexpr int PTS = HALF ? 32 : 64;      // points per wavefront and trip
  const int64_t nchunks = (n + PTS - 1) / PTS;
  const float *w0p = img.w0p(), *whp = img.whp(), *b0 = img.b0(), *bh = img.bh(), *wo = img.wo();      // the exact chains'
  const float *whT = img.whT(), *w0T = img.w0T();
  const float bo = img.bo();
  float* dF = img.behind() + wave * WAVE_LDS;       // this wavefront's d-feat tile [64][FP]
  int* rec = reinterpret_cast<int*>(dF + 64 * FP);                      // SCAT: its cell records [64][L][REC]
  uint32_t scatter_mask = 0;
  if (SCAT)
    for (int l = 0; l < L; ++l)
      if (g.lv[l].grad && !((g.ignore_mask >> l) & 1u) && !((defer_mask >> l) & 1u)) scatter_mask |= 1u << l;

  float loss_sdf = 0.0f, loss_fs = 0.0f;
  float inv_n = lin.inv_n;
  if (lin.n_live) { const int live = *lin.n_live; inv_n = 1.0f / (float)(live > 1 ? live : 1); }
  ChunkSched sched(nchunks, wave, NW, true);
  const int row_l = HALF ? (lane & 31) : lane;      // this lane's row of the wavefront's LDS tile / records
  float f[2 * KS0];
  // Rotated (scattering, room for two record blocks): chunk k+1's gathers are requested between chunk k's decoder
  // backward and its atomics.  The atomics execute at the memory side at a fixed rate and queue up in the CU's memory
  // pipeline; a gather requested behind them waits for all of them, and with every wavefront of the launch in the same
  // phase the kernel took (decoder time) + (atomic time).  Requested in front of them, the next chunk's rows arrive
  // while the atomics drain and its decoder runs under them (cfg-3 trainer step 295 -> 279 us).
  int* rec_cur = rec;
  int* rec_nxt = rotate ? rec + 64 * L * REC : rec;
  int64_t p_n = 0, po_n = 0;      // (rotated) the coming chunk's point index (binned / caller order), ...
  bool valid_n = false;
  float4 l_in_n = make_float4(0.f, 1.f, 0.f, 1.f);
  if (rotate && sched.cur < sched.end) MISO_TRAIN_GATHER(sched.cur, rec_cur, p_n, po_n, valid_n, l_in_n)
  for (int64_t chunk = sched.cur; chunk < sched.end; chunk += sched.step) {
    asm volatile("" ::: "memory");      // see sdf_fwd_kernel (sdf_fused.hip): keeps the LDS reads of weights / biases inside the loop
    int64_t p, po;
    bool valid;
    float4 l_in;
    if (!rotate) MISO_TRAIN_GATHER(chunk, rec_cur, p, po, valid, l_in)
    else { p = p_n; po = po_n; valid = valid_n; l_in = l_in_n; }
    // ================================ forward =====================================================================
    uint32_t mw[MW];
    float p0 = 0.0f, p1 = 0.0f, poison = 0.0f;
    u32x4 maskB[H / 16][HALF ? 1 : 2];      // SPLIT: the last ReLU's mask as the first backward product's B operand
    if constexpr (SPLIT) {
      decoder_fwd_split<F, H, NH, HALF, false, true>(img.s_fwd(), img.s_bias(), lane, f, mw, maskB, p0, p1, poison);
    } else {
      f32x16 buf[2][RT][2];
      {
        f32x16 bias[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
          for (int j = 0; j < 16; ++j) bias[r][j] = b0[32 * r + row_of(j, hi)];
#pragma unroll
        for (int s = 0; s < KS0; ++s) {
          float bt0, bt1 = 0.0f;
          if (HALF) {      // both halves hold the same point: k = 0 from the low half, k = 1 from the high one
            bt0 = hi ? f[2 * s + 1] : f[2 * s];
          } else {
            auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(f[2 * s]), __float_as_uint(f[2 * s + 1]), false, false);
            bt0 = __uint_as_float(sw[0]); bt1 = __uint_as_float(sw[1]);
          }
#pragma unroll
          for (int r = 0; r < RT; ++r) {
            float a = w0p[(s * 64 + lane) * RT + r];
            buf[0][r][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bt0, s == 0 ? bias[r] : buf[0][r][0], 0, 0, 0);
            if (!HALF) buf[0][r][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bt1, s == 0 ? bias[r] : buf[0][r][1], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        uint32_t m = 0;
#pragma unroll
        for (int t = 0; t < (HALF ? 1 : 2); ++t)
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            buf[0][r][t][j] = relu1(buf[0][r][t][j]);
            push_gt0(m, buf[0][r][t][j]);
          }
        mw[r] = HALF ? (m << 16) : m;      // (tile 0's bits at 31..16 either way: mask_bit)
      }
#pragma unroll
      for (int h = 0; h + 1 < NH; ++h) {
        const int ci = h & 1, ni = ci ^ 1;
        f32x16 bias[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
          for (int j = 0; j < 16; ++j) bias[r][j] = bh[h * H + 32 * r + row_of(j, hi)];
#pragma unroll
        for (int rp = 0; rp < RT; ++rp)
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const int ks = rp * 16 + j;
#pragma unroll
            for (int r = 0; r < RT; ++r) {
              float a = whp[((h * KS1 + ks) * 64 + lane) * RT + r];
              buf[ni][r][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, buf[ci][rp][0][j], ks == 0 ? bias[r] : buf[ni][r][0], 0, 0, 0);
              if (!HALF) buf[ni][r][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, buf[ci][rp][1][j], ks == 0 ? bias[r] : buf[ni][r][1], 0, 0, 0);
            }
          }
#pragma unroll
        for (int r = 0; r < RT; ++r) {
          uint32_t m = 0;
#pragma unroll
          for (int t = 0; t < (HALF ? 1 : 2); ++t)
#pragma unroll
            for (int j = 0; j < 16; ++j) {
              buf[ni][r][t][j] = relu1(buf[ni][r][t][j]);
              push_gt0(m, buf[ni][r][t][j]);
            }
          mw[(h + 1) * RT + r] = HALF ? (m << 16) : m;
        }
      }
      if (NH == 0) {
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            float wv = wo[32 * r + row_of(j, hi)];
            p0 += wv * buf[0][r][0][j];
            if (!HALF) p1 += wv * buf[0][r][1][j];
          }
      } else {
        constexpr int h = NH > 0 ? NH - 1 : 0, ci = h & 1;
#pragma unroll
        for (int r = 0; r < RT; ++r) {
          f32x16 a0, a1, bias;
#pragma unroll
          for (int j = 0; j < 16; ++j) bias[j] = bh[h * H + 32 * r + row_of(j, hi)];
#pragma unroll
          for (int rp = 0; rp < RT; ++rp)
#pragma unroll
            for (int j = 0; j < 16; ++j) {
              const int ks = rp * 16 + j;
              float a = whp[((h * KS1 + ks) * 64 + lane) * RT + r];
              a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, buf[ci][rp][0][j], ks == 0 ? bias : a0, 0, 0, 0);
              if (!HALF) a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, buf[ci][rp][1][j], ks == 0 ? bias : a1, 0, 0, 0);
            }
          uint32_t m = 0, m1 = 0;
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const float y0 = relu1(a0[j]), y1 = HALF ? 0.0f : relu1(a1[j]);
            push_gt0(m, y0);
            if (!HALF) push_gt0(m1, y1);
            float wv = wo[32 * r + row_of(j, hi)];
            p0 += wv * y0;
            if (!HALF) p1 += wv * y1;
          }
          mw[(h + 1) * RT + r] = (m << 16) | m1;
        }
      }
    }
    // decoder.hpp's close_fwd, written out: through the function (a HALF form of it, by value or by reference) between
    // 22 and 46 of this kernel's 78 instantiations changed registers past their first matrix instruction
    p0 += __shfl_xor(p0, 32);
    if (!HALF) p1 += __shfl_xor(p1, 32);
    const float sdf_v = SPLIT ? (((!HALF && hi) ? p1 : p0) + bo) + poison : ((!HALF && hi) ? p1 : p0) + bo;
    const bool mine = !(HALF && hi);      // HALF: the high half mirrors the low one -- stored / counted once
    if (valid && sdf && mine) sdf[po] = sdf_v;
    // ================================ loss: lane = point ============================================================
    float gl = 0.0f;
    if (valid && mine) {
      float gsd, gfs;
      map_loss_one(lin.p, sdf_v, l_in.x, l_in.w, l_in.y == 1.0f, lin.p.w_fs > 0.f && l_in.z == 1.0f, gsd, gfs,
                   loss_sdf, loss_fs);
      gl = (gsd + gfs) * inv_n;
    }
    // the backward works on two tiles of 32 points, lane (hi, c) on point 32 t + c of tile t
    float ds[2];
    ds[0] = __shfl(gl, lane & 31);
    ds[1] = HALF ? 0.0f : __shfl(gl, 32 + (lane & 31));
    // ================================ backward ======================================================================
    f32x16 df[2];
    if constexpr (SPLIT) {
      decoder_bwd_split<F, H, NH, HALF>(img.s_bwd(), lane, maskB, mw, ds, df);
    } else {
      f32x16 dbuf[2][RT][2];
#pragma unroll
      for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          float wv = wo[32 * r + row_of(j, hi)];
#pragma unroll
          for (int t = 0; t < (HALF ? 1 : 2); ++t) dbuf[0][r][t][j] = gate(wv * ds[t], mw[NH * RT + r], t, j);
        }
#pragma unroll
      for (int hh = 0; hh < NH; ++hh) {
        const int h = NH - 1 - hh;
        const int ci = hh & 1, ni = ci ^ 1;
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
          for (int j = 0; j < 16; ++j) { dbuf[ni][r][0][j] = 0.0f; if (!HALF) dbuf[ni][r][1][j] = 0.0f; }
#pragma unroll
        for (int rp = 0; rp < RT; ++rp)
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const int ks = rp * 16 + j;
#pragma unroll
            for (int r = 0; r < RT; ++r) {
              float a = whT[((h * KS1 + ks) * 64 + lane) * RT + r];
              dbuf[ni][r][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, dbuf[ci][rp][0][j], dbuf[ni][r][0], 0, 0, 0);
              if (!HALF) dbuf[ni][r][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, dbuf[ci][rp][1][j], dbuf[ni][r][1], 0, 0, 0);
            }
          }
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
          for (int t = 0; t < (HALF ? 1 : 2); ++t)
#pragma unroll
            for (int j = 0; j < 16; ++j) dbuf[ni][r][t][j] = gate(dbuf[ni][r][t][j], mw[h * RT + r], t, j);
      }
      f32x16 (&d)[RT][2] = dbuf[NH & 1];
#pragma unroll
      for (int j = 0; j < 16; ++j) { df[0][j] = 0.0f; if (!HALF) df[1][j] = 0.0f; }
#pragma unroll
      for (int rp = 0; rp < RT; ++rp)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          float a = w0T[(rp * 16 + j) * 64 + lane];
          df[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, d[rp][0][j], df[0], 0, 0, 0);
          if (!HALF) df[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, d[rp][1][j], df[1], 0, 0, 0);
        }
    }
    // ---- d-feat rows: accumulator layout -> LDS tile -> 64 contiguous rows of the (N, F) buffer, 16-B stores --------
    memory_phase(true);
    dfeat_to_tile<F, HALF ? 1 : 2>(df, dF, lane & 31, hi);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (!SCAT || dfeat_out) tile_to_rows<F, PTS>(dF, dfeat_out + chunk * PTS * F, n - chunk * PTS, lane);
    if (rotate && chunk + sched.step < sched.end) MISO_TRAIN_GATHER(chunk + sched.step, rec_nxt, p_n, po_n, valid_n, l_in_n)
    if (SCAT) scatter_tile<C, L, true, GridK>(g, scatter_mask, dF, rec_cur, PTS, lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();      // the next chunk overwrites the tile (and the records)
    memory_phase(false);
    if (rotate) { int* t_ = rec_cur; rec_cur = rec_nxt; rec_nxt = t_; }
  }
  // loss sums: as sdf_fwd_kernel (every block stores its pair into its own slot, the slots nobody owns are cleared)
  for (int o = 32; o > 0; o >>= 1) { loss_sdf += __shfl_down(loss_sdf, o); loss_fs += __shfl_down(loss_fs, o); }
  __syncthreads();
  if (lane == 0) { smem[2 * wave] = loss_sdf; smem[2 * wave + 1] = loss_fs; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = (smem[0] + smem[2]) + (smem[4] + smem[6]), b = (smem[1] + smem[3]) + (smem[5] + smem[7]);
    if (NW == 8) {
      a += (smem[8] + smem[10]) + (smem[12] + smem[14]);
      b += (smem[9] + smem[11]) + (smem[13] + smem[15]);
    }
    float2* slots = reinterpret_cast<float2*>(lin.loss_out);
    slots[blockIdx.x] = make_float2(lin.p.w_sdf * a * inv_n, lin.p.w_fs * b * inv_n);
    for (int sl = blockIdx.x + gridDim.x; sl < MISO_LOSS_SLOTS; sl += gridDim.x) slots[sl] = make_float2(0.f, 0.f);
  }
}

// ---------------------------------------------------------------------------
// host side: the launch is planned in one place (plan_train) and made in one place (launch_train_t)
// ---------------------------------------------------------------------------
// what the planner looks at beside the decoder shape
struct TrainCase {
  bool split;           // bf16x3 decoder (the exact fp32 pack is the smaller one)
  bool scat;            // some level is scattered from the kernel
  bool perm;            // the batch comes with a perm[] array
  bool binned;          // ... or is binned at all (perm[], or the index in xn[p].w)
  bool deferred;        // d-feat rows are written for the pull / push
  bool full_trips;      // MISO_F_FULL_TRIPS
  int64_t n;
};

struct TrainPlan {
  int wavefronts;       // per workgroup: 8 (one workgroup per CU) or 4 (two)
  bool half;            // 32-point trips
  bool rotate;          // two blocks of cell records per wavefront (the kernel's rotate_records)
  unsigned blocks;      // workgroups
  size_t lds_bytes;     // the pack, then per wavefront a d-feat tile [64][FP] and, scattering, its cell records [64][L][8]
};

static TrainPlan plan_train(int C, int L, int H, int NH, const TrainCase& c) {
  const PackLayout pl(C * L, H, NH);
  const int F = C * L, FP = dfeat_pitch(F), tile = 64 * FP, records = 64 * L * CELL_REC;
  const int pack = image_floats(pl, c.split, true);
  const auto bytes = [&](int wavefronts, int record_blocks) {
    return (size_t)(pack + wavefronts * (tile + record_blocks * records)) * sizeof(float);
  };
  const auto fits = [](size_t b) { return b <= MISO_LDS_LIMIT; };
  const auto at_most = [](int64_t v, int64_t cap) { return (unsigned)(v < cap ? v : cap); };
  const int64_t nchunks = (c.n + 63) / 64;
  const unsigned blocks8 = at_most((nchunks + 7) / 8, 256);      // persistent: one workgroup per CU
  // ... or two (256 .. 1024 measured: 512 and up equal), one loss slot per block
  const unsigned blocks4 = at_most((nchunks + 3) / 4, MISO_LOSS_SLOTS < 512 ? MISO_LOSS_SLOTS : 512);
  // Nothing scattered from the kernel (the mapping step): ONE workgroup of eight wavefronts per CU instead of two of
  // four -- the same two wavefronts per SIMD, half the copies of the 48 KB pack out of L2 at the start of the launch,
  // one barrier per CU (cfg-2: 72.9 -> 72.0 us, A/B in one process).
  if (!c.scat) return {8, false, false, blocks8, bytes(8, 0)};
  // Scattering: with room for a second block of cell records the kernel rotates its loop (feature rows up to
  // MISO_ROTATE_MAX_F floats).  Narrow rows of a binned batch (cfg-3's C = 4, L = 2): eight wavefronts and their two
  // record blocks each fit beside the pack, and the four-wavefront form is ONE workgroup per CU there (the bf16x3 pack
  // is 67 KB) -- one wavefront per SIMD.  Wide rows keep four wavefronts: their cell records would not fit beside eight
  // d-feat tiles.
  const bool may_rotate = F <= MISO_ROTATE_MAX_F;
  if (may_rotate && c.binned && fits(bytes(8, 2))) return {8, false, true, blocks8, bytes(8, 2)};
  const bool rotate = may_rotate && fits(bytes(4, 2));
  const size_t lds = bytes(4, rotate ? 2 : 1);
  // an unbinned batch of at most one 64-point chunk per SIMD (<= 65 536 samples): 32-point trips -- the batch is latency, not
  // throughput, and half the matrix chain per wavefront on twice the wavefronts is what shortens it
  if (!c.perm && !c.deferred && nchunks <= 1024 && !c.full_trips)
    return {4, true, rotate, at_most(((c.n + 31) / 32 + 3) / 4, MISO_LOSS_SLOTS), lds};
  return {4, false, rotate, blocks4, lds};
}

template <int C, int L, int H, int NH>
static hipError_t launch_train_t(FusedShape<C, L, H, NH>, const GridK& g, const float* packed, const float* x, int64_t n,
                                 float* sdf, const int* perm, const LossInK& lin, float* dfeat_out, uint32_t defer_mask,
                                 bool scat, hipStream_t s) {
  const bool split = use_split(g.flags & MISO_F_EXACT_F32);
  const TrainCase c = {split, scat, perm != nullptr, perm || (g.flags & MISO_F_INDEX_IN_XN), dfeat_out != nullptr,
                       (g.flags & MISO_F_FULL_TRIPS) != 0, n};
  const TrainPlan p = plan_train(C, L, H, NH, c);
  // sdf_train_kernel<C, L, H, NH, SCAT, NW, HALF, SPLIT>: the plan is eight wavefronts exactly where nothing is
  // scattered, or narrow rows are; four, in whole or half trips, for every other scattering launch
  void (*k)(GridK, const float*, const float*, int64_t, float*, const int*, LossInK, float*, uint32_t, bool) = nullptr;
  if (!scat) {
    k = split ? sdf_train_kernel<C, L, H, NH, false, 8, false, true> : sdf_train_kernel<C, L, H, NH, false, 8, false, false>;
  } else if (p.wavefronts == 8) {
    if constexpr (C * L <= MISO_ROTATE_MAX_F)      // (the plan names this form for such rows only)
      k = split ? sdf_train_kernel<C, L, H, NH, true, 8, false, true> : sdf_train_kernel<C, L, H, NH, true, 8, false, false>;
  } else if (p.half) {
    k = split ? sdf_train_kernel<C, L, H, NH, true, 4, true, true> : sdf_train_kernel<C, L, H, NH, true, 4, true, false>;
  } else {
    k = split ? sdf_train_kernel<C, L, H, NH, true, 4, false, true> : sdf_train_kernel<C, L, H, NH, true, 4, false, false>;
  }
  if (!k) return hipErrorInvalidValue;
  hipError_t e = allow_lds((const void*)k, p.lds_bytes);
  if (e != hipSuccess) return e;
  k<<<p.blocks, 64 * p.wavefronts, p.lds_bytes, s>>>(g, packed, x, n, sdf, perm, lin, dfeat_out, defer_mask, p.rotate);
  return hipGetLastError();
}

// dynamic LDS of the widest form of the sdf_train_kernel launch for this shape: the most plan_train asks for over both
// decoder forms and binned / unbinned batches; 0: the shape is not covered, or that form does not fit a workgroup
int64_t sdf_train_lds_bytes(int C, int L, int H, int NH, bool scat) {
  if (!fused_shape_supported(C, L, H, NH)) return 0;
  size_t most = 0;
  for (int split = 0; split < 2; ++split)
    for (int binned = 0; binned < 2; ++binned) {
      const TrainCase c = {split != 0, scat, binned != 0, binned != 0, binned != 0, false, (int64_t)1 << 20};
      const size_t lds = plan_train(C, L, H, NH, c).lds_bytes;
      if (lds > most) most = lds;
    }
  return most <= MISO_LDS_LIMIT ? (int64_t)most : 0;
}

// forward + mapping loss + decoder backward of a batch in one launch (sdf_train_kernel): d-feat rows for the levels in
// defer_mask (formed by the pull / push afterwards), float atomics for the other levels with a gradient (scat: there
// are such levels), loss slots; sdf (caller order) optional; perm == nullptr: an unbinned batch
hipError_t launch_sdf_train(int C, int L, int H, int NH, const GridK& g, const float* packed, const float* x,
                            int64_t n, float* sdf, const int* perm, const LossInK& lin, float* dfeat_out,
                            uint32_t defer_mask, bool scat, hipStream_t s) {
  if (n == 0) return hipSuccess;
  return with_fused_shape(C, L, H, NH, hipErrorInvalidValue, [&](auto shape) {
    return launch_train_t(shape, g, packed, x, n, sdf, perm, lin, dfeat_out, defer_mask, scat, s);
  });
}

}  // namespace miso

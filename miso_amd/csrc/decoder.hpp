// Frozen-decoder MLP (MLPNet: grid_opt/models/modules.py:11-32) on the matrix cores: the packed-weight layout shared by
// mlp_pack_kernel and every kernel that decodes, the register-level helpers of the ReLU / gate passes, and the decoder
// chains:
//   decoder_fwd_split / decoder_bwd_split   bf16x3 split products (mlp_split.hpp), the default arithmetic
//   decoder_fwd_exact / decoder_bwd_exact   exact fp32 chains, behind MISO_F_EXACT_F32
// Who runs them:       forward                                backward
//   sdf_fused.hip      sdf_fwd_kernel                         sdf_bwd_kernel
//   sdf_train.hip      sdf_train_kernel: the split chains (HALF: 32-point trips too); its exact chains are written out
//                      in the kernel -- through decoder_*_exact ten of its exact instantiations took 1 .. 28 VGPRs more
//                      and the step was 0.3 - 0.6 % slower (profiles/decoder_shared.json)
//   hash_sdf.hip       hash_sdf_fwd_kernel                    (sdf_bwd_kernel)
//   atlas_eval.hpp     AtlasDecoder (atlas.hip, trace.hip, hash_trace.hip)
//   atlas_bwd.hip      atlas_sdf_bwd_kernel                   the same kernel
//   pair_sdf.hip       pair_sdf_stage_kernel                  the same kernel
// Where the pack lies in LDS for them is said once, in PackImage below; the kernels that only query go through
// FwdDecoder and are launched by FwdLaunch.
// decoder_wgrad.hip keeps chains of its own: it holds every layer's activations and interleaves the outer products of the
// weight gradients, a different computation.  What happens to d feats behind a backward chain is in dfeat_tile.hpp.
#pragma once
#include "common.hpp"
#include "mlp_split.hpp"

namespace miso {

// On gfx950 the fp32 MFMA shares the vector FMA datapath (tools/ubench/mfma_valu.hip): every VALU
// instruction between two MFMAs costs matrix throughput, so the MLP phase is trimmed of them.
// * ReLU on the raw bits: max_i32(bits, 0) is ONE instruction and exact (negative floats, -0 included,
//   are negative integers); fmaxf(x, 0) costs two (a canonicalising v_max x,x first).
// * Sign bit for the backward from the ReLU output: min_u32(bits, 1) then shift-or -- two instructions
//   instead of compare + select + or.
// * The bias enters as the C operand of the first MFMA of each chain (no accumulator init moves).
// (Inline-asm variants were tried: the hazard recogniser does not see that the asm reads MFMA results,
//  and the missing wait states returned stale accumulators.)
__device__ __forceinline__ float relu1(float x) { return __int_as_float(max(__float_as_int(x), 0)); }
// y = relu1(x): bit <- (x > 0)
// The bits are SHIFTED IN (the k-th of 32 pushes ends at bit 31 - k): y's bits are a non-negative integer, so
// bit 31 of y + 0x7fffffff is (y != 0) and v_alignbit(m, that, 31) = (m << 1) | bit -- two instructions.  (min(y, 1)
// << k | m is canonicalised by the compiler into compare + select + or, with a wait state after every compare.)
__device__ __forceinline__ void push_gt0(uint32_t& m, float y) {
  m = __builtin_amdgcn_alignbit(m, __float_as_uint(y) + 0x7fffffffu, 31);
}
__device__ __forceinline__ bool mask_bit(uint32_t m, int t, int j) { return (m >> (31 - (t * 16 + j))) & 1u; }
// mask_bit ? x : 0 as v_bfe_i32 (the bit, sign-extended: 0 or ~0) + v_and -- the select form costs and + compare +
// select and a wait state per element
__device__ __forceinline__ float gate(float x, uint32_t m, int t, int j) {
  int e = __builtin_amdgcn_sbfe((int)m, 31 - (t * 16 + j), 1);
  asm("" : "+v"(e));      // opaque: and(x, sext(bit)) would be folded back into compare + select
  return __uint_as_float(__float_as_uint(x) & (uint32_t)e);
}

// acc += a b.  Left as a product and a sum (PIN_FMA = false), whether the two become one v_fma is up to the vectoriser
// and the contraction heuristics, which decide by the surrounding code: in sdf_fwd_kernel every one of them does.  A
// kernel that has to give sdf_fwd_kernel's bits from inside other code (atlas_eval.hpp: inlined into two kernels, at
// several places) asks for the fused form outright (PIN_FMA = true) in the gather and in the output dot product.
template <bool PIN_FMA>
__device__ __forceinline__ void mul_acc(float& acc, float a, float b) {
  if constexpr (PIN_FMA) acc = __builtin_fmaf(a, b, acc);
  else acc += a * b;
}

// lane-per-point trilinear gather of one level (channels-last rows of C floats, 16-B loads): f[0..C) = sum_k w_k v_k
template <int C, bool PIN_FMA = false>
__device__ __forceinline__ void gather_level(const LevelK& lv, const Cell& c, float* f) {
  // lane-per-point gather of one level: 8 corners x C channels, channels-last.
#pragma unroll
  for (int q = 0; q < C; ++q) f[q] = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const bool in = corner_in(c, k);
    const float w = corner_weight<0>(c, k, in).w;
    int off = in ? corner_offset(c, lv, k) : 0;      // (the weight before the offset: sdf_train_kernel's registers)
#ifdef MISO_ABL_UNIFORM_GATHER      // dev ablation (wrong results): every lane reads lane 0's rows -- perfectly coalesced gathers
    off = __builtin_amdgcn_readfirstlane(off);
#endif
#ifdef MISO_ABL_QUAD_GATHER         // dev ablation (wrong results): groups of four lanes read one lane's rows
    off = __builtin_amdgcn_mov_dpp(off, 0x00, 0xf, 0xf, true);
#endif
#pragma unroll
    for (int q = 0; q < C; q += 4) {
      float4 v = *reinterpret_cast<const float4*>(lv.data + off + q);
      mul_acc<PIN_FMA>(f[q + 0], v.x, w); mul_acc<PIN_FMA>(f[q + 1], v.y, w);
      mul_acc<PIN_FMA>(f[q + 2], v.z, w); mul_acc<PIN_FMA>(f[q + 3], v.w, w);
    }
  }
}


// ---------------------------------------------------------------------------
// Packed decoder layout (floats).  RT = H/32 row tiles, KS0 = ceil(F/2),
// KS1 = H/2 k-steps for an HxH layer, NH hidden (HxH) layers.
//   fwd: W0p [KS0][64][RT]   A(l) = W0[32r + (l&31)][2s + (l>>5)]
//        Whp [NH][KS1][64][RT] A(l) = Wh[32r + (l&31)][32rp + row_of(j, l>>5)], ks = 16rp + j
//        b0 [H], bh [NH][H], wo [H], bo [4]
//   bwd: WhTp [NH][KS1][64][RT] A(l) = Wh[32rp + row_of(j, l>>5)][32r + (l&31)]
//        W0Tp [KS1][64]         A(l) = W0[32rp + row_of(j, l>>5)][l&31]   (0 for l&31 >= F)
// Behind it (round 6), the same matrices as bf16x3 pieces for v_mfma_f32_32x32x16_bf16 (mlp_split.hpp; dword offsets,
// one block [kb][r][piece][64 lanes][4 dwords] per matrix, KB0 = ceil(F/16) and KBH = H/16 k-blocks):
//   forward:  s_w0  W0 rows 32r + (l&31), contraction split_k_feat;  s_wh [NH] Wh rows 32r + (l&31), contraction split_k_acc
//   backward: s_bfirst  the FIRST backward product with the output weights folded in -- its B operand is the last ReLU's
//                       0 / 1 mask, exact in one bf16 piece (three matrix instructions per k-block instead of six, nothing to
//                       split): NH >= 1: V[k][m] = fl(Wh[NH-1][m][k] wo[m]) (RT row tiles); NH == 0: U[f][m] = fl(W0[m][f] wo[m])
//             s_whT [NH-1]  Wh[h]^T, h = 0 .. NH-2;   s_w0T  W0^T (one row tile; NH >= 1 only)
// ---------------------------------------------------------------------------
struct PackLayout {
  int F, H, NH, RT, KS0, KS1;
  int o_w0, o_wh, o_b0, o_bh, o_wo, o_bo, fwd_end;
  int o_whT, o_w0T, total;
  int KB0, KBH;
  int s_w0, s_wh, s_fwd_end, s_bfirst, s_whT, s_w0T, total_all;
  __host__ __device__ PackLayout(int F_, int H_, int NH_) {
    F = F_; H = H_; NH = NH_; RT = H / 32; KS0 = (F + 1) / 2; KS1 = H / 2;
    int o = 0;
    o_w0 = o; o += KS0 * 64 * RT;
    o_wh = o; o += NH * KS1 * 64 * RT;
    o_b0 = o; o += H;
    o_bh = o; o += NH * H;
    o_wo = o; o += H;
    o_bo = o; o += 4;
    fwd_end = o;
    o_whT = o; o += NH * KS1 * 64 * RT;
    o_w0T = o; o += KS1 * 64;
    total = o;
    KB0 = (F + 15) / 16; KBH = H / 16;
    s_w0 = o; o += split_matrix_dwords(KB0, RT);
    s_wh = o; o += NH * split_matrix_dwords(KBH, RT);
    s_fwd_end = o;
    s_bfirst = o; o += split_matrix_dwords(KBH, NH >= 1 ? RT : 1);
    s_whT = o; o += (NH > 1 ? NH - 1 : 0) * split_matrix_dwords(KBH, RT);
    s_w0T = o; o += NH >= 1 ? split_matrix_dwords(KBH, 1) : 0;
    total_all = o;
  }
  __host__ __device__ int n_bias() const { return fwd_end - o_b0; }      // b0, bh, wo, bo: contiguous
};

// ---------------------------------------------------------------------------------------------------------------------
// The pack in LDS.  Two images, each in the two arithmetics:
//   forward  exact: the fp32 forward pack [0, fwd_end);  split: the bf16x3 forward block [s_w0, s_fwd_end), then the
//            biases and output weights [o_b0, fwd_end)
//   whole    exact: forward pack and transposed weights [0, total);  split: the bf16x3 section [s_w0, total_all), then
//            the biases and output weights
// (sdf_bwd_kernel has a backward-only image of its own, in sdf_fused.hip.)
// A kernel stages and addresses its image through PackImage; its launcher sizes the dynamic LDS with image_floats, and
// whatever lies behind the image (d-feat tiles, cell records, a pose partial) starts at that size on both sides.
__host__ __device__ inline int image_floats(const PackLayout& pl, bool split, bool whole) {
  return split ? (whole ? pl.total_all : pl.s_fwd_end) - pl.s_w0 + (pl.n_bias() + 3) / 4 * 4
               : ((whole ? pl.total : pl.fwd_end) + 3) / 4 * 4;
}

// The image lies at the start of the block's dynamic LDS -- this array, which the kernels declare under the same name.
// PackImage names it directly, not through a pointer it is handed: with the pointer as a member, the addresses of
// sdf_train_kernel's weight reads were formed differently and 65 of its 78 instantiations changed registers.
extern __shared__ __attribute__((aligned(16))) float smem[];

template <bool SPLIT, bool WHOLE>
struct PackImage {
  PackLayout pl;
  __device__ __forceinline__ PackImage(int F, int H, int NH) : pl(F, H, NH) {}
  __device__ __forceinline__ int n_split() const { return (WHOLE ? pl.total_all : pl.s_fwd_end) - pl.s_w0; }
  __device__ __forceinline__ int floats() const { return image_floats(pl, SPLIT, WHOLE); }
  __device__ __forceinline__ float* behind() const { return smem + floats(); }
  // the copy, by all threads of the block; no barrier: the caller may have more to write in front of it
  __device__ __forceinline__ void stage(const float* packed) const {
    if (SPLIT) {
      for (int i = threadIdx.x * 4; i < n_split(); i += blockDim.x * 4)
        *reinterpret_cast<float4*>(smem + i) = *reinterpret_cast<const float4*>(packed + pl.s_w0 + i);
      for (int i = threadIdx.x * 4; i < pl.n_bias(); i += blockDim.x * 4)
        *reinterpret_cast<float4*>(smem + n_split() + i) = *reinterpret_cast<const float4*>(packed + pl.o_b0 + i);
    } else {
      for (int i = threadIdx.x * 4; i < (WHOLE ? pl.total : pl.fwd_end); i += blockDim.x * 4)
        *reinterpret_cast<float4*>(smem + i) = *reinterpret_cast<const float4*>(packed + i);
    }
  }
  // exact: the fp32 pack at its PackLayout offsets
  __device__ __forceinline__ const float* w0p() const { return smem + pl.o_w0; }
  __device__ __forceinline__ const float* whp() const { return smem + pl.o_wh; }
  __device__ __forceinline__ const float* b0() const { return smem + pl.o_b0; }
  __device__ __forceinline__ const float* bh() const { return smem + pl.o_bh; }
  __device__ __forceinline__ const float* wo() const { return smem + pl.o_wo; }
  __device__ __forceinline__ const float* whT() const { return smem + pl.o_whT; }      // WHOLE
  __device__ __forceinline__ const float* w0T() const { return smem + pl.o_w0T; }      // WHOLE
  // split: decoder_fwd_split's sw and bias, decoder_bwd_split's sb
  __device__ __forceinline__ const uint32_t* s_fwd() const { return reinterpret_cast<const uint32_t*>(smem); }
  __device__ __forceinline__ const uint32_t* s_bwd() const { return s_fwd() + (pl.s_bfirst - pl.s_w0); }      // WHOLE
  __device__ __forceinline__ const float* s_bias() const { return smem + n_split(); }
  __device__ __forceinline__ float bo() const { return SPLIT ? s_bias()[pl.o_bo - pl.o_b0] : smem[pl.o_bo]; }
};

// ---------------------------------------------------------------------------------------------------------------------
// Split-precision chains.  NT = 1 (HALF: 32-point trips) or 2 point tiles per wavefront.
// One output row tile at a time (r outermost): its accumulators complete while the next row tile's products are still
// being issued, so the ReLU / split pass of row tile r runs beside the matrix instructions of row tile r + 1.
template <int KB, int NT>
__device__ __forceinline__ void mma_split_row(const uint32_t* __restrict__ A, int r, int RT, int lane,
                                              const Split3 (&B)[KB][NT], f32x16 (&acc)[NT], const f32x16& init) {
  constexpr int QA[6] = {2, 1, 0, 1, 0, 0};      // (piece of A, piece of B) in the order of accumulation: smallest first
  constexpr int QB[6] = {0, 1, 2, 0, 1, 0};
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    u32x4 a[3];
#pragma unroll
#ifdef MISO_ABL_NO_AREAD     // dev ablation (wrong results): no LDS reads of the weights
    for (int q = 0; q < 3; ++q) a[q] = u32x4{0x3f803f80u + (unsigned)lane, 0x3f803f80u, 0x3e803f80u, 0x3f803f00u + (unsigned)(kb + q)};
#else
    for (int q = 0; q < 3; ++q) a[q] = *reinterpret_cast<const u32x4*>(A + split_a_dword(kb, r, q, lane, RT));
#endif
#pragma unroll
    for (int c = 0; c < 6; ++c)
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[t] = mfma_bf16(a[QA[c]], B[kb][t].q[QB[c]], (kb == 0 && c == 0) ? init : acc[t]);
  }
}
// B exact in one piece (a 0 / 1 mask): the three pieces of A against it
template <int KB, int NT>
__device__ __forceinline__ void mma_mask_row(const uint32_t* __restrict__ A, int r, int RT, int lane,
                                             const u32x4 (&B)[KB][NT], f32x16 (&acc)[NT], const f32x16& init) {
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    u32x4 a[3];
#pragma unroll
#ifdef MISO_ABL_NO_AREAD
    for (int q = 0; q < 3; ++q) a[q] = u32x4{0x3f803f80u + (unsigned)lane, 0x3f803f80u, 0x3e803f80u, 0x3f803f00u + (unsigned)(kb + q)};
#else
    for (int q = 0; q < 3; ++q) a[q] = *reinterpret_cast<const u32x4*>(A + split_a_dword(kb, r, q, lane, RT));
#endif
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = mfma_bf16(a[2 - c], B[kb][t], (kb == 0 && c == 0) ? init : acc[t]);
  }
}

__device__ __forceinline__ f32x16 bias_block(const float* __restrict__ b, int r, int hi) {
  f32x16 v;
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = b[32 * r + row_of(j, hi)];
  return v;
}
__device__ __forceinline__ f32x16 zero_block() {
  f32x16 v;
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = 0.0f;
  return v;
}

// bf16 1.0 / 0.0 of (y > 0) for a ReLU output y (bits of a non-negative float; 0x3f80 as an integer is below every
// normal float's pattern), two elements per dword
__device__ __forceinline__ uint32_t mask_pair_bf16(float y0, float y1) {
  const uint32_t a = min(__float_as_uint(y0), 0x3f80u), b = min(__float_as_uint(y1), 0x3f80u);
  return a | (b << 16);
}
// the same dword from two adjacent sign bits of a mask word (bit position of element j: 31 - (16 t + j))
__device__ __forceinline__ uint32_t mask_pair_from_bits(uint32_t m, int t, int j) {
  const uint32_t b0 = (m >> (31 - (t * 16 + j))) & 1u, b1 = (m >> (31 - (t * 16 + j + 1))) & 1u;
  return (b0 ? 0x3f80u : 0u) | (b1 ? 0x3f800000u : 0u);
}

// Forward: lane-per-point feature rows f[0..F) -> partial output sums p0 (tile 0), p1 (tile 1) of this lane's 16 rows per row
// tile (the caller adds the two lane halves and the output bias).  mw: ReLU sign bits per layer and row tile (the layout
// of the exact kernels: word l*RT + r, tile t's element j at bit 31 - (16 t + j)); BITS_LAST = false leaves the last
// layer's words unwritten and MASKB = true returns the last ReLU's mask as the B operand of the first backward product.
//   sw: LDS, the pack's [s_w0, s_fwd_end) block;  bias: LDS, the pack's [o_b0, fwd_end) block (b0, bh, wo, bo)
template <int F, int H, int NH, bool HALF, bool BITS_LAST, bool MASKB, bool PIN_FMA = false, int FN = 0>
__device__ __forceinline__ void decoder_fwd_split(const uint32_t* __restrict__ sw, const float* __restrict__ bias, int lane,
                                                  const float (&f)[FN], uint32_t (&mw)[(NH + 1) * (H / 32)],
                                                  u32x4 (&maskB)[H / 16][HALF ? 1 : 2], float& p0, float& p1,
                                                  float& poison) {
  constexpr int RT = H / 32, KB0 = (F + 15) / 16, KBH = H / 16, NT = HALF ? 1 : 2;
  const int hi = lane >> 5;
  // A NaN among the features must come out as a NaN SDF (the trainers' NaN guards rely on it: trainer.py:205-211).  The
  // exact chains propagate it through their FMAs; here a NaN piece can leave the matrix core with its sign set, and the
  // integer ReLU would clear it.  So: 0 for a finite feature row, NaN otherwise, added to this lane's SDF by the caller.
  {
    float acc = f[0];
#pragma unroll
    for (int i = 1; i < F; ++i) acc += f[i];
    poison = acc - acc;
  }
  const float* b0 = bias;
  const float* bh = bias + H;
  const float* wo = bias + H + NH * H;
  // ---- feature rows -> B operand of layer 0: element i of k-block kb, lane half hi <-> feature 16 kb + 8 hi + i ---------
  Split3 B0[KB0][NT];
#pragma unroll
  for (int kb = 0; kb < KB0; ++kb) {
    auto fe = [&](int i) -> float { return (16 * kb + i < F) ? f[(16 * kb + i < FN) ? 16 * kb + i : 0] : 0.0f; };
    const Split3 lo = split8(fe(0), fe(1), fe(2), fe(3), fe(4), fe(5), fe(6), fe(7));
    Split3 up;
    if (16 * kb + 8 < F) up = split8(fe(8), fe(9), fe(10), fe(11), fe(12), fe(13), fe(14), fe(15));
    else {
#pragma unroll
      for (int q = 0; q < 3; ++q) up.q[q] = u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        if (HALF) {      // both lane halves hold the same point
          B0[kb][0].q[q][d] = hi ? up.q[q][d] : lo.q[q][d];
        } else {         // tile 0: (own low | low half's upper), tile 1: (high half's low | own upper)
          auto sw2 = __builtin_amdgcn_permlane32_swap(lo.q[q][d], up.q[q][d], false, false);
          B0[kb][0].q[q][d] = sw2[0];
          B0[kb][1].q[q][d] = sw2[1];
        }
      }
  }
  p0 = 0.0f; p1 = 0.0f;
  if constexpr (NH == 0) {
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      f32x16 acc[NT];
      mma_split_row<KB0, NT>(sw, r, RT, lane, B0, acc, bias_block(b0, r, hi));
      uint32_t m = 0, m1 = 0;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float y0 = relu1(acc[0][j]), y1 = HALF ? 0.0f : relu1(acc[NT - 1][j]);
        if (BITS_LAST) { push_gt0(m, y0); if (!HALF) push_gt0(m1, y1); }
        const float wv = wo[32 * r + row_of(j, hi)];
        mul_acc<PIN_FMA>(p0, wv, y0);
        if (!HALF) mul_acc<PIN_FMA>(p1, wv, y1);
        if (MASKB && (j & 1)) {
          maskB[2 * r + (j >> 3)][0][(j & 7) >> 1] = mask_pair_bf16(relu1(acc[0][j - 1]), y0);
          if (!HALF) maskB[2 * r + (j >> 3)][NT - 1][(j & 7) >> 1] = mask_pair_bf16(relu1(acc[NT - 1][j - 1]), y1);
        }
      }
      if (BITS_LAST) mw[r] = (m << 16) | m1;
    }
  } else {
    // ---- layer 0 -------------------------------------------------------------------------------------------------
    Split3 Bh[KBH][NT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      f32x16 acc[NT];
      mma_split_row<KB0, NT>(sw, r, RT, lane, B0, acc, bias_block(b0, r, hi));
      uint32_t m = 0;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int j = 0; j < 16; ++j) { acc[t][j] = relu1(acc[t][j]); push_gt0(m, acc[t][j]); }
      mw[r] = HALF ? (m << 16) : m;
#pragma unroll
      for (int t = 0; t < NT; ++t) { Bh[2 * r][t] = split_acc<0>(acc[t]); Bh[2 * r + 1][t] = split_acc<1>(acc[t]); }
    }
    const uint32_t* swh = sw + split_matrix_dwords(KB0, RT);
    // ---- hidden layers but the last ----------------------------------------------------------------------------------
#pragma unroll
    for (int h = 0; h + 1 < NH; ++h) {
      Split3 Bn[KBH][NT];
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        f32x16 acc[NT];
        mma_split_row<KBH, NT>(swh + h * split_matrix_dwords(KBH, RT), r, RT, lane, Bh, acc, bias_block(bh + h * H, r, hi));
        uint32_t m = 0;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int j = 0; j < 16; ++j) { acc[t][j] = relu1(acc[t][j]); push_gt0(m, acc[t][j]); }
        mw[(h + 1) * RT + r] = HALF ? (m << 16) : m;
#pragma unroll
        for (int t = 0; t < NT; ++t) { Bn[2 * r][t] = split_acc<0>(acc[t]); Bn[2 * r + 1][t] = split_acc<1>(acc[t]); }
      }
#pragma unroll
      for (int kb = 0; kb < KBH; ++kb)
#pragma unroll
        for (int t = 0; t < NT; ++t) Bh[kb][t] = Bn[kb][t];
    }
    // ---- last hidden layer + output layer (out_dim = 1): reduced row tile by row tile -----------------------------------
    constexpr int h = NH - 1;
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      f32x16 acc[NT];
      mma_split_row<KBH, NT>(swh + h * split_matrix_dwords(KBH, RT), r, RT, lane, Bh, acc, bias_block(bh + h * H, r, hi));
      uint32_t m = 0, m1 = 0;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float y0 = relu1(acc[0][j]), y1 = HALF ? 0.0f : relu1(acc[NT - 1][j]);
        if (BITS_LAST) { push_gt0(m, y0); if (!HALF) push_gt0(m1, y1); }
        const float wv = wo[32 * r + row_of(j, hi)];
        mul_acc<PIN_FMA>(p0, wv, y0);
        if (!HALF) mul_acc<PIN_FMA>(p1, wv, y1);
        if (MASKB && (j & 1)) {
          maskB[2 * r + (j >> 3)][0][(j & 7) >> 1] = mask_pair_bf16(relu1(acc[0][j - 1]), y0);
          if (!HALF) maskB[2 * r + (j >> 3)][NT - 1][(j & 7) >> 1] = mask_pair_bf16(relu1(acc[NT - 1][j - 1]), y1);
        }
      }
      if (BITS_LAST) mw[(h + 1) * RT + r] = (m << 16) | m1;
    }
  }
}

// the last ReLU's mask as a B operand, from its sign-bit words (the backward kernel; the training kernel forms it directly)
template <int H, int NH, bool HALF>
__device__ __forceinline__ void mask_operand_from_bits(const uint32_t (&mw)[(NH + 1) * (H / 32)],
                                                       u32x4 (&maskB)[H / 16][HALF ? 1 : 2]) {
  constexpr int RT = H / 32, NT = HALF ? 1 : 2;
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 16; j += 2)
        maskB[2 * r + (j >> 3)][t][(j & 7) >> 1] = mask_pair_from_bits(mw[NH * RT + r], t, j);
}

// Backward: d sdf of the wavefront's two point tiles (ds[t]: lane (hi, c) <-> point 32 t + c) -> d feats in accumulator
// layout df[t] (row = feature row_of(j, hi), see sdf_bwd_kernel).  sb: LDS, the pack's [s_bfirst, total_all) block.
template <int F, int H, int NH, bool HALF>
__device__ __forceinline__ void decoder_bwd_split(const uint32_t* __restrict__ sb, int lane,
                                                  const u32x4 (&maskB)[H / 16][HALF ? 1 : 2],
                                                  const uint32_t (&mw)[(NH + 1) * (H / 32)], const float (&ds)[2],
                                                  f32x16 (&df)[2]) {
  constexpr int RT = H / 32, KBH = H / 16, NT = HALF ? 1 : 2;
  if constexpr (NH == 0) {
    f32x16 acc[NT];
    mma_mask_row<KBH, NT>(sb, 0, 1, lane, maskB, acc, zero_block());
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 16; ++j) df[t][j] = acc[t][j] * ds[t];
  } else {
    Split3 Bd[KBH][NT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      f32x16 acc[NT];
      mma_mask_row<KBH, NT>(sb, r, RT, lane, maskB, acc, zero_block());
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[t][j] = gate(acc[t][j], mw[(NH - 1) * RT + r], t, j);
#pragma unroll
      for (int t = 0; t < NT; ++t) { Bd[2 * r][t] = split_acc<0>(acc[t]); Bd[2 * r + 1][t] = split_acc<1>(acc[t]); }
    }
    const uint32_t* swhT = sb + split_matrix_dwords(KBH, RT);
#pragma unroll
    for (int hh = 1; hh < NH; ++hh) {
      const int h = NH - 1 - hh;      // the product with Wh[h]^T, gated by layer h's ReLU
      Split3 Bn[KBH][NT];
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        f32x16 acc[NT];
        mma_split_row<KBH, NT>(swhT + h * split_matrix_dwords(KBH, RT), r, RT, lane, Bd, acc, zero_block());
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int j = 0; j < 16; ++j) acc[t][j] = gate(acc[t][j], mw[h * RT + r], t, j);
#pragma unroll
        for (int t = 0; t < NT; ++t) { Bn[2 * r][t] = split_acc<0>(acc[t]); Bn[2 * r + 1][t] = split_acc<1>(acc[t]); }
      }
#pragma unroll
      for (int kb = 0; kb < KBH; ++kb)
#pragma unroll
        for (int t = 0; t < NT; ++t) Bd[kb][t] = Bn[kb][t];
    }
    const uint32_t* sw0T = swhT + (NH - 1) * split_matrix_dwords(KBH, RT);
    f32x16 acc[NT];
    mma_split_row<KBH, NT>(sw0T, 0, 1, lane, Bd, acc, zero_block());
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 16; ++j) df[t][j] = acc[t][j] * ds[t];
  }
}

// A lane index the compiler takes for a new value at this point, for decoder_bwd_exact inside sdf_bwd_kernel's chunk
// loop.  The chain forms every LDS address of its weights from `lane`; given the kernel's own lane index, those addresses
// (one per k-step and output-weight row) are hoisted out of the loop and stay live across it: sdf_bwd_kernel<4, 4, 64, 1,
// true, false, false> then takes 211 VGPRs (205 with the chain written out in the kernel), 170 with kept_in_loop(lane),
// where the addresses are one base register and immediate offsets (profiles/decoder_shared.json lists every shape).
// sdf_fwd_kernel and the atlas kernels pass their lane index as it is: they called these chains before there was a
// kept_in_loop, their registers are what they were, and with it their instruction streams would change for no gain.
__device__ __forceinline__ int kept_in_loop(int lane) {
  asm volatile("" : "+v"(lane));
  return lane;
}

// The exact fp32 chains of the forward (v_mfma_f32_32x32x2_f32, behind MISO_F_EXACT_F32; the accumulators of a layer ARE the
// next layer's B operand: sdf_fused.hip's header).  w0p / whp / b0 / bh / wo: the fp32 pack's forward part in LDS.  Same outputs as decoder_fwd_split (p0 / p1: this lane's partial output sums).
template <int F, int H, int NH, bool PIN_FMA = false, int FN = 0>
__device__ __forceinline__ void decoder_fwd_exact(const float* __restrict__ w0p, const float* __restrict__ whp,
                                                  const float* __restrict__ b0, const float* __restrict__ bh,
                                                  const float* __restrict__ wo, int lane, const float (&f)[FN],
                                                  uint32_t (&mw)[(NH + 1) * (H / 32)], float& p0, float& p1) {
  constexpr int RT = H / 32, KS0 = (F + 1) / 2, KS1 = H / 2;
  const int hi = lane >> 5;
  // ---- layer 0: buf[0][r][t] = b0 + W0 * feats -------------------------------
  // Two accumulator sets ping-pong between layers (ReLU is applied in place, so
  // no third copy of the 64 activation registers is ever live).
  f32x16 buf[2][RT][2];
  {
    // the bias enters as the C operand of the first MFMA of each chain (one register block per
    // row tile, shared by both point tiles): no accumulator initialisation moves
    f32x16 bias[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int j = 0; j < 16; ++j) bias[r][j] = b0[32 * r + row_of(j, hi)];
#pragma unroll
    for (int s = 0; s < KS0; ++s) {
      auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(f[2 * s]), __float_as_uint(f[2 * s + 1]),
                                                 false, false);
      float bt0 = __uint_as_float(sw[0]), bt1 = __uint_as_float(sw[1]);
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        float a = w0p[(s * 64 + lane) * RT + r];
        buf[0][r][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bt0, s == 0 ? bias[r] : buf[0][r][0], 0, 0, 0);
        buf[0][r][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bt1, s == 0 ? bias[r] : buf[0][r][1], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    uint32_t m = 0;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        buf[0][r][t][j] = relu1(buf[0][r][t][j]);
        push_gt0(m, buf[0][r][t][j]);
      }
    mw[r] = m;
  }
  // ---- hidden HxH layers but the last ----------------------------------------------
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
          buf[ni][r][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, buf[ci][rp][1][j], ks == 0 ? bias[r] : buf[ni][r][1], 0, 0, 0);
        }
      }
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      uint32_t m = 0;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          buf[ni][r][t][j] = relu1(buf[ni][r][t][j]);
          push_gt0(m, buf[ni][r][t][j]);
        }
      mw[(h + 1) * RT + r] = m;
    }
  }
  // ---- last hidden layer + output layer (out_dim = 1), one 32-row tile at a time ----------
  // The last hidden activations feed only the output dot product, so each row tile is reduced
  // into (p0, p1) as soon as its MFMA chain ends: 32 accumulator registers live instead of 64.
  if (NH == 0) {
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        float wv = wo[32 * r + row_of(j, hi)];
        mul_acc<PIN_FMA>(p0, wv, buf[0][r][0][j]);
        mul_acc<PIN_FMA>(p1, wv, buf[0][r][1][j]);
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
          a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, buf[ci][rp][1][j], ks == 0 ? bias : a1, 0, 0, 0);
        }
      uint32_t m = 0, m1 = 0;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float y0 = relu1(a0[j]), y1 = relu1(a1[j]);
        push_gt0(m, y0);
        push_gt0(m1, y1);
        float wv = wo[32 * r + row_of(j, hi)];
        mul_acc<PIN_FMA>(p0, wv, y0);
        mul_acc<PIN_FMA>(p1, wv, y1);
      }
      mw[(h + 1) * RT + r] = (m << 16) | m1;
    }
  }
}

// The exact fp32 chains of the backward: d sdf of the two point tiles (ds[t]) -> d feats in
// accumulator layout, gated by the sign words mw of decoder_fwd_exact.  whT / w0T / wo: the fp32 pack's transposed weights
// and output weights in LDS.  Same outputs as decoder_bwd_split.
template <int F, int H, int NH>
__device__ __forceinline__ void decoder_bwd_exact(const float* __restrict__ whT, const float* __restrict__ w0T,
                                                  const float* __restrict__ wo, int lane,
                                                  const uint32_t (&mw)[(NH + 1) * (H / 32)], const float (&ds)[2],
                                                  f32x16 (&df)[2]) {
  constexpr int RT = H / 32, KS1 = H / 2;
  const int hi = lane >> 5;
  f32x16 dbuf[2][RT][2];      // two accumulator sets ping-pong
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float wv = wo[32 * r + row_of(j, hi)];
#pragma unroll
      for (int t = 0; t < 2; ++t) dbuf[0][r][t][j] = gate(wv * ds[t], mw[NH * RT + r], t, j);
    }
#pragma unroll
  for (int hh = 0; hh < NH; ++hh) {
    const int h = NH - 1 - hh;
    const int ci = hh & 1, ni = ci ^ 1;
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int j = 0; j < 16; ++j) { dbuf[ni][r][0][j] = 0.0f; dbuf[ni][r][1][j] = 0.0f; }
#pragma unroll
    for (int rp = 0; rp < RT; ++rp)
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int ks = rp * 16 + j;
#pragma unroll
        for (int r = 0; r < RT; ++r) {
          const float a = whT[((h * KS1 + ks) * 64 + lane) * RT + r];
          dbuf[ni][r][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, dbuf[ci][rp][0][j], dbuf[ni][r][0], 0, 0, 0);
          dbuf[ni][r][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, dbuf[ci][rp][1][j], dbuf[ni][r][1], 0, 0, 0);
        }
      }
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 16; ++j) dbuf[ni][r][t][j] = gate(dbuf[ni][r][t][j], mw[h * RT + r], t, j);
  }
  f32x16 (&d)[RT][2] = dbuf[NH & 1];
  // d feats = W0^T d   (one 32-row tile; rows >= F are zero)
#pragma unroll
  for (int j = 0; j < 16; ++j) { df[0][j] = 0.0f; df[1][j] = 0.0f; }
#pragma unroll
  for (int rp = 0; rp < RT; ++rp)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float a = w0T[(rp * 16 + j) * 64 + lane];
      df[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, d[rp][0][j], df[0], 0, 0, 0);
      df[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, d[rp][1][j], df[1], 0, 0, 0);
    }
}

// The closing of a forward chain: the two lane halves' partial sums added, this lane's tile chosen, then the output bias
// and, after a split chain, its poison term -- in this order, a rounding each.  (No HALF form: its one user would be
// sdf_train_kernel, which keeps these lines written out -- see there.)
template <bool SPLIT>
__device__ __forceinline__ float close_fwd(float p0, float p1, int hi, float bo, float poison) {
  p0 += __shfl_xor(p0, 32);
  p1 += __shfl_xor(p1, 32);
  const float p = hi ? p1 : p0;
  return SPLIT ? (p + bo) + poison : p + bo;
}

// The forward decoder of the kernels that only query: the forward image in LDS and the chain on one feature row per
// lane.  decode() holds matrix instructions and a cross-lane exchange: every lane of the wavefront must call it (full
// EXEC).  PIN_FMA: mul_acc's fused form in the output dot product, for code that is inlined into several kernels and
// has to give sdf_fwd_kernel's bits in each.
template <int F, int H, int NH, bool SPLIT, bool PIN_FMA>
struct FwdDecoder {
  static constexpr int RT = H / 32, KS0 = (F + 1) / 2, NF = 2 * KS0, MW = (NH + 1) * RT;
  PackImage<SPLIT, false> img;
  int lane, hi;
  float bo = 0.0f;

  // stages (all threads of the block) and ends in a barrier; staged = false: a feature-only query, nothing to decode
  __device__ __forceinline__ FwdDecoder(const float* __restrict__ packed, bool staged = true)
      : img(F, H, NH) {
    if (staged) img.stage(packed);
    __syncthreads();
    lane = threadIdx.x & 63;
    hi = lane >> 5;
    if (staged) bo = img.bo();
  }

  // f -> SDF; mw receives the ReLU sign words (BITS = false: a split chain leaves the last layer's unwritten)
  template <bool BITS>
  __device__ __forceinline__ float decode(const float (&f)[NF], uint32_t (&mw)[MW]) const {
    float p0 = 0.0f, p1 = 0.0f, poison = 0.0f;
    if constexpr (SPLIT) {
      u32x4 no_mask[H / 16][2];
      decoder_fwd_split<F, H, NH, false, BITS, false, PIN_FMA>(img.s_fwd(), img.s_bias(), lane, f, mw, no_mask, p0, p1, poison);
    } else {
      decoder_fwd_exact<F, H, NH, PIN_FMA>(img.w0p(), img.whp(), img.b0(), img.bh(), img.wo(), lane, f, mw, p0, p1);
    }
    return close_fwd<SPLIT>(p0, p1, hi, bo, poison);
  }
};

// Launch shape of the kernels that run a FwdDecoder: dynamic LDS for the forward image (`staged` = false: a feature-only
// query, which stages nothing) and a persistent grid of four wavefronts per block, one per 64 points at a time, `cap`
// blocks at the most.
struct FwdLaunch {
  size_t lds;
  unsigned blocks;
  FwdLaunch(int F, int H, int NH, bool split, int64_t n, unsigned cap, bool staged = true) {
    lds = staged ? (size_t)image_floats(PackLayout(F, H, NH), split, false) * sizeof(float) : 16;
    const int64_t nchunks = (n + 63) / 64;
    blocks = (unsigned)((nchunks + 3) / 4);
    if (blocks > cap) blocks = cap;
  }
};

}  // namespace miso

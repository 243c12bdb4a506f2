// Fused SDF alignment residual of the pairs of one alignment iteration: value and pose cotangents in one pass.
//
// Reference: pairwise_loss_sdf, grid_opt/align/miso.py:14-113 -- per iteration and pair a dataset draw, a per-keyframe
// loop with a host read-back, two nonzero compactions, the encode + decoder forward of both submaps and autograd back
// through the destination's -- and, with the measured SDF as the target, the inter-map loss of Vox-Fusion++
// (grid_opt/align/vfpp.py).  The source side depends on no optimised pose (sub_from(coords_from) reads the
// keyframe-in-submap poses only), so the caller stages it once: rows p_i in the source frame and their target ref_i.
// Here, one wavefront per 64 rows (lane = row), per row
//     w_i = R_s p_i + t_s ;  q_i = R_d^T (w_i - t_d) ;  m_i = q_i in bound(dst)        (src_to_dst, pair_stage.hpp)
//     s_i = decoder(encode_dst(q_i))   and   grad_q s_i:  decoder forward with its ReLU signs kept, decoder backward of
//           d s = 1 to d feat (decoder.hpp, dfeat_tile.hpp), the corner loop for d q (trilinear.hpp) -- steps 1-2 and the
//           x branch of step 3 of atlas_sdf_bwd_kernel, for one submap
//     r_i = ref_i - s_i ;  term_i = r^2 (L2) | |r| (L1) | w r^2 with w = c / (c + r^2)^2 held constant (GM)
//     g_i = (d term_i / d s_i) grad_q s_i
// and reduces the 24 doubles of miso_pair_latent -- sum term, sum m, sum g, sum (w - t_d) g^T, sum (R_d g) p^T -- as
// pair_latent.hip does: fp32 per lane, the wavefront by a shuffle tree, then in double across the workgroup and by fp64
// atomics across workgroups.  align_epilogue_a_kernel takes them from there.
// The decoder holds matrix instructions and a cross-lane exchange: every lane runs it (full EXEC); out-of-bound lanes and
// tail lanes feed it a zero row and their result is dropped.  A wavefront with no in-bound lane leaves before the
// decoder (wave-uniform), and so does one whose 64 rows' box (miso_align_src_boxes) cannot reach the destination bound.
#include "sdf_fused.hpp"
#include "pair_stage.hpp"

namespace miso {

constexpr int PAIR_SDF_WAVES = 4;

// KIND: 0 the SDF residuals above; the projected match of MIPS-Fusion (grid_opt/align/mips.py, miso_align_t.residual 3):
// 1 point-to-plane, 2 point-to-point.  With g = grad_q s held constant and the projected point q - s g mapped back to the
// source frame, p - match_src = s M^T g, M = Rd^T Rs (the rest of the reference's expression is p - p):
//   plane   a = g . (M n), n = the source normal of the row (feats_src, pitch ld); term (s a)^2; cotangent to q
//           2 s a^2 g; and, M standing in a explicitly, d term / d M = 2 s^2 a g n^T, summed as S2 (9 more accumulators)
//           and folded into the two 3x3 blocks in the fp64 tail: R_s S2^T to d / d R_d, R_d S2 to d / d R_s
//   point   term s^2 |g|^2 (the mean is over 3 count elements: n_ch = 3 in the plan); cotangent to q 2 s |g|^2 g; the
//           dependence of |M^T g|^2 on M is normal to the rotation manifold and is not summed
template <int C, int L, int H, int NH, bool SPLIT, int KIND>
__global__ __launch_bounds__(64 * PAIR_SDF_WAVES) void pair_sdf_stage_kernel(
    const AlignPairK* __restrict__ plan, const float* __restrict__ pose_all, int loss_type, float gm_scale,
    const float* __restrict__ packed, double* __restrict__ out_all, const int32_t* __restrict__ stopped,
    const int32_t* __restrict__ order) {
  constexpr int F = C * L, RT = H / 32, KS0 = (F + 1) / 2, NF = 2 * KS0, MW = (NH + 1) * RT;
  constexpr int FP = dfeat_pitch(F);
  constexpr int NACC = KIND == 1 ? 23 : 14;
  if (stopped && *stopped) return;
  // launch slot blockIdx.y -> pair, as in pair_stage_kernel
  const int o_ = order ? order[blockIdx.y] : 0;
  const unsigned pair = o_ > 0 ? (unsigned)(o_ - 1) : blockIdx.y;
  const AlignPairK& d = plan[pair];
  const int64_t n = d.n;
  if ((int64_t)blockIdx.x * blockDim.x >= n) return;      // (the whole workgroup: before any barrier)
  const GridK& g = d.g;
  double* out = out_all + 24 * pair;
  const float* pose_s = pose_all + 12 * d.src;
  const float* pose_d = pose_all + 12 * d.dst;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  const PackImage<SPLIT, true> img(F, H, NH);      // the whole pack (decoder.hpp)
  img.stage(packed);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hi = lane >> 5;
  const int nw = blockDim.x >> 6;
  const float bo = img.bo();
  float* dF = img.behind() + wave * (64 * FP);      // this wavefront's d-feat tile [64][FP]

  float Rs[9], ts[3], Rd[9], td[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) { Rs[i] = pose_s[i]; Rd[i] = pose_d[i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) { ts[i] = pose_s[9 + i]; td[i] = pose_d[9 + i]; }
  const float bmin[3] = {g.bmin[0], g.bmin[1], g.bmin[2]}, bmax[3] = {g.bmax[0], g.bmax[1], g.bmax[2]};
  // the composed map q = M p + q_0 and the slack of the box cull: pair_latent_body's, where the reasons are given
  float M[3][4];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    M[a][0] = Rd[a] * Rs[0] + Rd[3 + a] * Rs[3] + Rd[6 + a] * Rs[6];
    M[a][1] = Rd[a] * Rs[1] + Rd[3 + a] * Rs[4] + Rd[6 + a] * Rs[7];
    M[a][2] = Rd[a] * Rs[2] + Rd[3 + a] * Rs[5] + Rd[6 + a] * Rs[8];
    M[a][3] = Rd[a] * (ts[0] - td[0]) + Rd[3 + a] * (ts[1] - td[1]) + Rd[6 + a] * (ts[2] - td[2]);
  }
  const float slack = BOX_SLACK + 4e-6f * (fabsf(ts[0]) + fabsf(ts[1]) + fabsf(ts[2]) + fabsf(td[0]) + fabsf(td[1]) + fabsf(td[2])) +
                      1e-5f * (fmaxf(fabsf(bmin[0]), fabsf(bmax[0])) + fmaxf(fabsf(bmin[1]), fabsf(bmax[1])) +
                               fmaxf(fabsf(bmin[2]), fabsf(bmax[2])));

  // per lane: {term, in-bound count, G = sum g (3), S = sum p (x) g (9)}; the two 3x3 sums of the output are linear in S
  // and G and are formed once per workgroup in double (pair_latent_body).  KIND 1: then S2 = sum 2 s^2 a g (x) n (9)
  float acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.0f;

  static_assert(ALIGN_BOX_VERTS == 64, "one box per wavefront and chunk");
  const int64_t nchunks = (n + 63) / 64;
  for (int64_t chunk = (int64_t)blockIdx.x * nw + wave; chunk < nchunks; chunk += (int64_t)gridDim.x * nw) {
    asm volatile("" ::: "memory");      // (keeps the LDS reads of weights / biases inside the loop: sdf_fwd_kernel)
    if (d.boxes) {      // (wave-uniform) the chunk's box in the destination frame against the bound widened by the slack
      const float* bb = d.boxes + chunk * 6;
      const float c[3] = {0.5f * (bb[0] + bb[3]), 0.5f * (bb[1] + bb[4]), 0.5f * (bb[2] + bb[5])};
      const float e[3] = {0.5f * (bb[3] - bb[0]), 0.5f * (bb[4] - bb[1]), 0.5f * (bb[5] - bb[2])};
      bool outside = false;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float qc = M[a][0] * c[0] + M[a][1] * c[1] + M[a][2] * c[2] + M[a][3];
        const float r = fabsf(M[a][0]) * e[0] + fabsf(M[a][1]) * e[1] + fabsf(M[a][2]) * e[2] + slack +
                        1e-6f * (fabsf(qc) + fabsf(M[a][3]));
        outside = outside || qc - r > bmax[a] || qc + r < bmin[a];
      }
      if (__all(outside)) continue;
    }
    const int64_t i = chunk * 64 + lane;
    const bool valid = i < n;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (valid) { px = d.p[i * 3 + 0]; py = d.p[i * 3 + 1]; pz = d.p[i * 3 + 2]; }
    float dd[3], q[3];
    src_to_dst(Rs, ts, Rd, td, px, py, pz, dd, q);
    const bool inb = valid && q[0] >= bmin[0] && q[0] <= bmax[0] && q[1] >= bmin[1] && q[1] <= bmax[1] &&
                     q[2] >= bmin[2] && q[2] <= bmax[2];
    if (!__any(inb)) continue;      // (wave-uniform)
    // ================================ encode + decoder forward, ReLU signs kept =====================================
    float f[NF];
#pragma unroll
    for (int k = 0; k < NF; ++k) f[k] = 0.0f;
    if (inb) {
#pragma unroll
      for (int l = 0; l < L; ++l) {
        if ((g.ignore_mask >> l) & 1u) continue;      // zeros: utils.py:160-163
        const LevelK lv = g.lv[l];
        Axis ax[3];
        const Cell c = level_cell(g, lv, q[0], q[1], q[2], ax);
        float fl[C];
        gather_level<C, true>(lv, c, fl);
#pragma unroll
        for (int k = 0; k < C; ++k) f[l * C + k] = fl[k];
      }
    }
    uint32_t mw[MW];
    u32x4 maskB[H / 16][2];      // SPLIT: the last ReLU's mask as the first backward product's B operand
    float p0 = 0.0f, p1 = 0.0f, poison = 0.0f;
    if constexpr (SPLIT) decoder_fwd_split<F, H, NH, false, false, true, true>(img.s_fwd(), img.s_bias(), lane, f, mw, maskB, p0, p1, poison);
    else decoder_fwd_exact<F, H, NH, true>(img.w0p(), img.whp(), img.b0(), img.bh(), img.wo(), lane, f, mw, p0, p1);
    const float sdf = close_fwd<SPLIT>(p0, p1, hi, bo, poison);
    // ================================ decoder backward of d s = 1 ====================================================
    const float ds[2] = {1.0f, 1.0f};
    f32x16 df[2];
    if constexpr (SPLIT) decoder_bwd_split<F, H, NH, false>(img.s_bwd(), lane, maskB, mw, ds, df);
    else decoder_bwd_exact<F, H, NH>(img.whT(), img.w0T(), img.wo(), lane, mw, ds, df);
    dfeat_to_tile<F, 2>(df, dF, lane & 31, hi);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (inb) {
      float dfe[F];
#pragma unroll
      for (int k = 0; k < F; k += 4) {
        const float4 v = *reinterpret_cast<const float4*>(dF + lane * FP + k);
        dfe[k] = v.x; dfe[k + 1] = v.y; dfe[k + 2] = v.z; dfe[k + 3] = v.w;
      }
      // ---- d s / d q: the corner loop of atlas_sdf_bwd_kernel's x branch, lane = row -------------------------------
      float dq[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int l = 0; l < L; ++l) {
        if ((g.ignore_mask >> l) & 1u) continue;
        const LevelK lv = g.lv[l];
        Axis ax[3];
        const Cell c = level_cell(g, lv, q[0], q[1], q[2], ax);
        float sx_ = 0.f, sy_ = 0.f, sz_ = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
          if (!(c.inx[dx] && c.iny[dy] && c.inz[dz])) continue;
          const int off = (c.k0 + dz) * lv.sZ + (c.j0 + dy) * lv.sY + (c.i0 + dx) * lv.sX;
          float dot = 0.f;
#pragma unroll
          for (int ch = 0; ch < C; ch += 4) {
            const float4 gv = *reinterpret_cast<const float4*>(lv.data + off + ch);
            dot += gv.x * dfe[l * C + ch] + gv.y * dfe[l * C + ch + 1] + gv.z * dfe[l * C + ch + 2] + gv.w * dfe[l * C + ch + 3];
          }
          const float sx = dx ? 1.f : -1.f, sy = dy ? 1.f : -1.f, sz = dz ? 1.f : -1.f;
          sx_ += dot * sx * c.wy[dy] * c.wz[dz];
          sy_ += dot * sy * c.wx[dx] * c.wz[dz];
          sz_ += dot * sz * c.wx[dx] * c.wy[dy];
        }
        dq[0] += sx_ * ax[0].mult;
        dq[1] += sy_ * ax[1].mult;
        dq[2] += sz_ * ax[2].mult;
      }
      // ---- residual, term and d term / d s ----------------------------------------------------------------------------
      const float r = KIND == 0 ? d.fsrc[i * d.ld] - sdf : 0.0f;      // (the projected match has no reference column)
      float term, coef;
      if constexpr (KIND == 1) {
        const float* nr = d.fsrc + i * d.ld;
        const float nn[3] = {nr[0], nr[1], nr[2]};
        float a = 0.0f;
#pragma unroll
        for (int r_ = 0; r_ < 3; ++r_) a += dq[r_] * (M[r_][0] * nn[0] + M[r_][1] * nn[1] + M[r_][2] * nn[2]);
        const float c_ = sdf * a;
        term = c_ * c_; coef = 2.0f * (c_ * a);
        const float c2 = 2.0f * (sdf * c_);
#pragma unroll
        for (int r_ = 0; r_ < 3; ++r_)
#pragma unroll
          for (int b = 0; b < 3; ++b) acc[14 + r_ * 3 + b] += (c2 * dq[r_]) * nn[b];
      } else if constexpr (KIND == 2) {
        const float g2 = (dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2];
        const float sg = sdf * g2;
        term = sdf * sg; coef = 2.0f * sg;
      } else if (loss_type == 2) {
        term = r * r; coef = -2.0f * r;
      } else if (loss_type == 1) {      // |r|_2 of a one-column row; vector_norm's backward: sign(0) = 0
        term = fabsf(r); coef = r > 0.0f ? -1.0f : (r < 0.0f ? 1.0f : 0.0f);
      } else {                          // Geman-McClure, the weight a constant (e = resid.detach())
        const float den = gm_scale + r * r;
        const float w = gm_scale / (den * den);
        term = w * (r * r); coef = -2.0f * (w * r);
      }
      const float gq[3] = {coef * dq[0], coef * dq[1], coef * dq[2]};
      const float pp[3] = {px, py, pz};
      acc[0] += term; acc[1] += 1.0f;
#pragma unroll
      for (int a = 0; a < 3; ++a) acc[2 + a] += gq[a];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) acc[5 + a * 3 + b] += pp[a] * gq[b];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();          // the next chunk overwrites the tile
  }
  // Reduction, as pair_latent_body: the wavefront by an fp32 shuffle tree, then in double -- the wave sums of the
  // workgroup, the two 3x3 products with the poses, one fp64 atomic per value per workgroup.
  __shared__ double red[PAIR_SDF_WAVES + 1][NACC + 2];
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    float v = acc[i];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if (lane == 0) red[wave][i] = (double)v;
  }
  __syncthreads();
  static_assert(PAIR_SDF_WAVES == 4, "the fixed tree below adds four wave sums");
  if (threadIdx.x < NACC)
    red[4][threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
  __syncthreads();
  // (a workgroup without an in-bound row adds nothing: its sums are zeros, and a NaN pose -- no row in bound -- would
  // turn the products with the pose below into NaN)
  if (threadIdx.x < 23 && red[4][1] != 0.0) {
    const double* T = red[4];
    const int t = threadIdx.x;
    double v;
    if (t < 5) {
      v = T[t];
    } else if (t < 14) {      // sum d_a g_b = (Rs S)_ab + (ts - td)_a G_b
      const int a = (t - 5) / 3, b = (t - 5) % 3;
      v = ((double)pose_s[3 * a] * T[5 + b] + (double)pose_s[3 * a + 1] * T[8 + b]) + (double)pose_s[3 * a + 2] * T[11 + b] +
          ((double)pose_s[9 + a] - (double)pose_d[9 + a]) * T[2 + b];
      if constexpr (KIND == 1)      // + (Rs S2^T)_ab
        v += ((double)pose_s[3 * a] * T[14 + 3 * b] + (double)pose_s[3 * a + 1] * T[15 + 3 * b]) + (double)pose_s[3 * a + 2] * T[16 + 3 * b];
    } else {                  // sum (Rd g)_a p_b = sum_c Rd[a][c] S[b][c]
      const int a = (t - 14) / 3, b = (t - 14) % 3;
      v = ((double)pose_d[3 * a] * T[5 + 3 * b] + (double)pose_d[3 * a + 1] * T[6 + 3 * b]) + (double)pose_d[3 * a + 2] * T[7 + 3 * b];
      if constexpr (KIND == 1)      // + (Rd S2)_ab
        v += ((double)pose_d[3 * a] * T[14 + b] + (double)pose_d[3 * a + 1] * T[17 + b]) + (double)pose_d[3 * a + 2] * T[20 + b];
    }
    if (v != 0.0) atomic_add_f64(out + t, v);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// dynamic LDS of a launch: the decoder image beside one d-feat tile per wavefront; 0 = more than a workgroup can have
static size_t pair_sdf_lds_bytes(int C, int L, int H, int NH, bool split) {
  const PackLayout pl(C * L, H, NH);
  const int pack = image_floats(pl, split, true);
  const size_t bytes = (size_t)(pack + PAIR_SDF_WAVES * 64 * dfeat_pitch(C * L)) * sizeof(float);
  return bytes <= MISO_LDS_LIMIT ? bytes : 0;
}

// can the SDF pair stage serve this decoder shape, in both arithmetic forms?
bool pair_sdf_covered(int C, int L, int H, int NH) {
  return fused_shape_supported(C, L, H, NH) && pair_sdf_lds_bytes(C, L, H, NH, true) && pair_sdf_lds_bytes(C, L, H, NH, false);
}

template <int C, int L, int H, int NH>
static hipError_t launch_pair_sdf_t(FusedShape<C, L, H, NH>, const PairSdfK& k, const AlignPairK* plan_dev, int n_pairs,
                                    int64_t max_n, const float* pose_all, int loss_type, double* out_all,
                                    const int32_t* stopped, const int32_t* order, bool split, hipStream_t s) {
  const size_t lds = pair_sdf_lds_bytes(C, L, H, NH, split);
  if (!lds) return hipErrorInvalidValue;      // (miso_align_plan_build has asked pair_sdf_covered)
  // a workgroup stages the decoder image once and walks chunks of 64 rows with its four wavefronts: ~2000 workgroups in
  // all (a few rounds of what is resident beside that much LDS), at least 16 and at most 512 per pair
  const int64_t per = 64 * PAIR_SDF_WAVES;
  unsigned blocks = (unsigned)((max_n + per - 1) / per);
  unsigned cap = 2048u / (unsigned)n_pairs;
  cap = cap < 16u ? 16u : (cap > 512u ? 512u : cap);
  if (blocks > cap) blocks = cap;
  auto kern = k.constraint == 1 ? (split ? pair_sdf_stage_kernel<C, L, H, NH, true, 1> : pair_sdf_stage_kernel<C, L, H, NH, false, 1>)
            : k.constraint == 2 ? (split ? pair_sdf_stage_kernel<C, L, H, NH, true, 2> : pair_sdf_stage_kernel<C, L, H, NH, false, 2>)
                                : (split ? pair_sdf_stage_kernel<C, L, H, NH, true, 0> : pair_sdf_stage_kernel<C, L, H, NH, false, 0>);
  hipError_t e = allow_dynamic_lds((const void*)kern, lds);
  if (e != hipSuccess) return e;
  kern<<<dim3(blocks, (unsigned)n_pairs), 64 * PAIR_SDF_WAVES, lds, s>>>(plan_dev, pose_all, loss_type, k.gm_scale, k.packed,
                                                                           out_all, stopped, order);
  return hipGetLastError();
}

hipError_t launch_pair_sdf_stage(const PairSdfK& k, const AlignPairK* plan_dev, int n_pairs, int64_t max_n,
                                 const float* pose_all, int loss_type, double* out_all, const int32_t* stopped,
                                 const int32_t* order, hipStream_t s) {
  if (n_pairs <= 0 || max_n <= 0) return hipSuccess;
  const bool split = use_split(k.exact);
  return with_fused_shape(k.C, k.L, k.H, k.NH, hipErrorInvalidValue, [&](auto shape) {
    return launch_pair_sdf_t(shape, k, plan_dev, n_pairs, max_n, pose_all, loss_type, out_all, stopped, order, split, s);
  });
}

}  // namespace miso

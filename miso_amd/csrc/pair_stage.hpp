// What the two pair stages of an alignment iteration share -- the latent residual (pair_latent.hip) and the SDF residual
// (pair_sdf.hip): the one arithmetic of src -> world -> dst that every in-bound decision is taken on, the slack of the
// box cull, and the fp64 atomic their reductions end in.
#pragma once
#include "common.hpp"

namespace miso {

constexpr float BOX_SLACK = 2e-3f;      // metres, plus terms in the size of the coordinates (pair_latent_body)

// hardware fp64 add at L2 (global_atomic_add_f64, no return value)
__device__ __forceinline__ void atomic_add_f64(double* p, double v) {
  (void)__builtin_amdgcn_global_atomic_fadd_f64((__attribute__((address_space(1))) double*)(p), v);
}

// src -> world -> dst of one source vertex (transform_points_to, then transfrom_points_from: utils_geometry.py:214-240)
// in ONE fixed arithmetic: d = (Rs p + ts) - td with the row sums as fma chains, q = Rd^T d likewise.  Every in-bound
// decision -- pass 1 and pass 2 of the latent pair stage, the SDF pair stage, the point-list and the lattice form of the
// overlap gate -- is taken on these bits.  Written as plain products and sums, the copies of this expression came out of
// the compiler with different contractions, and the two forms of the gate disagreed on one vertex of 4 M for two submaps
// 0.35 degrees apart (test_lattice_overlap_gate_counts_equal_the_point_list_gate).
__device__ __forceinline__ void src_to_dst(const float (&Rs)[9], const float (&ts)[3], const float (&Rd)[9],
                                           const float (&td)[3], float px, float py, float pz, float (&d)[3],
                                           float (&q)[3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float w = __fadd_rn(__fmaf_rn(Rs[3 * r + 2], pz, __fmaf_rn(Rs[3 * r + 1], py, __fmul_rn(Rs[3 * r], px))), ts[r]);
    d[r] = __fsub_rn(w, td[r]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) q[c] = __fmaf_rn(Rd[6 + c], d[2], __fmaf_rn(Rd[3 + c], d[1], __fmul_rn(Rd[c], d[0])));
}

// The SDF residual of a plan (miso_align_t.residual != 0), as launch_pair_batch hands it to pair_sdf.hip
struct PairSdfK {
  int C, L, H, NH;        // the decoder shape: one for all pairs of the plan (miso_align_plan_build)
  bool exact;             // MISO_F_EXACT_F32 of the destination grids
  const float* packed;    // miso_mlp_pack's output
  float gm_scale;
  int constraint;         // miso_align_t.constraint: 0 the SDF residuals; 1 / 2 the projected match, plane / point
};

}  // namespace miso

/*
 * miso_hash_sdf.h -- fused SDF query of hash-indexed levels: the C ABI of csrc/hash_sdf.hip, in the same libmiso_hip.so
 * and with the conventions of miso_hip.h and miso_hash.h (raw DEVICE pointers, sizes, a hipStream_t as void*, nothing
 * allocated, asynchronous on that stream; 0 or a MISO_E_* / hipError_t code; every argument checked before any launch).
 *
 * sdf = decoder(concat_l trilinear(level l, x)) in one launch: the corner rows are gathered through the tables of a
 * miso_hash_grid_t exactly as miso_hash_encode_fwd gathers them, and the feature row goes straight to the frozen
 * decoder's matrix-core chains of miso_sdf_fwd (`packed`: miso_mlp_pack's output for `mlp`).  Covered: grids that
 * miso_hash_encode_fwd accepts whose levels share one C in {4, 8}, with a decoder of input width C * n_levels, output
 * width 1 and a (C, n_levels, hidden_dim, n_linear - 2) that miso_sdf_supported covers for dense levels of that C.
 * Anything else is MISO_E_UNSUPPORTED.
 *
 * decoder_flags: 0 (bf16x3 split products) or MISO_F_EXACT_F32 (exact fp32 chains); any other bit is MISO_E_BADARG.
 * The sampling flags stay in miso_hash_grid_t.flags.  Points are in the caller's order.  n == 0 is valid and launches
 * nothing.
 *
 * Like the other two headers this file is read by miso_amd/_lib.py (into tables of its own): keep its narrow style.
 */
#ifndef MISO_HASH_SDF_H
#define MISO_HASH_SDF_H

#include "miso_hip.h"
#include "miso_hash.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host query: 1 if (grid, mlp) is covered by miso_hash_sdf_fwd / miso_hash_sdf_bwd, else 0.  No pointer of a level is
 * dereferenced. */
int miso_hash_sdf_supported(const miso_hash_grid_t* grid, const miso_mlp_t* mlp);

/* Floats of miso_hash_sdf_bwd's workspace for n points: n * F (F = sum of C over levels); 0 for n <= 0 or a grid that
 * miso_hash_encode_fwd refuses. */
int64_t miso_hash_sdf_bwd_workspace_floats(const miso_hash_grid_t* grid, int64_t n);

/* sdf[n] of x (N,3) row-major metres.  relu_mask (or NULL): the ReLU sign bits the backward reads,
 * miso_sdf_mask_words(mlp) words per point slot, slots in whole blocks of 64 points -- the layout of miso_sdf_fwd. */
int miso_hash_sdf_fwd(const miso_hash_grid_t* grid, const miso_mlp_t* mlp, const float* packed, uint32_t decoder_flags,
                      const float* x, int64_t n, float* sdf, uint32_t* relu_mask, void* stream);

/* First backward for d loss / d sdf = grad_sdf[n], at most three launches: the decoder's backward chain writes the
 * d-feat rows (n, F) into `workspace` (16-byte aligned, miso_hash_sdf_bwd_workspace_floats; left there for the
 * caller), then miso_hash_encode_bwd's two launches read them -- grad_x (N,3), or NULL; and for each level with
 * level[l].grad != NULL: grad[row] += w * d-feat (float atomics; the caller zero-initialises).  relu_mask: as written
 * by miso_hash_sdf_fwd over the same points with the same decoder_flags.  When grad_x is non-NULL every level's
 * table must be valid.  The decoder's weights take no gradient; there is no second backward. */
int miso_hash_sdf_bwd(const miso_hash_grid_t* grid, const miso_mlp_t* mlp, const float* packed, uint32_t decoder_flags,
                      const float* x, int64_t n, const float* grad_sdf, const uint32_t* relu_mask, float* grad_x,
                      float* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif

/*
 * miso_hash.h -- hash-indexed feature levels: the C ABI of csrc/hash_encode.hip, in the same libmiso_hip.so and with the
 * conventions of miso_hip.h (raw DEVICE pointers, sizes, a hipStream_t as void*, nothing allocated, asynchronous on
 * that stream; 0 or a MISO_E_* / hipError_t code; every argument checked before any launch).
 *
 * A level has the geometry of a dense level (X, Y, Z vertices over the bound, sampled exactly as miso_encode_fwd samples
 * it: zeros padding and align_corners=False unless the flags say otherwise); only the address of a vertex changes.  Its
 * values are a table of `rows` rows of C contiguous floats, C in {1, 2, 4, 8}:
 *   dense-indexed (log2_rows == 0, rows == X Y Z <= 2^28)
 *       row(i, j, k) = (k Y + j) X + i                    -- the flat channels-last layout of the dense level
 *   hashed (MISO_HASH_LOG2_MIN <= log2_rows <= MISO_HASH_LOG2_MAX, rows == 2^log2_rows < X Y Z)
 *       row(i, j, k) = ((uint32_t)i * 1u ^ (uint32_t)j * 2654435761u ^ (uint32_t)k * 805459861u) & (rows - 1)
 *                                                         -- products wrap in uint32 (Instant-NGP's primes)
 * miso_hash_rows says which of the two a level of a given shape is.  A corner out of range is never hashed and adds
 * nothing; a level in ignore_mask gives zeros.
 *
 * Like miso_hip.h this file is read by miso_amd/_lib.py (into tables of its own): keep its narrow style.
 */
#ifndef MISO_HASH_H
#define MISO_HASH_H

#include "miso_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MISO_HASH_LOG2_MIN 4
#define MISO_HASH_LOG2_MAX 28

typedef struct {
  const float* table; /* (rows, C) values (may be NULL where only `grad` is used) */
  float* grad;        /* (rows, C) scatter-add target, or NULL */
  int64_t rows;
  int32_t X, Y, Z, C;
  int32_t log2_rows;  /* 0 = dense-indexed */
} miso_hash_level_t;

typedef struct {
  int32_t n_levels;
  uint32_t ignore_mask;             /* bit l set => level l contributes zeros */
  float bound_min[3], bound_max[3]; /* x,y,z metres (unused with COORDS_NORMALIZED) */
  uint32_t flags;                   /* MISO_F_ALIGN_CORNERS | MISO_F_PAD_BORDER | MISO_F_COORDS_NORMALIZED */
  miso_hash_level_t level[MISO_MAX_LEVELS];
} miso_hash_grid_t;

/* Host query: the rows of a level of X x Y x Z vertices behind a table of at most 2^log2_hashmap_size rows -- X Y Z
 * (dense-indexed) when that fits, else 2^log2_hashmap_size (hashed).  0: a size < 1 or a log2 outside MIN..MAX. */
int64_t miso_hash_rows(int32_t X, int32_t Y, int32_t Z, int32_t log2_hashmap_size);

/* feats[n, F] (row stride ld_out floats, F = sum of C over levels) = concat_l trilinear(level l, point n); x (N,3)
 * row-major metres.  All levels in one launch. */
int miso_hash_encode_fwd(const miso_hash_grid_t* grid, const float* x, int64_t n, float* feats, int64_t ld_out,
                         void* stream);

/* First backward: one launch for grad_x and one for the table gradients, all levels in each.  grad_feats (N,F) row
 * stride ld_g.  For each level with level[l].grad != NULL: grad[row] += w * grad_feats (float atomics; the caller
 * zero-initialises).  grad_x (N,3) may be NULL; when non-NULL every level's table must be valid.  There is no second
 * backward. */
int miso_hash_encode_bwd(const miso_hash_grid_t* grid, const float* x, int64_t n, const float* grad_feats, int64_t ld_g,
                         float* grad_x, void* stream);

#ifdef __cplusplus
}
#endif
#endif

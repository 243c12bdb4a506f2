/*
 * miso_hash_trace.h -- sphere tracing through hash-indexed levels in one launch: the C ABI of csrc/hash_trace.hip, in
 * the same libmiso_hip.so and with the conventions of the other three headers (raw DEVICE pointers, sizes, a hipStream_t
 * as void*, nothing allocated, asynchronous on that stream; 0 or a MISO_E_* / hipError_t code; every argument checked
 * before any launch).
 *
 * The loop of miso_atlas_sphere_trace (miso_hip.h) with the field of miso_hash_sdf_fwd (miso_hash_sdf.h): per ray
 * p = origin + min_dist dir, then up to max_iters rounds of dist = |p - origin|, s = sdf(p), stop where s < epsilon
 * (hit) or dist > max_dist, else p += s dir.  A ray sees at every point the bits miso_hash_sdf_fwd returns there for
 * the same (grid, mlp, packed, decoder_flags); the shapes covered are that entry's.  A NaN field value never stops a
 * ray and leaves its hit flag 0.
 *
 * decoder_flags: 0 (bf16x3 split products) or MISO_F_EXACT_F32 (exact fp32 chains); any other bit is MISO_E_BADARG.
 * n == 0 is valid and launches nothing.
 *
 * Like the other headers this file is read by miso_amd/_lib.py (into tables of its own): keep its narrow style.
 */
#ifndef MISO_HASH_TRACE_H
#define MISO_HASH_TRACE_H

#include "miso_hip.h"
#include "miso_hash.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host query: 1 if (grid, mlp) is covered by miso_hash_sphere_trace, else 0.  No pointer of a level is dereferenced. */
int miso_hash_trace_supported(const miso_hash_grid_t* grid, const miso_mlp_t* mlp);

/* origins, dirs (n,3) row-major, dirs of unit length (the caller normalises); max_iters >= 1.  points (n,3): where each
 * ray stopped or was cut off; hit (n): 1 where s < epsilon in the ray's last round.  Optional outputs, each NULL or
 * valid: sdf_or_null (n) the field at points; steps_or_null (n) the rounds in which the ray moved; grad_or_null (n,3)
 * central differences (sdf(p + fd_step e_a) - sdf(p - fd_step e_a)) / (2 fd_step) at points, which needs a finite
 * fd_step > 0. */
int miso_hash_sphere_trace(const miso_hash_grid_t* grid, const miso_mlp_t* mlp, const float* packed,
                           uint32_t decoder_flags, const float* origins, const float* dirs, int64_t n, float min_dist,
                           float max_dist, int32_t max_iters, float epsilon, float fd_step, float* points, uint8_t* hit,
                           float* sdf_or_null, int32_t* steps_or_null, float* grad_or_null, void* stream);

#ifdef __cplusplus
}
#endif
#endif

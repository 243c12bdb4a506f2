// The trilinear sampler, said once: sample position per axis, the cell, its corner table and the lerp tree.  This is the
// text that has to mirror the reference's grid_sample operation for operation (bit parity with the PyTorch path rests
// on it); every kernel that samples a feature grid takes these steps from here.
//   level_cell      point -> Axis x3 -> Cell of one level
//   corner          corner k of a cell: in-range flag and element offset
//   corner_weight   its trilinear weight, with the first-derivative (and mixed second-derivative) weights on request
//   lerp_tree       eight zero-padded corner values -> value and derivatives, where corner weights cost too many registers
#pragma once
#include "common.hpp"

namespace miso {

__device__ __forceinline__ void load_point(const GridK& g, const float* __restrict__ x, int64_t p, float& px,
                                           float& py, float& pz) {
  if (g.xstride == 4) {
    const float4 v = reinterpret_cast<const float4*>(x)[p];
    px = v.x; py = v.y; pz = v.z;
  } else {
    px = x[p * 3 + 0]; py = x[p * 3 + 1]; pz = x[p * 3 + 2];
  }
}

// Per-axis sample position.  Mirrors the reference op by op (no FMA
// contraction) so coordinates are bit-identical to the PyTorch path:
//   utils.normalize_coordinates (grid_opt/utils/utils.py:49):
//       xn = 2 * (x - bmin) / (bmax - bmin) - 1
//   ATen grid_sampler_unnormalize (align_corners=False): ix = ((xn + 1) * size - 1) / 2
// `mult` is d(ix)/d(x) as autograd forms it.
struct Axis {
  float pos;   // continuous index ix
  float mult;  // d ix / d x  (0 where border padding clipped the coordinate)
};

// The two halves of axis_coord.  A kernel that evaluates several levels at one point calls them apart: the normalised
// coordinate and the factor 2 / len do not depend on the level (two IEEE divisions per axis and level otherwise).
__device__ __forceinline__ void axis_norm(float x, float bmin, float bmax, uint32_t flags, float& xn, float& m) {
  xn = x; m = 1.0f;
  if (!(flags & MISO_F_COORDS_NORMALIZED)) {
    const float len = __fsub_rn(bmax, bmin);
    xn = __fsub_rn(__fdiv_rn(__fmul_rn(2.0f, __fsub_rn(x, bmin)), len), 1.0f);
    m = __fdiv_rn(2.0f, len);
  }
}
// (Without OCML_BASIC_ROUNDED_OPERATIONS HIP's __fadd_rn / __fsub_rn / __fmul_rn are plain operators, so the compiler may
// contract them: (xn + 1) * size - 1 below is one v_fma_f32, a single rounding.)
__device__ __forceinline__ Axis axis_from_norm(float xn, float m, int size, uint32_t flags) {
  const float fs = (float)size;
  float ix;
  if (flags & MISO_F_ALIGN_CORNERS) {
    ix = __fmul_rn(__fmul_rn(__fadd_rn(xn, 1.0f), 0.5f), (float)(size - 1));   // x / 2 == x * 0.5 exactly
    m *= 0.5f * (float)(size - 1);
  } else {
    ix = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(xn, 1.0f), fs), 1.0f), 0.5f);   // (an IEEE divide is ~10 instructions)
    m *= 0.5f * fs;
  }
  if (flags & MISO_F_PAD_BORDER) {
    const float hi = (float)(size - 1);
    if (ix <= 0.0f) { ix = 0.0f; m = 0.0f; }
    else if (ix >= hi) { ix = hi; m = 0.0f; }
  }
  Axis a; a.pos = ix; a.mult = m;
  return a;
}
__device__ __forceinline__ Axis axis_coord(float x, float bmin, float bmax, int size, uint32_t flags) {
  float xn, m;
  axis_norm(x, bmin, bmax, flags, xn, m);
  return axis_from_norm(xn, m, size, flags);
}

// Trilinear cell: base corner, the two 1-D weights per axis (ATen forms them
// as (i0+1-ix) and (ix-i0), gridsample_cuda.cu:335-342) and in-range flags.
struct Cell {
  int i0, j0, k0;
  float wx[2], wy[2], wz[2];
  bool inx[2], iny[2], inz[2];
};

__device__ __forceinline__ void axis_cell(float pos, int size, int& i0, float w[2], bool in[2]) {
  float f = floorf(pos);
  // clamp before the int conversion so far-away points cannot overflow
  f = fminf(fmaxf(f, -2.0f), (float)size + 1.0f);
  i0 = (int)f;
  if (pos != pos) { i0 = -2; }  // NaN coordinate: every corner out of range
  w[0] = __fsub_rn(f + 1.0f, pos);
  w[1] = __fsub_rn(pos, f);
  in[0] = (i0 >= 0) && (i0 < size);
  in[1] = (i0 + 1 >= 0) && (i0 + 1 < size);
}

__device__ __forceinline__ Cell make_cell(const Axis& ax, const Axis& ay, const Axis& az,
                                          const LevelK& lv) {
  Cell c;
  axis_cell(ax.pos, lv.X, c.i0, c.wx, c.inx);
  axis_cell(ay.pos, lv.Y, c.j0, c.wy, c.iny);
  axis_cell(az.pos, lv.Z, c.k0, c.wz, c.inz);
  return c;
}

// The cell of point (px, py, pz) in level lv, and the three sample positions a[0..2] (x, y, z) it was formed from.  The
// bound comes as two arrays, so that a kernel that keeps laundered copies of it (sdf_fwd_kernel) can hand those in.
__device__ __forceinline__ Cell level_cell(const float bmin[3], const float bmax[3], uint32_t flags, const LevelK& lv,
                                           float px, float py, float pz, Axis (&a)[3]) {
  a[0] = axis_coord(px, bmin[0], bmax[0], lv.X, flags);
  a[1] = axis_coord(py, bmin[1], bmax[1], lv.Y, flags);
  a[2] = axis_coord(pz, bmin[2], bmax[2], lv.Z, flags);
  return make_cell(a[0], a[1], a[2], lv);
}
__device__ __forceinline__ Cell level_cell(const GridK& g, const LevelK& lv, float px, float py, float pz, Axis (&a)[3]) {
  return level_cell(g.bmin, g.bmax, g.flags, lv, px, py, pz, a);
}
// ... from the halves: xn / mn are axis_norm's results, formed once for all levels
__device__ __forceinline__ Cell level_cell_from_norm(const float xn[3], const float mn[3], uint32_t flags, const LevelK& lv,
                                                     Axis (&a)[3]) {
  a[0] = axis_from_norm(xn[0], mn[0], lv.X, flags);
  a[1] = axis_from_norm(xn[1], mn[1], lv.Y, flags);
  a[2] = axis_from_norm(xn[2], mn[2], lv.Z, flags);
  return make_cell(a[0], a[1], a[2], lv);
}

// Corner k = dx + 2 dy + 4 dz of the cell: whether it lies in the level, and its element offset (channel 0).
// ADD_STRIDES: the base corner's offset once, the others by additions (pair_latent.hip: a 32-bit integer multiply is a
// quarter-rate instruction, and three per corner were 24 of them per level and vertex).  The same integer either way.
__device__ __forceinline__ bool corner_in(const Cell& c, int k) { return c.inx[k & 1] && c.iny[(k >> 1) & 1] && c.inz[k >> 2]; }
template <bool ADD_STRIDES = false>
__device__ __forceinline__ int corner_offset(const Cell& c, const LevelK& lv, int k) {
  const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
  if (ADD_STRIDES) return (c.k0 * lv.sZ + c.j0 * lv.sY + c.i0 * lv.sX) + (dz ? lv.sZ : 0) + (dy ? lv.sY : 0) + (dx ? lv.sX : 0);
  return (c.k0 + dz) * lv.sZ + (c.j0 + dy) * lv.sY + (c.i0 + dx) * lv.sX;
}
// ... both: off = 0 for a corner out of range, a valid address, so a kernel may load first and zero afterwards
template <bool ADD_STRIDES = false>
__device__ __forceinline__ bool corner(const Cell& c, const LevelK& lv, int k, int& off) {
  const bool in = corner_in(c, k);
  off = in ? corner_offset<ADD_STRIDES>(c, lv, k) : 0;
  return in;
}

// Weight of corner k, (wx wy) wz as ATen multiplies it, zero out of range (`in`: corner's answer).
//   ORDER 0  w
//   ORDER 1  + dx, dy, dz: d w / d (ix, iy, iz)
//   ORDER 2  + dxy, dxz, dyz, the mixed second derivatives (d2 w / d ix2 = 0).  Masked by a PRODUCT with 0 / 1 where the
//            others select: at a NaN coordinate these weights are NaN, not 0, as the second backward always answered.
struct CornerW { float w, dx, dy, dz, dxy, dxz, dyz; };
template <int ORDER>
__device__ __forceinline__ CornerW corner_weight(const Cell& c, int k, bool in) {
  const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
  const float sx = dx ? 1.f : -1.f, sy = dy ? 1.f : -1.f, sz = dz ? 1.f : -1.f;
  CornerW r = {};
  if constexpr (ORDER == 2) {
    const float m = in ? 1.0f : 0.0f;
    r.w = m * (c.wx[dx] * c.wy[dy]) * c.wz[dz];
    r.dx = m * sx * c.wy[dy] * c.wz[dz];
    r.dy = m * sy * c.wx[dx] * c.wz[dz];
    r.dz = m * sz * c.wx[dx] * c.wy[dy];
    r.dxy = m * sx * sy * c.wz[dz];
    r.dxz = m * sx * sz * c.wy[dy];
    r.dyz = m * sy * sz * c.wx[dx];
  } else {
    r.w = in ? (c.wx[dx] * c.wy[dy]) * c.wz[dz] : 0.0f;
    if constexpr (ORDER == 1) {
      r.dx = in ? sx * c.wy[dy] * c.wz[dz] : 0.0f;
      r.dy = in ? sy * c.wx[dx] * c.wz[dz] : 0.0f;
      r.dz = in ? sz * c.wx[dx] * c.wy[dy] : 0.0f;
    }
  }
  return r;
}

// Value, first and (SECOND) mixed second derivatives of the trilinear interpolant of eight corner values v[k] (zero where
// the corner is out of range) at the upper-corner weights (tx, ty, tz) = (wx[1], wy[1], wz[1]), by lerps along x, y, z:
// the same polynomial as sum_k v_k w_k with the corner weights above, without a weight register per corner and
// derivative.
struct Lerp3 { float f, fx, fy, fz, fxy, fxz, fyz; };
template <bool SECOND>
__device__ __forceinline__ Lerp3 lerp_tree(const float v[8], float tx, float ty, float tz) {
  Lerp3 r;
  const float d00 = v[1] - v[0], d10 = v[3] - v[2], d01 = v[5] - v[4], d11 = v[7] - v[6];       // d/dx on the (y,z) edges
  const float a00 = v[0] + tx * d00, a10 = v[2] + tx * d10, a01 = v[4] + tx * d01, a11 = v[6] + tx * d11;
  const float e0 = a10 - a00, e1 = a11 - a01;                                                     // d/dy at z = 0, 1
  const float b0 = a00 + ty * e0, b1 = a01 + ty * e1;
  r.f = b0 + tz * (b1 - b0);
  r.fz = b1 - b0;
  r.fy = e0 + tz * (e1 - e0);
  const float gx0 = d00 + ty * (d10 - d00), gx1 = d01 + ty * (d11 - d01);
  r.fx = gx0 + tz * (gx1 - gx0);
  if (SECOND) {
    r.fyz = e1 - e0;
    r.fxy = (d10 - d00) + tz * ((d11 - d01) - (d10 - d00));
    r.fxz = (d01 - d00) + ty * ((d11 - d10) - (d01 - d00));
  } else {
    r.fyz = r.fxy = r.fxz = 0.0f;
  }
  return r;
}

}  // namespace miso

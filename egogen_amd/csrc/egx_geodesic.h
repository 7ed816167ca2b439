// A geodesic distance field (geodesic.hip) read at a world point: the one device function behind egx_geodesic_sample and the goal
// term of the selection kernels (genop.hip), so both see the same bits.
#pragma once
#include "egx_common.h"

// The field of a launch as the selection kernels carry it; dist == nullptr: no field.
struct GeoFieldDev {
  const float* dist;    // [F,H,W]
  const float* origin;  // [F,2]
  const int* index;     // field of each group, or null: field 0
  float cell;
  int H, W, F;
};

// dist [H,W] of one field at (x, y): bilinear over the four surrounding cell centres (cell (i,j) has its centre at origin +
// (i + 0.5, j + 0.5) * cell); corners outside the raster, holding +inf or of weight 0 drop out and the rest are renormalised;
// EGX_GEODESIC_OFF where none is left, NaN for a NaN coordinate.  Every operation rounds on its own, in every kernel this is
// inlined into.
__device__ __forceinline__ float egx_geodesic_sample_at(const float* __restrict__ dist, int H, int W, float ox, float oy, float cell,
                                                        float x, float y) {
#pragma clang fp contract(off)
  if (isnan(x) || isnan(y)) return __builtin_nanf("");
  const float u = egx_sub((x - ox) / cell, 0.5f), v = egx_sub((y - oy) / cell, 0.5f);
  if (!(u > -1.f && u < (float)H && v > -1.f && v < (float)W)) return EGX_GEODESIC_OFF;   // no corner inside (also +-inf)
  const float fi = floorf(u), fj = floorf(v);
  const int i0 = (int)fi, j0 = (int)fj;                       // in [-1, H-1] x [-1, W-1]
  const float a1 = egx_sub(u, fi), b1 = egx_sub(v, fj), a0 = egx_sub(1.f, a1), b0 = egx_sub(1.f, b1);
  float sw = 0.f, sv = 0.f;
  for (int c = 0; c < 4; ++c) {                               // corner order (i0,j0), (i0,j0+1), (i0+1,j0), (i0+1,j0+1)
    const int i = i0 + (c >> 1), j = j0 + (c & 1);
    const float w = egx_mul((c >> 1) ? a1 : a0, (c & 1) ? b1 : b0);
    if (i < 0 || i >= H || j < 0 || j >= W || !(w > 0.f)) continue;
    const float d = dist[(size_t)i * W + j];
    if (!(d < __builtin_inff())) continue;
    sw = egx_add(sw, w);
    sv = egx_add(sv, egx_mul(w, d));
  }
  return sw > 0.f ? sv / sw : EGX_GEODESIC_OFF;
}

// the field of group g at (x, y)
__device__ __forceinline__ float egx_geodesic_sample_group(const GeoFieldDev& f, int g, float x, float y) {
  const int k = f.index ? min(max(f.index[g], 0), f.F - 1) : 0;
  return egx_geodesic_sample_at(f.dist + (size_t)k * f.H * f.W, f.H, f.W, f.origin[k * 2 + 0], f.origin[k * 2 + 1], f.cell, x, y);
}

// A person as the 67 blended markers of a candidate row in the world: the device functions the marker models share - the pair model
// of the joint step (genop_joint_markers.hip) and the marker model of recorded tracks (genop_obstacle_markers.hip).  Stated once so
// that both units round alike: the blend of the two marker sources, the row's frame applied with the nesting of field_row_cost
// (genop.hip) extended to z, and the squared distance of two markers.
#pragma once
#include "egx_common.h"

constexpr int EGX_MK = 67, EGX_MK_DIM = EGX_MK * 3;      // markers of a body, floats of a frame of them
constexpr int EGX_MK_FRAMES = 20, EGX_MK_SEED = 2;        // frames of a primitive, of which the first two are the seed

// the hand-off's blend of the body model's marker and the prior's, rf * proj + (1 - rf) * pred (blend_marker of genop.hip), with its
// roundings written out as the compiler contracted that expression in genop_joint_markers.hip: 1 - rf rounded, its product with
// pred rounded, then one fused multiply-add of rf and proj onto it
__device__ __forceinline__ float blend_marker(float rf, float proj, float pred) { return fmaf(rf, proj, egx_mul(egx_sub(1.f, rf), pred)); }

// world marker a of row r (of `rows`) at frame t (2..19): the blended local marker (markers_proj [rows*20,67,3], Y_gen [18,rows,201])
// in the row's frame (R0 [rows,9], T0 [rows,3]), pelvis_xy's nesting extended to z; .w = 1 where a coordinate is not finite
__device__ __forceinline__ float4 egx_world_marker(const float* markers_proj, const float* Y_gen, const float* R0_all, const float* T0_all,
                                                   size_t rows, float rf, size_t r, int t, int a) {
  const float* pr = markers_proj + (r * EGX_MK_FRAMES + t) * EGX_MK_DIM + 3 * a;
  const float* pd = Y_gen + ((size_t)(t - EGX_MK_SEED) * rows + r) * EGX_MK_DIM + 3 * a;
  const float* R0 = R0_all + r * 9;
  const float* T0 = T0_all + r * 3;
  const float m0 = blend_marker(rf, pr[0], pd[0]), m1 = blend_marker(rf, pr[1], pd[1]), m2 = blend_marker(rf, pr[2], pd[2]);
  float4 v;
  v.x = fmaf(R0[2], m2, fmaf(R0[1], m1, R0[0] * m0)) + T0[0];
  v.y = fmaf(R0[5], m2, fmaf(R0[4], m1, R0[3] * m0)) + T0[1];
  v.z = fmaf(R0[8], m2, fmaf(R0[7], m1, R0[6] * m0)) + T0[2];
  v.w = (isfinite(v.x) && isfinite(v.y) && isfinite(v.z)) ? 0.f : 1.f;
  return v;
}

// the squared distance of two world markers: three rounded differences, three rounded squares, (dx^2 + dy^2) + dz^2 in that order,
// no contraction.  The same bits with the two markers exchanged.
__device__ __forceinline__ float dist2(const float4& a, const float4& b) {
  const float dx = egx_sub(a.x, b.x), dy = egx_sub(a.y, b.y), dz = egx_sub(a.z, b.z);
  return egx_add(egx_add(egx_mul(dx, dx), egx_mul(dy, dy)), egx_mul(dz, dz));
}

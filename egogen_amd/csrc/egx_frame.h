// Canonical-frame algebra shared by the env kernels (env.hip) and the primitive hand-off (genop.hip): 3x3 products,
// CanonicalCoordinateExtractor.get_new_coordinate_torch and SMPLXParser.update_transl_glorot as device functions.
// Everything is force-inlined, so each kernel carries its own copy of the same arithmetic.
#pragma once
#include "egx_common.h"

__device__ __forceinline__ void mat3_mul(const float* A, const float* B, float* C) {  // C = A B
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) C[r * 3 + c] = A[r * 3 + 0] * B[0 * 3 + c] + A[r * 3 + 1] * B[1 * 3 + c] + A[r * 3 + 2] * B[2 * 3 + c];
}
__device__ __forceinline__ void mat3T_vec(const float* A, const float* v, float* o) {  // o = A^T v
  for (int r = 0; r < 3; ++r) o[r] = A[0 * 3 + r] * v[0] + A[1 * 3 + r] * v[1] + A[2 * 3 + r] * v[2];
}
__device__ __forceinline__ void mat3_vec(const float* A, const float* v, float* o) {
  for (int r = 0; r < 3; ++r) o[r] = A[r * 3 + 0] * v[0] + A[r * 3 + 1] * v[1] + A[r * 3 + 2] * v[2];
}

// CanonicalCoordinateExtractor.get_new_coordinate_torch: x = j2-j1 (z zeroed, normalised WITHOUT eps),
// z = (0,0,1), y = normalise(z x x); R = [x y z] as columns; T = j0
__device__ __forceinline__ void canonical_frame(const float* j0, const float* j1, const float* j2, float* R, float* T) {
  float x0 = j2[0] - j1[0], x1 = j2[1] - j1[1];
  const float nx = sqrtf(x0 * x0 + x1 * x1);
  x0 /= nx; x1 /= nx;
  float y0 = -x1, y1 = x0;  // (0,0,1) x (x0,x1,0)
  const float ny = sqrtf(y0 * y0 + y1 * y1);
  y0 /= ny; y1 /= ny;
  R[0] = x0; R[1] = y0; R[2] = 0.f;
  R[3] = x1; R[4] = y1; R[5] = 0.f;
  R[6] = 0.f; R[7] = 0.f; R[8] = 1.f;
  T[0] = j0[0]; T[1] = j0[1]; T[2] = j0[2];
}

// SMPLXParser.update_transl_glorot (torch branch): xb[0:6] -> new transl / glorot for frame (R,T), delta = rest root
__device__ __forceinline__ void update_transl_glorot(const float* R, const float* T, const float* delta, const float* xb, float* out6) {
  float go[9], gn[9], Rt[9];
  egx_tgm_aa_to_rotmat(xb + 3, go);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Rt[r * 3 + c] = R[c * 3 + r];
  mat3_mul(Rt, go, gn);
  egx_tgm_rotmat_to_aa(gn, out6 + 3);
  const float v[3] = {xb[0] + delta[0] - T[0], xb[1] + delta[1] - T[1], xb[2] + delta[2] - T[2]};
  float o[3];
  mat3T_vec(R, v, o);
  out6[0] = o[0] - delta[0]; out6[1] = o[1] - delta[1]; out6[2] = o[2] - delta[2];
}

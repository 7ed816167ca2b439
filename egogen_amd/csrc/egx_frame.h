// Canonical-frame algebra shared by the env kernels (env.hip) and the primitive hand-off (genop.hip): 3x3 products,
// CanonicalCoordinateExtractor.get_new_coordinate_torch and SMPLXParser.update_transl_glorot as device functions.
// Everything is force-inlined, so each kernel carries its own copy of the same arithmetic.
#pragma once
#include "egx_common.h"

// ---- rotation helpers shared with the network kernels (torchgeometry 0.1.2 semantics) ----
__device__ __forceinline__ void egx_tgm_rotmat_to_aa(const float* R /*row-major 3x3*/, float* aa) {
  // rotation_matrix_to_quaternion works on R^T: m[a][b] = R[b][a]
  const float m00 = R[0], m01 = R[3], m02 = R[6], m10 = R[1], m11 = R[4], m12 = R[7], m20 = R[2], m21 = R[5], m22 = R[8];
  float q0, q1, q2, q3, t;
  if (m22 < 1e-6f) {
    if (m00 > m11) {
      t = 1.f + m00 - m11 - m22;
      q0 = m12 - m21; q1 = t; q2 = m01 + m10; q3 = m20 + m02;
    } else {
      t = 1.f - m00 + m11 - m22;
      q0 = m20 - m02; q1 = m01 + m10; q2 = t; q3 = m12 + m21;
    }
  } else {
    if (m00 < -m11) {
      t = 1.f - m00 - m11 + m22;
      q0 = m01 - m10; q1 = m20 + m02; q2 = m12 + m21; q3 = t;
    } else {
      t = 1.f + m00 + m11 + m22;
      q0 = t; q1 = m12 - m21; q2 = m20 - m02; q3 = m01 - m10;
    }
  }
  const float sc = 0.5f / sqrtf(t);
  q0 *= sc; q1 *= sc; q2 *= sc; q3 *= sc;
  const float sin_sq = q1 * q1 + q2 * q2 + q3 * q3;
  const float sin_t = sqrtf(sin_sq);
  const float two_theta = 2.f * ((q0 < 0.f) ? atan2f(-sin_t, -q0) : atan2f(sin_t, q0));
  const float k = (sin_sq > 0.f) ? two_theta / sin_t : 2.f;
  aa[0] = q1 * k; aa[1] = q2 * k; aa[2] = q3 * k;
}

__device__ __forceinline__ void egx_tgm_aa_to_rotmat(const float* aa, float* R) {
  const float theta2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2];
  if (theta2 > 1e-6f) {
    const float theta = sqrtf(theta2);
    const float wx = aa[0] / (theta + 1e-6f), wy = aa[1] / (theta + 1e-6f), wz = aa[2] / (theta + 1e-6f);
    const float c = cosf(theta), s = sinf(theta), oc = 1.f - c;
    R[0] = c + wx * wx * oc;      R[1] = wx * wy * oc - wz * s; R[2] = wy * s + wx * wz * oc;
    R[3] = wz * s + wx * wy * oc; R[4] = c + wy * wy * oc;      R[5] = -wx * s + wy * wz * oc;
    R[6] = -wy * s + wx * wz * oc; R[7] = wx * s + wy * wz * oc; R[8] = c + wz * wz * oc;
  } else {
    R[0] = 1.f; R[1] = -aa[2]; R[2] = aa[1];
    R[3] = aa[2]; R[4] = 1.f; R[5] = -aa[0];
    R[6] = -aa[1]; R[7] = aa[0]; R[8] = 1.f;
  }
}

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

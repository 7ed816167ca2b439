// Reward arithmetic of CrowdEnv.step (motion/crowd_ppo/crowd_env_2f.py:171-235) shared by the env step (env.hip) and the
// candidate scoring of the primitive search (genop.hip): the per-frame skate and floor terms over the six feet markers, the
// target in the canonical frame, the facing term and the clipped target distance.  Each function returns the ARGUMENT the
// reference feeds its exp / threshold with; what a kernel does with it (reward or cost) is the kernel's business.
// Everything is force-inlined, so each kernel carries its own copy of the same arithmetic.
#pragma once
#include "egx_common.h"
#include "egx_frame.h"

// The two per-frame terms read the blended markers through an accessor `at(t, i)` = coordinate i (marker m at m*3 .. m*3 + 2) of
// frame t, so that each kernel keeps its own storage (and the compiler its address space).
// skating of central-difference frame t + 1 (:181-185): slowest of the six feet markers between frames t and t + 2, as a speed at
// 40 fps, above 0.075 m/s
template <class At>
__device__ __forceinline__ float reward_skate_frame(At at, int t, const int* feet_marker_idx) {
  float mn = 3.4e38f;
  for (int k = 0; k < 6; ++k) {
    const int m = feet_marker_idx[k];
    const float dx = at(t + 2, m * 3 + 0) - at(t, m * 3 + 0);
    const float dy = at(t + 2, m * 3 + 1) - at(t, m * 3 + 1);
    const float dz = at(t + 2, m * 3 + 2) - at(t, m * 3 + 2);
    const float sp = sqrtf(dx * dx + dy * dy + dz * dz) / 2.f / (1.f / 40.f);
    mn = fminf(mn, sp);
  }
  return fmaxf(mn - 0.075f, 0.f);
}

// floor contact of frame t (:190-194): |lowest world-frame z of the six feet markers - 0.02|
template <class At>
__device__ __forceinline__ float reward_floor_frame(const float* R0, const float* T0, At at, int t, const int* feet_marker_idx) {
  float mn = 3.4e38f;
  for (int k = 0; k < 6; ++k) {
    const int m = feet_marker_idx[k];
    const float z = (R0[6] * at(t, m * 3 + 0) + R0[7] * at(t, m * 3 + 1) + R0[8] * at(t, m * 3 + 2)) + T0[2];
    mn = fminf(mn, z);
  }
  return fabsf(mn - 0.02f);
}

// world target -> the canonical frame (R0, T0): R0^T (target - T0)
__device__ __forceinline__ void target_to_local(const float* R0, const float* T0, const float* target_w, float* tl) {
  const float v[3] = {target_w[0] - T0[0], target_w[1] - T0[1], target_w[2] - T0[2]};
  mat3T_vec(R0, v, tl);
}

// facing the target (:217-219): ((unit xy direction pelvis -> target) . (body orientation) + 1) / 2 with the body orientation
// (0,0,1) x normalise(joint2 - joint1) of the last body.  tl receives the target in the frame (R0, T0), dir2 the unit direction
// (the distance and the looking term reuse them).
__device__ __forceinline__ float reward_face(const float* j19, const float* R0, const float* T0, const float* target_w, float* tl,
                                             float* dir2) {
  float xa0 = j19[2 * 3 + 0] - j19[1 * 3 + 0], xa1 = j19[2 * 3 + 1] - j19[1 * 3 + 1];
  float nrm = fmaxf(sqrtf(xa0 * xa0 + xa1 * xa1), 1e-12f);
  xa0 /= nrm; xa1 /= nrm;
  const float bo0 = -xa1, bo1 = xa0;  // (0,0,1) x x_axis, xy part
  target_to_local(R0, T0, target_w, tl);
  float f0 = tl[0] - j19[0], f1 = tl[1] - j19[1];
  nrm = fmaxf(sqrtf(f0 * f0 + f1 * f1), 1e-12f);
  f0 /= nrm; f1 /= nrm;
  dir2[0] = f0; dir2[1] = f1;
  return ((f0 * bo0 + f1 * bo1) + 1.f) / 2.0f;
}

// the clipped 3-D distance pelvis -> target (:232; _get_feature, :680-727)
__device__ __forceinline__ float target_distance(const float* target_l, const float* pelvis) {
  const float fx = target_l[0] - pelvis[0], fy = target_l[1] - pelvis[1], fz = target_l[2] - pelvis[2];
  return fmaxf(sqrtf(fx * fx + fy * fy + fz * fz), 1e-12f);
}

// SDF penetration (:171-177): argument of the exp from the summed count of the 20 bodies, collision from the largest
__device__ __forceinline__ float reward_pene_arg(float total_count) { return total_count / 20.f / 10.f; }

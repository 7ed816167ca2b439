// Moving obstacles of the primitive search (genop.hip): S sets of up to EGX_MAX_OBSTACLES tracks, a track a world xy per absolute
// frame and a radius: a person as a vertical cylinder.  The device functions behind the obstacle phase of the selection kernels:
// the window of one primitive staged into LDS, and the clearance of one point against one frame of that window.  With the marker
// model of recorded tracks the phase reads its frame clearances from a table instead (frame_clearance below) and stages nothing.
#pragma once
#include "egx_common.h"

constexpr int EGX_OBS_FRAMES = 18;   // the predicted frames 2..19 of a primitive: what the obstacle term scores

// The obstacles of a launch as the selection kernels carry them; term == nullptr: no obstacle phase.
struct ObstaclesDev {
  const float* xy;      // [S,O_max,T,2] world xy per absolute frame
  const float* radius;  // [S,O_max] metres
  const int* count;     // [S] live tracks of each set
  const int* index;     // set of each group, or null: set 0
  int S, O_max, T, frame0;
  float w, margin, body_radius;
  float* term;          // [rows] outputs of the phase
  float* clearance;     // [rows]
  int* hit;             // [rows]
  const float* frame_clearance;  // [rows,18] c_t of every row and predicted frame, written ahead of the launch by
                                 // egx_obstacle_marker_clearance (genop_obstacle_markers.hip): the marker model; null: cylinders
};

// The window of group g's set for the primitive that starts at absolute frame ob.frame0, by the whole workgroup: s_x / s_y [f][o] the
// position of obstacle o at absolute frame clamp(frame0 + 2 + f, 0, T - 1) (before its track an obstacle stands at its first
// position, after it where it stopped), s_rr [o] = radius + body_radius, one rounded addition.  Returns the number of live
// obstacles (the same in every thread); the caller's barrier makes the window visible.
__device__ __forceinline__ int egx_obstacles_stage(const ObstaclesDev& ob, int g, float (*s_x)[EGX_MAX_OBSTACLES],
                                                   float (*s_y)[EGX_MAX_OBSTACLES], float* s_rr) {
  if (ob.O_max < 1) return 0;
  const int set = ob.index ? min(max(ob.index[g], 0), ob.S - 1) : 0;
  const int cnt = min(max(ob.count[set], 0), min(ob.O_max, EGX_MAX_OBSTACLES));
  for (int e = threadIdx.x; e < EGX_OBS_FRAMES * cnt; e += blockDim.x) {
    const int f = e / cnt, o = e % cnt;
    const long long a = min(max((long long)ob.frame0 + 2 + f, 0LL), (long long)ob.T - 1);
    const float* q = ob.xy + (((size_t)set * ob.O_max + o) * ob.T + (size_t)a) * 2;
    s_x[f][o] = q[0];
    s_y[f][o] = q[1];
  }
  for (int o = threadIdx.x; o < cnt; o += blockDim.x) s_rr[o] = egx_add(ob.radius[(size_t)set * ob.O_max + o], ob.body_radius);
  return cnt;
}

// min over the cnt obstacles of one frame of sqrt((x - ox)^2 + (y - oy)^2) - (r + body_radius): two rounded differences, two rounded
// squares, their rounded sum, the correctly rounded root, one rounded difference; min is order-free.  +inf for an empty set, NaN
// for a NaN coordinate.
__device__ __forceinline__ float egx_obstacle_clearance(float x, float y, int cnt, const float* s_x, const float* s_y, const float* s_rr) {
#pragma clang fp contract(off)
  if (isnan(x) || isnan(y)) return __builtin_nanf("");
  float m = __builtin_inff();
  for (int o = 0; o < cnt; ++o) {
    const float dx = egx_sub(x, s_x[o]), dy = egx_sub(y, s_y[o]);
    const float d = sqrtf(egx_add(egx_mul(dx, dx), egx_mul(dy, dy)));
    m = fminf(m, egx_sub(d, s_rr[o]));
  }
  return m;
}

// The same against the members of a group of the joint search (genop_joint.hip): the cnt columns of one frame of the group's table
// except column `skip` (the member itself), every member the same cylinder, rr = body_radius + body_radius rounded once by the
// caller.  The same roundings in the same order.  +inf where no other member is left; NaN for a NaN x / y; another member's NaN
// coordinate gives a NaN distance, which fminf drops: that member is not there in this frame.
__device__ __forceinline__ float egx_pair_clearance(float x, float y, int cnt, int skip, const float* s_x, const float* s_y, float rr) {
#pragma clang fp contract(off)
  if (isnan(x) || isnan(y)) return __builtin_nanf("");
  float m = __builtin_inff();
  for (int o = 0; o < cnt; ++o) {
    if (o == skip) continue;
    const float dx = egx_sub(x, s_x[o]), dy = egx_sub(y, s_y[o]);
    const float d = sqrtf(egx_add(egx_mul(dx, dx), egx_mul(dy, dy)));
    m = fminf(m, egx_sub(d, rr));
  }
  return m;
}

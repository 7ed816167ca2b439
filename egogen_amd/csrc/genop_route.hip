// Waypoint routes of the primitive search (egogen_amd/route.py, `generate_sequence_to_goal(route=)`): egx_route_advance, the one
// launch per primitive that moves every sequence's cursor along its route and rewrites the two device buffers through which every
// other kernel of the loop sees the goal - the live goal [b,3] and, with a geodesic field, the field index [b].  It comes after the
// hand-off (egx_primitive_advance_select) and reads only what the hand-off recorded for the primitive: pelvis [b,20,3], rotmat
// [b,3,3], transl [b,3].  So a float64 restatement can be fed from a returned `PrimitiveSequence` alone
// (tests/genop_route_ref.py).
//
// One wave per sequence, lanes 0..17 one predicted frame each (f = lane + 2; frames 0 and 1 are the seed every candidate shared).
// The world xy of the frame's pelvis has the nesting of field_row_cost / obstacle_group (genop.hip); the horizontal distance to a
// waypoint rounds once per operation: h = sqrt(dx * dx + dy * dy), dx = x - wx, dy = y - wy.  Which frame passes first is a ballot
// and the recorded distance a minimum: neither depends on an order.  No atomics; lane 0 writes everything with plain stores.
#include <cmath>

#include "egx_common.h"

namespace {

constexpr int NT = 20, THIS = 2, NPRED = NT - THIS;
constexpr int RT_BLK = 256, RT_WAVES = RT_BLK / 64;

struct RouteArgs {
  const float* pelvis;      // [b,20,3]
  const float* R;           // [b,9]
  const float* T;           // [b,3]
  const float* waypoints;   // [b,P,3]
  const int* count;         // [b]
  const int* field_of;      // [b,P] or null
  int b, P;
  float radius;
  int* cursor;              // [b] read and written
  float* goal;              // [b,3]
  int* field_index;         // [b] or null
  int* reached;             // [b] read and written
  int* route_cursor;        // [b]
  float* route_goal;        // [b,3]
  float* pass_dist;         // [b]
};

__device__ __forceinline__ float wave_min(float v) {   // every lane's partner chain ends in lane 0; min is order-free
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_down(v, o, 64));
  return v;
}

__device__ __forceinline__ float horizontal(float x, float y, const float* w) {
  const float dx = egx_sub(x, w[0]), dy = egx_sub(y, w[1]);
  return sqrtf(egx_add(egx_mul(dx, dx), egx_mul(dy, dy)));
}

}  // namespace

__global__ __launch_bounds__(RT_BLK) void egx_route_advance_kernel(RouteArgs p) {
  const int g = blockIdx.x * RT_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (g >= p.b) return;                                   // the same in every lane of a wave
  const int n = min(max(p.count[g], 1), p.P);
  const int c0 = min(max(p.cursor[g], 0), n - 1);
  const float* W = p.waypoints + (size_t)g * p.P * 3;
  const bool mine = lane < NPRED;
  float x = 0.f, y = 0.f;
  if (mine) {
    const float* R = p.R + (size_t)g * 9;
    const float* T = p.T + (size_t)g * 3;
    const float* j = p.pelvis + ((size_t)g * NT + THIS + lane) * 3;
    x = egx_add(fmaf(R[2], j[2], fmaf(R[1], j[1], egx_mul(R[0], j[0]))), T[0]);
    y = egx_add(fmaf(R[5], j[2], fmaf(R[4], j[1], egx_mul(R[3], j[0]))), T[1]);
  }
  const bool any_nan = __ballot(mine && (isnan(x) || isnan(y))) != 0ull;
  const float h0 = mine ? horizontal(x, y, W + (size_t)c0 * 3) : __builtin_inff();
  const float dmin = wave_min(h0);                         // read only where no position is NaN
  int c = c0, f0 = 0;                                      // f0: the first lane that may pass the current waypoint
  while (!any_nan && c < n - 1) {                          // wave-uniform
    const float h = mine ? horizontal(x, y, W + (size_t)c * 3) : __builtin_inff();
    const unsigned long long hit = __ballot(mine && lane >= f0 && h < p.radius);
    if (!hit) break;
    f0 = __ffsll((long long)hit) - 1;                      // the next waypoint may be passed at that same frame
    ++c;
  }
  if (lane != 0) return;
  const float* w0 = W + (size_t)c0 * 3;
  const float* w1 = W + (size_t)c * 3;
  for (int e = 0; e < 3; ++e) {
    p.route_goal[(size_t)g * 3 + e] = w0[e];
    p.goal[(size_t)g * 3 + e] = w1[e];
  }
  p.pass_dist[g] = any_nan ? __builtin_nanf("") : dmin;
  p.cursor[g] = c;
  p.route_cursor[g] = c;
  if (p.field_index) p.field_index[g] = p.field_of[(size_t)g * p.P + c];
  if (c0 != n - 1) p.reached[g] = 0;                       // the flag was written against an intermediate point
}

extern "C" int egx_route_advance(const float* pelvis_loc, const float* transf_rotmat, const float* transf_transl, const float* waypoints,
                                 const int32_t* count, const int32_t* field_of, int num_sequences, int max_waypoints, float pass_radius,
                                 int32_t* cursor, float* goal, int32_t* field_index, int32_t* reached, int32_t* route_cursor,
                                 float* route_goal, float* route_pass_dist, void* stream) {
  EGX_REQUIRE(pelvis_loc && transf_rotmat && transf_transl && waypoints && count, "null input");
  EGX_REQUIRE(cursor && goal && reached && route_cursor && route_goal && route_pass_dist, "null output");
  EGX_REQUIRE(!field_index || field_of, "a field index buffer needs field_of");
  EGX_REQUIRE(num_sequences >= 1, "need a non-empty batch");
  EGX_REQUIRE(max_waypoints >= 1 && max_waypoints <= EGX_MAX_WAYPOINTS, "max_waypoints must be in [1, EGX_MAX_WAYPOINTS]");
  EGX_REQUIRE(pass_radius >= 0.f, "pass_radius must not be negative or NaN");
  RouteArgs p{};
  p.pelvis = pelvis_loc; p.R = transf_rotmat; p.T = transf_transl; p.waypoints = waypoints; p.count = count; p.field_of = field_of;
  p.b = num_sequences; p.P = max_waypoints; p.radius = pass_radius;
  p.cursor = cursor; p.goal = goal; p.field_index = field_index; p.reached = reached; p.route_cursor = route_cursor;
  p.route_goal = route_goal; p.pass_dist = route_pass_dist;
  hipLaunchKernelGGL(egx_route_advance_kernel, dim3((unsigned)egx_ceil_div(num_sequences, RT_WAVES)), dim3(RT_BLK), 0,
                     static_cast<hipStream_t>(stream), p);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

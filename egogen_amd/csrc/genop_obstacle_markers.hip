// The marker model of recorded tracks in the primitive search (`generate_sequence_to_goal(obstacles=, obstacle_model="markers")`): the
// people of a `MovingObstacles` are their 67 world markers per absolute frame, not cylinders round the pelvis, and a candidate row is
// its own 67 blended markers in the world (egx_markers.h: what genop_joint_markers.hip makes of a row).  One launch per primitive,
// ahead of the selection:
//
//   egx_obstacle_marker_clearance   frame_clearance[r, f] = sqrt(min over the live tracks o and the 67 x 67 marker pairs of the squared
//                                   distance of row r at predicted frame f + 2 and track o at absolute frame clamp(frame0 + 2 + f,
//                                   0, T - 1)) - skin.  The selection entries egx_primitive_select_obstacle_markers /
//                                   egx_primitive_beam_select_obstacle_markers (genop.hip) read that table where the cylinder entries
//                                   compute their c_t; everything after c_t is theirs.
//
// One workgroup of 9 waves per row.  The row's 18 x 67 world markers are staged once in LDS as float4 (19.3 KB); a wave takes the
// frames w and w + 9.  The loop is bound by the arithmetic only if a read of LDS serves several distances (the finding of
// egx_pair_marker_dist_kernel), so a lane keeps marker `lane` of OB tracks of the frame in registers and walks the row's 67 markers,
// every lane reading one address (a broadcast): OB distances per read.  The tracks' markers 64..66 are held by lanes 0 .. 3 OB - 1
// and handed round by shuffles, against marker `lane` and (lanes 0..2) 64 + lane of the row.  A minimum does not depend on the order
// it is taken in, so any tiling gives the same bits.  No atomics, no spin waits, nothing passes between workgroups; the one barrier
// stands outside every loop, and every loop bound is a launch argument, a constant or the row's set's count: uniform in a workgroup.
#include <cmath>

#include "egx_markers.h"

namespace {

constexpr int NF = EGX_MK_FRAMES - EGX_MK_SEED;            // the 18 predicted frames
constexpr int OM_WAVES = 9, OM_BLK = OM_WAVES * 64;        // two frames per wave
constexpr int OB = 4;                                      // tracks a lane holds in registers at a time
constexpr int TAIL = EGX_MK - 64;                          // markers 64..66
static_assert(NF == 2 * OM_WAVES, "a wave takes frames w and w + 9");
static_assert(3 * OB <= 64 && TAIL == 3, "lanes 0 .. 3 OB - 1 hold the markers 64..66 of a block of tracks");
static_assert(sizeof(float4) * NF * EGX_MK <= 64 * 1024, "the row's markers fit one workgroup's LDS");

struct ClearArgs {
  const float* markers_proj;  // [rows*20,67,3]
  const float* Y_gen;         // [18,rows,201]
  const float* R0;            // [rows,9]
  const float* T0;            // [rows,3]
  const float* obs;           // [S,O_max,T,67,3] world markers per absolute frame
  const int* count;           // [S]
  const int* index;           // [groups] or null: set 0
  size_t rows;
  int per_group, S, O_max, T, frame0;
  float rf, skin;
  float* out;                 // [rows,18]
};

__device__ __forceinline__ float wave_min(float v) {   // every lane's partner chain ends in lane 0; min is order-free
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_down(v, o, 64));
  return v;
}

// marker j of a track's frame (q: its 67 x 3 floats); a track past the live ones is not there: NaN, which fminf drops
__device__ __forceinline__ float4 track_marker(const float* q, int j, bool live) {
  const float nan = __builtin_nanf("");
  float4 v;
  v.x = live ? q[3 * j + 0] : nan;
  v.y = live ? q[3 * j + 1] : nan;
  v.z = live ? q[3 * j + 2] : nan;
  v.w = 0.f;
  return v;
}

}  // namespace

__global__ __launch_bounds__(OM_BLK) void egx_obstacle_marker_clearance_kernel(ClearArgs p) {
  __shared__ float4 s_w[NF][EGX_MK];              // 19.3 KB: one read of 16 bytes per OB distances
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const size_t r = blockIdx.x;                    // < rows by the grid
  const int g = (int)(r / (size_t)p.per_group);
  const int set = p.index ? min(max(p.index[g], 0), p.S - 1) : 0;
  const int cnt = min(max(p.count[set], 0), min(p.O_max, EGX_MAX_OBSTACLES));

  for (int e = tid; e < NF * EGX_MK; e += OM_BLK)
    s_w[e / EGX_MK][e % EGX_MK] = egx_world_marker(p.markers_proj, p.Y_gen, p.R0, p.T0, p.rows, p.rf, r, EGX_MK_SEED + e / EGX_MK, e % EGX_MK);
  __syncthreads();

  for (int k = 0; k < 2; ++k) {
    const int f = w + k * OM_WAVES;
    const long long a = min(max((long long)p.frame0 + EGX_MK_SEED + f, 0LL), (long long)p.T - 1);
    const float4 a_lane = s_w[f][lane], a_more = s_w[f][lane < TAIL ? 64 + lane : lane];
    const bool bad = __any(a_lane.w != 0.f || a_more.w != 0.f);
    float least = __builtin_inff();
    for (int o0 = 0; o0 < cnt; o0 += OB) {
      float4 mine[OB];
      float d2[OB];
#pragma unroll
      for (int u = 0; u < OB; ++u) {
        const int o = min(o0 + u, cnt - 1);
        mine[u] = track_marker(p.obs + (((size_t)set * p.O_max + o) * p.T + (size_t)a) * EGX_MK_DIM, lane, o0 + u < cnt);
        d2[u] = __builtin_inff();
      }
      const int ou = min(lane / 3, OB - 1);       // lanes 0 .. 3 OB - 1 count
      const float4 more = track_marker(p.obs + (((size_t)set * p.O_max + min(o0 + ou, cnt - 1)) * p.T + (size_t)a) * EGX_MK_DIM,
                                       64 + lane % 3, o0 + ou < cnt);
      for (int m = 0; m < EGX_MK; ++m) {
        const float4 row = s_w[f][m];
#pragma unroll
        for (int u = 0; u < OB; ++u) d2[u] = fminf(d2[u], dist2(row, mine[u]));
      }
#pragma unroll
      for (int u = 0; u < OB; ++u) {
#pragma unroll
        for (int j = 0; j < TAIL; ++j) {
          float4 b;
          b.x = __shfl(more.x, 3 * u + j, 64); b.y = __shfl(more.y, 3 * u + j, 64); b.z = __shfl(more.z, 3 * u + j, 64); b.w = 0.f;
          d2[u] = fminf(d2[u], dist2(a_lane, b));
          if (lane < TAIL) d2[u] = fminf(d2[u], dist2(a_more, b));
        }
        least = fminf(least, d2[u]);
      }
    }
    least = wave_min(least);
    if (lane == 0) p.out[r * NF + f] = bad ? __builtin_nanf("") : egx_sub(sqrtf(least), p.skin);
  }
}

extern "C" int egx_obstacle_marker_clearance(const float* markers_proj, const float* Y_gen, float reproj_factor, const float* R0,
                                             const float* T0, int num_sequences, int rows_per_sequence, const float* obs_markers,
                                             const int32_t* obs_count, const int32_t* obs_index, int num_sets, int max_obstacles,
                                             int num_frames, int frame0, float skin, float* frame_clearance, void* stream) {
  EGX_REQUIRE(markers_proj && Y_gen && R0 && T0 && obs_markers && obs_count, "null input");
  EGX_REQUIRE(frame_clearance, "null output");
  EGX_REQUIRE(num_sequences > 0, "need a non-empty batch");
  EGX_REQUIRE(rows_per_sequence >= 1 && rows_per_sequence <= EGX_MAX_CANDIDATES, "rows_per_sequence must be in [1, EGX_MAX_CANDIDATES]");
  EGX_REQUIRE(reproj_factor >= 0.f && reproj_factor <= 1.f, "reproj_factor must be in [0, 1]");
  EGX_REQUIRE(max_obstacles >= 0 && max_obstacles <= EGX_MAX_OBSTACLES, "max_obstacles must be in [0, EGX_MAX_OBSTACLES]");
  EGX_REQUIRE(num_frames >= 1 && num_sets >= 1, "num_frames and num_sets must be at least 1");
  EGX_REQUIRE(skin >= 0.f && skin < __builtin_inff(), "skin must not be negative and must be finite");
  const long long rows = (long long)num_sequences * rows_per_sequence;
  EGX_REQUIRE(rows <= 0x7fffffffLL, "num_sequences * rows_per_sequence must stay below 2^31");
  ClearArgs p{};
  p.markers_proj = markers_proj; p.Y_gen = Y_gen; p.R0 = R0; p.T0 = T0; p.obs = obs_markers; p.count = obs_count; p.index = obs_index;
  p.rows = (size_t)rows; p.per_group = rows_per_sequence; p.S = num_sets; p.O_max = max_obstacles; p.T = num_frames; p.frame0 = frame0;
  p.rf = reproj_factor; p.skin = skin; p.out = frame_clearance;
  hipLaunchKernelGGL(egx_obstacle_marker_clearance_kernel, dim3((unsigned)rows), dim3(OM_BLK), 0, static_cast<hipStream_t>(stream), p);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

// Look-ahead against recorded tracks in the primitive search (`generate_sequence_to_goal(obstacles=, lookahead=H)`, H > 0, the
// cylinder model): a candidate row is predicted H further primitives ahead by repeating its own net displacement, the recorded
// people are read where their tracks say they will be.  One launch per primitive, ahead of the selection:
//
//   egx_obstacle_ahead_clearance   frame_clearance[r, f] = min(c_0, min_{h=1..H} max(0, c_h) + h * slack), c_h the cylinder clearance
//                                  (egx_obstacles.h) of p(t) + h * d, t = f + 2, d = p(19) - p(1), against the set's live tracks at
//                                  absolute frame clamp(frame0 + t + 18 h, 0, T - 1).  The selection entries
//                                  egx_primitive_select_obstacle_markers / egx_primitive_beam_select_obstacle_markers (genop.hip) read
//                                  that table where the cylinder entries compute their c_t; everything after c_t is theirs.
//
// A prediction can cost but only the present can veto: max(0, .) keeps a predicted overlap out of the colliding class.  c_0 is the
// cylinder entries' own c_t, same functions, same roundings: with H = 0 the table gives their bits.
//
// One workgroup of 8 waves per sequence.  The window of the sequence's set over all (H + 1) x 18 absolute frames - they are
// consecutive: clamp(frame0 + 2 + k, 0, T - 1), k = 18 h + f - is staged once into LDS (at most 9 x 18 x 32 xy and 32 radii, 41.6 KB);
// a wave takes one row at a time, lanes 0..17 one predicted frame each, looping over h; p(1) and p(19) are the same address in every
// lane.  A minimum does not depend on the order it is taken in, so the tiling does not reach the bits.  No atomics, no spin waits,
// nothing passes between workgroups; the one barrier stands outside every loop, and every loop bound is a launch argument, a constant
// or the set's count: uniform in a workgroup.
#include <cmath>

#include "egx_common.h"
#include "egx_obstacles.h"

namespace {

constexpr int NT = 20, THIS = 2, NF = EGX_OBS_FRAMES;
constexpr int OA_BLK = 512, OA_WAVES = OA_BLK / 64;
constexpr int WIN = (EGX_MAX_LOOKAHEAD + 1) * NF;           // frames of the longest window
static_assert(NT - THIS == NF && NF <= 64, "one lane per predicted frame");
static_assert(sizeof(float) * (2 * WIN + 1) * EGX_MAX_OBSTACLES <= 64 * 1024, "the window fits one workgroup's LDS");

struct AheadArgs {
  const float* joints;   // [rows*20,jpb,3]
  const float* R0;       // [rows,9]
  const float* T0;       // [rows,3]
  const float* xy;       // [S,O_max,T,2]
  const float* radius;   // [S,O_max]
  const int* count;      // [S]
  const int* index;      // [b] or null: set 0
  int M, jpb, S, O_max, T, frame0, H;
  float body_radius, slack;
  float* out;            // [rows,18]
};

// world xy of joint 0 of body t of a row, with the nesting of obstacle_group (genop.hip)
__device__ __forceinline__ void pelvis_xy(const AheadArgs& p, size_t row, int t, float& x, float& y) {
  const float* R0 = p.R0 + row * 9;
  const float* T0 = p.T0 + row * 3;
  const float* j = p.joints + (row * NT + t) * p.jpb * 3;
  x = fmaf(R0[2], j[2], fmaf(R0[1], j[1], R0[0] * j[0])) + T0[0];
  y = fmaf(R0[5], j[2], fmaf(R0[4], j[1], R0[3] * j[0])) + T0[1];
}

}  // namespace

__global__ __launch_bounds__(OA_BLK) void egx_obstacle_ahead_clearance_kernel(AheadArgs p) {
  __shared__ float s_x[WIN][EGX_MAX_OBSTACLES], s_y[WIN][EGX_MAX_OBSTACLES], s_rr[EGX_MAX_OBSTACLES];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, g = blockIdx.x;
  const int win = (p.H + 1) * NF;                  // <= WIN by the entry's check

  // egx_obstacles_stage over the longer window: the same clamps, the same rounded r_o + body_radius
  int cnt = 0;
  if (p.O_max >= 1) {
    const int set = p.index ? min(max(p.index[g], 0), p.S - 1) : 0;
    cnt = min(max(p.count[set], 0), min(p.O_max, EGX_MAX_OBSTACLES));
    for (int e = tid; e < win * cnt; e += OA_BLK) {
      const int k = e / cnt, o = e % cnt;
      const long long a = min(max((long long)p.frame0 + THIS + k, 0LL), (long long)p.T - 1);
      const float* q = p.xy + (((size_t)set * p.O_max + o) * p.T + (size_t)a) * 2;
      s_x[k][o] = q[0];
      s_y[k][o] = q[1];
    }
    for (int o = tid; o < cnt; o += OA_BLK) s_rr[o] = egx_add(p.radius[(size_t)set * p.O_max + o], p.body_radius);
  }
  __syncthreads();

  const int f = min(lane, NF - 1);                 // no branch round a load: the lanes past 17 read frame 19 again
  for (int n = w; n < p.M; n += OA_WAVES) {
    const size_t row = (size_t)g * p.M + n;
    float x, y, x1, y1, x19, y19;
    pelvis_xy(p, row, THIS + f, x, y);
    pelvis_xy(p, row, 1, x1, y1);
    pelvis_xy(p, row, NT - 1, x19, y19);
    const float dx = egx_sub(x19, x1), dy = egx_sub(y19, y1);
    float c = egx_obstacle_clearance(x, y, cnt, s_x[f], s_y[f], s_rr);
    bool bad = isnan(c);
    for (int h = 1; h <= p.H; ++h) {
      const float hf = (float)h;
      const float ch = egx_obstacle_clearance(egx_add(x, egx_mul(hf, dx)), egx_add(y, egx_mul(hf, dy)), cnt, s_x[h * NF + f], s_y[h * NF + f], s_rr);
      bad = bad || isnan(ch);                      // before the max: fmaxf(0, NaN) is 0
      c = fminf(c, egx_add(fmaxf(0.f, ch), egx_mul(hf, p.slack)));
    }
    if (lane < NF) p.out[row * NF + lane] = bad ? __builtin_nanf("") : c;
  }
}

extern "C" int egx_obstacle_ahead_clearance(const float* joints, int joints_per_body, const float* R0, const float* T0, int num_sequences,
                                            int rows_per_sequence, const float* obs_xy, const float* obs_radius, const int32_t* obs_count,
                                            const int32_t* obs_index, int num_sets, int max_obstacles, int num_frames, int frame0,
                                            float body_radius, int lookahead, float slack, float* frame_clearance, void* stream) {
  EGX_REQUIRE(joints && R0 && T0, "null input");
  EGX_REQUIRE(frame_clearance, "null output");
  EGX_REQUIRE(num_sequences > 0 && joints_per_body >= 1, "need a non-empty batch and at least one joint per body");
  EGX_REQUIRE(rows_per_sequence >= 1 && rows_per_sequence <= EGX_MAX_CANDIDATES, "rows_per_sequence must be in [1, EGX_MAX_CANDIDATES]");
  EGX_REQUIRE(max_obstacles >= 0 && max_obstacles <= EGX_MAX_OBSTACLES, "max_obstacles must be in [0, EGX_MAX_OBSTACLES]");
  EGX_REQUIRE(max_obstacles == 0 || (obs_xy && obs_radius && obs_count), "null obstacle input with max_obstacles > 0");
  EGX_REQUIRE(num_frames >= 1 && num_sets >= 1, "num_frames and num_sets must be at least 1");
  EGX_REQUIRE(lookahead >= 0 && lookahead <= EGX_MAX_LOOKAHEAD, "lookahead must be in [0, EGX_MAX_LOOKAHEAD]");
  EGX_REQUIRE(slack >= 0.f && slack < __builtin_inff(), "lookahead_slack must not be negative and must be finite");
  EGX_REQUIRE(body_radius >= 0.f && body_radius < __builtin_inff(), "body_radius must not be negative and must be finite");
  const long long rows = (long long)num_sequences * rows_per_sequence;
  EGX_REQUIRE(rows <= 0x7fffffffLL, "num_sequences * rows_per_sequence must stay below 2^31");
  const AheadArgs p{joints, R0, T0, obs_xy, obs_radius, obs_count, obs_index, rows_per_sequence, joints_per_body, num_sets, max_obstacles,
                    num_frames, frame0, lookahead, body_radius, slack, frame_clearance};
  hipLaunchKernelGGL(egx_obstacle_ahead_clearance_kernel, dim3((unsigned)num_sequences), dim3(OA_BLK), 0, static_cast<hipStream_t>(stream), p);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

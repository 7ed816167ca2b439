// The policy as the proposal distribution of the primitive search (egogen_amd/genop.py, `policy=`): two launches per primitive
// around egx_policy_forward.
//   egx_primitive_observe  the observation of one sequence as the env would have it after the chosen primitive
//                          (crowd_ppo/crowd_env_2f.py:311-312 what step() returns, :524-613 _calc_egosensing, :680-727 _get_feature),
//                          built from what the hand-off left on the device: the arithmetic of egx_env_step_post_kernel's sections
//                          5 (target distance), 6 (marker features) and 8 (egosensing), through the same device functions
//                          (egx_egosense.h, egx_reward.h, egx_frame.h)
//   egx_policy_propose     mu, logvar, eps -> the candidate rows of a sequence (crowd_ppo/ppo_policy.py:169-178, the
//                          reparameterised sample of egx_sample_action through the same device functions, egx_action.h)
// One workgroup per sequence, no atomics, nothing between workgroups: row i of every output depends on sequence i's inputs only.
#include "egx_action.h"
#include "egx_common.h"
#include "egx_egosense.h"
#include "egx_frame.h"
#include "egx_reward.h"

namespace {

constexpr int NM = 67, NJO = EGX_NUM_JOINTS_OUT, SD = 402, ZD = 128;
constexpr int OBS_BLK = 256;        // wave 0: the 64 (frame, ray) pairs in float64; waves 1..3: the 2 x 67 markers and the scalars
constexpr int LDS_EDGES = 1024;     // edges of one scene staged in LDS (16 KB); a larger scene is read from global memory

struct ObserveArgs {
  const float* joints;     // [rows * frames_per_row, 127, 3]
  int frames_per_row, first_frame;
  const int* choice;       // [b] or null (candidate 0)
  int N;
  const float *R_prev, *T_prev;   // [b,9] / [b,3]: the frame the joints are expressed in
  const float *R0, *T0;           // [b*N,9] / [b*N,3]: the new frame, read at row i * N
  const float *x0, *x1;           // the new seed frames, 201 values at row i * N of stride x_ld
  int x_ld;
  const float* goal;       // [b,3]
  const float* edges;      // [E,4] or null
  const int* edge_off;     // [S+1]
  const int* scene_idx;    // [b]
  int num_scenes;
  float ray_len;
  int step, max_depth;
  float *state, *ego, *dist, *time;
};

}  // namespace

__global__ __launch_bounds__(OBS_BLK) void egx_primitive_observe_kernel(ObserveArgs p) {
  __shared__ float s_edges[LDS_EDGES * 4];
  __shared__ int s_off[2];
  const int i = blockIdx.x, tid = threadIdx.x;
  int c = p.choice ? p.choice[i] : 0;
  c = c < 0 ? 0 : (c >= p.N ? p.N - 1 : c);
  const size_t row0 = (size_t)i * p.N;
  const float* J = p.joints + ((row0 + c) * p.frames_per_row + p.first_frame) * NJO * 3;   // the two seed bodies
  float R0o[9], T0o[3], R0n[9], T0n[3];
  for (int e = 0; e < 9; ++e) { R0o[e] = p.R_prev[(size_t)i * 9 + e]; R0n[e] = p.R0[row0 * 9 + e]; }
  for (int e = 0; e < 3; ++e) { T0o[e] = p.T_prev[(size_t)i * 3 + e]; T0n[e] = p.T0[row0 * 3 + e]; }
  const float wp[3] = {p.goal[(size_t)i * 3 + 0], p.goal[(size_t)i * 3 + 1], p.goal[(size_t)i * 3 + 2]};

  // ---- the scene's edges: once per workgroup into LDS ----------------------------------------------------------------------
  int ne = 0;
  const float* edges = nullptr;
  if (p.edges) {
    int sc_i = p.scene_idx[i];
    sc_i = sc_i < 0 ? 0 : (sc_i >= p.num_scenes ? p.num_scenes - 1 : sc_i);
    const int e0 = p.edge_off[sc_i];
    ne = p.edge_off[sc_i + 1] - e0;
    ne = ne < 0 ? 0 : ne;
    edges = p.edges + (size_t)e0 * 4;
    if (ne <= LDS_EDGES) {
      for (int e = tid; e < ne * 4; e += OBS_BLK) s_edges[e] = edges[e];
      edges = s_edges;
    }
    if (tid == 0) { s_off[0] = 0; s_off[1] = ne; }
  }
  __syncthreads();

  if (tid < 64) {
    // ---- egosensing from the world-frame eye joints of the two seed bodies: lane = (frame, ray) ----------------------------
    const int t = tid >> 5;
    float* out = p.ego + ((size_t)i * 2 + t) * NRAY;
    if (!p.edges) {
      // no polygon: the eye is inside an unbounded plane, no ray leaves it, d = ray_len
      const double ray_len = (double)p.ray_len;
      out[tid & 31] = -1.f + 2.f * (float)(ray_len / ray_len);
    } else {
      SceneDev sc;
      sc.edges = edges; sc.edge_off = s_off; sc.tris = nullptr; sc.tri_off = nullptr; sc.floor_h = nullptr; sc.map_lin = nullptr;
      sc.map_res = 0; sc.crowd_bbox = nullptr; sc.crowd_G = 0; sc.crowd_S = 0; sc.crowd_k = 0; sc.crowd_half = 0.f;
      sc.crowd_polygon = 0; sc.crowd_static = 0;
      const float* jt = J + (size_t)t * NJO * 3;
      float w23[3], w24[3], w56[3], w57[3];
      const int ids[4] = {23, 24, 56, 57};
      float* outs[4] = {w23, w24, w56, w57};
      for (int q = 0; q < 4; ++q) {
        // R_prev j + T_prev with the roundings the env step kernel's build gives `mat3_vec(...) + T0`: the middle product rounded,
        // the other two fused onto it, then one addition (with contraction left to the compiler the two kernels differ in the last bit)
        const float* v = jt + ids[q] * 3;
        for (int r = 0; r < 3; ++r)
          outs[q][r] = egx_add(fmaf(R0o[r * 3 + 2], v[2], fmaf(R0o[r * 3 + 0], v[0], egx_mul(R0o[r * 3 + 1], v[1]))), T0o[r]);
      }
      egosensing_frame(sc, 0, w23, w24, w56, w57, (double)p.ray_len, out, tid & 31, 32);
    }
  } else {
    // ---- state: the seed frames' canonical markers + unit vectors to the target in the NEW frame ---------------------------
    float tln[3];
    {
      const float v[3] = {wp[0] - T0n[0], wp[1] - T0n[1], wp[2] - T0n[2]};
      mat3T_vec(R0n, v, tln);
    }
    for (int k = tid - 64; k < 2 * NM; k += OBS_BLK - 64) {
      const int t = k / NM, m = k % NM;
      const float* x = (t ? p.x1 : p.x0) + row0 * p.x_ld + m * 3;
      const float ms[3] = {x[0], x[1], x[2]};
      float* st = p.state + ((size_t)i * 2 + t) * SD;
      st[m * 3 + 0] = ms[0]; st[m * 3 + 1] = ms[1]; st[m * 3 + 2] = ms[2];
      marker_target_feature(tln, ms, st + 201 + m * 3);
    }
    if (tid == OBS_BLK - 1) {
      // ---- dist, time: the last body's pelvis against the target in the frame the joints are expressed in -----------------
      const float* j19 = J + (size_t)NJO * 3;
      float tl[3];
      target_to_local(R0o, T0o, wp, tl);
      const float d2t = target_distance(tl, j19);
      p.dist[i] = 1.f / (d2t + 1.f);
      const int steps = p.step < p.max_depth ? p.step : p.max_depth;   // the policy never saw a step above max_depth
      p.time[i] = 1.f - (float)steps / (float)p.max_depth;
    }
  }
}

// one thread per float4 of z: 32 threads a row
__global__ __launch_bounds__(256) void egx_policy_propose_kernel(const float* __restrict__ mu, const float* __restrict__ logvar,
                                                                 const float* eps, float min_lv, float max_lv, int b, int N,
                                                                 int n_mean, int n_policy, float temperature, float* z) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)b * N * (ZD / 4)) return;
  const size_t row = idx / (ZD / 4);
  const int c4 = (int)(idx % (ZD / 4));
  const int i = (int)(row / N), n = (int)(row % N);
  float4* out = reinterpret_cast<float4*>(z) + idx;
  if (n >= n_policy) {   // the prior's sample, bit for bit
    if (z != eps) *out = reinterpret_cast<const float4*>(eps)[idx];
    return;
  }
  const float4 m = reinterpret_cast<const float4*>(mu)[(size_t)i * (ZD / 4) + c4];
  if (n < n_mean) {
    *out = m;
    return;
  }
  const float4 lv = reinterpret_cast<const float4*>(logvar)[(size_t)i * (ZD / 4) + c4];
  const float4 e = reinterpret_cast<const float4*>(eps)[idx];
  float4 r;
  r.x = egx_action_sample(m.x, egx_mul(temperature, egx_action_sigma(egx_action_clamp_logvar(lv.x, min_lv, max_lv))), e.x);
  r.y = egx_action_sample(m.y, egx_mul(temperature, egx_action_sigma(egx_action_clamp_logvar(lv.y, min_lv, max_lv))), e.y);
  r.z = egx_action_sample(m.z, egx_mul(temperature, egx_action_sigma(egx_action_clamp_logvar(lv.z, min_lv, max_lv))), e.z);
  r.w = egx_action_sample(m.w, egx_mul(temperature, egx_action_sigma(egx_action_clamp_logvar(lv.w, min_lv, max_lv))), e.w);
  *out = r;
}

extern "C" int egx_primitive_observe(const float* joints, int frames_per_row, int first_frame, const int32_t* choice, int num_candidates,
                                     const float* R_prev, const float* T_prev, const float* R0, const float* T0, const float* x0,
                                     const float* x1, int x_ld, const float* goal, const float* edges, const int32_t* edge_off,
                                     const int32_t* scene_idx, int num_scenes, float ray_len, int step, int max_depth,
                                     int num_sequences, float* state, float* egosensing, float* dist, float* time, void* stream) {
  EGX_REQUIRE(joints && R_prev && T_prev && R0 && T0 && x0 && x1 && goal && state && egosensing && dist && time, "null argument");
  EGX_REQUIRE(num_sequences > 0 && num_candidates >= 1 && num_candidates <= EGX_MAX_CANDIDATES, "empty batch or bad num_candidates");
  EGX_REQUIRE(frames_per_row >= 2 && first_frame >= 0 && first_frame + 2 <= frames_per_row, "the two seed bodies must lie inside a row");
  EGX_REQUIRE(x_ld >= 201, "x_ld must hold the 201 marker coordinates");
  EGX_REQUIRE((edges && edge_off && scene_idx && num_scenes >= 1) || (!edges && !edge_off && !scene_idx),
              "edges, edge_off and scene_idx: all three or none");
  EGX_REQUIRE(ray_len > 0.f && step >= 0 && max_depth >= 1, "ray_len and max_depth must be positive, step not negative");
  ObserveArgs p;
  p.joints = joints; p.frames_per_row = frames_per_row; p.first_frame = first_frame; p.choice = choice; p.N = num_candidates;
  p.R_prev = R_prev; p.T_prev = T_prev; p.R0 = R0; p.T0 = T0; p.x0 = x0; p.x1 = x1; p.x_ld = x_ld; p.goal = goal;
  p.edges = edges; p.edge_off = edge_off; p.scene_idx = scene_idx; p.num_scenes = num_scenes; p.ray_len = ray_len; p.step = step;
  p.max_depth = max_depth; p.state = state; p.ego = egosensing; p.dist = dist; p.time = time;
  hipLaunchKernelGGL(egx_primitive_observe_kernel, dim3(num_sequences), dim3(OBS_BLK), 0, static_cast<hipStream_t>(stream), p);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

extern "C" int egx_policy_propose(const float* mu, const float* logvar, const float* eps, float min_logvar, float max_logvar,
                                  int num_sequences, int num_candidates, int n_mean, int n_policy, float temperature, float* z,
                                  void* stream) {
  EGX_REQUIRE(mu && logvar && eps && z, "null argument");
  EGX_REQUIRE(num_sequences > 0 && num_candidates >= 1 && num_candidates <= EGX_MAX_CANDIDATES, "empty batch or bad num_candidates");
  EGX_REQUIRE(0 <= n_mean && n_mean <= n_policy && n_policy <= num_candidates, "need 0 <= n_mean <= n_policy <= num_candidates");
  EGX_REQUIRE(temperature >= 0.f && min_logvar <= max_logvar, "temperature must not be negative (or NaN), min_logvar <= max_logvar");
  EGX_REQUIRE(((uintptr_t)mu | (uintptr_t)logvar | (uintptr_t)eps | (uintptr_t)z) % 16 == 0, "mu, logvar, eps and z must be 16-byte aligned");
  const size_t n4 = (size_t)num_sequences * num_candidates * (ZD / 4);
  hipLaunchKernelGGL(egx_policy_propose_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), mu,
                     logvar, eps, min_logvar, max_logvar, num_sequences, num_candidates, n_mean, n_policy, temperature, z);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

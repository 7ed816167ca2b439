// The policy as the proposal distribution of the primitive search (egogen_amd/genop.py, `policy=`, egogen_amd/proposal.py): the
// launches of a primitive around egx_policy_forward.
//   egx_primitive_observe  the observation of one sequence as the env would have it after the chosen primitive
//                          (crowd_ppo/crowd_env_2f.py:311-312 what step() returns, :524-613 _calc_egosensing, :680-727 _get_feature),
//                          built from what the hand-off left on the device: the arithmetic of egx_env_step_post_kernel's sections
//                          5 (target distance), 6 (marker features) and 8 (egosensing), through the same device functions
//                          (egx_egosense.h, egx_reward.h, egx_frame.h)
//   egx_policy_propose     mu, logvar, eps -> the candidate rows of a sequence (crowd_ppo/ppo_policy.py:169-178, the
//                          reparameterised sample of egx_sample_action through the same device functions, egx_action.h)
// and, in a crowd call with `sense_people=True`, the people of a sequence's group and its obstacle tracks as holes of the walkable
// polygon the rays are cast against, as in the reference's crowd evaluation (crowd_env_crowd_eval.py:345-352 the world xy box of
// the two seed frames' markers; dummy_vector_env.py:34-39,81-84 the other agents' boxes as holes; :796-820 egosensing against that
// polygon):
//   egx_primitive_people_boxes   per sequence the box (minx, miny, maxx, maxy) of the world xy of the 2 x 67 markers of its seed
//                                frames, one wave per sequence, min / max by wave shuffles
//   egx_primitive_observe_people egx_primitive_observe with the rays cast against the static polygon minus the union of the
//                                group-mates' boxes and the boxes of the obstacle tracks at the two seed frames (HoleEdges,
//                                egx_egosense.h)
// The two observe kernels are one body, observe_body<PEOPLE>: the holes are staged only where they are compiled in, and
// everything else, the rays of a sequence without a hole included, is the same code on the same inputs.
// One workgroup per sequence, no atomics, nothing between workgroups: row i of every output depends on sequence i's inputs, its
// mates' box rows and its obstacle set.  These are latency-bound launches of b small workgroups: the holes and the static edges are
// staged in LDS once, and nothing beyond that is optimised (profiles/genop_policy_people.md).
#include "egx_action.h"
#include "egx_common.h"
#include "egx_egosense.h"
#include "egx_frame.h"
#include "egx_reward.h"

namespace {

constexpr int NM = 67, NJO = EGX_NUM_JOINTS_OUT, SD = 402, ZD = 128;
constexpr int OBS_BLK = 256;        // wave 0: the holes, then the 64 (frame, ray) pairs in float64; waves 1..3: the 2 x 67 markers and the scalars
constexpr int LDS_EDGES = 1024;     // edges of one scene staged in LDS (16 KB); a larger scene is read from global memory
constexpr int MAXP = EGX_MAX_GROUP, MAXO = EGX_MAX_OBSTACLES;
constexpr int MAX_HOLES = MAXP + MAXO;   // 31 mates + 32 tracks where the sequence is a member of its own group, one more where not
constexpr int BOX_BLK = 256, BOX_WAVES = BOX_BLK / 64;
static_assert(MAX_HOLES <= 64, "one lane of wave 0 per hole");

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

// what egx_primitive_observe_people reads beyond ObserveArgs
struct PeopleArgs {
  int b;
  const float* box;           // [b,4] or null
  const int* group_start;     // [G+1] or null
  const int* group_member;    // [group_start[G]]
  const int* member_group;    // [b]
  int G;
  const float* obs_xy;        // [S,O_max,T,2] or null
  const float* obs_radius;    // [S,O_max]
  const int* obs_count;       // [S]
  const int* obs_index;       // [b] or null: set 0
  int obs_S, O_max, T, frame;
  int* people_count;          // [b]
};

__device__ __forceinline__ float wave_min_all(float v) {   // every lane holds the result; min / max are order-free
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max_all(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

}  // namespace

// one wave per sequence: lane l holds the markers l, l + 64, l + 128 (< 134) of the two seed frames
__global__ __launch_bounds__(BOX_BLK) void egx_primitive_people_boxes_kernel(const float* __restrict__ x0, const float* __restrict__ x1,
                                                                             int x_ld, const float* __restrict__ R0,
                                                                             const float* __restrict__ T0, int N, int b, float* box) {
  const int i = blockIdx.x * BOX_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= b) return;                                   // the same in every lane of the wave
  const size_t row0 = (size_t)i * N;
  const float* R = R0 + row0 * 9;
  const float* T = T0 + row0 * 3;
  const float r0 = R[0], r1 = R[1], r2 = R[2], r3 = R[3], r4 = R[4], r5 = R[5], tx = T[0], ty = T[1];
  float lox = __builtin_inff(), loy = __builtin_inff(), hix = -__builtin_inff(), hiy = -__builtin_inff();
  int bad = 0;
  for (int k = lane; k < 2 * NM; k += 64) {
    const int t = k / NM, m = k % NM;
    const float* v = (t ? x1 : x0) + row0 * x_ld + m * 3;
    // the nesting of the obstacle entries' world pelvis: the first product rounded, two fused onto it, one rounded addition
    const float wx = egx_add(fmaf(r2, v[2], fmaf(r1, v[1], egx_mul(r0, v[0]))), tx);
    const float wy = egx_add(fmaf(r5, v[2], fmaf(r4, v[1], egx_mul(r3, v[0]))), ty);
    bad |= (isfinite(wx) && isfinite(wy)) ? 0 : 1;      // fminf / fmaxf would drop a NaN
    lox = fminf(lox, wx); hix = fmaxf(hix, wx);
    loy = fminf(loy, wy); hiy = fmaxf(hiy, wy);
  }
  lox = wave_min_all(lox); loy = wave_min_all(loy);
  hix = wave_max_all(hix); hiy = wave_max_all(hiy);
  const bool any_bad = __ballot(bad) != 0ull;
  if (lane == 0) {
    const float nan = __builtin_nanf("");
    float* o = box + (size_t)i * 4;
    o[0] = any_bad ? nan : lox; o[1] = any_bad ? nan : loy; o[2] = any_bad ? nan : hix; o[3] = any_bad ? nan : hiy;
  }
}

namespace {

// the body of both observe kernels; without PEOPLE `h` is not looked at
template <bool PEOPLE>
__device__ __forceinline__ void observe_body(const ObserveArgs& p, const PeopleArgs& h) {
  __shared__ float s_edges[LDS_EDGES * 4];
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
  }

  int nbox = 0;
  const float* boxes = nullptr;
  if constexpr (PEOPLE) {
    // ---- the holes: wave 0, lanes 0..31 the members of the group, lanes 32..63 the tracks of the obstacle set ---------------
    __shared__ float s_box[MAX_HOLES * 4];
    __shared__ int s_nbox;
    if (tid < 64) {
      float lox = 0.f, loy = 0.f, hix = 0.f, hiy = 0.f;
      bool have = false;
      if (tid < MAXP) {
        if (h.group_start) {
          // membership clamped as egx_primitive_select_joint clamps it
          int g = h.member_group[i];
          g = min(max(g, 0), h.G - 1);
          const int total = max(h.group_start[h.G], 0);
          const int start = min(max(h.group_start[g], 0), total);
          const int P = min(min(max(h.group_start[g + 1], start), total) - start, MAXP);
          if (tid < P) {
            const int m = min(max(h.group_member[start + tid], 0), h.b - 1);
            if (m != i) {
              const float* q = h.box + (size_t)m * 4;
              lox = q[0]; loy = q[1]; hix = q[2]; hiy = q[3];
              have = true;
            }
          }
        }
      } else if (h.obs_xy && h.O_max >= 1) {
        // the set and its live tracks clamped as egx_obstacles_stage clamps them; a track is held outside its frames
        const int o = tid - MAXP;
        const int set = h.obs_index ? min(max(h.obs_index[i], 0), h.obs_S - 1) : 0;
        const int cnt = min(max(h.obs_count[set], 0), min(h.O_max, MAXO));
        if (o < cnt) {
          const float r = h.obs_radius[(size_t)set * h.O_max + o];
          const long long fa = min(max((long long)h.frame, 0LL), (long long)h.T - 1);
          const long long fb = min(max((long long)h.frame + 1, 0LL), (long long)h.T - 1);
          const float* qa = h.obs_xy + (((size_t)set * h.O_max + o) * h.T + (size_t)fa) * 2;
          const float* qb = h.obs_xy + (((size_t)set * h.O_max + o) * h.T + (size_t)fb) * 2;
          const float ax = qa[0], ay = qa[1], bx = qb[0], by = qb[1];
          lox = fminf(egx_sub(ax, r), egx_sub(bx, r)); hix = fmaxf(egx_add(ax, r), egx_add(bx, r));
          loy = fminf(egx_sub(ay, r), egx_sub(by, r)); hiy = fmaxf(egx_add(ay, r), egx_add(by, r));
          have = !(isnan(ax) || isnan(ay) || isnan(bx) || isnan(by) || isnan(r));     // fminf / fmaxf would drop a NaN
        }
      }
      have = have && isfinite(lox) && isfinite(loy) && isfinite(hix) && isfinite(hiy);   // a box with a non-finite entry is skipped
      const unsigned long long mask = __ballot(have);
      if (have) {                                          // compacted in lane order: no atomics
        const int at = __popcll(mask & ((1ull << tid) - 1ull));
        s_box[at * 4 + 0] = lox; s_box[at * 4 + 1] = loy; s_box[at * 4 + 2] = hix; s_box[at * 4 + 3] = hiy;
      }
      if (tid == 0) {
        const int n = __popcll(mask);
        s_nbox = n;
        h.people_count[i] = n;
      }
    }
    __syncthreads();
    boxes = s_box;
    nbox = s_nbox;
  } else {
    __syncthreads();   // one barrier either way: the edges are staged, and with PEOPLE the holes
  }

  if (tid < 64) {
    // ---- egosensing from the world-frame eye joints of the two seed bodies: lane = (frame, ray) ----------------------------
    const int t = tid >> 5;
    float* out = p.ego + ((size_t)i * 2 + t) * NRAY;
    if (!p.edges && nbox == 0) {
      // no polygon, no hole: the eye is inside an unbounded plane, no ray leaves it, d = ray_len
      const double ray_len = (double)p.ray_len;
      out[tid & 31] = -1.f + 2.f * (float)(ray_len / ray_len);
    } else {
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
      egosensing_rays(HoleEdges{edges, ne, boxes, nbox}, w23, w24, w56, w57, (double)p.ray_len, out, tid & 31, 32);
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

}  // namespace

__global__ __launch_bounds__(OBS_BLK) void egx_primitive_observe_kernel(ObserveArgs p) { observe_body<false>(p, PeopleArgs{}); }
__global__ __launch_bounds__(OBS_BLK) void egx_primitive_observe_people_kernel(ObserveArgs p, PeopleArgs h) { observe_body<true>(p, h); }

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

namespace {

// what the two observe entries share (as advance_entry and select_entry of genop.hip): the common checks, the common fields and
// the launch check; launch(p) is the entry's own kernel
template <class Launch>
int observe_entry(const float* joints, int frames_per_row, int first_frame, const int32_t* choice, int num_candidates,
                  const float* R_prev, const float* T_prev, const float* R0, const float* T0, const float* x0, const float* x1,
                  int x_ld, const float* goal, const float* edges, const int32_t* edge_off, const int32_t* scene_idx, int num_scenes,
                  float ray_len, int step, int max_depth, int num_sequences, float* state, float* egosensing, float* dist, float* time,
                  Launch launch) {
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
  launch(p);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

}  // namespace

extern "C" int egx_primitive_observe(const float* joints, int frames_per_row, int first_frame, const int32_t* choice, int num_candidates,
                                     const float* R_prev, const float* T_prev, const float* R0, const float* T0, const float* x0,
                                     const float* x1, int x_ld, const float* goal, const float* edges, const int32_t* edge_off,
                                     const int32_t* scene_idx, int num_scenes, float ray_len, int step, int max_depth,
                                     int num_sequences, float* state, float* egosensing, float* dist, float* time, void* stream) {
  EGX_REQUIRE(joints && R_prev && T_prev && R0 && T0 && x0 && x1 && goal && state && egosensing && dist && time, "null argument");
  return observe_entry(joints, frames_per_row, first_frame, choice, num_candidates, R_prev, T_prev, R0, T0, x0, x1, x_ld, goal, edges,
                       edge_off, scene_idx, num_scenes, ray_len, step, max_depth, num_sequences, state, egosensing, dist, time,
                       [&](const ObserveArgs& p) {
    hipLaunchKernelGGL(egx_primitive_observe_kernel, dim3(num_sequences), dim3(OBS_BLK), 0, static_cast<hipStream_t>(stream), p);
  });
}

extern "C" int egx_primitive_people_boxes(const float* x0, const float* x1, int x_ld, const float* R0, const float* T0,
                                          int num_candidates, int num_sequences, float* box, void* stream) {
  EGX_REQUIRE(x0 && x1 && R0 && T0 && box, "null argument");
  EGX_REQUIRE(num_sequences > 0 && num_candidates >= 1 && num_candidates <= EGX_MAX_CANDIDATES, "empty batch or bad num_candidates");
  EGX_REQUIRE(x_ld >= 201, "x_ld must hold the 201 marker coordinates");
  hipLaunchKernelGGL(egx_primitive_people_boxes_kernel, dim3((unsigned)((num_sequences + BOX_WAVES - 1) / BOX_WAVES)), dim3(BOX_BLK), 0,
                     static_cast<hipStream_t>(stream), x0, x1, x_ld, R0, T0, num_candidates, num_sequences, box);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

extern "C" int egx_primitive_observe_people(const float* joints, int frames_per_row, int first_frame, const int32_t* choice,
                                            int num_candidates, const float* R_prev, const float* T_prev, const float* R0,
                                            const float* T0, const float* x0, const float* x1, int x_ld, const float* goal,
                                            const float* edges, const int32_t* edge_off, const int32_t* scene_idx, int num_scenes,
                                            float ray_len, int step, int max_depth, int num_sequences, const float* box,
                                            const int32_t* group_start, const int32_t* group_member, const int32_t* member_group,
                                            int num_groups, const float* obs_xy, const float* obs_radius, const int32_t* obs_count,
                                            const int32_t* obs_index, int num_sets, int max_obstacles, int num_frames, int frame,
                                            int32_t* people_count, float* state, float* egosensing, float* dist, float* time,
                                            void* stream) {
  EGX_REQUIRE(joints && R_prev && T_prev && R0 && T0 && x0 && x1 && goal && people_count && state && egosensing && dist && time,
              "null argument");
  EGX_REQUIRE((group_start && group_member && member_group && num_groups >= 1) || (!group_start && !group_member && !member_group),
              "group_start, group_member and member_group: all three (with num_groups >= 1) or none");
  EGX_REQUIRE(box || !group_start, "groups need the boxes of egx_primitive_people_boxes");
  EGX_REQUIRE(max_obstacles >= 0 && max_obstacles <= EGX_MAX_OBSTACLES, "max_obstacles must be in [0, EGX_MAX_OBSTACLES]");
  EGX_REQUIRE((obs_xy && obs_radius && obs_count && num_sets >= 1) || (!obs_xy && !obs_radius && !obs_count && !obs_index),
              "obs_xy, obs_radius and obs_count: all three (with num_sets >= 1) or none, and no obs_index without them");
  EGX_REQUIRE(!obs_xy || num_frames >= 1, "num_frames must be at least 1 with obstacles");
  PeopleArgs h;
  h.b = num_sequences;
  h.box = box; h.group_start = group_start; h.group_member = group_member; h.member_group = member_group; h.G = num_groups;
  h.obs_xy = obs_xy; h.obs_radius = obs_radius; h.obs_count = obs_count; h.obs_index = obs_index; h.obs_S = num_sets;
  h.O_max = max_obstacles; h.T = num_frames; h.frame = frame; h.people_count = people_count;
  return observe_entry(joints, frames_per_row, first_frame, choice, num_candidates, R_prev, T_prev, R0, T0, x0, x1, x_ld, goal, edges,
                       edge_off, scene_idx, num_scenes, ray_len, step, max_depth, num_sequences, state, egosensing, dist, time,
                       [&](const ObserveArgs& p) {
    hipLaunchKernelGGL(egx_primitive_observe_people_kernel, dim3(num_sequences), dim3(OBS_BLK), 0, static_cast<hipStream_t>(stream), p, h);
  });
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

// The joint step of the greedy primitive search (egx_primitive_select_joint): one launch between the selection
// (egx_primitive_select, _field or _obstacles: genop.hip) and the hand-off (egx_primitive_advance_select), in which the people of
// one scene and time line - a group of up to EGX_MAX_GROUP sequences of the launch - choose again against each other's CURRENT
// choices.  One workgroup per group holds, in LDS, the world xy of the pelvis of every member's chosen row at the 18 predicted
// frames (the table), and runs `sweeps` Gauss-Seidel sweeps over the members in order: every candidate row of member i gets the
// clearance term of egx_obstacles.h against the other columns of the table (egx_pair_clearance), added to the cost the selection
// wrote; member i takes the first row in the selection's total order (key_before), and its column of the table is rewritten before
// member i + 1 is visited.  All sweeps always run: every trip count and barrier is workgroup-uniform.  No float atomics, no spin
// waits, nothing passes between workgroups: a group's outputs are the same bits in any batch.
//
// A member step is a chain of latencies, not of work: the rows' inputs from memory, the clearances against the table, three wave
// reductions per row, the choice by wave 0, two barriers.  So the inputs of four rows of a wave are read in one batch with no
// branch between the loads, the world xy of the visited member's rows stays in LDS (37 KB) and the winner's column is copied from
// there instead of being read and computed again, and the table's rows are 33 floats apart (no bank conflicts between the frames).
//
// A translation unit of its own: profiles/geodesic.md records how code placed next to score_group changes the last bits of the
// selection kernels, so nothing here is compiled together with them; the four small helpers the selection kernels keep in their
// anonymous namespace (wave_sum, wave_min, wave_max, key_before) are restated below, same trees, same order.
#include <cmath>

#include "egx_common.h"
#include "egx_obstacles.h"
#include "egx_reward.h"

namespace {

constexpr int NT = 20, THIS = 2;
constexpr int JOINT_BLK = 512, JOINT_WAVES = JOINT_BLK / 64;   // as SEL_BLK of genop.hip: 8 waves, one candidate row per wave at a time
constexpr int MAXC = EGX_MAX_CANDIDATES, MAXP = EGX_MAX_GROUP;
constexpr int TAB_LD = MAXP + 1;   // row stride of the table: lane t reads row t, 33 floats apart keeps the 18 lanes on 18 banks
constexpr int ROW_LD = EGX_OBS_FRAMES;   // the visited member's rows: lane t writes and reads frame t of a row, consecutive floats
constexpr int ROWS_AHEAD = 4;            // rows of a wave whose inputs are in flight together: N <= 32 is one batch per member step
static_assert(EGX_OBS_FRAMES == NT - THIS, "the table holds the predicted frames of a primitive");
static_assert(EGX_OBS_FRAMES <= 64 && MAXP <= JOINT_BLK, "one lane per frame, one thread per member");

struct JointArgs {
  const float* joints;        // [b*N*20,jpb,3]
  const float* R0;            // [b*N,9]
  const float* T0;            // [b*N,3]
  const float* goal;          // [b,3]
  const float* cost;          // [b*N]    what the selection wrote, read only
  const float* terms;         // [b*N,5]
  const int* colliding;       // [b*N]
  const int* group_start;     // [G+1]
  const int* group_member;    // [group_start[G]] sequence indices
  int b, N, jpb, G, S;
  float w, margin, rr, goal_thresh;
  int* choice;                // [b] in: the selection's, out: the joint choice
  int* status;                // [b]
  int* reached;               // [b] rewritten where the choice changed
  float* goal_dist;           // [b]
  float* pair_term;           // [S,b*N] traces
  float* pair_clearance;
  float* joint_cost;
  int* pair_hit;
  int* choice_trace;          // [S,b]
  int* changed;               // [S,G]
  float* crowd_clearance;     // [b]
  int* crowd_hit;             // [b]
};

__device__ __forceinline__ float wave_sum(float v) {   // lane 0 holds the sum; the fixed tree of the selection kernels
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_down(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_down(v, o, 64));
  return v;
}
// the total order of the greedy selection: class, then cost, then row index
__device__ __forceinline__ bool key_before(int ca, float xa, int ia, int cb, float xb, int ib) {
  if (ca != cb) return ca < cb;
  if (xa != xb) return xa < xb;
  return ia < ib;
}

// world xy of joint 0 of body t of a row, with the nesting of field_row_cost / obstacle_group (genop.hip)
__device__ __forceinline__ void pelvis_xy(const JointArgs& p, size_t row, int t, float& x, float& y) {
  const float* R0 = p.R0 + row * 9;
  const float* T0 = p.T0 + row * 3;
  const float* j = p.joints + (row * NT + t) * p.jpb * 3;
  x = fmaf(R0[2], j[2], fmaf(R0[1], j[1], R0[0] * j[0])) + T0[0];
  y = fmaf(R0[5], j[2], fmaf(R0[4], j[1], R0[3] * j[0])) + T0[1];
}

// What a wave makes of one track against the table: lanes 0..17 hold the frame clearances c_t of (x, y) against every column but
// `skip`; lane 0 returns term = (sum_t max(0, margin - c_t)) / 18 by the wave_sum tree and clearance = min_t c_t; a NaN frame
// makes both NaN (obstacle_group's arithmetic).
__device__ __forceinline__ void track_terms(float x, float y, bool live, int cnt, int skip, const float* s_x, const float* s_y, float rr,
                                            float margin, float& term, float& clearance) {
  float c = __builtin_inff(), pen = 0.f;
  int bad = 0;
  if (live) {
    c = egx_pair_clearance(x, y, cnt, skip, s_x, s_y, rr);
    bad = isnan(c) ? 1 : 0;
    pen = bad ? c : fmaxf(0.f, egx_sub(margin, c));
  }
  const float sum = wave_sum(pen);
  const float cmin = wave_min(bad ? __builtin_inff() : c);
  const int any_bad = wave_max(bad);
  term = sum / (float)EGX_OBS_FRAMES;
  clearance = any_bad ? __builtin_nanf("") : cmin;
}

}  // namespace

__global__ __launch_bounds__(JOINT_BLK) void egx_primitive_select_joint_kernel(JointArgs p) {
  __shared__ float s_x[EGX_OBS_FRAMES][TAB_LD], s_y[EGX_OBS_FRAMES][TAB_LD];   // [frame][member]: the chosen tracks
  __shared__ float s_rx[MAXC][ROW_LD], s_ry[MAXC][ROW_LD];                     // [row][frame]: the rows of the member being visited, 37 KB
  __shared__ float s_cost[MAXC];
  __shared__ int s_cls[MAXC];
  __shared__ int s_member[MAXP], s_choice[MAXP], s_first[MAXP], s_chosen_cls[MAXP];
  const int g = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63, N = p.N;
  const size_t rows = (size_t)p.b * N;

  // membership: start and size clamped into the member list, the size to EGX_MAX_GROUP, every index into [0, b)
  const int total = max(p.group_start[p.G], 0);
  const int start = min(max(p.group_start[g], 0), total);
  const int P = min(min(max(p.group_start[g + 1], start), total) - start, MAXP);
  if (tid < P) {
    const int m = min(max(p.group_member[start + tid], 0), p.b - 1);
    const int c = min(max(p.choice[m], 0), N - 1);
    s_member[tid] = m;
    s_choice[tid] = c;
    s_first[tid] = c;
    s_chosen_cls[tid] = 0;
  }
  __syncthreads();
  for (int e = tid; e < EGX_OBS_FRAMES * P; e += JOINT_BLK) {
    const int f = e / P, j = e % P;
    pelvis_xy(p, (size_t)s_member[j] * N + s_choice[j], THIS + f, s_x[f][j], s_y[f][j]);
  }
  __syncthreads();

  for (int s = 0; s < p.S; ++s) {
    int nchanged = 0;                                    // lane 0 of wave 0 counts
    for (int i = 0; i < P; ++i) {
      const int m = s_member[i];
      // A wave takes a row at a time, lanes 0..17 one frame each; ROWS_AHEAD rows of a wave are read before the first is scored,
      // what lane 0 needs of a row (cost, terms, colliding) with them: one trip to memory per batch, not two per row.
      for (int n0 = w; n0 < N; n0 += JOINT_WAVES * ROWS_AHEAD) {
        const bool live = lane < EGX_OBS_FRAMES;
        float x[ROWS_AHEAD], y[ROWS_AHEAD], base[ROWS_AHEAD];
        bool fin[ROWS_AHEAD], coll[ROWS_AHEAD];
#pragma unroll
        for (int u = 0; u < ROWS_AHEAD; ++u) {
          const int n = n0 + u * JOINT_WAVES;
          const size_t row = (size_t)m * N + min(n, N - 1);
          pelvis_xy(p, row, THIS + min(lane, EGX_OBS_FRAMES - 1), x[u], y[u]);      // no branch round a load: the lanes past 17 read frame 19 again
          const float* tm = p.terms + row * 5;
          const float t0 = tm[0], t1 = tm[1], t2 = tm[2], t3 = tm[3], t4 = tm[4];
          base[u] = p.cost[row];
          coll[u] = p.colliding[row] != 0;
          fin[u] = isfinite(base[u]) & isfinite(t0) & isfinite(t1) & isfinite(t2) & isfinite(t3) & isfinite(t4);   // & not &&: no load waits for a branch
        }
#pragma unroll
        for (int u = 0; u < ROWS_AHEAD; ++u) {
          const int n = n0 + u * JOINT_WAVES;
          if (n >= N) break;                             // the same in every lane of the wave
          const size_t row = (size_t)m * N + n;
          float term, clearance;
          track_terms(x[u], y[u], live, P, i, s_x[live ? lane : 0], s_y[live ? lane : 0], p.rr, p.margin, term, clearance);
          if (live) {                                    // kept for the rewrite of the table
            s_rx[n][lane] = x[u];
            s_ry[n][lane] = y[u];
          }
          if (lane == 0) {
            const bool hit = clearance < 0.f;            // false for NaN
            const float jc = egx_add(base[u], egx_mul(p.w, term));
            const bool finite = fin[u] && isfinite(term) && isfinite(jc);
            const size_t at = (size_t)s * rows + row;
            p.pair_term[at] = term;
            p.pair_clearance[at] = clearance;
            p.joint_cost[at] = jc;
            p.pair_hit[at] = hit ? 1 : 0;
            s_cost[n] = finite ? jc : 0.f;               // a non-finite row is ranked by collision and index only
            s_cls[n] = (finite ? 0 : 2) | (coll[u] ? 1 : 0) | (hit ? 1 : 0);
          }
        }
      }
      __syncthreads();
      if (w == 0) {                                      // the reduction of egx_primitive_select_kernel
        int bc = 4, bi = 0x7fffffff;
        float bx = 0.f;
        for (int n = lane; n < N; n += 64)
          if (key_before(s_cls[n], s_cost[n], n, bc, bx, bi)) { bc = s_cls[n]; bx = s_cost[n]; bi = n; }
        for (int o = 32; o > 0; o >>= 1) {
          const int oc = __shfl_xor(bc, o, 64), oi = __shfl_xor(bi, o, 64);
          const float ox = __shfl_xor(bx, o, 64);
          if (key_before(oc, ox, oi, bc, bx, bi)) { bc = oc; bx = ox; bi = oi; }
        }
        if (lane < EGX_OBS_FRAMES) {                     // every lane holds the winner: column i of the table follows it
          s_x[lane][i] = s_rx[bi][lane];
          s_y[lane][i] = s_ry[bi][lane];
        }
        if (lane == 0) {
          nchanged += (bi != s_choice[i]) ? 1 : 0;
          s_choice[i] = bi;
          s_chosen_cls[i] = bc;
          p.choice_trace[(size_t)s * p.b + m] = bi;
        }
      }
      __syncthreads();
    }
    if (tid == 0) p.changed[(size_t)s * p.G + g] = nchanged;
  }

  // the crowd as written: every member's final track against the others' final tracks
  for (int i = w; i < P; i += JOINT_WAVES) {
    const bool live = lane < EGX_OBS_FRAMES;
    float term, clearance;
    track_terms(live ? s_x[lane][i] : 0.f, live ? s_y[lane][i] : 0.f, live, P, i, s_x[live ? lane : 0], s_y[live ? lane : 0], p.rr,
                p.margin, term, clearance);
    if (lane == 0) {
      p.crowd_clearance[s_member[i]] = clearance;
      p.crowd_hit[s_member[i]] = (clearance < 0.f) ? 1 : 0;
    }
  }
  if (tid < P) {
    const int m = s_member[tid], c = s_choice[tid], cls = s_chosen_cls[tid];
    p.choice[m] = c;
    p.status[m] = (cls & 1) | (cls >= 2 ? 2 : 0);
    if (c != s_first[tid]) {                             // the distance of the new row, as score_group calls for it
      const size_t row = (size_t)m * N + c;
      const float* j19 = p.joints + (row * NT + 19) * p.jpb * 3;
      float tl[3], dir[2];
      (void)reward_face(j19, p.R0 + row * 9, p.T0 + row * 3, p.goal + (size_t)m * 3, tl, dir);
      const float dist = target_distance(tl, j19);
      p.goal_dist[m] = dist;
      p.reached[m] = (dist < p.goal_thresh) ? 1 : 0;
    }
  }
}

extern "C" int egx_primitive_select_joint(const float* joints, int joints_per_body, const float* R0, const float* T0, const float* goal,
                                          const float* cost, const float* cost_terms, const int32_t* colliding, int num_sequences,
                                          int num_candidates, const int32_t* group_start, const int32_t* group_member, int num_groups,
                                          int sweeps, float pair_weight, float margin, float body_radius, float goal_thresh,
                                          int32_t* choice, int32_t* status, int32_t* reached, float* goal_dist, float* pair_term,
                                          float* pair_clearance, float* joint_cost, int32_t* pair_hit, int32_t* choice_trace,
                                          int32_t* changed, float* crowd_clearance, int32_t* crowd_hit, void* stream) {
  EGX_REQUIRE(joints && R0 && T0 && goal && cost && cost_terms && colliding && group_start && group_member, "null input");
  EGX_REQUIRE(choice && status && reached && goal_dist && pair_term && pair_clearance && joint_cost && pair_hit && choice_trace &&
              changed && crowd_clearance && crowd_hit, "null output");
  EGX_REQUIRE(num_sequences > 0 && joints_per_body >= 3, "need a non-empty batch and >= 3 joints per body");
  EGX_REQUIRE(num_candidates >= 1 && num_candidates <= MAXC, "num_candidates must be in [1, EGX_MAX_CANDIDATES]");
  EGX_REQUIRE(sweeps >= 1 && sweeps <= EGX_MAX_SWEEPS, "sweeps must be in [1, EGX_MAX_SWEEPS]");
  EGX_REQUIRE(num_groups >= 1, "num_groups must be at least 1");
  EGX_REQUIRE(margin >= 0.f && body_radius >= 0.f, "margin and body_radius must not be negative");
  EGX_REQUIRE(std::isfinite(pair_weight), "pair_weight must be finite");
  JointArgs p{};
  p.joints = joints; p.R0 = R0; p.T0 = T0; p.goal = goal; p.cost = cost; p.terms = cost_terms; p.colliding = colliding;
  p.group_start = group_start; p.group_member = group_member;
  p.b = num_sequences; p.N = num_candidates; p.jpb = joints_per_body; p.G = num_groups; p.S = sweeps;
  p.w = pair_weight; p.margin = margin; p.rr = body_radius + body_radius; p.goal_thresh = goal_thresh;   // doubling is exact
  p.choice = choice; p.status = status; p.reached = reached; p.goal_dist = goal_dist;
  p.pair_term = pair_term; p.pair_clearance = pair_clearance; p.joint_cost = joint_cost; p.pair_hit = pair_hit;
  p.choice_trace = choice_trace; p.changed = changed; p.crowd_clearance = crowd_clearance; p.crowd_hit = crowd_hit;
  hipLaunchKernelGGL(egx_primitive_select_joint_kernel, dim3(num_groups), dim3(JOINT_BLK), 0, static_cast<hipStream_t>(stream), p);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

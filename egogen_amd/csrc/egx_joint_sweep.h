// The sweeps of the joint step of the greedy primitive search, stated once for its pair models (the cylinders of genop_joint.hip,
// the markers of genop_joint_markers.hip).  One workgroup per group runs S Gauss-Seidel sweeps over the P members in order: every
// candidate row of member i gets the clearance term of its 18 frame clearances c_t against the other members' CURRENT choices,
// added to the cost the selection wrote; member i takes the first row in the selection's total order (key_before) before member
// i + 1 is visited.  All sweeps always run: every trip count and barrier is workgroup-uniform.  No float atomics, no spin waits,
// nothing passes between workgroups: a group's outputs are the same bits in any batch.
//
// A pair model is a template argument, never a run-time flag.  It says where c_t comes from, and owns whatever LDS that takes:
//   void  prepare(grp)                  by the whole workgroup once the membership is known; the skeleton's barrier follows
//   Row   load(row, lane)               what a lane reads of candidate row `row`, with no branch round a load
//   float clearance(grp, i, n, r, lane) c_t of row n of member i for the frame of this lane (lanes 0..17), r as `load` gave it
//   void  keep(n, r, lane)              what it retains of a scored row
//   void  chosen(i, n, lane)            member i's winner n is known: every lane of wave 0, before the barrier that ends the step
//   float final_clearance(grp, i, lane) c_t of member i's final choice against the others' final choices
//
// A member step is a chain of latencies, not of work: the rows' inputs from memory, the clearances, three wave reductions per row,
// the choice by wave 0, two barriers.  So the inputs of ROWS_AHEAD rows of a wave are read in one batch with no branch between the
// loads, what lane 0 needs of a row (cost, terms, colliding) with them: one trip to memory per batch, not two per row.
//
// For the joint translation units only, which are apart from genop.hip (genop_joint.hip says why): the four small helpers the
// selection kernels keep in their anonymous namespace (wave_sum, wave_min, wave_max, key_before) are stated here for them, same
// trees, same order.
#pragma once
#include <cmath>

#include "egx_common.h"
#include "egx_reward.h"

namespace {

constexpr int NT = 20, THIS = 2, NF = NT - THIS;   // the predicted frames of a primitive
constexpr int JOINT_BLK = 512, JOINT_WAVES = JOINT_BLK / 64;   // as SEL_BLK of genop.hip: 8 waves, one candidate row per wave at a time
constexpr int MAXC = EGX_MAX_CANDIDATES, MAXP = EGX_MAX_GROUP;
constexpr int ROWS_AHEAD = 4;                      // rows of a wave whose inputs are in flight together: N <= 32 is one batch per member step
static_assert(NF <= 64 && MAXP <= JOINT_BLK, "one lane per frame, one thread per member");

// what both sweep entries pass; a model carries its extras itself
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
  float w, margin, goal_thresh;
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

// a group as its workgroup holds it in LDS: the members' sequence indices and their current choices
struct JointGroup {
  int P;
  const int* member;
  const int* choice;
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

__device__ __forceinline__ int finite01(float v) { return isfinite(v) ? 1 : 0; }   // an int: the & of several is no branch

// membership: the group's first slot and its size, both clamped into the member list, the size to EGX_MAX_GROUP
__device__ __forceinline__ void group_span(const int* group_start, int G, int g, int& start, int& P) {
  const int total = max(group_start[G], 0);
  start = min(max(group_start[g], 0), total);
  P = min(min(max(group_start[g + 1], start), total) - start, MAXP);
}

// What a wave makes of the frame clearances c_t in lanes 0..17 (`live`): lane 0 returns term = (sum_t max(0, margin - c_t)) / 18 by
// the wave_sum tree and clearance = min_t c_t; a NaN frame makes both NaN (obstacle_group's arithmetic).
__device__ __forceinline__ void frame_terms(float c, bool live, float margin, float& term, float& clearance) {
  float pen = 0.f;
  int bad = 0;
  if (live) {
    bad = isnan(c) ? 1 : 0;
    pen = bad ? c : fmaxf(0.f, egx_sub(margin, c));
  } else {
    c = __builtin_inff();
  }
  const float sum = wave_sum(pen);
  const float cmin = wave_min(bad ? __builtin_inff() : c);
  const int any_bad = wave_max(bad);
  term = sum / (float)NF;
  clearance = any_bad ? __builtin_nanf("") : cmin;
}

template <class Model>
__device__ __forceinline__ void joint_sweep(const JointArgs& p, Model& model) {
  __shared__ float s_cost[MAXC];
  __shared__ int s_cls[MAXC];
  __shared__ int s_member[MAXP], s_choice[MAXP], s_first[MAXP], s_chosen_cls[MAXP];
  const int g = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63, N = p.N;
  const size_t rows = (size_t)p.b * N;
  const bool live = lane < NF;

  int start, P;
  group_span(p.group_start, p.G, g, start, P);
  if (tid < P) {                                         // every index into [0, b), every choice into [0, N)
    const int m = min(max(p.group_member[start + tid], 0), p.b - 1);
    const int c = min(max(p.choice[m], 0), N - 1);
    s_member[tid] = m;
    s_choice[tid] = c;
    s_first[tid] = c;
    s_chosen_cls[tid] = 0;
  }
  __syncthreads();
  const JointGroup grp{P, s_member, s_choice};
  model.prepare(grp);
  __syncthreads();

  for (int s = 0; s < p.S; ++s) {
    int nchanged = 0;                                    // lane 0 of wave 0 counts
    for (int i = 0; i < P; ++i) {
      const int m = s_member[i];
      // a wave takes a row at a time, lanes 0..17 one frame each; ROWS_AHEAD rows of a wave are read before the first is scored
      for (int n0 = w; n0 < N; n0 += JOINT_WAVES * ROWS_AHEAD) {
        typename Model::Row r[ROWS_AHEAD];
        float base[ROWS_AHEAD];
        bool fin[ROWS_AHEAD], coll[ROWS_AHEAD];
#pragma unroll
        for (int u = 0; u < ROWS_AHEAD; ++u) {
          const size_t row = (size_t)m * N + min(n0 + u * JOINT_WAVES, N - 1);   // no branch round a load: a row past N - 1 reads row N - 1 again
          r[u] = model.load(row, lane);
          const float* tm = p.terms + row * 5;
          const float t0 = tm[0], t1 = tm[1], t2 = tm[2], t3 = tm[3], t4 = tm[4];
          base[u] = p.cost[row];
          coll[u] = p.colliding[row] != 0;
          fin[u] = finite01(base[u]) & finite01(t0) & finite01(t1) & finite01(t2) & finite01(t3) & finite01(t4);   // & not &&: no load waits for a branch
        }
#pragma unroll
        for (int u = 0; u < ROWS_AHEAD; ++u) {
          const int n = n0 + u * JOINT_WAVES;
          if (n >= N) break;                             // the same in every lane of the wave
          const size_t row = (size_t)m * N + n;
          float term, clearance;
          frame_terms(model.clearance(grp, i, n, r[u], lane), live, p.margin, term, clearance);
          model.keep(n, r[u], lane);
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
        model.chosen(i, bi, lane);                       // every lane holds the winner
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

  // the crowd as written: every member's final choice against the others' final choices
  for (int i = w; i < P; i += JOINT_WAVES) {
    float term, clearance;
    frame_terms(model.final_clearance(grp, i, lane), live, p.margin, term, clearance);
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

// The argument checks the two sweep entries share, in their order; `inputs`: every input pointer of the entry is there; `reach`: the
// model's reach under its name (body_radius, pair_skin).  Returns the EGX_* code with the error message set.
static inline int joint_check_args(bool inputs, const JointArgs& p, float reach, const char* reach_name) {
  EGX_REQUIRE(inputs, "null input");
  EGX_REQUIRE(p.choice && p.status && p.reached && p.goal_dist && p.pair_term && p.pair_clearance && p.joint_cost && p.pair_hit &&
              p.choice_trace && p.changed && p.crowd_clearance && p.crowd_hit, "null output");
  EGX_REQUIRE(p.b > 0 && p.jpb >= 3, "need a non-empty batch and >= 3 joints per body");
  EGX_REQUIRE(p.N >= 1 && p.N <= MAXC, "num_candidates must be in [1, EGX_MAX_CANDIDATES]");
  EGX_REQUIRE(p.S >= 1 && p.S <= EGX_MAX_SWEEPS, "sweeps must be in [1, EGX_MAX_SWEEPS]");
  EGX_REQUIRE(p.G >= 1, "num_groups must be at least 1");
  EGX_REQUIRE(p.margin >= 0.f && reach >= 0.f, std::string("margin and ") + reach_name + " must not be negative");
  EGX_REQUIRE(std::isfinite(p.w), "pair_weight must be finite");
  return EGX_OK;
}

}  // namespace

// The marker-level pair model of the joint step of the greedy primitive search (`generate_sequence_to_goal(groups=, pair_model=
// "markers")`): a person is the 67 blended markers of a candidate row in the world, not a cylinder round the pelvis.  Two launches
// stand where egx_primitive_select_joint (genop_joint.hip) stands in the cylinder model:
//
//   egx_pair_marker_dist                 every distance a sweep can ask for, before the first sweep: the members only ever choose
//                                        among their own N rows, so D[pair, n_i, n_j, frame] over the unordered pairs of members of a
//                                        group is all there is.  Fully parallel: one workgroup per (pair, row of the first member,
//                                        tile of TILE rows of the second); the first row's world markers stay in LDS, the second
//                                        member's rows stream through registers, RB at a time; a wave takes a frame at a time, the
//                                        67 x 67 squared distances spread over its lanes (the shape of egx_crowd_metrics, in float32).
//                                        A second part of the same grid, one workgroup per sequence, writes row_bad.
//   egx_primitive_select_joint_markers   the sweep loop of egx_primitive_select_joint with the frame clearances read from that table
//                                        through the members' current choices: no xy tables in LDS, no marker arithmetic.
//
// No float atomics, no spin waits, nothing passes between workgroups within a launch, every loop bound is a launch argument or a
// constant: a group's outputs are the same bits in any batch.  A translation unit of its own, for the reason genop_joint.hip gives:
// nothing here is compiled together with the selection kernels or with the cylinder kernel; wave_sum, wave_min, wave_max and
// key_before are restated below, same trees, same order, and so is the expression of blend_marker (genop.hip).
#include <cmath>

#include "egx_common.h"
#include "egx_reward.h"

namespace {

constexpr int NT = 20, THIS = 2, NF = NT - THIS, NMK = 67, MD = NMK * 3;
constexpr int MAXC = EGX_MAX_CANDIDATES, MAXP = EGX_MAX_GROUP;
constexpr int DIST_WAVES = 9, DIST_BLK = DIST_WAVES * 64;   // 18 frames: two per wave
constexpr int TILE = 8;                                      // rows of the second member per workgroup
constexpr int RB = 4;                                        // of which a lane holds this many in registers at a time
static_assert(TILE % RB == 0 && 3 * RB <= 64, "a tile is whole register blocks; lanes 0 .. 3 RB - 1 hold the markers 64..66 of a block");
constexpr int JOINT_BLK = 512, JOINT_WAVES = JOINT_BLK / 64;
static_assert(NF == 2 * DIST_WAVES, "a wave of the distance kernel takes frames w and w + 9");
static_assert(NF <= 32, "row_bad is a mask of the predicted frames");

struct DistArgs {
  const float* markers_proj;  // [rows*20,67,3]
  const float* Y_gen;         // [18,rows,201]
  const float* R0;            // [rows,9]
  const float* T0;            // [rows,3]
  const int* group_start;     // [G+1]
  const int* group_member;
  const int* pair_start;      // [G+1]
  int b, N, G, npairs, tiles;
  unsigned pair_blocks;
  float rf;
  float* D;                   // [npairs,N,N,18]
  int* row_bad;               // [rows]
};

struct SweepArgs {
  const float* D;             // [npairs,N,N,18]
  const int* row_bad;         // [rows]
  const int* pair_start;      // [G+1]
  const float* joints;        // [b*N*20,jpb,3]
  const float* R0;
  const float* T0;
  const float* goal;          // [b,3]
  const float* cost;          // [b*N]    what the selection wrote, read only
  const float* terms;         // [b*N,5]
  const int* colliding;       // [b*N]
  const int* group_start;
  const int* group_member;
  int b, N, jpb, G, S, npairs;
  float w, margin, skin, goal_thresh;
  int* choice;
  int* status;
  int* reached;
  float* goal_dist;
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

__device__ __forceinline__ float blend_marker(float rf, float proj, float pred) { return rf * proj + (1.f - rf) * pred; }

// world marker a of row r at frame t (2..19): the blended local marker in the row's frame, pelvis_xy's nesting extended to z;
// .w = 1 where a coordinate is not finite
__device__ __forceinline__ float4 world_marker(const DistArgs& p, size_t r, int t, int a) {
  const size_t rows = (size_t)p.b * p.N;
  const float* pr = p.markers_proj + (r * NT + t) * MD + 3 * a;
  const float* pd = p.Y_gen + ((size_t)(t - THIS) * rows + r) * MD + 3 * a;
  const float* R0 = p.R0 + r * 9;
  const float* T0 = p.T0 + r * 3;
  const float m0 = blend_marker(p.rf, pr[0], pd[0]), m1 = blend_marker(p.rf, pr[1], pd[1]), m2 = blend_marker(p.rf, pr[2], pd[2]);
  float4 v;
  v.x = fmaf(R0[2], m2, fmaf(R0[1], m1, R0[0] * m0)) + T0[0];
  v.y = fmaf(R0[5], m2, fmaf(R0[4], m1, R0[3] * m0)) + T0[1];
  v.z = fmaf(R0[8], m2, fmaf(R0[7], m1, R0[6] * m0)) + T0[2];
  v.w = (isfinite(v.x) && isfinite(v.y) && isfinite(v.z)) ? 0.f : 1.f;
  return v;
}

// the world markers of the 18 predicted frames of row r into s [18][67], by the whole workgroup; the caller's barrier follows
__device__ __forceinline__ void stage_row(const DistArgs& p, size_t r, float4 (*s)[NMK]) {
  for (int e = threadIdx.x; e < NF * NMK; e += DIST_BLK) s[e / NMK][e % NMK] = world_marker(p, r, THIS + e / NMK, e % NMK);
}

// the squared distance of two world markers: three rounded differences, three rounded squares, (dx^2 + dy^2) + dz^2 in that order,
// no contraction.  The same bits with the two markers exchanged.
__device__ __forceinline__ float dist2(const float4& a, const float4& b) {
  const float dx = egx_sub(a.x, b.x), dy = egx_sub(a.y, b.y), dz = egx_sub(a.z, b.z);
  return egx_add(egx_add(egx_mul(dx, dx), egx_mul(dy, dy)), egx_mul(dz, dz));
}

// membership as egx_primitive_select_joint clamps it: the group's first slot and its size
__device__ __forceinline__ void group_span(const int* group_start, int G, int g, int& start, int& P) {
  const int total = max(group_start[G], 0);
  start = min(max(group_start[g], 0), total);
  P = min(min(max(group_start[g + 1], start), total) - start, MAXP);
}

// local pair q of a group of P, lexicographic (a, b), a < b  <->  (a, b)
__device__ __forceinline__ int pair_index(int P, int a, int b) { return a * (2 * P - a - 1) / 2 + (b - a - 1); }

// What a wave makes of the frame clearances c_t in lanes 0..17 (own_bad: the row's own frame is bad, c_t = NaN): lane 0 returns
// term = (sum_t max(0, margin - c_t)) / 18 by the wave_sum tree and clearance = min_t c_t; a NaN frame makes both NaN.  The
// arithmetic of track_terms (genop_joint.hip).
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

// c_t of row n of member i (slot index within the group) against the other members' current choices, for the frame of this lane:
// min over j != i of D - skin, one rounded difference after the minimum (a difference is monotone: the same bits as the minimum of
// the differences); +inf where nobody else is there; NaN where the row's own frame is bad.
__device__ __forceinline__ float frame_clearance(const SweepArgs& p, int pair0, int P, int i, int n, int f, const int* s_choice, bool own_bad) {
  const size_t N = (size_t)p.N;
  float m = __builtin_inff();
#pragma unroll 4
  for (int j = 0; j < P; ++j) {
    if (j == i) continue;
    const int q = pair0 + (i < j ? pair_index(P, i, j) : pair_index(P, j, i));
    if (q >= p.npairs) continue;
    const size_t na = i < j ? n : s_choice[j], nb = i < j ? s_choice[j] : n;
    m = fminf(m, p.D[(((size_t)q * N + na) * N + nb) * NF + f]);
  }
  return own_bad ? __builtin_nanf("") : egx_sub(m, p.skin);
}

}  // namespace

__global__ __launch_bounds__(DIST_BLK) void egx_pair_marker_dist_kernel(DistArgs p) {
  __shared__ float4 s_a[NF][NMK];                 // 19.3 KB: one read of 16 bytes per RB distances
  __shared__ int s_mask[DIST_WAVES];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, N = p.N;

  if (blockIdx.x >= p.pair_blocks) {              // row_bad of the N rows of one sequence
    const int m = (int)(blockIdx.x - p.pair_blocks);
    for (int n = 0; n < N; ++n) {
      const size_t r = (size_t)m * N + n;
      int mask = 0;
      for (int k = 0; k < 2; ++k) {
        const int f = w + k * DIST_WAVES;
        bool bad = world_marker(p, r, THIS + f, lane).w != 0.f;
        if (lane < NMK - 64) bad |= world_marker(p, r, THIS + f, 64 + lane).w != 0.f;
        if (__any(bad)) mask |= 1 << f;
      }
      if (lane == 0) s_mask[w] = mask;
      __syncthreads();
      if (tid == 0) {
        int all = 0;
        for (int k = 0; k < DIST_WAVES; ++k) all |= s_mask[k];
        p.row_bad[r] = all;
      }
      __syncthreads();
    }
    return;
  }

  // (pair, row of the first member, tile of the second member's rows) of this workgroup; the pair's group by bisection of pair_start
  const int tile = blockIdx.x % p.tiles;
  const int na = (blockIdx.x / p.tiles) % N;
  const int q = blockIdx.x / p.tiles / N;         // < npairs by the grid
  int lo = 0, hi = p.G;                           // the last g with pair_start[g] <= q
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (p.pair_start[mid] <= q) lo = mid; else hi = mid;
  }
  const int g = lo;
  int start, P;
  group_span(p.group_start, p.G, g, start, P);
  const int ql = q - p.pair_start[g];
  if (ql < 0 || ql >= P * (P - 1) / 2) return;    // pair_start does not describe this group: nothing is written (uniform)
  int a = 0, rem = ql;
  while (rem >= P - 1 - a) { rem -= P - 1 - a; ++a; }
  const int bm = a + 1 + rem;
  const int ma = min(max(p.group_member[start + a], 0), p.b - 1), mb = min(max(p.group_member[start + bm], 0), p.b - 1);

  stage_row(p, (size_t)ma * N + na, s_a);
  __syncthreads();
  // A wave takes frames w and w + 9.  The loop is bound by the arithmetic only if a read of LDS serves several distances, so a
  // lane keeps marker `lane` of RB rows of the second member in registers (computed from memory: nobody else needs them) and walks
  // the first row's 67 markers, every lane reading one address (a broadcast): RB distances per read.  The second member's markers
  // 64..66 are computed by lanes 0 .. 3 RB - 1 and handed round by readlane, against marker `lane` and (lanes 0..2) 64 + lane of the
  // first row.  A minimum does not depend on the order it is taken in.
  const int nb0 = tile * TILE, nb_end = min(nb0 + TILE, N);
  for (int k = 0; k < 2; ++k) {
    const int f = w + k * DIST_WAVES;
    const float4 a_lane = s_a[f][lane], a_more = s_a[f][lane < NMK - 64 ? 64 + lane : lane];
    const bool bad_a = __any(a_lane.w != 0.f || a_more.w != 0.f);
    for (int nb = nb0; nb < nb_end; nb += RB) {
      float4 mine[RB];
      float d2[RB];
#pragma unroll
      for (int u = 0; u < RB; ++u) {
        mine[u] = world_marker(p, (size_t)mb * N + min(nb + u, N - 1), THIS + f, lane);
        d2[u] = __builtin_inff();
      }
      const float4 more = world_marker(p, (size_t)mb * N + min(nb + min(lane / 3, RB - 1), N - 1), THIS + f, 64 + lane % 3);   // lanes 0 .. 3 RB - 1 count
      for (int m = 0; m < NMK; ++m) {
        const float4 a = s_a[f][m];
#pragma unroll
        for (int u = 0; u < RB; ++u) d2[u] = fminf(d2[u], dist2(a, mine[u]));
      }
      const unsigned long long bad_more = __ballot(more.w != 0.f);
#pragma unroll
      for (int u = 0; u < RB; ++u) {
#pragma unroll
        for (int j = 0; j < NMK - 64; ++j) {
          float4 b;
          b.x = __shfl(more.x, 3 * u + j, 64); b.y = __shfl(more.y, 3 * u + j, 64); b.z = __shfl(more.z, 3 * u + j, 64); b.w = 0.f;
          d2[u] = fminf(d2[u], dist2(a_lane, b));
          if (lane < NMK - 64) d2[u] = fminf(d2[u], dist2(a_more, b));
        }
      }
#pragma unroll
      for (int u = 0; u < RB; ++u) {
        const bool bad = bad_a || __any(mine[u].w != 0.f) || ((bad_more >> (3 * u)) & 7ull) != 0;
        const float least = wave_min(d2[u]);
        if (lane == 0 && nb + u < nb_end) p.D[(((size_t)q * N + na) * N + nb + u) * NF + f] = bad ? __builtin_inff() : sqrtf(least);
      }
    }
  }
}

__global__ __launch_bounds__(JOINT_BLK) void egx_primitive_select_joint_markers_kernel(SweepArgs p) {
  __shared__ float s_cost[MAXC];
  __shared__ int s_cls[MAXC];
  __shared__ int s_member[MAXP], s_choice[MAXP], s_first[MAXP], s_chosen_cls[MAXP];
  const int g = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63, N = p.N;
  const size_t rows = (size_t)p.b * N;
  const bool live = lane < NF;
  const int f = live ? lane : 0;

  int start, P;
  group_span(p.group_start, p.G, g, start, P);
  const int pair0 = min(max(p.pair_start[g], 0), p.npairs);
  if (tid < P) {
    const int m = min(max(p.group_member[start + tid], 0), p.b - 1);
    const int c = min(max(p.choice[m], 0), N - 1);
    s_member[tid] = m;
    s_choice[tid] = c;
    s_first[tid] = c;
    s_chosen_cls[tid] = 0;
  }
  __syncthreads();

  for (int s = 0; s < p.S; ++s) {
    int nchanged = 0;                                    // lane 0 of wave 0 counts
    for (int i = 0; i < P; ++i) {
      const int m = s_member[i];
      for (int n = w; n < N; n += JOINT_WAVES) {         // a wave takes a row at a time, lanes 0..17 one frame each
        const size_t row = (size_t)m * N + n;
        const bool own_bad = (p.row_bad[row] >> f) & 1;
        const float c = frame_clearance(p, pair0, P, i, n, f, s_choice, own_bad);
        float term, clearance;
        frame_terms(c, live, p.margin, term, clearance);
        if (lane == 0) {
          const float* tm = p.terms + row * 5;
          const float base = p.cost[row];
          const bool fin = isfinite(base) && isfinite(tm[0]) && isfinite(tm[1]) && isfinite(tm[2]) && isfinite(tm[3]) && isfinite(tm[4]);
          const bool hit = clearance < 0.f;              // false for NaN
          const float jc = egx_add(base, egx_mul(p.w, term));
          const bool finite = fin && isfinite(term) && isfinite(jc);
          const size_t at = (size_t)s * rows + row;
          p.pair_term[at] = term;
          p.pair_clearance[at] = clearance;
          p.joint_cost[at] = jc;
          p.pair_hit[at] = hit ? 1 : 0;
          s_cost[n] = finite ? jc : 0.f;                 // a non-finite row is ranked by collision and index only
          s_cls[n] = (finite ? 0 : 2) | (p.colliding[row] != 0 ? 1 : 0) | (hit ? 1 : 0);
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

  // the crowd as written: every member's final row against the others' final rows
  for (int i = w; i < P; i += JOINT_WAVES) {
    const size_t row = (size_t)s_member[i] * N + s_choice[i];
    const bool own_bad = (p.row_bad[row] >> f) & 1;
    const float c = frame_clearance(p, pair0, P, i, s_choice[i], f, s_choice, own_bad);
    float term, clearance;
    frame_terms(c, live, p.margin, term, clearance);
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

extern "C" int egx_pair_marker_dist(const float* markers_proj, const float* Y_gen, float reproj_factor, const float* R0, const float* T0,
                                    int num_sequences, int num_candidates, const int32_t* group_start, const int32_t* group_member,
                                    const int32_t* pair_start, int num_groups, int num_pairs, float* pair_dist, int32_t* row_bad,
                                    void* stream) {
  EGX_REQUIRE(markers_proj && Y_gen && R0 && T0 && group_start && group_member && pair_start, "null input");
  EGX_REQUIRE(row_bad, "null output");
  EGX_REQUIRE(num_sequences > 0, "need a non-empty batch");
  EGX_REQUIRE(num_candidates >= 1 && num_candidates <= MAXC, "num_candidates must be in [1, EGX_MAX_CANDIDATES]");
  EGX_REQUIRE(num_groups >= 1, "num_groups must be at least 1");
  EGX_REQUIRE(reproj_factor >= 0.f && reproj_factor <= 1.f, "reproj_factor must be in [0, 1]");
  EGX_REQUIRE(num_pairs >= 0 && (num_pairs == 0) == (pair_dist == nullptr), "pair_dist must be NULL exactly where num_pairs is 0");
  DistArgs p{};
  p.markers_proj = markers_proj; p.Y_gen = Y_gen; p.R0 = R0; p.T0 = T0;
  p.group_start = group_start; p.group_member = group_member; p.pair_start = pair_start;
  p.b = num_sequences; p.N = num_candidates; p.G = num_groups; p.npairs = num_pairs; p.tiles = egx_ceil_div(num_candidates, TILE);
  p.rf = reproj_factor; p.D = pair_dist; p.row_bad = row_bad;
  const long long pair_blocks = (long long)num_pairs * num_candidates * p.tiles;
  EGX_REQUIRE(pair_blocks + num_sequences <= 0x7fffffffLL, "num_pairs * num_candidates * tiles + num_sequences must stay below 2^31");
  p.pair_blocks = (unsigned)pair_blocks;
  hipLaunchKernelGGL(egx_pair_marker_dist_kernel, dim3((unsigned)(pair_blocks + num_sequences)), dim3(DIST_BLK), 0,
                     static_cast<hipStream_t>(stream), p);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

extern "C" int egx_primitive_select_joint_markers(const float* pair_dist, const int32_t* row_bad, const int32_t* pair_start, int num_pairs,
                                                  const float* joints, int joints_per_body, const float* R0, const float* T0,
                                                  const float* goal, const float* cost, const float* cost_terms,
                                                  const int32_t* colliding, int num_sequences, int num_candidates,
                                                  const int32_t* group_start, const int32_t* group_member, int num_groups, int sweeps,
                                                  float pair_weight, float margin, float pair_skin, float goal_thresh, int32_t* choice,
                                                  int32_t* status, int32_t* reached, float* goal_dist, float* pair_term,
                                                  float* pair_clearance, float* joint_cost, int32_t* pair_hit, int32_t* choice_trace,
                                                  int32_t* changed, float* crowd_clearance, int32_t* crowd_hit, void* stream) {
  EGX_REQUIRE(row_bad && pair_start && joints && R0 && T0 && goal && cost && cost_terms && colliding && group_start && group_member,
              "null input");
  EGX_REQUIRE(choice && status && reached && goal_dist && pair_term && pair_clearance && joint_cost && pair_hit && choice_trace &&
              changed && crowd_clearance && crowd_hit, "null output");
  EGX_REQUIRE(num_sequences > 0 && joints_per_body >= 3, "need a non-empty batch and >= 3 joints per body");
  EGX_REQUIRE(num_candidates >= 1 && num_candidates <= MAXC, "num_candidates must be in [1, EGX_MAX_CANDIDATES]");
  EGX_REQUIRE(sweeps >= 1 && sweeps <= EGX_MAX_SWEEPS, "sweeps must be in [1, EGX_MAX_SWEEPS]");
  EGX_REQUIRE(num_groups >= 1, "num_groups must be at least 1");
  EGX_REQUIRE(margin >= 0.f && pair_skin >= 0.f, "margin and pair_skin must not be negative");
  EGX_REQUIRE(std::isfinite(pair_weight), "pair_weight must be finite");
  EGX_REQUIRE(num_pairs >= 0 && (num_pairs == 0) == (pair_dist == nullptr), "pair_dist must be NULL exactly where num_pairs is 0");
  SweepArgs p{};
  p.D = pair_dist; p.row_bad = row_bad; p.pair_start = pair_start;
  p.joints = joints; p.R0 = R0; p.T0 = T0; p.goal = goal; p.cost = cost; p.terms = cost_terms; p.colliding = colliding;
  p.group_start = group_start; p.group_member = group_member;
  p.b = num_sequences; p.N = num_candidates; p.jpb = joints_per_body; p.G = num_groups; p.S = sweeps; p.npairs = num_pairs;
  p.w = pair_weight; p.margin = margin; p.skin = pair_skin; p.goal_thresh = goal_thresh;
  p.choice = choice; p.status = status; p.reached = reached; p.goal_dist = goal_dist;
  p.pair_term = pair_term; p.pair_clearance = pair_clearance; p.joint_cost = joint_cost; p.pair_hit = pair_hit;
  p.choice_trace = choice_trace; p.changed = changed; p.crowd_clearance = crowd_clearance; p.crowd_hit = crowd_hit;
  hipLaunchKernelGGL(egx_primitive_select_joint_markers_kernel, dim3(num_groups), dim3(JOINT_BLK), 0, static_cast<hipStream_t>(stream), p);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

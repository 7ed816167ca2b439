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
//   egx_primitive_select_joint_markers   the sweeps of egx_joint_sweep.h with the frame clearances read from that table through the
//                                        members' current choices: no xy tables in LDS, no marker arithmetic.
//
// No float atomics, no spin waits, nothing passes between workgroups within a launch, every loop bound is a launch argument or a
// constant: a group's outputs are the same bits in any batch.  A translation unit of its own, for the reason genop_joint.hip gives:
// nothing here is compiled together with the selection kernels or with the cylinder kernel; the blend, the world marker and the
// squared distance are those of egx_markers.h, shared with the marker model of recorded tracks (genop_obstacle_markers.hip).
#include "egx_joint_sweep.h"
#include "egx_markers.h"

namespace {

constexpr int NMK = EGX_MK;
constexpr int DIST_WAVES = 9, DIST_BLK = DIST_WAVES * 64;   // 18 frames: two per wave
constexpr int TILE = 8;                                      // rows of the second member per workgroup
constexpr int RB = 4;                                        // of which a lane holds this many in registers at a time
static_assert(TILE % RB == 0 && 3 * RB <= 64, "a tile is whole register blocks; lanes 0 .. 3 RB - 1 hold the markers 64..66 of a block");
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

// world marker a of row r at frame t (2..19) of the launch's rows (egx_markers.h)
__device__ __forceinline__ float4 world_marker(const DistArgs& p, size_t r, int t, int a) {
  return egx_world_marker(p.markers_proj, p.Y_gen, p.R0, p.T0, (size_t)p.b * p.N, p.rf, r, t, a);
}

// the world markers of the 18 predicted frames of row r into s [18][67], by the whole workgroup; the caller's barrier follows
__device__ __forceinline__ void stage_row(const DistArgs& p, size_t r, float4 (*s)[NMK]) {
  for (int e = threadIdx.x; e < NF * NMK; e += DIST_BLK) s[e / NMK][e % NMK] = world_marker(p, r, THIS + e / NMK, e % NMK);
}

// local pair q of a group of P, lexicographic (a, b), a < b  <->  (a, b)
__device__ __forceinline__ int pair_index(int P, int a, int b) { return a * (2 * P - a - 1) / 2 + (b - a - 1); }

// The marker model of the sweeps: c_t is read from the table D of egx_pair_marker_dist.
struct Markers {
  using Row = int;                 // row_bad of the row: the mask of its own bad frames, where c_t = NaN
  const float* D;                  // [npairs,N,N,18]
  const int* row_bad;              // [rows]
  int pair0, npairs, N;            // the group's first pair
  float skin;

  // c_t of row n of member i (slot index within the group) against the other members' current choices, for frame f: min over j != i
  // of D - skin, one rounded difference after the minimum (a difference is monotone: the same bits as the minimum of the
  // differences); +inf where nobody else is there; NaN where the row's own frame is bad.
  __device__ __forceinline__ float frame_clearance(const JointGroup& g, int i, int n, int f, bool own_bad) const {
    const size_t N = (size_t)this->N;
    float m = __builtin_inff();
#pragma unroll 4
    for (int j = 0; j < g.P; ++j) {
      if (j == i) continue;
      const int q = pair0 + (i < j ? pair_index(g.P, i, j) : pair_index(g.P, j, i));
      if (q >= npairs) continue;
      const size_t na = i < j ? n : g.choice[j], nb = i < j ? g.choice[j] : n;
      m = fminf(m, D[(((size_t)q * N + na) * N + nb) * NF + f]);
    }
    return own_bad ? __builtin_nanf("") : egx_sub(m, skin);
  }
  static __device__ __forceinline__ int frame(int lane) { return lane < NF ? lane : 0; }
  __device__ __forceinline__ void prepare(const JointGroup&) {}
  __device__ __forceinline__ Row load(size_t row, int) const { return row_bad[row]; }
  __device__ __forceinline__ float clearance(const JointGroup& g, int i, int n, const Row& r, int lane) const {
    return frame_clearance(g, i, n, frame(lane), (r >> frame(lane)) & 1);
  }
  __device__ __forceinline__ void keep(int, const Row&, int) {}
  __device__ __forceinline__ void chosen(int, int, int) {}
  __device__ __forceinline__ float final_clearance(const JointGroup& g, int i, int lane) const {
    return clearance(g, i, g.choice[i], load((size_t)g.member[i] * N + g.choice[i], lane), lane);
  }
};

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

__global__ __launch_bounds__(JOINT_BLK) void egx_primitive_select_joint_markers_kernel(JointArgs p, const float* D, const int* row_bad,
                                                                                       const int* pair_start, int npairs, float skin) {
  Markers model{D, row_bad, min(max(pair_start[blockIdx.x], 0), npairs), npairs, p.N, skin};
  joint_sweep(p, model);
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
  const JointArgs p{joints, R0, T0, goal, cost, cost_terms, colliding, group_start, group_member, num_sequences, num_candidates, joints_per_body,
                    num_groups, sweeps, pair_weight, margin, goal_thresh, choice, status, reached, goal_dist, pair_term, pair_clearance,
                    joint_cost, pair_hit, choice_trace, changed, crowd_clearance, crowd_hit};
  const int bad = joint_check_args(row_bad && pair_start && joints && R0 && T0 && goal && cost && cost_terms && colliding && group_start && group_member,
                                   p, pair_skin, "pair_skin");
  if (bad != EGX_OK) return bad;
  EGX_REQUIRE(num_pairs >= 0 && (num_pairs == 0) == (pair_dist == nullptr), "pair_dist must be NULL exactly where num_pairs is 0");
  hipLaunchKernelGGL(egx_primitive_select_joint_markers_kernel, dim3(num_groups), dim3(JOINT_BLK), 0, static_cast<hipStream_t>(stream), p,
                     pair_dist, row_bad, pair_start, num_pairs, pair_skin);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

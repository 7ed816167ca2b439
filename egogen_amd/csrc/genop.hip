// Hand-off between two motion primitives of a chain (one workgroup per sequence, one launch, no sync), and the best-of-N search on
// top of it: scoring and selection of N candidates per sequence (egx_primitive_select) and the hand-off from the chosen one
// (egx_primitive_advance_select).  The beam search keeps W partial paths per sequence: egx_primitive_beam_select scores the W * N
// rows of a sequence with the same row scoring and keeps the W best path keys, egx_primitive_advance_beam hands each kept row on
// to the N rows of its slot (one workgroup per slot, R0 / T0 from one buffer into another), egx_beam_backtrack gathers the
// records of the returned path.  With a geodesic field (egx_primitive_select_field, egx_primitive_beam_select_field; geodesic.hip
// builds it) the goal term of both selections is the field's distance along the walkable raster (field_row_cost, a phase after
// the scoring); the entries without a field launch the same kernels with a null field.  With moving obstacles
// (egx_primitive_select_obstacles, egx_primitive_beam_select_obstacles; egx_obstacles.h) a third phase adds the obstacle term to
// the cost and the hit to the collision of every row (obstacle_group); the other entries launch the same kernels with a null
// obstacle descriptor.  With the marker model of recorded tracks (egx_primitive_select_obstacle_markers,
// egx_primitive_beam_select_obstacle_markers) that phase reads its frame clearances from the table egx_obstacle_marker_clearance
// (genop_obstacle_markers.hip) wrote: kernels of their own, compile-time variants of the same bodies.  Device code is shared (advance_body, score_group, field_row_cost, obstacle_group, key_before); so is the host side: the three hand-off entries go through advance_entry and the selection entries
// through select_entry (common checks, common fields, launch check), and each entry states only the checks, fields and launch
// that are its own.
//
// Reference: the motion-only tail of CrowdEnv.step, motion/crowd_ppo/crowd_env_2f.py:144-155 (pelvis, blended markers) and
// :238-265 (new canonical frame from the second-last body, accumulated world frame, seed parameters and seed markers in the new
// frame) without _get_feature; the frame algebra is the code the env kernels use (egx_frame.h), the cost terms are the arguments
// of the env's reward terms (:171-235, egx_reward.h).
#include "egx_common.h"
#include "egx_frame.h"
#include "egx_geodesic.h"
#include "egx_obstacles.h"
#include "egx_reward.h"

namespace {

constexpr int NT = 20, THIS = 2, NM = 67, MD = NM * 3, XB = EGX_XB_DIM;
constexpr int BLK = 256;
constexpr int SEL_BLK = 512, SEL_WAVES = SEL_BLK / 64;   // scoring: 8 waves per sequence, one candidate row per wave at a time
constexpr int NF = 6;                                     // feet markers
constexpr int MAXC = EGX_MAX_CANDIDATES;
constexpr int NV4 = NT * MD / 4;   // float4 packets of one sequence's markers
static_assert(NT * MD % 4 == 0, "a sequence's markers are whole float4 packets");

struct AdvanceArgs {
  const float* pred_params;   // [B,20,93]
  const float* Y_gen;         // [18,B,201]
  const float* x0;            // seed frames, row stride x_ld
  const float* x1;
  const float* joints;        // [B*20,jpb,3]
  const float* markers_proj;  // [B*20,67,3]
  const float* delta_T;       // [B,3]
  const float* R0;            // [B,9] read before the barrier ...
  const float* T0;            // [B,3]
  float* R0_out;              // ... written after it: the same buffers in the one-workgroup-per-group entries (in place), other
  float* T0_out;              // buffers where several workgroups share a group (egx_primitive_advance_beam)
  float* out_marker_b;        // [B,20,67,3]
  float* out_pelvis;          // [B,20,3]
  float* out_R;               // [B,9]
  float* out_T;               // [B,3]
  float* out_seed;            // [B,2,93]
  float* out_x0;              // next seed frames, row stride out_x_ld
  float* out_x1;
  float* out_params;          // [b,20,93] record of the handed-on row, or null
  int* nonfinite;             // [1] or null
  int* beam_status;           // [b*W] of the beam hand-off: bit 2 of row `rec` is set on a non-finite value (no counter there)
  float rf;
  int B /* rows of the per-row inputs */, jpb, x_ld, out_x_ld;
};

__device__ __forceinline__ bool nonfin(float v) { return !isfinite(v); }

// cat(x, Y_gen)[t] of row `row`, coordinate d
__device__ __forceinline__ float predicted_marker(const AdvanceArgs& p, int row, int t, int d) {
  return (t == 0)   ? p.x0[(size_t)row * p.x_ld + d]
         : (t == 1) ? p.x1[(size_t)row * p.x_ld + d]
                    : p.Y_gen[((size_t)(t - THIS) * p.B + row) * MD + d];
}
// the blended marker (:151-152); one expression for the hand-off and the scoring, so both see the same values
__device__ __forceinline__ float blend_marker(float rf, float proj, float pred) { return rf * proj + (1.f - rf) * pred; }

}  // namespace

// The hand-off of one sequence by one workgroup: reads row `src` of the per-row inputs, writes the record outputs to row `rec`
// and the next state (R0, T0, seed parameters, seed frames) to the `ndst` rows from `dst0`.  Every read of R0 / T0 precedes the
// barrier, every write of them (to R0_out / T0_out) follows it.  BEAM: a non-finite value marks beam_status[rec], not the counter.
template <bool BEAM>
__device__ __forceinline__ void advance_body(const AdvanceArgs& p, int src, int rec, int dst0, int ndst) {
  __shared__ float s_mb[THIS][MD];   // blended markers of frames 18, 19 (old frame)
  __shared__ float s_frame[24];      // R_[9], T_[3], new R0[9], new T0[3]
  __shared__ float s_seed6[THIS][6];
  const int tid = threadIdx.x;
  const float* J = p.joints + (size_t)src * NT * p.jpb * 3;
  const float* PP = p.pred_params + (size_t)src * NT * XB;
  bool bad = false;

  // ---- frame algebra in the last two lanes of the block (one per seed frame); the other waves start on the markers ----
  if (tid >= BLK - THIS) {
    const int f = tid - (BLK - THIS);
    const float* j18 = J + (size_t)18 * p.jpb * 3;
    float Rn[9], Tn[3], o6[6];
    canonical_frame(j18 + 0, j18 + 3, j18 + 6, Rn, Tn);
    const float delta[3] = {p.delta_T[(size_t)src * 3 + 0], p.delta_T[(size_t)src * 3 + 1], p.delta_T[(size_t)src * 3 + 2]};
    update_transl_glorot(Rn, Tn, delta, PP + (18 + f) * XB, o6);
    for (int e = 0; e < 6; ++e) { s_seed6[f][e] = o6[e]; bad |= nonfin(o6[e]); }
    if (f == 0) {
      float R0o[9], T0o[3], T0n[3], R0n[9];
      for (int e = 0; e < 9; ++e) R0o[e] = p.R0[(size_t)src * 9 + e];
      for (int e = 0; e < 3; ++e) T0o[e] = p.T0[(size_t)src * 3 + e];
      mat3_vec(R0o, Tn, T0n);
      T0n[0] += T0o[0]; T0n[1] += T0o[1]; T0n[2] += T0o[2];
      mat3_mul(R0o, Rn, R0n);
      for (int e = 0; e < 9; ++e) {
        s_frame[e] = Rn[e];
        s_frame[12 + e] = R0n[e];
        p.out_R[(size_t)rec * 9 + e] = R0o[e];
        bad |= nonfin(R0n[e]);
      }
      for (int e = 0; e < 3; ++e) {
        s_frame[9 + e] = Tn[e];
        s_frame[21 + e] = T0n[e];
        p.out_T[(size_t)rec * 3 + e] = T0o[e];
        bad |= nonfin(T0n[e]);
      }
    }
  }

  // ---- pelvis of the 20 bodies ----------------------------------------------------------------------------------------
  if (tid < NT * 3) {
    const float v = J[(size_t)(tid / 3) * p.jpb * 3 + tid % 3];
    p.out_pelvis[(size_t)rec * NT * 3 + tid] = v;
    bad |= nonfin(v);
  }
  if (p.out_params)
    for (int i = tid; i < NT * XB; i += BLK) p.out_params[(size_t)rec * NT * XB + i] = PP[i];

  // ---- blended markers: projected and output as float4 across the block, predicted gathered per element ------------------
  const float rf = p.rf;
  const f32x4* proj4 = reinterpret_cast<const f32x4*>(p.markers_proj + (size_t)src * NT * MD);
  f32x4* out4 = reinterpret_cast<f32x4*>(p.out_marker_b + (size_t)rec * NT * MD);
  for (int i = tid; i < NV4; i += BLK) {
    const f32x4 pr = proj4[i];
    f32x4 o;
    for (int k = 0; k < 4; ++k) {
      const int e = i * 4 + k, t = e / MD, d = e % MD;
      const float v = blend_marker(rf, pr[k], predicted_marker(p, src, t, d));
      o[k] = v;
      if (t >= NT - THIS) s_mb[t - (NT - THIS)][d] = v;
      bad |= nonfin(v);
    }
    out4[i] = o;
  }
  __syncthreads();

  // ---- accumulated world frame of the next primitive, to every row of the group ---------------------------------------------
  for (int i = tid; i < ndst * 12; i += BLK) {
    const int n = i / 12, e = i % 12;
    if (e < 9) p.R0_out[(size_t)(dst0 + n) * 9 + e] = s_frame[12 + e];
    else p.T0_out[(size_t)(dst0 + n) * 3 + (e - 9)] = s_frame[12 + e];
  }
  // ---- next seed: markers of frames 18, 19 in (R_, T_), parameters with the new transl / glorot ---------------------------
  float Rn[9], Tn[3];
  for (int e = 0; e < 9; ++e) Rn[e] = s_frame[e];
  for (int e = 0; e < 3; ++e) Tn[e] = s_frame[9 + e];
  for (int i = tid; i < THIS * NM; i += BLK) {
    const int t = i / NM, m = i % NM;
    const float v[3] = {s_mb[t][m * 3 + 0] - Tn[0], s_mb[t][m * 3 + 1] - Tn[1], s_mb[t][m * 3 + 2] - Tn[2]};
    float ms[3];
    mat3T_vec(Rn, v, ms);
    for (int n = 0; n < ndst; ++n) {
      float* st = (t == 0 ? p.out_x0 : p.out_x1) + (size_t)(dst0 + n) * p.out_x_ld + m * 3;
      st[0] = ms[0]; st[1] = ms[1]; st[2] = ms[2];
    }
    bad |= nonfin(ms[0]) || nonfin(ms[1]) || nonfin(ms[2]);
  }
  for (int i = tid; i < THIS * XB; i += BLK) {
    const int t = i / XB, d = i % XB;
    const float v = (d < 6) ? s_seed6[t][d] : PP[(18 + t) * XB + d];
    for (int n = 0; n < ndst; ++n) p.out_seed[((size_t)(dst0 + n) * THIS + t) * XB + d] = v;
    bad |= nonfin(v);
  }
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (BEAM) {
    if (tid == 0 && any_bad) p.beam_status[rec] |= 4;
  } else {
    if (tid == 0 && any_bad && p.nonfinite) atomicAdd(p.nonfinite, 1);
  }
}

__global__ __launch_bounds__(BLK) void egx_primitive_advance_kernel(AdvanceArgs p) {
  const int b = blockIdx.x;
  advance_body<false>(p, b, b, b, 1);
}

// workgroup i hands sequence i on from candidate choice[i] of its num_candidates rows (a choice outside the group is clamped)
__global__ __launch_bounds__(BLK) void egx_primitive_advance_select_kernel(AdvanceArgs p, const int* __restrict__ choice, int N) {
  const int g = blockIdx.x;
  const int c = min(max(choice[g], 0), N - 1);
  advance_body<false>(p, g * N + c, g, g * N, N);
}

// workgroup (i, s) hands slot s of sequence i on from row beam_row[i,s] of the sequence's W * N rows (clamped into the group) to the
// N rows of slot s.  Another slot of the group may read the row this one overwrites: R0 / T0 and the seed frames go to other
// buffers than they are read from; pred_params, joints and markers are only read.
__global__ __launch_bounds__(BLK) void egx_primitive_advance_beam_kernel(AdvanceArgs p, const int* __restrict__ beam_row, int W, int N) {
  const int slot = blockIdx.x, g = slot / W;
  const int r = min(max(beam_row[slot], 0), W * N - 1);
  advance_body<true>(p, g * W * N + r, slot, slot * N, N);
}

// ---- scoring and selection -----------------------------------------------------------------------------------------------
// One workgroup of 8 waves per sequence.  A wave scores one candidate row at a time: its 64 lanes gather and blend the six feet
// markers of the 20 frames (360 values, the only markers the terms read) into the wave's slice of LDS, lanes 0..19 evaluate one
// frame each, the sums are wave shuffles in a fixed order, lane 0 adds the two scalar terms of the last body.  After the rows,
// wave 0 reduces (class, cost, index) over the N rows with a total order, so the result does not depend on the reduction tree.
namespace {

struct SelectArgs {
  const float* Y_gen;         // [18,B*N,201]
  const float* x0;
  const float* x1;
  const float* joints;        // [B*N*20,jpb,3]
  const float* markers_proj;  // [B*N*20,67,3]
  const float* R0;            // [B*N,9]
  const float* T0;            // [B*N,3]
  const int* pene_count;      // [B*N*20] or null
  const float* goal;          // [B,3]
  const int* feet_marker_idx; // [6]
  float w_goal, w_skate, w_floor, w_pene, w_face, pene_thres, goal_thresh, rf;
  int rows, N, jpb, x_ld;
  int* choice;                // [B]
  int* status;                // [B]
  int* reached;               // [B]
  float* goal_dist;           // [B]
  float* cost;                // [B*N]
  float* terms;               // [B*N,5] dist, skate, floor, pene, face
  int* colliding;             // [B*N]
  GeoFieldDev field;          // field.dist null: the goal term is the Euclidean distance
};

__device__ __forceinline__ float wave_sum(float v) {   // lane 0 holds the sum; fixed tree
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_down(v, o, 64));
  return v;
}
// The order of both selections, a total one: key class, then cost, then row index.  Greedy: class 0 clean, 1 colliding, 2 / 3 the
// same with a non-finite value, cost of the row.  Beam: class (non-finite, colliding nodes on the path), accumulated path cost.
__device__ __forceinline__ bool key_before(int ca, float xa, int ia, int cb, float xb, int ib) {
  if (ca != cb) return ca < cb;
  if (xa != xb) return xa < xb;
  return ia < ib;
}

// the carried state of the beam's slots and what its selection writes per kept slot
struct BeamArgs {
  const float* acc;      // [b,W] sum of q along the path into each slot
  const int* ncoll;      // [b,W] colliding nodes on it
  int* beam_row;         // [b,W] outputs per kept slot
  int* parent;
  float* acc_out;
  int* ncoll_out;
  float* path_cost;
  int* beam_status;
  float* goal_dist;
  int* reached;
  int W, N;
};

constexpr int NONFINITE_KEY = 1 << 30;   // above any count of colliding nodes on a path

// what lane 0 of the scoring wave knows of a row; q is the cost without its goal term, accumulated on its own
struct RowScore {
  float cost, q, dist;
  bool collides, finite;
};

// The row scoring of both searches: the 8 waves of the workgroup score the M rows of group g (rows g * M ...), one row per wave at
// a time; lane 0 of the wave writes cost / terms / colliding of the row and hands its RowScore to keep(n, score).  Ends on a
// barrier: what keep() put into LDS is visible to the whole workgroup.
template <class Keep>
__device__ __forceinline__ void score_group(const SelectArgs& p, int g, int M, float (*s_feet)[NT][NF * 3], Keep keep) {
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int feet_local[NF] = {0, 1, 2, 3, 4, 5};
  const float goal[3] = {p.goal[(size_t)g * 3 + 0], p.goal[(size_t)g * 3 + 1], p.goal[(size_t)g * 3 + 2]};

  for (int n0 = 0; n0 < M; n0 += SEL_WAVES) {      // the same trip count in every wave: the barriers are uniform
    const int n = n0 + w;
    const bool active = n < M;
    const size_t row = (size_t)g * M + (active ? n : 0);
    if (active)
      for (int e = lane; e < NT * NF * 3; e += 64) {
        const int t = e / (NF * 3), r = e % (NF * 3);
        const int m = min(max(p.feet_marker_idx[r / 3], 0), NM - 1), d = m * 3 + r % 3;
        const float pred = (t == 0)   ? p.x0[row * p.x_ld + d]
                           : (t == 1) ? p.x1[row * p.x_ld + d]
                                      : p.Y_gen[((size_t)(t - THIS) * p.rows + row) * MD + d];
        s_feet[w][t][r] = blend_marker(p.rf, p.markers_proj[(row * NT + t) * MD + d], pred);
      }
    __syncthreads();
    if (active) {
      float R0[9], T0[3];
      for (int e = 0; e < 9; ++e) R0[e] = p.R0[row * 9 + e];
      for (int e = 0; e < 3; ++e) T0[e] = p.T0[row * 3 + e];
      const auto feet_at = [&](int t, int i) { return s_feet[w][t][i]; };
      float sk = 0.f, fl = 0.f, cs = 0.f;
      int cm = 0;
      if (lane < 18) sk = reward_skate_frame(feet_at, lane, feet_local);   // central difference frames 1..18
      if (lane < NT) {
        fl = reward_floor_frame(R0, T0, feet_at, lane, feet_local);
        if (p.pene_count) {
          cm = p.pene_count[row * NT + lane];
          cs = (float)cm;
        }
      }
      const float skate = wave_sum(sk) / 18.f;
      const float floor_ = wave_sum(fl) / (float)NT;
      const float pene = reward_pene_arg(wave_sum(cs));
      const int cmax = wave_max(cm);
      if (lane == 0) {
        const float* j19 = p.joints + (row * NT + 19) * p.jpb * 3;
        float tl[3], dir[2];
        const float face = 1.f - reward_face(j19, R0, T0, goal, tl, dir);
        const float dist = target_distance(tl, j19);
        const float cost = p.w_goal * dist + p.w_skate * skate + p.w_floor * floor_ + p.w_pene * pene + p.w_face * face;
        const float q = p.w_skate * skate + p.w_floor * floor_ + p.w_pene * pene + p.w_face * face;
        const bool collides = p.pene_count && !((float)cmax < p.pene_thres);
        const bool finite = isfinite(cost) && isfinite(dist) && isfinite(skate) && isfinite(floor_) && isfinite(pene) && isfinite(face);
        p.cost[row] = cost;
        float* tm = p.terms + row * 5;
        tm[0] = dist; tm[1] = skate; tm[2] = floor_; tm[3] = pene; tm[4] = face;
        p.colliding[row] = collides ? 1 : 0;
        keep(n, RowScore{cost, q, dist, collides, finite});
      }
    }
    __syncthreads();
  }
}

// The goal term of a launch with a field.  score_group scores every row with the Euclidean distance, exactly as in a launch without
// a field; this then replaces, per row, terms[0] by the field of group g at the world xy of the row's last pelvis (R0 j19 + T0)
// and the cost by the sum with that term, every rounding stated (four rounded products added in order, the facing term as one
// fused multiply-add; the other terms are read back from `terms`), and returns the cost.  It is a phase of its own after
// score_group's closing barrier, one row per thread, and not a branch inside the scoring: any code added to the block that
// computes the distance, the facing term and the cost changes how the compiler vectorises and contracts THAT arithmetic (measured:
// last-bit changes of dist, face and cost against the build before the field came, with the field term inlined, out of line, and
// in a block of its own behind the scoring).
__device__ __forceinline__ float field_row_cost(const SelectArgs& p, int g, size_t row) {
  const float* R0 = p.R0 + row * 9;
  const float* T0 = p.T0 + row * 3;
  const float* j19 = p.joints + (row * NT + 19) * p.jpb * 3;
  const float x = fmaf(R0[2], j19[2], fmaf(R0[1], j19[1], R0[0] * j19[0])) + T0[0];
  const float y = fmaf(R0[5], j19[2], fmaf(R0[4], j19[1], R0[3] * j19[0])) + T0[1];
  const float geo = egx_geodesic_sample_group(p.field, g, x, y);
  float* tm = p.terms + row * 5;
  const float sum4 = egx_add(egx_add(egx_add(egx_mul(p.w_goal, geo), egx_mul(p.w_skate, tm[1])), egx_mul(p.w_floor, tm[2])),
                             egx_mul(p.w_pene, tm[3]));
  const float cost = fmaf(p.w_face, tm[4], sum4);      // NaN for a NaN position: the row then ranks as non-finite
  tm[0] = geo;
  p.cost[row] = cost;
  return cost;
}

__device__ __forceinline__ float wave_min(float v) {   // every lane's partner chain ends in lane 0; min is order-free
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_down(v, o, 64));
  return v;
}

// The obstacle term and veto of a launch with obstacles: a phase of its own after score_group's closing barrier and after the
// field phase, for the reason field_row_cost states.  The workgroup stages the window of group g's set into LDS once (every row
// of a group shares the time window and the set), then a wave takes one row at a time: lanes 0..17 one predicted frame each
// (t = lane + 2; the world xy of the frame's pelvis with field_row_cost's nesting, then the obstacles in LDS), the frame sum by
// the fixed wave_sum tree, divided by 18; clearance by wave_min.  Lane 0 writes obs_term / obs_clearance / obs_hit and the row's
// cost = cost_prev + w_obs * term (cost_prev read back: what the launch wrote so far), both rounded on their own, and hands
// (n, row, term, cost, hit) to update(), which redoes the LDS key tables of the row.  Ends on a barrier.
//
// TABLE (the marker model of recorded tracks, entries *_obstacle_markers): nothing is staged and c_t is read from ob.frame_clearance
// [rows,18], which egx_obstacle_marker_clearance (genop_obstacle_markers.hip) wrote ahead of the launch; everything after c_t is the
// same code.  A compile-time variant and not a branch: the cylinder instantiation is the code as it stood before the table came.
template <bool TABLE, class Update>
__device__ __forceinline__ void obstacle_group(const SelectArgs& p, const ObstaclesDev& ob, int g, int M, Update update) {
  __shared__ float s_ox[EGX_OBS_FRAMES][EGX_MAX_OBSTACLES], s_oy[EGX_OBS_FRAMES][EGX_MAX_OBSTACLES], s_rr[EGX_MAX_OBSTACLES];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  int cnt = 0;
  if constexpr (!TABLE) {
    cnt = egx_obstacles_stage(ob, g, s_ox, s_oy, s_rr);
    __syncthreads();
  }
  for (int n = w; n < M; n += SEL_WAVES) {
    const size_t row = (size_t)g * M + n;
    float c = __builtin_inff(), pen = 0.f;
    int bad = 0;
    if (lane < EGX_OBS_FRAMES) {
      if constexpr (TABLE) {
        c = ob.frame_clearance[row * EGX_OBS_FRAMES + lane];
      } else {
        const float* R0 = p.R0 + row * 9;
        const float* T0 = p.T0 + row * 3;
        const float* j = p.joints + (row * NT + THIS + lane) * p.jpb * 3;
        const float x = fmaf(R0[2], j[2], fmaf(R0[1], j[1], R0[0] * j[0])) + T0[0];
        const float y = fmaf(R0[5], j[2], fmaf(R0[4], j[1], R0[3] * j[0])) + T0[1];
        c = egx_obstacle_clearance(x, y, cnt, s_ox[lane], s_oy[lane], s_rr);
      }
      bad = isnan(c) ? 1 : 0;
      pen = bad ? c : fmaxf(0.f, egx_sub(ob.margin, c));
    }
    const float sum = wave_sum(pen);                       // NaN where a frame is NaN
    const float cmin = wave_min(bad ? __builtin_inff() : c);
    const int any_bad = wave_max(bad);
    if (lane == 0) {
      const float term = sum / (float)EGX_OBS_FRAMES;
      const float clearance = any_bad ? __builtin_nanf("") : cmin;
      const bool hit = clearance < 0.f;                    // false for NaN
      const float cost = egx_add(p.cost[row], egx_mul(ob.w, term));
      ob.term[row] = term;
      ob.clearance[row] = clearance;
      ob.hit[row] = hit ? 1 : 0;
      p.cost[row] = cost;
      update(n, row, term, cost, hit);
    }
  }
  __syncthreads();
}

}  // namespace

namespace {
// the body of the greedy selection kernels; TABLE: the obstacle phase reads its frame clearances from a table (obstacle_group)
template <bool TABLE>
__device__ __forceinline__ void select_body(const SelectArgs& p, const ObstaclesDev& ob) {
  __shared__ float s_feet[SEL_WAVES][NT][NF * 3];   // blended feet markers of the row a wave is scoring
  __shared__ float s_cost[MAXC], s_dist[MAXC];
  __shared__ int s_cls[MAXC];
  const int g = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63, N = p.N;
  score_group(p, g, N, s_feet, [&](int n, const RowScore& r) {
    s_cost[n] = r.finite ? r.cost : 0.f;      // a non-finite row is ranked by collision and index only
    s_dist[n] = r.dist;
    s_cls[n] = (r.finite ? 0 : 2) | (r.collides ? 1 : 0);
  });
  if (p.field.dist) {                          // workgroup-uniform; score_group ended on a barrier: the rows' terms are visible
    for (int n = tid; n < N; n += SEL_BLK) {
      const float c = field_row_cost(p, g, (size_t)g * N + n);
      const bool finite = !(s_cls[n] & 2) && isfinite(c);
      s_cost[n] = finite ? c : 0.f;
      s_cls[n] = (finite ? 0 : 2) | (s_cls[n] & 1);
    }
    __syncthreads();
  }
  if (ob.term)                                 // workgroup-uniform; the costs of the rows are visible: a barrier precedes
    obstacle_group<TABLE>(p, ob, g, N, [&](int n, size_t row, float term, float c, bool hit) {
      const bool finite = !(s_cls[n] & 2) && isfinite(term) && isfinite(c);
      const int coll = (s_cls[n] & 1) | (hit ? 1 : 0);
      p.colliding[row] = coll;
      s_cost[n] = finite ? c : 0.f;
      s_cls[n] = (finite ? 0 : 2) | coll;
    });

  if (w == 0) {
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
      const float dist = s_dist[bi];
      p.choice[g] = bi;
      p.status[g] = (bc & 1) | (bc & 2);
      p.reached[g] = (dist < p.goal_thresh) ? 1 : 0;
      p.goal_dist[g] = dist;
    }
  }
}
}  // namespace

__global__ __launch_bounds__(SEL_BLK) void egx_primitive_select_kernel(SelectArgs p, ObstaclesDev ob) { select_body<false>(p, ob); }
__global__ __launch_bounds__(SEL_BLK) void egx_primitive_select_obstacle_markers_kernel(SelectArgs p, ObstaclesDev ob) {
  select_body<true>(p, ob);
}

// ---- beam: scoring and top-W selection -------------------------------------------------------------------------------------
// One workgroup per sequence scores its W * N rows as above, then every row counts the rows whose path key precedes its own:
// (non-finite, colliding nodes on the path, accumulated cost, row index) is a total order, so that count is the row's rank
// whatever the order of the comparisons, and the rows of rank < W are the beam, slot = rank.
namespace {
template <bool TABLE>
__device__ __forceinline__ void beam_select_body(const SelectArgs& p, const BeamArgs& q, const ObstaclesDev& ob) {
  __shared__ float s_feet[SEL_WAVES][NT][NF * 3];
  __shared__ float s_path[MAXC], s_q[MAXC], s_dist[MAXC];   // path cost (0 where non-finite), q and dist of every row
  __shared__ int s_key[MAXC], s_flag[MAXC];                 // (non-finite, colliding nodes) in one int; bit 0 collides, bit 1 non-finite
  const int g = blockIdx.x, tid = threadIdx.x, W = q.W, N = q.N, M = W * N;
  score_group(p, g, M, s_feet, [&](int n, const RowScore& r) {
    const int s = n / N;
    const float path = q.acc[(size_t)g * W + s] + (r.finite ? r.cost : 0.f);
    const int nc = q.ncoll[(size_t)g * W + s] + (r.collides ? 1 : 0);
    const bool finite = r.finite && isfinite(path);          // a path through a non-finite node stays non-finite
    s_path[n] = finite ? path : 0.f;
    s_q[n] = r.q;
    s_dist[n] = r.dist;
    s_key[n] = finite ? min(max(nc, 0), NONFINITE_KEY - 1) : NONFINITE_KEY + min(max(nc, 0), NONFINITE_KEY - 1);
    s_flag[n] = (r.collides ? 1 : 0) | (finite ? 0 : 2);
  });
  if (p.field.dist) {                          // as in the greedy kernel; the path key of every row again with the field's cost
    for (int n = tid; n < M; n += SEL_BLK) {
      const float c = field_row_cost(p, g, (size_t)g * M + n);
      const bool row_finite = !(s_flag[n] & 2) && isfinite(c);
      const float path = q.acc[(size_t)g * W + n / N] + (row_finite ? c : 0.f);
      const bool finite = row_finite && isfinite(path);
      const int nc = s_key[n] & (NONFINITE_KEY - 1);
      s_path[n] = finite ? path : 0.f;
      s_key[n] = finite ? nc : NONFINITE_KEY + nc;
      s_flag[n] = (s_flag[n] & 1) | (finite ? 0 : 2);
    }
    __syncthreads();
  }
  if (ob.term)                                 // as in the greedy kernel; q gains the product the cost gained, a hit is a colliding node
    obstacle_group<TABLE>(p, ob, g, M, [&](int n, size_t row, float term, float c, bool hit) {
      const bool row_finite = !(s_flag[n] & 2) && isfinite(term) && isfinite(c);
      const float path = q.acc[(size_t)g * W + n / N] + (row_finite ? c : 0.f);
      const bool finite = row_finite && isfinite(path);
      const int coll = (s_flag[n] & 1) | (hit ? 1 : 0);
      const int nc = min(max(q.ncoll[(size_t)g * W + n / N] + coll, 0), NONFINITE_KEY - 1);
      p.colliding[row] = coll;
      s_q[n] = egx_add(s_q[n], egx_mul(ob.w, term));
      s_path[n] = finite ? path : 0.f;
      s_key[n] = finite ? nc : NONFINITE_KEY + nc;
      s_flag[n] = coll | (finite ? 0 : 2);
    });

  if (tid < M) {
    const int kc = s_key[tid];
    const float kx = s_path[tid];
    int rank = 0;
    for (int m = 0; m < M; ++m) rank += key_before(s_key[m], s_path[m], m, kc, kx, tid) ? 1 : 0;
    if (rank < W) {
      const int s = tid / N;
      const size_t o = (size_t)g * W + rank;
      q.beam_row[o] = tid;
      q.parent[o] = s;
      q.acc_out[o] = q.acc[(size_t)g * W + s] + s_q[tid];
      q.ncoll_out[o] = q.ncoll[(size_t)g * W + s] + (s_flag[tid] & 1);
      q.path_cost[o] = kx;
      q.beam_status[o] = s_flag[tid];
      q.goal_dist[o] = s_dist[tid];
      q.reached[o] = (s_dist[tid] < p.goal_thresh) ? 1 : 0;
    }
  }
}
}  // namespace

__global__ __launch_bounds__(SEL_BLK) void egx_primitive_beam_select_kernel(SelectArgs p, BeamArgs q, ObstaclesDev ob) {
  beam_select_body<false>(p, q, ob);
}
__global__ __launch_bounds__(SEL_BLK) void egx_primitive_beam_select_obstacle_markers_kernel(SelectArgs p, BeamArgs q, ObstaclesDev ob) {
  beam_select_body<true>(p, q, ob);
}

// ---- beam: the returned path --------------------------------------------------------------------------------------------
// Workgroup (k, i) walks from slot 0 of the last depth back to depth k along `parent` and copies the records of the slot it lands
// on into row (k, i) of the [K,b,...] outputs.
namespace {

struct BacktrackArgs {
  const int* parent;         // [K,b,W]
  const int* beam_row;       // [K,b,W] per-slot records of the selection ...
  const int* beam_status;
  const float* goal_dist;
  const int* reached;
  const float* rec_marker_b; // [K,b,W,20,67,3] ... and of the hand-off
  const float* rec_pelvis;   // [K,b,W,20,3]
  const float* rec_R;        // [K,b,W,9]
  const float* rec_T;        // [K,b,W,3]
  const float* rec_params;   // [K,b,W,20,93]
  int K, b, W;
  int* path_slot;            // [K,b]
  int* choice;
  int* status;
  float* out_goal_dist;
  int* out_reached;
  float* out_marker_b;       // [K,b,20,67,3]
  float* out_pelvis;
  float* out_R;
  float* out_T;
  float* out_params;
};

constexpr int NP4 = NT * XB / 4;
static_assert(NT * XB % 4 == 0, "a sequence's parameters are whole float4 packets");

}  // namespace

__global__ __launch_bounds__(BLK) void egx_beam_backtrack_kernel(BacktrackArgs p) {
  const int k = blockIdx.x / p.b, i = blockIdx.x % p.b, tid = threadIdx.x, W = p.W;
  int slot = 0;                                               // every lane walks the same few words
  for (int d = p.K - 1; d > k; --d) slot = min(max(p.parent[((size_t)d * p.b + i) * W + slot], 0), W - 1);
  const size_t src = ((size_t)k * p.b + i) * W + slot, dst = (size_t)k * p.b + i;
  if (tid == 0) {
    p.path_slot[dst] = slot;
    p.choice[dst] = p.beam_row[src];
    p.status[dst] = p.beam_status[src];
    p.out_goal_dist[dst] = p.goal_dist[src];
    p.out_reached[dst] = p.reached[src];
  }
  const f32x4* m4 = reinterpret_cast<const f32x4*>(p.rec_marker_b + src * NT * MD);
  f32x4* om4 = reinterpret_cast<f32x4*>(p.out_marker_b + dst * NT * MD);
  for (int e = tid; e < NV4; e += BLK) om4[e] = m4[e];
  const f32x4* p4 = reinterpret_cast<const f32x4*>(p.rec_params + src * NT * XB);
  f32x4* op4 = reinterpret_cast<f32x4*>(p.out_params + dst * NT * XB);
  for (int e = tid; e < NP4; e += BLK) op4[e] = p4[e];
  if (tid < NT * 3) p.out_pelvis[dst * NT * 3 + tid] = p.rec_pelvis[src * NT * 3 + tid];
  if (tid >= 64 && tid < 64 + 9) p.out_R[dst * 9 + (tid - 64)] = p.rec_R[src * 9 + (tid - 64)];
  if (tid >= 128 && tid < 128 + 3) p.out_T[dst * 3 + (tid - 128)] = p.rec_T[src * 3 + (tid - 128)];
}

// ---- host: one argument path per kernel family --------------------------------------------------------------------------
namespace {

// What the three hand-off entries share: the checks on their common arguments, the fields these fill, the launch check.  `launch`
// sets what is the entry's own (R0_out / T0_out, out_params, nonfinite, beam_status: null unless set; B) and launches its kernel.
// EGX_REQUIRE returns from the function it stands in: the entry checks its own arguments first, then returns this one's result.
template <class Launch>
int advance_entry(const float* pred_params, const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints,
                  int joints_per_body, const float* markers_proj, const float* delta_T, float reproj_factor, int num_sequences,
                  const float* R0, const float* T0, float* out_marker_b, float* out_pelvis, float* out_R, float* out_T,
                  float* out_seed_params, float* out_x0, float* out_x1, int out_x_ld, Launch launch) {
  EGX_REQUIRE(pred_params && Y_gen && x0 && x1 && joints && markers_proj && delta_T && R0 && T0, "null input");
  EGX_REQUIRE(out_marker_b && out_pelvis && out_R && out_T && out_seed_params && out_x0 && out_x1, "null output");
  EGX_REQUIRE(num_sequences > 0 && joints_per_body >= 3, "need a non-empty batch and >= 3 joints per body");
  EGX_REQUIRE(x_ld >= MD && out_x_ld >= MD, "a seed frame holds 201 floats: the row strides cannot be smaller");
  EGX_REQUIRE(((uintptr_t)markers_proj & 15) == 0 && ((uintptr_t)out_marker_b & 15) == 0,
              "markers_proj and out_marker_b must be 16-byte aligned");
  AdvanceArgs p{};
  p.pred_params = pred_params; p.Y_gen = Y_gen; p.x0 = x0; p.x1 = x1; p.joints = joints; p.markers_proj = markers_proj;
  p.delta_T = delta_T; p.R0 = R0; p.T0 = T0; p.out_marker_b = out_marker_b; p.out_pelvis = out_pelvis; p.out_R = out_R;
  p.out_T = out_T; p.out_seed = out_seed_params; p.out_x0 = out_x0; p.out_x1 = out_x1;
  p.rf = reproj_factor; p.jpb = joints_per_body; p.x_ld = x_ld; p.out_x_ld = out_x_ld;
  launch(p);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

// The same for the selection entries, for num_sequences groups of `group_rows` rows; `launch` sets the per-group outputs of
// the greedy selection (null unless set; the beam's are in BeamArgs) and launches with the obstacle descriptor it is handed: `obs`
// checked, or a null one (no phase) where obs is null.
template <class Launch>
int select_entry(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints, int joints_per_body,
                 const float* markers_proj, const float* R0, const float* T0, const int32_t* pene_count, const float* goal,
                 const int32_t* feet_marker_idx, const float* weights, float pene_thres, float goal_thresh, float reproj_factor,
                 int num_sequences, int group_rows, float* cost, float* cost_terms, int32_t* colliding, const GeoFieldDev& field,
                 const ObstaclesDev* obs, Launch launch) {
  EGX_REQUIRE(Y_gen && x0 && x1 && joints && markers_proj && R0 && T0 && goal && feet_marker_idx && weights, "null input");
  EGX_REQUIRE(cost && cost_terms && colliding, "null output");
  EGX_REQUIRE(num_sequences > 0 && joints_per_body >= 3, "need a non-empty batch and >= 3 joints per body");
  EGX_REQUIRE(x_ld >= MD, "a seed frame holds 201 floats: the row stride cannot be smaller");
  if (field.dist) {
    EGX_REQUIRE(field.origin && field.H >= 1 && field.W >= 1 && field.F >= 1, "a field needs its origin, size and count");
    EGX_REQUIRE(field.cell > 0.f && field.cell < __builtin_inff(), "field_cell must be positive and finite");
    EGX_REQUIRE((long long)field.F * field.H * field.W <= 0x7fffffffLL, "the fields must stay below 2^31 cells");
  }
  SelectArgs p{};
  p.Y_gen = Y_gen; p.x0 = x0; p.x1 = x1; p.joints = joints; p.markers_proj = markers_proj; p.R0 = R0; p.T0 = T0;
  p.pene_count = pene_count; p.goal = goal; p.feet_marker_idx = feet_marker_idx;
  p.w_goal = weights[0]; p.w_skate = weights[1]; p.w_floor = weights[2]; p.w_pene = weights[3]; p.w_face = weights[4];
  p.pene_thres = pene_thres; p.goal_thresh = goal_thresh; p.rf = reproj_factor;
  p.rows = num_sequences * group_rows; p.N = group_rows; p.jpb = joints_per_body; p.x_ld = x_ld;
  p.cost = cost; p.terms = cost_terms; p.colliding = colliding;
  if (field.dist) p.field = field;
  ObstaclesDev ob{};
  if (obs) {
    EGX_REQUIRE(obs->term && obs->clearance && obs->hit, "null obstacle output");
    EGX_REQUIRE(obs->O_max >= 0 && obs->O_max <= EGX_MAX_OBSTACLES, "max_obstacles must be in [0, EGX_MAX_OBSTACLES]");
    EGX_REQUIRE(obs->O_max == 0 || (obs->xy && obs->radius && obs->count), "obstacles need obs_xy, obs_radius and obs_count");
    EGX_REQUIRE(obs->T >= 1 && obs->S >= 1, "num_frames and num_sets must be at least 1");
    EGX_REQUIRE(obs->margin >= 0.f && obs->body_radius >= 0.f, "margin and body_radius must not be negative");
    ob = *obs;
  }
  launch(p, ob);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

// the greedy selection behind egx_primitive_select, _select_field and _select_obstacles: its own checks, then select_entry
int greedy_select(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints, int joints_per_body,
                  const float* markers_proj, const float* R0, const float* T0, const int32_t* pene_count, const float* goal,
                  const int32_t* feet_marker_idx, const float* weights, float pene_thres, float goal_thresh, float reproj_factor,
                  int num_sequences, int num_candidates, int32_t* choice, int32_t* status, int32_t* reached, float* goal_dist, float* cost,
                  float* cost_terms, int32_t* colliding, const GeoFieldDev& field, const ObstaclesDev* obs, void* stream) {
  EGX_REQUIRE(choice && status && reached && goal_dist, "null output");
  EGX_REQUIRE(num_candidates >= 1 && num_candidates <= MAXC, "num_candidates must be in [1, EGX_MAX_CANDIDATES]");
  return select_entry(Y_gen, x0, x1, x_ld, joints, joints_per_body, markers_proj, R0, T0, pene_count, goal, feet_marker_idx, weights,
                      pene_thres, goal_thresh, reproj_factor, num_sequences, num_candidates, cost, cost_terms, colliding, field, obs,
                      [&](SelectArgs& p, const ObstaclesDev& ob) {
    p.choice = choice; p.status = status; p.reached = reached; p.goal_dist = goal_dist;
    hipLaunchKernelGGL(ob.frame_clearance ? egx_primitive_select_obstacle_markers_kernel : egx_primitive_select_kernel, dim3(num_sequences),
                       dim3(SEL_BLK), 0, static_cast<hipStream_t>(stream), p, ob);
  });
}

// the beam selection behind egx_primitive_beam_select, _beam_select_field and _beam_select_obstacles
int beam_select(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints, int joints_per_body,
                const float* markers_proj, const float* R0, const float* T0, const int32_t* pene_count, const float* goal,
                const int32_t* feet_marker_idx, const float* weights, float pene_thres, float goal_thresh, float reproj_factor,
                int num_sequences, int beam_width, int num_candidates, const float* acc, const int32_t* ncoll, float* cost,
                float* cost_terms, int32_t* colliding, int32_t* beam_row, int32_t* parent, float* acc_out, int32_t* ncoll_out,
                float* path_cost, int32_t* beam_status, float* goal_dist, int32_t* reached, const GeoFieldDev& field,
                const ObstaclesDev* obs, void* stream) {
  EGX_REQUIRE(acc && ncoll, "null input");
  EGX_REQUIRE(beam_row && parent && acc_out && ncoll_out && path_cost && beam_status && goal_dist && reached, "null output");
  EGX_REQUIRE(beam_width >= 1 && beam_width <= EGX_MAX_BEAM, "beam_width must be in [1, EGX_MAX_BEAM]");
  EGX_REQUIRE(num_candidates >= 1 && num_candidates <= MAXC && beam_width * num_candidates <= MAXC,
              "beam_width * num_candidates must be in [1, EGX_MAX_CANDIDATES]");
  EGX_REQUIRE(acc != acc_out && ncoll != ncoll_out, "acc / ncoll are read from one buffer and written to another");
  return select_entry(Y_gen, x0, x1, x_ld, joints, joints_per_body, markers_proj, R0, T0, pene_count, goal, feet_marker_idx, weights,
                      pene_thres, goal_thresh, reproj_factor, num_sequences, beam_width * num_candidates, cost, cost_terms, colliding,
                      field, obs, [&](SelectArgs& p, const ObstaclesDev& ob) {
    const BeamArgs q{acc, ncoll, beam_row, parent, acc_out, ncoll_out, path_cost, beam_status, goal_dist, reached, beam_width, num_candidates};
    hipLaunchKernelGGL(ob.frame_clearance ? egx_primitive_beam_select_obstacle_markers_kernel : egx_primitive_beam_select_kernel,
                       dim3(num_sequences), dim3(SEL_BLK), 0, static_cast<hipStream_t>(stream), p, q, ob);
  });
}

}  // namespace

extern "C" int egx_primitive_advance(const float* pred_params, const float* Y_gen, const float* x0, const float* x1, int x_ld,
                                     const float* joints, int joints_per_body, const float* markers_proj, const float* delta_T,
                                     float reproj_factor, int num_sequences, float* R0, float* T0, float* out_marker_b,
                                     float* out_pelvis, float* out_R, float* out_T, float* out_seed_params, float* out_x0,
                                     float* out_x1, int out_x_ld, int32_t* nonfinite, void* stream) {
  return advance_entry(pred_params, Y_gen, x0, x1, x_ld, joints, joints_per_body, markers_proj, delta_T, reproj_factor, num_sequences,
                       R0, T0, out_marker_b, out_pelvis, out_R, out_T, out_seed_params, out_x0, out_x1, out_x_ld, [&](AdvanceArgs& p) {
    p.R0_out = R0; p.T0_out = T0; p.nonfinite = nonfinite; p.B = num_sequences;
    hipLaunchKernelGGL(egx_primitive_advance_kernel, dim3(num_sequences), dim3(BLK), 0, static_cast<hipStream_t>(stream), p);
  });
}

extern "C" int egx_primitive_select_field(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints,
                                          int joints_per_body, const float* markers_proj, const float* R0, const float* T0,
                                          const int32_t* pene_count, const float* goal, const int32_t* feet_marker_idx,
                                          const float* weights, float pene_thres, float goal_thresh, float reproj_factor,
                                          int num_sequences, int num_candidates, int32_t* choice, int32_t* status, int32_t* reached,
                                          float* goal_dist, float* cost, float* cost_terms, int32_t* colliding, const float* field_dist,
                                          const float* field_origin, float field_cell, int field_H, int field_W, int num_fields,
                                          const int32_t* field_index, void* stream) {
  return greedy_select(Y_gen, x0, x1, x_ld, joints, joints_per_body, markers_proj, R0, T0, pene_count, goal, feet_marker_idx, weights,
                       pene_thres, goal_thresh, reproj_factor, num_sequences, num_candidates, choice, status, reached, goal_dist, cost,
                       cost_terms, colliding, GeoFieldDev{field_dist, field_origin, field_index, field_cell, field_H, field_W, num_fields},
                       nullptr, stream);
}

// egx_primitive_select_field with the marker model of recorded tracks: the obstacle phase on a table of frame clearances
extern "C" int egx_primitive_select_obstacle_markers(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints,
                                                     int joints_per_body, const float* markers_proj, const float* R0, const float* T0,
                                                     const int32_t* pene_count, const float* goal, const int32_t* feet_marker_idx,
                                                     const float* weights, float pene_thres, float goal_thresh, float reproj_factor,
                                                     int num_sequences, int num_candidates, int32_t* choice, int32_t* status,
                                                     int32_t* reached, float* goal_dist, float* cost, float* cost_terms, int32_t* colliding,
                                                     const float* field_dist, const float* field_origin, float field_cell, int field_H,
                                                     int field_W, int num_fields, const int32_t* field_index, const float* frame_clearance,
                                                     float obstacle_weight, float margin, float* obs_term, float* obs_clearance,
                                                     int32_t* obs_hit, void* stream) {
  EGX_REQUIRE(frame_clearance, "null input");
  const ObstaclesDev obs{nullptr, nullptr, nullptr, nullptr, 1, 0, 1, 0, obstacle_weight, margin, 0.f, obs_term, obs_clearance, obs_hit,
                         frame_clearance};
  return greedy_select(Y_gen, x0, x1, x_ld, joints, joints_per_body, markers_proj, R0, T0, pene_count, goal, feet_marker_idx, weights,
                       pene_thres, goal_thresh, reproj_factor, num_sequences, num_candidates, choice, status, reached, goal_dist, cost,
                       cost_terms, colliding, GeoFieldDev{field_dist, field_origin, field_index, field_cell, field_H, field_W, num_fields},
                       &obs, stream);
}

// extends egx_primitive_select_field
extern "C" int egx_primitive_select_obstacles(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints,
                                              int joints_per_body, const float* markers_proj, const float* R0, const float* T0,
                                              const int32_t* pene_count, const float* goal, const int32_t* feet_marker_idx,
                                              const float* weights, float pene_thres, float goal_thresh, float reproj_factor,
                                              int num_sequences, int num_candidates, int32_t* choice, int32_t* status, int32_t* reached,
                                              float* goal_dist, float* cost, float* cost_terms, int32_t* colliding,
                                              const float* field_dist, const float* field_origin, float field_cell, int field_H,
                                              int field_W, int num_fields, const int32_t* field_index, const float* obs_xy,
                                              const float* obs_radius, const int32_t* obs_count, const int32_t* obs_index, int num_sets,
                                              int max_obstacles, int num_frames, int frame0, float obstacle_weight, float margin,
                                              float body_radius, float* obs_term, float* obs_clearance, int32_t* obs_hit, void* stream) {
  const ObstaclesDev obs{obs_xy, obs_radius, obs_count, obs_index, num_sets, max_obstacles, num_frames, frame0, obstacle_weight, margin,
                         body_radius, obs_term, obs_clearance, obs_hit};
  return greedy_select(Y_gen, x0, x1, x_ld, joints, joints_per_body, markers_proj, R0, T0, pene_count, goal, feet_marker_idx, weights,
                       pene_thres, goal_thresh, reproj_factor, num_sequences, num_candidates, choice, status, reached, goal_dist, cost,
                       cost_terms, colliding, GeoFieldDev{field_dist, field_origin, field_index, field_cell, field_H, field_W, num_fields},
                       &obs, stream);
}

extern "C" int egx_primitive_select(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints,
                                    int joints_per_body, const float* markers_proj, const float* R0, const float* T0,
                                    const int32_t* pene_count, const float* goal, const int32_t* feet_marker_idx,
                                    const float* weights, float pene_thres, float goal_thresh, float reproj_factor,
                                    int num_sequences, int num_candidates, int32_t* choice, int32_t* status, int32_t* reached,
                                    float* goal_dist, float* cost, float* cost_terms, int32_t* colliding, void* stream) {
  return egx_primitive_select_field(Y_gen, x0, x1, x_ld, joints, joints_per_body, markers_proj, R0, T0, pene_count, goal, feet_marker_idx,
                                    weights, pene_thres, goal_thresh, reproj_factor, num_sequences, num_candidates, choice, status, reached,
                                    goal_dist, cost, cost_terms, colliding, nullptr, nullptr, 0.f, 0, 0, 0, nullptr, stream);
}

extern "C" int egx_primitive_advance_select(const float* pred_params, const float* Y_gen, const float* x0, const float* x1, int x_ld,
                                            const float* joints, int joints_per_body, const float* markers_proj,
                                            const float* delta_T, float reproj_factor, int num_sequences, const int32_t* choice,
                                            int num_candidates, float* R0, float* T0, float* out_marker_b, float* out_pelvis,
                                            float* out_R, float* out_T, float* out_params, float* out_seed_params, float* out_x0,
                                            float* out_x1, int out_x_ld, int32_t* nonfinite, void* stream) {
  EGX_REQUIRE(choice, "null input");
  EGX_REQUIRE(num_candidates >= 1 && num_candidates <= MAXC, "num_candidates must be in [1, EGX_MAX_CANDIDATES]");
  return advance_entry(pred_params, Y_gen, x0, x1, x_ld, joints, joints_per_body, markers_proj, delta_T, reproj_factor, num_sequences,
                       R0, T0, out_marker_b, out_pelvis, out_R, out_T, out_seed_params, out_x0, out_x1, out_x_ld, [&](AdvanceArgs& p) {
    p.R0_out = R0; p.T0_out = T0; p.out_params = out_params; p.nonfinite = nonfinite; p.B = num_sequences * num_candidates;
    hipLaunchKernelGGL(egx_primitive_advance_select_kernel, dim3(num_sequences), dim3(BLK), 0, static_cast<hipStream_t>(stream), p,
                       choice, num_candidates);
  });
}

extern "C" int egx_primitive_beam_select_field(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints,
                                               int joints_per_body, const float* markers_proj, const float* R0, const float* T0,
                                               const int32_t* pene_count, const float* goal, const int32_t* feet_marker_idx,
                                               const float* weights, float pene_thres, float goal_thresh, float reproj_factor,
                                               int num_sequences, int beam_width, int num_candidates, const float* acc,
                                               const int32_t* ncoll, float* cost, float* cost_terms, int32_t* colliding,
                                               int32_t* beam_row, int32_t* parent, float* acc_out, int32_t* ncoll_out, float* path_cost,
                                               int32_t* beam_status, float* goal_dist, int32_t* reached, const float* field_dist,
                                               const float* field_origin, float field_cell, int field_H, int field_W, int num_fields,
                                               const int32_t* field_index, void* stream) {
  return beam_select(Y_gen, x0, x1, x_ld, joints, joints_per_body, markers_proj, R0, T0, pene_count, goal, feet_marker_idx, weights,
                     pene_thres, goal_thresh, reproj_factor, num_sequences, beam_width, num_candidates, acc, ncoll, cost, cost_terms,
                     colliding, beam_row, parent, acc_out, ncoll_out, path_cost, beam_status, goal_dist, reached,
                     GeoFieldDev{field_dist, field_origin, field_index, field_cell, field_H, field_W, num_fields}, nullptr, stream);
}

// egx_primitive_beam_select_field with the marker model of recorded tracks
extern "C" int egx_primitive_beam_select_obstacle_markers(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints,
                                                          int joints_per_body, const float* markers_proj, const float* R0, const float* T0,
                                                          const int32_t* pene_count, const float* goal, const int32_t* feet_marker_idx,
                                                          const float* weights, float pene_thres, float goal_thresh, float reproj_factor,
                                                          int num_sequences, int beam_width, int num_candidates, const float* acc,
                                                          const int32_t* ncoll, float* cost, float* cost_terms, int32_t* colliding,
                                                          int32_t* beam_row, int32_t* parent, float* acc_out, int32_t* ncoll_out,
                                                          float* path_cost, int32_t* beam_status, float* goal_dist, int32_t* reached,
                                                          const float* field_dist, const float* field_origin, float field_cell,
                                                          int field_H, int field_W, int num_fields, const int32_t* field_index,
                                                          const float* frame_clearance, float obstacle_weight, float margin,
                                                          float* obs_term, float* obs_clearance, int32_t* obs_hit, void* stream) {
  EGX_REQUIRE(frame_clearance, "null input");
  const ObstaclesDev obs{nullptr, nullptr, nullptr, nullptr, 1, 0, 1, 0, obstacle_weight, margin, 0.f, obs_term, obs_clearance, obs_hit,
                         frame_clearance};
  return beam_select(Y_gen, x0, x1, x_ld, joints, joints_per_body, markers_proj, R0, T0, pene_count, goal, feet_marker_idx, weights,
                     pene_thres, goal_thresh, reproj_factor, num_sequences, beam_width, num_candidates, acc, ncoll, cost, cost_terms,
                     colliding, beam_row, parent, acc_out, ncoll_out, path_cost, beam_status, goal_dist, reached,
                     GeoFieldDev{field_dist, field_origin, field_index, field_cell, field_H, field_W, num_fields}, &obs, stream);
}

// extends egx_primitive_beam_select_field
extern "C" int egx_primitive_beam_select_obstacles(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints,
                                                   int joints_per_body, const float* markers_proj, const float* R0, const float* T0,
                                                   const int32_t* pene_count, const float* goal, const int32_t* feet_marker_idx,
                                                   const float* weights, float pene_thres, float goal_thresh, float reproj_factor,
                                                   int num_sequences, int beam_width, int num_candidates, const float* acc,
                                                   const int32_t* ncoll, float* cost, float* cost_terms, int32_t* colliding,
                                                   int32_t* beam_row, int32_t* parent, float* acc_out, int32_t* ncoll_out,
                                                   float* path_cost, int32_t* beam_status, float* goal_dist, int32_t* reached,
                                                   const float* field_dist, const float* field_origin, float field_cell, int field_H,
                                                   int field_W, int num_fields, const int32_t* field_index, const float* obs_xy,
                                                   const float* obs_radius, const int32_t* obs_count, const int32_t* obs_index,
                                                   int num_sets, int max_obstacles, int num_frames, int frame0, float obstacle_weight,
                                                   float margin, float body_radius, float* obs_term, float* obs_clearance,
                                                   int32_t* obs_hit, void* stream) {
  const ObstaclesDev obs{obs_xy, obs_radius, obs_count, obs_index, num_sets, max_obstacles, num_frames, frame0, obstacle_weight, margin,
                         body_radius, obs_term, obs_clearance, obs_hit};
  return beam_select(Y_gen, x0, x1, x_ld, joints, joints_per_body, markers_proj, R0, T0, pene_count, goal, feet_marker_idx, weights,
                     pene_thres, goal_thresh, reproj_factor, num_sequences, beam_width, num_candidates, acc, ncoll, cost, cost_terms,
                     colliding, beam_row, parent, acc_out, ncoll_out, path_cost, beam_status, goal_dist, reached,
                     GeoFieldDev{field_dist, field_origin, field_index, field_cell, field_H, field_W, num_fields}, &obs, stream);
}

extern "C" int egx_primitive_beam_select(const float* Y_gen, const float* x0, const float* x1, int x_ld, const float* joints,
                                         int joints_per_body, const float* markers_proj, const float* R0, const float* T0,
                                         const int32_t* pene_count, const float* goal, const int32_t* feet_marker_idx,
                                         const float* weights, float pene_thres, float goal_thresh, float reproj_factor,
                                         int num_sequences, int beam_width, int num_candidates, const float* acc,
                                         const int32_t* ncoll, float* cost, float* cost_terms, int32_t* colliding, int32_t* beam_row,
                                         int32_t* parent, float* acc_out, int32_t* ncoll_out, float* path_cost, int32_t* beam_status,
                                         float* goal_dist, int32_t* reached, void* stream) {
  return egx_primitive_beam_select_field(Y_gen, x0, x1, x_ld, joints, joints_per_body, markers_proj, R0, T0, pene_count, goal,
                                         feet_marker_idx, weights, pene_thres, goal_thresh, reproj_factor, num_sequences, beam_width,
                                         num_candidates, acc, ncoll, cost, cost_terms, colliding, beam_row, parent, acc_out, ncoll_out,
                                         path_cost, beam_status, goal_dist, reached, nullptr, nullptr, 0.f, 0, 0, 0, nullptr, stream);
}

extern "C" int egx_primitive_advance_beam(const float* pred_params, const float* Y_gen, const float* x0, const float* x1, int x_ld,
                                          const float* joints, int joints_per_body, const float* markers_proj, const float* delta_T,
                                          float reproj_factor, int num_sequences, int beam_width, int num_candidates,
                                          const int32_t* beam_row, const float* R0, const float* T0, float* R0_out, float* T0_out,
                                          float* out_marker_b, float* out_pelvis, float* out_R, float* out_T, float* out_params,
                                          float* out_seed_params, float* out_x0, float* out_x1, int out_x_ld, int32_t* beam_status,
                                          void* stream) {
  EGX_REQUIRE(beam_row, "null input");
  EGX_REQUIRE(R0_out && T0_out && beam_status, "null output");
  EGX_REQUIRE(beam_width >= 1 && beam_width <= EGX_MAX_BEAM, "beam_width must be in [1, EGX_MAX_BEAM]");
  EGX_REQUIRE(num_candidates >= 1 && num_candidates <= MAXC && beam_width * num_candidates <= MAXC,
              "beam_width * num_candidates must be in [1, EGX_MAX_CANDIDATES]");
  EGX_REQUIRE(R0 != R0_out && T0 != T0_out && x0 != out_x0 && x1 != out_x1,
              "a slot may read a row another slot writes: R0 / T0 and the seed frames are written to other buffers");
  return advance_entry(pred_params, Y_gen, x0, x1, x_ld, joints, joints_per_body, markers_proj, delta_T, reproj_factor, num_sequences,
                       R0, T0, out_marker_b, out_pelvis, out_R, out_T, out_seed_params, out_x0, out_x1, out_x_ld, [&](AdvanceArgs& p) {
    p.R0_out = R0_out; p.T0_out = T0_out; p.out_params = out_params; p.beam_status = beam_status;
    p.B = num_sequences * beam_width * num_candidates;
    hipLaunchKernelGGL(egx_primitive_advance_beam_kernel, dim3(num_sequences * beam_width), dim3(BLK), 0,
                       static_cast<hipStream_t>(stream), p, beam_row, beam_width, num_candidates);
  });
}

extern "C" int egx_beam_backtrack(const int32_t* parent, const int32_t* beam_row, const int32_t* beam_status, const float* goal_dist,
                                  const int32_t* reached, const float* rec_marker_b, const float* rec_pelvis, const float* rec_R,
                                  const float* rec_T, const float* rec_params, int num_primitives, int num_sequences, int beam_width,
                                  int32_t* path_slot, int32_t* choice, int32_t* status, float* out_goal_dist, int32_t* out_reached,
                                  float* out_marker_b, float* out_pelvis, float* out_R, float* out_T, float* out_params, void* stream) {
  EGX_REQUIRE(parent && beam_row && beam_status && goal_dist && reached && rec_marker_b && rec_pelvis && rec_R && rec_T && rec_params,
              "null input");
  EGX_REQUIRE(path_slot && choice && status && out_goal_dist && out_reached && out_marker_b && out_pelvis && out_R && out_T && out_params,
              "null output");
  EGX_REQUIRE(num_primitives > 0 && num_sequences > 0, "need at least one primitive and one sequence");
  EGX_REQUIRE(beam_width >= 1 && beam_width <= EGX_MAX_BEAM, "beam_width must be in [1, EGX_MAX_BEAM]");
  EGX_REQUIRE((long long)num_primitives * num_sequences <= 0x7fffffffLL, "num_primitives * num_sequences workgroups exceed the grid");
  EGX_REQUIRE(((uintptr_t)rec_marker_b & 15) == 0 && ((uintptr_t)out_marker_b & 15) == 0 && ((uintptr_t)rec_params & 15) == 0 &&
                  ((uintptr_t)out_params & 15) == 0, "the marker and parameter records must be 16-byte aligned");
  BacktrackArgs p;
  p.parent = parent; p.beam_row = beam_row; p.beam_status = beam_status; p.goal_dist = goal_dist; p.reached = reached;
  p.rec_marker_b = rec_marker_b; p.rec_pelvis = rec_pelvis; p.rec_R = rec_R; p.rec_T = rec_T; p.rec_params = rec_params;
  p.K = num_primitives; p.b = num_sequences; p.W = beam_width; p.path_slot = path_slot; p.choice = choice; p.status = status;
  p.out_goal_dist = out_goal_dist; p.out_reached = out_reached; p.out_marker_b = out_marker_b; p.out_pelvis = out_pelvis;
  p.out_R = out_R; p.out_T = out_T; p.out_params = out_params;
  hipLaunchKernelGGL(egx_beam_backtrack_kernel, dim3(num_primitives * num_sequences), dim3(BLK), 0, static_cast<hipStream_t>(stream), p);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

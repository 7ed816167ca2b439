// The cylinder pair model of the joint step of the greedy primitive search (egx_primitive_select_joint): one launch between the
// selection (egx_primitive_select, _field or _obstacles: genop.hip) and the hand-off (egx_primitive_advance_select), in which the
// people of one scene and time line - a group of up to EGX_MAX_GROUP sequences of the launch - choose again against each other's
// CURRENT choices, by the sweeps of egx_joint_sweep.h.  A person is a cylinder round the pelvis: the workgroup holds, in LDS, the
// world xy of the pelvis of every member's chosen row at the 18 predicted frames (the table); a frame clearance is that of
// egx_obstacles.h against the other columns (egx_pair_clearance).  The world xy of the visited member's rows stays in LDS too
// (37 KB): the winner's column is copied from there instead of being read and computed again.
//
// A translation unit of its own: profiles/geodesic.md records how code placed next to score_group changes the last bits of the
// selection kernels, so nothing here is compiled together with them.
#include "egx_joint_sweep.h"
#include "egx_obstacles.h"

namespace {

constexpr int TAB_LD = MAXP + 1;   // row stride of the table: lane t reads row t, 33 floats apart keeps the 18 lanes on 18 banks
constexpr int ROW_LD = NF;         // the visited member's rows: lane t writes and reads frame t of a row, consecutive floats
static_assert(EGX_OBS_FRAMES == NF, "the table holds the predicted frames of a primitive");

struct Cylinders {
  struct Row { float x, y; };
  const JointArgs& p;
  float rr;                        // body_radius + body_radius
  float (*s_x)[TAB_LD], (*s_y)[TAB_LD];   // [frame][member]: the chosen tracks
  float (*s_rx)[ROW_LD], (*s_ry)[ROW_LD]; // [row][frame]: the rows of the member being visited

  // world xy of joint 0 of body t of a row, with the nesting of field_row_cost / obstacle_group (genop.hip)
  __device__ __forceinline__ Row pelvis_xy(size_t row, int t) const {
    const float* R0 = p.R0 + row * 9;
    const float* T0 = p.T0 + row * 3;
    const float* j = p.joints + (row * NT + t) * p.jpb * 3;
    return {fmaf(R0[2], j[2], fmaf(R0[1], j[1], R0[0] * j[0])) + T0[0], fmaf(R0[5], j[2], fmaf(R0[4], j[1], R0[3] * j[0])) + T0[1]};
  }
  // c_t of the track point r against every column of the table but `skip`
  __device__ __forceinline__ float against_table(const Row& r, int P, int skip, int lane) const {
    return lane < NF ? egx_pair_clearance(r.x, r.y, P, skip, s_x[lane], s_y[lane], rr) : __builtin_inff();
  }
  __device__ __forceinline__ void prepare(const JointGroup& g) {
    for (int e = threadIdx.x; e < NF * g.P; e += JOINT_BLK) {
      const int f = e / g.P, j = e % g.P;
      const Row r = pelvis_xy((size_t)g.member[j] * p.N + g.choice[j], THIS + f);
      s_x[f][j] = r.x;
      s_y[f][j] = r.y;
    }
  }
  // no branch round a load: the lanes past 17 read frame 19 again
  __device__ __forceinline__ Row load(size_t row, int lane) const { return pelvis_xy(row, THIS + min(lane, NF - 1)); }
  __device__ __forceinline__ float clearance(const JointGroup& g, int i, int, const Row& r, int lane) const {
    return against_table(r, g.P, i, lane);
  }
  __device__ __forceinline__ void keep(int n, const Row& r, int lane) {   // for the rewrite of the table
    if (lane < NF) {
      s_rx[n][lane] = r.x;
      s_ry[n][lane] = r.y;
    }
  }
  __device__ __forceinline__ void chosen(int i, int n, int lane) {        // column i of the table follows the winner
    if (lane < NF) {
      s_x[lane][i] = s_rx[n][lane];
      s_y[lane][i] = s_ry[n][lane];
    }
  }
  __device__ __forceinline__ float final_clearance(const JointGroup& g, int i, int lane) const {
    return against_table(lane < NF ? Row{s_x[lane][i], s_y[lane][i]} : Row{0.f, 0.f}, g.P, i, lane);
  }
};

}  // namespace

__global__ __launch_bounds__(JOINT_BLK) void egx_primitive_select_joint_kernel(JointArgs p, float rr) {
  __shared__ float s_x[NF][TAB_LD], s_y[NF][TAB_LD], s_rx[MAXC][ROW_LD], s_ry[MAXC][ROW_LD];   // 37 KB
  Cylinders model{p, rr, s_x, s_y, s_rx, s_ry};
  joint_sweep(p, model);
}

extern "C" int egx_primitive_select_joint(const float* joints, int joints_per_body, const float* R0, const float* T0, const float* goal,
                                          const float* cost, const float* cost_terms, const int32_t* colliding, int num_sequences,
                                          int num_candidates, const int32_t* group_start, const int32_t* group_member, int num_groups,
                                          int sweeps, float pair_weight, float margin, float body_radius, float goal_thresh,
                                          int32_t* choice, int32_t* status, int32_t* reached, float* goal_dist, float* pair_term,
                                          float* pair_clearance, float* joint_cost, int32_t* pair_hit, int32_t* choice_trace,
                                          int32_t* changed, float* crowd_clearance, int32_t* crowd_hit, void* stream) {
  const JointArgs p{joints, R0, T0, goal, cost, cost_terms, colliding, group_start, group_member, num_sequences, num_candidates, joints_per_body,
                    num_groups, sweeps, pair_weight, margin, goal_thresh, choice, status, reached, goal_dist, pair_term, pair_clearance,
                    joint_cost, pair_hit, choice_trace, changed, crowd_clearance, crowd_hit};
  const int bad = joint_check_args(joints && R0 && T0 && goal && cost && cost_terms && colliding && group_start && group_member, p, body_radius,
                                   "body_radius");
  if (bad != EGX_OK) return bad;
  hipLaunchKernelGGL(egx_primitive_select_joint_kernel, dim3(num_groups), dim3(JOINT_BLK), 0, static_cast<hipStream_t>(stream), p,
                     body_radius + body_radius);   // doubling is exact
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

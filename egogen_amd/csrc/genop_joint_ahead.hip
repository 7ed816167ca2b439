// The look-ahead pair model of the joint step of the greedy primitive search (egx_primitive_select_joint_ahead): the cylinder model
// of genop_joint.hip plus a displacement for each member and for each row.  Everybody is predicted H further primitives ahead by
// repeating the net displacement d = p(19) - p(1) of the own primitive - a candidate row its own, another member that of its CURRENT
// choice - and a frame clearance is
//
//   c_t = min(c_{t,0}, min_{h=1..H} max(0, c_{t,h}) + h * slack),   c_{t,h} = min_{j != i} |(p_i(t) + h d_i) - (p_j(t) + h d_j)| - rr
//
// with egx_pair_clearance's roundings (egx_obstacles.h); c_{t,0} is that function itself, so H = 0 gives the bits of
// egx_primitive_select_joint.  A prediction can cost but only the present can veto (the max), and crowd_clearance / crowd_hit stay at
// h = 0: did the crowd as written overlap.  The sweeps are those of egx_joint_sweep.h; the table holds d_j of every member's current
// choice next to its 18 xy columns, `keep` / `chosen` carry a row's d with its track.
//
// A translation unit of its own, as genop_joint.hip is and for its reason.
#include "egx_joint_sweep.h"
#include "egx_obstacles.h"

namespace {

constexpr int TAB_LD = MAXP + 1;   // as genop_joint.hip: lane t reads row t, 33 floats apart keeps the 18 lanes on 18 banks
constexpr int ROW_LD = NF;
static_assert(EGX_OBS_FRAMES == NF, "the table holds the predicted frames of a primitive");

struct CylindersAhead {
  struct Row { float x, y, dx, dy; };
  const JointArgs& p;
  float rr;                        // body_radius + body_radius
  int H;                           // further primitives looked ahead
  float slack;                     // metres per primitive of look-ahead
  float (*s_x)[TAB_LD], (*s_y)[TAB_LD];   // [frame][member]: the chosen tracks
  float *s_dx, *s_dy;                     // [member]: the displacement of every member's chosen row
  float (*s_rx)[ROW_LD], (*s_ry)[ROW_LD]; // [row][frame]: the rows of the member being visited
  float *s_rdx, *s_rdy;                   // [row]: their displacements

  // world xy of joint 0 of body t of a row, with the nesting of field_row_cost / obstacle_group (genop.hip)
  __device__ __forceinline__ void pelvis_xy(size_t row, int t, float& x, float& y) const {
    const float* R0 = p.R0 + row * 9;
    const float* T0 = p.T0 + row * 3;
    const float* j = p.joints + (row * NT + t) * p.jpb * 3;
    x = fmaf(R0[2], j[2], fmaf(R0[1], j[1], R0[0] * j[0])) + T0[0];
    y = fmaf(R0[5], j[2], fmaf(R0[4], j[1], R0[3] * j[0])) + T0[1];
  }
  // d = p(19) - p(1): one rounded difference per axis
  __device__ __forceinline__ void displacement(size_t row, float& dx, float& dy) const {
    float x1, y1, x19, y19;
    pelvis_xy(row, 1, x1, y1);
    pelvis_xy(row, NT - 1, x19, y19);
    dx = egx_sub(x19, x1);
    dy = egx_sub(y19, y1);
  }
  // c_{t,h}, h >= 1: egx_pair_clearance with both people moved h displacements on, one rounded product and one rounded addition per axis each
  __device__ __forceinline__ float predicted(const Row& r, float hf, int P, int skip, int lane) const {
#pragma clang fp contract(off)
    const float x = egx_add(r.x, egx_mul(hf, r.dx)), y = egx_add(r.y, egx_mul(hf, r.dy));
    if (isnan(x) || isnan(y)) return __builtin_nanf("");
    float m = __builtin_inff();
    for (int o = 0; o < P; ++o) {
      if (o == skip) continue;
      const float ox = egx_add(s_x[lane][o], egx_mul(hf, s_dx[o])), oy = egx_add(s_y[lane][o], egx_mul(hf, s_dy[o]));
      const float ex = egx_sub(x, ox), ey = egx_sub(y, oy);
      const float d = sqrtf(egx_add(egx_mul(ex, ex), egx_mul(ey, ey)));
      m = fminf(m, egx_sub(d, rr));                // another member's NaN drops out
    }
    return m;
  }
  __device__ __forceinline__ float against_table(float x, float y, int P, int skip, int lane) const {
    return lane < NF ? egx_pair_clearance(x, y, P, skip, s_x[lane], s_y[lane], rr) : __builtin_inff();
  }
  __device__ __forceinline__ void prepare(const JointGroup& g) {
    for (int e = threadIdx.x; e < NF * g.P; e += JOINT_BLK) {
      const int f = e / g.P, j = e % g.P;
      float x, y;
      pelvis_xy((size_t)g.member[j] * p.N + g.choice[j], THIS + f, x, y);
      s_x[f][j] = x;
      s_y[f][j] = y;
    }
    if ((int)threadIdx.x < g.P) {
      float dx, dy;
      displacement((size_t)g.member[threadIdx.x] * p.N + g.choice[threadIdx.x], dx, dy);
      s_dx[threadIdx.x] = dx;
      s_dy[threadIdx.x] = dy;
    }
  }
  // no branch round a load: the lanes past 17 read frame 19 again; p(1) and p(19) are one address in every lane
  __device__ __forceinline__ Row load(size_t row, int lane) const {
    Row r;
    pelvis_xy(row, THIS + min(lane, NF - 1), r.x, r.y);
    displacement(row, r.dx, r.dy);
    return r;
  }
  __device__ __forceinline__ float clearance(const JointGroup& g, int i, int, const Row& r, int lane) const {
    if (lane >= NF) return __builtin_inff();
    float c = against_table(r.x, r.y, g.P, i, lane);
    bool bad = isnan(c);
    for (int h = 1; h <= H; ++h) {                 // H is a launch argument: the same trip count in every lane
      const float hf = (float)h;
      const float ch = predicted(r, hf, g.P, i, lane);
      bad = bad || isnan(ch);                      // before the max: fmaxf(0, NaN) is 0
      c = fminf(c, egx_add(fmaxf(0.f, ch), egx_mul(hf, slack)));
    }
    return bad ? __builtin_nanf("") : c;
  }
  __device__ __forceinline__ void keep(int n, const Row& r, int lane) {   // for the rewrite of the table
    if (lane < NF) {
      s_rx[n][lane] = r.x;
      s_ry[n][lane] = r.y;
    }
    if (lane == 0) {
      s_rdx[n] = r.dx;
      s_rdy[n] = r.dy;
    }
  }
  __device__ __forceinline__ void chosen(int i, int n, int lane) {        // column i of the table follows the winner, d with it
    if (lane < NF) {
      s_x[lane][i] = s_rx[n][lane];
      s_y[lane][i] = s_ry[n][lane];
    }
    if (lane == 0) {
      s_dx[i] = s_rdx[n];
      s_dy[i] = s_rdy[n];
    }
  }
  // h = 0 only: the crowd as written
  __device__ __forceinline__ float final_clearance(const JointGroup& g, int i, int lane) const {
    const int f = min(lane, NF - 1);
    return against_table(s_x[f][i], s_y[f][i], g.P, i, lane);
  }
};

}  // namespace

__global__ __launch_bounds__(JOINT_BLK) void egx_primitive_select_joint_ahead_kernel(JointArgs p, float rr, int H, float slack) {
  __shared__ float s_x[NF][TAB_LD], s_y[NF][TAB_LD], s_rx[MAXC][ROW_LD], s_ry[MAXC][ROW_LD];   // 37 KB
  __shared__ float s_dx[MAXP], s_dy[MAXP], s_rdx[MAXC], s_rdy[MAXC];                             // 2.3 KB
  CylindersAhead model{p, rr, H, slack, s_x, s_y, s_dx, s_dy, s_rx, s_ry, s_rdx, s_rdy};
  joint_sweep(p, model);
}

extern "C" int egx_primitive_select_joint_ahead(const float* joints, int joints_per_body, const float* R0, const float* T0, const float* goal,
                                                const float* cost, const float* cost_terms, const int32_t* colliding, int num_sequences,
                                                int num_candidates, const int32_t* group_start, const int32_t* group_member, int num_groups,
                                                int sweeps, float pair_weight, float margin, float body_radius, int lookahead, float slack,
                                                float goal_thresh, int32_t* choice, int32_t* status, int32_t* reached, float* goal_dist,
                                                float* pair_term, float* pair_clearance, float* joint_cost, int32_t* pair_hit,
                                                int32_t* choice_trace, int32_t* changed, float* crowd_clearance, int32_t* crowd_hit,
                                                void* stream) {
  const JointArgs p{joints, R0, T0, goal, cost, cost_terms, colliding, group_start, group_member, num_sequences, num_candidates, joints_per_body,
                    num_groups, sweeps, pair_weight, margin, goal_thresh, choice, status, reached, goal_dist, pair_term, pair_clearance,
                    joint_cost, pair_hit, choice_trace, changed, crowd_clearance, crowd_hit};
  const int bad = joint_check_args(joints && R0 && T0 && goal && cost && cost_terms && colliding && group_start && group_member, p, body_radius,
                                   "body_radius");
  if (bad != EGX_OK) return bad;
  EGX_REQUIRE(lookahead >= 0 && lookahead <= EGX_MAX_LOOKAHEAD, "lookahead must be in [0, EGX_MAX_LOOKAHEAD]");
  EGX_REQUIRE(slack >= 0.f && slack < __builtin_inff(), "lookahead_slack must not be negative and must be finite");
  hipLaunchKernelGGL(egx_primitive_select_joint_ahead_kernel, dim3(num_groups), dim3(JOINT_BLK), 0, static_cast<hipStream_t>(stream), p,
                     body_radius + body_radius, lookahead, slack);   // doubling is exact
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

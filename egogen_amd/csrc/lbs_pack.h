// Host-only packing of a body description (egx_body_model_host) into the images, lists and constants the LBS kernels read.
// lbs_pack.hip calls no HIP runtime function: it links into a stand-alone program (tests/lbs_pack_check.hip) that checks every
// packed byte on a machine without a GPU.  egx_body_model_create (body_model.hip) uploads an LbsPacked as it stands.
#pragma once
#include <vector>

#include "lbs.h"

// The scalars and one vector per device array of egx_body_model (lbs.h documents each layout there).
struct LbsPacked : LbsModelDims {
  std::vector<int> perm;                    // -> vorig
  std::vector<f32x4> dirs;
  std::vector<float> dirs_rm, tj_w, lmk_bary, cull_E, cull_D0;
  std::vector<unsigned short> dirs3, dirs4, skinW;
  std::vector<int> tj_off, tj_idx, skin_ks_off, pick_slot, marker_slot, extra_slot, lmk_slot, pick_tiles, sdf_tiles;
  std::vector<uint8_t> vflags;
  std::vector<PoseConsts> pc;               // one record
};

// Validates the description (EGX_ERR_ARG + egx_set_error on a null table, an id outside [0, V) in the marker, extra, landmark or
// feet table, parents that are not topologically ordered) and fills `out`.
int lbs_pack_model(const egx_body_model_host* d, LbsPacked* out);

// What the body model and the point sets (body_points.hip) both derive from a description:
// depth[j] of every joint and the largest; false when a parent of joint j > 0 lies outside [0, j) (not topologically ordered)
bool lbs_joint_depths(const int32_t* parents, int* depth /* [NJ] */, int* max_depth);
// rest joints as an affine function of betas, the joint regressor folded through the shape space in double precision:
//   J(betas) = J_regressor (v_template + shapedirs betas) = Jt + Jsd betas,   Jt [NJ*3], Jsd [NJ*3][10]
void lbs_fold_joint_regressor(const egx_body_model_host* d, float* Jt, float* Jsd);

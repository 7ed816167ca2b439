// Hand-off between two motion primitives of a chain (one workgroup per sequence, one launch, no sync).
//
// Reference: the motion-only tail of CrowdEnv.step, motion/crowd_ppo/crowd_env_2f.py:144-155 (pelvis, blended markers) and
// :238-265 (new canonical frame from the second-last body, accumulated world frame, seed parameters and seed markers in the new
// frame) without _get_feature; the frame algebra is the code the env kernels use (egx_frame.h).
#include "egx_common.h"
#include "egx_frame.h"

namespace {

constexpr int NT = 20, THIS = 2, NM = 67, MD = NM * 3, XB = EGX_XB_DIM;
constexpr int BLK = 256;
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
  float* R0;                  // [B,9] in place
  float* T0;                  // [B,3] in place
  float* out_marker_b;        // [B,20,67,3]
  float* out_pelvis;          // [B,20,3]
  float* out_R;               // [B,9]
  float* out_T;               // [B,3]
  float* out_seed;            // [B,2,93]
  float* out_x0;              // next seed frames, row stride out_x_ld
  float* out_x1;
  int* nonfinite;             // [1] or null
  float rf;
  int B, jpb, x_ld, out_x_ld;
};

__device__ __forceinline__ bool nonfin(float v) { return !isfinite(v); }

}  // namespace

__global__ __launch_bounds__(BLK) void egx_primitive_advance_kernel(AdvanceArgs p) {
  __shared__ float s_mb[THIS][MD];   // blended markers of frames 18, 19 (old frame)
  __shared__ float s_frame[12];      // R_[9], T_[3]
  __shared__ float s_seed6[THIS][6];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* J = p.joints + (size_t)b * NT * p.jpb * 3;
  const float* PP = p.pred_params + (size_t)b * NT * XB;
  bool bad = false;

  // ---- frame algebra in the last two lanes of the block (one per seed frame); the other waves start on the markers ----
  if (tid >= BLK - THIS) {
    const int f = tid - (BLK - THIS);
    const float* j18 = J + (size_t)18 * p.jpb * 3;
    float Rn[9], Tn[3], o6[6];
    canonical_frame(j18 + 0, j18 + 3, j18 + 6, Rn, Tn);
    const float delta[3] = {p.delta_T[(size_t)b * 3 + 0], p.delta_T[(size_t)b * 3 + 1], p.delta_T[(size_t)b * 3 + 2]};
    update_transl_glorot(Rn, Tn, delta, PP + (18 + f) * XB, o6);
    for (int e = 0; e < 6; ++e) { s_seed6[f][e] = o6[e]; bad |= nonfin(o6[e]); }
    if (f == 0) {
      float R0o[9], T0o[3], T0n[3], R0n[9];
      for (int e = 0; e < 9; ++e) R0o[e] = p.R0[(size_t)b * 9 + e];
      for (int e = 0; e < 3; ++e) T0o[e] = p.T0[(size_t)b * 3 + e];
      mat3_vec(R0o, Tn, T0n);
      T0n[0] += T0o[0]; T0n[1] += T0o[1]; T0n[2] += T0o[2];
      mat3_mul(R0o, Rn, R0n);
      for (int e = 0; e < 9; ++e) {
        s_frame[e] = Rn[e];
        p.out_R[(size_t)b * 9 + e] = R0o[e];
        p.R0[(size_t)b * 9 + e] = R0n[e];
        bad |= nonfin(R0n[e]);
      }
      for (int e = 0; e < 3; ++e) {
        s_frame[9 + e] = Tn[e];
        p.out_T[(size_t)b * 3 + e] = T0o[e];
        p.T0[(size_t)b * 3 + e] = T0n[e];
        bad |= nonfin(T0n[e]);
      }
    }
  }

  // ---- pelvis of the 20 bodies ----------------------------------------------------------------------------------------
  if (tid < NT * 3) {
    const float v = J[(size_t)(tid / 3) * p.jpb * 3 + tid % 3];
    p.out_pelvis[(size_t)b * NT * 3 + tid] = v;
    bad |= nonfin(v);
  }

  // ---- blended markers: projected and output as float4 across the block, predicted gathered per element ------------------
  const float rf = p.rf;
  const f32x4* proj4 = reinterpret_cast<const f32x4*>(p.markers_proj + (size_t)b * NT * MD);
  f32x4* out4 = reinterpret_cast<f32x4*>(p.out_marker_b + (size_t)b * NT * MD);
  for (int i = tid; i < NV4; i += BLK) {
    const f32x4 pr = proj4[i];
    f32x4 o;
    for (int k = 0; k < 4; ++k) {
      const int e = i * 4 + k, t = e / MD, d = e % MD;
      const float pred = (t == 0)   ? p.x0[(size_t)b * p.x_ld + d]
                         : (t == 1) ? p.x1[(size_t)b * p.x_ld + d]
                                    : p.Y_gen[((size_t)(t - THIS) * p.B + b) * MD + d];
      const float v = rf * pr[k] + (1.f - rf) * pred;
      o[k] = v;
      if (t >= NT - THIS) s_mb[t - (NT - THIS)][d] = v;
      bad |= nonfin(v);
    }
    out4[i] = o;
  }
  __syncthreads();

  // ---- next seed: markers of frames 18, 19 in (R_, T_), parameters with the new transl / glorot ---------------------------
  float Rn[9], Tn[3];
  for (int e = 0; e < 9; ++e) Rn[e] = s_frame[e];
  for (int e = 0; e < 3; ++e) Tn[e] = s_frame[9 + e];
  for (int i = tid; i < THIS * NM; i += BLK) {
    const int t = i / NM, m = i % NM;
    const float v[3] = {s_mb[t][m * 3 + 0] - Tn[0], s_mb[t][m * 3 + 1] - Tn[1], s_mb[t][m * 3 + 2] - Tn[2]};
    float ms[3];
    mat3T_vec(Rn, v, ms);
    float* st = (t == 0 ? p.out_x0 : p.out_x1) + (size_t)b * p.out_x_ld + m * 3;
    st[0] = ms[0]; st[1] = ms[1]; st[2] = ms[2];
    bad |= nonfin(ms[0]) || nonfin(ms[1]) || nonfin(ms[2]);
  }
  for (int i = tid; i < THIS * XB; i += BLK) {
    const int t = i / XB, d = i % XB;
    const float v = (d < 6) ? s_seed6[t][d] : PP[(18 + t) * XB + d];
    p.out_seed[((size_t)b * THIS + t) * XB + d] = v;
    bad |= nonfin(v);
  }
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (tid == 0 && any_bad && p.nonfinite) atomicAdd(p.nonfinite, 1);
}

extern "C" int egx_primitive_advance(const float* pred_params, const float* Y_gen, const float* x0, const float* x1, int x_ld,
                                     const float* joints, int joints_per_body, const float* markers_proj, const float* delta_T,
                                     float reproj_factor, int num_sequences, float* R0, float* T0, float* out_marker_b,
                                     float* out_pelvis, float* out_R, float* out_T, float* out_seed_params, float* out_x0,
                                     float* out_x1, int out_x_ld, int32_t* nonfinite, void* stream) {
  EGX_REQUIRE(pred_params && Y_gen && x0 && x1 && joints && markers_proj && delta_T && R0 && T0, "null input");
  EGX_REQUIRE(out_marker_b && out_pelvis && out_R && out_T && out_seed_params && out_x0 && out_x1, "null output");
  EGX_REQUIRE(num_sequences > 0 && joints_per_body >= 3, "need a non-empty batch and >= 3 joints per body");
  EGX_REQUIRE(x_ld >= MD && out_x_ld >= MD, "a seed frame holds 201 floats: the row strides cannot be smaller");
  EGX_REQUIRE(((uintptr_t)markers_proj & 15) == 0 && ((uintptr_t)out_marker_b & 15) == 0,
              "markers_proj and out_marker_b must be 16-byte aligned");
  AdvanceArgs p;
  p.pred_params = pred_params; p.Y_gen = Y_gen; p.x0 = x0; p.x1 = x1; p.joints = joints; p.markers_proj = markers_proj;
  p.delta_T = delta_T; p.R0 = R0; p.T0 = T0; p.out_marker_b = out_marker_b; p.out_pelvis = out_pelvis; p.out_R = out_R;
  p.out_T = out_T; p.out_seed = out_seed_params; p.out_x0 = out_x0; p.out_x1 = out_x1; p.nonfinite = nonfinite;
  p.rf = reproj_factor; p.B = num_sequences; p.jpb = joints_per_body; p.x_ld = x_ld; p.out_x_ld = out_x_ld;
  hipLaunchKernelGGL(egx_primitive_advance_kernel, dim3(num_sequences), dim3(BLK), 0, static_cast<hipStream_t>(stream), p);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

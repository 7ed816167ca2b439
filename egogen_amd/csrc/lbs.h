// What more than one file of the linear-blend-skinning (LBS) forward needs: the layout constants of the blend GEMM, the pose constants,
// the fix-up band of the mixed blend, the loaded model (packed on the host by lbs_pack.hip, see lbs_pack.h), the parameter block and
// per-wave state of the fused kernels, small device helpers, and the host launchers each kernel file exports.  The library is built without relocatable device code: a __global__
// function is launched, and has its attributes set, only from the file that defines it (lbs_pose.hip, lbs_fused.hip,
// lbs_fused3.hip, lbs_fix.hip, lbs_cull.hip); device code shared by several kernels is __forceinline__ here and in lbs_epilogue.h.
#pragma once
#include <mutex>

#include "egx_common.h"
#include "egx_sdf.h"

namespace {

constexpr int NJ = EGX_NUM_JOINTS;
// GEMM K axis: 10 betas + 9 rotation features of the 51 joints that can move through this API (global orient is not a
// blend feature; jaw and both eyes have no field in xb[93], their R - I is exactly 0 and their 27 columns are dropped)
constexpr int KACT = 10 + 51 * 9;      // 469 live columns
constexpr int KDIM = EGX_BLEND_K;      // 472 = 469 padded to a multiple of 8
constexpr int KSTEPS = KDIM / 2;       // 236 MFMA k-steps (32x32x2)
constexpr int KGROUPS = KSTEPS / 4;    // 59 float4 groups
static_assert(KGROUPS >= 2, "the operand ring preloads two k-groups");
// 3-term bf16 split of the blend GEMM (LBS blend mode 1): every fp32 operand x = hi + mid + lo with three bf16 terms
// (24+ significant bits, i.e. the whole fp32 mantissa); the product keeps the six partial products down to 2^-24 relative
// (hi.hi, hi.mid, mid.hi, hi.lo, lo.hi, mid.mid), accumulated in fp32 by v_mfma_f32_32x32x16_bf16 - 6 MFMAs of 32 cycles
// per 16 k instead of 8 fp32 MFMAs of 64 cycles.  K is padded to 480 = 30 steps of 16.
constexpr int KS3 = 30;
__host__ __device__ inline void egx_bf16_split3(float x, unsigned short* h) {
  h[0] = egx_bf16_rne(x);
  const float r1 = x - egx_bf16_to_f32(h[0]);   // exact
  h[1] = egx_bf16_rne(r1);
  const float r2 = r1 - egx_bf16_to_f32(h[1]);  // exact
  h[2] = egx_bf16_rne(r2);
}
// Mixed blend (LBS blend mode 3): the two k-steps that hold metre-scale or shape columns - k-step 0 (10 betas + 6 pose
// columns) and k-step 29 (pose columns, template, template residual) - keep the two-plane bf16 split (three products); the 28
// k-steps in between hold pose-corrective columns only (centimetre-scale offsets) and run as ONE v_mfma_f32_32x32x16_f16 product
// on operands rounded to fp16 (11 significant bits: 2^-12 per operand; fp16's range covers both the bases, |x| < 1, and the
// features R - I in [-2, 2]).  Against float64 that moves a vertex by ~4 um rms / ~22 um worst case on the synthetic body
// (offsets 1.3 cm rms, 7 cm max) - 2e-5 of a metre-scale coordinate, a fifth of north_star's 1e-4 - for 204 instead of 540
// MFMAs per wave and item and a third of the operand bytes.  Operand images are sequences of 1 KiB PIECES:
//   bases    [vt][96 pieces][64 lanes] 8 x 16 bit: k-step 0 (plane, coord) 0..5 | k-steps 1..28 coord 6..89 | k-step 29 (plane, coord) 90..95
//   features [bt][32 pieces][64 lanes]            : k-step 0 planes 0, 1         | k-steps 1..28 2..29        | k-step 29 planes 30, 31
constexpr int M4_BASE_PIECES = 96, M4_FEAT_PIECES = 32;
constexpr int M4_FKS = 4;                       // fp16 k-steps per stage (7 stages) between the two precise stages
__host__ __device__ inline int egx_m4_feat_piece(int s, int pl) { return s == 0 ? pl : (s <= 28 ? s + 1 : 30 + pl); }
__host__ __device__ inline int egx_m4_base_piece(int s, int pl, int c) { return s == 0 ? pl * 3 + c : (s <= 28 ? 6 + (s - 1) * 3 + c : 90 + pl * 3 + c); }
__host__ __device__ inline unsigned short egx_f16_rne(float x) {
  const _Float16 h = (_Float16)x;
  unsigned short u;
  __builtin_memcpy(&u, &h, 2);
  return u;
}
__host__ __device__ inline int egx_compact_joint(int j) { return (j - 1) - (j > 24 ? 3 : 0); }  // j in 1..54, j != 22..24
__host__ __device__ inline int egx_expand_joint(int jc) { return jc + 1 + (jc >= 21 ? 3 : 0); }  // its inverse: jc in 0..50
constexpr int NLMK = 51, NEXTRA = 21;  // landmarks (three corners each) and vertex joints behind the 55 kinematic joints

}  // namespace

// (external linkage: the type is part of the pose kernel's signature)
struct PoseConsts {
  int parents[NJ];
  int depth[NJ];
  int max_depth;
  float J_template[NJ * 3];
  float J_shapedirs[NJ * 3 * 10];
  float hand_comps[2 * 12 * 45];
  float hand_mean[2 * 45];
  float fix_c[NJ];   // per joint: largest |pose-corrective base column| (3-vector norm) over its 9 columns and all vertices
  float fix_d[NJ];   // per joint: largest |fp16(column) - column| (3-vector norm) over its columns of the fp16 k-steps and all vertices
  float fix_pf;      // largest Frobenius norm of one vertex's pose-corrective block (459 columns x 3)
  float fix_dpf;     // largest Frobenius norm of one vertex's fp16 rounding errors of the columns of the fp16 k-steps
  float shape_c[10]; // per shape component: largest |shapedirs column| (3-vector norm) over all vertices
  float vt_max;      // largest |v_template|
  float w_abs_max;   // largest sum_j |W[v, j]| over the vertices (1 for convex skinning weights)
};

namespace {

// Fix-up of the mixed blend (mode 3).  The count-only tiles evaluate the pose-corrective columns as ONE fp16 product, and one vertex
// that lies close to the scene surface may then be counted differently from the reference's fp32 evaluation
// (crowd_env_2f.py:169-177).  So the cheap evaluation only CLASSIFIES: a vertex whose interpolated SDF value is further from zero
// than the value change its position error can cause keeps the cheap decision; the ones inside that band are re-evaluated in fp32
// (vertex-major fp32 bases, fp32 skinning: lbs_fix_process / egx_lbs_fix_kernel) and counted from that.  The band is a HARD bound
// of the position error of the cheap evaluation, whatever the rounding pattern (pose kernel, per body, u = 2^-11):
//   fp16 k-steps (columns k = 16..463, set H): features F_k and bases P_k rounded to fp16, products exact in the fp32 accumulator:
//     f~ p~ - F P = dF_k P_k + f~_k dP_k  EXACTLY, with dF = f~ - F computed in the pose kernel and dP = p~ - P known at load, so
//     |error| <= min( |dF_H|_2 PF + |f~_H|_2 DPF ,  sum_j (sum_{e in H} |dF_je|) C_j + (sum_{e in H} |f~_je|) D_j )
//     (Cauchy-Schwarz over the columns, or the triangle inequality per joint: PF, DPF, C_j, D_j = fix_pf, fix_dpf, fix_c, fix_d).
//     Since dF and dP are the actual rounding errors, fp16 subnormals (features of near-identity rotations, small base entries)
//     are covered as they are; for normal numbers the second form is at most (2u + u^2) sum_j |R_j - I|_1 C_j.
//   two-plane bf16 columns (betas and the 11 pose columns of k-steps 0 and 29): hi.hi + hi.mid + mid.hi, each operand's hi + mid
//     off by <= 2^-18 relative, the dropped mid.mid <= 2^-18 (1 + 2^-8)^2: <= LBS_TWO_PLANE_ERR |f| |b| per column.  The template
//     column (its third term rides on column 470) is off by < 2^-36 |v_template|.
//   fp32 accumulation, one rounding of <= 2^-24 |partial sum| per product added: the first LBS_ACC_ADDS_OFFSETS additions sum
//     shape and pose offsets only (|partial| <= O = sum_k |beta_k| S_k + min(|F|_2 PF, sum_j |F_j|_1 C_j)), the last
//     LBS_ACC_ADDS_LAST (k-step 29: three MFMAs of 16 products) also the template (|partial| <= |v| <= VB = vt_max + O).
//   skinning: the blend error reaches the posed vertex through sum_j W[v, j] R_j - times at most w_abs_max.
// The result is scaled by LBS_FIX_MARGIN for the fp32 evaluation of the bound itself; LBS_FIX_SLACK_M allows for the fp32 round-off
// both evaluations have apart from the blend (rotations, joint transforms, world / voxel map, interpolation): it is what the test
// band of 2e-5 m allows against float64, not a worst case.  tests/lbs_mode3.py mirrors this formula and builds a body for which a
// statistical band (ten standard deviations of independent roundings) is off by a factor of three.
constexpr float LBS_FIX_SLACK_M = 3e-6f;
constexpr float LBS_TWO_PLANE_ERR = 1.2e-5f;        // >= 3.02 x 2^-18
constexpr float LBS_ACC_ADDS_OFFSETS = 496.f;       // k-step 0 (3 x 16) + k-steps 1..28 (28 x 16)
constexpr float LBS_ACC_ADDS_LAST = 48.f;           // k-step 29 (3 x 16)
constexpr float LBS_FIX_MARGIN = 1.001f;
// Matrix-pipe skinning of the count-only tiles (lbs_epilogue_cell): weights and transforms as two bf16 planes, products hi.hi + hi.mid +
// mid.hi.  Each operand is off by <= 2^-18 relative and the dropped mid.mid term is <= 2^-18, so a coordinate moves by at most
// 3.02 x 2^-18 sum_j |W[v, j]| (|v| + |t_j|) and the position by sqrt(3) times that <= 2.0e-5 w_abs_max (VB + max_j |t_j|): the hard
// bound, with VB the body's bound of |v_posed| above.
constexpr float LBS_SKIN_ERR = 2.0e-5f;
// The fix-up queue is LBS_FIX_NQ sub-queues, a workgroup appends to sub-queue blockIdx % NQ: one counter for the whole launch made
// every append (and, in the first version, every processed vertex) an atomic on ONE address - ~12 ns each at the L2, 190 us for
// 16 000 vertices.  Counters sit 128 bytes apart: fix_stats[LBS_FIX_CNT0 + 32 q]; fix_stats[0] counts the vertices re-evaluated
// inside the fused kernel (a full sub-queue).
constexpr int LBS_FIX_NQ = 64;
constexpr int LBS_FIX_CNT0 = 32;
constexpr int LBS_FIX_STATS_INTS = LBS_FIX_CNT0 + 32 * LBS_FIX_NQ;
constexpr int LBS_FIXQ_CAP = 1 << 12;   // entries per sub-queue: 64 x 4096 x 8 bytes = 2 MB of workspace, 25 vertices per body at 10 240 bodies

}  // namespace

// Skinning of the count-only tiles of the mixed blend on the matrix pipe (see lbs_epilogue_cell): T = W x A', W = the tile's skinning
// weights [32 vertices x the joints of the tile's list], A' = the bodies' joint transforms premultiplied by the agent's
// canonical-frame -> SDF-cell map, both as two bf16 planes.  One v_mfma_f32_32x32x16_bf16 k-step covers EIGHT joints of the list
// with both planes of A' folded into K: lane half 0 holds (W_hi | A'_hi), lane half 1 (W_hi | A'_mid), so one MFMA yields
// W_hi A'_hi + W_hi A'_mid; a second one with (W_mid | 0) on the same A' registers adds W_mid A'_hi.
//   skinB  [bt][joint][plane][n] 8 x bf16 = entries (a, c) of rows a = 0, 1, then [bt][joint][plane][n] 4 x bf16 = row a = 2
//   skinW  [ks_off[vt] + ks][operand 0 | 1][64 lanes] 8 x bf16, lane (h, row): operand 0 = W_hi[row][list[8 ks + e]] in both halves,
//          operand 1 = W_mid in half 0, zero in half 1
constexpr int SKIN_BT_A = NJ * 2 * 32;            // 16-byte records of rows a = 0, 1 per 32-body tile
constexpr int SKIN_BT_BYTES = NJ * 2 * 32 * 24;   // both parts

// the scalars of a loaded model: the packing (lbs_pack.hip) fills them, egx_body_model_create copies the block as it is
struct LbsModelDims {
  int V = 0, NVT = 0, NW = 0, M = 0, NP = 0;
  int n_pick_tiles = 0, n_sdf_tiles = 0;           // entries of pick_tiles / sdf_tiles
  int verts_pick_tiles = 0, verts_sdf_tiles = 0;   // real vertices inside the two tile lists (work accounting)
  int cull_ok = 0;             // skinning weights are a convex combination (>= 0, rows sum to 1) and the bound is tight: items are culled
  int sdf_lead_picks = 0;      // sdf_tiles starts with pick_tiles (in the same order)
  float rest_pelvis[3] = {0.f, 0.f, 0.f};   // root joint of the mean shape (host copy)
  float cull_ref_margin = 0.f;              // blend-shape margin of the median tile at the reference pose (metres)
};

struct egx_body_model : LbsModelDims {
  float* dirs_rm = nullptr;    // [NVT*32 rows][3 coords][KDIM] fp32, vertex-major: what the fp32 re-evaluation of single vertices reads (lbs_fix_one)
  bf16x8* skinW = nullptr;     // matrix-pipe skinning weights (see SKIN_BT_BYTES)
  int* skin_ks_off = nullptr;  // [NVT+1] k-steps (8 joints of the tile's list each) before tile vt
  f32x4* dirs = nullptr;       // [NVT][59][3][64] float4 (fp32 blend)
  bf16x8* dirs3 = nullptr;     // [NVT][30 k-steps][3 planes][3 coords][64 lanes] 8 x bf16 (bf16x3 blend)
  bf16x8* dirs4 = nullptr;     // [NVT][96 pieces][64 lanes] 8 x 16 bit (mixed blend, mode 3: see M4_BASE_PIECES)
  int* tj_off = nullptr;       // [NVT+1] offsets into the per-tile joint lists
  int* tj_idx = nullptr;       // [tj_off[NVT]] joints with a non-zero skinning weight on some vertex of the tile
  float* tj_w = nullptr;       // [tj_off[NVT]][32] dense weights of the tile's 32 vertices for that joint
  int* pick_slot = nullptr;    // [NVT*32], -1 = not picked
  int* pick_tiles = nullptr;   // [n_pick_tiles] vertex tiles that hold a picked vertex (all a markers-and-joints-only call needs)
  int* sdf_tiles = nullptr;    // [n_sdf_tiles] tiles that hold a picked vertex or a vertex of the penetration count (non-feet)
  uint8_t* vflags = nullptr;   // [NVT*32] bit0 feet, bit1 valid
  int* vorig = nullptr;        // [NVT*32] original vertex id of every (sorted) row, -1 = padding
  PoseConsts* pc = nullptr;
  int* marker_slot = nullptr;  // [M]
  int* extra_slot = nullptr;   // [21]
  int* lmk_slot = nullptr;     // [153]
  float* lmk_bary = nullptr;   // [153]
  // free-space culling of SDF work items (see egx_lbs_cull_kernel): per-tile bounds of how far a posed vertex can be from the
  // posed joints it is bound to
  float* cull_E = nullptr;     // [NVT][64]: [0,10) shape terms, [10,61) pose terms per movable joint (compact order), rest 0
  float* cull_D0 = nullptr;    // [tj_off[NVT]]: rest distance bound per (tile, joint of its list)
};

// Rotation matrix of joint j of one body from its parameter row x[93] (transl 3 | global orient 3 | body pose 63 | hand PCA 12 + 12;
// jaw and eyes - joints 22..24 - have no field: identity): axis-angle -> smplx batch_rodrigues (angle = ||a + 1e-8||).
__device__ __forceinline__ void lbs_joint_rotation(const PoseConsts* __restrict__ pc, const float* __restrict__ x, int j, float (&R)[9]) {
  float a[3] = {0.f, 0.f, 0.f};
  if (j == 0) {
    a[0] = x[3]; a[1] = x[4]; a[2] = x[5];
  } else if (j <= 21) {
    a[0] = x[6 + 3 * (j - 1)]; a[1] = x[7 + 3 * (j - 1)]; a[2] = x[8 + 3 * (j - 1)];
  } else if (j >= 25) {
    const int side = (j >= 40) ? 1 : 0;
    const int o = 3 * (j - (side ? 40 : 25));
    const float* comps = pc->hand_comps + side * 12 * 45;
    const float* pca = x + 69 + side * 12;
    for (int c = 0; c < 3; ++c) {
      float s = 0.f;
      for (int k = 0; k < 12; ++k) s += pca[k] * comps[k * 45 + o + c];
      a[c] = s + pc->hand_mean[side * 45 + o + c];
    }
  }
  const float ex = a[0] + 1e-8f, ey = a[1] + 1e-8f, ez = a[2] + 1e-8f;
  const float angle = sqrtf(ex * ex + ey * ey + ez * ez);
  const float rx = a[0] / angle, ry = a[1] / angle, rz = a[2] / angle;
  const float sn = sinf(angle), cs = 1.f - cosf(angle);
  R[0] = 1.f + cs * (-(ry * ry + rz * rz)); R[1] = -sn * rz + cs * (rx * ry);     R[2] = sn * ry + cs * (rx * rz);
  R[3] = sn * rz + cs * (rx * ry);          R[4] = 1.f + cs * (-(rx * rx + rz * rz)); R[5] = -sn * rx + cs * (ry * rz);
  R[6] = -sn * ry + cs * (rx * rz);         R[7] = sn * rx + cs * (ry * rz);      R[8] = 1.f + cs * (-(rx * rx + ry * ry));
}

// Parameter block of the fused blend GEMM + skinning + (SDF count) + (vertex picks) + (vertex write) kernels and of the fix-up kernel
struct LbsParams {
  const f32x4* dirs;
  const int* tj_off;
  const int* tj_idx;
  const float* tj_w;
  const int* pick_slot;
  const int* tiles;    // vertex tiles to compute (null = all NVT); n_tiles of them
  int n_tiles;
  const uint8_t* vflags;
  const int* vorig;    // original vertex id per sorted row
  const bf16x8* dirs3; // bf16x3 bases (blend mode 1)
  const bf16x8* feat3; // [bt][30][3 planes][64] 8 x bf16
  const bf16x8* dirs4; // mixed-blend bases (mode 3), [vt][96 pieces][64]
  const bf16x8* feat4; // mixed-blend features, [bt][32 pieces][64]
  int n_precise;       // mode 3: the first n_precise entries of `tiles` (the tiles that hold picked vertices) use the two-plane split
  const f32x4* feat;   // [bt][59][64] float4
  const f32x4* A4;     // [bt][55][3][32] float4
  const float* xb;     // transl = xb[b*93 + 0..2]
  int B, V, NVT, NW, NP, fpa;
  int nbg;             // body groups (256 bodies each)
  int bg_block;        // body groups per L2 block of the item order (bf16x3 kernel)
  int dbg;             // development ablations (EGX_LBS_DBG): 1 = skip the epilogue, 2 = skip the MFMA loop
  float* verts;        // [B][V][3] or null
  float* picked;       // [B][NP][3] or null
  SdfDev sdf;
  const float* R0;     // [A][9] or null
  const float* T0;     // [A][3] or null
  int* pene;           // [B]
  // culled launches (egx_lbs_cull_kernel): operand slot -> body order, and per-XCD lists of the active work items
  const int* agent_of_slot;   // [B / fpa] or null (identity)
  const int* items;           // [8][items_stride] codes tile_index * nbg + body_group, or null (walk every item)
  const int* item_counts;     // [8]
  int items_stride;
  // fix-up of the mixed blend (see LBS_FIX_SLACK_M)
  const float* fix_e;         // [Bp] per slot: position error bound (metres)
  const float* sdf_aux;       // aux floats of the SDF's bracket table (egx_sdf_aux_offset): [0..2] largest sample step per axis
  int* fix_stats;             // [0] vertices re-evaluated inside the fused kernel, [LBS_FIX_CNT0 + 32 q] fill of sub-queue q (cleared by the pose kernel)
  const float* dirs_rm;       // vertex-major fp32 bases (fix-up)
  const PoseConsts* pc;       // pose constants (fix-up: the body's rotation features are recomputed from xb)
  const float* betas;         // [A][10]
  int2* fixq;                 // fix-up queue: LBS_FIX_NQ sub-queues of fixq_cap entries (vertex tile * 32 + row, operand slot)
  int fixq_cap;
  // matrix-pipe skinning of the count-only tiles (lbs_epilogue_cell)
  const bf16x8* skinW;        // [k-step][2][64] (see SKIN_BT_BYTES)
  const int* skin_ks_off;     // [NVT+1]
  const bf16x8* skinB;        // [bt] SKIN_BT_BYTES each
  const f32x4* cinit;         // [Bp]
  // scene sets (egx_lbs_forward_scenes, the MS instantiations): the scene of body b is agent_scene[b / fpa], an index into `scenes`;
  // `sdf` then holds only the grid dimensions the scenes share
  const SdfSceneDev* scenes;  // [n_scenes] or null (one scene: sdf, sdf_aux)
  const int* agent_scene;     // [A]
  int n_scenes;
};

// Scene of agent `ag` of a set launch: false when agent_scene names no scene of the set (the pose kernel gave that body the count -1;
// the epilogues then count nothing for it); `s` is clamped into the set either way, so every read stays inside the table.
__device__ __forceinline__ bool lbs_scene_of(const LbsParams& p, int ag, int& s) {
  const int v = p.agent_scene[ag];
  const bool ok = v >= 0 && v < p.n_scenes;
  s = ok ? v : 0;
  return ok;
}

// Operand slot of body column n of 32-body tile bt: the slot itself, or, for the dead columns of the last tile (B % 32 != 0) and of a
// tile past it, the last live slot - whose feature, transform and skinning records the pose kernel wrote in this call.  The results
// of those columns are discarded; reading written records keeps them finite, whatever the workspace held before.
__device__ __forceinline__ int lbs_live_slot(int bt, int n, int B) { return min(bt * 32 + n, B - 1); }

// one v_fma_f32, opaque to the SLP vectoriser (which would pair adjacent rows into v_pk_fma_f32 again)
__device__ __forceinline__ float lbs_fma(float a, float b, float c) {
  float d;
  asm("v_fma_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}

// Per-wave state of the fused kernels: lane coordinates and the wave's private LDS regions (metadata of the current
// vertex tile, penetration counters, queue of undecided SDF points / vertex transpose buffer).
struct LbsWave {
  int lane, n, half;
  float* s_W;          // [jj][row] dense skinning weights of the tile's joint list
  int* s_jl;           // [jj] joint ids
  int* s_slot;         // [row] pick slot or -1
  unsigned* s_masks;   // [0] rows with a pick slot, [1] rows in the SDF count
  int* s_cnt;          // [q*32 + n] penetration count of this item's 64 bodies
  unsigned* s_fixmap;  // [q*32 + n] bit r = vertex row r of that body awaits the fp32 re-evaluation (mixed blend only)
  float* s_thr;        // [q*32 + n] |SDF value| below which the cheap evaluation does not decide (mixed blend only)
  float* lds;          // vertex transpose buffer (vertex-writing variants)
  f32x4* s_queue;      // undecided SDF points (voxel x, y, z, counter slot)
  int qn;              // queued points (wave-uniform)
#ifdef EGX_LBS_TIMING
  unsigned long long et[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // per-wave cycle totals, written out once when the kernel ends
#endif
};
constexpr int LBS_NB = 2;  // 32-body MFMA column tiles per wave

#ifdef EGX_LBS_TIMING
// development build only (make CXXFLAGS+=-DEGX_LBS_TIMING): cycle totals of the phases of the bf16x3 stage loop
#define LBS_T(i, v) do { tacc[i] += (unsigned long long)(v); } while (0)
#define LBS_NOW() __builtin_readcyclecounter()
#else
#define LBS_T(i, v) do { } while (0)
#define LBS_NOW() 0ull
#endif

__device__ __forceinline__ float lbs_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ------------------------------------------------------------------------------------------------
// host side: what the launcher (body_model.hip) calls, one or two functions per kernel file
// ------------------------------------------------------------------------------------------------
// Per-device launch facts of a file of persistent kernels: the CU count, read on the file's first launch on a device - which is also
// when `raise_caps` raises the dynamic-LDS caps of the file's instantiations.  That launch must not be part of a graph capture;
// the first egx_lbs_forward of a process never is.
constexpr int kMaxDevices = 64;
struct LbsDeviceInfo {
  std::mutex mu;
  int num_cu = 0;
};
template <typename Raise>
inline int lbs_device_cus(LbsDeviceInfo (&devs)[kMaxDevices], Raise&& raise_caps, int* num_cu) {
  int dev = 0;
  EGX_HIP_CHECK(hipGetDevice(&dev));
  EGX_REQUIRE(dev >= 0 && dev < kMaxDevices, "device ordinal out of range");
  LbsDeviceInfo& di = devs[dev];
  std::lock_guard<std::mutex> lk(di.mu);
  if (di.num_cu == 0) {
    hipDeviceProp_t prop;
    EGX_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    if (int rc = raise_caps()) return rc;
    di.num_cu = prop.multiProcessorCount;
  }
  *num_cu = di.num_cu;
  return EGX_OK;
}

// lbs_pose.hip: egx_pose_chain_kernel<ms> on ceil(B / 4) blocks.  The members are the kernel's arguments (documented there), which it
// takes one by one; null / zero = that output is not wanted.
struct LbsPoseArgs {
  const PoseConsts* pc = nullptr;
  const float *xb = nullptr, *betas = nullptr, *R0 = nullptr, *T0 = nullptr;
  int B = 0, fpa = 0, joints_ld = 0, Bp = 0;
  float *feat = nullptr, *out_joints = nullptr, *fvec = nullptr, *jpos = nullptr, *fix_e = nullptr;
  unsigned short *feat3 = nullptr, *feat4 = nullptr, *skinB = nullptr;
  f32x4 *A4 = nullptr, *cinit = nullptr;
  int *zero_counts = nullptr, *fix_stats = nullptr;
  const int* agent_of_slot = nullptr;
  float template_lo_feat = 0.f;
  SdfDev sdf = {};
  const SdfSceneDev* scenes = nullptr;   // scene sets: the table, the agents' indices into it, its size
  const int* agent_scene = nullptr;
  int n_scenes = 0;
};
void lbs_launch_pose(bool ms, hipStream_t stream, const LbsPoseArgs& a);
// lbs_cull.hip: egx_lbs_agent_order_kernel in front of the pose kernel, egx_lbs_cull_kernel + egx_lbs_compact_kernel behind it
void lbs_launch_cull_order(const egx_body_model* m, const float* xb, const float* R0, const float* T0, const SdfDev& sd, const float* mips,
                           int B, int fpa, int nbg_all, int* order, int* flags, int* counts, hipStream_t stream);
void lbs_launch_cull_items(const egx_body_model* m, const float* fvec, const float* jpos, int Bp, const int* order, int B, int fpa,
                           int nbg_all, const float* R0, const float* T0, const SdfDev& sd, const float* mips, int* flags, int* items,
                           int items_stride, int* counts, hipStream_t stream);
// lbs_fused.hip: egx_lbs_fused_kernel<p.verts != null, do_sdf, ms> (blend mode 0 and every vertex-writing call)
int lbs_launch_fused(const LbsParams& p, bool do_sdf, bool ms, hipStream_t stream);
// lbs_fused3.hip: egx_lbs_fused3_kernel of blend mode 1, 2 or 3; forced_tile = the wave-tile switch (0 = by launch size)
int lbs_launch_fused3(const LbsParams& p, int mode, bool do_sdf, bool ms, int forced_tile, hipStream_t stream);
// lbs_fix.hip: egx_lbs_fix_kernel<ms> on the queue the fused3 kernel filled
void lbs_launch_fix(const LbsParams& p, bool ms, hipStream_t stream);

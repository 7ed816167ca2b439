// Differentiable SMPL-X points: the rows of the body model at a list of vertex ids plus the 55 kinematic-tree joints, forward and
// reverse mode (include/egogen_hip.h: egx_point_set_*, egx_points_forward, egx_points_backward).
//
// The function is `bm(return_verts=True, **bparam).vertices[:, vids]` / `.joints[:, :55]` (models/baseops.py:382) - the body the
// regressor's loss differentiates through (models_GAMMA_primitive.py:617-633) - with the arithmetic of smplx 0.1.28
// lbs.lbs / batch_rodrigues / batch_rigid_transform [upstream]:
//     x_p = T_p^R v_posed_p + T_p^t + transl,   T_p = sum_j w_pj A_j,   A_j = [GR_j | Gt_j - GR_j J_j]
//     G_j = G_parent [R_j | J_j - J_parent],    joints55_j = Gt_j + transl
//     v_posed = v_template + S beta + feat P,   feat = vec(R_1..54 - I),   J = J_template + J_shapedirs beta
//
// One workgroup of 256 threads per body, everything about the body in LDS, fp32 FMA.  The backward kernel recomputes the forward
// quantities from xb / betas (nothing is saved, no workspace) and writes every output element from one thread with an ordinary
// store: sums over points are wave-strided partial sums, a shuffle tree and a fixed-order sum over the four waves, sums over the
// children of a joint follow the child list in ascending order - two calls on the same inputs give the same bits.
#include <algorithm>
#include <utility>
#include <vector>

#include "lbs_pack.h"   // NJ; the joint depths and the folded joint regressor shared with the body model

namespace {

constexpr int NFEAT = 486;       // 54 x 9 pose features
constexpr int NPOSE = 165;       // 55 x 3 axis-angle entries
constexpr int PTS_MAX = 1024;
constexpr int PTS_THREADS = 256;

// device tree table (int32): parents | joints ordered by depth | first entry of each depth level | first child | children
constexpr int T_PAR = 0, T_ORD = 55, T_LOFF = 110, T_COFF = 166, T_CIDX = 222, T_SIZE = 277;

struct PtsDev {
  int P, P3, num_levels;
  const float* vt;    // [3P]        template rows
  const float* sd;    // [3P][10]    shape directions
  const float* pd;    // [486][3P]   pose directions, point index fastest
  const float* wT;    // [55][P]     skinning weights, point index fastest
  const float* Jt;    // [165]       J_regressor v_template          (folded in float64)
  const float* Jsd;   // [165][10]   J_regressor shapedirs           (folded in float64)
  const float* hc;    // [24][45]    hand PCA components, left rows 0..11, right rows 12..23
  const float* hm;    // [90]        hand means, left | right
  const int* tree;    // [T_SIZE]
};

// LDS carve (floats).  Forward part, then the backward's.
constexpr int L_POSE = 0, L_R = 168, L_J = 664, L_G = 832, L_A = 1492, L_FEAT = 2152, L_BETA = 2640, L_TREE = 2652, L_FWD = 2932;
// (the backward part sits between the forward part and the per-point arrays; dG is held in double, hence the even offsets)
constexpr int L_DA = 0, L_DG = 660, L_DREL = 1980, L_DJ = 2148, L_DFEAT = 2316, L_DPOSE = 2804, L_GJ = 2972, L_RED = 3140,
              L_GSUM = 3204, L_BWD = 3220;
static_assert(L_TREE + T_SIZE <= L_FWD, "tree table");
static_assert(L_FWD % 2 == 0 && L_DG % 2 == 0 && L_BWD % 2 == 0, "8-byte alignment of the double region");

size_t pts_lds_bytes(int P, bool bwd) { return (size_t)(L_FWD + 3 * P + (bwd ? L_BWD + 6 * P : 0)) * sizeof(float); }

// smplx lbs.batch_rodrigues, operation by operation: angle = |r + 1e-8|, d = r / angle, R = I + sin K + (1 - cos) K K.
__device__ __forceinline__ void pts_rodrigues(const float* r, float* R) {
  const float px = r[0] + 1e-8f, py = r[1] + 1e-8f, pz = r[2] + 1e-8f;
  const float angle = sqrtf(px * px + py * py + pz * pz);
  const float dx = r[0] / angle, dy = r[1] / angle, dz = r[2] / angle;
  const float s = sinf(angle), oc = 1.f - cosf(angle);
  R[0] = 1.f + oc * -(dy * dy + dz * dz); R[1] = s * -dz + oc * (dx * dy);        R[2] = s * dy + oc * (dx * dz);
  R[3] = s * dz + oc * (dx * dy);         R[4] = 1.f + oc * -(dx * dx + dz * dz); R[5] = s * -dx + oc * (dy * dz);
  R[6] = s * -dy + oc * (dx * dz);        R[7] = s * dx + oc * (dy * dz);         R[8] = 1.f + oc * -(dx * dx + dy * dy);
}

// Reverse mode of the function above, through the same operations (g = dL/dR row-major -> dL/dr).  At r = 0 the direction is 0,
// sin(angle) / angle is 1 and the result is the antisymmetric part of g, the finite value autograd gives.
//
// The joint-level part of the backward (this function, the sums up the tree and dR) runs in double: it is 55 threads' work, and
// the gradients of the root accumulate every joint's, which in fp32 costs a good part of the few ulps the tests allow.
__device__ __forceinline__ void pts_rodrigues_bwd(const float* rf, const double* g, float* dr) {
  const double r[3] = {(double)rf[0], (double)rf[1], (double)rf[2]};
  const double px = r[0] + 1e-8, py = r[1] + 1e-8, pz = r[2] + 1e-8;
  const double angle = sqrt(px * px + py * py + pz * pz);
  const double inv = 1.0 / angle;
  const double dx = r[0] / angle, dy = r[1] / angle, dz = r[2] / angle;
  const double s = sin(angle), c = cos(angle), oc = 1.0 - c;
  const double s01 = g[1] + g[3], s02 = g[2] + g[6], s12 = g[5] + g[7];
  const double dLds = dx * (g[7] - g[5]) + dy * (g[2] - g[6]) + dz * (g[3] - g[1]);
  const double dLdoc = -(g[0] * (dy * dy + dz * dz) + g[4] * (dx * dx + dz * dz) + g[8] * (dx * dx + dy * dy)) + s01 * (dx * dy) +
                      s02 * (dx * dz) + s12 * (dy * dz);
  const double ddx = s * (g[7] - g[5]) + oc * (s01 * dy + s02 * dz - 2.0 * dx * (g[4] + g[8]));
  const double ddy = s * (g[2] - g[6]) + oc * (s01 * dx + s12 * dz - 2.0 * dy * (g[0] + g[8]));
  const double ddz = s * (g[3] - g[1]) + oc * (s02 * dx + s12 * dy - 2.0 * dz * (g[0] + g[4]));
  const double dangle = (dLds * c + dLdoc * s) - (ddx * dx + ddy * dy + ddz * dz) * inv;   // sin, 1 - cos; d = r / angle
  dr[0] = (float)(ddx * inv + dangle * (px * inv));
  dr[1] = (float)(ddy * inv + dangle * (py * inv));
  dr[2] = (float)(ddz * inv + dangle * (pz * inv));
}

// Pose, rotations, rest joints, chain and posed points of one body into LDS (ends with a barrier).
__device__ __forceinline__ void pts_recompute(const PtsDev& S, float* L, float* vposed, const float* __restrict__ xb,
                                              const float* __restrict__ betas) {
  const int tid = threadIdx.x;
  float *pose = L + L_POSE, *R = L + L_R, *J = L + L_J, *G = L + L_G, *A = L + L_A, *feat = L + L_FEAT, *beta = L + L_BETA;
  int* tree = reinterpret_cast<int*>(L + L_TREE);
  for (int i = tid; i < T_SIZE; i += PTS_THREADS) tree[i] = S.tree[i];
  if (tid < 10) beta[tid] = betas[tid];
  if (tid < NPOSE) {
    float v = 0.f;                                   // jaw and eyes stay at rest
    if (tid < 66) {
      v = xb[3 + tid];
    } else if (tid >= 75) {
      const int m = tid - 75, side = m >= 45, mm = m - 45 * side;
      const float* c = S.hc + side * 12 * 45 + mm;
      const float* x = xb + 69 + 12 * side;
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < 12; ++k) a = fmaf(x[k], c[k * 45], a);
      v = a + S.hm[m];
    }
    pose[tid] = v;
  }
  __syncthreads();
  if (tid < NJ) {
    pts_rodrigues(pose + 3 * tid, R + 9 * tid);
  } else if (tid >= 64 && tid < 64 + NPOSE) {
    const int i = tid - 64;
    float a = 0.f;
#pragma unroll
    for (int l = 0; l < 10; ++l) a = fmaf(S.Jsd[i * 10 + l], beta[l], a);
    J[i] = S.Jt[i] + a;
  }
  __syncthreads();
  for (int k = tid; k < NFEAT; k += PTS_THREADS) {
    const int e = k % 9;
    feat[k] = R[9 + k] - ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f);
  }
  // world transforms, one depth level per step: G_j = G_parent [R_j | J_j - J_parent];  A_j = [GR_j | Gt_j - GR_j J_j]
  for (int lev = 0; lev < S.num_levels; ++lev) {
    for (int idx = tree[T_LOFF + lev] + tid; idx < tree[T_LOFF + lev + 1]; idx += PTS_THREADS) {
      const int j = tree[T_ORD + idx];
      float g[12];
      if (j == 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) g[e] = R[e];
        g[9] = J[0]; g[10] = J[1]; g[11] = J[2];
      } else {
        const int p = tree[T_PAR + j];
        const float* Gp = G + 12 * p;
        const float* Rj = R + 9 * j;
        const float rel[3] = {J[3 * j] - J[3 * p], J[3 * j + 1] - J[3 * p + 1], J[3 * j + 2] - J[3 * p + 2]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int c = 0; c < 3; ++c) g[3 * r + c] = Gp[3 * r] * Rj[c] + Gp[3 * r + 1] * Rj[3 + c] + Gp[3 * r + 2] * Rj[6 + c];
          g[9 + r] = Gp[3 * r] * rel[0] + Gp[3 * r + 1] * rel[1] + Gp[3 * r + 2] * rel[2] + Gp[9 + r];
        }
      }
#pragma unroll
      for (int e = 0; e < 12; ++e) G[12 * j + e] = g[e];
#pragma unroll
      for (int e = 0; e < 9; ++e) A[12 * j + e] = g[e];
#pragma unroll
      for (int r = 0; r < 3; ++r)
        A[12 * j + 9 + r] = g[9 + r] - (g[3 * r] * J[3 * j] + g[3 * r + 1] * J[3 * j + 1] + g[3 * r + 2] * J[3 * j + 2]);
    }
    __syncthreads();
  }
  // v_posed = v_template + S beta + feat P: one thread per coordinate, the loads of a wave are contiguous
  const int P3 = S.P3;
  for (int i = tid; i < P3; i += PTS_THREADS) {
    float sh = 0.f;
#pragma unroll
    for (int l = 0; l < 10; ++l) sh = fmaf(S.sd[i * 10 + l], beta[l], sh);
    // 486 = 8 x 60 + 6: eight independent chains, sixteen loads in flight (this loop is the latency of the forward)
    float a[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] = 0.f;
    const float* pd = S.pd + i;
#pragma unroll 2
    for (int k = 0; k < 480; k += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] = fmaf(feat[k + u], pd[(size_t)(k + u) * P3], a[u]);
    }
#pragma unroll
    for (int u = 0; u < 6; ++u) a[u] = fmaf(feat[480 + u], pd[(size_t)(480 + u) * P3], a[u]);
    vposed[i] = (((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))) + (S.vt[i] + sh);
  }
  __syncthreads();
}

__device__ __forceinline__ float pts_wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

__global__ __launch_bounds__(PTS_THREADS) void egx_points_fwd_kernel(PtsDev S, const float* __restrict__ xb_all,
                                                                     const float* __restrict__ betas_all, int fpa,
                                                                     float* __restrict__ out_points, float* __restrict__ out_joints) {
  extern __shared__ __attribute__((aligned(16))) float L[];
  float* vposed = L + L_FWD;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* xb = xb_all + (size_t)b * 93;
  pts_recompute(S, L, vposed, xb, betas_all + (size_t)(b / fpa) * 10);
  const float* A = L + L_A;
  const float tx = xb[0], ty = xb[1], tz = xb[2];
  const int P = S.P;
  for (int p = tid; p < P; p += PTS_THREADS) {
    float T[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = 0.f;
    for (int j = 0; j < NJ; ++j) {
      const float w = S.wT[j * P + p];
#pragma unroll
      for (int e = 0; e < 12; ++e) T[e] = fmaf(w, A[12 * j + e], T[e]);
    }
    const float v0 = vposed[3 * p], v1 = vposed[3 * p + 1], v2 = vposed[3 * p + 2];
    float* o = out_points + ((size_t)b * P + p) * 3;
    o[0] = (T[0] * v0 + T[1] * v1 + T[2] * v2 + T[9]) + tx;
    o[1] = (T[3] * v0 + T[4] * v1 + T[5] * v2 + T[10]) + ty;
    o[2] = (T[6] * v0 + T[7] * v1 + T[8] * v2 + T[11]) + tz;
  }
  if (out_joints && tid < NPOSE) out_joints[(size_t)b * NPOSE + tid] = L[L_G + 12 * (tid / 3) + 9 + tid % 3] + xb[tid % 3];
}

__global__ __launch_bounds__(PTS_THREADS) void egx_points_bwd_kernel(PtsDev S, const float* __restrict__ xb_all,
                                                                     const float* __restrict__ betas_all, int fpa,
                                                                     const float* __restrict__ grad_points,
                                                                     const float* __restrict__ grad_joints,
                                                                     float* __restrict__ grad_xb, float* __restrict__ grad_betas) {
  extern __shared__ __attribute__((aligned(16))) float L[];
  const int P = S.P, P3 = S.P3;
  float* Bw = L + L_FWD;              // backward part
  float* vposed = Bw + L_BWD;
  float* gx = vposed + P3;            // [3P] incoming point gradients
  float* dvp = gx + P3;               // [3P] d v_posed
  double* dG = reinterpret_cast<double*>(Bw + L_DG);   // [55][12] dGR | dGt
  float *dA = Bw + L_DA, *drel = Bw + L_DREL, *dJ = Bw + L_DJ, *dfeat = Bw + L_DFEAT, *dpose = Bw + L_DPOSE,
        *gj = Bw + L_GJ, *red = Bw + L_RED, *gsum = Bw + L_GSUM;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* xb = xb_all + (size_t)b * 93;
  pts_recompute(S, L, vposed, xb, betas_all + (size_t)(b / fpa) * 10);
  const float *R = L + L_R, *J = L + L_J, *G = L + L_G, *A = L + L_A, *pose = L + L_POSE;
  const int* tree = reinterpret_cast<const int*>(L + L_TREE);
  const bool has_gp = grad_points != nullptr;

  // ---- points: gx into LDS, d v_posed = (T^R)^T gx; the partial sums of g_transl
  float part[13];                     // 3..12 d beta through the points (0..2 unused)
  double tsum[3] = {0.0, 0.0, 0.0};   // g_transl: a plain sum of up to 1079 cotangents, in double
#pragma unroll
  for (int e = 0; e < 13; ++e) part[e] = 0.f;
  if (tid < NPOSE) {
    const float v = grad_joints ? grad_joints[(size_t)b * NPOSE + tid] : 0.f;
    gj[tid] = v;
  }
  if (has_gp) {
    for (int p = tid; p < P; p += PTS_THREADS) {
      const float* gp = grad_points + ((size_t)b * P + p) * 3;
      const float g0 = gp[0], g1 = gp[1], g2 = gp[2];
      gx[3 * p] = g0; gx[3 * p + 1] = g1; gx[3 * p + 2] = g2;
      tsum[0] += (double)g0; tsum[1] += (double)g1; tsum[2] += (double)g2;
      float T[9];
#pragma unroll
      for (int e = 0; e < 9; ++e) T[e] = 0.f;
      for (int j = 0; j < NJ; ++j) {
        const float w = S.wT[j * P + p];
#pragma unroll
        for (int e = 0; e < 9; ++e) T[e] = fmaf(w, A[12 * j + e], T[e]);
      }
      dvp[3 * p] = T[0] * g0 + T[3] * g1 + T[6] * g2;
      dvp[3 * p + 1] = T[1] * g0 + T[4] * g1 + T[7] * g2;
      dvp[3 * p + 2] = T[2] * g0 + T[5] * g1 + T[8] * g2;
    }
  }
  __syncthreads();
  if (has_gp) {
    // ---- dA_j = sum_p w_pj [gx_p v_posed_p^T | gx_p]: a wave per joint, lanes over the points
    for (int j = wave; j < NJ; j += 4) {
      float acc[12];
#pragma unroll
      for (int e = 0; e < 12; ++e) acc[e] = 0.f;
      for (int p = lane; p < P; p += 64) {
        const float w = S.wT[j * P + p];
        const float v0 = vposed[3 * p], v1 = vposed[3 * p + 1], v2 = vposed[3 * p + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const float a = w * gx[3 * p + r];
          acc[3 * r] = fmaf(a, v0, acc[3 * r]);
          acc[3 * r + 1] = fmaf(a, v1, acc[3 * r + 1]);
          acc[3 * r + 2] = fmaf(a, v2, acc[3 * r + 2]);
          acc[9 + r] += a;
        }
      }
#pragma unroll
      for (int e = 0; e < 12; ++e) acc[e] = pts_wave_sum(acc[e]);
      if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 12; ++e) dA[12 * j + e] = acc[e];
      }
    }
    // ---- d feat_k = sum_i posedirs[k][i] d v_posed[i]: a wave per eight features (eight loads in flight), lanes over the
    // coordinates; the last group of a wave is cut at 486 (wave-uniform tests)
    for (int k0 = wave * 8; k0 < NFEAT; k0 += 32) {
      float acc[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] = 0.f;
      for (int i = lane; i < P3; i += 64) {
        const float d = dvp[i];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (k0 + u < NFEAT) acc[u] = fmaf(S.pd[(size_t)(k0 + u) * P3 + i], d, acc[u]);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float v = pts_wave_sum(acc[u]);
        if (lane == 0 && k0 + u < NFEAT) dfeat[k0 + u] = v;
      }
    }
    // ---- d beta through the shape directions of the points
    for (int i = tid; i < P3; i += PTS_THREADS) {
      const float d = dvp[i];
#pragma unroll
      for (int l = 0; l < 10; ++l) part[3 + l] = fmaf(S.sd[i * 10 + l], d, part[3 + l]);
    }
  } else {
    for (int i = tid; i < NJ * 12; i += PTS_THREADS) dA[i] = 0.f;
    for (int i = tid; i < NFEAT; i += PTS_THREADS) dfeat[i] = 0.f;
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {          // the wave's sum as a float pair: slots e and 13 + e
    double v = tsum[e];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    const float hi = (float)v;
    if (lane == 0) { red[wave * 16 + e] = hi; red[wave * 16 + 13 + e] = (float)(v - (double)hi); }
  }
#pragma unroll
  for (int e = 3; e < 13; ++e) {
    const float v = pts_wave_sum(part[e]);
    if (lane == 0) red[wave * 16 + e] = v;
  }
  __syncthreads();
  if (tid < 3) {
    double v = 0.0;
    for (int w = 0; w < 4; ++w) v += (double)red[w * 16 + tid] + (double)red[w * 16 + 13 + tid];
    for (int j = 0; j < NJ; ++j) v += (double)gj[3 * j + tid];
    gsum[tid] = (float)v;
  } else if (tid < 13) {
    gsum[tid] = (red[tid] + red[16 + tid]) + (red[32 + tid] + red[48 + tid]);
  }
  // ---- dGR_j = dA_j^R - dA_j^t J_j^T, dGt_j = dA_j^t + gj_j, dJ_j = -GR_j^T dA_j^t
  if (tid < NJ) {
    const int j = tid;
    const double t0 = dA[12 * j + 9], t1 = dA[12 * j + 10], t2 = dA[12 * j + 11];
    const double tt[3] = {t0, t1, t2};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) dG[12 * j + 3 * r + c] = (double)dA[12 * j + 3 * r + c] - tt[r] * (double)J[3 * j + c];
      dG[12 * j + 9 + r] = tt[r] + (double)gj[3 * j + r];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      dJ[3 * j + c] = (float)-((double)G[12 * j + c] * t0 + (double)G[12 * j + 3 + c] * t1 + (double)G[12 * j + 6 + c] * t2);
  }
  __syncthreads();
  // ---- up the tree, deepest level first: dGR_q += sum_children dGR_c R_c^T + dGt_c rel_c^T, dGt_q += sum_children dGt_c
  for (int lev = S.num_levels - 2; lev >= 0; --lev) {
    for (int idx = tree[T_LOFF + lev] + tid; idx < tree[T_LOFF + lev + 1]; idx += PTS_THREADS) {
      const int q = tree[T_ORD + idx];
      double acc[12];
#pragma unroll
      for (int e = 0; e < 12; ++e) acc[e] = dG[12 * q + e];
      for (int ci = tree[T_COFF + q]; ci < tree[T_COFF + q + 1]; ++ci) {
        const int c = tree[T_CIDX + ci];
        const double* dc = dG + 12 * c;
        const float* Rc = R + 9 * c;
        const double rel[3] = {(double)J[3 * c] - (double)J[3 * q], (double)J[3 * c + 1] - (double)J[3 * q + 1],
                               (double)J[3 * c + 2] - (double)J[3 * q + 2]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int k = 0; k < 3; ++k)
            acc[3 * r + k] += dc[3 * r] * (double)Rc[3 * k] + dc[3 * r + 1] * (double)Rc[3 * k + 1] + dc[3 * r + 2] * (double)Rc[3 * k + 2] +
                              dc[9 + r] * rel[k];
          acc[9 + r] += dc[9 + r];
        }
      }
#pragma unroll
      for (int e = 0; e < 12; ++e) dG[12 * q + e] = acc[e];
    }
    __syncthreads();
  }
  // ---- dR_j = GR_par^T dGR_j (+ d feat_j), drel_j = GR_par^T dGt_j; back through the rotation of each joint
  if (tid < NJ) {
    const int j = tid;
    double dR[9];
    float dr[3];
    if (j == 0) {
#pragma unroll
      for (int e = 0; e < 9; ++e) dR[e] = dG[e];
      drel[0] = (float)dG[9]; drel[1] = (float)dG[10]; drel[2] = (float)dG[11];
    } else {
      const float* Gp = G + 12 * tree[T_PAR + j];
      const double* d = dG + 12 * j;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double g0 = Gp[r], g1 = Gp[3 + r], g2 = Gp[6 + r];
#pragma unroll
        for (int c = 0; c < 3; ++c) dR[3 * r + c] = (g0 * d[c] + g1 * d[3 + c] + g2 * d[6 + c]) + (double)dfeat[9 * (j - 1) + 3 * r + c];
        drel[3 * j + r] = (float)(g0 * d[9] + g1 * d[10] + g2 * d[11]);
      }
    }
    pts_rodrigues_bwd(pose + 3 * j, dR, dr);
    dpose[3 * j] = dr[0]; dpose[3 * j + 1] = dr[1]; dpose[3 * j + 2] = dr[2];
  }
  __syncthreads();
  // ---- dJ_j += drel_j - sum_children drel_c
  if (tid < NPOSE) {
    const int j = tid / 3, c = tid % 3;
    float v = dJ[tid] + drel[tid];
    for (int ci = tree[T_COFF + j]; ci < tree[T_COFF + j + 1]; ++ci) v -= drel[3 * tree[T_CIDX + ci] + c];
    dJ[tid] = v;
  }
  __syncthreads();
  // ---- outputs: transl | global orientation and body pose | hand coefficients through the PCA components; betas
  if (tid < 93) {
    float v;
    if (tid < 3) {
      v = gsum[tid];
    } else if (tid < 69) {
      v = dpose[tid - 3];
    } else {
      const int k = tid - 69;                                   // row of the [24][45] components
      const float* c = S.hc + k * 45;
      const float* d = dpose + (k < 12 ? 75 : 120);
      v = 0.f;
      for (int m = 0; m < 45; ++m) v = fmaf(c[m], d[m], v);
    }
    grad_xb[(size_t)b * 93 + tid] = v;
  } else if (tid >= 128 && tid < 138) {
    const int l = tid - 128;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int i = 0; i < NPOSE; i += 3) {
      a0 = fmaf(S.Jsd[i * 10 + l], dJ[i], a0);
      a1 = fmaf(S.Jsd[(i + 1) * 10 + l], dJ[i + 1], a1);
      a2 = fmaf(S.Jsd[(i + 2) * 10 + l], dJ[i + 2], a2);
    }
    grad_betas[(size_t)b * 10 + l] = ((a0 + a1) + a2) + gsum[3 + l];
  }
}

}  // namespace

struct egx_point_set {
  PtsDev dev;
  void* arena = nullptr;
};

extern "C" int egx_point_set_create(const egx_body_model_host* d, const int32_t* vids, int num_points, egx_point_set** out) {
  EGX_REQUIRE(d && vids && out, "null argument");
  EGX_REQUIRE(d->v_template_host && d->shapedirs_host && d->posedirs_host && d->J_regressor_host && d->parents_host &&
                  d->lbs_weights_host && d->hand_comps_l_host && d->hand_comps_r_host && d->hand_mean_l_host && d->hand_mean_r_host,
              "the body description lacks a table");
  EGX_REQUIRE(d->num_verts >= 1, "num_verts");
  EGX_REQUIRE(num_points >= 1 && num_points <= PTS_MAX, "a point set holds 1..1024 points");
  const int V = d->num_verts, P = num_points, P3 = 3 * P;
  for (int p = 0; p < P; ++p)
    if (vids[p] < 0 || vids[p] >= V) {
      egx_set_error("egx_point_set_create: vertex id " + std::to_string(vids[p]) + " (entry " + std::to_string(p) + ") outside [0, " +
                    std::to_string(V) + ")");
      return EGX_ERR_ARG;
    }
  // the tree: parents, joints by depth, children in ascending order
  std::vector<int> tree(T_SIZE, 0), depth(NJ, 0);
  int max_depth = 0;
  if (!lbs_joint_depths(d->parents_host, depth.data(), &max_depth)) { egx_set_error("egx_point_set_create: parents must be topologically ordered"); return EGX_ERR_ARG; }
  tree[T_PAR] = -1;
  for (int j = 1; j < NJ; ++j) tree[T_PAR + j] = d->parents_host[j];
  int n = 0;
  for (int lev = 0; lev <= max_depth; ++lev) {
    tree[T_LOFF + lev] = n;
    for (int j = 0; j < NJ; ++j)
      if (depth[j] == lev) tree[T_ORD + n++] = j;
  }
  for (int lev = max_depth + 1; lev <= NJ; ++lev) tree[T_LOFF + lev] = n;
  n = 0;
  for (int q = 0; q < NJ; ++q) {
    tree[T_COFF + q] = n;
    for (int j = 1; j < NJ; ++j)
      if (tree[T_PAR + j] == q) tree[T_CIDX + n++] = j;
  }
  tree[T_COFF + NJ] = n;

  // tables gathered at the points
  std::vector<float> vt(P3), sd((size_t)P3 * 10), pd((size_t)NFEAT * P3), wT((size_t)NJ * P), Jt(NPOSE), Jsd(NPOSE * 10), hc(24 * 45), hm(90);
  for (int p = 0; p < P; ++p) {
    const size_t v = (size_t)vids[p];
    for (int c = 0; c < 3; ++c) {
      vt[3 * p + c] = d->v_template_host[v * 3 + c];
      for (int l = 0; l < 10; ++l) sd[(size_t)(3 * p + c) * 10 + l] = d->shapedirs_host[(v * 3 + c) * 10 + l];
      for (int k = 0; k < NFEAT; ++k) pd[(size_t)k * P3 + 3 * p + c] = d->posedirs_host[(size_t)k * 3 * V + v * 3 + c];
    }
    for (int j = 0; j < NJ; ++j) wT[(size_t)j * P + p] = d->lbs_weights_host[v * NJ + j];
  }
  lbs_fold_joint_regressor(d, Jt.data(), Jsd.data());   // rest joints as an affine function of betas
  for (int i = 0; i < 12 * 45; ++i) { hc[i] = d->hand_comps_l_host[i]; hc[12 * 45 + i] = d->hand_comps_r_host[i]; }
  for (int i = 0; i < 45; ++i) { hm[i] = d->hand_mean_l_host[i]; hm[45 + i] = d->hand_mean_r_host[i]; }

  // one arena, every table 256-byte aligned
  const std::vector<std::pair<const void*, size_t>> parts = {
      {vt.data(), vt.size() * 4}, {sd.data(), sd.size() * 4}, {pd.data(), pd.size() * 4}, {wT.data(), wT.size() * 4},
      {Jt.data(), Jt.size() * 4}, {Jsd.data(), Jsd.size() * 4}, {hc.data(), hc.size() * 4}, {hm.data(), hm.size() * 4},
      {tree.data(), tree.size() * 4}};
  size_t total = 0;
  std::vector<size_t> off;
  for (const auto& pr : parts) { off.push_back(total); total += egx_align_up(pr.second, 256); }
  egx_point_set* s = new egx_point_set();
  hipError_t e = hipMalloc(&s->arena, total);
  if (e != hipSuccess) {
    delete s;
    egx_set_error(std::string("egx_point_set_create: hipMalloc: ") + hipGetErrorString(e));
    return EGX_ERR_HIP;
  }
  char* base = static_cast<char*>(s->arena);
  for (size_t i = 0; i < parts.size(); ++i) {
    e = hipMemcpy(base + off[i], parts[i].first, parts[i].second, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(s->arena);
      delete s;
      egx_set_error(std::string("egx_point_set_create: hipMemcpy: ") + hipGetErrorString(e));
      return EGX_ERR_HIP;
    }
  }
  PtsDev& D = s->dev;
  D.P = P; D.P3 = P3; D.num_levels = max_depth + 1;
  D.vt = reinterpret_cast<const float*>(base + off[0]);
  D.sd = reinterpret_cast<const float*>(base + off[1]);
  D.pd = reinterpret_cast<const float*>(base + off[2]);
  D.wT = reinterpret_cast<const float*>(base + off[3]);
  D.Jt = reinterpret_cast<const float*>(base + off[4]);
  D.Jsd = reinterpret_cast<const float*>(base + off[5]);
  D.hc = reinterpret_cast<const float*>(base + off[6]);
  D.hm = reinterpret_cast<const float*>(base + off[7]);
  D.tree = reinterpret_cast<const int*>(base + off[8]);
  *out = s;
  return EGX_OK;
}

extern "C" void egx_point_set_destroy(egx_point_set* set) {
  if (!set) return;
  if (set->arena) (void)hipFree(set->arena);
  delete set;
}

extern "C" int egx_point_set_size(const egx_point_set* set) { return set ? set->dev.P : 0; }

extern "C" int egx_points_forward(const egx_point_set* set, const float* xb, const float* betas, int num_bodies, int frames_per_agent,
                                  float* out_points, float* out_joints55, void* stream_) {
  EGX_REQUIRE(set && xb && betas && out_points, "null argument");
  EGX_REQUIRE(num_bodies >= 1 && frames_per_agent >= 1 && num_bodies % frames_per_agent == 0, "num_bodies must be a positive multiple of frames_per_agent");
  hipLaunchKernelGGL(egx_points_fwd_kernel, dim3(num_bodies), dim3(PTS_THREADS), pts_lds_bytes(set->dev.P, false),
                     static_cast<hipStream_t>(stream_), set->dev, xb, betas, frames_per_agent, out_points, out_joints55);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

extern "C" int egx_points_backward(const egx_point_set* set, const float* xb, const float* betas, int num_bodies, int frames_per_agent,
                                   const float* grad_points, const float* grad_joints55, float* grad_xb, float* grad_betas_body,
                                   void* stream_) {
  EGX_REQUIRE(set && xb && betas && grad_xb && grad_betas_body, "null argument");
  EGX_REQUIRE(grad_points || grad_joints55, "at least one incoming gradient");
  EGX_REQUIRE(num_bodies >= 1 && frames_per_agent >= 1 && num_bodies % frames_per_agent == 0, "num_bodies must be a positive multiple of frames_per_agent");
  hipLaunchKernelGGL(egx_points_bwd_kernel, dim3(num_bodies), dim3(PTS_THREADS), pts_lds_bytes(set->dev.P, true),
                     static_cast<hipStream_t>(stream_), set->dev, xb, betas, frames_per_agent, grad_points, grad_joints55, grad_xb,
                     grad_betas_body);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

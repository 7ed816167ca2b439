// Glue of the combo training step (GAMMAPrimitiveComboTrainOP, models_GAMMA_primitive.py:713-1093) between the predictor, the
// regressor and the body model: the reverse mode of the 6D -> axis-angle tail, the L1 + temporal-difference marker loss with
// its gradient, and the no-grad re-seeding block of calc_loss_rollout.  Plain fp32 / fp64 vector code, no atomics: every entry
// gives the same bits on the same inputs.
#include <algorithm>

#include "egx_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// egx_cont6d_to_aa_backward: reverse mode of egx_cont6d_item (egx_nets.h), recomputed from xb6 in double.
// Near the identity the gradient of 2 atan2(|v|, w) / |v| is a difference of two nearly equal terms (relative size |v|^2),
// so the per-joint arithmetic runs in double like pts_rodrigues_bwd of body_points.hip.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// a[6] read as a (3,2) matrix, g_aa[3] -> g_a[6]
__device__ void cont6d_joint_bwd(const float* __restrict__ a, const float* __restrict__ g_aa, float* __restrict__ g_a) {
  // ---- forward (baseops.py:119-130 cont2rotmat)
  const double a1[3] = {a[0], a[2], a[4]}, a2[3] = {a[1], a[3], a[5]};
  const double n1 = fmax(sqrt(dot3(a1, a1)), 1e-12);
  const double b1[3] = {a1[0] / n1, a1[1] / n1, a1[2] / n1};
  const double d = dot3(b1, a2);
  const double u[3] = {a2[0] - d * b1[0], a2[1] - d * b1[1], a2[2] - d * b1[2]};
  const double n2 = fmax(sqrt(dot3(u, u)), 1e-12);
  const double b2[3] = {u[0] / n2, u[1] / n2, u[2] / n2};
  double b3[3];
  cross3(b1, b2, b3);
  // rotation_matrix_to_quaternion works on m = R^T, whose rows are b1, b2, b3
  const double m00 = b1[0], m01 = b1[1], m02 = b1[2], m10 = b2[0], m11 = b2[1], m12 = b2[2], m20 = b3[0], m21 = b3[1], m22 = b3[2];
  int br;
  double t, p[4];
  if (m22 < 1e-6) {
    if (m00 > m11) { br = 0; t = 1.0 + m00 - m11 - m22; p[0] = m12 - m21; p[1] = t; p[2] = m01 + m10; p[3] = m20 + m02; }
    else           { br = 1; t = 1.0 - m00 + m11 - m22; p[0] = m20 - m02; p[1] = m01 + m10; p[2] = t; p[3] = m12 + m21; }
  } else {
    if (m00 < -m11) { br = 2; t = 1.0 - m00 - m11 + m22; p[0] = m01 - m10; p[1] = m20 + m02; p[2] = m12 + m21; p[3] = t; }
    else            { br = 3; t = 1.0 + m00 + m11 + m22; p[0] = t; p[1] = m12 - m21; p[2] = m20 - m02; p[3] = m01 - m10; }
  }
  const double sc = 0.5 / sqrt(t);
  const double w = p[0] * sc, v[3] = {p[1] * sc, p[2] * sc, p[3] * sc};
  const double s2 = dot3(v, v), s = sqrt(s2);
  // ---- backward: aa = v k(s, w), k = 2 atan2(+-s, +-w) / s; both signs have the same partial derivatives
  const double ga[3] = {g_aa[0], g_aa[1], g_aa[2]};
  double gv[3], gw;
  if (s2 > 0.0) {
    const double two_theta = 2.0 * ((w < 0.0) ? atan2(-s, -w) : atan2(s, w));
    const double k = two_theta / s, r2 = s2 + w * w;
    const double dk_ds = (2.0 * w / r2 - k) / s, dk_dw = -2.0 / r2;
    const double gk = dot3(ga, v);
    for (int e = 0; e < 3; ++e) gv[e] = ga[e] * k + gk * dk_ds * v[e] / s;
    gw = gk * dk_dw;
  } else {  // k = 2 is a constant of the graph here (torch's own graph gives sqrt'(0) * 0 = NaN)
    for (int e = 0; e < 3; ++e) gv[e] = 2.0 * ga[e];
    gw = 0.0;
  }
  // q = sc p, sc = 0.5 t^-1/2
  const double gq[4] = {gw, gv[0], gv[1], gv[2]};
  double gp[4], gt = 0.0;
  for (int e = 0; e < 4; ++e) { gp[e] = gq[e] * sc; gt += gq[e] * p[e]; }
  gt *= -0.5 * sc / t;
  // p and t are linear in m; gm[3*r + c] is the gradient of m_rc
  double gm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (br == 0) {
    gt += gp[1];
    gm[0] += gt; gm[4] -= gt; gm[8] -= gt;
    gm[5] += gp[0]; gm[7] -= gp[0]; gm[1] += gp[2]; gm[3] += gp[2]; gm[6] += gp[3]; gm[2] += gp[3];
  } else if (br == 1) {
    gt += gp[2];
    gm[0] -= gt; gm[4] += gt; gm[8] -= gt;
    gm[6] += gp[0]; gm[2] -= gp[0]; gm[1] += gp[1]; gm[3] += gp[1]; gm[5] += gp[3]; gm[7] += gp[3];
  } else if (br == 2) {
    gt += gp[3];
    gm[0] -= gt; gm[4] -= gt; gm[8] += gt;
    gm[1] += gp[0]; gm[3] -= gp[0]; gm[6] += gp[1]; gm[2] += gp[1]; gm[5] += gp[2]; gm[7] += gp[2];
  } else {
    gt += gp[0];
    gm[0] += gt; gm[4] += gt; gm[8] += gt;
    gm[5] += gp[1]; gm[7] -= gp[1]; gm[6] += gp[2]; gm[2] -= gp[2]; gm[1] += gp[3]; gm[3] -= gp[3];
  }
  double gb1[3] = {gm[0], gm[1], gm[2]}, gb2[3] = {gm[3], gm[4], gm[5]};
  const double gb3[3] = {gm[6], gm[7], gm[8]};
  // b3 = b1 x b2
  double c[3];
  cross3(b2, gb3, c);
  for (int e = 0; e < 3; ++e) gb1[e] += c[e];
  cross3(gb3, b1, c);
  for (int e = 0; e < 3; ++e) gb2[e] += c[e];
  // b2 = u / max(|u|, eps), u = a2 - (b1 . a2) b1
  double gu[3];
  {
    const double pr = (sqrt(dot3(u, u)) > 1e-12) ? dot3(b2, gb2) : 0.0;
    for (int e = 0; e < 3; ++e) gu[e] = (gb2[e] - b2[e] * pr) / n2;
  }
  const double gd = -dot3(gu, b1);
  double ga2[3];
  for (int e = 0; e < 3; ++e) {
    gb1[e] += -d * gu[e] + gd * a2[e];
    ga2[e] = gu[e] + gd * b1[e];
  }
  // b1 = a1 / max(|a1|, eps)
  const double pr1 = (sqrt(dot3(a1, a1)) > 1e-12) ? dot3(b1, gb1) : 0.0;
  for (int e = 0; e < 3; ++e) {
    g_a[2 * e] = (float)((gb1[e] - b1[e] * pr1) / n1);
    g_a[2 * e + 1] = (float)ga2[e];
  }
}

__global__ __launch_bounds__(256) void egx_cont6d_to_aa_bwd_kernel(const float* __restrict__ xb6, const float* __restrict__ g_out, int n,
                                                                   float* __restrict__ g_xb6) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * 23) return;
  const int row = idx / 23, j = idx % 23;
  const float* go = g_out + (size_t)row * 93;
  float* gx = g_xb6 + (size_t)row * 159;
  if (j == 22) {  // transl + hands: the incoming gradient passes through
    gx[0] = go[0]; gx[1] = go[1]; gx[2] = go[2];
    for (int e = 0; e < 24; ++e) gx[135 + e] = go[69 + e];
    return;
  }
  cont6d_joint_bwd(xb6 + (size_t)row * 159 + 3 + 6 * j, go + 3 + 3 * j, gx + 3 + 6 * j);
}

// ------------------------------------------------------------------------------------------------
// egx_primitive_loss_*: _calc_loss_rec (models_GAMMA_primitive.py:773-784) on Y, Y_rec [T,b,D] (row = b*D elements per frame)
// ------------------------------------------------------------------------------------------------
constexpr int LOSS_BLOCK = 256;
constexpr int LOSS_MAX_BLOCKS = EGX_PRIMITIVE_LOSS_WS_BYTES / (2 * (int)sizeof(double));   // 256

__device__ __forceinline__ float sgn(float x) { return (float)((x > 0.f) - (x < 0.f)); }

// temporal-difference residual of frame pair (t, t+1) at element e of the frame, formed as torch forms it: two fp32
// differences, then their fp32 difference (no products, so nothing for the compiler to contract)
__device__ __forceinline__ float td_residual(const float* __restrict__ Y, const float* __restrict__ Yr, size_t i, size_t row) {
  const float dr = Yr[i + row] - Yr[i], dy = Y[i + row] - Y[i];
  return dr - dy;
}

// stage 1: block g sums the elements g*chunk .. (g+1)*chunk; each thread adds its elements in index order, then a fixed tree
__global__ __launch_bounds__(LOSS_BLOCK) void egx_primitive_loss_partial_kernel(const float* __restrict__ Y, const float* __restrict__ Yr,
                                                                                size_t n, size_t row, size_t chunk,
                                                                                double* __restrict__ part) {
  __shared__ double sh[2][LOSS_BLOCK];
  const size_t lo = (size_t)blockIdx.x * chunk, hi = (lo + chunk < n) ? lo + chunk : n;
  const size_t n_td = n - row;
  double rec = 0.0, td = 0.0;
  for (size_t i = lo + threadIdx.x; i < hi; i += LOSS_BLOCK) {
    rec += (double)fabsf(Y[i] - Yr[i]);
    if (i < n_td) td += (double)fabsf(td_residual(Y, Yr, i, row));
  }
  sh[0][threadIdx.x] = rec;
  sh[1][threadIdx.x] = td;
  __syncthreads();
  for (int s = LOSS_BLOCK / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + s];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = sh[0][0];
    part[2 * blockIdx.x + 1] = sh[1][0];
  }
}

// stage 2: the partials in block order, the two means, one rounding to fp32 each
__global__ __launch_bounds__(64) void egx_primitive_loss_final_kernel(const double* __restrict__ part, int blocks, double n, double n_td,
                                                                      float w_rec, float w_td, float* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double rec = 0.0, td = 0.0;
  for (int g = 0; g < blocks; ++g) { rec += part[2 * g]; td += part[2 * g + 1]; }
  rec /= n;
  td = (n_td > 0.0) ? td / n_td : 0.0;
  out[0] = (float)((double)w_rec * rec + (double)w_td * td);
  out[1] = (float)rec;
  out[2] = (float)td;
}

__global__ __launch_bounds__(256) void egx_primitive_loss_bwd_kernel(const float* __restrict__ Y, const float* __restrict__ Yr, size_t n,
                                                                     size_t row, const float* __restrict__ g_loss, float w_rec,
                                                                     float w_td, float* __restrict__ g_Yr) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double g = (double)g_loss[0];
  const size_t n_td = n - row;
  const float s_rec = (float)(g * (double)w_rec / (double)n);
  const float s_td = n_td ? (float)(g * (double)w_td / (double)n_td) : 0.f;
  float k = 0.f;                                              // sign(D[t-1]) - sign(D[t])
  if (i >= row) k += sgn(td_residual(Y, Yr, i - row, row));
  if (i < n_td) k -= sgn(td_residual(Y, Yr, i, row));
  g_Yr[i] = fmaf(s_td, k, s_rec * sgn(Yr[i] - Y[i]));         // both products are exact (factors 0, +-1, +-2)
}

// ------------------------------------------------------------------------------------------------
// egx_primitive_reseed: the no-grad block of calc_loss_rollout (models_GAMMA_primitive.py:959-984), one workgroup per sequence
// ------------------------------------------------------------------------------------------------
struct ReseedArgs {
  const float *joints, *X_prev, *Yg, *R_prev, *T_prev;
  float *R_new, *T_new, *R_curr, *T_curr, *X, *Y;
  int J, t_his, t_pred, b;
};

__global__ __launch_bounds__(256) void egx_primitive_reseed_kernel(ReseedArgs a) {
  const int b = blockIdx.x;
  // canonical frame of the seed body (baseops.py:214-225; the arithmetic of egx_canonical_frame): every thread derives the
  // same twelve numbers from three joints, which is cheaper than a broadcast through LDS
  const float* j = a.joints + (size_t)b * a.J * 3;
  float x0 = j[6] - j[3], x1 = j[7] - j[4];
  const float nx = sqrtf(x0 * x0 + x1 * x1);
  x0 /= nx; x1 /= nx;
  float y0 = -x1, y1 = x0;
  const float ny = sqrtf(y0 * y0 + y1 * y1);
  y0 /= ny; y1 /= ny;
  const float Rn[9] = {x0, y0, 0.f, x1, y1, 0.f, 0.f, 0.f, 1.f};
  const float Tn[3] = {j[0], j[1], j[2]};
  float Rp[9], Tp[3], Rc[9], Tc[3];
  for (int e = 0; e < 9; ++e) Rp[e] = a.R_prev[(size_t)b * 9 + e];
  for (int e = 0; e < 3; ++e) Tp[e] = a.T_prev[(size_t)b * 3 + e];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Rc[3 * r + c] = fmaf(Rp[3 * r + 2], Rn[6 + c], fmaf(Rp[3 * r + 1], Rn[3 + c], Rp[3 * r] * Rn[c]));
    Tc[r] = fmaf(Rp[3 * r + 2], Tn[2], fmaf(Rp[3 * r + 1], Tn[1], Rp[3 * r] * Tn[0])) + Tp[r];
  }
  if (threadIdx.x == 0) {   // constant indices only: a runtime index into Rn / Rc would move them to scratch
#pragma unroll
    for (int e = 0; e < 9; ++e) { a.R_new[(size_t)b * 9 + e] = Rn[e]; a.R_curr[(size_t)b * 9 + e] = Rc[e]; }
#pragma unroll
    for (int e = 0; e < 3; ++e) { a.T_new[(size_t)b * 3 + e] = Tn[e]; a.T_curr[(size_t)b * 3 + e] = Tc[e]; }
  }
  // X = R_^T (X_prev - T_), Y = R_curr^T (Yg - T_curr): 67 points per frame; the frames of sequence b are the b-th rows of [t,b,201]
  for (int q = threadIdx.x; q < a.t_his * 67; q += blockDim.x) {
    const size_t off = ((size_t)(q / 67) * a.b + b) * 201 + 3 * (q % 67);
    const float v0 = a.X_prev[off] - Tn[0], v1 = a.X_prev[off + 1] - Tn[1], v2 = a.X_prev[off + 2] - Tn[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) a.X[off + c] = fmaf(Rn[6 + c], v2, fmaf(Rn[3 + c], v1, Rn[c] * v0));
  }
  for (int q = threadIdx.x; q < a.t_pred * 67; q += blockDim.x) {
    const size_t off = ((size_t)(q / 67) * a.b + b) * 201 + 3 * (q % 67);
    const float v0 = a.Yg[off] - Tc[0], v1 = a.Yg[off + 1] - Tc[1], v2 = a.Yg[off + 2] - Tc[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) a.Y[off + c] = fmaf(Rc[6 + c], v2, fmaf(Rc[3 + c], v1, Rc[c] * v0));
  }
}

}  // namespace

extern "C" int egx_cont6d_to_aa_backward(const float* xb6, const float* g_out, int num_rows, float* g_xb6, void* stream) {
  EGX_REQUIRE(xb6 && g_out && g_xb6, "null argument");
  EGX_REQUIRE(num_rows > 0 && num_rows <= (1 << 24), "1 <= num_rows <= 2^24");
  hipLaunchKernelGGL(egx_cont6d_to_aa_bwd_kernel, dim3(egx_ceil_div(num_rows * 23, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     xb6, g_out, num_rows, g_xb6);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

extern "C" int egx_primitive_loss_forward(const float* Y, const float* Y_rec, int T, int b, int D, float w_rec, float w_td, float* out3,
                                          void* workspace, void* stream) {
  EGX_REQUIRE(Y && Y_rec && out3 && workspace, "null argument");
  EGX_REQUIRE(T > 0 && b > 0 && D > 0, "empty tensor");
  const size_t row = (size_t)b * D, n = row * T;
  // 2048 elements per block at least; the grid depends on n alone, so the summation order does too
  const int blocks = (int)std::min<size_t>(LOSS_MAX_BLOCKS, (n + 2047) / 2048);
  const size_t chunk = (n + blocks - 1) / blocks;
  double* part = static_cast<double*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(egx_primitive_loss_partial_kernel, dim3(blocks), dim3(LOSS_BLOCK), 0, st, Y, Y_rec, n, row, chunk, part);
  hipLaunchKernelGGL(egx_primitive_loss_final_kernel, dim3(1), dim3(64), 0, st, part, blocks, (double)n, (double)(n - row), w_rec, w_td,
                     out3);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

extern "C" int egx_primitive_loss_backward(const float* Y, const float* Y_rec, int T, int b, int D, float w_rec, float w_td,
                                           const float* g_loss, float* g_Y_rec, void* stream) {
  EGX_REQUIRE(Y && Y_rec && g_loss && g_Y_rec, "null argument");
  EGX_REQUIRE(T > 0 && b > 0 && D > 0, "empty tensor");
  const size_t row = (size_t)b * D, n = row * T;
  EGX_REQUIRE((n + 255) / 256 < (1ull << 31), "tensor too large");
  hipLaunchKernelGGL(egx_primitive_loss_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), Y,
                     Y_rec, n, row, g_loss, w_rec, w_td, g_Y_rec);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

extern "C" int egx_primitive_reseed(const float* joints, int joints_per_body, const float* X_prev, const float* Yg, const float* R_prev,
                                    const float* T_prev, int t_his, int t_pred, int num_seqs, float* out_R_new, float* out_T_new,
                                    float* out_R_curr, float* out_T_curr, float* out_X, float* out_Y, void* stream) {
  EGX_REQUIRE(joints && X_prev && Yg && R_prev && T_prev && out_R_new && out_T_new && out_R_curr && out_T_curr && out_X && out_Y,
              "null argument");
  EGX_REQUIRE(joints_per_body >= 3 && t_his > 0 && t_pred > 0 && num_seqs > 0, "need >= 3 joints per body and non-empty windows");
  ReseedArgs a{joints, X_prev, Yg, R_prev, T_prev, out_R_new, out_T_new, out_R_curr, out_T_curr, out_X, out_Y,
               joints_per_body, t_his, t_pred, num_seqs};
  hipLaunchKernelGGL(egx_primitive_reseed_kernel, dim3(num_seqs), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

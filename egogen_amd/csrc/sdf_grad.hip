// Differentiable calc_sdf (crowd_ppo/utils.py:54-84 under torch autograd): value and gradient of the negated trilinear field from
// the eight corners a point gathers anyway, and a penetration penalty on arbitrary points with its backward.  Gather-bound like
// egx_sdf_sample (sdf.hip, profiles/r06_sdf_sample.md): four points per lane are in flight together, and the corners come from the
// bricked copy of the grid when the descriptor carries the tables of egx_sdf_build_coarse.  Resources, errors against float64
// and timings: profiles/sdf_grad.md.
#include "egx_common.h"
#include "egx_sdf.h"

#include <cmath>
#include <type_traits>

#ifndef EGX_SDF_GRAD_PPT
#define EGX_SDF_GRAD_PPT 4   // points per lane and trip
#endif

namespace {
enum { ROWMAJOR = 0, BRICKS = 1, SCENE_SET = 2 };   // where the corners come from; a set reads its body's scene, always bricked

struct SdfValGrad { float v, gx, gy, gz; double v64; };

// double arithmetic that rounds once per operation in every kernel it is inlined into (as egx_mul / egx_add for float)
__device__ __forceinline__ double d_mul(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ double d_add(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ double d_sub(double a, double b) {
#pragma clang fp contract(off)
  return a - b;
}
// clamped voxel coordinate of a world coordinate in double (the map of egx_sdf_voxel_coords)
__device__ __forceinline__ double voxel_coord_f64(float w, float c, float scale, int d) {
  const double n = d_mul(d_sub((double)w, (double)c), (double)scale);
  const double p = d_mul(d_sub(d_mul(d_add(n, 1.0), (double)d), 1.0), 0.5);
  return fmin(fmax(p, 0.0), (double)(d - 1));
}

// s = -trilinear and g = d s / d (x, y, z) from the cell of the point (egx_sdf.h).  The value is the shared accumulation
// egx_sdf_cell_neg_value, so it has the bits of egx_sdf_sample and of the LBS count.  The gradient
// takes the four corner differences along each axis first and combines them with the other two axes' weights (the differences
// of neighbouring samples are small and exact to a rounding; eight signed products would cancel instead), then multiplies by
// d voxel / d metre = scale * d_a / 2.  An axis whose clamped coordinate sits on the first or last sample plane has an
// unclamped coordinate <= 0 or >= d_a - 1: aten's clip_coordinates_set_grad gives exactly 0 there.  Every operation is spelled
// out (no contraction), so every kernel this is inlined into produces the same bits.
// WITH_F64 (the penalty's forward) also evaluates the value in double from the same eight corners: coordinates, weights and
// products in double, in the cell the float32 floor chose (the field is continuous, so a point within a rounding of a cell
// face is extrapolated from the neighbouring cell by that rounding).  What is left of float32 there is the samples themselves.
template <bool FROM_BRICKS, bool WITH_F64 = false>
__device__ __forceinline__ SdfValGrad sdf_value_grad_at(const SdfDev& s, const float* __restrict__ bricks, float x, float y, float z) {
#pragma clang fp contract(off)
  float px, py, pz;
  egx_sdf_voxel_coords(s, x, y, z, px, py, pz);
  const EgxSdfCell c = egx_sdf_cell<FROM_BRICKS>(s, bricks, px, py, pz);
  // gradient in voxel units: corner (i, j, k) is v{i}{j}0 for k = 0 and c{i}{j}y for k = 1
  const float b00 = egx_mul(c.wy0, c.wz0), b01 = egx_mul(c.wy0, c.wz1e), b10 = egx_mul(c.wy1e, c.wz0), b11 = egx_mul(c.wy1e, c.wz1e);   // (y, z)
  const float e00 = egx_mul(c.wx0, c.wz0), e01 = egx_mul(c.wx0, c.wz1e), e10 = egx_mul(c.wx1e, c.wz0), e11 = egx_mul(c.wx1e, c.wz1e);   // (x, z)
  float dx = egx_mul(egx_sub(c.v100, c.v000), b00);
  dx = __builtin_fmaf(egx_sub(c.c10y, c.c00y), b01, dx);
  dx = __builtin_fmaf(egx_sub(c.v110, c.v010), b10, dx);
  dx = __builtin_fmaf(egx_sub(c.c11y, c.c01y), b11, dx);
  float dy = egx_mul(egx_sub(c.v010, c.v000), e00);
  dy = __builtin_fmaf(egx_sub(c.c01y, c.c00y), e01, dy);
  dy = __builtin_fmaf(egx_sub(c.v110, c.v100), e10, dy);
  dy = __builtin_fmaf(egx_sub(c.c11y, c.c10y), e11, dy);
  float dz = egx_mul(egx_sub(c.c00y, c.v000), c.a00);
  dz = __builtin_fmaf(egx_sub(c.c01y, c.v010), c.a01, dz);
  dz = __builtin_fmaf(egx_sub(c.c10y, c.v100), c.a10, dz);
  dz = __builtin_fmaf(egx_sub(c.c11y, c.v110), c.a11, dz);
  const float kx = egx_mul(egx_mul((float)s.d0, 0.5f), s.scale), ky = egx_mul(egx_mul((float)s.d1, 0.5f), s.scale),
              kz = egx_mul(egx_mul((float)s.d2, 0.5f), s.scale);
  SdfValGrad r;
  r.v = egx_sdf_cell_neg_value(c);
  r.v64 = 0.0;
  if (WITH_F64) {
    const double qx = voxel_coord_f64(x, s.cx, s.scale, s.d0), qy = voxel_coord_f64(y, s.cy, s.scale, s.d1),
                 qz = voxel_coord_f64(z, s.cz, s.scale, s.d2);
    const double ux1 = c.x1_in ? d_sub(qx, (double)c.x0) : 0.0, uy1 = c.y1_in ? d_sub(qy, (double)c.y0) : 0.0, uz1 = c.z1_in ? d_sub(qz, (double)c.z0) : 0.0;
    const double ux0 = c.x1_in ? d_sub(1.0, ux1) : 1.0, uy0 = c.y1_in ? d_sub(1.0, uy1) : 1.0, uz0 = c.z1_in ? d_sub(1.0, uz1) : 1.0;
    const double lo0 = d_add(d_mul((double)c.v000, uz0), d_mul((double)c.c00y, uz1)), lo1 = d_add(d_mul((double)c.v010, uz0), d_mul((double)c.c01y, uz1));
    const double hi0 = d_add(d_mul((double)c.v100, uz0), d_mul((double)c.c10y, uz1)), hi1 = d_add(d_mul((double)c.v110, uz0), d_mul((double)c.c11y, uz1));
    const double lo = d_add(d_mul(lo0, uy0), d_mul(lo1, uy1)), hi = d_add(d_mul(hi0, uy0), d_mul(hi1, uy1));
    r.v64 = -d_add(d_mul(lo, ux0), d_mul(hi, ux1));
  }
  r.gx = (px > 0.f && px < (float)(s.d0 - 1)) ? -egx_mul(dx, kx) : 0.f;
  r.gy = (py > 0.f && py < (float)(s.d1 - 1)) ? -egx_mul(dy, ky) : 0.f;
  r.gz = (pz > 0.f && pz < (float)(s.d2 - 1)) ? -egx_mul(dz, kz) : 0.f;
  return r;
}

template <bool FROM_BRICKS>
__global__ __launch_bounds__(256) void egx_sdf_value_grad_kernel(SdfDev s, const float* __restrict__ bricks, const float* __restrict__ pts,
                                                                int64_t n, const float* __restrict__ cot, float* __restrict__ out_val,
                                                                float* __restrict__ out_grad) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += EGX_SDF_GRAD_PPT * stride) {
    SdfValGrad r[EGX_SDF_GRAD_PPT];
    float c[EGX_SDF_GRAD_PPT];
#pragma unroll
    for (int u = 0; u < EGX_SDF_GRAD_PPT; ++u) {
      const int64_t i = min(i0 + u * stride, n - 1);
      r[u] = sdf_value_grad_at<FROM_BRICKS>(s, bricks, pts[i * 3 + 0], pts[i * 3 + 1], pts[i * 3 + 2]);
      c[u] = cot ? cot[i] : 1.f;
    }
#pragma unroll
    for (int u = 0; u < EGX_SDF_GRAD_PPT; ++u) {
      const int64_t i = i0 + u * stride;
      if (i < n) {
        if (out_val) out_val[i] = r[u].v;
        out_grad[i * 3 + 0] = egx_mul(c[u], r[u].gx);
        out_grad[i * 3 + 1] = egx_mul(c[u], r[u].gy);
        out_grad[i * 3 + 2] = egx_mul(c[u], r[u].gz);
      }
    }
  }
}

// What a penalty launch reads its field from: one descriptor, or the table of a scene set (then `s` holds the shared dimensions).
struct PenaltyField {
  SdfDev s;
  const float* bricks;            // one scene with tables
  const SdfSceneDev* table;       // scene set
  const int* agent_scene;
  int n_scenes, fpa;
  size_t bricks_offset;           // bytes from a scene's bracket table to its bricked copy
};

// the field of body b; false when the body's agent names no scene of the set (nothing is read then)
template <int MODE>
__device__ __forceinline__ bool penalty_field_of(const PenaltyField& f, int b, SdfDev& s, const float*& bricks) {
  s = f.s;
  bricks = f.bricks;
  if (MODE == SCENE_SET) {
    const int sc = f.agent_scene[b / f.fpa];
    if (sc < 0 || sc >= f.n_scenes) return false;
    s = egx_sdf_scene(f.s, f.table[sc]);
    bricks = reinterpret_cast<const float*>(reinterpret_cast<const char*>(s.coarse) + f.bricks_offset);
  }
  return true;
}

// One workgroup per body.  The terms are formed in double from a double evaluation of the field (sdf_value_grad_at<.., true>):
// a float32 term carries the rounding of its voxel coordinate times the field's slope, and over a thousand terms that alone is
// an ulp of the sum.  Every lane sums its own points in index order, the 64 lanes of a wave combine in a butterfly (both
// partners of an exchange add the same two numbers), and lane 0 adds the four waves' sums in wave order: the order depends on P
// alone, so the penalty is bit-reproducible, and it is the float64 penalty of the float32 samples rounded once.  The count
// uses the float32 value, the bits of calc_sdf.
template <int MODE>
__global__ __launch_bounds__(256) void egx_sdf_penalty_forward_kernel(PenaltyField f, const float* __restrict__ pts, int P,
                                                                     const float* __restrict__ weights, float margin, int power,
                                                                     float* __restrict__ out_penalty, int* __restrict__ out_count) {
  __shared__ double s_sum[4];
  __shared__ int s_cnt[4];
  const int b = blockIdx.x;
  SdfDev s;
  const float* bricks;
  if (!penalty_field_of<MODE>(f, b, s, bricks)) {   // uniform per workgroup
    if (threadIdx.x == 0) {
      out_penalty[b] = 0.f;
      if (out_count) out_count[b] = -1;
    }
    return;
  }
  const float* __restrict__ bp = pts + (size_t)b * (size_t)P * 3;
  double sum = 0.0;
  int cnt = 0;
  for (int p0 = threadIdx.x; p0 < P; p0 += EGX_SDF_GRAD_PPT * 256) {
    float v[EGX_SDF_GRAD_PPT], w[EGX_SDF_GRAD_PPT];
    double v64[EGX_SDF_GRAD_PPT];
#pragma unroll
    for (int u = 0; u < EGX_SDF_GRAD_PPT; ++u) {
      const int p = min(p0 + u * 256, P - 1);
      const SdfValGrad r = sdf_value_grad_at<MODE != ROWMAJOR, true>(s, bricks, bp[(size_t)p * 3 + 0], bp[(size_t)p * 3 + 1], bp[(size_t)p * 3 + 2]);
      v[u] = r.v;       // the bits of calc_sdf: the count
      v64[u] = r.v64;   // the penalty
      w[u] = weights ? weights[p] : 1.f;
    }
#pragma unroll
    for (int u = 0; u < EGX_SDF_GRAD_PPT; ++u) {
      if (p0 + u * 256 < P) {
        const double h = fmax(d_sub((double)margin, v64[u]), 0.0);
        sum = d_add(sum, d_mul((double)w[u], power == 2 ? d_mul(h, h) : h));
        cnt += (w[u] > 0.f && v[u] < 0.f) ? 1 : 0;
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    sum = d_add(sum, __shfl_xor(sum, o));
    cnt += __shfl_xor(cnt, o);
  }
  if ((threadIdx.x & 63) == 0) {
    s_sum[threadIdx.x >> 6] = sum;
    s_cnt[threadIdx.x >> 6] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    out_penalty[b] = (float)d_add(d_add(d_add(s_sum[0], s_sum[1]), s_sum[2]), s_sum[3]);
    if (out_count) out_count[b] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
  }
}

// Work item = (body, run of 256 x PPT points): the scene of an item is uniform.  Everything is recomputed from the points.
template <int MODE>
__global__ __launch_bounds__(256) void egx_sdf_penalty_backward_kernel(PenaltyField f, const float* __restrict__ pts, int P, int runs,
                                                                      int64_t items, const float* __restrict__ weights, float margin,
                                                                      int power, const float* __restrict__ grad_penalty,
                                                                      float* __restrict__ grad_pts) {
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int b = (int)(item / runs);
    const int p0 = (int)(item - (int64_t)b * runs) * (EGX_SDF_GRAD_PPT * 256) + threadIdx.x;
    const float* __restrict__ bp = pts + (size_t)b * (size_t)P * 3;
    float* __restrict__ gp = grad_pts + (size_t)b * (size_t)P * 3;
    SdfDev s;
    const float* bricks;
    if (!penalty_field_of<MODE>(f, b, s, bricks)) {
#pragma unroll
      for (int u = 0; u < EGX_SDF_GRAD_PPT; ++u) {
        const int p = p0 + u * 256;
        if (p < P) gp[(size_t)p * 3 + 0] = gp[(size_t)p * 3 + 1] = gp[(size_t)p * 3 + 2] = 0.f;
      }
      continue;
    }
    const float gb = grad_penalty[b];
    SdfValGrad r[EGX_SDF_GRAD_PPT];
    float w[EGX_SDF_GRAD_PPT];
#pragma unroll
    for (int u = 0; u < EGX_SDF_GRAD_PPT; ++u) {
      const int p = min(p0 + u * 256, P - 1);
      r[u] = sdf_value_grad_at<MODE != ROWMAJOR>(s, bricks, bp[(size_t)p * 3 + 0], bp[(size_t)p * 3 + 1], bp[(size_t)p * 3 + 2]);
      w[u] = weights ? weights[p] : 1.f;
    }
#pragma unroll
    for (int u = 0; u < EGX_SDF_GRAD_PPT; ++u) {
      const int p = p0 + u * 256;
      if (p < P) {
        // d/ds of max(margin - s, 0)^power: -2 max(margin - s, 0), or -1 where s < margin strictly
        const float dh = power == 2 ? egx_mul(-2.f, fmaxf(egx_sub(margin, r[u].v), 0.f)) : (r[u].v < margin ? -1.f : 0.f);
        const float c = egx_mul(egx_mul(gb, w[u]), dh);
        gp[(size_t)p * 3 + 0] = egx_mul(c, r[u].gx);
        gp[(size_t)p * 3 + 1] = egx_mul(c, r[u].gy);
        gp[(size_t)p * 3 + 2] = egx_mul(c, r[u].gz);
      }
    }
  }
}

constexpr int MAX_POINTS_PER_BODY = 1 << 20;

// shared argument checks of the two penalty calls; fills the field and the instantiation to launch
int penalty_field(const egx_sdf_grid* sdf, const egx_sdf_scene_set* scenes, const int32_t* agent_scene, const float* pts, int B, int P,
                  int fpa, float margin, int power, PenaltyField* f, int* mode) {
  EGX_REQUIRE((sdf != nullptr) != (scenes != nullptr), "exactly one of sdf / scenes");
  EGX_REQUIRE(pts && B >= 1 && P >= 1 && P <= MAX_POINTS_PER_BODY, "points [B,P,3] with B >= 1 and 1 <= P <= 2^20");
  EGX_REQUIRE(fpa >= 1 && B % fpa == 0, "num_bodies must be a multiple of frames_per_agent");
  EGX_REQUIRE((power == 1 || power == 2) && std::isfinite(margin), "power in {1, 2} and a finite margin");
  *f = PenaltyField{};
  f->fpa = fpa;
  if (sdf) {
    EGX_REQUIRE(egx_sdf_grid_ok(sdf), "sdf grid needs d2 >= 2 and fewer than 2^32 samples");
    f->s = egx_sdf_dev(*sdf);
    f->bricks = egx_sdf_bricks(*sdf);   // the tables of egx_sdf_build_coarse are there: gather from the bricked copy
    *mode = f->bricks ? BRICKS : ROWMAJOR;
  } else {
    EGX_REQUIRE(agent_scene && scenes->S >= 1 && scenes->table, "a scene set needs agent_scene");
    f->s = egx_sdf_dev(scenes->dims);   // the scenes of a set carry their tables (egx_sdf_scene_set_create)
    f->table = scenes->table;
    f->agent_scene = agent_scene;
    f->n_scenes = scenes->S;
    f->bricks_offset = egx_sdf_bricks_offset(f->s.c0, f->s.c1, f->s.c2);
    *mode = SCENE_SET;
  }
  return EGX_OK;
}

// launch(mode as an std::integral_constant) for the mode penalty_field chose: the three instantiations of a penalty kernel
template <typename Launch>
void with_penalty_mode(int mode, Launch&& launch) {
  if (mode == ROWMAJOR) launch(std::integral_constant<int, ROWMAJOR>{});
  else if (mode == BRICKS) launch(std::integral_constant<int, BRICKS>{});
  else launch(std::integral_constant<int, SCENE_SET>{});
}
}  // namespace

extern "C" int egx_sdf_value_grad(const egx_sdf_grid* sdf, const float* pts, int64_t n, const float* cotangent, float* out_val,
                                  float* out_grad, void* stream_) {
  EGX_REQUIRE(egx_sdf_grid_ok(sdf), "sdf grid needs d2 >= 2 and fewer than 2^32 samples");
  if (n == 0) return EGX_OK;  // empty input is legal
  EGX_REQUIRE(pts && out_grad && n > 0, "null points / gradient output");
  const SdfDev s = egx_sdf_dev(*sdf);
  const float* bricks = egx_sdf_bricks(*sdf);
  const int64_t blocks = (n + 256 * EGX_SDF_GRAD_PPT - 1) / (256 * EGX_SDF_GRAD_PPT);
  const int grid = (int)(blocks < 8192 ? blocks : 8192);
  hipStream_t st = static_cast<hipStream_t>(stream_);
  if (bricks)
    hipLaunchKernelGGL(egx_sdf_value_grad_kernel<true>, dim3(grid), dim3(256), 0, st, s, bricks, pts, n, cotangent, out_val, out_grad);
  else
    hipLaunchKernelGGL(egx_sdf_value_grad_kernel<false>, dim3(grid), dim3(256), 0, st, s, bricks, pts, n, cotangent, out_val, out_grad);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

extern "C" int egx_sdf_penalty_forward(const egx_sdf_grid* sdf, const egx_sdf_scene_set* scenes, const int32_t* agent_scene,
                                       const float* pts, int num_bodies, int points_per_body, int frames_per_agent, const float* weights,
                                       float margin, int power, float* out_penalty, int32_t* out_count, void* stream_) {
  PenaltyField f;
  int mode;
  if (int rc = penalty_field(sdf, scenes, agent_scene, pts, num_bodies, points_per_body, frames_per_agent, margin, power, &f, &mode)) return rc;
  EGX_REQUIRE(out_penalty, "null penalty output");
  hipStream_t st = static_cast<hipStream_t>(stream_);
  const dim3 grid(num_bodies), block(256);
  with_penalty_mode(mode, [&](auto m) {
    hipLaunchKernelGGL(egx_sdf_penalty_forward_kernel<decltype(m)::value>, grid, block, 0, st, f, pts, points_per_body, weights, margin, power,
                       out_penalty, out_count);
  });
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

extern "C" int egx_sdf_penalty_backward(const egx_sdf_grid* sdf, const egx_sdf_scene_set* scenes, const int32_t* agent_scene,
                                        const float* pts, int num_bodies, int points_per_body, int frames_per_agent, const float* weights,
                                        float margin, int power, const float* grad_penalty, float* grad_pts, void* stream_) {
  PenaltyField f;
  int mode;
  if (int rc = penalty_field(sdf, scenes, agent_scene, pts, num_bodies, points_per_body, frames_per_agent, margin, power, &f, &mode)) return rc;
  EGX_REQUIRE(grad_penalty && grad_pts, "null penalty cotangent / gradient output");
  hipStream_t st = static_cast<hipStream_t>(stream_);
  const int runs = egx_ceil_div(points_per_body, EGX_SDF_GRAD_PPT * 256);
  const int64_t items = (int64_t)num_bodies * runs;
  const dim3 grid((unsigned)(items < 16384 ? items : 16384)), block(256);
  with_penalty_mode(mode, [&](auto m) {
    hipLaunchKernelGGL(egx_sdf_penalty_backward_kernel<decltype(m)::value>, grid, block, 0, st, f, pts, points_per_body, runs, items, weights,
                       margin, power, grad_penalty, grad_pts);
  });
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

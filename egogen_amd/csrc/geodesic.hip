// Geodesic distance to a goal over the walkable raster (free [H,W], origin, cell of scene_gen.walkable_grid and of the scene files):
// egx_geodesic_field builds F fields by pull-form relaxation, egx_geodesic_sample reads them at points (egx_geodesic.h, the function
// the selection kernels of genop.hip call).
//
// The field is the fixed point dist[c] = min(seed value of c, min over allowed neighbours n of dist[n] + w) on the 8-neighbour
// graph of free cells (no diagonal past a blocked axis cell), one float32 addition per edge.  Float32 addition of a constant is
// monotone, so the fixed point does not depend on the order of relaxation and equals float32 Dijkstra bit for bit; every value a
// pass holds is the length of some path from a seed, i.e. never below the fixed point, and values only fall.
//
// One launch is one pass: a workgroup loads a 32 x 32 tile with a one-cell halo from the buffer the pass reads, relaxes it in LDS
// until the tile stops changing (each thread owns four cells and takes the minimum over their neighbours; no atomics), writes the
// interior to the buffer the pass writes and raises the pass's flag if a cell fell.  Workgroups meet only at kernel boundaries.
// The host launches EGX_GEODESIC_BATCH passes between two reads of the flag and stops at the first batch whose last pass
// changed nothing: then the buffer it read is a fixed point (and equal to the one it wrote).  The loop is capped at H*W + 1 passes:
// the k-th cell in Dijkstra's order is final after k - 1 passes, whatever the tiles do.
#include "egx_common.h"
#include "egx_geodesic.h"

#include <limits.h>

namespace {

constexpr int T = 32, TH = T + 2;          // tile and tile with halo
constexpr int GBLK = 256, CPT = T * T / GBLK;
constexpr int MAX_INNER = T * T + 1;       // a shortest path inside a tile has at most T*T cells: the inner loop cannot run longer

__global__ __launch_bounds__(GBLK) void egx_geodesic_fill_kernel(float* __restrict__ dist, size_t total) {
  const size_t i = (size_t)blockIdx.x * GBLK + threadIdx.x;
  if (i < total) dist[i] = __builtin_inff();
}

// seeds onto the filled buffer; an integer minimum on the bits (non-negative floats order like their bits) settles two seeds on one cell
__global__ __launch_bounds__(GBLK) void egx_geodesic_seed_kernel(const uint8_t* __restrict__ free_mask, const int* __restrict__ field_scene,
                                                                 int S, int F, int HW, const int* __restrict__ seed_cell,
                                                                 const float* __restrict__ seed_value, int n, float* __restrict__ dist) {
  const int s = blockIdx.x * GBLK + threadIdx.x;
  if (s >= n) return;
  const long long c = seed_cell[s];
  const float v = seed_value[s];
  if (c < 0 || c >= (long long)F * HW || !(v >= 0.f && v < __builtin_inff())) return;
  const int f = (int)(c / HW), sc = field_scene ? min(max(field_scene[f], 0), S - 1) : 0;
  if (!free_mask[(size_t)sc * HW + (size_t)(c % HW)]) return;
  atomicMin(reinterpret_cast<int*>(dist) + c, __float_as_int(v));
}

__global__ __launch_bounds__(GBLK) void egx_geodesic_pass_kernel(const uint8_t* __restrict__ free_mask, const int* __restrict__ field_scene,
                                                                 int S, int H, int W, int tiles_w, float w1, float w2,
                                                                 const float* __restrict__ in, float* __restrict__ out,
                                                                 int* __restrict__ changed) {
  __shared__ float s_d[TH][TH];
  __shared__ uint8_t s_f[TH][TH];
  const int tid = threadIdx.x, f = blockIdx.y;
  const int i0 = (blockIdx.x / tiles_w) * T, j0 = (blockIdx.x % tiles_w) * T;
  const int sc = field_scene ? min(max(field_scene[f], 0), S - 1) : 0;
  const size_t HW = (size_t)H * W;
  const uint8_t* fm = free_mask + (size_t)sc * HW;
  const float* din = in + (size_t)f * HW;
  const float inf = __builtin_inff();

  for (int e = tid; e < TH * TH; e += GBLK) {
    const int li = e / TH, lj = e % TH, gi = i0 + li - 1, gj = j0 + lj - 1;
    const bool inside = gi >= 0 && gi < H && gj >= 0 && gj < W;
    const bool fr = inside && fm[(size_t)gi * W + gj] != 0;
    s_f[li][lj] = fr ? 1 : 0;
    s_d[li][lj] = fr ? din[(size_t)gi * W + gj] : inf;          // a blocked cell is +inf whatever the buffer holds
  }
  __syncthreads();

  int li[CPT], lj[CPT];
  unsigned diag[CPT];      // bit 0..3: the diagonal (-1,-1), (-1,+1), (+1,-1), (+1,+1) is allowed; bit 4: the cell is free
  float v[CPT], first[CPT];
  for (int k = 0; k < CPT; ++k) {
    const int c = tid + k * GBLK;
    li[k] = c / T + 1; lj[k] = c % T + 1;
    const bool up = s_f[li[k] - 1][lj[k]], dn = s_f[li[k] + 1][lj[k]], lf = s_f[li[k]][lj[k] - 1], rt = s_f[li[k]][lj[k] + 1];
    diag[k] = (up && lf ? 1u : 0u) | (up && rt ? 2u : 0u) | (dn && lf ? 4u : 0u) | (dn && rt ? 8u : 0u) | (s_f[li[k]][lj[k]] ? 16u : 0u);
    v[k] = first[k] = s_d[li[k]][lj[k]];
  }

  for (int it = 0; it < MAX_INNER; ++it) {
    float nv[CPT];
    for (int k = 0; k < CPT; ++k) {
      const int a = li[k], b = lj[k];
      float m = v[k];
      if (diag[k] & 16u) {                                          // blocked neighbours hold +inf: the axis steps need no test
        m = fminf(m, s_d[a - 1][b] + w1);
        m = fminf(m, s_d[a + 1][b] + w1);
        m = fminf(m, s_d[a][b - 1] + w1);
        m = fminf(m, s_d[a][b + 1] + w1);
        if (diag[k] & 1u) m = fminf(m, s_d[a - 1][b - 1] + w2);
        if (diag[k] & 2u) m = fminf(m, s_d[a - 1][b + 1] + w2);
        if (diag[k] & 4u) m = fminf(m, s_d[a + 1][b - 1] + w2);
        if (diag[k] & 8u) m = fminf(m, s_d[a + 1][b + 1] + w2);
      }
      nv[k] = m;
    }
    __syncthreads();                                                 // every read of this round precedes every write of it
    int ch = 0;
    for (int k = 0; k < CPT; ++k)
      if (nv[k] < v[k]) { v[k] = nv[k]; s_d[li[k]][lj[k]] = nv[k]; ch = 1; }
    if (!__syncthreads_or(ch)) break;
  }

  int fell = 0;
  float* dout = out + (size_t)f * HW;
  for (int k = 0; k < CPT; ++k) {
    const int gi = i0 + li[k] - 1, gj = j0 + lj[k] - 1;
    if (gi < H && gj < W) {
      dout[(size_t)gi * W + gj] = v[k];
      fell |= (v[k] < first[k]) ? 1 : 0;
    }
  }
  if (__syncthreads_or(fell) && tid == 0) *changed = 1;
}

__global__ __launch_bounds__(GBLK) void egx_geodesic_sample_kernel(const float* __restrict__ dist, const float* __restrict__ origin,
                                                                   float cell, int F, int H, int W, const float* __restrict__ points,
                                                                   int n, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * GBLK + threadIdx.x;
  if (i >= (size_t)F * n) return;
  const int f = (int)(i / n);
  out[i] = egx_geodesic_sample_at(dist + (size_t)f * H * W, H, W, origin[f * 2 + 0], origin[f * 2 + 1], cell, points[i * 2 + 0],
                                  points[i * 2 + 1]);
}

}  // namespace

extern "C" int egx_geodesic_field(const uint8_t* free_mask, const int32_t* field_scene, int num_scenes, int num_fields, int H, int W,
                                  float w1, float w2, const int32_t* seed_cell, const float* seed_value, int num_seeds, float* dist,
                                  float* tmp, int32_t* flags, int32_t* passes_host, void* stream_) {
  EGX_REQUIRE(free_mask && seed_cell && seed_value && dist && tmp && flags, "null argument");
  EGX_REQUIRE(num_scenes >= 1 && num_fields >= 1 && H >= 1 && W >= 1 && num_seeds >= 1, "need a raster, a field and a seed");
  EGX_REQUIRE(field_scene || num_scenes == 1, "several rasters need field_scene");
  EGX_REQUIRE(w1 > 0.f && w2 > 0.f && w1 < __builtin_inff() && w2 < __builtin_inff(), "edge weights must be positive and finite");
  EGX_REQUIRE(dist != tmp, "dist and tmp are read and written in turn");
  const long long HW = (long long)H * W, total = HW * num_fields;
  EGX_REQUIRE(total <= INT_MAX && HW * num_scenes <= INT_MAX, "F*H*W and S*H*W must stay below 2^31");
  EGX_REQUIRE(num_fields <= 65535, "at most 65535 fields per call");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (passes_host) *passes_host = 0;

  hipLaunchKernelGGL(egx_geodesic_fill_kernel, dim3((unsigned)((total + GBLK - 1) / GBLK)), dim3(GBLK), 0, stream, dist, (size_t)total);
  hipLaunchKernelGGL(egx_geodesic_seed_kernel, dim3((unsigned)egx_ceil_div(num_seeds, GBLK)), dim3(GBLK), 0, stream, free_mask, field_scene,
                     num_scenes, num_fields, (int)HW, seed_cell, seed_value, num_seeds, dist);
  EGX_HIP_CHECK(hipGetLastError());

  const int tiles_h = egx_ceil_div(H, T), tiles_w = egx_ceil_div(W, T);
  const long long cap = HW + 1;
  long long passes = 0;
  float *src = dist, *dst = tmp;
  while (passes < cap) {
    const int nb = (int)((cap - passes < EGX_GEODESIC_BATCH) ? cap - passes : EGX_GEODESIC_BATCH);
    EGX_HIP_CHECK(hipMemsetAsync(flags, 0, EGX_GEODESIC_BATCH * sizeof(int32_t), stream));
    for (int k = 0; k < nb; ++k) {
      hipLaunchKernelGGL(egx_geodesic_pass_kernel, dim3((unsigned)(tiles_h * tiles_w), (unsigned)num_fields), dim3(GBLK), 0, stream,
                         free_mask, field_scene, num_scenes, H, W, tiles_w, w1, w2, src, dst, flags + k);
      float* t = src; src = dst; dst = t;
    }
    EGX_HIP_CHECK(hipGetLastError());
    passes += nb;
    int32_t last = 1;
    EGX_HIP_CHECK(hipMemcpyAsync(&last, flags + (nb - 1), sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    EGX_HIP_CHECK(hipStreamSynchronize(stream));
    if (passes_host) *passes_host = (int32_t)passes;
    if (!last) return EGX_OK;       // the last pass changed nothing: the buffer it read equals the one it wrote, so dist holds the field
  }
  egx_set_error("egx_geodesic_field: the field still changed after H*W + 1 passes");
  return EGX_ERR_CONVERGENCE;
}

extern "C" int egx_geodesic_sample(const float* dist, const float* origin, float cell, int num_fields, int H, int W, const float* points,
                                   int num_points, float* out, void* stream) {
  EGX_REQUIRE(dist && origin && points && out, "null argument");
  EGX_REQUIRE(num_fields >= 1 && H >= 1 && W >= 1 && num_points >= 1, "need a field and a point");
  EGX_REQUIRE(cell > 0.f && cell < __builtin_inff(), "cell must be positive and finite");
  EGX_REQUIRE((long long)num_fields * H * W <= INT_MAX && (long long)num_fields * num_points <= INT_MAX, "sizes must stay below 2^31");
  const long long n = (long long)num_fields * num_points;
  hipLaunchKernelGGL(egx_geodesic_sample_kernel, dim3((unsigned)((n + GBLK - 1) / GBLK)), dim3(GBLK), 0, static_cast<hipStream_t>(stream), dist,
                     origin, cell, num_fields, H, W, points, num_points, out);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

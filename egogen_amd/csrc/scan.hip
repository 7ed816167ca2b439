// Scene preparation from scanned room meshes (open triangle soups): the signed distance grid of an oriented, possibly open mesh
// (BVH nearest-triangle search, sign from the pseudo-normal of the nearest feature) and the walkable raster of the floor
// (support + clearance per cell).  The host side (welding, pseudo-normals, BVH build, floor detection, erosion) is in
// egogen_amd/scene_gen.py.
#include "egx_common.h"
#include "egx_sdf.h"   // egx_sdf_dims_ok

namespace {

// Closest point of triangle (a, b, c) to p (Ericson, Real-Time Collision Detection 5.1.5), relative to a.  Returns the squared
// distance; `region` names the feature the closest point lies on: 0 face, 1/2/3 vertex a/b/c, 4/5/6 edge ab/bc/ca.
__device__ __forceinline__ float scan_tri_closest(const float4 A, const float4 B, const float4 Cv, float px, float py, float pz,
                                                  int& region) {
  const float abx = B.x - A.x, aby = B.y - A.y, abz = B.z - A.z;
  const float acx = Cv.x - A.x, acy = Cv.y - A.y, acz = Cv.z - A.z;
  const float apx = px - A.x, apy = py - A.y, apz = pz - A.z;
  const float d1 = abx * apx + aby * apy + abz * apz, d2 = acx * apx + acy * apy + acz * apz;
  float cx, cy, cz;
  if (d1 <= 0.f && d2 <= 0.f) {
    cx = cy = cz = 0.f;
    region = 1;
  } else {
    const float bpx = apx - abx, bpy = apy - aby, bpz = apz - abz;
    const float d3 = abx * bpx + aby * bpy + abz * bpz, d4 = acx * bpx + acy * bpy + acz * bpz;
    const float cpx = apx - acx, cpy = apy - acy, cpz = apz - acz;
    const float d5 = abx * cpx + aby * cpy + abz * cpz, d6 = acx * cpx + acy * cpy + acz * cpz;
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d3 >= 0.f && d4 <= d3) {
      cx = abx; cy = aby; cz = abz;
      region = 2;
    } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
      const float v = d1 / (d1 - d3);
      cx = v * abx; cy = v * aby; cz = v * abz;
      region = 4;
    } else if (d6 >= 0.f && d5 <= d6) {
      cx = acx; cy = acy; cz = acz;
      region = 3;
    } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
      const float w = d2 / (d2 - d6);
      cx = w * acx; cy = w * acy; cz = w * acz;
      region = 6;
    } else if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {
      const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
      cx = abx + w * (acx - abx); cy = aby + w * (acy - aby); cz = abz + w * (acz - abz);
      region = 5;
    } else {
      const float den = 1.f / (va + vb + vc);
      const float v = vb * den, w = vc * den;
      cx = abx * v + acx * w; cy = aby * v + acy * w; cz = abz * v + acz * w;
      region = 0;
    }
  }
  const float dx = apx - cx, dy = apy - cy, dz = apz - cz;
  return dx * dx + dy * dy + dz * dz;
}

__device__ __forceinline__ float scan_seg_d2(const float4 A, const float4 B, float px, float py, float pz) {
  const float ex = B.x - A.x, ey = B.y - A.y, ez = B.z - A.z;
  const float apx = px - A.x, apy = py - A.y, apz = pz - A.z;
  const float t = fminf(fmaxf((apx * ex + apy * ey + apz * ez) / fmaxf(ex * ex + ey * ey + ez * ez, 1e-30f), 0.f), 1.f);
  const float dx = apx - t * ex, dy = apy - t * ey, dz = apz - t * ez;
  return dx * dx + dy * dy + dz * dz;
}

// squared distance from p to an axis-aligned box (0 inside; +inf for the empty boxes of padding leaves)
__device__ __forceinline__ float scan_box_d2(const float4* __restrict__ nodes, unsigned h, float px, float py, float pz) {
  const float4 lo = nodes[2 * (size_t)(h - 1)], hi = nodes[2 * (size_t)(h - 1) + 1];
  const float dx = fmaxf(fmaxf(lo.x - px, px - hi.x), 0.f);
  const float dy = fmaxf(fmaxf(lo.y - py, py - hi.y), 0.f);
  const float dz = fmaxf(fmaxf(lo.z - pz, pz - hi.z), 0.f);
  return dx * dx + dy * dy + dz * dz;
}

// One lane per sample; a wave covers a 4x4x4 brick of samples, so its lanes walk similar paths through the tree.  The tree is
// the implicit complete binary tree of the host builder (heap index h: children 2h, 2h+1; leaves at depth `levels`), so the
// traversal needs no stack: `pend` holds one bit per level whose far child is still to visit, `near_r` which child was near.
// Backtracking re-tests the far child's box against the (by then smaller) best distance.
__global__ __launch_bounds__(256) void egx_scan_sdf_kernel(const float4* __restrict__ nodes, int levels, const float4* __restrict__ tris,
                                                          const float* __restrict__ pn, int F, int leaf, float cx, float cy, float cz,
                                                          float inv_scale, int d0, int d1, int d2, float* __restrict__ out) {
  const int nb1 = (d1 + 3) >> 2, nb2 = (d2 + 3) >> 2;
  const size_t brick = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int bk = (int)(brick % nb2), bj = (int)((brick / nb2) % nb1), bi = (int)(brick / ((size_t)nb1 * nb2));
  const int i = bi * 4 + (lane >> 4), j = bj * 4 + ((lane >> 2) & 3), k = bk * 4 + (lane & 3);
  if (i >= d0 || j >= d1 || k >= d2) return;
  const float px = cx + ((2 * i + 1) / (float)d0 - 1.f) * inv_scale;
  const float py = cy + ((2 * j + 1) / (float)d1 - 1.f) * inv_scale;
  const float pz = cz + ((2 * k + 1) / (float)d2 - 1.f) * inv_scale;

  float best = 3.4e38f, best_s = 3.4e38f;   // nearest triangle of any kind / nearest non-degenerate one (decides the sign)
  int best_t = -1;
  unsigned h = 1, pend = 0, near_r = 0;
  int depth = 0;
  for (;;) {
    bool descend = false;
    if (depth == levels) {
      const int t0 = (int)(h - (1u << levels)) * leaf, t1 = min(t0 + leaf, F);
      for (int t = t0; t < t1; ++t) {
        const float4 A = tris[3 * (size_t)t], B = tris[3 * (size_t)t + 1], Cv = tris[3 * (size_t)t + 2];
        if (A.w != 0.f) {   // zero-area triangle: distance to its edges, never the sign
          const float d = fminf(fminf(scan_seg_d2(A, B, px, py, pz), scan_seg_d2(B, Cv, px, py, pz)), scan_seg_d2(Cv, A, px, py, pz));
          best = fminf(best, d);
        } else {
          int region;
          const float d = scan_tri_closest(A, B, Cv, px, py, pz, region);
          best = fminf(best, d);
          if (d < best_s) { best_s = d; best_t = t; }
        }
      }
    } else {
      const float dl = scan_box_d2(nodes, 2 * h, px, py, pz), dr = scan_box_d2(nodes, 2 * h + 1, px, py, pz);
      const bool r = dr < dl;
      const float dn = r ? dr : dl, df = r ? dl : dr;
      if (dn <= best_s) {   // a box is pruned only when it is farther than the best non-degenerate triangle
        const unsigned bit = 1u << depth;
        pend = df <= best_s ? (pend | bit) : (pend & ~bit);
        near_r = r ? (near_r | bit) : (near_r & ~bit);
        h = 2 * h + (r ? 1u : 0u);
        ++depth;
        descend = true;
      }
    }
    if (descend) continue;
    bool found = false;
    while (pend) {
      const int d = 31 - __clz(pend);
      pend &= ~(1u << d);
      const unsigned anc = h >> (depth - d);
      const unsigned far = 2 * anc + (((near_r >> d) & 1u) ? 0u : 1u);
      if (scan_box_d2(nodes, far, px, py, pz) <= best_s) {
        h = far;
        depth = d + 1;
        found = true;
        break;
      }
    }
    if (!found) break;
  }

  const float dist = sqrtf(best);
  float v = -dist;   // no non-degenerate triangle at all: free space
  if (best_t >= 0) {
    const float4 A = tris[3 * (size_t)best_t], B = tris[3 * (size_t)best_t + 1], Cv = tris[3 * (size_t)best_t + 2];
    int region;
    (void)scan_tri_closest(A, B, Cv, px, py, pz, region);
    // pseudo-normal table per triangle: face, edge ab / bc / ca, vertex a / b / c (3 floats each)
    const int slot = region == 0 ? 0 : (region >= 4 ? region - 3 : region + 3);
    const float* n = pn + (size_t)best_t * 21 + slot * 3;
    // the closest point: recomputed from the region so that the direction p - c matches the feature
    float qx, qy, qz;
    if (region == 1) { qx = A.x; qy = A.y; qz = A.z; }
    else if (region == 2) { qx = B.x; qy = B.y; qz = B.z; }
    else if (region == 3) { qx = Cv.x; qy = Cv.y; qz = Cv.z; }
    else { qx = A.x; qy = A.y; qz = A.z; }   // edges and the face: any point of the feature's plane / line gives the same sign
    float s;
    if (region >= 4) {
      const float4 P = region == 4 ? A : (region == 5 ? B : Cv), Q = region == 4 ? B : (region == 5 ? Cv : A);
      const float ex = Q.x - P.x, ey = Q.y - P.y, ez = Q.z - P.z;
      const float t = fminf(fmaxf(((px - P.x) * ex + (py - P.y) * ey + (pz - P.z) * ez) / fmaxf(ex * ex + ey * ey + ez * ez, 1e-30f), 0.f), 1.f);
      qx = P.x + t * ex; qy = P.y + t * ey; qz = P.z + t * ez;
    }
    s = (px - qx) * n[0] + (py - qy) * n[1] + (pz - qz) * n[2];
    v = s > 0.f ? -dist : dist;   // negative on the side the normals face (free space)
  }
  out[((size_t)i * d1 + j) * d2 + k] = v;
}

// ------------------------------------------------------------------------------------------------ walkable raster
constexpr int RASTER_CHUNK = 256;
constexpr int RASTER_REC = 24;   // floats per staged triangle (see the layout below)

__global__ __launch_bounds__(256) void egx_walkable_raster_kernel(const float* __restrict__ tris, int F, float ox, float oy, float cell,
                                                                 int nx, int ny, float floor_h, float floor_tol, float min_up_nz,
                                                                 float z_lo, float z_hi, int* __restrict__ support,
                                                                 float* __restrict__ clearance) {
  // staged record: [0..5] xy of the triangle, [6..8] z, [9] up-facing flag; [10..19] xy of the slab part (<= 5 vertices),
  // [20] vertex count of the slab part (0: outside the slab), [21] its signed area in xy
  __shared__ float s_r[RASTER_CHUNK * RASTER_REC];
  const int n = nx * ny;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int id = idx < n ? idx : n - 1;
  const int ci = id / ny, cj = id % ny;
  const float px = ox + (ci + 0.5f) * cell, py = oy + (cj + 0.5f) * cell;
  int sup = 0;
  float best = 3.4e38f;
  for (int f0 = 0; f0 < F; f0 += RASTER_CHUNK) {
    const int nf = min(RASTER_CHUNK, F - f0);
    __syncthreads();
    if ((int)threadIdx.x < nf) {
      const float* t = tris + (size_t)(f0 + threadIdx.x) * 9;
      float* r = s_r + threadIdx.x * RASTER_REC;
      float v[9];
#pragma unroll
      for (int e = 0; e < 9; ++e) v[e] = t[e];
      r[0] = v[0]; r[1] = v[1]; r[2] = v[3]; r[3] = v[4]; r[4] = v[6]; r[5] = v[7];
      r[6] = v[2]; r[7] = v[5]; r[8] = v[8];
      const float ux = v[3] - v[0], uy = v[4] - v[1], uz = v[5] - v[2], wx = v[6] - v[0], wy = v[7] - v[1], wz = v[8] - v[2];
      const float nxv = uy * wz - uz * wy, nyv = uz * wx - ux * wz, nzv = ux * wy - uy * wx;
      const float nn = sqrtf(nxv * nxv + nyv * nyv + nzv * nzv);
      const float zmin = fminf(fminf(v[2], v[5]), v[8]), zmax = fmaxf(fmaxf(v[2], v[5]), v[8]);
      r[9] = (nn > 0.f && nzv >= min_up_nz * nn && zmax >= floor_h - floor_tol && zmin <= floor_h + floor_tol) ? 1.f : 0.f;
      // Sutherland-Hodgman clip of the triangle to z_lo <= z <= z_hi: at most 5 vertices
      float ax[5], ay[5], az[5], bx[5], by[5], bz[5];
      int na = 3, nb = 0;
      ax[0] = v[0]; ay[0] = v[1]; az[0] = v[2]; ax[1] = v[3]; ay[1] = v[4]; az[1] = v[5]; ax[2] = v[6]; ay[2] = v[7]; az[2] = v[8];
      if (zmax < z_lo || zmin > z_hi) na = 0;
      for (int pass = 0; pass < 2 && na > 0; ++pass) {
        const float lim = pass == 0 ? z_lo : z_hi;
        const float sg = pass == 0 ? 1.f : -1.f;   // inside: sg * (z - lim) >= 0
        nb = 0;
        for (int e = 0; e < na; ++e) {
          const int e2 = e + 1 == na ? 0 : e + 1;
          const float sa = sg * (az[e] - lim), sb = sg * (az[e2] - lim);
          if (sa >= 0.f && nb < 5) { bx[nb] = ax[e]; by[nb] = ay[e]; bz[nb] = az[e]; ++nb; }
          if ((sa >= 0.f) != (sb >= 0.f) && sa != 0.f && sb != 0.f && nb < 5) {
            const float u = sa / (sa - sb);
            bx[nb] = ax[e] + u * (ax[e2] - ax[e]); by[nb] = ay[e] + u * (ay[e2] - ay[e]); bz[nb] = lim; ++nb;
          }
        }
        for (int e = 0; e < nb; ++e) { ax[e] = bx[e]; ay[e] = by[e]; az[e] = bz[e]; }
        na = nb;
      }
      float area = 0.f;
      for (int e = 0; e < 5; ++e) {
        const int src = e < na ? e : 0;
        r[10 + 2 * e] = ax[src];
        r[11 + 2 * e] = ay[src];
      }
      for (int e = 0; e < na; ++e) {
        const int e2 = e + 1 == na ? 0 : e + 1;
        area += ax[e] * ay[e2] - ax[e2] * ay[e];
      }
      r[20] = (float)na;
      r[21] = area;
    }
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
      const float* r = s_r + f * RASTER_REC;
      if (r[9] != 0.f && !sup) {
        // covered in xy (inclusive, either orientation) and the triangle's height there within the floor tolerance
        const float e0 = (r[2] - r[0]) * (py - r[1]) - (r[3] - r[1]) * (px - r[0]);
        const float e1 = (r[4] - r[2]) * (py - r[3]) - (r[5] - r[3]) * (px - r[2]);
        const float e2 = (r[0] - r[4]) * (py - r[5]) - (r[1] - r[5]) * (px - r[4]);
        const float a2 = e0 + e1 + e2;
        if (a2 != 0.f && ((e0 >= 0.f && e1 >= 0.f && e2 >= 0.f) || (e0 <= 0.f && e1 <= 0.f && e2 <= 0.f))) {
          const float z = (e1 * r[6] + e2 * r[7] + e0 * r[8]) / a2;
          if (fabsf(z - floor_h) <= floor_tol) sup = 1;
        }
      }
      const int m = (int)r[20];
      if (m > 0) {
        float d2 = 3.4e38f;
        bool inside = r[21] != 0.f;
        for (int e = 0; e < m; ++e) {
          const int e2 = e + 1 == m ? 0 : e + 1;
          const float qx = r[10 + 2 * e], qy = r[11 + 2 * e], ex = r[10 + 2 * e2] - qx, ey = r[11 + 2 * e2] - qy;
          const float L = fmaxf(ex * ex + ey * ey, 1e-30f);
          const float t = fminf(fmaxf(((px - qx) * ex + (py - qy) * ey) / L, 0.f), 1.f);
          const float dx = qx + t * ex - px, dy = qy + t * ey - py;
          d2 = fminf(d2, dx * dx + dy * dy);
          const float side = ex * (py - qy) - ey * (px - qx);
          inside = inside && (r[21] > 0.f ? side >= 0.f : side <= 0.f);
        }
        best = fminf(best, inside ? 0.f : d2);
      }
    }
  }
  if (idx < n) {
    support[idx] = sup;
    clearance[idx] = sqrtf(best);
  }
}
}  // namespace

extern "C" int egx_scan_sdf(const float* bvh_nodes, int bvh_levels, const float* triangles, const float* pseudo_normals, int num_triangles,
                            int leaf_size, const float* center_host, float scale, int d0, int d1, int d2, float* out_grid, void* stream_) {
  EGX_REQUIRE(bvh_nodes && triangles && pseudo_normals && center_host && out_grid && num_triangles > 0, "null tree / mesh / centre / grid");
  EGX_REQUIRE(bvh_levels >= 0 && bvh_levels <= 30 && leaf_size > 0 && ((int64_t)leaf_size << bvh_levels) >= num_triangles,
              "the tree's leaves (leaf_size << bvh_levels) must hold every triangle, depth <= 30");
  EGX_REQUIRE(scale > 0.f && egx_sdf_dims_ok(d0, d1, d2), "scale must be positive, the grid needs d2 >= 2 and fewer than 2^32 samples");
  const size_t bricks = (size_t)((d0 + 3) / 4) * ((d1 + 3) / 4) * ((d2 + 3) / 4);
  hipLaunchKernelGGL(egx_scan_sdf_kernel, dim3((unsigned)((bricks + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream_),
                     reinterpret_cast<const float4*>(bvh_nodes), bvh_levels, reinterpret_cast<const float4*>(triangles), pseudo_normals,
                     num_triangles, leaf_size, center_host[0], center_host[1], center_host[2], 1.f / scale, d0, d1, d2, out_grid);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

extern "C" int egx_walkable_raster(const float* triangles, int num_triangles, float origin_x, float origin_y, float cell, int nx, int ny,
                                   float floor_height, float floor_tol, float min_up_nz, float z_lo, float z_hi, int* out_support,
                                   float* out_clearance, void* stream_) {
  EGX_REQUIRE(triangles && out_support && out_clearance && num_triangles > 0, "null mesh / outputs");
  EGX_REQUIRE(cell > 0.f && nx > 0 && ny > 0 && (int64_t)nx * ny < (1ll << 31), "cell must be positive, 0 < nx * ny < 2^31");
  EGX_REQUIRE(z_lo <= z_hi && floor_tol >= 0.f, "z_lo <= z_hi, floor_tol >= 0");
  const int n = nx * ny;
  hipLaunchKernelGGL(egx_walkable_raster_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream_),
                     triangles, num_triangles, origin_x, origin_y, cell, nx, ny, floor_height, floor_tol, min_up_nz, z_lo, z_hi,
                     out_support, out_clearance);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

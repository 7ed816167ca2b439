// The SDF field of libegogen_hip.so in one place: the device descriptor of a grid, the layout of the tables behind it
// (egx_sdf_build_coarse, sdf.hip), the bracket lookups of the LBS count and the trilinear cell every evaluation of calc_sdf
// starts from - the sampler (sdf.hip), value / gradient / penalty (sdf_grad.hip) and the SDF epilogue of the fused LBS kernels
// (lbs_epilogue.h) - so that they give the same bits by construction.
#pragma once
#include "egx_common.h"

// Trilinear SDF lookup with torch.grid_sample semantics (align_corners=False, padding 'border'),
// NEGATED as crowd_ppo/utils.py:83-84 does.  Corner order / weight products follow
// aten GridSamplerKernel so that fp32 results match the CPU path to the last bits.
struct SdfDev {
  const float* grid;
  int d0, d1, d2;
  float cx, cy, cz, scale;
  const float2* coarse;  // optional padded bracket table [(c0+2)][(c1+2)][(c2+2)] {min,max} (egx_sdf_build_coarse)
  int c0, c1, c2;
};

// One scene of an SDF scene set (egx_sdf_scene_set, device table of 40-byte records): what the LBS count reads per body.  Every
// scene of a set has the grid dimensions of the launch's SdfDev; only the pointers, the map to voxels and the slope differ.
struct SdfSceneDev {
  const float* grid;
  const float2* coarse;   // bracket table (egx_sdf_build_coarse)
  float cx, cy, cz, scale;
  float slope;            // aux[3] of the table: steepest slope of the interpolated field (fix-up band of the mixed blend)
  float pad;
};
static_assert(sizeof(SdfSceneDev) == 40, "scene record");
__host__ __device__ inline SdfDev egx_sdf_scene(const SdfDev& dims, const SdfSceneDev& e) {
  SdfDev s = dims;
  s.grid = e.grid; s.coarse = e.coarse;
  s.cx = e.cx; s.cy = e.cy; s.cz = e.cz; s.scale = e.scale;
  return s;
}
// The opaque egx_sdf_scene_set of the header (made by egx_sdf_scene_set_create, sdf.hip; read by the LBS launcher and by
// the penalty calls of sdf_grad.hip).
struct egx_sdf_scene_set {
  int S = 0;
  egx_sdf_grid dims{};          // scene 0's descriptor: the grid dimensions every scene of the set shares
  SdfSceneDev* table = nullptr; // device [S]
};

// ---- the tables behind a grid (one buffer, every part 256-byte aligned): brackets, pyramid, aux floats, bricks ----

// Free-space pyramid behind the bracket table (same buffer, after the float2 entries, 256-byte aligned): level l = 1..4 holds,
// per block of 2^l x 2^l x 2^l PADDED bracket cells, the maximum of their `max` entries.  A box of padded cells whose pyramid
// entries are all < 0 contains only points whose interpolated value is < 0 (convexity of the interpolation), i.e. free space
// under the count's sign convention (a vertex counts when -trilinear < 0).  Used by the LBS work-item culling (lbs_cull.hip).
constexpr int EGX_SDF_MIP_LEVELS = 4;
__host__ __device__ inline int egx_sdf_mip_dim(int c, int l) { return ((c + 2) + (1 << l) - 1) >> l; }
__host__ __device__ inline size_t egx_sdf_mip_offset(int c0, int c1, int c2, int l) {   // in floats, from the start of the pyramid
  size_t off = 0;
  for (int k = 1; k < l; ++k) off += (size_t)egx_sdf_mip_dim(c0, k) * egx_sdf_mip_dim(c1, k) * egx_sdf_mip_dim(c2, k);
  return off;
}
__host__ __device__ inline size_t egx_sdf_table_bytes(int c0, int c1, int c2) {       // bracket table, padded to 256 bytes
  return ((size_t)(c0 + 2) * (c1 + 2) * (c2 + 2) * 8 + 255) / 256 * 256;
}

// After the pyramid (256-byte aligned): EGX_SDF_AUX_FLOATS floats written by egx_sdf_build_coarse -
//   [0..2] the largest |difference| of two neighbouring samples along x, y, z
//   [3]    the steepest slope of the interpolated field, value per metre of world space (sdf.hip: egx_sdf_axis_steps_kernel):
//          a position error bound times this is a bound on the change of the sampled value (fix-up of the mixed blend).
constexpr int EGX_SDF_AUX_FLOATS = 64;
__host__ __device__ inline size_t egx_sdf_aux_offset(int c0, int c1, int c2) {       // in bytes, from the start of the table
  return (egx_sdf_table_bytes(c0, c1, c2) + egx_sdf_mip_offset(c0, c1, c2, EGX_SDF_MIP_LEVELS + 1) * sizeof(float) + 255) / 256 * 256;
}

// After the aux floats (256-byte aligned): the grid again as 4 x 4 x 4 BRICKS of 256 contiguous bytes ([bx][by][bz][x & 3][y & 3][z & 3],
// samples past the grid's end repeat the last plane) for the gathers of calc_sdf outside the LBS kernels: the eight corners of a
// point then sit in 2.3 cache lines on average instead of four (egx_sdf_cell<true> below).
__host__ __device__ inline size_t egx_sdf_bricks_offset(int c0, int c1, int c2) {
  return (egx_sdf_aux_offset(c0, c1, c2) + EGX_SDF_AUX_FLOATS * sizeof(float) + 255) / 256 * 256;
}

// Host view of the tables of a grid d0 x d1 x d2 at `tables` (egx_sdf_grid::coarse_minmax; null: sizes only): the cell counts
// c = ceil(d / 4) and typed pointers to the parts.  Only egx_sdf_build_coarse writes through them.
struct EgxSdfTables {
  int c0, c1, c2;
  char* base;
  EgxSdfTables(int d0, int d1, int d2, const void* tables = nullptr)
      : c0(egx_ceil_div(d0, 4)), c1(egx_ceil_div(d1, 4)), c2(egx_ceil_div(d2, 4)), base(static_cast<char*>(const_cast<void*>(tables))) {}
  explicit EgxSdfTables(const egx_sdf_grid& g) : EgxSdfTables(g.d0, g.d1, g.d2, g.coarse_minmax) {}
  float2* brackets() const { return reinterpret_cast<float2*>(base); }
  float* mips() const { return reinterpret_cast<float*>(base + egx_sdf_table_bytes(c0, c1, c2)); }   // the pyramid, level 1 first
  float* mip(int l) const { return mips() + egx_sdf_mip_offset(c0, c1, c2, l); }
  float* aux() const { return reinterpret_cast<float*>(base + egx_sdf_aux_offset(c0, c1, c2)); }
  float* bricks() const { return reinterpret_cast<float*>(base + egx_sdf_bricks_offset(c0, c1, c2)); }
  size_t bytes() const { return egx_sdf_bricks_offset(c0, c1, c2) + (size_t)c0 * c1 * c2 * 64 * sizeof(float); }
};

inline bool egx_sdf_dims_ok(int d0, int d1, int d2) {
  return d2 >= 2 && (unsigned long long)d0 * (unsigned long long)d1 * (unsigned long long)d2 < (1ull << 32);
}
// what every call that evaluates the field asks of its descriptor (the trilinear cell below relies on it)
inline bool egx_sdf_grid_ok(const egx_sdf_grid* g) {
  return g && g->grid && g->d0 > 0 && g->d1 > 0 && g->d2 > 0 && egx_sdf_dims_ok(g->d0, g->d1, g->d2);
}

// The grid of a descriptor: dimensions, the map to voxels and, where egx_sdf_build_coarse has made its tables, their cell counts.
// What only one caller reads stays with it: the bracket table pointer (LBS launcher), the bricked copy (sdf.hip, sdf_grad.hip).
inline SdfDev egx_sdf_dev(const egx_sdf_grid& g) {
  SdfDev s{g.grid, g.d0, g.d1, g.d2, g.center[0], g.center[1], g.center[2], g.scale, nullptr, 0, 0, 0};
  if (g.coarse_minmax) { const EgxSdfTables t(g); s.c0 = t.c0; s.c1 = t.c1; s.c2 = t.c2; }
  return s;
}
// the bricked copy of a descriptor with tables, else null: gather from the row-major grid
inline const float* egx_sdf_bricks(const egx_sdf_grid& g) { return g.coarse_minmax ? EgxSdfTables(g).bricks() : nullptr; }

// ---- device side ----

// Continuous voxel coordinates of a world point, clamped to the grid (align_corners=False, padding "border").
// every operation rounds on its own (contraction off below), so the coordinates round exactly like the CPU path
__device__ __forceinline__ void egx_sdf_voxel_coords(const SdfDev& s, float x, float y, float z, float& px, float& py, float& pz) {
#pragma clang fp contract(off)   // __fmul_rn / __fadd_rn are plain * and + under hip-clang: without this the compiler fuses them
  const float nx = egx_mul(egx_sub(x, s.cx), s.scale), ny = egx_mul(egx_sub(y, s.cy), s.scale),
              nz = egx_mul(egx_sub(z, s.cz), s.scale);
  px = egx_mul(egx_sub(egx_mul(egx_add(nx, 1.f), (float)s.d0), 1.f), 0.5f);
  py = egx_mul(egx_sub(egx_mul(egx_add(ny, 1.f), (float)s.d1), 1.f), 0.5f);
  pz = egx_mul(egx_sub(egx_mul(egx_add(nz, 1.f), (float)s.d2), 1.f), 0.5f);
  px = fminf(fmaxf(px, 0.f), (float)(s.d0 - 1));
  py = fminf(fmaxf(py, 0.f), (float)(s.d1 - 1));
  pz = fminf(fmaxf(pz, 0.f), (float)(s.d2 - 1));
}

// {min,max} bracket of the samples the interpolation can touch for a point with UNCLAMPED voxel coordinates (rx,ry,rz):
// entry (jx,jy,jz) of the padded table built by egx_sdf_build_coarse (sdf.hip), j = clamp(floor(r / 4) + 1, 0, c + 1).
// A coordinate within round-off of a cell border may land in the neighbouring cell; both cells' footprints contain the
// samples such a point touches (block footprints include their border planes), so the bracket stays valid.
__device__ __forceinline__ float2 egx_sdf_coarse_at_raw(const SdfDev& s, float rx, float ry, float rz) {
  const float jx = __builtin_amdgcn_fmed3f(floorf(fmaf(rx, 0.25f, 1.f)), 0.f, (float)(s.c0 + 1));
  const float jy = __builtin_amdgcn_fmed3f(floorf(fmaf(ry, 0.25f, 1.f)), 0.f, (float)(s.c1 + 1));
  const float jz = __builtin_amdgcn_fmed3f(floorf(fmaf(rz, 0.25f, 1.f)), 0.f, (float)(s.c2 + 1));
  const unsigned idx = ((unsigned)jx * (unsigned)(s.c1 + 2) + (unsigned)jy) * (unsigned)(s.c2 + 2) + (unsigned)jz;
  return s.coarse[idx];
}

// The same lookup from CELL coordinates c = r / 4 + 1 (the caller folds the 1/4 and the +1 into its affine map).  The table
// index is formed in fp32 - exact while the padded table has fewer than 2^24 entries (a 256^3 grid: 66^3) - and converted
// once: two FMAs and one conversion instead of three conversions, two integer multiplies (quarter rate) and two adds.
__device__ __forceinline__ float2 egx_sdf_coarse_at_cell(const SdfDev& s, float cx, float cy, float cz) {
  const float jx = __builtin_amdgcn_fmed3f(floorf(cx), 0.f, (float)(s.c0 + 1));
  const float jy = __builtin_amdgcn_fmed3f(floorf(cy), 0.f, (float)(s.c1 + 1));
  const float jz = __builtin_amdgcn_fmed3f(floorf(cz), 0.f, (float)(s.c2 + 1));
  unsigned idx;
  if ((unsigned)(s.c0 + 2) * (unsigned)(s.c1 + 2) * (unsigned)(s.c2 + 2) < (1u << 24))   // uniform
    idx = (unsigned)fmaf(fmaf(jx, (float)(s.c1 + 2), jy), (float)(s.c2 + 2), jz);
  else
    idx = ((unsigned)jx * (unsigned)(s.c1 + 2) + (unsigned)jy) * (unsigned)(s.c2 + 2) + (unsigned)jz;
  return s.coarse[idx];
}

struct __attribute__((packed, aligned(4))) EgxF2 { float x, y; };  // two z-neighbours, 4-byte aligned

__device__ __forceinline__ float egx_sdf_brick_at(const float* __restrict__ bricks, unsigned nb1, unsigned nb2, unsigned x, unsigned y, unsigned z) {
  const unsigned b = ((x >> 2) * nb1 + (y >> 2)) * nb2 + (z >> 2);
  return bricks[(size_t)b * 64 + ((x & 3) << 4) + ((y & 3) << 2) + (z & 3)];
}

// The cell of one point at clamped voxel coordinates, aten grid_sampler_3d corner order and rounding: what the value, the
// gradient and the float64 value are all formed from.  Corner (i, j, k) is v{i}{j}0 for k = 0 and c{i}{j}y for k = 1; corners
// that fall off the grid have weight exactly 0 (aten drops them) and the value of a sample inside; on the last z plane the
// k = 0 corner is the plane's own sample (z1_in substitution).
struct EgxSdfCell {
  float x0, y0, z0;                          // floor of the coordinates
  bool x1_in, y1_in, z1_in;                  // the cell's upper neighbour along the axis is on the grid
  float wx0, wy0, wz0, wx1e, wy1e, wz1e;     // weights; the upper ones are 0 where the neighbour is off the grid
  float v000, c00y, v010, c01y, v100, c10y, v110, c11y;
  float a00, a01, a10, a11;                  // (x, y) weight products
};

// FROM_BRICKS: the corners come from the bricked copy (s.c1, s.c2 set), else from the row-major grid, where the two
// z-neighbours of each (x,y) corner column are one 8-byte load.  Same samples either way.  Requires d2 >= 2 and
// d0*d1*d2 < 2^32 (egx_sdf_grid_ok).
template <bool FROM_BRICKS>
__device__ __forceinline__ EgxSdfCell egx_sdf_cell(const SdfDev& s, const float* __restrict__ bricks, float px, float py, float pz) {
#pragma clang fp contract(off)
  const float x0 = floorf(px), y0 = floorf(py), z0 = floorf(pz);
  const float wx1 = egx_sub(px, x0), wy1 = egx_sub(py, y0), wz1 = egx_sub(pz, z0);
  const float wx0 = egx_sub(egx_add(x0, 1.f), px), wy0 = egx_sub(egx_add(y0, 1.f), py), wz0 = egx_sub(egx_add(z0, 1.f), pz);
  const unsigned ix0 = (unsigned)x0, iy0 = (unsigned)y0, iz0 = (unsigned)z0;
  const bool x1_in = ix0 + 1 < (unsigned)s.d0, y1_in = iy0 + 1 < (unsigned)s.d1, z1_in = iz0 + 1 < (unsigned)s.d2;
  const unsigned zb = z1_in ? iz0 : iz0 - 1;                      // pair (zb, zb+1) always inside the row
  float c00x, c00y, c01x, c01y, c10x, c10y, c11x, c11y;
  if (FROM_BRICKS) {
    const unsigned ix1 = x1_in ? ix0 + 1 : ix0, iy1 = y1_in ? iy0 + 1 : iy0;   // off-grid corners: weight exactly 0, any valid sample
    const unsigned nb1 = (unsigned)s.c1, nb2 = (unsigned)s.c2;
    c00x = egx_sdf_brick_at(bricks, nb1, nb2, ix0, iy0, zb); c00y = egx_sdf_brick_at(bricks, nb1, nb2, ix0, iy0, zb + 1);
    c01x = egx_sdf_brick_at(bricks, nb1, nb2, ix0, iy1, zb); c01y = egx_sdf_brick_at(bricks, nb1, nb2, ix0, iy1, zb + 1);
    c10x = egx_sdf_brick_at(bricks, nb1, nb2, ix1, iy0, zb); c10y = egx_sdf_brick_at(bricks, nb1, nb2, ix1, iy0, zb + 1);
    c11x = egx_sdf_brick_at(bricks, nb1, nb2, ix1, iy1, zb); c11y = egx_sdf_brick_at(bricks, nb1, nb2, ix1, iy1, zb + 1);
  } else {
    const unsigned i00 = (ix0 * (unsigned)s.d1 + iy0) * (unsigned)s.d2 + zb;
    const unsigned sy = y1_in ? (unsigned)s.d2 : 0u, sx = x1_in ? (unsigned)s.d1 * (unsigned)s.d2 : 0u;
    const EgxF2 c00 = *reinterpret_cast<const EgxF2*>(s.grid + i00), c01 = *reinterpret_cast<const EgxF2*>(s.grid + (i00 + sy)),
                c10 = *reinterpret_cast<const EgxF2*>(s.grid + (i00 + sx)), c11 = *reinterpret_cast<const EgxF2*>(s.grid + (i00 + sx + sy));
    c00x = c00.x; c00y = c00.y; c01x = c01.x; c01y = c01.y; c10x = c10.x; c10y = c10.y; c11x = c11.x; c11y = c11.y;
  }
  const float wx1e = x1_in ? wx1 : 0.f, wy1e = y1_in ? wy1 : 0.f, wz1e = z1_in ? wz1 : 0.f;
  const float v000 = z1_in ? c00x : c00y, v010 = z1_in ? c01x : c01y, v100 = z1_in ? c10x : c10y, v110 = z1_in ? c11x : c11y;
  const float a00 = egx_mul(wx0, wy0), a01 = egx_mul(wx0, wy1e), a10 = egx_mul(wx1e, wy0), a11 = egx_mul(wx1e, wy1e);
  return EgxSdfCell{x0, y0, z0, x1_in, y1_in, z1_in, wx0, wy0, wz0, wx1e, wy1e, wz1e, v000, c00y, v010, c01y, v100, c10y, v110, c11y,
                    a00, a01, a10, a11};
}

// -trilinear of a cell: products and sums round one by one, in the order of aten's kernel, in every kernel this is inlined into
__device__ __forceinline__ float egx_sdf_cell_neg_value(const EgxSdfCell& c) {
#pragma clang fp contract(off)
  float acc;
  acc = egx_mul(c.v000, egx_mul(c.a00, c.wz0));
  acc = egx_add(acc, egx_mul(c.c00y, egx_mul(c.a00, c.wz1e)));
  acc = egx_add(acc, egx_mul(c.v010, egx_mul(c.a01, c.wz0)));
  acc = egx_add(acc, egx_mul(c.c01y, egx_mul(c.a01, c.wz1e)));
  acc = egx_add(acc, egx_mul(c.v100, egx_mul(c.a10, c.wz0)));
  acc = egx_add(acc, egx_mul(c.c10y, egx_mul(c.a10, c.wz1e)));
  acc = egx_add(acc, egx_mul(c.v110, egx_mul(c.a11, c.wz0)));
  acc = egx_add(acc, egx_mul(c.c11y, egx_mul(c.a11, c.wz1e)));
  return -acc;
}

// -trilinear(grid) at clamped voxel coordinates, from the row-major grid (the LBS kernels)
__device__ __forceinline__ float egx_sdf_neg_trilinear_at(const SdfDev& s, float px, float py, float pz) {
  return egx_sdf_cell_neg_value(egx_sdf_cell<false>(s, nullptr, px, py, pz));
}

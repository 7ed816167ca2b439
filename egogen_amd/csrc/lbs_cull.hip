// ------------------------------------------------------------------------------------------------
// Free-space culling of the SDF work items (training path: split blend modes, picks + penetration counts, no vertex output).
//
// The penetration count needs EVERY vertex of every body (crowd_env_2f.py:165-175), which is what makes the blend GEMM the
// dominant cost - but a vertex can only count where the scene has geometry.  A posed vertex lies in the convex hull of balls
// around the posed joints it is bound to (radii bounded per tile at load, egx_body_model_create), so a (vertex tile, body)
// pair whose hull's bounding box - mapped to voxel coordinates - only covers cells of the free-space pyramid with max < 0
// cannot contribute to the count: trilinear interpolation is a convex combination of the samples a cell's bracket covers.
// A work item (tile x 256 bodies) all of whose bodies pass that test is skipped ENTIRELY (GEMM, skinning, SDF) unless the tile
// holds picked vertices.  The result is bit-identical to the unculled launch (tests/test_lbs_gpu.py); what changes is how much
// of the scene-independent work is done.  Three small launches in front of the fused kernel:
//   egx_lbs_agent_order_kernel  agents whose neighbourhood is free first: bodies near geometry share body groups
//   egx_lbs_cull_kernel         the test per (tile, body), OR-reduced per item
//   egx_lbs_compact_kernel      per-XCD item lists (non-picked tiles dealt by tile chunk: an XCD streams an eighth of the bases)
// ------------------------------------------------------------------------------------------------
#include "egx_sdf.h"
#include "lbs.h"

namespace {
constexpr int CULL_TILES_PER_BLOCK = 16;
constexpr float CULL_SLACK_M = 2e-3f;        // metres added to every radius: covers the fp32 / bf16x2 evaluation of the vertex
constexpr float CULL_SLACK_VOX = 0.02f;      // voxels added to the box: covers the rounding of the affine map

// raw (unclamped) voxel-coordinate box [lo, hi] -> true if every point in it interpolates to a value < 0 (free space)
__device__ __forceinline__ bool cull_box_free(const SdfDev& s, const float* __restrict__ mips, const float (&lo)[3], const float (&hi)[3]) {
  if (!(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) return false;   // NaN / inverted: not provable
  const int cdim[3] = {s.c0, s.c1, s.c2};
  int jl[3], jh[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    jl[a] = (int)__builtin_amdgcn_fmed3f(floorf(fmaf(lo[a], 0.25f, 1.f)), 0.f, (float)(cdim[a] + 1));
    jh[a] = (int)__builtin_amdgcn_fmed3f(floorf(fmaf(hi[a], 0.25f, 1.f)), 0.f, (float)(cdim[a] + 1));
  }
  for (int l = 0; l <= EGX_SDF_MIP_LEVELS; ++l) {
    if ((jh[0] >> l) - (jl[0] >> l) > 1 || (jh[1] >> l) - (jl[1] >> l) > 1 || (jh[2] >> l) - (jl[2] >> l) > 1) continue;
    const int e1 = l == 0 ? s.c1 + 2 : egx_sdf_mip_dim(s.c1, l), e2 = l == 0 ? s.c2 + 2 : egx_sdf_mip_dim(s.c2, l);
    const float* mp = l == 0 ? nullptr : mips + egx_sdf_mip_offset(s.c0, s.c1, s.c2, l);
    float mx = -3.4e38f;
    for (int x = jl[0] >> l; x <= jh[0] >> l; ++x)
      for (int y = jl[1] >> l; y <= jh[1] >> l; ++y)
        for (int z = jl[2] >> l; z <= jh[2] >> l; ++z) {
          const size_t idx = ((size_t)x * e1 + y) * e2 + z;
          mx = fmaxf(mx, l == 0 ? s.coarse[idx].y : mp[idx]);
        }
    return mx < 0.f;
  }
  return false;   // larger than two cells of the coarsest level
}

// canonical frame -> raw voxel coordinates of an agent: r = Mw x + tw (the affine map of the SDF epilogue)
__device__ __forceinline__ void cull_agent_map(const SdfDev& s, const float* R0, const float* T0, int ag, float (&Mw)[9], float (&tw)[3], float (&kk)[3]) {
  kk[0] = s.scale * (float)s.d0 * 0.5f; kk[1] = s.scale * (float)s.d1 * 0.5f; kk[2] = s.scale * (float)s.d2 * 0.5f;
  const float cc[3] = {s.cx, s.cy, s.cz};
  const float dd[3] = {(float)s.d0, (float)s.d1, (float)s.d2};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int e = 0; e < 3; ++e) Mw[a * 3 + e] = kk[a] * (R0 ? R0[(size_t)ag * 9 + a * 3 + e] : ((a == e) ? 1.f : 0.f));
    tw[a] = kk[a] * ((T0 ? T0[(size_t)ag * 3 + a] : 0.f) - cc[a]) + (dd[a] - 1.f) * 0.5f;
  }
}

// One block.  (1) clears the item flags and counters of this launch; (2) classifies every agent: "far" = the 1 m cube around
// the pelvis of its first and last frame is free space; (3) slot order = far agents, then near agents (stable).
__global__ __launch_bounds__(256) void egx_lbs_agent_order_kernel(const float* __restrict__ xb, const float* __restrict__ R0,
                                                                  const float* __restrict__ T0, SdfDev sdf, const float* __restrict__ mips,
                                                                  int A, int fpa, float px, float py, float pz,
                                                                  int* __restrict__ agent_of_slot, int* __restrict__ flags, int n_flags,
                                                                  int* __restrict__ counts) {
  extern __shared__ int s_key[];   // [A]
  const int tid = threadIdx.x;
  for (int i = tid; i < n_flags; i += 256) flags[i] = 0;
  if (tid < 16) counts[tid] = tid == 15 ? 0x43554c4c : 0;   // [15]: marks the workspace as holding a culled launch's counters
  for (int a = tid; a < A; a += 256) {
    float Mw[9], tw[3], kk[3];
    cull_agent_map(sdf, R0, T0, a, Mw, tw, kk);
    bool far = true;
    for (int f = 0; f < fpa; f += max(1, fpa - 1)) {   // first and last frame
      const float* x = xb + ((size_t)a * fpa + f) * EGX_XB_DIM;
      const float c[3] = {x[0] + px, x[1] + py, x[2] + pz};
      float lo[3], hi[3];
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) {
        const float r = fmaf(Mw[ax * 3 + 0], c[0], fmaf(Mw[ax * 3 + 1], c[1], fmaf(Mw[ax * 3 + 2], c[2], tw[ax])));
        lo[ax] = r - 1.0f * kk[ax]; hi[ax] = r + 1.0f * kk[ax];
      }
      far = far && cull_box_free(sdf, mips, lo, hi);
    }
    s_key[a] = far ? 0 : 1;
  }
  __syncthreads();
  if (tid < 64) {   // stable partition by one wave: 64 agents per step
    int base = 0;
    for (int pass = 0; pass < 2; ++pass)
      for (int a0 = 0; a0 < A; a0 += 64) {
        const int a = a0 + tid;
        const bool mine = a < A && s_key[a] == pass;
        const unsigned long long bm = __ballot(mine);
        if (mine) agent_of_slot[base + __builtin_amdgcn_mbcnt_hi((unsigned)(bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bm, 0u))] = a;
        base += __popcll(bm);
      }
  }
}

// grid (nbg, tile chunks), 256 threads = the 256 slots of a body group.  flags[ti * nbg + bg] = 1 where some body of the
// group cannot be proven clear of geometry for tile ti of the launch's tile list (ti >= first_tile: the picked tiles in
// front are always evaluated).
__global__ __launch_bounds__(256) void egx_lbs_cull_kernel(const int* __restrict__ tiles, int first_tile, int n_tiles,
                                                           const int* __restrict__ tj_off, const int* __restrict__ tj_idx,
                                                           const float* __restrict__ D0, const float* __restrict__ E,
                                                           const float* __restrict__ fvec, const float* __restrict__ jpos, int Bp,
                                                           const int* __restrict__ agent_of_slot, int B, int fpa, int nbg,
                                                           const float* __restrict__ R0, const float* __restrict__ T0, SdfDev sdf,
                                                           const float* __restrict__ mips, int* __restrict__ flags) {
  const int bg = blockIdx.x, tid = threadIdx.x;
  const int slot = bg * 256 + tid;
  const bool valid = slot < B;
  const int ss = valid ? slot : B - 1;
  const int body = agent_of_slot ? agent_of_slot[ss / fpa] * fpa + ss % fpa : ss;
  float Mw[9], tw[3], kk[3];
  cull_agent_map(sdf, R0, T0, body / fpa, Mw, tw, kk);
  float f[61];
#pragma unroll
  for (int i = 0; i < 61; ++i) f[i] = fvec[(size_t)i * Bp + ss];
  const int t_lo = first_tile + blockIdx.y * CULL_TILES_PER_BLOCK, t_hi = min(n_tiles, t_lo + CULL_TILES_PER_BLOCK);
  for (int ti = t_lo; ti < t_hi; ++ti) {
    const int vt = __builtin_amdgcn_readfirstlane(tiles ? tiles[ti] : ti);   // uniform: the tables below are read with scalar loads
    const float* Et = E + (size_t)vt * 64;
    float margin = CULL_SLACK_M;
#pragma unroll
    for (int i = 0; i < 61; ++i) margin = fmaf(f[i], Et[i], margin);
    float lo[3] = {3.4e38f, 3.4e38f, 3.4e38f}, hi[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
    const int jj_lo = __builtin_amdgcn_readfirstlane(tj_off[vt]), jj_hi = __builtin_amdgcn_readfirstlane(tj_off[vt + 1]);
    for (int jj = jj_lo; jj < jj_hi; ++jj) {
      const int j = __builtin_amdgcn_readfirstlane(tj_idx[jj]) & 0xff;
      const float rho = (D0[jj] + margin) * 1.0001f;
      const float c0 = jpos[(size_t)(j * 3 + 0) * Bp + ss], c1 = jpos[(size_t)(j * 3 + 1) * Bp + ss], c2 = jpos[(size_t)(j * 3 + 2) * Bp + ss];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float r = fmaf(Mw[a * 3 + 0], c0, fmaf(Mw[a * 3 + 1], c1, fmaf(Mw[a * 3 + 2], c2, tw[a])));
        const float ext = rho * kk[a] + CULL_SLACK_VOX + 1e-5f * fabsf(r);
        lo[a] = fminf(lo[a], r - ext); hi[a] = fmaxf(hi[a], r + ext);
      }
    }
    const bool active = valid && !cull_box_free(sdf, mips, lo, hi);
    if (__ballot(active) != 0ull && (tid & 63) == 0) flags[(size_t)ti * nbg + bg] = 1;
  }
}

// 8 blocks of one wave: block x builds the item list of XCD x.  Picked tiles (ti < first_tile, always active) go to XCD
// bg % 8; the other tiles are dealt round-robin (an XCD streams only an eighth of the bases), in the order
// "block of bg_block body groups, tile, group of the block" so that the features of a block stay in the XCD's L2.
__global__ __launch_bounds__(64) void egx_lbs_compact_kernel(const int* __restrict__ flags, int first_tile, int n_tiles, int nbg, int bg_block,
                                                             int* __restrict__ items, int items_stride, int* __restrict__ counts) {
  const int x = blockIdx.x, lane = threadIdx.x;
  int* list = items + (size_t)x * items_stride;
  int n = 0;
  auto append = [&](bool on, int code) {
    const unsigned long long bm = __ballot(on);
    if (on) list[n + __builtin_amdgcn_mbcnt_hi((unsigned)(bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bm, 0u))] = code;
    n += __popcll(bm);
  };
  const int n_mine = (nbg - x + 7) / 8;   // body groups x, x + 8, ...
  for (int i0 = 0; i0 < n_mine * first_tile; i0 += 64) {
    const int i = i0 + lane;
    const bool on = i < n_mine * first_tile;
    const int bg = x + 8 * (on ? i / first_tile : 0), ti = on ? i % first_tile : 0;
    append(on, ti * nbg + bg);
  }
  // tiles first_tile + x, + 8, ...: the active tiles of standing bodies are neighbours in the joint-sorted tile order (the
  // legs), so contiguous chunks would leave most XCDs idle
  const int n_np = n_tiles - first_tile;
  const int t_n = max(0, (n_np - x + 7) / 8);
  const int PB = max(1, bg_block), n_blk = (nbg + PB - 1) / PB;
  const int total = n_blk * t_n * PB;
  for (int i0 = 0; i0 < total; i0 += 64) {
    const int i = i0 + lane;
    bool on = i < total;
    const int blk = on ? i / (t_n * PB) : 0, r = on ? i % (t_n * PB) : 0;
    const int ti = first_tile + x + 8 * (r / PB), bg = blk * PB + r % PB;
    on = on && bg < nbg && flags[(size_t)ti * nbg + bg] != 0;
    append(on, ti * nbg + bg);
  }
  if (lane == 0) { counts[x] = n; atomicAdd(&counts[8], n); }
}
}  // namespace

void lbs_launch_cull_order(const egx_body_model* m, const float* xb, const float* R0, const float* T0, const SdfDev& sd, const float* mips,
                           int B, int fpa, int nbg_all, int* order, int* flags, int* counts, hipStream_t stream) {
  const int A = B / fpa;
  // rest pelvis of the mean shape: the classification of an agent only steers the slot order, it decides nothing
  const float* pel = m->rest_pelvis;
  hipLaunchKernelGGL(egx_lbs_agent_order_kernel, dim3(1), dim3(256), (size_t)A * sizeof(int), stream, xb, R0, T0, sd, mips, A, fpa,
                     pel[0], pel[1], pel[2], order, flags, m->n_sdf_tiles * nbg_all, counts);
}

void lbs_launch_cull_items(const egx_body_model* m, const float* fvec, const float* jpos, int Bp, const int* order, int B, int fpa,
                           int nbg_all, const float* R0, const float* T0, const SdfDev& sd, const float* mips, int* flags, int* items,
                           int items_stride, int* counts, hipStream_t stream) {
  const int n_np = m->n_sdf_tiles - m->n_pick_tiles;
  hipLaunchKernelGGL(egx_lbs_cull_kernel, dim3(nbg_all, egx_ceil_div(n_np, CULL_TILES_PER_BLOCK)), dim3(256), 0, stream, m->sdf_tiles,
                     m->n_pick_tiles, m->n_sdf_tiles, m->tj_off, m->tj_idx, m->cull_D0, m->cull_E, fvec, jpos, Bp,
                     static_cast<const int*>(order), B, fpa, nbg_all, R0, T0, sd, mips, flags);
  hipLaunchKernelGGL(egx_lbs_compact_kernel, dim3(8), dim3(64), 0, stream, flags, m->n_pick_tiles, m->n_sdf_tiles, nbg_all, 2, items,
                     items_stride, counts);
}

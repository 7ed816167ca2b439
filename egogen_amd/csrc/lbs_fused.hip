// ------------------------------------------------------------------------------------------------
// kernel 2: fused blend GEMM + skinning + (SDF count) + (vertex picks) + (vertex write)
// ------------------------------------------------------------------------------------------------
#include <algorithm>

#include "lbs_epilogue.h"

// fp32 blend GEMM of one work item on v_mfma_f32_32x32x2_f32: acc = [v_template | bases] x [1 | features]
__device__ __forceinline__ void lbs_blend_f32(const LbsParams& p, f32x16 (&acc)[3][LBS_NB], int vt, int bt0, int lane) {
  constexpr int NB = LBS_NB;
  const f32x4* dp = p.dirs + (size_t)vt * KGROUPS * 3 * 64 + lane;
  const f32x4* fp[NB];
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    const int ls = lbs_live_slot(bt0 + q, lane & 31, p.B);
    fp[q] = p.feat + (size_t)(ls >> 5) * KGROUPS * 64 + (lane & 32) + (ls & 31);
  }

  // Operand bursts.  Measured on gfx950 (scripts/ubench/mfma_loads.hip): a wave that issues v_mfma_f32_32x32x2_f32
  // while its own global loads are still in flight runs the matrix pipe at about half rate (72 vs 136 TFLOP/s
  // chip-wide for this exact loop), whereas "load a burst, s_waitcnt vmcnt(0), then only MFMAs" keeps 98 % of the
  // load-free rate - the exposed load latency is covered by the other wave of the SIMD, whose MFMAs are not affected
  // by this wave's returning data.  So: no software prefetch; LBS_BURST k-groups of operands per burst.
  constexpr int LBS_BURST = 2;
  if (!(p.dbg & 2)) {
    f32x4 a_st[LBS_BURST][3], b_st[LBS_BURST][NB];
    constexpr int KMAIN = KGROUPS / LBS_BURST * LBS_BURST;
    for (int g0 = 0; g0 < KMAIN; g0 += LBS_BURST) {
#pragma unroll
      for (int u = 0; u < LBS_BURST; ++u) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a_st[u][c] = dp[((g0 + u) * 3 + c) * 64];
#pragma unroll
        for (int q = 0; q < NB; ++q) b_st[u][q] = fp[q][(g0 + u) * 64];
      }
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < LBS_BURST; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int q = 0; q < NB; ++q)
              acc[c][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_st[u][c][e], b_st[u][q][e], acc[c][q], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int g = KMAIN; g < KGROUPS; ++g) {  // tail groups, one at a time
#pragma unroll
      for (int c = 0; c < 3; ++c) a_st[0][c] = dp[(g * 3 + c) * 64];
#pragma unroll
      for (int q = 0; q < NB; ++q) b_st[0][q] = fp[q][g * 64];
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int q = 0; q < NB; ++q)
            acc[c][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_st[0][c][e], b_st[0][q][e], acc[c][q], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

}

// fp32-MFMA variant (blend mode 0 and every vertex-writing call): persistent workgroups, one per CU, eight waves = two
// SETS of four waves; each set walks its own stream of work items (vertex tile x 256 bodies: 4 waves x 64 bodies), so
// one wave of a SIMD can wait for its operand burst while the other issues MFMAs.  Nothing synchronises across waves
// (per-wave LDS metadata, no barriers).  The fp32 MFMA shares the fp32 VALU lanes (scripts/ubench/mfma_valu.hip), so here
// the epilogue's VALU work adds to the MFMA time whatever the relative phase of the two sets (a phase offset between
// them was tried and changes nothing).
// MS: scene-set launch (egx_lbs_forward_scenes) - every read of scene data uses the body's own scene
template <bool WRITE_VERTS, bool DO_SDF, bool MS = false>
__global__ __launch_bounds__(LBS_THREADS, 1) void egx_lbs_fused_kernel(LbsParams p) {
  constexpr int NB = LBS_NB;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int set = wave >> 2, w4 = wave & 3;  // two independent sets of four waves, each walking its own item stream
  char* my = smem_raw + wave * (LBS_META_BYTES + (WRITE_VERTS ? LBS_VERT_BYTES : (DO_SDF ? LBS_QCAP * 16 : 0)));
  LbsWave w = lbs_wave_init<WRITE_VERTS, DO_SDF>(my, lane);
  // work streams.  With >= 8 body groups every XCD (block id % 8) owns a contiguous chunk of body groups, so their packed
  // features / transforms stay in that XCD's L2 while the blend bases stream through once per XCD; the streams of an XCD
  // walk its (vertex tile, body group) list vertex-tile-major, i.e. at any time they share a dozen consecutive tiles.
  int bg_lo, nper, n_streams, stream;
  if (p.nbg >= 8 && (gridDim.x & 7) == 0) {
    const int per = (p.nbg + 7) / 8, xcd = blockIdx.x & 7;
    bg_lo = xcd * per;
    nper = max(0, min(per, p.nbg - bg_lo));
    n_streams = (gridDim.x >> 3) * 2;
    stream = (blockIdx.x >> 3) * 2 + set;
  } else {
    bg_lo = 0; nper = p.nbg;
    n_streams = gridDim.x * 2;
    stream = blockIdx.x * 2 + set;
  }
  const int n_items = p.n_tiles * nper;
  for (int item = stream; item < n_items; item += n_streams) {
    const int vti = item / nper, bg = bg_lo + item % nper;
    const int vt = p.tiles ? p.tiles[vti] : vti;
    const int bt0 = bg * 8 + w4 * NB;  // first 32-body tile of this wave
    const int JT = lbs_load_meta(p, w, vt);
    f32x16 acc[3][NB];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int q = 0; q < NB; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][q][r] = 0.f;
    if (!(p.dbg & 2)) lbs_blend_f32(p, acc, vt, bt0, lane);
    if (p.dbg & 1) {
      float sum = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int q = 0; q < NB; ++q)
#pragma unroll
          for (int r = 0; r < 16; ++r) sum += acc[c][q][r];
      if (sum == 123.456f) p.pene[0] = 1;
      continue;
    }
    lbs_epilogue<WRITE_VERTS, DO_SDF, 8, LBS_QCAP, LBS_NB, false, MS>(p, w, acc, vt, bt0, JT);
  }
}

// One table for both the instantiations whose dynamic-LDS cap is raised and the ones that can be launched.
int lbs_launch_fused(const LbsParams& p, bool do_sdf, bool ms, hipStream_t stream) {
  constexpr size_t lds_meta = (size_t)8 * LBS_META_BYTES, lds_verts = (size_t)8 * (LBS_META_BYTES + LBS_VERT_BYTES),
                   lds_sdf = (size_t)8 * (LBS_META_BYTES + LBS_QCAP * 16);
  static const struct { void (*fn)(LbsParams); bool verts, sdf, ms; size_t lds; } variants[] = {
      {egx_lbs_fused_kernel<true, true>, true, true, false, lds_verts},         {egx_lbs_fused_kernel<true, false>, true, false, false, lds_verts},
      {egx_lbs_fused_kernel<false, true>, false, true, false, lds_sdf},         {egx_lbs_fused_kernel<false, false>, false, false, false, lds_meta},
      {egx_lbs_fused_kernel<true, true, true>, true, true, true, lds_verts},    {egx_lbs_fused_kernel<false, true, true>, false, true, true, lds_sdf},
  };
  // one persistent workgroup per CU; per-device launch facts (CU count, raised dynamic-LDS caps) are set up once per device
  static LbsDeviceInfo devs[kMaxDevices];
  int num_cu = 0;
  auto raise_caps = [&]() -> int {
    for (const auto& v : variants)
      EGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(v.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.lds));
    return EGX_OK;
  };
  if (int rc = lbs_device_cus(devs, raise_caps, &num_cu)) return rc;
  const int n_items = p.nbg * p.n_tiles;
  const int grid = std::max(1, std::min(num_cu, (n_items + 1) / 2));
  for (const auto& v : variants)
    if (v.verts == (p.verts != nullptr) && v.sdf == do_sdf && v.ms == ms) {
      hipLaunchKernelGGL(v.fn, dim3(grid), dim3(LBS_THREADS), v.lds, stream, p);
      return EGX_OK;
    }
  egx_set_error("no fp32 fused LBS kernel for this call");
  return EGX_ERR_ARG;
}

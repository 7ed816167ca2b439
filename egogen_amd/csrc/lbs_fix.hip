// The fix-up queue of a mixed-blend launch (lbs_fix_process): one wave per queued vertex, re-evaluated in fp32 and counted.
#include "lbs_epilogue.h"

constexpr int LBS_FIX_BLOCKS = 1024;
static_assert((LBS_FIX_BLOCKS * 4) % LBS_FIX_NQ == 0, "waves of the fix-up kernel per sub-queue");
template <bool MS>
__global__ __launch_bounds__(256) void egx_lbs_fix_kernel(LbsParams p) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = gridDim.x * 4;
  const int sq = wave % LBS_FIX_NQ;   // n_waves is a multiple of LBS_FIX_NQ: a wave stays with one sub-queue
  const int count = min(p.fix_stats[LBS_FIX_CNT0 + 32 * sq], p.fixq_cap);
  for (int i = wave / LBS_FIX_NQ; i < count; i += n_waves / LBS_FIX_NQ) {
    const int2 e = p.fixq[(size_t)sq * p.fixq_cap + i];
    if (e.x < 0) continue;   // wave-uniform
    const int vt = e.x >> 5, row = e.x & 31, slot = e.y;
    const int j_lo = p.tj_off[vt], JT = p.tj_off[vt + 1] - j_lo;
    const float sv = lbs_fix_one<true, MS>(p, lane, vt, row, slot, JT, p.tj_idx + j_lo, p.tj_w + (size_t)j_lo * 32);
    if (lane == 0 && sv < 0.f) {
      const int body = p.agent_of_slot ? p.agent_of_slot[slot / p.fpa] * p.fpa + slot % p.fpa : slot;
      atomicAdd(p.pene + body, 1);
    }
  }
}

void lbs_launch_fix(const LbsParams& p, bool ms, hipStream_t stream) {
  hipLaunchKernelGGL(ms ? egx_lbs_fix_kernel<true> : egx_lbs_fix_kernel<false>, dim3(LBS_FIX_BLOCKS), dim3(256), 0, stream, p);
}

// The GRU cell of the dense3 scheme (d3.h): both products, the gate math and the packed images of h in one launch.
#include <cstddef>
#include "d3.h"

// ---------------------------------------------------------------------------------------------------------
// GRU cell (torch.nn.GRU / GRUCell, gate order r, z, n) in one launch: workgroup = 32 rows x 16 hidden columns of all
// three gates on both sides,
//   gi = gi_in + Ai Bi^T + bias_i      (stored to gi_out when asked: the decoder keeps it as a running sum, prior.hip)
//   gh = Ah Bh^T + bias_h              (Ah null: zero previous state, gh = bias_h)
//   r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r gh_n), h = (1 - z) n + z h_prev
// h is written fp32 row-major (the next cell's h_prev) and packed (the next products' A operand).
// ---------------------------------------------------------------------------------------------------------
struct D3Gru2 {
  D3Gru g0, g1;
  int blocks0;   // blocks [0, blocks0) work on g0, the rest on g1 (the policy's two encoders)
  int rowmap;
};
static_assert(offsetof(D3Gru2, g0) == 0 && offsetof(D3Gru2, g1) == sizeof(D3Gru), "layout");
template <int TRIP, int NPL>
__global__ __launch_bounds__(512) void egx_gru3_kernel(D3Gru2 two) {
  // eight waves: waves 0-3 split the reduction of the x side (x W_ih^T), waves 4-7 that of the h side (h W_hh^T) - the two
  // products are independent, so their operand bursts are in flight together and a cell whose sides are each <= 4 TRIP
  // k-steps deep (the decoder cell: 8 + 8) is ONE memory round trip instead of two
  const bool second = (int)blockIdx.x >= two.blocks0;
  const D3Gru a = d3_kernarg<D3Gru>(second ? 1 : 0);   // all fields in SGPRs from the start: no scalar load in the epilogue
  const int gru_bid = second ? (int)blockIdx.x - two.blocks0 : (int)blockIdx.x;
  extern __shared__ __attribute__((aligned(16))) float gsm[];
  float* red = gsm;                  // [8 waves][24][64]
  float* tile = gsm + 8 * 24 * 64;   // [32][20]: h of this workgroup's 32 x 16 block
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int MT = (a.M + 31) >> 5, CT = a.H >> 4;
  int mt, ct;
  if (!d3_tile(gru_bid, MT, CT, mt, ct, d3_rowmap(two.rowmap, a.M, 3 * a.H))) return;
  const int sd = wave >> 2, w4 = wave & 3;
  // The element this lane finishes after the reduction - wave w takes position (mi, r) = (w >> 2, w & 3) of every lane - is
  // known from the start, and so is everything its gate math reads from memory: gi_in and both biases of the three gates, and
  // h_prev.  They are requested as ONE batch (ten loads in flight, one round trip) on a wait the kernel pays anyway: ahead of
  // the k-loop, where they come back with the first operand burst, when the registers allow it (three planes: 1 workgroup per
  // CU either way), else between the partial sums' LDS writes and the barrier (no register lives through the loop: the
  // two-plane and one-plane kernels keep their 2 workgroups per CU).  Rows >= M load nothing.
  constexpr bool EARLY = NPL == 3;
  const int e_mi = wave >> 2, e_r = wave & 3;
  const int e_col = lane & 15, e_c = ct * 16 + e_col;
  const int e_row = 16 * e_mi + 4 * (lane >> 4) + e_r, e_m = mt * 32 + e_row;
  float pre_gi[3] = {0.f, 0.f, 0.f}, pre_bi[3] = {0.f, 0.f, 0.f}, pre_bh[3] = {0.f, 0.f, 0.f}, pre_hp = 0.f;
  auto prefetch = [&]() __attribute__((always_inline)) {
    if (e_m >= a.M) return;
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const int n = g * a.H + e_c;
      if (a.gi_in) pre_gi[g] = d3_g(a.gi_in)[(size_t)e_m * 3 * a.H + n];
      if (a.bias_i) pre_bi[g] = d3_g(a.bias_i)[n];
      pre_bh[g] = d3_g(a.bias_h)[n];
    }
    if (a.h_prev) pre_hp = d3_g(a.h_prev)[(size_t)e_m * a.ldh + e_c];
  };
  if (EARLY) prefetch();
  f32x4 acc[2][3];   // [row half][gate] of this wave's side
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int g = 0; g < 3; ++g) acc[mi][g] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    const D3_GLOBAL bf16x8* A = d3_g(sd ? a.Ah : a.Ai);
    const D3_GLOBAL bf16x8* B = d3_g(sd ? a.Bh : a.Bi);
    const int S = A ? (sd ? a.Sh : a.Si) : 0, SA = sd ? a.SAh : a.SAi, sa0 = sd ? a.sah0 : a.sai0;
    const int per = (S + 3) >> 2;
    const int s_lo = w4 * per, s_hi = min(S, s_lo + per);
    const D3_GLOBAL bf16x8* pa[2];
    const D3_GLOBAL bf16x8* pb[3];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) pa[mi] = A + ((size_t)(2 * mt + mi) * SA + sa0) * 3 * 64 + lane;
#pragma unroll
    for (int g = 0; g < 3; ++g) pb[g] = B + (size_t)(g * CT + ct) * S * 3 * 64 + lane;
    for (int s = s_lo; s < s_hi; s += TRIP) {
      bf16x8 fa[TRIP][2][NPL], fb[TRIP][3][NPL];
#pragma unroll
      for (int u = 0; u < TRIP; ++u) {
        const int su = min(s + u, s_hi - 1);
#pragma unroll
        for (int p = 0; p < NPL; ++p) {
#pragma unroll
          for (int mi = 0; mi < 2; ++mi) fa[u][mi][p] = pa[mi][(size_t)(su * 3 + p) * 64];
#pragma unroll
          for (int g = 0; g < 3; ++g) fb[u][g][p] = pb[g][(size_t)(su * 3 + p) * 64];
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < TRIP; ++u) {
        if (s + u >= s_hi) break;
        d3_mma_tiles<2, 3, NPL>(fa[u], fb[u], acc);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(wave * 24 + (g * 2 + mi) * 4 + r) * 64 + lane] = acc[mi][g][r];
  if (!EARLY) prefetch();
  __syncthreads();
  // all six gate values of the lane's element in one thread; loads are all behind it, so the stores go out together at the end
  {
    const int mi = e_mi, r = e_r, col = e_col, c = e_c, row = e_row, m = e_m;
    float gv[2][3];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        const int q = (g * 2 + mi) * 4 + r;
        gv[s2][g] = ((red[((s2 * 4 + 0) * 24 + q) * 64 + lane] + red[((s2 * 4 + 1) * 24 + q) * 64 + lane]) +
                     red[((s2 * 4 + 2) * 24 + q) * 64 + lane]) + red[((s2 * 4 + 3) * 24 + q) * 64 + lane];
      }
    float hv = 0.f;
    if (m < a.M) {
      float gi[3], gh[3];
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        gi[g] = pre_gi[g] + gv[0][g] + pre_bi[g];
        gh[g] = gv[1][g] + pre_bh[g];
      }
      const float rg = 1.f / (1.f + expf(-(gi[0] + gh[0])));
      const float zg = 1.f / (1.f + expf(-(gi[1] + gh[1])));
      const float ng = tanhf(gi[2] + rg * gh[2]);
      const float hp = pre_hp;
      {
        // both products rounded, then added: with h_prev already in a register the compiler would otherwise contract one of them
        // into a fused multiply-add, and h would differ in its last bit from what this kernel has always computed
#pragma clang fp contract(off)
        const float keep = (1.f - zg) * ng, carry = zg * hp;
        hv = keep + carry;
      }
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        const int n = g * a.H + c;
        if (a.gi_out) d3_g(a.gi_out)[(size_t)m * 3 * a.H + n] = gi[g];
        if (a.gh_out) d3_g(a.gh_out)[(size_t)m * 3 * a.H + n] = gh[g];
      }
      if (a.h_out) d3_g(a.h_out)[(size_t)m * a.ldo + c] = hv;
    }
    tile[row * 20 + col] = hv;
  }
  if (a.h_out3 || a.h_out3T) __syncthreads();
  if (a.h_out3T && wave == 2) {
    // transposed image (rows = hidden columns, reduction index = batch rows): one whole fragment, row tile col0T / 16 + ct
    const int c = lane & 15, kg = lane >> 4;
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = tile[(8 * kg + e) * 20 + c];
    bf16x8 pl[NPL];
    d3_split<NPL>(x, pl);
    D3_GLOBAL bf16x8* o = d3_g(a.h_out3T) + ((size_t)((a.col0T >> 4) + ct) * a.S3T + a.s3T0 + mt) * 3 * 64 + lane;
#pragma unroll
    for (int p = 0; p < NPL; ++p) o[p * 64] = pl[p];
  }
  if (a.h_out3) {
    // 16 columns = k groups 2 (ct & 1), 2 (ct & 1) + 1 of k-step s30 + ct / 2: half of the lanes of each fragment
    if (wave < 2 && lane < 32) {
      const int row = 16 * wave + (lane & 15), g = lane >> 4;   // g in {0, 1}
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(&tile[row * 20 + 8 * g]), x1 = *reinterpret_cast<const f32x4*>(&tile[row * 20 + 8 * g + 4]);
      const float x[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
      bf16x8 pl[NPL];
      d3_split<NPL>(x, pl);
      D3_GLOBAL bf16x8* o = d3_g(a.h_out3) + ((size_t)(2 * mt + wave) * a.S3 + a.s30 + (ct >> 1)) * 3 * 64 + 32 * (ct & 1) + lane;
#pragma unroll
      for (int p = 0; p < NPL; ++p) o[p * 64] = pl[p];
    }
  }
}

static void d3_launch_gru(hipStream_t st, const D3Gru& g0, const D3Gru* g1) {
  constexpr size_t lds = (size_t)(8 * 24 * 64 + 32 * 20) * sizeof(float);   // 50.5 KiB: within the default dynamic-LDS cap
  D3Gru2 two;
  two.g0 = g0; two.g1 = g1 ? *g1 : g0;
  two.rowmap = -1;   // the M >= N rule of d3_rowmap
  two.blocks0 = d3_blocks((g0.M + 31) >> 5, g0.H >> 4, d3_rowmap(-1, g0.M, 3 * g0.H));
  const int total = two.blocks0 + (g1 ? d3_blocks((g1->M + 31) >> 5, g1->H >> 4, d3_rowmap(-1, g1->M, 3 * g1->H)) : 0);
  switch (g0.prec) {
    case 2: hipLaunchKernelGGL((egx_gru3_kernel<2, 2>), dim3(total), dim3(512), lds, st, two); break;
    case 1: hipLaunchKernelGGL((egx_gru3_kernel<4, 1>), dim3(total), dim3(512), lds, st, two); break;
    default: hipLaunchKernelGGL((egx_gru3_kernel<2, 3>), dim3(total), dim3(512), lds, st, two);
  }
}
int egx_launch_gru3(hipStream_t st, const D3Gru& g) {
  d3_launch_gru(st, g, nullptr);
  return EGX_OK;
}
int egx_launch_gru3_pair(hipStream_t st, const D3Gru& g0, const D3Gru& g1) {
  d3_launch_gru(st, g0, &g1);
  return EGX_OK;
}

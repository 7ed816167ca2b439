// The plain dense layer of the dense3 scheme (d3.h): out = act(A B^T + bias) + res on packed operands, with the split-K
// reduction, the fp32 outputs and the packed images of the result in its epilogue.  Also here: the one-product C ABI entry
// egx_gemm3 on fp32 row-major operands.
#include <algorithm>
#include <cstddef>
#include "d3.h"

// One output element after the reduction (bias already added): activation, saved activation, residual, and the value that goes
// into the packed images (0 outside the matrix).  The element's residual and saved-activation operands come in as values (the
// kernel requests them ahead of the reduction barrier) and its fp32 outputs leave as values (v_act, v_out: stored by
// d3_store once the lane's last element is finished), so that no memory operation waits for another one in here.
__device__ __forceinline__ float d3_finish(const D3Plain& a, float v, int m, int n, float resv, float dactv, float& v_act, float& v_out) {
  v = d3_act(v, a.act, a.slope);
  const bool live = m < a.M && n < a.N;
  v_act = v;   // activation before the skip connection (saved for backward)
  if (live && a.res && !(a.n_split > 0 && n >= a.n_split)) v += resv;
  v_out = v;
  // gradient launches: what goes on to the next products is v x act'(saved activation of the layer below)
  if (live && a.dact) v *= d3_act_grad(dactv, a.dact_code, a.dact_slope);
  return live ? v : 0.f;
}
__device__ __forceinline__ void d3_store(const D3Plain& a, float v_act, float v_out, int m, int n, int row_base) {
  if (!(m < a.M && n < a.N)) return;
  if (a.out_act) d3_g(a.out_act)[(size_t)m * a.ldact + n] = v_act;
  if (a.n_split > 0 && n >= a.n_split) {
    // weight-gradient launch: the B operand's extra row of ones makes column n_split the bias gradient
    if (n == a.n_split && a.bias_out) d3_g(a.bias_out)[m] = v_out;
  } else if (a.out) {
    d3_g(a.out)[(size_t)(row_base + m) * a.ldo + n] = v_out;
  }
}

// Packed images of a finished tile (values in `tile`, pitch TN + 4).  Row-major image (the consumer's A operand): 16-row tiles
// MI mt + i, k-steps s30 + nt NI/2 + j.  Transposed image (rows = this layer's columns, reduction index = its rows - what a
// weight-gradient product reads): row tiles NI nt + j, k-steps s3T0 + mt MI/2 + i.  One wave per fragment.
template <int MI, int NI, int NW, int NPL>
__device__ __forceinline__ void d3_write_packed(const D3Plain& a, const float* tile, int mt, int nt, int batch, int wave, int lane) {
  constexpr int PITCH = 16 * NI + 4;
  constexpr int NR = MI * (NI / 2), NTT = NI * (MI / 2);
  const int ntask = (a.out3 ? NR : 0) + (a.out3T ? NTT : 0);
  const int m_ksteps = (a.M + 31) >> 5, n_ksteps = (a.N + 31) >> 5;   // extents of the images (even tile counts)
  for (int task = wave; task < ntask; task += NW) {
    float x[8];
    D3_GLOBAL bf16x8* o;
    if (a.out3 && task < NR) {
      const int i = task / (NI / 2), j = task % (NI / 2);
      if (MI * mt + i >= 2 * m_ksteps || nt * (NI / 2) + j >= n_ksteps) continue;   // past the image (ragged last tile)
      const int row = 16 * i + (lane & 15), g = lane >> 4;
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(&tile[row * PITCH + 32 * j + 8 * g]), x1 = *reinterpret_cast<const f32x4*>(&tile[row * PITCH + 32 * j + 8 * g + 4]);
      x[0] = x0[0]; x[1] = x0[1]; x[2] = x0[2]; x[3] = x0[3]; x[4] = x1[0]; x[5] = x1[1]; x[6] = x1[2]; x[7] = x1[3];
      o = d3_g(a.out3) + (size_t)batch * a.batch_stride3 + ((size_t)(MI * mt + i) * a.S3 + a.s30 + nt * (NI / 2) + j) * 3 * 64 + lane;
    } else {
      const int tt = task - (a.out3 ? NR : 0);
      const int j = tt / (MI / 2), i = tt % (MI / 2);
      if (NI * nt + j >= 2 * n_ksteps || mt * (MI / 2) + i >= m_ksteps) continue;
      const int c = 16 * j + (lane & 15), kg = lane >> 4;
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = tile[(32 * i + 8 * kg + e) * PITCH + c];
      o = d3_g(a.out3T) + ((size_t)(NI * nt + j) * a.S3T + a.s3T0 + mt * (MI / 2) + i) * 3 * 64 + lane;
    }
    bf16x8 pl[NPL];
    d3_split<NPL>(x, pl);
#pragma unroll
    for (int p = 0; p < NPL; ++p) o[p * 64] = pl[p];
  }
}

// ---------------------------------------------------------------------------------------------------------
// plain layer: out = act(A B^T + bias) + res for a 32 x 32 output tile per workgroup, the reduction split over the four
// waves; up to EGX_DENSE3_MAX independent layers may share a launch.
// ---------------------------------------------------------------------------------------------------------
struct D3ArgsN {
  D3Plain p[EGX_DENSE3_MAX];
  int end[EGX_DENSE3_MAX];   // blocks [end[i - 1], end[i]) work on p[i] (from 0 for p[0]); unused slots end where the grid ends
  int rowmap;
};

// d3_kernarg reads the block's layer as element `which` of an array of D3Plain at the start of the kernel-argument segment
static_assert(offsetof(D3ArgsN, p) == 0 && sizeof(D3Plain) % 8 == 0, "layout");
static_assert(sizeof(D3ArgsN) <= 4096, "kernel-argument segment limit");

// MI x NI MFMA tiles of 16 x 16 per workgroup of NW waves (instantiated: 2 x 2 tiles; four waves, eight for 9..16 k-steps).
template <int TRIP, int MI, int NI, int NW, int NPL>
__global__ __launch_bounds__(64 * NW) void egx_dense3_kernel(D3ArgsN args) {
  constexpr int TM = 16 * MI, TN = 16 * NI, NACC = MI * NI * 4, PITCH = TN + 4;
  const int bx = (int)blockIdx.x;
  // the ends are constant-indexed fields of the argument block: scalar loads and scalar compares, nothing per lane.  (Leaving
  // after the first three ends when the block lies before the fourth - every launch of up to four layers - was measured and
  // is not faster: profiles/update_tail.md.)
  int which = 0, first = 0;
#pragma unroll
  for (int i = 0; i + 1 < EGX_DENSE3_MAX; ++i) {
    const int e = args.end[i];
    if (bx >= e) { which = i + 1; first = e; }
  }
  const D3Plain a = d3_kernarg<D3Plain>(which);
  const int bid = bx - first;
  extern __shared__ __attribute__((aligned(16))) float d3_smem[];
  float* red = d3_smem;                      // [NW waves][NACC][64]
  float* tile = d3_smem + NW * NACC * 64;    // [TM][PITCH]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int MT = (a.M + TM - 1) / TM, NT = (a.N + TN - 1) / TN;
  const int rowmap = d3_rowmap(args.rowmap, a.M, a.N);
  const int per_batch = d3_blocks(MT, NT, rowmap);
  const int batch = bid / per_batch;
  int mt, nt;
  if (!d3_tile(bid - batch * per_batch, MT, NT, mt, nt, rowmap)) return;
  const D3_GLOBAL bf16x8* Ab = d3_g(a.A) + (size_t)batch * a.batch_strideA;
  const int per = (a.S + NW - 1) / NW;
  const int s_lo = wave * per, s_hi = min(a.S, s_lo + per);
  f32x4 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  // fragment streams of this tile: A row tiles MI mt + i (k-steps sa0 + s of a buffer with SA per row tile); B column tiles
  // NI nt + j, clamped to the image (packed images hold an even number of 16-row tiles; columns past N are never stored)
  const int a_tiles = 2 * ((a.M + 31) >> 5), b_tiles = 2 * ((a.N + 31) >> 5);
  const D3_GLOBAL bf16x8* pa[MI];
  const D3_GLOBAL bf16x8* pb[NI];
#pragma unroll
  for (int i = 0; i < MI; ++i) pa[i] = Ab + ((size_t)min(MI * mt + i, a_tiles - 1) * a.SA + a.sa0) * 3 * 64 + lane;
#pragma unroll
  for (int j = 0; j < NI; ++j) pb[j] = d3_g(a.B) + (size_t)min(NI * nt + j, b_tiles - 1) * a.S * 3 * 64 + lane;
  for (int s = s_lo; s < s_hi; s += TRIP) {
    bf16x8 fa[TRIP][MI][NPL], fb[TRIP][NI][NPL];
#pragma unroll
    for (int u = 0; u < TRIP; ++u) {
      const int su = min(s + u, s_hi - 1);
#pragma unroll
      for (int p = 0; p < NPL; ++p) {
#pragma unroll
        for (int i = 0; i < MI; ++i) fa[u][i][p] = pa[i][(size_t)(su * 3 + p) * 64];
#pragma unroll
        for (int j = 0; j < NI; ++j) fb[u][j][p] = pb[j][(size_t)(su * 3 + p) * 64];
      }
    }
    // burst, wait, then only MFMAs: a wave that issues MFMAs with its own loads in flight runs the matrix pipe at about
    // half rate on this part (scripts/ubench/mfma_bf16.hip)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < TRIP; ++u)
      if (s + u < s_hi) d3_mma_tiles<MI, NI, NPL>(fa[u], fb[u], acc);
    __builtin_amdgcn_sched_barrier(0);
  }
  // split-K reduction through LDS; wave w then finishes MFMA tiles w, w + NW, ...: bias, activation, residual
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(wave * NACC + (mi * NI + ni) * 4 + r) * 64 + lane] = acc[mi][ni][r];
  // The elements this lane finishes - tiles t = wave, wave + NW, ..., rows 4 (lane >> 4) + r of each - follow from wave and lane
  // alone, so everything their epilogue reads from memory (bias, residual, the saved activation of a gradient launch) is
  // requested HERE as one batch: the round trip runs under the barrier and the LDS reduction.  (Ahead of the k-loop it would
  // ride on the operand wait for nothing at all, but the nine registers per tile would have to live through the loop, and
  // <3,2,2,4,2> and <2,2,2,8,3> sit exactly on an occupancy step: profiles/dense3_epilogue.md.)  Out-of-range lanes read a
  // clamped element - never an address past the matrix - and d3_finish masks the value.
  constexpr int TW = (MI * NI + NW - 1) / NW;   // tiles per wave
  const int row_base = batch * a.batch_rows_out;
  float pre_bias[TW], pre_res[TW][4], pre_dact[TW][4];
#pragma unroll
  for (int k = 0; k < TW; ++k) {
    pre_bias[k] = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) pre_res[k][r] = pre_dact[k][r] = 0.f;
    const int t = k * NW + wave;
    if (t >= MI * NI) continue;
    const int mi = t / NI, ni = t % NI;
    const int n = nt * TN + 16 * ni + (lane & 15);
    const int nc = min(n, a.N - 1), nr = min(n, (a.n_split > 0 ? a.n_split : a.N) - 1);   // res has no columns >= n_split
    const int m0 = mt * TM + 16 * mi + 4 * (lane >> 4);
    if (a.bias) pre_bias[k] = d3_g(a.bias)[nc];
    if (a.res) {
#pragma unroll
      for (int r = 0; r < 4; ++r) pre_res[k][r] = d3_g(a.res)[(size_t)(row_base + min(m0 + r, a.M - 1)) * a.ldr + nr];
    }
    if (a.dact) {
#pragma unroll
      for (int r = 0; r < 4; ++r) pre_dact[k][r] = d3_g(a.dact)[(size_t)min(m0 + r, a.M - 1) * a.lddact + nc];
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < TW; ++k) {
    const int t = k * NW + wave;
    if (t >= MI * NI) continue;
    const int mi = t / NI, ni = t % NI;
    const int col = 16 * ni + (lane & 15), n = nt * TN + col;
    const float bsv = n < a.N ? pre_bias[k] : 0.f;
    float v_act[4], v_out[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = t * 4 + r;
      float v = (red[(0 * NACC + q) * 64 + lane] + red[(1 * NACC + q) * 64 + lane]) + red[(2 * NACC + q) * 64 + lane];
#pragma unroll
      for (int w2 = 3; w2 < NW; ++w2) v += red[(w2 * NACC + q) * 64 + lane];
      const int row = 16 * mi + 4 * (lane >> 4) + r, m = mt * TM + row;
      tile[row * PITCH + col] = d3_finish(a, v + bsv, m, n, pre_res[k][r], pre_dact[k][r], v_act[r], v_out[r]);
    }
    // all fp32 stores of the tile together, after its last load
#pragma unroll
    for (int r = 0; r < 4; ++r) d3_store(a, v_act[r], v_out[r], mt * TM + 16 * mi + 4 * (lane >> 4) + r, n, row_base);
  }
  if (!a.out3 && !a.out3T) return;
  __syncthreads();
  d3_write_packed<MI, NI, NW, NPL>(a, tile, mt, nt, batch, wave, lane);
}

// ---- launchers ------------------------------------------------------------------------------------------
namespace {
template <int TRIP, int MI, int NI, int NW, int NPL>
void d3_launch_cfg(hipStream_t st, const D3Plain* ps, int n) {
  constexpr int TM = 16 * MI, TN = 16 * NI;
  constexpr size_t lds = (size_t)(NW * MI * NI * 4 * 64 + TM * (TN + 4)) * sizeof(float);
  static_assert(lds <= 64 * 1024, "within the default dynamic-LDS cap (above it: d3_raise_lds_cap)");
  D3ArgsN f;
  f.rowmap = -1;   // the M >= N rule of d3_rowmap
  int total = 0;
  for (int i = 0; i < EGX_DENSE3_MAX; ++i) {
    f.p[i] = ps[i < n ? i : n - 1];
    if (i < n) total += d3_blocks(egx_ceil_div(ps[i].M, TM), egx_ceil_div(ps[i].N, TN), d3_rowmap(-1, ps[i].M, ps[i].N)) * std::max(1, ps[i].batches);
    f.end[i] = total;
  }
  hipLaunchKernelGGL((egx_dense3_kernel<TRIP, MI, NI, NW, NPL>), dim3(total), dim3(64 * NW), lds, st, f);
}
// the three configurations of one arithmetic mode; DEEP_TRIP: k-steps per operand round trip of the deep one
template <int NPL, int DEEP_TRIP>
void d3_launch_mode(hipStream_t st, const D3Plain* ps, int n, bool wide, bool deep) {
  if (wide) d3_launch_cfg<2, 2, 2, 8, NPL>(st, ps, n);
  else if (deep) d3_launch_cfg<DEEP_TRIP, 2, 2, 4, NPL>(st, ps, n);
  else d3_launch_cfg<2, 2, 2, 4, NPL>(st, ps, n);
}
}  // namespace

// 32 x 32 tile per 4-wave workgroup, the reduction split over the waves; three k-steps per round trip for deep reductions
// (more than 16 k-steps), five with one plane; two otherwise.
// (Measured for the update's 1152-deep layers, profiles/r03_update_experiments.md: 64 x 64 and 64 x 32 tiles, eight-wave
// split-K, a software-pipelined loop and two k-steps per trip all land within a few per cent of this form or behind it.)
// All layers of a launch share the arithmetic mode of the first (the callers build them from one setting).
// The configuration follows from the launch as a whole (its deepest reduction, its tile count), so a product's kernel - and with
// it the split of its reduction over the waves, i.e. its bits - depends on its companions: a caller that merges launches and
// must keep results asks here first (update3.hip).
int egx_dense3_config(const D3Plain* ps, int n) {
  int smax = 0, tiles = 0;
  for (int i = 0; i < n; ++i) {
    smax = std::max(smax, ps[i].S);
    tiles += egx_ceil_div(ps[i].M, 32) * egx_ceil_div(ps[i].N, 32) * std::max(1, ps[i].batches);
  }
  if (smax > 16) return EGX_DENSE3_DEEP;
  // 9..16 k-steps: eight waves take two k-steps each, ONE operand round trip (four waves need two) - for a latency-bound launch:
  // at most two workgroups per CU
  return smax > 8 && tiles <= 512 ? EGX_DENSE3_WIDE : EGX_DENSE3_BASE;
}
int egx_launch_dense3_n(hipStream_t st, const D3Plain* ps, int n) {
  EGX_REQUIRE(ps && n >= 1 && n <= EGX_DENSE3_MAX, "1 to EGX_DENSE3_MAX products per launch");
  const int cfg = egx_dense3_config(ps, n);
  const bool deep = cfg == EGX_DENSE3_DEEP, wide = cfg == EGX_DENSE3_WIDE;
  switch (ps[0].prec) {
    case 2: d3_launch_mode<2, 3>(st, ps, n, wide, deep); break;
    case 1: d3_launch_mode<1, 5>(st, ps, n, wide, deep); break;
    default: d3_launch_mode<3, 3>(st, ps, n, wide, deep);
  }
  return EGX_OK;
}
void egx_launch_dense3(hipStream_t st, const D3Plain& p) { egx_launch_dense3_n(st, &p, 1); }
void egx_launch_dense3_pair(hipStream_t st, const D3Plain& p, const D3Plain& q) {
  const D3Plain ps[2] = {p, q};
  egx_launch_dense3_n(st, ps, 2);
}
void egx_launch_dense3_triple(hipStream_t st, const D3Plain& p, const D3Plain& q, const D3Plain& r) {
  const D3Plain ps[3] = {p, q, r};
  egx_launch_dense3_n(st, ps, 3);
}

// ---- one product on fp32 row-major operands (training-side autograd nodes: fused_ops.py) ---------------------------------
extern "C" size_t egx_gemm3_workspace_bytes(int M, int N, int K) { return egx_pack3_bytes(M, K) + egx_pack3_bytes(N, K); }

extern "C" int egx_gemm3(const float* A, int lda, int trans_a, const float* B, int ldb, int trans_b, int M, int N, int K,
                         const float* bias, int act, float slope, const float* res, int ldr, float* out, int ldo, float* out_act,
                         int ldact, void* workspace, size_t workspace_bytes, void* stream) {
  EGX_REQUIRE(A && B && out && M > 0 && N > 0 && K > 0 && workspace, "bad arguments");
  EGX_REQUIRE(lda >= (trans_a ? M : K) && ldb >= (trans_b ? N : K) && ldo >= N && (!res || ldr >= N) && (!out_act || ldact >= N),
              "leading dimension smaller than the row");
  EGX_REQUIRE(workspace_bytes >= egx_gemm3_workspace_bytes(M, N, K), "workspace too small (egx_gemm3_workspace_bytes)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int S = egx_ceil_div(K, 32);
  char* ws = static_cast<char*>(workspace);
  void* img_a = ws;
  void* img_b = ws + egx_pack3_bytes(M, K);
  D3Pack jobs[2];
  jobs[0].src = A; jobs[0].R = M; jobs[0].K = K; jobs[0].ld = lda; jobs[0].col0 = 0; jobs[0].dst = img_a; jobs[0].S_total = S; jobs[0].s0 = 0;
  jobs[0].transpose = trans_a ? 1 : 0;
  jobs[1].src = B; jobs[1].R = N; jobs[1].K = K; jobs[1].ld = ldb; jobs[1].col0 = 0; jobs[1].dst = img_b; jobs[1].S_total = S; jobs[1].s0 = 0;
  jobs[1].transpose = trans_b ? 1 : 0;
  egx_launch_pack3(st, jobs, 2);
  D3Plain p;
  p.A = static_cast<const bf16x8*>(img_a); p.SA = S; p.sa0 = 0;
  p.B = static_cast<const bf16x8*>(img_b); p.S = S;
  p.bias = bias; p.res = res; p.ldr = ldr; p.out = out; p.ldo = ldo; p.M = M; p.N = N; p.act = act; p.slope = slope;
  p.out_act = out_act; p.ldact = ldact;
  egx_launch_dense3(st, p);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

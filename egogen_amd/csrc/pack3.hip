// Operand images of the dense3 kernels (d3.h) from fp32 row-major matrices: the packing kernel, the positional-encoding kernel
// that writes its columns straight into an image, and the C ABI of the former.
#include "d3.h"

// ---------------------------------------------------------------------------------------------------------
// packing: fp32 rows [R, K] (leading dimension ld, starting at column col0) -> [2 ceil(R/32)][S][3][64] fragments at k-step
// offset s0 of a buffer with S_total k-steps per row tile.  Fragment lane l = (r & 15) + 16 ((k >> 3) & 3), element k & 7.
// Rows >= R and columns >= K are zero; the row-tile count is even so that a 32-row workgroup tile always finds both of its
// 16-row halves.  Up to four jobs per launch (the motion prior's x0 / x1 / z, the policy's two frames of state and egosensing).
// ---------------------------------------------------------------------------------------------------------
struct D3PackJob {
  const float* src;
  int R, K, ld, col0;
  bf16x8* dst;
  int S_total, s0;
  int transpose;   // 1: the source block is [K rows (the reduction index), R columns]: image rows = source columns
};
struct D3PackJobs {
  D3PackJob j0, j1, j2, j3;
  int end0, end1, end2;   // running fragment counts: job i owns fragments [end(i-1), end(i))
};

__global__ __launch_bounds__(256) void egx_pack3_kernel(D3PackJobs jobs) {
  int frag = blockIdx.x * 4 + (threadIdx.x >> 6);   // (rt, s) of one of the jobs
  const int which = frag < jobs.end0 ? 0 : (frag < jobs.end1 ? 1 : (frag < jobs.end2 ? 2 : 3));
  const D3PackJob& j = which == 0 ? jobs.j0 : (which == 1 ? jobs.j1 : (which == 2 ? jobs.j2 : jobs.j3));
  frag -= which == 0 ? 0 : (which == 1 ? jobs.end0 : (which == 2 ? jobs.end1 : jobs.end2));
  const int lane = threadIdx.x & 63;
  const int RT = 2 * ((j.R + 31) >> 5), S = (j.K + 31) >> 5;
  if (!j.src || frag >= RT * S) return;
  const int rt = frag / S, s = frag % S;
  const int row = rt * 16 + (lane & 15), k0 = s * 32 + 8 * (lane >> 4);
  float x[8];
  if (!j.transpose) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = (row < j.R && k0 + e < j.K) ? j.src[(size_t)row * j.ld + j.col0 + k0 + e] : 0.f;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = (row < j.R && k0 + e < j.K) ? j.src[(size_t)(k0 + e) * j.ld + j.col0 + row] : 0.f;
  }
  bf16x8 pl[3];
  d3_split(x, pl);
  bf16x8* o = j.dst + ((size_t)rt * j.S_total + j.s0 + s) * 3 * 64 + lane;
#pragma unroll
  for (int p = 0; p < 3; ++p) o[p * 64] = pl[p];
}

void egx_launch_pack3(hipStream_t st, const D3Pack* jobs, int njobs) {
  D3PackJobs J;
  D3PackJob* dst[4] = {&J.j0, &J.j1, &J.j2, &J.j3};
  int frags[4] = {0, 0, 0, 0};
  for (int i = 0; i < 4; ++i) {
    D3PackJob& d = *dst[i];
    if (i < njobs) {
      d.src = jobs[i].src; d.R = jobs[i].R; d.K = jobs[i].K; d.ld = jobs[i].ld; d.col0 = jobs[i].col0;
      d.dst = static_cast<bf16x8*>(jobs[i].dst); d.S_total = jobs[i].S_total; d.s0 = jobs[i].s0;
      d.transpose = jobs[i].transpose;
      frags[i] = (int)d3_img_frags(d.R, d.K);
    } else {
      d.src = nullptr; d.R = d.K = d.ld = d.col0 = d.S_total = d.s0 = d.transpose = 0; d.dst = nullptr;
    }
  }
  J.end0 = frags[0]; J.end1 = J.end0 + frags[1]; J.end2 = J.end1 + frags[2];
  const int total = J.end2 + frags[3];
  hipLaunchKernelGGL(egx_pack3_kernel, dim3(egx_ceil_div(total, 4)), dim3(256), 0, st, J);
}

// positional_encoding (models_policy_ppo.py:276-285) of dist and time as the last 128 columns of the policy's [hx | he | pe]
// input: fp32 into `out` (row stride ld, the residual of the first MLP unit) and packed into k-steps s0 .. s0 + 3 of `out3`.
__global__ __launch_bounds__(256) void egx_posenc3_kernel(const float* __restrict__ dist, const float* __restrict__ time, int n,
                                                          float* __restrict__ out, int ld, bf16x8* __restrict__ out3, int S3, int s0,
                                                          bf16x8* __restrict__ out3T, int S3T, int col0T, float* __restrict__ zero6) {
  // (the update chain's loss kernel accumulates six sums with atomics: cleared here, several launches ahead of it, instead of
  // by a launch of their own)
  if (zero6 && blockIdx.x == 0 && threadIdx.x < 6) zero6[threadIdx.x] = 0.f;
  egx_posenc3_role(dist, time, n, out, ld, out3, S3, s0, out3T, S3T, col0T, (int)blockIdx.x, EgxRowsIdentity());   // the body: d3.h
}
void egx_launch_posenc3(hipStream_t st, const float* dist, const float* time, int n, float* out, int ld, void* out3, int S3, int s0,
                        void* out3T, int S3T, int col0T, float* zero6) {
  const int frags = 2 * egx_ceil_div(n, 32) * 4 + (out3T ? 8 * egx_ceil_div(n, 32) : 0);
  hipLaunchKernelGGL(egx_posenc3_kernel, dim3(egx_ceil_div(frags, 4)), dim3(256), 0, st, dist, time, n, out, ld,
                     static_cast<bf16x8*>(out3), S3, s0, static_cast<bf16x8*>(out3T), S3T, col0T, zero6);
}

// ---- C ABI: packing (weights once, raw network inputs per call) -------------------------------------------
extern "C" size_t egx_pack3_bytes(int num_rows, int num_cols) {
  if (num_rows <= 0 || num_cols <= 0) return 0;
  return d3_img_frags(num_rows, num_cols) * D3_FRAG_BYTES;
}
extern "C" int egx_pack3(const float* src, int num_rows, int num_cols, int src_ld, int src_col0, void* dst, int dst_ksteps,
                         int dst_kstep0, void* stream) {
  EGX_REQUIRE(src && dst && num_rows > 0 && num_cols > 0 && src_ld >= src_col0 + num_cols, "bad arguments");
  const int S = egx_ceil_div(num_cols, 32);
  EGX_REQUIRE(dst_kstep0 >= 0 && dst_ksteps >= dst_kstep0 + S, "destination k-step range too small");
  D3Pack job{src, num_rows, num_cols, src_ld, src_col0, dst, dst_ksteps, dst_kstep0};
  egx_launch_pack3(static_cast<hipStream_t>(stream), &job, 1);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

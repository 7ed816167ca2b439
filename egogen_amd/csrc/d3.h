// Device-side helpers of the "dense3" kernels: dense layers on the bf16 matrix pipe with fp32-equivalent arithmetic.  Included by
// .hip files only (dense3.hip, gru3.hip, pack3.hip, regressor3.hip, vposer3.hip, update3.hip, prior.hip).
//
// The rollout networks (C-VAE decoder models/models_GAMMA_primitive.py:83-133, policy models/models_policy_ppo.py:24-39,
// 287-350) are chains of small dependent products (M = agents, K, N <= 1536): what a launch costs is its latency, and on
// gfx950 the fp32 MFMA runs at 1/16 of the bf16 rate.  Here every fp32 operand x is carried as three bf16 terms
// x = hi + mid + lo (24+ significant bits) and a product keeps the six partial products down to 2^-24 relative
// (mid.mid, hi.lo, lo.hi, hi.mid, mid.hi, hi.hi), accumulated in fp32 by v_mfma_f32_16x16x32_bf16 - the arithmetic of the
// LBS blend GEMM's three-plane mode (lbs_fused3.hip).  What makes it pay for latency-bound layers:
//   * operands live in HBM already split and in MFMA fragment order ("packed": [16-row tile][32-wide k-step][plane][lane]
//     16 bytes), so a wave's loads are whole contiguous KiB and no consumer spends VALU time on splitting;
//   * the PRODUCER of an activation writes that packed form from its epilogue (one split per element instead of one per
//     consuming workgroup), next to the fp32 row-major copy only where a non-GEMM consumer needs it;
//   * concatenated inputs ([hx | z], [x_enc | ego_enc | posenc]) are k-step ranges of one packed buffer: no copies;
//   * the GRU cell is ONE launch (gru3.hip), and the body regressor and the VPoser encoder are whole networks per launch with
//     their activations as packed planes in LDS (regressor3.hip, vposer3.hip).
// Weights are packed once (motion prior: at load; policy: after every optimiser step, update3.hip).
#pragma once
#include <mutex>
#include "egx_nets.h"

typedef __bf16 bf16v8 __attribute__((ext_vector_type(8)));
typedef float f32x4a1 __attribute__((ext_vector_type(4), aligned(4)));

// Arithmetic of a product ("prec" of D3Plain / D3Gru) = how many of the bf16 planes of each operand take part:
//   prec 0: three planes, six partial products (2^-24 relative: fp32-equivalent)
//   prec 2: two planes (hi, mid: 16 significant bits per operand), three partial products - the LBS blend GEMM's default mode
//   prec 1: the leading plane only (operands rounded to bf16), one product - "bf16 MFMA, fp32 accumulate"
// Accumulation, biases, activations and every fp32 output are the same in all three.  Images always have room for three
// planes; a layer only READS the planes its mode uses and only WRITES those planes of the activation images it produces
// (weight images and raw-input images always carry all three: they are shared with launches of other modes).
__host__ __device__ constexpr int d3_planes(int prec) { return prec == 0 ? 3 : (prec == 2 ? 2 : 1); }

// Packed image of a matrix [rows, red] (red = the reduction index): an EVEN count of 16-row tiles, so that a 32-row workgroup
// tile always finds both of its halves, times ceil(red / 32) k-steps of one fragment each: 3 planes x 64 lanes x 16 bytes.
static inline int d3_img_tiles(int rows) { return 2 * egx_ceil_div(rows, 32); }
static inline size_t d3_img_frags(int rows, int red) { return (size_t)d3_img_tiles(rows) * egx_ceil_div(red, 32); }
constexpr size_t D3_FRAG_BYTES = 3 * 64 * 16;

// x[8] -> NP bf16 planes (v_cvt_pk_bf16_f32, round to nearest even; the residuals are exact in fp32)
template <int NP = 3>
static __device__ __forceinline__ void d3_split(const float (&x)[8], bf16x8 (&pl)[NP]) {
  float r[8];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    bf16v8 h;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = (p == 0) ? x[e] : r[e];
      h[e] = (__bf16)v;
      r[e] = v - (float)h[e];
    }
    pl[p] = __builtin_bit_cast(bf16x8, h);
  }
}

// The same split of four consecutive columns v[rt][0..3] of one row per row tile, stored as one 8-byte LDS write per plane and
// row tile into the packed planes of `dst` ([row tile][KS k-steps][3 planes][64 lanes]): lane (m = lane & 15, g = lane >> 4)
// holds row 16 rt + m, columns 16 ct16 + 4 g .. + 3, i.e. k-step ct16 >> 1, fragment lane 16 (2 (ct16 & 1) + (g >> 1)) + m,
// elements 4 (g & 1) .. + 3 of its eight.
template <int KS, int NRT>
static __device__ __forceinline__ void d3_store_packed(const float (&v)[NRT][4], bf16x8* dst, int ct16, int lane) {
  typedef __bf16 bf16v4 __attribute__((ext_vector_type(4)));
  const int g = lane >> 4;
  char* o = reinterpret_cast<char*>(dst + (size_t)((ct16 >> 1) * 3) * 64 + 16 * (2 * (ct16 & 1) + (g >> 1)) + (lane & 15)) + 8 * (g & 1);
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt) {
    float r[4];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      bf16v4 h;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x = (p == 0) ? v[rt][e] : r[e];
        h[e] = (__bf16)x;
        r[e] = x - (float)h[e];
      }
      *reinterpret_cast<bf16v4*>(o + (size_t)((rt * KS) * 3 + p) * 64 * sizeof(bf16x8)) = h;
    }
  }
}

// The significant partial products of a mode, small ones first: product pr multiplies plane d3_pa(pr) of one operand with plane
// d3_pb(pr) of the other (0 = hi, 1 = mid, 2 = lo).  Three planes: mid.mid, hi.lo, lo.hi, hi.mid, mid.hi, hi.hi; two planes: the
// last three of those; one plane: hi.hi.
constexpr int d3_nprod(int npl) { return npl == 3 ? 6 : (npl == 2 ? 3 : 1); }
template <int NPL>
__host__ __device__ constexpr int d3_pa(int pr) {
  constexpr int plane[6] = {1, 0, 2, 0, 1, 0};
  return plane[pr + 6 - d3_nprod(NPL)];
}
template <int NPL>
__host__ __device__ constexpr int d3_pb(int pr) {
  constexpr int plane[6] = {1, 2, 0, 1, 0, 0};
  return plane[pr + 6 - d3_nprod(NPL)];
}

// acc += a . b for a block of MI x NI output tiles, product-major: consecutive MFMAs go to different accumulators, so none
// waits for the previous one's result.
template <int MI, int NI, int NPL>
static __device__ __forceinline__ void d3_mma_tiles(const bf16x8 (&fa)[MI][NPL], const bf16x8 (&fb)[NI][NPL], f32x4 (&acc)[MI][NI]) {
#pragma unroll
  for (int pr = 0; pr < d3_nprod(NPL); ++pr) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[mi][d3_pa<NPL>(pr)], fb[ni][d3_pb<NPL>(pr)], acc[mi][ni], 0, 0, 0);
  }
}

// Every pointer of D3Plain / D3Gru is a device-memory address, but the kernels copy those structs out of the kernel-argument
// segment as ints (d3_kernarg), which hides that from the compiler: it then emits FLAT loads and stores, and those count on the
// LDS counter as well as on the vector-memory one, so that every wait for an LDS read also waits for all of them.  d3_g() states
// the address space where a pointer is used: global loads and stores, which the epilogues can keep in flight across LDS traffic.
#if defined(__HIP_DEVICE_COMPILE__)
#define D3_GLOBAL __attribute__((address_space(1)))
#else
#define D3_GLOBAL
#endif
template <class T>
static __device__ __forceinline__ D3_GLOBAL T* d3_g(T* p) { return (D3_GLOBAL T*)p; }

// The layer a block works on, of the several a launch carries (D3ArgsN, D3Gru2).  Picking one of the structs by reference
// (`which == 0 ? args.p[0] : ...`, or `args.p[which]`) makes the compiler copy all of the kernel arguments to scratch in every wave and read the
// fields back with vector loads; selecting field by field keeps them in SGPRs but loads all of the structs, or reads each field
// where it is first used - a scalar round trip in the middle of the epilogue.  Reading the one struct straight from the
// kernel-argument segment (constant address space, uniform offset: scalar loads, all at the top of the kernel) touches only
// what is used.  The array of structs is the kernels' first argument, so element 0 sits at offset 0 of the segment.
template <class T>
static __device__ __forceinline__ T d3_kernarg(int which) {
  T a;
  static_assert(sizeof(T) % 4 == 0, "layout");
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const __attribute__((address_space(4))) char* kptr;
  typedef const __attribute__((address_space(4))) int* iptr;
  iptr src = (iptr)((kptr)__builtin_amdgcn_kernarg_segment_ptr() + (size_t)which * sizeof(T));
  int* dst = reinterpret_cast<int*>(&a);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 4); ++i) dst[i] = src[i];
#else
  (void)which;
#endif
  return a;
}

static __device__ __forceinline__ float d3_act(float v, int act, float slope) {
  switch (act) {
    case 1: return tanhf(v);
    case 2: return fmaxf(v, 0.f);
    case 3: return v > 0.f ? v : v * slope;
    default: return v;
  }
}

// derivative of the activation as a function of its OUTPUT a = act(z) (tanh: 1 - a^2; relu / leaky relu keep the sign of z)
static __device__ __forceinline__ float d3_act_grad(float a, int act, float slope) {
  switch (act) {
    case 1: return 1.f - a * a;
    case 2: return a > 0.f ? 1.f : 0.f;
    case 3: return a > 0.f ? 1.f : slope;
    default: return 1.f;
  }
}

// XCD-aware tile map (blocks are dealt round-robin to the 8 XCDs, each with a private L2): every XCD owns a contiguous chunk
// of column tiles - i.e. of the weights - and sweeps the row tiles.
// With rowmap every XCD owns a chunk of ROW tiles - of the activations - and sweeps the weights instead.  An XCD's L2 is filled
// with all of the operand it sweeps and an eighth of the one it owns, so the map follows the larger operand: rows when M >= N
// (the decoder's 512-row layers: 8.1 -> 6.9 us), columns otherwise (the policy's 256 x 1152 layers: 18.4 against 19.8 us with
// rows).  mode < 0: that rule, which is what every launcher passes; 0 / 1: columns / rows always.
__host__ __device__ inline int d3_rowmap(int mode, int M, int N) { return mode < 0 ? (M >= N ? 1 : 0) : mode; }
static __device__ __forceinline__ bool d3_tile(int bid, int MT, int NT, int& mt, int& nt, int rowmap = 0) {
  const int xcd = bid & 7, local = bid >> 3;
  if (rowmap) {
    const int per = (MT + 7) >> 3;
    mt = xcd * per + local / NT;
    nt = local % NT;
    return local < per * NT && mt < MT;
  }
  const int per = (NT + 7) >> 3;
  nt = xcd * per + local / MT;
  mt = local % MT;
  return local < per * MT && nt < NT;
}
__host__ __device__ inline int d3_blocks(int MT, int NT, int rowmap = 0) {
  return rowmap ? 8 * ((MT + 7) / 8) * NT : 8 * ((NT + 7) / 8) * MT;
}

// A launch that asks for more dynamic LDS than the 64 KiB default cap needs the cap of its kernel raised first: done once per
// device and kernel (Kernel: the address of the __global__ function), outside graph capture.
template <auto Kernel>
static int d3_raise_lds_cap(size_t lds) {
  if (lds <= 64 * 1024) return EGX_OK;
  static std::mutex mu;
  static bool attr_set[64] = {false};
  int dev = 0;
  EGX_HIP_CHECK(hipGetDevice(&dev));
  EGX_REQUIRE(dev >= 0 && dev < 64, "device ordinal out of range");
  std::lock_guard<std::mutex> lk(mu);
  if (!attr_set[dev]) {
    EGX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set[dev] = true;
  }
  return EGX_OK;
}

// positional_encoding (models_policy_ppo.py:276-285) of dist and time, work of block `bid` (four fragments): the 128 columns as
// fp32 into `out` (row stride ld) and packed into k-steps s0 .. s0 + 3 of `out3`; blocks past those, with out3T != null: the same
// columns as rows col0T .. col0T + 127 of the transposed image (reduction index = batch row).  One body for egx_posenc3_kernel
// (pack3.hip: rows as they are) and egx_update_head_kernel (update3.hip: gathered rows), see the row maps in egx_nets.h.
template <class Rows>
static __device__ __forceinline__ void egx_posenc3_role(const float* __restrict__ dist, const float* __restrict__ time, int n,
                                                        float* __restrict__ out, int ld, bf16x8* __restrict__ out3, int S3, int s0,
                                                        bf16x8* __restrict__ out3T, int S3T, int col0T, int bid, const Rows& rows) {
  int frag = bid * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int RT = 2 * ((n + 31) >> 5);
  if (frag >= RT * 4) {
    frag -= RT * 4;
    const int Sn = (n + 31) >> 5;
    if (!out3T || frag >= 8 * Sn) return;
    const int t = frag / Sn, s = frag % Sn;
    const int c = 16 * t + (lane & 15), m0 = 32 * s + 8 * (lane >> 4);
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int m = m0 + e;
      float v = 0.f;
      if (m < n) {
        const size_t sm = rows(m);
        const float f = ((c < 64) ? dist[sm] : time[sm]) * exp2f((float)((c & 63) >> 1));
        v = (c & 1) ? cosf(f) : sinf(f);
      }
      x[e] = v;
    }
    bf16x8 pl[3];
    d3_split(x, pl);
    bf16x8* o = out3T + ((size_t)((col0T >> 4) + t) * S3T + s) * 3 * 64 + lane;
#pragma unroll
    for (int p = 0; p < 3; ++p) o[p * 64] = pl[p];
    return;
  }
  const int rt = frag >> 2, s = frag & 3;
  const int row = rt * 16 + (lane & 15), c0 = s * 32 + 8 * (lane >> 4);
  const size_t srow = row < n ? rows(row) : 0;
  float x[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = c0 + e;
    float v = 0.f;
    if (row < n) {
      const float f = ((c < 64) ? dist[srow] : time[srow]) * exp2f((float)((c & 63) >> 1));
      v = (c & 1) ? cosf(f) : sinf(f);
      out[(size_t)row * ld + c] = v;
    }
    x[e] = v;
  }
  bf16x8 pl[3];
  d3_split(x, pl);
  bf16x8* o = out3 + ((size_t)rt * S3 + s0 + s) * 3 * 64 + lane;
#pragma unroll
  for (int p = 0; p < 3; ++p) o[p * 64] = pl[p];
}

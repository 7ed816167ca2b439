// One PPO minibatch - forward, clipped-PPO loss, backward - of the policy networks as a fixed chain of hand-written launches
// (crowd_ppo/ppo_policy.py:189-252 `learn`, through models/models_policy_ppo.py:24-39, 287-350).  No autograd graph, no library
// GEMM: every product runs on the dense3 kernels (bf16 matrix pipe, three-term splits = fp32-equivalent), with what used to be
// separate launches folded into their epilogues:
//   forward   activation, skip connection, the saved activation for backward, and the packed images the next products read
//             (row-major image for the next layer, transposed image for this layer's weight gradient);
//   backward  dX = G W^T-image with the skip gradient added and the result multiplied by act'(saved activation) on its way into
//             the packed images of the next gradient; dW = G^T-image x X^T-image, whose extra row of ones makes the bias
//             gradient one more output column; input- and weight-gradient products of the actor AND the critic share a launch;
//   GRU       cell forward = one launch per time step for both encoders (dense3 gru kernel), cell backward = one launch per
//             step producing the gate gradients directly as packed images.
// 19 launches per minibatch (egx_update_head_kernel first) instead of ~85.  Gradients are WRITTEN (not accumulated) into the flat
// gradient buffer - every parameter is used exactly once per minibatch - so the buffer needs no zero fill.
//   optimiser  the step that follows a minibatch (egx_adamw_clip_step_train): norm partials and constants as in ppo.hip, then ONE
//             pass over the weights, egx_adamw_table_kernel - AdamW inside the blocks that make the weight images, the biases in
//             blocks of their own - instead of egx_adamw_flat_kernel and a weight-image launch that reads back what it wrote.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
#include "adamw.h"
#include "d3.h"

namespace {

// ---- table-driven packing: any number of matrices per launch, optionally transposed, optionally with a row of ones ----------
struct PackEntry {
  const float* src;
  int red, cols, ld, col0;   // source block: `red` rows x `cols` columns starting at column col0 (leading dimension ld)
  bf16x8* dst;
  int S_total, s0;           // destination: k-steps per row tile, first k-step
  int transpose;             // 0: image rows = source rows (reduction along the columns); 1: image rows = source columns;
                             // 2: BOTH images of the whole matrix from one read (dst: rows = source rows, dst2: rows = source
                             //    columns), a 32 x 32 source block per wave
  int ones_row;              // transposed images: image row that is all ones (-1: none)
  int frag_end;              // running fragment count (this entry owns [previous frag_end, frag_end)); blocks for transpose 2
  bf16x8* dst2;              // transpose 2: the transposed image
  int S_total2;              //              and its k-steps per row tile
};

// one fragment of a plain (transpose 0) or transposed (1) table entry: shared by egx_pack3_table_kernel (rows as they are) and
// egx_update_head_kernel (gathered rows), so that the two cannot drift apart
template <class Rows>
__device__ __forceinline__ void u3_pack_fragment(const PackEntry& e, const float* __restrict__ src, int frag, int lane, int nplanes,
                                                 const Rows& rows) {
  float x[8];
  int rt, s;
  if (!e.transpose) {
    const int S = (e.cols + 31) >> 5;
    rt = frag / S; s = frag % S;
    const int row = rt * 16 + (lane & 15), k0 = s * 32 + 8 * (lane >> 4);
    const size_t srow = row < e.red ? rows(row) : 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) x[q] = (row < e.red && k0 + q < e.cols) ? src[srow * e.ld + e.col0 + k0 + q] : 0.f;
  } else {
    const int S = (e.red + 31) >> 5;
    rt = frag / S; s = frag % S;
    const int irow = rt * 16 + (lane & 15), k0 = s * 32 + 8 * (lane >> 4);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      float v = 0.f;
      if (k0 + q < e.red) {
        if (irow < e.cols) v = src[rows(k0 + q) * e.ld + e.col0 + irow];
        else if (irow == e.ones_row) v = 1.f;
      }
      x[q] = v;
    }
  }
  bf16x8 pl[3];
  d3_split(x, pl);
  bf16x8* o = e.dst + ((size_t)rt * e.S_total + e.s0 + s) * 3 * 64 + lane;
#pragma unroll
  for (int p = 0; p < 3; ++p)
    if (p < nplanes) o[p * 64] = pl[p];   // planes no consumer reads are not written (a third of the image bytes per plane)
}

__global__ __launch_bounds__(256) void egx_pack3_table_kernel(const PackEntry* __restrict__ tab, int n, int nplanes) {
  int frag = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (n <= 0 || frag >= tab[n - 1].frag_end) return;
  int lo = 0, hi = n - 1;   // first entry whose running count exceeds `frag`
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (frag >= tab[mid].frag_end) lo = mid + 1; else hi = mid;
  }
  const PackEntry e = tab[lo];
  frag -= lo > 0 ? tab[lo - 1].frag_end : 0;
  float x[8];
  if (e.transpose == 2) {
    // weight matrix W [red, cols] -> image of W (the forward products' operand) and image of W^T (the input-gradient
    // products'): the wave reads its 32 x 32 block once, writes W's two fragments from registers and W^T's two after a
    // transposition through its LDS strip
    __shared__ float sblk[4][32][33];
    float (*sb)[33] = sblk[threadIdx.x >> 6];
    const int BJ = (e.cols + 31) >> 5;
    const int bi = frag / BJ, bj = frag % BJ;
    const int r = lane & 15, kg = lane >> 4;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int row = 32 * bi + 16 * t + r, k0 = 32 * bj + 8 * kg;
      const float* sp = e.src + (size_t)row * e.ld + e.col0 + k0;
      if (row < e.red && k0 + 7 < e.cols && (reinterpret_cast<uintptr_t>(sp) & 15) == 0) {   // the interior: two 16-byte loads
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(sp), x1 = *reinterpret_cast<const f32x4*>(sp + 4);
        x[0] = x0[0]; x[1] = x0[1]; x[2] = x0[2]; x[3] = x0[3]; x[4] = x1[0]; x[5] = x1[1]; x[6] = x1[2]; x[7] = x1[3];
      } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) x[q] = (row < e.red && k0 + q < e.cols) ? sp[q] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) sb[16 * t + r][8 * kg + q] = x[q];
      bf16x8 pl[3];
      d3_split(x, pl);
      bf16x8* o = e.dst + ((size_t)(2 * bi + t) * e.S_total + e.s0 + bj) * 3 * 64 + lane;
#pragma unroll
      for (int p = 0; p < 3; ++p)
        if (p < nplanes) o[p * 64] = pl[p];
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int q = 0; q < 8; ++q) x[q] = sb[8 * kg + q][16 * t + r];
      bf16x8 pl[3];
      d3_split(x, pl);
      bf16x8* o = e.dst2 + ((size_t)(2 * bj + t) * e.S_total2 + bi) * 3 * 64 + lane;
#pragma unroll
      for (int p = 0; p < 3; ++p)
        if (p < nplanes) o[p * 64] = pl[p];
    }
    return;
  }
  u3_pack_fragment(e, e.src, frag, lane, nplanes, EgxRowsIdentity());
}

// ---- the optimiser step's pass over the weights: AdamW and both weight images from ONE read of every parameter.  In the flat
// parameter buffer every weight matrix is an entry of the weight table (each exactly once) and the rest is biases and alignment
// padding, so AdamW can run in egx_pack3_table_kernel's own blocks: the wave that holds a 32 x 32 block (or a 16 x 32 fragment)
// of p loads the same elements of g, m and v, updates them (egx_adamw_elem, adamw.h: egx_adamw_flat_kernel's arithmetic), stores
// p, m and v and writes the images from the updated values in its registers - instead of a second launch that reads back what
// the first has just written.  The grid is partitioned by role; no role reads what another one writes (no fence, no ticket):
//   [0, b_tab)       table role: egx_pack3_table_kernel's work on the weight table, same fragment order, search and LDS strip
//   [.., + n_rem)    remainder role: egx_adamw_flat_kernel's body on the spans of [0, n) no table entry owns, <= 1024 elements
//                    a block (`rem`, made by the host from the entries' offsets: egx_policy_train_bind_flat)
// The host has checked that every entry is a whole contiguous matrix inside [0, n) and that no two overlap: no element is
// updated twice, and no index leaves the flat buffers.
struct RemBlock { size_t start, end; };   // flat elements [start, end), end - start <= 1024
struct AdamwTabArgs {
  const PackEntry* tab;
  int n_tab, frags_tab, nplanes;
  float* p; const float* g; float* m; float* v;
  size_t n_clip;
  const float* consts;   // egx_adamw_consts_kernel's: clip coefficient, step size, sqrt(bias correction 2)
  double lr, b1, b2, eps, wd;
  const RemBlock* rem;
  int b_tab, n_rem;
};

__device__ __forceinline__ bool u3_aligned16(const void* a, const void* b, const void* c, const void* d) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}
// p, g, m and v move with nontemporal accesses: each is touched once per optimiser step and by nothing else before the next one,
// while the images written beside them are what the next launches read.  With plain accesses the 369 MB of this pass push the
// images out of the last-level cache and the launches that follow pay for it (profiles/update_fused_tail.md).
__device__ __forceinline__ void u3_load8(const float* s, float (&x)[8]) {
  const f32x4 x0 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(s));
  const f32x4 x1 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(s + 4));
  x[0] = x0[0]; x[1] = x0[1]; x[2] = x0[2]; x[3] = x0[3]; x[4] = x1[0]; x[5] = x1[1]; x[6] = x1[2]; x[7] = x1[3];
}
__device__ __forceinline__ void u3_store8(float* d, const float (&x)[8]) {
  __builtin_nontemporal_store(f32x4{x[0], x[1], x[2], x[3]}, reinterpret_cast<f32x4*>(d));
  __builtin_nontemporal_store(f32x4{x[4], x[5], x[6], x[7]}, reinterpret_cast<f32x4*>(d + 4));
}
// AdamW on the flat elements fi .. fi + valid - 1 (valid <= 8: a row's in-range columns of a fragment lane) in two steps, so that
// a wave can have the loads of both halves of its block in flight before it computes: load (x = p), then update and store (x = the
// updated parameters, zero from `valid` on).  The interior - eight elements, 16-byte aligned in all four buffers - moves as two
// 16-byte accesses per array, ragged or unaligned rows element by element; nothing outside [fi, fi + valid) is read or written.
struct U3Adamw8 {
  size_t fi;
  int valid;
  bool fast;
  float x[8], gr[8], mv[8], vv[8];
};
__device__ __forceinline__ void u3_adamw8_load(const AdamwTabArgs& a, size_t fi, int valid, U3Adamw8& w) {
  const float *pp = a.p + fi, *gp = a.g + fi, *mp = a.m + fi, *vp = a.v + fi;
  w.fi = fi; w.valid = valid;
  w.fast = valid == 8 && u3_aligned16(pp, gp, mp, vp);
  if (w.fast) {
    u3_load8(pp, w.x); u3_load8(gp, w.gr); u3_load8(mp, w.mv); u3_load8(vp, w.vv);
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const bool in = q < valid;
      w.x[q] = in ? pp[q] : 0.f; w.gr[q] = in ? gp[q] : 0.f; w.mv[q] = in ? mp[q] : 0.f; w.vv[q] = in ? vp[q] : 0.f;
    }
  }
}
__device__ __forceinline__ void u3_adamw8_step(const AdamwTabArgs& a, const EgxAdamwK& k, U3Adamw8& w) {
#pragma unroll
  for (int q = 0; q < 8; ++q)
    if (q < w.valid) egx_adamw_elem(w.x[q], w.gr[q], w.mv[q], w.vv[q], w.fi + q < a.n_clip, k);
  float *pp = a.p + w.fi, *mp = a.m + w.fi, *vp = a.v + w.fi;
  if (w.fast) {
    u3_store8(pp, w.x); u3_store8(mp, w.mv); u3_store8(vp, w.vv);
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (q < w.valid) { pp[q] = w.x[q]; mp[q] = w.mv[q]; vp[q] = w.vv[q]; }
  }
}

__global__ __launch_bounds__(256) void egx_adamw_table_kernel(AdamwTabArgs a) {
  const EgxAdamwK k(a.consts, a.lr, a.b1, a.b2, a.eps, a.wd);
  if ((int)blockIdx.x >= a.b_tab) {   // ---- remainder role: egx_adamw_flat_kernel's body on one block of a span
    const int rb = (int)blockIdx.x - a.b_tab;
    if (rb >= a.n_rem) return;
    const RemBlock blk = a.rem[rb];
    const size_t i0 = blk.start + 4 * (size_t)threadIdx.x;
    if (i0 >= blk.end) return;
    const int cnt = (int)((blk.end - i0 < 4) ? (blk.end - i0) : 4);
    float gr[4], pv[4], mv[4], vv[4];
    const bool vec = cnt == 4 && u3_aligned16(a.p + i0, a.g + i0, a.m + i0, a.v + i0);
    if (vec) {
      *reinterpret_cast<f32x4*>(gr) = *reinterpret_cast<const f32x4*>(a.g + i0);
      *reinterpret_cast<f32x4*>(pv) = *reinterpret_cast<const f32x4*>(a.p + i0);
      *reinterpret_cast<f32x4*>(mv) = *reinterpret_cast<const f32x4*>(a.m + i0);
      *reinterpret_cast<f32x4*>(vv) = *reinterpret_cast<const f32x4*>(a.v + i0);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = e < cnt;
        gr[e] = in ? a.g[i0 + e] : 0.f; pv[e] = in ? a.p[i0 + e] : 0.f; mv[e] = in ? a.m[i0 + e] : 0.f; vv[e] = in ? a.v[i0 + e] : 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < cnt) egx_adamw_elem(pv[e], gr[e], mv[e], vv[e], i0 + e < a.n_clip, k);
    if (vec) {
      *reinterpret_cast<f32x4*>(a.p + i0) = *reinterpret_cast<const f32x4*>(pv);
      *reinterpret_cast<f32x4*>(a.m + i0) = *reinterpret_cast<const f32x4*>(mv);
      *reinterpret_cast<f32x4*>(a.v + i0) = *reinterpret_cast<const f32x4*>(vv);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) { a.p[i0 + e] = pv[e]; a.m[i0 + e] = mv[e]; a.v[i0 + e] = vv[e]; }
    }
    return;
  }
  // ---- table role: egx_pack3_table_kernel on the weight table, AdamW in place of the plain loads
  const PackEntry* __restrict__ tab = a.tab;
  int frag = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, nplanes = a.nplanes;
  if (frag >= a.frags_tab) return;
  int lo = 0, hi = a.n_tab - 1;   // first entry whose running count exceeds `frag`
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (frag >= tab[mid].frag_end) lo = mid + 1; else hi = mid;
  }
  const PackEntry e = tab[lo];
  frag -= lo > 0 ? tab[lo - 1].frag_end : 0;
  const size_t base = (size_t)(e.src - a.p) + e.col0;   // flat index of the matrix's element (0, 0)
  float x[8];
  if (e.transpose == 2) {
    __shared__ float sblk[4][32][33];
    float (*sb)[33] = sblk[threadIdx.x >> 6];
    const int BJ = (e.cols + 31) >> 5;
    const int bi = frag / BJ, bj = frag % BJ;
    const int r = lane & 15, kg = lane >> 4;
    U3Adamw8 w[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {   // the loads of the whole block first
      const int row = 32 * bi + 16 * t + r, k0 = 32 * bj + 8 * kg;
      const int valid = row < e.red ? min(max(e.cols - k0, 0), 8) : 0;
      u3_adamw8_load(a, valid ? base + (size_t)row * e.ld + k0 : 0, valid, w[t]);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      u3_adamw8_step(a, k, w[t]);
#pragma unroll
      for (int q = 0; q < 8; ++q) sb[16 * t + r][8 * kg + q] = w[t].x[q];
      bf16x8 pl[3];
      d3_split(w[t].x, pl);
      bf16x8* o = e.dst + ((size_t)(2 * bi + t) * e.S_total + e.s0 + bj) * 3 * 64 + lane;
#pragma unroll
      for (int p = 0; p < 3; ++p)
        if (p < nplanes) o[p * 64] = pl[p];
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int q = 0; q < 8; ++q) x[q] = sb[8 * kg + q][16 * t + r];
      bf16x8 pl[3];
      d3_split(x, pl);
      bf16x8* o = e.dst2 + ((size_t)(2 * bj + t) * e.S_total2 + bi) * 3 * 64 + lane;
#pragma unroll
      for (int p = 0; p < 3; ++p)
        if (p < nplanes) o[p * 64] = pl[p];
    }
    return;
  }
  // transpose 0 (the host admits no other): u3_pack_fragment's fragment with rows as they are
  const int S = (e.cols + 31) >> 5;
  const int rt = frag / S, s = frag % S;
  const int row = rt * 16 + (lane & 15), k0 = s * 32 + 8 * (lane >> 4);
  const int valid = row < e.red ? min(max(e.cols - k0, 0), 8) : 0;
  U3Adamw8 w;
  u3_adamw8_load(a, valid ? base + (size_t)row * e.ld + k0 : 0, valid, w);
  u3_adamw8_step(a, k, w);
  bf16x8 pl[3];
  d3_split(w.x, pl);
  bf16x8* o = e.dst + ((size_t)rt * e.S_total + e.s0 + s) * 3 * 64 + lane;
#pragma unroll
  for (int p = 0; p < 3; ++p)
    if (p < nplanes) o[p * 64] = pl[p];
}

// ---- the head of a minibatch: ONE launch for what used to be five (index copy aside): the row gather, the advantage
// statistics, the input images, the positional encoding and the clearing of the loss sums.  The grid is partitioned by role;
// no role reads what another one writes, so the blocks are independent (no fence, no ticket, no last-block epilogue):
//   [0, b_pack)          egx_pack3_table_kernel's work on the input table, entry row r reading row idx[r] of the ROLLOUT's
//                        state / egosensing (the first half of the table's entries is the state's, the second the ego's)
//   [.., + b_pe)         egx_posenc3_kernel's work on dist[idx[r]] / time[idx[r]]; its first block clears the six loss sums
//   [.., + b_gather)     act, adv, returns, logp_old rows idx[r] into the compact buffers the loss kernel reads (8 rows a block)
//   one more (optional)  mean / unbiased std of adv[idx[.]] in the reduction order of egx_adv_stats_kernel (ppo.hip)
// idx = perm + k n with k = *cursor (a device scalar a LATER single-block launch of the chain advances, egx_adamw_consts_kernel:
// never a block of this launch), clamped to [0, max_cursor]; the loss sums of minibatch k are row k of `log`.  Row indices are
// clamped to the rollout's rows: a bad index reads a wrong row, never another allocation.
struct HeadArgs {
  const PackEntry* tab;
  int n_tab, frags_tab, nplanes;
  const float *state, *ego;
  const long long* perm;
  const int* cursor;
  int max_cursor, n, num_src;
  const float *dist, *time, *act, *adv, *ret, *logp;
  float *act_c, *adv_c, *ret_c, *logp_c;
  float* stats;   // null: no statistics role (data parallel: the caller wrote the global ones)
  float* log;
  float* pe_out;
  int pe_ld;
  bf16x8* pe3;
  int S3, s0;
  bf16x8* pe3T;
  int S3T, col0T;
  int b_pack, b_pe, b_gather;
};
__device__ __forceinline__ int head_cursor(const HeadArgs& a) {
  const int k = a.cursor ? *a.cursor : 0;
  return min(max(k, 0), a.max_cursor);
}

__global__ __launch_bounds__(256) void egx_update_head_kernel(HeadArgs a) {
  const int k = head_cursor(a);
  const EgxRowsGathered rows{a.perm + (size_t)k * a.n, a.num_src};
  const int lane = threadIdx.x & 63;
  int bid = blockIdx.x;
  if (bid < a.b_pack) {   // ---- input images (egx_pack3_table_kernel, transpose 0 / 1, gathered rows)
    int frag = bid * 4 + (threadIdx.x >> 6);
    const PackEntry* __restrict__ tab = a.tab;
    if (frag >= a.frags_tab) return;
    int lo = 0, hi = a.n_tab - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (frag >= tab[mid].frag_end) lo = mid + 1; else hi = mid;
    }
    const PackEntry e = tab[lo];
    const float* __restrict__ src = (lo < (a.n_tab >> 1)) ? a.state : a.ego;
    frag -= lo > 0 ? tab[lo - 1].frag_end : 0;
    u3_pack_fragment(e, src, frag, lane, a.nplanes, rows);
    return;
  }
  bid -= a.b_pack;
  if (bid < a.b_pe) {   // ---- positional encoding (egx_posenc3_kernel, pack3.hip) of the gathered dist / time
    if (bid == 0 && threadIdx.x < 6) a.log[6 * (size_t)k + threadIdx.x] = 0.f;
    egx_posenc3_role(a.dist, a.time, a.n, a.pe_out, a.pe_ld, a.pe3, a.S3, a.s0, a.pe3T, a.S3T, a.col0T, bid, rows);
    return;
  }
  bid -= a.b_pe;
  if (bid < a.b_gather) {   // ---- compact rows for the loss kernel: 8 rows per block, 32 threads x 16 bytes = one act row
    const int r = bid * 8 + (threadIdx.x >> 5), c4 = threadIdx.x & 31;
    if (r >= a.n) return;
    const size_t srow = rows(r);
    reinterpret_cast<f32x4*>(a.act_c + (size_t)r * 128)[c4] = reinterpret_cast<const f32x4*>(a.act + srow * 128)[c4];
    if (c4 == 0) a.adv_c[r] = a.adv[srow];
    else if (c4 == 1) a.ret_c[r] = a.ret[srow];
    else if (c4 == 2) a.logp_c[r] = a.logp[srow];
    return;
  }
  if (!a.stats) return;
  egx_adv_stats_role(a.adv, a.n, a.stats, rows);   // egx_adv_stats_kernel's body on adv[idx[.]]: same additions, same order
}

// ---- GRU cell backward (torch.nn.GRU gate order r, z, n) with packed outputs ---------------------------------------------
//   r = s(gi_r + gh_r), z = s(gi_z + gh_z), nn = tanh(gi_n + r gh_n), h = (1 - z) nn + z hp
//   dnn = dh (1 - z), dz = dh (hp - nn), dhp = dh z, dpn = dnn (1 - nn^2), dgi_n = dpn, dgh_n = dpn r, dr = dpn gh_n,
//   dgi_r = dgh_r = dr r (1 - r), dgi_z = dgh_z = dz z (1 - z)
// Workgroup = 32 rows x 32 hidden columns.  Outputs: dgi / dgh as transposed images (rows = the 3H gate rows, reduction
// index = batch rows, k-step s0T + row tile / 2) for the weight-gradient products, dgh also as a row-major image (the product
// dh_prev += dgh W_hh) and dh z as fp32 - the last two only where asked.
struct GruBwd {
  const float* gi;        // [M, 3H]
  const float* gh;        // [M, 3H] or null: gh = bias_h (first step: zero previous state)
  const float* bias_h;
  const float* h_prev;    // [M, H] or null (zero)
  const float* dh0;       // gradient of h: dh0[m * ld0 + c] (+ dh1[m * ld1 + c] when dh1 != null)
  const float* dh1;
  int ld0, ld1;
  bf16x8* dgiT;           // images with ST k-steps per row tile
  bf16x8* dghT;
  int ST, s0T;
  bf16x8* dgh_r;          // [M rows, reduction 3H] or null
  float* dhp;             // [M, H] or null
  int M, H;
};
struct GruBwd2 {
  GruBwd a, b;
  int blocks0;
};

__global__ __launch_bounds__(256) void egx_gru_bwd3_kernel(GruBwd2 two) {
  const bool second = (int)blockIdx.x >= two.blocks0;
  const GruBwd& a = second ? two.b : two.a;
  const int bid = second ? (int)blockIdx.x - two.blocks0 : (int)blockIdx.x;
  __shared__ __attribute__((aligned(16))) float tile[6][32 * 36];   // [dgi r,z,n | dgh r,z,n]
  const int CT = a.H >> 5;
  const int mt = bid / CT, ct = bid % CT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int H = a.H;
  // thread t: column c = t & 31, rows (t >> 5) + 8 j
  const int cl = threadIdx.x & 31, c = ct * 32 + cl;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int rl = (threadIdx.x >> 5) + 8 * j, m = mt * 32 + rl;
    float o[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (m < a.M) {
      const float* gim = a.gi + (size_t)m * 3 * H;
      const float* ghm = a.gh ? a.gh + (size_t)m * 3 * H : a.bias_h;
      const float ghn = ghm[2 * H + c];
      const float r = 1.f / (1.f + expf(-(gim[c] + ghm[c])));
      const float z = 1.f / (1.f + expf(-(gim[H + c] + ghm[H + c])));
      const float nn = tanhf(gim[2 * H + c] + r * ghn);
      const float hp = a.h_prev ? a.h_prev[(size_t)m * H + c] : 0.f;
      float dh = a.dh0[(size_t)m * a.ld0 + c];
      if (a.dh1) dh += a.dh1[(size_t)m * a.ld1 + c];
      const float dnn = dh * (1.f - z), dz = dh * (hp - nn);
      const float dpn = dnn * (1.f - nn * nn);
      const float dpr = dpn * ghn * r * (1.f - r), dpz = dz * z * (1.f - z);
      o[0] = dpr; o[1] = dpz; o[2] = dpn; o[3] = dpr; o[4] = dpz; o[5] = dpn * r;
      if (a.dhp) a.dhp[(size_t)m * H + c] = dh * z;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) tile[q][rl * 36 + cl] = o[q];
  }
  __syncthreads();
  // transposed fragments: 6 tiles x 2 column halves; row-major fragments of dgh: 3 tiles x 2 row halves
  const int ntask = 12 + (a.dgh_r ? 6 : 0);
  for (int task = wave; task < ntask; task += 4) {
    float x[8];
    bf16x8* o;
    if (task < 12) {
      const int q = task >> 1, half = task & 1;   // q: tile, gate g = q % 3
      const int cc = 16 * half + (lane & 15), kg = lane >> 4;
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = tile[q][(8 * kg + e) * 36 + cc];
      bf16x8* img = q < 3 ? a.dgiT : a.dghT;
      const int row_tile = ((q % 3) * H + ct * 32) / 16 + half;
      o = img + ((size_t)row_tile * a.ST + a.s0T + mt) * 3 * 64 + lane;
    } else {
      const int g = (task - 12) >> 1, half = (task - 12) & 1;
      const int row = 16 * half + (lane & 15), kg = lane >> 4;
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(&tile[3 + g][row * 36 + 8 * kg]), x1 = *reinterpret_cast<const f32x4*>(&tile[3 + g][row * 36 + 8 * kg + 4]);
      x[0] = x0[0]; x[1] = x0[1]; x[2] = x0[2]; x[3] = x0[3]; x[4] = x1[0]; x[5] = x1[1]; x[6] = x1[2]; x[7] = x1[3];
      const int S = (3 * H) >> 5;
      o = a.dgh_r + ((size_t)(2 * mt + half) * S + (g * H) / 32 + ct) * 3 * 64 + lane;
    }
    bf16x8 pl[3];
    d3_split(x, pl);
#pragma unroll
    for (int p = 0; p < 3; ++p) o[p * 64] = pl[p];
  }
}

// ---- device arena ---------------------------------------------------------------------------------------------------------
struct Arena {
  char* base = nullptr;
  size_t off = 0, cap = 0;
  void* take(size_t bytes) {
    void* p = base ? base + off : nullptr;
    off = egx_align_up(off + bytes, 256);
    return p;
  }
};

constexpr int HD = 512, CAT = 1152, ZP = 256, ST_DIM = 402, EGO_DIM = 32;

struct Branch {   // actor or critic MLP block
  const float* W[4]; const float* b[4]; const float* Wout; const float* bout;
  float* gW[4]; float* gb[4]; float* gWout; float* gbout;
  int nout;
  bf16x8 *W_r[4], *W_t[4], *Wout_r, *Wout_t;   // weight images
  float *a[4], *u1f, *du2, *du1, *dhx;         // saved activations (fp32), unit-1 output, fp32 gradients of u2 / u1 / hx
  bf16x8 *a1_r, *u1_r, *a3_r, *u2_r, *a1T, *u1T, *a3T, *u2T;
  bf16x8 *g_r[4], *gT[4];                      // images of the gradient w.r.t. the pre-activation of layer l (and their transposes)
  float* head;                                 // zp [n,256] / value [n]
  float* ghead;                                // loss gradient w.r.t. the head's output
  bf16x8 *ghead_r, *gheadT;
};
struct Encoder {   // one 2-step GRU
  const float *Wih, *Whh, *bih, *bhh;
  float *gWih, *gWhh, *gbih, *gbhh;
  int in_dim, cat_off;
  bf16x8 *Wih_r, *Whh_r, *Whh_t;
  bf16x8 *x0_r, *x1_r, *xT;        // inputs: the two frames, and [x0; x1]^T with a row of ones
  float *gi1, *gi2, *gh2, *h1f;
  bf16x8 *h1_r, *hprevT;           // h1 as an operand; [h0 = 0; h1]^T with a row of ones
  bf16x8 *dgiT, *dghT, *dgh_r;
  float *dhp, *dh1;
};

}  // namespace

struct egx_policy_train {
  int n = 0, Sn = 0;
  Arena ar;
  Encoder enc[2];
  Branch br[2];
  float* catf = nullptr;
  bf16x8 *cat_r = nullptr, *catT = nullptr;
  PackEntry* tab_weights = nullptr; int n_weights = 0, frags_weights = 0;
  PackEntry* tab_inputs = nullptr; int n_inputs = 0, frags_inputs = 0;
  PackEntry* tab_loss = nullptr; int n_loss = 0, frags_loss = 0;
  std::vector<PackEntry> h_inputs;   // host copy: the source pointers of the observation change per call
  const float* bound_state = nullptr; const float* bound_ego = nullptr;
  int prec = 0;   // arithmetic of every product of the chain (D3Plain::prec): egx_policy_train_set_precision
  int dense3_launches = 0;   // egx_dense3_kernel launches of the last step call (egx_policy_train_dense3_launches)
  bool merge = true;   // independent products of the backward pass share launches (EGX_UPDATE_MERGE=0 at creation: the old sequence)
  // the optimiser step's fused tail (egx_adamw_table_kernel): wanted unless EGX_UPDATE_FUSED_TAIL=0 at creation, in force once
  // egx_policy_train_bind_flat has found every table entry a matrix of its own inside the flat buffer it was given
  bool fused_wanted = true, fused = false;
  std::vector<PackEntry> h_weights;
  const float* flat_p = nullptr; size_t flat_n = 0;
  RemBlock* rem = nullptr; int n_rem = 0;
};

namespace {

int upload_table(std::vector<PackEntry>& v, PackEntry** dev, int* frags) {
  int run = 0;
  for (PackEntry& e : v) {
    if (e.transpose == 2) {
      run += egx_ceil_div(e.red, 32) * egx_ceil_div(e.cols, 32);
    } else {
      const int rows = e.transpose ? e.cols + (e.ones_row >= 0 ? 1 : 0) : e.red;
      const int red = e.transpose ? e.red : e.cols;
      run += (int)d3_img_frags(rows, red);
    }
    e.frag_end = run;
  }
  *frags = run;
  if (!*dev) EGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(dev), v.size() * sizeof(PackEntry)));
  EGX_HIP_CHECK(hipMemcpy(*dev, v.data(), v.size() * sizeof(PackEntry), hipMemcpyHostToDevice));
  return EGX_OK;
}
void run_table(hipStream_t st, const PackEntry* tab, int n, int frags, int nplanes = 3) {
  hipLaunchKernelGGL(egx_pack3_table_kernel, dim3(egx_ceil_div(frags, 4)), dim3(256), 0, st, tab, n, nplanes);
}

// carve every buffer of a handle; with ar.base == nullptr this only measures
void layout(egx_policy_train* h) {
  const int n = h->n;
  Arena& ar = h->ar;
  ar.off = 0;
  auto img = [&](int rows, int red) { return static_cast<bf16x8*>(ar.take(d3_img_frags(rows, red) * D3_FRAG_BYTES)); };
  auto f32 = [&](size_t count) { return static_cast<float*>(ar.take(count * sizeof(float))); };
  for (int e = 0; e < 2; ++e) {
    Encoder& E = h->enc[e];
    E.Wih_r = img(3 * HD, E.in_dim); E.Whh_r = img(3 * HD, HD); E.Whh_t = img(HD, 3 * HD);
    E.x0_r = img(n, E.in_dim); E.x1_r = img(n, E.in_dim); E.xT = img(E.in_dim + 1, 2 * n);
    E.gi1 = f32((size_t)n * 3 * HD); E.gi2 = f32((size_t)n * 3 * HD); E.gh2 = f32((size_t)n * 3 * HD); E.h1f = f32((size_t)n * HD);
    E.h1_r = img(n, HD); E.hprevT = img(HD + 1, 2 * n);
    E.dgiT = img(3 * HD, 2 * n); E.dghT = img(3 * HD, 2 * n); E.dgh_r = img(n, 3 * HD);
    E.dhp = f32((size_t)n * HD); E.dh1 = f32((size_t)n * HD);
  }
  h->catf = f32((size_t)n * CAT); h->cat_r = img(n, CAT); h->catT = img(CAT + 1, n);
  for (int b = 0; b < 2; ++b) {
    Branch& B = h->br[b];
    for (int l = 0; l < 4; ++l) { B.W_r[l] = img(CAT, CAT); B.W_t[l] = img(CAT, CAT); B.a[l] = f32((size_t)n * CAT); }
    B.Wout_r = img(B.nout, CAT); B.Wout_t = img(CAT, B.nout);
    B.u1f = f32((size_t)n * CAT); B.du2 = f32((size_t)n * CAT); B.du1 = f32((size_t)n * CAT); B.dhx = f32((size_t)n * CAT);
    B.a1_r = img(n, CAT); B.u1_r = img(n, CAT); B.a3_r = img(n, CAT); B.u2_r = img(n, CAT);
    B.a1T = img(CAT + 1, n); B.u1T = img(CAT + 1, n); B.a3T = img(CAT + 1, n); B.u2T = img(CAT + 1, n);
    for (int l = 0; l < 4; ++l) { B.g_r[l] = img(n, CAT); B.gT[l] = img(CAT, n); }
    B.head = f32((size_t)n * B.nout); B.ghead = f32((size_t)n * B.nout);
    B.ghead_r = img(n, B.nout); B.gheadT = img(B.nout, n);
  }
}

// the all-ones row of a transposed activation image whose other rows are written by kernel epilogues
__global__ void egx_ones_row_kernel(bf16x8* img, int row, int S_total, int s_lo, int s_hi) {
  const int s = s_lo + blockIdx.x, kg = threadIdx.x;   // 4 threads: the k-groups of one fragment
  if (s >= s_hi) return;
  const int lane = (row & 15) + 16 * kg;
  bf16x8 one;
#pragma unroll
  for (int e = 0; e < 8; ++e) one[e] = (short)0x3F80;   // bf16 1.0
  img[((size_t)(row >> 4) * S_total + s) * 3 * 64 + lane] = one;   // plane 0; planes 1, 2 stay zero
}

}  // namespace

extern "C" int egx_policy_train_create(const egx_policy_weights* w, const egx_policy_grads* g, int num_rows, egx_policy_train** out) {
  EGX_REQUIRE(w && g && out, "null argument");
  EGX_REQUIRE(num_rows > 0 && num_rows % 32 == 0, "the minibatch must be a multiple of 32 rows");
  auto* h = new egx_policy_train();
  h->n = num_rows; h->Sn = num_rows / 32;
  if (const char* e = getenv("EGX_UPDATE_MERGE")) h->merge = !(e[0] == '0' && e[1] == 0);
  if (const char* e = getenv("EGX_UPDATE_FUSED_TAIL")) h->fused_wanted = !(e[0] == '0' && e[1] == 0);
  Encoder& X = h->enc[0];
  X.Wih = w->x_enc_w_ih; X.Whh = w->x_enc_w_hh; X.bih = w->x_enc_b_ih; X.bhh = w->x_enc_b_hh;
  X.gWih = g->x_enc_w_ih; X.gWhh = g->x_enc_w_hh; X.gbih = g->x_enc_b_ih; X.gbhh = g->x_enc_b_hh;
  X.in_dim = ST_DIM; X.cat_off = 0;
  Encoder& E = h->enc[1];
  E.Wih = w->ego_enc_w_ih; E.Whh = w->ego_enc_w_hh; E.bih = w->ego_enc_b_ih; E.bhh = w->ego_enc_b_hh;
  E.gWih = g->ego_enc_w_ih; E.gWhh = g->ego_enc_w_hh; E.gbih = g->ego_enc_b_ih; E.gbhh = g->ego_enc_b_hh;
  E.in_dim = EGO_DIM; E.cat_off = HD;
  for (int l = 0; l < 4; ++l) {
    h->br[0].W[l] = w->actor_w[l]; h->br[0].b[l] = w->actor_b[l]; h->br[0].gW[l] = g->actor_w[l]; h->br[0].gb[l] = g->actor_b[l];
    h->br[1].W[l] = w->critic_w[l]; h->br[1].b[l] = w->critic_b[l]; h->br[1].gW[l] = g->critic_w[l]; h->br[1].gb[l] = g->critic_b[l];
  }
  h->br[0].Wout = w->actor_out_w; h->br[0].bout = w->actor_out_b; h->br[0].gWout = g->actor_out_w; h->br[0].gbout = g->actor_out_b;
  h->br[0].nout = ZP;
  h->br[1].Wout = w->critic_out_w; h->br[1].bout = w->critic_out_b; h->br[1].gWout = g->critic_out_w; h->br[1].gbout = g->critic_out_b;
  h->br[1].nout = 1;
  layout(h);
  h->ar.cap = h->ar.off;
  if (hipMalloc(reinterpret_cast<void**>(&h->ar.base), h->ar.cap) != hipSuccess) {
    delete h;
    egx_set_error("egx_policy_train_create: device allocation failed");
    return EGX_ERR_HIP;
  }
  // every failure below releases the handle, its arena and whatever tables were uploaded (the caller never sees `h`)
  auto fail = [&](int rc_) { egx_policy_train_destroy(h); return rc_; };
#define U3_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { egx_set_error(std::string("egx_policy_train_create: ") + hipGetErrorString(e_)); return fail(EGX_ERR_HIP); } } while (0)
  U3_CHECK(hipMemset(h->ar.base, 0, h->ar.cap));
  layout(h);
  const int n = h->n, Sn = h->Sn;
  // rows of ones of the transposed activation images the epilogues fill (the tables write their own)
  auto ones = [&](bf16x8* img, int row, int S_total, int s_lo, int s_hi) {
    hipLaunchKernelGGL(egx_ones_row_kernel, dim3(s_hi - s_lo), dim3(4), 0, nullptr, img, row, S_total, s_lo, s_hi);
  };
  for (int e = 0; e < 2; ++e) ones(h->enc[e].hprevT, HD, 2 * Sn, 0, 2 * Sn);
  ones(h->catT, CAT, Sn, 0, Sn);
  for (int b = 0; b < 2; ++b)
    for (bf16x8* img : {h->br[b].a1T, h->br[b].u1T, h->br[b].a3T, h->br[b].u2T}) ones(img, CAT, Sn, 0, Sn);
  U3_CHECK(hipGetLastError());
  // ---- pack tables
  std::vector<PackEntry> tw;
  auto add = [](std::vector<PackEntry>& v, const float* src, int red, int cols, int ld, int col0, bf16x8* dst, int S_total, int s0,
                int transpose, int ones_row) {
    PackEntry e;
    e.src = src; e.red = red; e.cols = cols; e.ld = ld; e.col0 = col0; e.dst = dst; e.S_total = S_total; e.s0 = s0;
    e.transpose = transpose; e.ones_row = ones_row; e.frag_end = 0; e.dst2 = nullptr; e.S_total2 = 0;
    v.push_back(e);
  };
  // W and W^T images of a whole weight matrix [rows, cols] from one read of it
  auto add_both = [](std::vector<PackEntry>& v, const float* src, int rows, int cols, bf16x8* img, bf16x8* imgT) {
    PackEntry e;
    e.src = src; e.red = rows; e.cols = cols; e.ld = cols; e.col0 = 0; e.dst = img; e.S_total = egx_ceil_div(cols, 32); e.s0 = 0;
    e.transpose = 2; e.ones_row = -1; e.frag_end = 0; e.dst2 = imgT; e.S_total2 = egx_ceil_div(rows, 32);
    v.push_back(e);
  };
  for (int e = 0; e < 2; ++e) {
    Encoder& En = h->enc[e];
    add(tw, En.Wih, 3 * HD, En.in_dim, En.in_dim, 0, En.Wih_r, egx_ceil_div(En.in_dim, 32), 0, 0, -1);
    add_both(tw, En.Whh, 3 * HD, HD, En.Whh_r, En.Whh_t);
  }
  for (int b = 0; b < 2; ++b) {
    Branch& B = h->br[b];
    for (int l = 0; l < 4; ++l) {
      add_both(tw, B.W[l], CAT, CAT, B.W_r[l], B.W_t[l]);
    }
    add_both(tw, B.Wout, B.nout, CAT, B.Wout_r, B.Wout_t);
  }
  h->n_weights = (int)tw.size();
  int rc = upload_table(tw, &h->tab_weights, &h->frags_weights);
  if (rc) return fail(rc);
  h->h_weights = tw;
  // inputs: the two frames of every encoder as operands, and [frame 0; frame 1]^T (+ ones) for the weight gradient of W_ih
  for (int e = 0; e < 2; ++e) {
    Encoder& En = h->enc[e];
    const int d = En.in_dim, S = egx_ceil_div(d, 32);
    add(h->h_inputs, nullptr, n, d, 2 * d, 0, En.x0_r, S, 0, 0, -1);
    add(h->h_inputs, nullptr, n, d, 2 * d, d, En.x1_r, S, 0, 0, -1);
    add(h->h_inputs, nullptr, n, d, 2 * d, 0, En.xT, 2 * Sn, 0, 1, d);
    add(h->h_inputs, nullptr, n, d, 2 * d, d, En.xT, 2 * Sn, Sn, 1, d);
  }
  h->n_inputs = (int)h->h_inputs.size();
  // uploaded now with no sources: the head launch (egx_update_head_kernel) takes the rollout's state / egosensing as kernel
  // arguments and reads only the destinations; egx_policy_train_bind fills in the sources the table kernel reads
  if ((rc = upload_table(h->h_inputs, &h->tab_inputs, &h->frags_inputs))) return fail(rc);
  std::vector<PackEntry> tl;
  for (int b = 0; b < 2; ++b) {
    Branch& B = h->br[b];
    add(tl, B.ghead, n, B.nout, B.nout, 0, B.ghead_r, egx_ceil_div(B.nout, 32), 0, 0, -1);
    add(tl, B.ghead, n, B.nout, B.nout, 0, B.gheadT, Sn, 0, 1, -1);
  }
  h->n_loss = (int)tl.size();
  if ((rc = upload_table(tl, &h->tab_loss, &h->frags_loss))) return fail(rc);
  U3_CHECK(hipDeviceSynchronize());
#undef U3_CHECK
  *out = h;
  return EGX_OK;
}

extern "C" void egx_policy_train_destroy(egx_policy_train* h) {
  if (!h) return;
  (void)hipFree(h->ar.base); (void)hipFree(h->tab_weights); (void)hipFree(h->tab_inputs); (void)hipFree(h->tab_loss);
  (void)hipFree(h->rem);
  delete h;
}

// The flat buffers the optimiser steps this handle's weights in: `param` (n floats; gradient and both moments have its layout).
// Decides whether egx_adamw_clip_step_train may run the fused kernel: every entry of the weight table must be a whole contiguous
// matrix inside [param, param + n) and no two may overlap - then the spans between them (biases, padding, any parameter without an
// image) are cut into the remainder role's blocks.  Otherwise the handle keeps the two-launch tail and egx_last_error() says why.
extern "C" int egx_policy_train_bind_flat(egx_policy_train* h, const float* param, size_t n) {
  EGX_REQUIRE(h && param && n > 0, "bad arguments");
  h->fused = false; h->flat_p = param; h->flat_n = n;
  auto off_tail = [&](const std::string& why) {
    egx_set_error("egx_policy_train_bind_flat: the optimiser step keeps its two-launch tail - " + why);
    return EGX_OK;
  };
  if (!h->fused_wanted) return EGX_OK;   // EGX_UPDATE_FUSED_TAIL=0: asked for, nothing to report
  std::vector<std::pair<size_t, size_t>> own;   // [start, end) of every entry, in flat elements
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(param);
  for (size_t i = 0; i < h->h_weights.size(); ++i) {
    const PackEntry& e = h->h_weights[i];
    const std::string which = "weight table entry " + std::to_string(i);
    if (e.transpose != 0 && e.transpose != 2) return off_tail(which + " is a transposed view");
    if (e.col0 != 0 || e.ld != e.cols || e.red <= 0 || e.cols <= 0) return off_tail(which + " is not a whole contiguous matrix");
    const uintptr_t s = reinterpret_cast<uintptr_t>(e.src);
    const size_t cnt = (size_t)e.red * e.cols;
    if (s < p0 || (s - p0) % sizeof(float) != 0 || (s - p0) / sizeof(float) > n || cnt > n - (s - p0) / sizeof(float))
      return off_tail(which + " does not lie wholly inside the flat parameter buffer");
    own.emplace_back((s - p0) / sizeof(float), (s - p0) / sizeof(float) + cnt);
  }
  std::sort(own.begin(), own.end());
  for (size_t i = 1; i < own.size(); ++i)
    if (own[i].first < own[i - 1].second) return off_tail("two weight table entries overlap");
  std::vector<RemBlock> rem;
  size_t at = 0;
  auto span = [&](size_t lo, size_t hi) {
    for (; lo < hi; lo += 1024) rem.push_back({lo, std::min(lo + 1024, hi)});
  };
  for (const auto& o : own) { span(at, o.first); at = o.second; }
  span(at, n);
  (void)hipFree(h->rem);
  h->rem = nullptr; h->n_rem = (int)rem.size();
  EGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&h->rem), std::max<size_t>(1, rem.size()) * sizeof(RemBlock)));
  if (!rem.empty()) EGX_HIP_CHECK(hipMemcpy(h->rem, rem.data(), rem.size() * sizeof(RemBlock), hipMemcpyHostToDevice));
  h->fused = true;
  return EGX_OK;
}

extern "C" int egx_policy_train_fused_tail(const egx_policy_train* h) { return h ? (h->fused ? 1 : 0) : -1; }

extern "C" int egx_policy_train_refresh(egx_policy_train* h, void* stream) {
  EGX_REQUIRE(h, "null handle");
  // the weight images are read by this chain (h->prec) and by the rollout forward (egx_policy_get_precision): only the planes
  // one of them uses are written
  const int planes = std::max(d3_planes(h->prec), d3_planes(egx_policy_get_precision()));
  run_table(static_cast<hipStream_t>(stream), h->tab_weights, h->n_weights, h->frags_weights, planes);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

// The optimiser step of the policy this handle trains, its weight images included: egx_sumsq_partial_kernel, egx_adamw_consts_kernel
// and egx_adamw_table_kernel - three launches for the four of egx_adamw_clip_step + egx_policy_train_refresh, which is what runs
// where the fused kernel does not apply (EGX_UPDATE_FUSED_TAIL=0, a table that failed egx_policy_train_bind_flat, other buffers
// than the bound ones).  Either way p, m, v and this handle's images are those of the four launches, bit for bit.
static int adamw_clip_step_train(egx_policy_train* h, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                                 size_t n_clip, float max_norm, double lr, double beta1, double beta2, double eps, double weight_decay,
                                 float* step, float* workspace, int* cursor, void* stream_) {
  EGX_REQUIRE(h && param && grad && exp_avg && exp_avg_sq && step && workspace && n > 0 && n_clip <= n, "bad arguments");
  if (!(h->fused && param == h->flat_p && n == h->flat_n && h->frags_weights > 0)) {
    const int rc = egx_adamw_clip_step_launches(param, grad, exp_avg, exp_avg_sq, n, n_clip, max_norm, lr, beta1, beta2, eps, weight_decay,
                                                step, workspace, cursor, stream_);
    return rc ? rc : egx_policy_train_refresh(h, stream_);
  }
  hipStream_t st = static_cast<hipStream_t>(stream_);
  const int rc = egx_adamw_launch_consts(grad, n_clip, max_norm, lr, beta1, beta2, step, workspace, cursor, st);
  if (rc) return rc;
  AdamwTabArgs a;
  a.tab = h->tab_weights; a.n_tab = h->n_weights; a.frags_tab = h->frags_weights;
  a.nplanes = std::max(d3_planes(h->prec), d3_planes(egx_policy_get_precision()));   // egx_policy_train_refresh's rule
  a.p = param; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq; a.n_clip = n_clip; a.consts = workspace + EGX_ADAMW_CONSTS;
  a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.wd = weight_decay;
  a.rem = h->rem; a.b_tab = egx_ceil_div(h->frags_weights, 4); a.n_rem = h->n_rem;
  hipLaunchKernelGGL(egx_adamw_table_kernel, dim3(a.b_tab + a.n_rem), dim3(256), 0, st, a);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}
extern "C" int egx_adamw_clip_step_train(egx_policy_train* h, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                                         size_t n_clip, float max_norm, double lr, double beta1, double beta2, double eps,
                                         double weight_decay, float* step, float* workspace, void* stream) {
  return adamw_clip_step_train(h, param, grad, exp_avg, exp_avg_sq, n, n_clip, max_norm, lr, beta1, beta2, eps, weight_decay, step,
                               workspace, nullptr, stream);
}
extern "C" int egx_adamw_clip_step_train_cursor(egx_policy_train* h, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                                size_t n, size_t n_clip, float max_norm, double lr, double beta1, double beta2, double eps,
                                                double weight_decay, float* step, float* workspace, int32_t* cursor, void* stream) {
  return adamw_clip_step_train(h, param, grad, exp_avg, exp_avg_sq, n, n_clip, max_norm, lr, beta1, beta2, eps, weight_decay, step,
                               workspace, cursor, stream);
}

extern "C" int egx_policy_train_set_precision(egx_policy_train* h, int prec) {
  EGX_REQUIRE(h, "null handle");
  EGX_REQUIRE(prec == 0 || prec == 1 || prec == 2, "precision must be 0 (three bf16 planes: fp32-equivalent), 2 (two planes) or 1 (bf16)");
  h->prec = prec;
  return EGX_OK;
}

extern "C" int egx_policy_train_dense3_launches(const egx_policy_train* h) { return h ? h->dense3_launches : -1; }

extern "C" int egx_policy_train_packed(const egx_policy_train* h, egx_policy_packed3* out) {
  EGX_REQUIRE(h && out, "null argument");
  out->x_enc_w_ih = h->enc[0].Wih_r; out->x_enc_w_hh = h->enc[0].Whh_r;
  out->ego_enc_w_ih = h->enc[1].Wih_r; out->ego_enc_w_hh = h->enc[1].Whh_r;
  for (int l = 0; l < 4; ++l) { out->actor_w[l] = h->br[0].W_r[l]; out->critic_w[l] = h->br[1].W_r[l]; }
  out->actor_out_w = h->br[0].Wout_r; out->critic_out_w = h->br[1].Wout_r;
  return EGX_OK;
}

extern "C" int egx_policy_train_bind(egx_policy_train* h, const float* state, const float* egosensing) {
  EGX_REQUIRE(h && state && egosensing, "null argument");
  if (h->bound_state == state && h->bound_ego == egosensing) return EGX_OK;
  for (int i = 0; i < 4; ++i) h->h_inputs[i].src = state;
  for (int i = 4; i < 8; ++i) h->h_inputs[i].src = egosensing;
  int rc = upload_table(h->h_inputs, &h->tab_inputs, &h->frags_inputs);
  if (rc) return rc;
  h->bound_state = state; h->bound_ego = egosensing;
  return EGX_OK;
}

namespace {

constexpr int S_HD = HD / 32, S_CAT = CAT / 32, S_G = 3 * HD / 32;
constexpr float LRELU_SLOPE = 0.01f;   // torch.nn.LeakyReLU() default (baseops.py:627-628)

struct LossConsts {
  float adv_eps = 0.f, min_logvar = 0.f, max_logvar = 0.f, eps_clip = 0.f, vf_coef = 0.f, ent_coef = 0.f;
};
// One minibatch as the entry points below describe it: its rows (compact, or with `hd` the head launch's outputs), the loss
// normaliser and constants, where the six loss sums go, and the head launch (null: input table + positional encoding instead).
struct StepIn {
  const float *dist = nullptr, *time = nullptr, *act = nullptr, *adv = nullptr, *ret = nullptr, *logp_old = nullptr;
  const float *adv_stats = nullptr, *scale = nullptr;
  LossConsts c;
  float* out_terms = nullptr;
  const egx_update_head* hd = nullptr;
};

void launch_n(egx_policy_train* h, hipStream_t st, D3Plain* ps, int cnt) {
  for (int i = 0; i < cnt; ++i) ps[i].prec = h->prec;
  ++h->dense3_launches;
  (void)egx_launch_dense3_n(st, ps, cnt);   // cnt <= EGX_DENSE3_MAX by the sizes of the callers' arrays
}
// Consecutive groups of independent products, cnt[g] each, as few launches as keep the results: a product's kernel configuration -
// its split of the reduction over the waves, hence its bits - is chosen per launch (egx_dense3_config), so a group joins the launch
// of the groups before it only where its own launch and the joint one pick the same configuration (at 256 rows every one does; from
// 288 rows on the GRU weight gradients run the deep configuration and stay a launch of their own).  Without h->merge: one launch per
// group, the sequence before the merge.
void launch_groups(egx_policy_train* h, hipStream_t st, D3Plain* ps, const int* cnt, int groups) {
  for (int g = 0; g < groups;) {
    int len = cnt[g++];
    const int cfg = egx_dense3_config(ps, len);
    while (h->merge && g < groups && len + cnt[g] <= EGX_DENSE3_MAX && egx_dense3_config(ps + len, cnt[g]) == cfg &&
           egx_dense3_config(ps, len + cnt[g]) == cfg)
      len += cnt[g++];
    launch_n(h, st, ps, len);
    ps += len;
  }
}

int head_args_ok(const egx_policy_train* h, const egx_update_head* a) {
  EGX_REQUIRE(h && a, "null argument");
  EGX_REQUIRE(a->perm && a->state && a->egosensing && a->dist && a->time && a->act && a->adv && a->ret && a->logp_old &&
                  a->act_c && a->adv_c && a->ret_c && a->logp_old_c && a->stats && a->log, "null field in egx_update_head");
  EGX_REQUIRE(h->n_inputs == 8 && h->tab_inputs, "the input table must hold four state entries followed by four egosensing entries");
  EGX_REQUIRE(a->num_src_rows > 0 && a->max_cursor >= 0, "egx_update_head: num_src_rows must be positive, max_cursor non-negative");
  return EGX_OK;
}

// gather, statistics, input images, positional encoding, cleared loss sums: one launch
void launch_head(egx_policy_train* h, const egx_update_head* a, hipStream_t st) {
  const int n = h->n, Sn = h->Sn;
  HeadArgs k;
  k.tab = h->tab_inputs; k.n_tab = h->n_inputs; k.frags_tab = h->frags_inputs; k.nplanes = d3_planes(h->prec);
  k.state = a->state; k.ego = a->egosensing;
  k.perm = reinterpret_cast<const long long*>(a->perm); k.cursor = a->cursor; k.max_cursor = a->max_cursor; k.n = n;
  k.num_src = a->num_src_rows;
  k.dist = a->dist; k.time = a->time; k.act = a->act; k.adv = a->adv; k.ret = a->ret; k.logp = a->logp_old;
  k.act_c = a->act_c; k.adv_c = a->adv_c; k.ret_c = a->ret_c; k.logp_c = a->logp_old_c;
  k.stats = a->compute_stats ? a->stats : nullptr;
  k.log = a->log;
  k.pe_out = h->catf + 2 * HD; k.pe_ld = CAT; k.pe3 = h->cat_r; k.S3 = S_CAT; k.s0 = 2 * S_HD;
  k.pe3T = h->catT; k.S3T = Sn; k.col0T = 2 * HD;
  k.b_pack = egx_ceil_div(h->frags_inputs, 4);
  k.b_pe = egx_ceil_div(2 * Sn * 4 + 8 * Sn, 4);
  k.b_gather = egx_ceil_div(n, 8);
  const int blocks = k.b_pack + k.b_pe + k.b_gather + (k.stats ? 1 : 0);
  hipLaunchKernelGGL(egx_update_head_kernel, dim3(blocks), dim3(256), 0, st, k);
}

void step_inputs(egx_policy_train* h, const StepIn& in, hipStream_t st) {
  if (in.hd) {
    launch_head(h, in.hd, st);
    return;
  }
  run_table(st, h->tab_inputs, h->n_inputs, h->frags_inputs, d3_planes(h->prec));
  egx_launch_posenc3(st, in.dist, in.time, h->n, h->catf + 2 * HD, CAT, h->cat_r, S_CAT, 2 * S_HD, h->catT, h->Sn, 2 * HD,
                     in.out_terms);   // also clears the loss sums
}

// 2 GRU steps of both encoders -> [hx | he | pe]; 4 layers and the output layer of both MLP blocks
void step_forward(egx_policy_train* h, hipStream_t st) {
  const int n = h->n, Sn = h->Sn;
  D3Gru g[2];
  for (int e = 0; e < 2; ++e) {   // step 1: zero previous state
    Encoder& E = h->enc[e];
    const int Sx = egx_ceil_div(E.in_dim, 32);
    D3Gru& q = g[e];
    q.prec = h->prec;
    q.M = n; q.H = HD;
    q.Ai = E.x0_r; q.SAi = Sx; q.Bi = E.Wih_r; q.Si = Sx; q.bias_i = E.bih; q.bias_h = E.bhh;
    q.gi_out = E.gi1; q.h_out = E.h1f; q.ldo = HD; q.h_out3 = E.h1_r; q.S3 = S_HD;
    q.h_out3T = E.hprevT; q.S3T = 2 * Sn; q.s3T0 = Sn; q.col0T = 0;
  }
  egx_launch_gru3_pair(st, g[0], g[1]);
  for (int e = 0; e < 2; ++e) {   // step 2 -> [hx | he | pe]
    Encoder& E = h->enc[e];
    D3Gru& q = g[e];
    q.Ai = E.x1_r; q.gi_out = E.gi2; q.gh_out = E.gh2;
    q.Ah = E.h1_r; q.SAh = S_HD; q.Bh = E.Whh_r; q.Sh = S_HD; q.h_prev = E.h1f; q.ldh = HD;
    q.h_out = h->catf + E.cat_off; q.ldo = CAT; q.h_out3 = h->cat_r; q.S3 = S_CAT; q.s30 = E.cat_off / 32;
    q.h_out3T = h->catT; q.S3T = Sn; q.s3T0 = 0; q.col0T = E.cat_off;
  }
  egx_launch_gru3_pair(st, g[0], g[1]);

  D3Plain L[2];
  // h = hx; per unit: h = lrelu(fc2(lrelu(fc1(h)))) + h   (models_policy_ppo.py:24-39, baseops.py:615-641)
  for (int l = 0; l < 4; ++l) {
    for (int b = 0; b < 2; ++b) {   // layer l of both MLP blocks: in -> lrelu(W_l in + b_l) (+ res)
      Branch& B = h->br[b];
      const bf16x8* const in[4] = {h->cat_r, B.a1_r, B.u1_r, B.a3_r};
      const float* const res[4] = {nullptr, h->catf, nullptr, B.u1f};   // the skip connection closes after fc2 of a unit
      float* const outf[4] = {nullptr, B.u1f, nullptr, nullptr};        // unit 1's output in fp32: the skip of unit 2
      bf16x8* const o3[4] = {B.a1_r, B.u1_r, B.a3_r, B.u2_r};           // images of the output: the next product's operand
      bf16x8* const o3T[4] = {B.a1T, B.u1T, B.a3T, B.u2T};             // and its transpose for the next layer's weight gradient
      D3Plain& q = L[b];
      q = D3Plain();
      q.M = n; q.N = CAT; q.A = in[l]; q.SA = S_CAT; q.S = S_CAT; q.B = B.W_r[l]; q.bias = B.b[l]; q.act = 3; q.slope = LRELU_SLOPE;
      q.out_act = B.a[l]; q.ldact = CAT;   // the activation saved for backward
      q.res = res[l]; q.ldr = CAT; q.out = outf[l]; q.ldo = CAT;
      q.out3 = o3[l]; q.S3 = S_CAT; q.out3T = o3T[l]; q.S3T = Sn;
    }
    launch_n(h, st, L, 2);
  }
  for (int b = 0; b < 2; ++b) {   // heads: zp = [mu | logvar] and the value
    Branch& B = h->br[b];
    D3Plain& q = L[b];
    q = D3Plain();
    q.M = n; q.N = B.nout; q.A = B.u2_r; q.SA = S_CAT; q.S = S_CAT; q.B = B.Wout_r; q.bias = B.bout; q.out = B.head; q.ldo = B.nout;
  }
  launch_n(h, st, L, 2);
}

// the loss and its gradient w.r.t. the two heads (ppo_policy.py:189-241), then the images of that gradient
int step_loss(egx_policy_train* h, const StepIn& in, hipStream_t st) {
  const egx_update_head* hd = in.hd;
  int rc = egx_ppo_loss_packed_precleared(h->br[0].head, h->br[1].head, in.act, in.adv, in.ret, in.logp_old, in.adv_stats, in.scale,
                                          in.c.adv_eps, in.c.min_logvar, in.c.max_logvar, in.c.eps_clip, in.c.vf_coef, in.c.ent_coef, h->n,
                                          h->br[0].ghead, h->br[1].ghead, in.out_terms, st, hd ? hd->cursor : nullptr,
                                          hd ? hd->max_cursor : 0);
  if (rc) return rc;
  run_table(st, h->tab_loss, h->n_loss, h->frags_loss, d3_planes(h->prec));
  return EGX_OK;
}

// Backward of the actor and critic blocks.  Input-gradient products form the dependent chain (out_fc -> unit 2 -> unit 1 -> GRU
// cells); each layer's weight-gradient product follows the launch that left its gradient image behind.  (Weight gradients on a
// second stream beside the chain, and fused into the input-gradient launches, were both measured and are not faster:
// profiles/r03_update_experiments.md.)
// `WL`: the eight weight-gradient products of the layers, left to the caller with `defer_wl` (train_step_parts).
void step_blocks_bwd(egx_policy_train* h, hipStream_t st, D3Plain* WL, bool defer_wl) {
  const int n = h->n, Sn = h->Sn;
  auto wgrad = [&](D3Plain& q, const bf16x8* gT, const bf16x8* xT, int rows, float* gW, float* gb) {
    q = D3Plain();
    q.M = rows; q.N = CAT + 1; q.A = gT; q.SA = Sn; q.S = Sn; q.B = xT; q.out = gW; q.ldo = CAT; q.n_split = CAT; q.bias_out = gb;
  };
  // the output layer's weight gradients and the l = 4 input gradients below both read only the images of `ghead`: one launch
  D3Plain first[4];
  D3Plain *W = first, *D = first + 2;
  for (int b = 0; b < 2; ++b) wgrad(W[b], h->br[b].gheadT, h->br[b].u2T, h->br[b].nout, h->br[b].gWout, h->br[b].gbout);
  // Layer l of both blocks, l = 4 being out_fc: the input gradient d = g_l W_l^T-image (+ skip) now, as fp32 `out` raw and as
  // images gated by lrelu'(a_l) = g_(l-1).  Its weight gradient dW_l = g_l^T x_l only needs the images the previous launch left
  // behind, so the eight weight-gradient products of the four layers go out afterwards in one launch (fewer, fuller launches:
  // ~10 us of every launch is fixed cost, profiles/r03_update_experiments.md).
  //   4: du2 = g W_out -> g4    3: d(a3) = g4 W4 -> g3    2: du1 = g3 W3 + du2 -> g2    1: d(a1) = g2 W2 -> g1    0: dhx = g1 W1 + du1
  for (int l = 4; l >= 0; --l) {
    for (int b = 0; b < 2; ++b) {
      Branch& B = h->br[b];
      bf16x8* const xT[4] = {h->catT, B.a1T, B.u1T, B.a3T};
      float* const res[5] = {B.du1, nullptr, B.du2, nullptr, nullptr};
      float* const outf[5] = {B.dhx, nullptr, B.du1, nullptr, B.du2};
      if (l < 4) wgrad(WL[2 * l + b], B.gT[l], xT[l], CAT, B.gW[l], B.gb[l]);
      const int S_in = l < 4 ? S_CAT : egx_ceil_div(B.nout, 32), gate = l - 1;
      D3Plain& d = D[b];
      d = D3Plain();
      d.M = n; d.N = CAT; d.A = l < 4 ? B.g_r[l] : B.ghead_r; d.SA = S_in; d.S = S_in; d.B = l < 4 ? B.W_t[l] : B.Wout_t;
      d.res = res[l]; d.ldr = CAT; d.out = outf[l]; d.ldo = CAT;
      if (gate >= 0) {
        d.dact = B.a[gate]; d.lddact = CAT; d.dact_code = 3; d.dact_slope = LRELU_SLOPE;
        d.out3 = B.g_r[gate]; d.S3 = S_CAT; d.out3T = B.gT[gate]; d.S3T = Sn;
      }
    }
    const int two[2] = {2, 2};
    if (l == 4) launch_groups(h, st, first, two, 2);
    else launch_n(h, st, D, 2);
  }
  const int four[2] = {4, 4};
  if (!defer_wl) launch_groups(h, st, WL, four, 2);
}

// Backward of the two GRU encoders (dhx = actor's + critic's).  `tail`: twelve products, the last four the encoders' weight
// gradients built here; with `with_wl` the first eight (step_blocks_bwd's deferred ones) go out with them.
void step_encoders_bwd(egx_policy_train* h, hipStream_t st, D3Plain* tail, bool with_wl) {
  const int n = h->n, Sn = h->Sn;
  GruBwd2 two;
  const int blocks = (n / 32) * (HD / 32);
  two.blocks0 = blocks;
  GruBwd* gb[2] = {&two.a, &two.b};
  for (int e = 0; e < 2; ++e) {   // step 2
    Encoder& E = h->enc[e];
    GruBwd& q = *gb[e];
    q.gi = E.gi2; q.gh = E.gh2; q.bias_h = E.bhh; q.h_prev = E.h1f;
    q.dh0 = h->br[0].dhx + E.cat_off; q.ld0 = CAT; q.dh1 = h->br[1].dhx + E.cat_off; q.ld1 = CAT;
    q.dgiT = E.dgiT; q.dghT = E.dghT; q.ST = 2 * Sn; q.s0T = Sn; q.dgh_r = E.dgh_r; q.dhp = E.dhp; q.M = n; q.H = HD;
  }
  hipLaunchKernelGGL(egx_gru_bwd3_kernel, dim3(2 * blocks), dim3(256), 0, st, two);
  D3Plain P[2];
  for (int e = 0; e < 2; ++e) {   // dh1 = dh z + dgh2 W_hh
    Encoder& E = h->enc[e];
    D3Plain& d = P[e];
    d = D3Plain();
    d.M = n; d.N = HD; d.A = E.dgh_r; d.SA = S_G; d.S = S_G; d.B = E.Whh_t; d.res = E.dhp; d.ldr = HD; d.out = E.dh1; d.ldo = HD;
  }
  launch_n(h, st, P, 2);
  for (int e = 0; e < 2; ++e) {   // step 1 (h0 = 0: gh = b_hh)
    Encoder& E = h->enc[e];
    GruBwd& q = *gb[e];
    q.gi = E.gi1; q.gh = nullptr; q.h_prev = nullptr; q.dh0 = E.dh1; q.ld0 = HD; q.dh1 = nullptr; q.ld1 = 0;
    q.s0T = 0; q.dgh_r = nullptr; q.dhp = nullptr;
  }
  hipLaunchKernelGGL(egx_gru_bwd3_kernel, dim3(2 * blocks), dim3(256), 0, st, two);
  for (int e = 0; e < 2; ++e) {   // dW_ih = [dgi1; dgi2]^T [x0; x1], dW_hh = [dgh1; dgh2]^T [0; h1]; the ones rows give the biases
    Encoder& E = h->enc[e];
    D3Plain& a = tail[8 + 2 * e];
    a = D3Plain();
    a.M = 3 * HD; a.N = E.in_dim + 1; a.A = E.dgiT; a.SA = 2 * Sn; a.S = 2 * Sn; a.B = E.xT; a.out = E.gWih; a.ldo = E.in_dim;
    a.n_split = E.in_dim; a.bias_out = E.gbih;
    D3Plain& c = tail[8 + 2 * e + 1];
    c = D3Plain();
    c.M = 3 * HD; c.N = HD + 1; c.A = E.dghT; c.SA = 2 * Sn; c.S = 2 * Sn; c.B = E.hprevT; c.out = E.gWhh; c.ldo = HD;
    c.n_split = HD; c.bias_out = E.gbhh;
  }
  const int four[3] = {4, 4, 4};
  if (with_wl) launch_groups(h, st, tail, four, 3);
  else launch_n(h, st, tail + 8, 4);
}

// Launches of one minibatch (parts = 3): 19 with `in.hd` - head 1 | GRU steps 2, layers 4, output layers 1 | loss 1, its images 1
// | backward of the blocks 5 (output-layer weight gradients with the first of 5 input gradients) | GRU encoders 4, the last of
// them all twelve weight gradients of the layers and the encoders - and 20 without (input images and positional encoding instead
// of the head; the caller's gather and statistics launches come on top: 22).  parts = 1 ends after the blocks' backward and their
// eight weight gradients in one launch (16 / 17) - the heads' half leaves exactly the actor's and the critic's part of the flat
// gradient final - and parts = 2 is the encoders' 4.  Without h->merge (EGX_UPDATE_MERGE=0, the checker of the merged sequence):
// 22 / 23, the output-layer weight gradients and the layers' 2 x four as launches of their own, parts = 1 18 / 19.
int train_step_parts(egx_policy_train* h, const StepIn& in, void* stream_, int parts) {
  {   // egx_last_error() quotes a failed condition: these names are part of its sentences
    const float *dist = in.dist, *time = in.time, *act = in.act, *adv = in.adv, *ret = in.ret, *logp_old = in.logp_old,
                *scale = in.scale, *out_terms = in.out_terms;
    const egx_update_head* hd = in.hd;
    EGX_REQUIRE(h && (!(parts & 1) || (dist && time && act && adv && ret && logp_old && scale && out_terms)), "null argument");
    EGX_REQUIRE(hd || !(parts & 1) || h->bound_state, "egx_policy_train_bind has not been called");
  }
  hipStream_t st = static_cast<hipStream_t>(stream_);
  h->dense3_launches = 0;
  if (parts & 1) {
    step_inputs(h, in, st);
    step_forward(h, st);
    int rc = step_loss(h, in, st);
    if (rc) return rc;
  }
  static_assert(8 + 4 <= EGX_DENSE3_MAX, "the weight gradients of one launch");
  D3Plain tail[12];
  const bool defer_wl = h->merge && parts == 3;
  if (parts & 1) step_blocks_bwd(h, st, tail, defer_wl);   // parts = 1: every gradient of the actor and critic blocks is enqueued
  if (parts & 2) step_encoders_bwd(h, st, tail, defer_wl);
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}

// the minibatch behind ONE head launch (egx_update_head_kernel): its rows are named by indices into the rollout, the loss reads
// the compact copies the head leaves behind and writes row `cursor` of the head's log
int train_step_head(egx_policy_train* h, const egx_update_head* head, const float* scale, const LossConsts& c, void* stream_,
                    int parts) {
  int rc = head_args_ok(h, head);
  if (rc) return rc;
  const StepIn in{head->dist, head->time, head->act_c, head->adv_c, head->ret_c, head->logp_old_c, head->stats, scale, c, head->log, head};
  return train_step_parts(h, in, stream_, parts);
}

}  // namespace

extern "C" int egx_policy_train_step(egx_policy_train* h, const float* dist, const float* time, const float* act, const float* adv,
                                     const float* ret, const float* logp_old, const float* adv_stats, const float* scale,
                                     float adv_eps, float min_logvar, float max_logvar, float eps_clip, float vf_coef, float ent_coef,
                                     float* out_terms, void* stream_) {
  const StepIn in{dist, time, act, adv, ret, logp_old, adv_stats, scale, {adv_eps, min_logvar, max_logvar, eps_clip, vf_coef, ent_coef},
                  out_terms};
  return train_step_parts(h, in, stream_, 3);
}

// The same chain in two halves, for data-parallel training: `egx_policy_train_step_heads` ends when the last weight gradient of
// the actor and critic blocks has been enqueued (forward, loss, their whole backward: the 10.3 M-parameter prefix of the flat
// gradient is final), `egx_policy_train_step_encoders` runs the rest (the two GRU encoders' backward).  The caller all-reduces
// the first bucket on a side stream while the second half runs (egogen_amd/ppo_policy.py).
extern "C" int egx_policy_train_step_heads(egx_policy_train* h, const float* dist, const float* time, const float* act, const float* adv,
                                           const float* ret, const float* logp_old, const float* adv_stats, const float* scale,
                                           float adv_eps, float min_logvar, float max_logvar, float eps_clip, float vf_coef,
                                           float ent_coef, float* out_terms, void* stream_) {
  const StepIn in{dist, time, act, adv, ret, logp_old, adv_stats, scale, {adv_eps, min_logvar, max_logvar, eps_clip, vf_coef, ent_coef},
                  out_terms};
  return train_step_parts(h, in, stream_, 1);
}
extern "C" int egx_policy_train_step_encoders(egx_policy_train* h, void* stream_) {
  EGX_REQUIRE(h, "null handle");
  return train_step_parts(h, StepIn(), stream_, 2);
}

extern "C" int egx_policy_train_head(egx_policy_train* h, const egx_update_head* head, void* stream_) {
  int rc = head_args_ok(h, head);
  if (rc) return rc;
  launch_head(h, head, static_cast<hipStream_t>(stream_));
  EGX_HIP_CHECK(hipGetLastError());
  return EGX_OK;
}
extern "C" int egx_policy_train_step_cursor(egx_policy_train* h, const egx_update_head* head, const float* scale, float adv_eps,
                                            float min_logvar, float max_logvar, float eps_clip, float vf_coef, float ent_coef,
                                            void* stream_) {
  return train_step_head(h, head, scale, {adv_eps, min_logvar, max_logvar, eps_clip, vf_coef, ent_coef}, stream_, 3);
}
extern "C" int egx_policy_train_step_heads_cursor(egx_policy_train* h, const egx_update_head* head, const float* scale, float adv_eps,
                                                  float min_logvar, float max_logvar, float eps_clip, float vf_coef, float ent_coef,
                                                  void* stream_) {
  return train_step_head(h, head, scale, {adv_eps, min_logvar, max_logvar, eps_clip, vf_coef, ent_coef}, stream_, 1);
}

// AdamW on one element (torch.optim.AdamW arithmetic, fused_adam_utils.cuh [upstream torch]: fp32 state, double hyper-parameters,
// the mixed expressions in double), shared by egx_adamw_flat_kernel (ppo.hip) and egx_adamw_table_kernel (update3.hip) so that
// the two cannot drift apart by a bit.  Included by .hip files only.
#pragma once
#include "egx_common.h"

// what every element of a launch shares: the three device constants of egx_adamw_consts_kernel and the hyper-parameter
// expressions (evaluated once per thread, in double)
struct EgxAdamwK {
  float coef, step_size, bc2s;   // clip coefficient, lr / bias correction 1, sqrt(bias correction 2)
  double b2, eps, omb1, omb2, lrwd;
  __device__ __forceinline__ EgxAdamwK(const float* __restrict__ consts, double lr, double b1, double b2_, double eps_, double wd)
      : coef(consts[0]), step_size(consts[1]), bc2s(consts[2]), b2(b2_), eps(eps_), omb1(1.0 - b1), omb2(1.0 - b2_), lrwd(lr * wd) {}
};

// p, m, v of one element from its gradient g (multiplied by the clip coefficient where `clip`).  Contraction is pinned: the
// three fused multiply-adds below are the ones the expressions
//   p - lrwd p,   m + omb1 (g - m),   b2 v + omb2 g g
// have always compiled to (-ffp-contract=fast), written out; nothing else may fuse, whatever code surrounds the call
// (profiles/dense3_epilogue.md: a moved load once let the compiler contract an expression and change the last bit).
static __device__ __forceinline__ void egx_adamw_elem(float& p, float g, float& m, float& v, bool clip, const EgxAdamwK& k) {
#pragma clang fp contract(off)
  float gg = g;
  if (clip) gg *= k.coef;
  const double gd = (double)gg, pd = (double)p, md = (double)m;
  float pn = (float)__builtin_fma(-k.lrwd, pd, pd);
  const float mn = (float)__builtin_fma(k.omb1, gd - md, md);
  const float vn = (float)__builtin_fma(k.omb2 * gd, gd, k.b2 * (double)v);
  const float denom = (float)((double)(sqrtf(vn) / k.bc2s) + k.eps);
  pn -= k.step_size * mn / denom;
  p = pn; m = mn; v = vn;
}

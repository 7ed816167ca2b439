// The reparameterised sample of GAMMAPPOPolicy.forward (crowd_ppo/ppo_policy.py:169-178) shared by egx_sample_action (nets.hip) and
// egx_policy_propose (genop_policy.hip): clamp logvar, sigma = exp(logvar)^0.5, act = mu + sigma * eps.
// Force-inlined, so each kernel carries its own copy of the same arithmetic.
#pragma once
#include "egx_common.h"

__device__ __forceinline__ float egx_action_clamp_logvar(float logvar, float min_lv, float max_lv) {
  return fminf(fmaxf(logvar, min_lv), max_lv);
}
__device__ __forceinline__ float egx_action_sigma(float clamped_logvar) { return sqrtf(expf(clamped_logvar)); }
__device__ __forceinline__ float egx_action_sample(float mu, float sigma, float eps) { return mu + sigma * eps; }

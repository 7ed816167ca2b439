// Shared helpers for libegogen_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/egogen_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
__host__ __device__ inline unsigned short egx_bf16_rne(float x) {
  union { float f; unsigned u; } c;
  c.f = x;
  if ((c.u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((c.u >> 16) | 0x40u);
  return (unsigned short)((c.u + 0x7fffu + ((c.u >> 16) & 1u)) >> 16);
}
__host__ __device__ inline float egx_bf16_to_f32(unsigned short h) {
  union { float f; unsigned u; } c;
  c.u = (unsigned)h << 16;
  return c.f;
}


void egx_set_error(const std::string& msg);

#define EGX_HIP_CHECK(expr)                                                                   \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) {                                                                   \
      egx_set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                       \
      return EGX_ERR_HIP;                                                                     \
    }                                                                                         \
  } while (0)

#define EGX_REQUIRE(cond, msg)                                                                \
  do {                                                                                        \
    if (!(cond)) {                                                                            \
      egx_set_error(std::string("argument check failed: ") + #cond + " - " + (msg));          \
      return EGX_ERR_ARG;                                                                     \
    }                                                                                         \
  } while (0)

static inline int egx_ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline size_t egx_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// device copy of a host vector (an empty one still gets an allocation); the caller frees *dptr, also after a failure
template <typename T>
static int egx_upload(T** dptr, const std::vector<T>& h) {
  EGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(dptr), (h.empty() ? 1 : h.size()) * sizeof(T)));
  if (!h.empty()) EGX_HIP_CHECK(hipMemcpy(*dptr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return EGX_OK;
}

// One rounding per operation, whatever the surrounding code: hip-clang's __fmul_rn / __fadd_rn are plain `*` / `+` compiled with
// the default -ffp-contract=fast, i.e. the compiler fuses them into FMAs differently from kernel to kernel (a last-bit
// difference between two kernels that inline the same function).  These are compiled with contraction off.
__device__ __forceinline__ float egx_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float egx_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float egx_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

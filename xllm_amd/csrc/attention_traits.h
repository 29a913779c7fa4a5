// attention_traits.h -- vector types and the per-dtype MFMA / transposed-LDS-read wrappers shared by the decode attention kernels
// (attention_decode.hip, attention_shared_prefix.hip): v_mfma_f32_16x16x32_{bf16,f16} and ds_read_b64_tr_b16.
#pragma once
#include "common.h"

namespace xm {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

template <typename T>
struct AttnTraits;
template <>
struct AttnTraits<bf16_t> {
  using x8 = bf16x8_t;
  using x4 = bf16x4_t;
  using elem = __bf16;
  static __device__ __forceinline__ f32x4_t mfma(x8 a, x8 b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ x4 tr_read(const void* lds_ptr) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) x4*)lds_ptr);
  }
};
template <>
struct AttnTraits<f16_t> {
  using x8 = f16x8_t;
  using x4 = f16x4_t;
  using elem = _Float16;
  static __device__ __forceinline__ f32x4_t mfma(x8 a, x8 b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ x4 tr_read(const void* lds_ptr) {
    typedef __fp16 hfp16x4 __attribute__((__vector_size__(8)));
    hfp16x4 r = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) hfp16x4*)lds_ptr);
    x4 o;
    __builtin_memcpy(&o, &r, 8);
    return o;
  }
};

}  // namespace xm

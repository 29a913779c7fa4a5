// rowwise_fp8.hip -- row-wise producers of the static-scale fp8 layer (xllm_mi355_fp8_static.h): kernels that emit the e4m3
// operand of the next linear instead of the 16-bit value it would be quantised from. With a static per-tensor scale the
// quantisation is element-wise, so there is no row reduction, no LDS and no second pass.
#include "common.h"
#include "xllm_mi355_fp8_static.h"

namespace xm {

// act_and_mul + static e4m3 quant: out_q = e4m3(r16(r16(act(x)) * y) / scale), the cast points of act_and_mul_kernel followed by the
// conversion of fp8_quant_kernel (rowwise.hip), through the same device functions -- byte for byte the two launches, without the
// 16-bit round trip ([T, d] written and read back: 2 x 2 bytes per element against the 1 byte stored here).
// vec: d % 8 == 0 and the bases admit 16-byte loads / 8-byte stores. A thread requests U chunk pairs (U x 2 x 16 bytes, clamped
// index, unconditional) before the first is consumed; gridDim.y workgroups share a row as in act_and_mul_kernel.
// r16(act(x)) as act_and_mul_kernel's code object computes it, last bit and sign of zero included. For f16 hipcc compiles the last
// multiply of act_f and the f16 rounding that follows in act_and_mul_kernel to ONE v_fma_mixlo_f16 with a +0 addend -- in every arm
// but the 16-byte arm of SiLU, which gets v_pk_mul_f32 + v_cvt_pk_f16_f32. The two forms differ on an MI355X: the fused one gives
// act(-0.0) = +0 (a gate of -0.0 is an f16 underflow; the same value, another byte, 0x00 / 0x80, after the multiply by `up`), and it
// disagrees with multiply-then-round in the last f16 bit of a few elements in millions (one rounding instead of two). The contract
// here is the bytes of the operator pair, so both forms are written out: f16(fma(a, b, +0)) over the factors of act_f where the
// pair's kernel fuses, and the f32 product kept a value of its own (the empty asm) where it does not. bf16 has no such
// instruction: multiply, then round, in both kernels.
// pair_vec: the arm act_and_mul_kernel takes for this input into a 16-byte aligned 16-bit tensor (d % 8 == 0, input 16-byte aligned),
// whatever arm this kernel takes for its own output. A template parameter: behind a run-time select hipcc no longer fuses.
template <typename T, int MODE, bool PAIR_VEC>
__device__ __forceinline__ float act_value16(float x) {
  float fa, fb;
  act_factors<MODE>(x, fa, fb);
  if constexpr (__is_same(T, f16_t)) {
    if constexpr (MODE != XM_ACT_SILU || !PAIR_VEC) return (float)(f16_t)__builtin_fmaf(fa, fb, 0.0f);
  }
  float a = fa * fb;
  asm volatile("" : "+v"(a));
  return r16<T>(a);
}

template <typename T, int MODE, bool PAIR_VEC>
__global__ __launch_bounds__(256) void act_and_mul_fp8_kernel(uint8_t* __restrict__ out_q, const T* __restrict__ in,
                                                              const float* __restrict__ scale, int d, bool vec) {
  const int64_t t = blockIdx.x;
  const T* x = in + t * 2 * (int64_t)d;
  const T* y = x + d;
  uint8_t* o = out_q + t * (int64_t)d;
  const float sinv = 1.0f / scale[0];
  if (vec) {
    typedef unsigned avec_t __attribute__((ext_vector_type(4)));
    constexpr int U = 5;
    const int nvec = d / 8;
    for (int c0 = blockIdx.y * U * blockDim.x + threadIdx.x; c0 < nvec; c0 += gridDim.y * U * blockDim.x) {
      avec_t xr[U], yr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = c0 + u * blockDim.x;
        const int cc = c < nvec ? c : c0;
        xr[u] = reinterpret_cast<const avec_t*>(x)[cc];
        yr[u] = reinterpret_cast<const avec_t*>(y)[cc];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = c0 + u * blockDim.x;
        if (c >= nvec) break;
        RowVec<T> xv, yv;
        xv.raw = make_uint4(xr[u][0], xr[u][1], xr[u][2], xr[u][3]);
        yv.raw = make_uint4(yr[u][0], yr[u][1], yr[u][2], yr[u][3]);
        uint32_t pk[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          uint32_t w = 0;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int j = h * 4 + e;
            const float r = r16<T>(act_value16<T, MODE, PAIR_VEC>(xv.get(j)) * yv.get(j));
            w |= (uint32_t)f32_to_e4m3_sat(r * sinv) << (8 * e);
          }
          pk[h] = w;
        }
        reinterpret_cast<uint2*>(o)[c] = make_uint2(pk[0], pk[1]);
      }
    }
  } else {
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < d; i += gridDim.y * blockDim.x)
      o[i] = f32_to_e4m3_sat(r16<T>(act_value16<T, MODE, PAIR_VEC>(to_f32(x[i])) * to_f32(y[i])) * sinv);
  }
}

template <typename T>
static int launch_act_fp8(uint8_t* out_q, const void* input, const float* scale, int64_t n_tokens, int64_t d, int act_mode,
                          hipStream_t s) {
  const bool pair_vec = (d % 8 == 0) && ((uintptr_t)input % 16 == 0);
  const bool vec = pair_vec && ((uintptr_t)out_q % 8 == 0);
  // workgroups per row as launch_act (rowwise.hip): ~4 workgroups per CU when the rows alone are few, each at least one U-chunk
  // batch per thread; the element-wise arm takes one 256-element stride per workgroup instead
  int64_t per_row = (1024 + n_tokens - 1) / n_tokens;
  const int64_t batches = vec ? (d / 8 + 5 * 256 - 1) / (5 * 256) : (d + 255) / 256;
  per_row = per_row > batches ? batches : per_row;
  per_row = per_row < 1 ? 1 : per_row;
  per_row = per_row > 65535 ? 65535 : per_row;
  const dim3 grid((unsigned)n_tokens, (unsigned)per_row);
#define XM_ACT_FP8_(MODE_, PV_) \
  hipLaunchKernelGGL((act_and_mul_fp8_kernel<T, MODE_, PV_>), grid, dim3(256), 0, s, out_q, (const T*)input, scale, (int)d, vec)
#define XM_ACT_FP8(MODE_)            \
  {                                  \
    if (pair_vec) XM_ACT_FP8_(MODE_, true); \
    else XM_ACT_FP8_(MODE_, false);  \
  }
  switch (act_mode) {
    case XM_ACT_SILU: XM_ACT_FP8(XM_ACT_SILU) break;
    case XM_ACT_GELU: XM_ACT_FP8(XM_ACT_GELU) break;
    case XM_ACT_GELU_TANH: XM_ACT_FP8(XM_ACT_GELU_TANH) break;
    default: return XM_ERR_UNSUPPORTED;
  }
#undef XM_ACT_FP8
#undef XM_ACT_FP8_
  return hip_check_launch();
}

}  // namespace xm

using namespace xm;

extern "C" {

int xllm_mi355_act_and_mul_static_fp8_quant(uint8_t* out_q, const void* input, const float* scale, int64_t n_tokens,
                                            int64_t d, int act_mode, int dtype, void* stream) {
  if (!out_q || !input || !scale || n_tokens < 0 || d <= 0) return XM_ERR_INVALID;
  if (dtype != XM_BF16 && dtype != XM_F16) return XM_ERR_UNSUPPORTED;
  if (act_mode != XM_ACT_SILU && act_mode != XM_ACT_GELU && act_mode != XM_ACT_GELU_TANH) return XM_ERR_UNSUPPORTED;
  if (n_tokens > 0x7fffffff || d > 0x3fffffff) return XM_ERR_UNSUPPORTED;   // grid x / the kernel's int column index
  if (n_tokens == 0) return XM_OK;
  XM_DISPATCH_HALF(dtype, T, return launch_act_fp8<T>(out_q, input, scale, n_tokens, d, act_mode, (hipStream_t)stream));
  return XM_OK;
}

}  // extern "C"

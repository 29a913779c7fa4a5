// attention_decode_kv8.hip -- the e4m3 paged KV cache with static per-tensor scales (xllm_mi355_kv_fp8.h): the two KV writers, decode
// attention over such a cache, its launch plan and their C-ABI entry points.
//
// The decode kernel is the 16-bit one (attention_decode.hip) with half the bytes per token row:
//  * one WAVE owns (sequence, kv head, token range), the GQA group is the N dimension of the MFMA, every KV byte leaves HBM once;
//    a workgroup = 4 waves = hpw kv heads x 4 / hpw token sub-ranges merged in LDS, grid-level split-KV partials (o, m, l) in f32
//    merged by a second tiny launch. The plan (hpw, split count) is the 16-bit kernel's: decode_heads_per_wg / decode_num_splits.
//  * e4m3 -> bf16 / f16 is exact, so the codes are converted in registers (v_cvt_pk_f32_fp8 + pack) and the 16-bit MFMAs stay.
//    k_scale is folded into the softmax scale (scores = codes . q * scale * k_scale), v_scale multiplies the normalised output
//    once in the epilogue: beyond the 16-bit kernel's arithmetic there is one f32 multiply on either side.
//  * K: QK^T is a dot product over d, so a lane may take ANY d slice as long as q is loaded under the same permutation. A lane
//    (token p16, group g) takes 16 contiguous bytes of its K row per 64 d -- bytes (c * 4 + g) * 16 .. + 15 of the head -- which
//    feed MFMA k-steps 2c (first 8 codes) and 2c + 1 (last 8); q fragment kk of lane g starts at d = ((kk >> 1) * 4 + g) * 16 +
//    (kk & 1) * 8. 16-byte loads, no LDS round trip for K.
//  * V: whole rows (D bytes: 64 / (D / 16) rows per wave-wide 16-byte load), converted BEFORE the LDS write into the 16-bit
//    row-major padded tile the 16-bit kernel keeps, read back with ds_read_b64_tr_b16.
//  * 32-token tiles are 8 KiB of K + V per wave at d = 128; THREE register stages keep two tiles (16 KiB per wave, what the 16-bit
//    kernel has in flight) outstanding while the third is computed.
//  * every load is unconditional and clamped to kv_len - 1 (no row past kv_len is dereferenced); the prefetches past a wave's range
//    read one row; rows outside [t_lo, kv_len) are zeroed in the V tile and masked to -inf in the scores, so NaN codes (0x7F) in
//    dead rows never reach the result. No workgroup barrier inside the token loop. P = hi + lo.
#include "common.h"
#include "attention_traits.h"
#include "xllm_mi355_kv_fp8.h"

namespace xm {

int decode_num_splits(int64_t batch, int64_t nkv, int hpw, int64_t max_kv_len);  // attention_api.hip
int decode_heads_per_wg(int64_t batch, int64_t nkv);

namespace {

constexpr int kTile8 = 32;           // tokens per tile (= K dim of the PV MFMA)
constexpr float kNegBig8 = -1e30f;   // finite "-inf" for the running max (log2 domain)

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));

// 16 e4m3 codes -> two 8-element 16-bit fragments (codes 0..7, 8..15). Exact: every e4m3fn value is a bf16 and an f16 value.
template <typename TR>
__device__ __forceinline__ void cvt16(const u32x4 raw, typename TR::x8& lo, typename TR::x8& hi) {
  using elem = typename TR::elem;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[w], false);
    const f32x2_t b = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[w], true);
    if (w < 2) {
      lo[w * 4 + 0] = (elem)a[0]; lo[w * 4 + 1] = (elem)a[1]; lo[w * 4 + 2] = (elem)b[0]; lo[w * 4 + 3] = (elem)b[1];
    } else {
      hi[(w - 2) * 4 + 0] = (elem)a[0]; hi[(w - 2) * 4 + 1] = (elem)a[1];
      hi[(w - 2) * 4 + 2] = (elem)b[0]; hi[(w - 2) * 4 + 3] = (elem)b[1];
    }
  }
}

// D = head dim (K and V), UNIFORM: block_size % 32 == 0 so a tile lives in one page
template <typename T, int D, bool UNIFORM>
__global__ __launch_bounds__(256, 2) void paged_decode_kv8_kernel(
    const T* __restrict__ q, const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc, const float* __restrict__ k_scale,
    const float* __restrict__ v_scale, T* __restrict__ out, float* __restrict__ part_o, float* __restrict__ part_ml,
    const int32_t* __restrict__ kv_lens, const int32_t* __restrict__ block_table, int max_blocks, int nq, int nkv, int block_size,
    int64_t q_stride, float scale_log2, int nsplit, int hpw, int window_left, int wide_store) {
  using TR = AttnTraits<T>;
  using x8 = typename TR::x8;
  using x4 = typename TR::x4;
  using elem = typename TR::elem;
  constexpr int KK = D / 32;            // MFMA k-steps over the head dim
  constexpr int NC = D / 64;            // 16-byte K loads per token row and lane
  constexpr int CH = D / 16;            // 16-byte chunks per V row
  constexpr int TPI = 64 / CH;          // V rows fetched per wave-wide load instruction
  constexpr int NV = kTile8 / TPI;      // V load instructions per tile
  constexpr int DB = D / 16;            // 16-wide output d blocks
  constexpr int RSB = D * 2 + 32;       // padded LDS row stride in bytes (16-bit rows)
  constexpr int WAVE_LDS = kTile8 * RSB;
  static_assert(WAVE_LDS >= 16 * D * 4, "epilogue staging must fit");

  __shared__ __attribute__((aligned(16))) char lds[4 * WAVE_LDS];
  __shared__ float ml_sh[4][16][2];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p16 = lane & 15, g = lane >> 4;
  const int nsub = 4 / hpw;
  const int ngroups = nkv / hpw;
  int wg = blockIdx.x;
  const int split = wg % nsplit; wg /= nsplit;
  const int hg = wg % ngroups;
  const int b = wg / ngroups;
  const int hs = wave % hpw, sub = wave / hpw;
  const int kvh = hg * hpw + hs;
  const int G = nq / nkv;

  const int kv_len = kv_lens[b];
  const int t_lo = (window_left >= 0 && kv_len - 1 - window_left > 0) ? kv_len - 1 - window_left : 0;
  const int tile_lo = t_lo / kTile8, tile_hi = (kv_len + kTile8 - 1) / kTile8;
  const int nslots = nsplit * nsub, slot = split * nsub + sub;
  const int ntiles = tile_hi - tile_lo > 0 ? tile_hi - tile_lo : 0;
  const int per = (ntiles + nslots - 1) / nslots;
  int my_lo = tile_lo + slot * per;
  int my_hi = my_lo + per < tile_hi ? my_lo + per : tile_hi;
  my_lo = __builtin_amdgcn_readfirstlane(my_lo);
  my_hi = __builtin_amdgcn_readfirstlane(my_hi);

  const int32_t* bt_row = block_table + (int64_t)b * max_blocks;
  const int64_t row_bytes = (int64_t)nkv * D;  // bytes per token row of the cache
  char* my_lds = lds + wave * WAVE_LDS;
  const float sl2 = scale_log2 * k_scale[0];   // k_scale folded into the softmax scale

  // ---- Q as the MFMA B operand under the d permutation of the K fetch: lane (n = q head p16, group g), k-step kk holds
  //      Q[p16][((kk >> 1) * 4 + g) * 16 + (kk & 1) * 8 .. + 7]
  x8 qf[KK];
  {
    const T* qp = q + (int64_t)b * q_stride + (int64_t)(kvh * G + p16) * D;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      if (p16 < G) qf[kk] = *reinterpret_cast<const x8*>(qp + ((kk >> 1) * 4 + g) * 16 + (kk & 1) * 8);
      else qf[kk] = x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }

  f32x4_t acc_o[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i) acc_o[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m_run = kNegBig8, l_run = 0.0f;

  // three named register stages (never runtime-indexed)
  u32x4 k0[2][NC], k1[2][NC], k2[2][NC];
  u32x4 v0[NV], v1[NV], v2[NV];

  auto page_of_tile = [&](int tile) -> int {  // UNIFORM only: scalar page id of a tile (clamped)
    int idx = (tile * kTile8) / block_size;
    const int last = (kv_len - 1) / block_size;
    idx = idx > last ? last : idx;
    idx = idx < 0 ? 0 : idx;
    return bt_row[idx];
  };
  // every load is unconditional: tokens past kv_len re-load the last token, and a request for a tile at or past my_hi (the
  // prefetches of the iterations that compute the wave's last two tiles: nobody consumes them) reads the FIRST row of the wave's
  // last tile in every lane -- one row instead of a tile. The KV stream is read once per launch: non-temporal loads.
  auto issue_loads = [&](int tile, int page, u32x4 (&kr)[2][NC], u32x4 (&vr)[NV]) {
    const bool past = tile >= my_hi;            // wave-uniform
    tile = past ? my_hi - 1 : tile;
    const int t0 = tile * kTile8;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      int tok = past ? t0 : t0 + blk * 16 + p16;
      tok = tok < kv_len ? tok : kv_len - 1;
      int64_t rowi;
      if constexpr (UNIFORM) rowi = (int64_t)page * block_size + (tok % block_size);
      else rowi = (int64_t)bt_row[tok / block_size] * block_size + (tok % block_size);
      const uint8_t* kp = kc + rowi * row_bytes + (int64_t)kvh * D + g * 16;
#pragma unroll
      for (int c = 0; c < NC; ++c) kr[blk][c] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(kp + c * 64));
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      int tok = past ? t0 : t0 + i * TPI + lane / CH;
      tok = tok < kv_len ? tok : kv_len - 1;
      int64_t rowi;
      if constexpr (UNIFORM) rowi = (int64_t)page * block_size + (tok % block_size);
      else rowi = (int64_t)bt_row[tok / block_size] * block_size + (tok % block_size);
      vr[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(vc + rowi * row_bytes + (int64_t)kvh * D + (lane % CH) * 16));
    }
  };
  auto page_clamped = [&](int tile) -> int {
    if constexpr (UNIFORM) return page_of_tile(tile < my_hi ? tile : my_hi - 1);
    else return 0;
  };

  auto compute_tile = [&](int tile, const u32x4 (&kr)[2][NC], const u32x4 (&vr)[NV]) {
    const int t0 = tile * kTile8;
    const bool partial = (t0 + kTile8 > kv_len) || (t0 < t_lo);

    // ---- K codes -> 16-bit MFMA A-operand fragments, in registers
    x8 kf[2][KK];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
      for (int c = 0; c < NC; ++c) cvt16<TR>(kr[blk][c], kf[blk][2 * c], kf[blk][2 * c + 1]);

    // ---- V tile -> 16 bits -> wave-private LDS (row major, padded rows); rows outside [t_lo, kv_len) zeroed (0 * NaN guard): they
    //      meet p = 0 in the PV MFMA and may hold anything, NaN codes included
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int r = i * TPI + lane / CH;
      x8 va, vb;
      cvt16<TR>(vr[i], va, vb);
      // one unsigned range test for t_lo <= t0 + r < kv_len (t_lo <= kv_len always; a row below t_lo wraps to a huge value)
      if (partial && (unsigned)(t0 - t_lo + r) >= (unsigned)(kv_len - t_lo)) {
        va = x8{0, 0, 0, 0, 0, 0, 0, 0};
        vb = x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
      char* dst = my_lds + r * RSB + (lane % CH) * 32;
      *reinterpret_cast<x8*>(dst) = va;
      *reinterpret_cast<x8*>(dst + 16) = vb;
    }

    // ---- S^T = K * Q^T : lane holds S[q = p16][token = blk*16 + 4g + r]
    f32x4_t s[2];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      s[blk] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) s[blk] = TR::mfma(kf[blk][kk], qf[kk], s[blk]);
    }
    // ---- online softmax (log2 domain), lane-local except the 2 cross-group maxima
    float mx = kNegBig8;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = s[blk][r] * sl2;
        if (partial) {
          const int tok = t0 + blk * 16 + g * 4 + r;
          if (tok >= kv_len || tok < t_lo) v = -INFINITY;
        }
        s[blk][r] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);
    const float alpha = exp2f(m_run - m_new);
    m_run = m_new;
    float psum = 0.0f;
    // P as hi + lo 16-bit parts (p = hi + lo to ~2^-17 relative), as in the 16-bit kernel
    x8 pf, pl;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = exp2f(s[blk][r] - m_new);
        psum += p;
        const elem hi = (elem)p;
        pf[blk * 4 + r] = hi;
        pl[blk * 4 + r] = (elem)(p - (float)hi);
      }
    l_run = l_run * alpha + psum;
#pragma unroll
    for (int i = 0; i < DB; ++i) acc_o[i] *= alpha;

    // ---- O^T += V^T * P^T : A = V^T via transposed LDS reads, k slot (g, j): j<4 -> token 4g+j, j>=4 -> token 16+4g+(j-4)
    const char* trb = my_lds + (4 * g + (p16 >> 2)) * RSB + (p16 & 3) * 8;
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      x4 lo = TR::tr_read(trb + db * 32);
      x4 hi = TR::tr_read(trb + 16 * RSB + db * 32);
      x8 vt;
      vt[0] = lo[0]; vt[1] = lo[1]; vt[2] = lo[2]; vt[3] = lo[3];
      vt[4] = hi[0]; vt[5] = hi[1]; vt[6] = hi[2]; vt[7] = hi[3];
      acc_o[db] = TR::mfma(vt, pf, acc_o[db]);
      acc_o[db] = TR::mfma(vt, pl, acc_o[db]);
    }
  };

  if (my_lo < my_hi) {
    int tile = my_lo;
    int pg2 = page_clamped(my_lo + 2), pg3;
    issue_loads(my_lo, page_clamped(my_lo), k0, v0);
    issue_loads(my_lo + 1, page_clamped(my_lo + 1), k1, v1);
    while (true) {
      pg3 = page_clamped(tile + 3);
      issue_loads(tile + 2, pg2, k2, v2);
      compute_tile(tile, k0, v0);
      pg2 = pg3;
      if (++tile >= my_hi) break;
      pg3 = page_clamped(tile + 3);
      issue_loads(tile + 2, pg2, k0, v0);
      compute_tile(tile, k1, v1);
      pg2 = pg3;
      if (++tile >= my_hi) break;
      pg3 = page_clamped(tile + 3);
      issue_loads(tile + 2, pg2, k1, v1);
      compute_tile(tile, k2, v2);
      pg2 = pg3;
      if (++tile >= my_hi) break;
    }
  }

  // ---- epilogue: stage (m, l, O) of every wave in LDS, merge the sub-ranges of each head (the 16-bit kernel's one-pass form)
  l_run += __shfl_xor(l_run, 16);
  l_run += __shfl_xor(l_run, 32);
  {
    float* o_st = reinterpret_cast<float*>(my_lds);
#pragma unroll
    for (int db = 0; db < DB; ++db)
      *reinterpret_cast<f32x4_t*>(o_st + p16 * D + db * 16 + g * 4) = acc_o[db];
    if (g == 0) { ml_sh[wave][p16][0] = m_run; ml_sh[wave][p16][1] = l_run; }
  }
  __syncthreads();
  // work items (head slot h_s, live query head qq < G, 8 consecutive d): hpw * G * D / 8 of them, at most 1024
  constexpr int DPI = D / 8;
  const int nitems = hpw * G * DPI;
  const float vs = v_scale[0];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int item = threadIdx.x + it * 256;
    if (item < nitems) {
      const int hq = item / DPI, d = (item % DPI) * 8;
      const int h_s = hq / G, qq = hq - h_s * G;
      float mw[4], lw[4];
      float m_star = kNegBig8;
#pragma unroll
      for (int sb = 0; sb < 4; ++sb)
        if (sb < nsub) {
          const float2 ml = *reinterpret_cast<const float2*>(&ml_sh[sb * hpw + h_s][qq][0]);
          mw[sb] = ml.x;
          lw[sb] = ml.y;
          m_star = fmaxf(m_star, ml.x);
        }
      float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      float l = 0.0f;
#pragma unroll
      for (int sb = 0; sb < 4; ++sb)
        if (sb < nsub) {
          const float f = exp2f(mw[sb] - m_star);
          const float* op = reinterpret_cast<const float*>(lds + (sb * hpw + h_s) * WAVE_LDS) + qq * D + d;
          const f32x4_t oa = *reinterpret_cast<const f32x4_t*>(op), ob = *reinterpret_cast<const f32x4_t*>(op + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            o[j] += f * oa[j];
            o[4 + j] += f * ob[j];
          }
          l += f * lw[sb];
        }
      const int head = (hg * hpw + h_s) * G + qq;
      if (nsplit > 1) {  // grid-level split-KV: (o, m, l) of this range, in code units (v_scale is applied by the merge)
        const int64_t pi = ((int64_t)b * nq + head) * nsplit + split;
        float* po = part_o + pi * D + d;
        if (wide_store) {
          *reinterpret_cast<f32x4_t*>(po) = f32x4_t{o[0], o[1], o[2], o[3]};
          *reinterpret_cast<f32x4_t*>(po + 4) = f32x4_t{o[4], o[5], o[6], o[7]};
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) po[j] = o[j];
        }
        if (d == 0) { part_ml[pi * 2] = m_star; part_ml[pi * 2 + 1] = l; }
      } else {
        u32x4 pk = {0u, 0u, 0u, 0u};
        T t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          t[j] = from_f32<T>(l > 0.0f ? o[j] / l * vs : 0.0f);
          uint16_t bits;
          __builtin_memcpy(&bits, &t[j], 2);
          pk[j >> 1] |= (unsigned)bits << ((j & 1) * 16);
        }
        T* op16 = out + (int64_t)b * nq * D + (int64_t)head * D + d;
        if (wide_store) *reinterpret_cast<u32x4*>(op16) = pk;
        else {
#pragma unroll
          for (int j = 0; j < 8; ++j) op16[j] = t[j];
        }
      }
    }
  }
}

// merge of the grid-level split-KV partials: one workgroup (D threads) per (sequence, head); v_scale applied to the quotient
template <typename T, int D>
__global__ void paged_decode_kv8_merge_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                              const float* __restrict__ v_scale, T* __restrict__ out, int nq, int nsplit) {
  const int b = blockIdx.x / nq, head = blockIdx.x % nq;
  const int d = threadIdx.x;
  const int64_t base = ((int64_t)b * nq + head) * nsplit;
  float m_star = kNegBig8;
  for (int s = 0; s < nsplit; ++s) m_star = fmaxf(m_star, part_ml[(base + s) * 2]);
  float o = 0.0f, l = 0.0f;
  for (int s = 0; s < nsplit; ++s) {
    const float f = exp2f(part_ml[(base + s) * 2] - m_star);
    o += f * part_o[(base + s) * D + d];
    l += f * part_ml[(base + s) * 2 + 1];
  }
  out[(int64_t)b * nq * D + (int64_t)head * D + d] = from_f32<T>(l > 0.0f ? o / l * v_scale[0] : 0.0f);
}

// ---- the launch plan: ONE function for the launcher and for xllm_mi355_paged_decode_kv8_plan
struct Kv8Plan {
  int hpw, nsplit_planned, nsplit, uniform;
};
Kv8Plan kv8_plan(int64_t batch, int64_t nq, int64_t nkv, int64_t head_dim, int64_t block_size, int64_t max_kv_len,
                 size_t ws_bytes) {
  Kv8Plan p;
  p.hpw = decode_heads_per_wg(batch, nkv);
  p.nsplit_planned = decode_num_splits(batch, nkv, p.hpw, max_kv_len);
  // degrade the split count to what the caller's workspace holds (1 split needs none)
  const size_t per_split = (size_t)batch * nq * (head_dim + 2) * sizeof(float);
  int n = p.nsplit_planned;
  if ((size_t)n * per_split > ws_bytes) n = (int)(ws_bytes / per_split);
  p.nsplit = n < 1 ? 1 : n;
  p.uniform = block_size % kTile8 == 0 ? 1 : 0;
  return p;
}

template <typename T, int D>
int launch_paged_decode_kv8(const void* q, const uint8_t* kc, const uint8_t* vc, const float* k_scale, const float* v_scale,
                            void* out, const int32_t* kv_lens, const int32_t* block_table, int64_t max_blocks, int64_t batch,
                            int64_t nq, int64_t nkv, int64_t block_size, int64_t q_stride, int64_t max_kv_len, float scale,
                            int64_t window_left, void* workspace, size_t ws_bytes, hipStream_t s) {
  const Kv8Plan p = kv8_plan(batch, nq, nkv, D, block_size, max_kv_len, workspace ? ws_bytes : 0);
  const int nsplit = p.nsplit;
  float* part_o = nsplit > 1 ? reinterpret_cast<float*>(workspace) : nullptr;
  float* part_ml = part_o ? part_o + (size_t)batch * nq * nsplit * D : nullptr;
  const float scale_log2 = scale * 1.4426950408889634f;
  const dim3 grid((unsigned)(batch * (nkv / p.hpw) * nsplit));
  const int wl = window_left < 0 ? -1 : (window_left > 0x3fffffff ? 0x3fffffff : (int)window_left);
  const int wide_store = nsplit > 1 ? (uintptr_t)part_o % 16 == 0 : (uintptr_t)out % 16 == 0;
#define XM_KV8_LAUNCH(UNI_)                                                                                                   \
  hipLaunchKernelGGL((paged_decode_kv8_kernel<T, D, UNI_>), grid, dim3(256), 0, s, (const T*)q, kc, vc, k_scale, v_scale,     \
                     (T*)out, part_o, part_ml, kv_lens, block_table, (int)max_blocks, (int)nq, (int)nkv, (int)block_size,     \
                     q_stride, scale_log2, nsplit, p.hpw, wl, wide_store)
  if (p.uniform) XM_KV8_LAUNCH(true);
  else XM_KV8_LAUNCH(false);
#undef XM_KV8_LAUNCH
  if (nsplit > 1)
    hipLaunchKernelGGL((paged_decode_kv8_merge_kernel<T, D>), dim3((unsigned)(batch * nq)), dim3(D), 0, s, part_o, part_ml,
                       v_scale, (T*)out, (int)nq, nsplit);
  return hip_check_launch();
}

// ------------------------------------------------------------------------------------------------ KV writers
// 8 consecutive 16-bit values -> 8 e4m3 codes, the expressions of fp8_quant_kernel (rowwise.hip)
template <typename T>
__device__ __forceinline__ uint2 quant8(const uint4 raw, float sinv) {
  RowVec<T> v;
  v.raw = raw;
  uint32_t pk[2];
#pragma unroll
  for (int j = 0; j < 8; j += 4) {
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) w |= (uint32_t)f32_to_e4m3_sat(v.get(j + e) * sinv) << (8 * e);
    pk[j / 4] = w;
  }
  return make_uint2(pk[0], pk[1]);
}

// one workgroup per token: static_scaled_fp8_quant of the k and v rows, scattered to the slot. VEC: rows of a multiple of 8
// elements with 16-byte aligned sources and 8-byte aligned cache rows
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void reshape_paged_cache_kv8_kernel(
    const int32_t* __restrict__ slot_ids, const T* __restrict__ k, const T* __restrict__ v, uint8_t* __restrict__ kc,
    uint8_t* __restrict__ vc, const float* __restrict__ k_scale, const float* __restrict__ v_scale, int row, int64_t k_stride,
    int64_t v_stride, int64_t block_size, int64_t n_blocks) {
  const int64_t t = blockIdx.x;
  const int64_t slot = slot_ids[t];
  if (slot < 0) return;
  if (slot / block_size >= n_blocks) return;
  const float ksi = 1.0f / k_scale[0], vsi = 1.0f / v_scale[0];
  const T* ks = k + t * k_stride;
  const T* vs = v + t * v_stride;
  uint8_t* kd = kc + slot * (int64_t)row;
  uint8_t* vd = vc + slot * (int64_t)row;
  if constexpr (VEC) {
    for (int i = threadIdx.x; i < row / 8; i += blockDim.x) {
      reinterpret_cast<uint2*>(kd)[i] = quant8<T>(reinterpret_cast<const uint4*>(ks)[i], ksi);
      reinterpret_cast<uint2*>(vd)[i] = quant8<T>(reinterpret_cast<const uint4*>(vs)[i], vsi);
    }
  } else {
    for (int i = threadIdx.x; i < row; i += blockDim.x) {
      kd[i] = f32_to_e4m3_sat(to_f32(ks[i]) * ksi);
      vd[i] = f32_to_e4m3_sat(to_f32(vs[i]) * vsi);
    }
  }
}

// RoPE on q, k in place with the arithmetic of rope_kernel (rowwise.hip), the rotated k (rounded to T as it is stored) and v
// quantised into the cache: rotary_embedding -> static_scaled_fp8_quant -> scatter, byte for byte
template <typename T, bool NEOX>
__global__ __launch_bounds__(256) void rope_and_cache_kv8_kernel(
    const int64_t* __restrict__ positions, T* __restrict__ q, T* __restrict__ k, const T* __restrict__ v,
    const T* __restrict__ cache, const int32_t* __restrict__ slot_ids, uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
    const float* __restrict__ k_scale, const float* __restrict__ v_scale, int rot_dim, int64_t q_stride, int64_t k_stride,
    int64_t v_stride, int head_size, int nq, int nk, int64_t block_size, int64_t n_blocks, int v_vec) {
  const int64_t t = blockIdx.x;
  const int half = rot_dim >> 1;
  const T* cp = cache + positions[t] * rot_dim;
  const int64_t slot = slot_ids[t];
  const bool store = slot >= 0 && slot / block_size < n_blocks;
  const float ksi = 1.0f / k_scale[0], vsi = 1.0f / v_scale[0];
  uint8_t* kc_row = kc + slot * (int64_t)nk * head_size;
  uint8_t* vc_row = vc + slot * (int64_t)nk * head_size;
  const int total = (nq + nk) * half;
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    const int h = i / half, j = i - h * half;
    const bool is_k = h >= nq;
    T* arr = is_k ? k + t * k_stride + (int64_t)(h - nq) * head_size : q + t * q_stride + (int64_t)h * head_size;
    const int xi = NEOX ? j : 2 * j, yi = NEOX ? half + j : 2 * j + 1;
    const float c = to_f32(cp[j]), s = to_f32(cp[half + j]);
    const float x = to_f32(arr[xi]), y = to_f32(arr[yi]);
    const T nx = from_f32<T>(r16<T>(x * c) - r16<T>(y * s));
    const T ny = from_f32<T>(r16<T>(y * c) + r16<T>(x * s));
    arr[xi] = nx;
    arr[yi] = ny;
    if (is_k && store) {
      kc_row[(h - nq) * head_size + xi] = f32_to_e4m3_sat(to_f32(nx) * ksi);
      kc_row[(h - nq) * head_size + yi] = f32_to_e4m3_sat(to_f32(ny) * ksi);
    }
  }
  if (!store) return;
  // un-rotated tail of k (rot_dim < head_size) and the whole v row
  const int tail = head_size - rot_dim;
  for (int i = threadIdx.x; i < nk * tail; i += blockDim.x) {
    const int h = i / tail, e = rot_dim + (i - h * tail);
    kc_row[h * head_size + e] = f32_to_e4m3_sat(to_f32(k[t * k_stride + (int64_t)h * head_size + e]) * ksi);
  }
  const int row = nk * head_size;
  const T* vs = v + t * v_stride;
  if (v_vec) {
    for (int i = threadIdx.x; i < row / 8; i += blockDim.x)
      reinterpret_cast<uint2*>(vc_row)[i] = quant8<T>(reinterpret_cast<const uint4*>(vs)[i], vsi);
  } else {
    for (int i = threadIdx.x; i < row; i += blockDim.x) vc_row[i] = f32_to_e4m3_sat(to_f32(vs[i]) * vsi);
  }
}

}  // namespace
}  // namespace xm

using namespace xm;

extern "C" {

int xllm_mi355_reshape_paged_cache_kv8(const int32_t* slot_ids, const void* k, const void* v, uint8_t* k_cache, uint8_t* v_cache,
                                       const float* k_scale, const float* v_scale, int64_t n_tokens, int64_t n_kv_heads,
                                       int64_t head_dim, int64_t block_size, int64_t n_blocks, int64_t k_stride, int64_t v_stride,
                                       int dtype, void* stream) {
  if (!slot_ids || !k || !v || !k_cache || !v_cache || !k_scale || !v_scale || n_tokens < 0 || n_kv_heads <= 0 || head_dim <= 0 ||
      block_size <= 0)
    return XM_ERR_INVALID;
  if (dtype != XM_BF16 && dtype != XM_F16) return XM_ERR_UNSUPPORTED;
  if (n_tokens == 0) return XM_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t row = n_kv_heads * head_dim;
  const bool vec = row % 8 == 0 && k_stride % 8 == 0 && v_stride % 8 == 0 && (uintptr_t)k % 16 == 0 && (uintptr_t)v % 16 == 0 &&
                   (uintptr_t)k_cache % 8 == 0 && (uintptr_t)v_cache % 8 == 0;
  XM_DISPATCH_HALF(dtype, T, {
    if (vec)
      hipLaunchKernelGGL((reshape_paged_cache_kv8_kernel<T, true>), dim3(n_tokens), dim3(256), 0, s, slot_ids, (const T*)k,
                         (const T*)v, k_cache, v_cache, k_scale, v_scale, (int)row, k_stride, v_stride, block_size, n_blocks);
    else
      hipLaunchKernelGGL((reshape_paged_cache_kv8_kernel<T, false>), dim3(n_tokens), dim3(256), 0, s, slot_ids, (const T*)k,
                         (const T*)v, k_cache, v_cache, k_scale, v_scale, (int)row, k_stride, v_stride, block_size, n_blocks);
  });
  return hip_check_launch();
}

int xllm_mi355_rotary_embedding_and_cache_kv8(const int64_t* positions, void* q, void* k, const void* v, const void* cos_sin_cache,
                                              const int32_t* slot_ids, uint8_t* k_cache, uint8_t* v_cache, const float* k_scale,
                                              const float* v_scale, int64_t n_tokens, int64_t n_q_heads, int64_t n_kv_heads,
                                              int64_t head_size, int64_t rot_dim, int64_t q_stride, int64_t k_stride,
                                              int64_t v_stride, int64_t block_size, int64_t n_blocks, int is_neox, int dtype,
                                              void* stream) {
  if (!positions || !q || !k || !v || !cos_sin_cache || !slot_ids || !k_cache || !v_cache || !k_scale || !v_scale ||
      n_tokens < 0 || rot_dim <= 0 || (rot_dim & 1) || rot_dim > head_size || block_size <= 0)
    return XM_ERR_INVALID;
  if (dtype != XM_BF16 && dtype != XM_F16) return XM_ERR_UNSUPPORTED;
  if (n_tokens == 0) return XM_OK;
  hipStream_t s = (hipStream_t)stream;
  const int v_vec = (n_kv_heads * head_size) % 8 == 0 && v_stride % 8 == 0 && (uintptr_t)v % 16 == 0 && (uintptr_t)v_cache % 8 == 0;
  XM_DISPATCH_HALF(dtype, T, {
    if (is_neox)
      hipLaunchKernelGGL((rope_and_cache_kv8_kernel<T, true>), dim3(n_tokens), dim3(256), 0, s, positions, (T*)q, (T*)k,
                         (const T*)v, (const T*)cos_sin_cache, slot_ids, k_cache, v_cache, k_scale, v_scale, (int)rot_dim,
                         q_stride, k_stride, v_stride, (int)head_size, (int)n_q_heads, (int)n_kv_heads, block_size, n_blocks,
                         v_vec);
    else
      hipLaunchKernelGGL((rope_and_cache_kv8_kernel<T, false>), dim3(n_tokens), dim3(256), 0, s, positions, (T*)q, (T*)k,
                         (const T*)v, (const T*)cos_sin_cache, slot_ids, k_cache, v_cache, k_scale, v_scale, (int)rot_dim,
                         q_stride, k_stride, v_stride, (int)head_size, (int)n_q_heads, (int)n_kv_heads, block_size, n_blocks,
                         v_vec);
  });
  return hip_check_launch();
}

int xllm_mi355_paged_decode_kv8_plan(int64_t batch, int64_t n_q_heads, int64_t n_kv_heads, int64_t head_dim, int64_t block_size,
                                     int64_t max_kv_len, size_t workspace_bytes, int32_t* hpw, int32_t* nsplit_planned,
                                     int32_t* nsplit, int32_t* uniform) {
  if (batch <= 0 || n_q_heads <= 0 || n_kv_heads <= 0 || n_q_heads % n_kv_heads || block_size <= 0 || max_kv_len < 0)
    return XM_ERR_INVALID;
  if (head_dim != 64 && head_dim != 128) return XM_ERR_UNSUPPORTED;
  const Kv8Plan p = kv8_plan(batch, n_q_heads, n_kv_heads, head_dim, block_size, max_kv_len, workspace_bytes);
  if (hpw) *hpw = p.hpw;
  if (nsplit_planned) *nsplit_planned = p.nsplit_planned;
  if (nsplit) *nsplit = p.nsplit;
  if (uniform) *uniform = p.uniform;
  return XM_OK;
}

int xllm_mi355_paged_decode_attention_kv8(const void* q, const uint8_t* k_cache, const uint8_t* v_cache, const float* k_scale,
                                          const float* v_scale, void* out, const int32_t* kv_lens, const int32_t* block_table,
                                          int64_t max_blocks, int64_t batch, int64_t n_q_heads, int64_t n_kv_heads,
                                          int64_t head_dim, int64_t block_size, int64_t n_blocks, int64_t q_stride,
                                          int64_t max_kv_len, float scale, int64_t window_left, int dtype, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  (void)n_blocks;
  if (!q || !k_cache || !v_cache || !k_scale || !v_scale || !out || !kv_lens || !block_table) return XM_ERR_INVALID;
  if (batch < 0 || n_q_heads <= 0 || n_kv_heads <= 0 || n_q_heads % n_kv_heads || block_size <= 0 || max_blocks <= 0)
    return XM_ERR_INVALID;
  if ((head_dim != 64 && head_dim != 128) || n_q_heads / n_kv_heads > 16 || (dtype != XM_BF16 && dtype != XM_F16))
    return XM_ERR_UNSUPPORTED;
  if ((uintptr_t)q % 16 || (uintptr_t)k_cache % 16 || (uintptr_t)v_cache % 16 || q_stride % 8) return XM_ERR_UNSUPPORTED;
  if (batch == 0) return XM_OK;
  hipStream_t s = (hipStream_t)stream;
#define XM_DECODE_KV8(T, DD)                                                                                                  \
  return launch_paged_decode_kv8<T, DD>(q, k_cache, v_cache, k_scale, v_scale, out, kv_lens, block_table, max_blocks, batch,  \
                                        n_q_heads, n_kv_heads, block_size, q_stride, max_kv_len, scale, window_left, workspace, \
                                        workspace ? workspace_bytes : 0, s)
  if (dtype == XM_BF16 && head_dim == 128) XM_DECODE_KV8(bf16_t, 128);
  if (dtype == XM_BF16 && head_dim == 64) XM_DECODE_KV8(bf16_t, 64);
  if (dtype == XM_F16 && head_dim == 128) XM_DECODE_KV8(f16_t, 128);
  if (dtype == XM_F16 && head_dim == 64) XM_DECODE_KV8(f16_t, 64);
#undef XM_DECODE_KV8
  return XM_ERR_UNSUPPORTED;
}

}  // extern "C"

// attention_prefill.hip -- causal varlen flash attention for prefill (packed K/V) and chunked prefill
// (K/V gathered from the paged cache through the block table) on gfx950.
//
// Reference semantics: FlashAttentionImpl::prefill_forward / paged_forward(is_chunked_prefill=true)
// (xllm/core/layers/dcu/flash_attention.cpp:167-288) == TorchAttentionImpl prefill / chunked branches
// (layers/dcu/torch_attention.cpp:152-277) with BOTTOM-RIGHT aligned causal masks: query i of a chunk
// of q_len sees keys j <= kv_len - q_len + i (SURVEY.md 8c caveat 2); window_left >= 0 additionally
// hides keys j < pos - window_left.
//
// Structure: one workgroup (4 waves) per (sequence, q head, block of 128 queries); each wave owns 32
// queries as two N=16 MFMA column blocks. K/V tiles of 32 tokens are staged global -> registers -> LDS
// (next tile in flight during the MFMAs, two LDS buffers, one barrier per tile). As in the decode kernel
// S^T = K Q^T and O^T = V^T P^T so softmax state is lane-local: each lane owns one query of each block.
// K fragments: ds_read_b128 from rows padded by 16 B; V^T fragments: ds_read_b64_tr_b16 from rows
// padded by 32 B.
#include <stdlib.h>

#include "common.h"

namespace xm {

typedef __bf16 pbf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 pbf16x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 pf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 pf16x4_t __attribute__((ext_vector_type(4)));
typedef float pf32x4_t __attribute__((ext_vector_type(4)));

template <typename T>
struct PfTraits;
template <>
struct PfTraits<bf16_t> {
  using x8 = pbf16x8_t;
  using x4 = pbf16x4_t;
  using elem = __bf16;
  static __device__ __forceinline__ pf32x4_t mfma(x8 a, x8 b, pf32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ x4 tr_read(const void* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) x4*)p);
  }
};
template <>
struct PfTraits<f16_t> {
  using x8 = pf16x8_t;
  using x4 = pf16x4_t;
  using elem = _Float16;
  static __device__ __forceinline__ pf32x4_t mfma(x8 a, x8 b, pf32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ x4 tr_read(const void* p) {
    typedef __fp16 hfp16x4 __attribute__((__vector_size__(8)));
    hfp16x4 r = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) hfp16x4*)p);
    x4 o;
    __builtin_memcpy(&o, &r, 8);
    return o;
  }
};

constexpr int kPfTile = 32;
constexpr int kPfQBlock = 128;
constexpr float kPfNegBig = -1e30f;

template <typename T, int D, bool PAGED>
__global__ __launch_bounds__(256, 2) void flash_prefill_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, T* __restrict__ out,
    const int32_t* __restrict__ cu_q, const int32_t* __restrict__ cu_k, const int32_t* __restrict__ kv_lens,
    const int32_t* __restrict__ block_table, int max_blocks, int nq, int nkv, int block_size, int64_t q_stride,
    int64_t k_stride, int64_t v_stride, float scale_log2, int causal, int window_left) {
  using TR = PfTraits<T>;
  using x8 = typename TR::x8;
  using x4 = typename TR::x4;
  using elem = typename TR::elem;
  constexpr int KK = D / 32, CH = D * 2 / 16, DB = D / 16;
  constexpr int NLD = kPfTile * CH / 256;  // 16-B chunks per thread per tile and operand
  constexpr int RSK = D * 2 + 16, RSV = D * 2 + 32;
  static_assert(NLD >= 1, "head dim too small");
  __shared__ __attribute__((aligned(16))) char lds[2][kPfTile * RSK + kPfTile * RSV];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p16 = lane & 15, g = lane >> 4;
  const int h = blockIdx.x, b = blockIdx.z;
  const int qb = gridDim.y - 1 - blockIdx.y;  // heaviest (latest) causal blocks first
  const int q_start = cu_q[b], q_len = cu_q[b + 1] - q_start;
  const int q0 = qb * kPfQBlock;
  if (q0 >= q_len) return;
  const int kv_len = PAGED ? kv_lens[b] : (cu_k[b + 1] - cu_k[b]);
  const int k_start = PAGED ? 0 : cu_k[b];
  const int G = nq / nkv, kvh = h / G;
  const int kvoff = kv_len - q_len;  // position of query 0 (bottom-right alignment)

  // tile range of the workgroup
  int q_hi = q0 + kPfQBlock < q_len ? q0 + kPfQBlock : q_len;  // exclusive
  int hi_tok = kv_len;
  if (causal) { int c = kvoff + q_hi; hi_tok = c < kv_len ? c : kv_len; }
  if (hi_tok < 0) hi_tok = 0;
  int lo_tok = 0;
  if (window_left >= 0) { lo_tok = kvoff + q0 - window_left; lo_tok = lo_tok > 0 ? lo_tok : 0; }
  const int tile_lo = lo_tok / kPfTile, tile_hi = (hi_tok + kPfTile - 1) / kPfTile;

  const int32_t* bt_row = PAGED ? block_table + (int64_t)b * max_blocks : nullptr;
  const int64_t row_elems = (int64_t)nkv * D;
  auto k_row_ptr = [&](int tok) -> const T* {
    tok = tok < kv_len ? tok : kv_len - 1;
    tok = tok < 0 ? 0 : tok;
    if constexpr (PAGED) return k + ((int64_t)bt_row[tok / block_size] * block_size + tok % block_size) * row_elems + (int64_t)kvh * D;
    else return k + (int64_t)(k_start + tok) * k_stride + (int64_t)kvh * D;
  };
  auto v_row_ptr = [&](int tok) -> const T* {
    tok = tok < kv_len ? tok : kv_len - 1;
    tok = tok < 0 ? 0 : tok;
    if constexpr (PAGED) return v + ((int64_t)bt_row[tok / block_size] * block_size + tok % block_size) * row_elems + (int64_t)kvh * D;
    else return v + (int64_t)(k_start + tok) * v_stride + (int64_t)kvh * D;
  };

  // Q fragments (B operand): lane (n = query p16 of block nb, k group g)
  x8 qf[2][KK];
  int qidx[2];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    qidx[nb] = q0 + wave * 32 + nb * 16 + p16;
    const bool ok = qidx[nb] < q_len;
    const T* qp = q + (int64_t)(q_start + (ok ? qidx[nb] : 0)) * q_stride + (int64_t)h * D;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      if (ok) qf[nb][kk] = *reinterpret_cast<const x8*>(qp + (kk * 4 + g) * 8);
      else qf[nb][kk] = x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  // wave-level query position bounds (for tile skipping / mask detection)
  const int wq_lo = kvoff + q0 + wave * 32;
  int wq_hi = kvoff + (q0 + wave * 32 + 31 < q_len - 1 ? q0 + wave * 32 + 31 : q_len - 1);
  const bool wave_active = (q0 + wave * 32) < q_len;

  pf32x4_t acc_o[2][DB];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int i = 0; i < DB; ++i) acc_o[nb][i] = pf32x4_t{0.f, 0.f, 0.f, 0.f};
  float m_run[2] = {kPfNegBig, kPfNegBig}, l_run[2] = {0.f, 0.f};

  uint4 rk[NLD], rv[NLD];
  auto load_global = [&](int tile) {
    const int t0 = tile * kPfTile;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int c = tid + i * 256, row = c / CH, col = c % CH;
      rk[i] = *reinterpret_cast<const uint4*>(k_row_ptr(t0 + row) + col * 8);
      rv[i] = *reinterpret_cast<const uint4*>(v_row_ptr(t0 + row) + col * 8);
    }
  };
  auto write_lds = [&](int buf, int tile) {
    const int t0 = tile * kPfTile;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int c = tid + i * 256, row = c / CH, col = c % CH;
      *reinterpret_cast<uint4*>(&lds[buf][row * RSK + col * 16]) = rk[i];
      uint4 vv = rv[i];
      // 0 * NaN guard for keys every query of the block masks: the rows past kv_len and, in the window's edge tile, the rows
      // below lo_tok (with pages shorter than the tile they may come from a page the cache has already recycled). One
      // unsigned range test for lo_tok <= t0 + row < kv_len (lo_tok <= kv_len always; a row below lo_tok wraps to a huge value)
      if ((unsigned)(t0 + row - lo_tok) >= (unsigned)(kv_len - lo_tok)) vv = make_uint4(0, 0, 0, 0);
      *reinterpret_cast<uint4*>(&lds[buf][kPfTile * RSK + row * RSV + col * 16]) = vv;
    }
  };

  if (tile_lo < tile_hi) {
    load_global(tile_lo);
    write_lds(0, tile_lo);
    __syncthreads();
    int cur = 0;
    for (int tile = tile_lo; tile < tile_hi; ++tile) {
      const bool more = tile + 1 < tile_hi;
#ifndef XM_ABL_PF_NOSTAGE  /* ablation builds (tools/build_ablations.sh): timing only, results are wrong */
      if (more) load_global(tile + 1);
#endif
      const int t0 = tile * kPfTile;
      const bool compute = wave_active && (!causal || t0 <= wq_hi) && (window_left < 0 || t0 + kPfTile > wq_lo - window_left);
      if (compute) {
        const char* lk = lds[cur];
        const char* lv = lds[cur] + kPfTile * RSK;
        pf32x4_t s[2][2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
          for (int blk = 0; blk < 2; ++blk) s[nb][blk] = pf32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
          for (int kk = 0; kk < KK; ++kk) {
            const x8 ka = *reinterpret_cast<const x8*>(lk + (blk * 16 + p16) * RSK + (kk * 4 + g) * 16);
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) s[nb][blk] = TR::mfma(ka, qf[nb][kk], s[nb][blk]);
          }
        const bool need_mask = (t0 + kPfTile > kv_len) || (causal && t0 + kPfTile - 1 > wq_lo) ||
                               (window_left >= 0 && t0 < wq_hi - window_left);
        x8 pf[2], pl[2];  // P = hi + lo 16-bit parts (see attention_decode.hip)
#ifdef XM_ABL_PF_NOSOFTMAX
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
          for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              pf[nb][blk * 4 + r] = (elem)s[nb][blk][r];
              pl[nb][blk * 4 + r] = (elem)s[nb][blk][r];
            }
        (void)need_mask;
#else
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          const int qpos = kvoff + qidx[nb];
          float mx = kPfNegBig;
#pragma unroll
          for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float val = s[nb][blk][r] * scale_log2;
              if (need_mask) {
                const int tok = t0 + blk * 16 + g * 4 + r;
                const bool vis = tok < kv_len && (!causal || tok <= qpos) && (window_left < 0 || tok >= qpos - window_left);
                if (!vis) val = -INFINITY;
              }
              s[nb][blk][r] = val;
              mx = fmaxf(mx, val);
            }
          mx = fmaxf(mx, __shfl_xor(mx, 16));
          mx = fmaxf(mx, __shfl_xor(mx, 32));
          const float m_new = fmaxf(m_run[nb], mx);
          const float alpha = __builtin_amdgcn_exp2f(m_run[nb] - m_new);  // v_exp_f32: results below 2^-126 flush to 0
          m_run[nb] = m_new;
          float psum = 0.0f;
#pragma unroll
          for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float p = __builtin_amdgcn_exp2f(s[nb][blk][r] - m_new);
              psum += p;
              const elem hi = (elem)p;
              pf[nb][blk * 4 + r] = hi;
              pl[nb][blk * 4 + r] = (elem)(p - (float)hi);
            }
          l_run[nb] = l_run[nb] * alpha + psum;
          // the running maximum settles after a few tiles; once no lane of the wave raised it, alpha == 1 everywhere
          // and the DB*4 multiplies are skipped (wave-uniform branch; multiplying by 1.0f is exact, so same bits)
          if (__any(alpha != 1.0f)) {
#pragma unroll
            for (int i = 0; i < DB; ++i) acc_o[nb][i] *= alpha;
          }
        }
#endif
        const char* trb = lv + (4 * g + (p16 >> 2)) * RSV + (p16 & 3) * 8;
#pragma unroll
        for (int db = 0; db < DB; ++db) {
          const x4 lo = TR::tr_read(trb + db * 32);
          const x4 hi = TR::tr_read(trb + 16 * RSV + db * 32);
          const x8 vt = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) {
#ifndef XM_ABL_PF_NOPV
            acc_o[nb][db] = TR::mfma(vt, pf[nb], acc_o[nb][db]);
#ifndef XM_ABL_PF_NOLO
            acc_o[nb][db] = TR::mfma(vt, pl[nb], acc_o[nb][db]);
#endif
#endif
          }
        }
      }
#ifndef XM_ABL_PF_NOSTAGE
      if (more) write_lds(cur ^ 1, tile + 1);
#endif
      __syncthreads();
      cur ^= 1;
    }
  }

  // epilogue: O^T lane (query p16, g) holds d = db*16 + 4g + r
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    float l = l_run[nb];
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (qidx[nb] >= q_len) continue;
    const float inv = l > 0.0f ? 1.0f / l : 0.0f;
    T* op = out + (int64_t)(q_start + qidx[nb]) * nq * D + (int64_t)h * D;
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      uint16_t hv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        T t = from_f32<T>(acc_o[nb][db][r] * inv);
        __builtin_memcpy(&hv[r], &t, 2);
      }
      *reinterpret_cast<uint2*>(op + db * 16 + g * 4) =
          make_uint2((uint32_t)hv[0] | ((uint32_t)hv[1] << 16), (uint32_t)hv[2] | ((uint32_t)hv[3] << 16));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// D = 128 fast path: the same math on 64-key tiles staged by LDS-DMA, with the matrix pipe and the VALU of a SIMD kept
// busy at the same time by two wave groups in opposite phases.
//   * K and V tiles (64 rows x 256 B each) are DMA'd (buffer_load ... lds, 1 KB per instruction) straight into LDS rings
//     (2 K + 2 V buffers): no staging registers, no LDS write instructions; a tile is requested two phases before its
//     first use;
//   * the buffer descriptor is rebuilt per tile (scalar base = first row of the tile; num_records = live rows), so rows
//     past kv_len arrive as zeros (V must be 0 there: 0 * NaN guard) and a tile inside ONE page needs one scalar page id;
//   * rows are unpadded (every DMA instruction fills 1 KB of contiguous LDS = 4 rows); bank conflicts are removed by
//     XOR-swizzling the 16-byte chunks of a row: K chunk ^= (row & 15) (a K fragment read touches 16 consecutive rows
//     at one logical chunk), V chunk ^= (row & 7) << 1 (a transposed V read touches 8 consecutive rows x 2 chunks);
//   * LDS reads of the DMA'd buffers are inline asm with counted waits (see attention_mla.hip: the compiler fences its
//     own LDS loads against all outstanding LDS-DMA with vmcnt(0));
//   * PING-PONG (tools/coissue_bench.hip, profiles/r01_prefill_attention.txt): on this chip an MFMA stream of one wave
//     runs at full rate underneath the VALU work of the OTHER wave of the SIMD, but two symmetric workgroups per CU fall
//     into lockstep (both in QK^T, both in softmax, both in PV) and get no overlap at all. So one workgroup = 8 waves =
//     256 queries: waves 0-3 (group 0) and 4-7 (group 1) sit pairwise on the same SIMDs and alternate, barrier to
//     barrier, between an MFMA block [O += P V of tile i-1 ; S = K Q^T of tile i] and a VALU block [softmax of tile i]:
//     step 2i + g is group g's MFMA block for tile i, step 2i + g + 1 its softmax.
typedef unsigned pu32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned pu32x2_t __attribute__((ext_vector_type(2)));
#define PF_DSR128(DST, ADDR, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(DST) : "v"(ADDR), "n"(OFF))
#define PF_DSR64TR(DST, ADDR, OFF) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(DST) : "v"(ADDR), "n"(OFF))
#define PF_LGKM1(N, A) asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(A) : "n"(N))
#define PF_LGKM2(N, A, B) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(A), "+v"(B) : "n"(N))

constexpr int kPf2Tile = 64;
constexpr int kPfDefaultPMode = 1;                  // XLLM_MI355_PREFILL_P default (see launch_flash_prefill)
constexpr int kPf2RowB = 256;                       // D = 128 16-bit elements per row, unpadded
constexpr int kPf2TileB = kPf2Tile * kPf2RowB;      // 16 KB per operand and tile
#ifdef XM_ABL_PF_TIMING  /* ablation build: shader-clock / wall-clock span of the tile loop of one workgroup */
__device__ long long pf_dbg[16];
#endif
#ifdef XM_ABL_PF_PHASES  /* with XM_ABL_PF_TIMING: per-phase shader cycles of waves 0 and 4 (forces completion at the marks) */
#define PF_MARK(I_, DEP_)                                                   \
  {                                                                         \
    float dep_;                                                             \
    asm volatile("v_mov_b32 %0, %1" : "=v"(dep_) : "v"(DEP_));              \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                      \
    const long long now_ = clock64();                                       \
    ph[I_] += now_ - ph_t;                                                  \
    ph_t = now_;                                                            \
  }
#else
#define PF_MARK(I_, DEP_)
#endif

// S^T = K Q^T of one tile for the wave's 2 x 16 queries. Fragment I = 4 blk + kk = rows 16 blk + p16, logical chunk
// 4 kk + g. The 16 fragment reads roll through 8 registers: read I + 8 is issued into the register of fragment I right
// after its MFMAs, so (LDS returns in order) fragment I < 8 is complete when 7 younger reads are outstanding.
template <typename T>
__device__ __forceinline__ void pf2_qk(pf32x4_t (&s)[2][4], const unsigned (&ka)[4], const typename PfTraits<T>::x8 (&qf)[2][4]) {
  using TR = PfTraits<T>;
  using x8 = typename TR::x8;
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) s[nb][blk] = pf32x4_t{0.f, 0.f, 0.f, 0.f};
  pu32x4_t kf[8];
#define PF_K_RD(I_) PF_DSR128(kf[(I_) & 7], ka[(I_) & 3], ((I_) >> 2) * 16 * kPf2RowB);
#define PF_K_MM(I_, WAIT_)                                                                                      \
  PF_LGKM1(WAIT_, kf[(I_) & 7]);                                                                                \
  s[0][(I_) >> 2] = TR::mfma(__builtin_bit_cast(x8, kf[(I_) & 7]), qf[0][(I_) & 3], s[0][(I_) >> 2]);          \
  s[1][(I_) >> 2] = TR::mfma(__builtin_bit_cast(x8, kf[(I_) & 7]), qf[1][(I_) & 3], s[1][(I_) >> 2]);
  PF_K_RD(0) PF_K_RD(1) PF_K_RD(2) PF_K_RD(3) PF_K_RD(4) PF_K_RD(5) PF_K_RD(6) PF_K_RD(7)
  PF_K_MM(0, 7) PF_K_RD(8) PF_K_MM(1, 7) PF_K_RD(9) PF_K_MM(2, 7) PF_K_RD(10) PF_K_MM(3, 7) PF_K_RD(11)
  PF_K_MM(4, 7) PF_K_RD(12) PF_K_MM(5, 7) PF_K_RD(13) PF_K_MM(6, 7) PF_K_RD(14) PF_K_MM(7, 7) PF_K_RD(15)
  PF_K_MM(8, 7) PF_K_MM(9, 6) PF_K_MM(10, 5) PF_K_MM(11, 4) PF_K_MM(12, 3) PF_K_MM(13, 2) PF_K_MM(14, 1) PF_K_MM(15, 0)
#undef PF_K_RD
#undef PF_K_MM
}

// O^T += V^T P^T of one tile (two 32-key halves, P = hi + lo). The reads of the second half roll into the registers of
// the first: the pair of block db is complete when 14 younger reads are outstanding (first half) / 2 (7 - db) (second).
template <typename T, bool P1>
__device__ __forceinline__ void pf2_pv(pf32x4_t (&acc_o)[2][8], const typename PfTraits<T>::x8 (&pf)[2][2],
                                       const typename PfTraits<T>::x8 (&pl)[2][2], const unsigned (&va)[8]) {
  using TR = PfTraits<T>;
  using x8 = typename TR::x8;
  using x4 = typename TR::x4;
  pu32x2_t vt[8][2];
#define PF_V_RD(KS_, DB_)                                                 \
  PF_DSR64TR(vt[DB_][0], va[DB_], (KS_) * 32 * kPf2RowB);                 \
  PF_DSR64TR(vt[DB_][1], va[DB_], (KS_) * 32 * kPf2RowB + 16 * kPf2RowB);
#ifdef XM_ABL_PF_NOLO  /* ablation build: timing only */
#define PF_V_LO(KS_, DB_)
#else
#define PF_V_LO(KS_, DB_)                                          \
  if constexpr (!P1) {                                             \
    acc_o[0][DB_] = TR::mfma(v8, pl[0][KS_], acc_o[0][DB_]);       \
    acc_o[1][DB_] = TR::mfma(v8, pl[1][KS_], acc_o[1][DB_]);       \
  }
#endif
#define PF_V_MM(KS_, DB_, WAIT_)                                                                                   \
  {                                                                                                                \
    PF_LGKM2(WAIT_, vt[DB_][0], vt[DB_][1]);                                                                       \
    const x8 v8 = __builtin_shufflevector(__builtin_bit_cast(x4, vt[DB_][0]), __builtin_bit_cast(x4, vt[DB_][1]),  \
                                          0, 1, 2, 3, 4, 5, 6, 7);                                                 \
    acc_o[0][DB_] = TR::mfma(v8, pf[0][KS_], acc_o[0][DB_]);                                                       \
    acc_o[1][DB_] = TR::mfma(v8, pf[1][KS_], acc_o[1][DB_]);                                                       \
    PF_V_LO(KS_, DB_)                                                                                              \
  }
  PF_V_RD(0, 0) PF_V_RD(0, 1) PF_V_RD(0, 2) PF_V_RD(0, 3) PF_V_RD(0, 4) PF_V_RD(0, 5) PF_V_RD(0, 6) PF_V_RD(0, 7)
  PF_V_MM(0, 0, 14) PF_V_RD(1, 0) PF_V_MM(0, 1, 14) PF_V_RD(1, 1) PF_V_MM(0, 2, 14) PF_V_RD(1, 2) PF_V_MM(0, 3, 14) PF_V_RD(1, 3)
  PF_V_MM(0, 4, 14) PF_V_RD(1, 4) PF_V_MM(0, 5, 14) PF_V_RD(1, 5) PF_V_MM(0, 6, 14) PF_V_RD(1, 6) PF_V_MM(0, 7, 14) PF_V_RD(1, 7)
  PF_V_MM(1, 0, 14) PF_V_MM(1, 1, 12) PF_V_MM(1, 2, 10) PF_V_MM(1, 3, 8)
  PF_V_MM(1, 4, 6) PF_V_MM(1, 5, 4) PF_V_MM(1, 6, 2) PF_V_MM(1, 7, 0)
#undef PF_V_RD
#undef PF_V_MM
#undef PF_V_LO
}

// (__builtin_bit_cast(float, vec[i]) on a vector ELEMENT reads element 0 for every i with hipcc / ROCm 7.2: by-value helper)
__device__ __forceinline__ float as_f32(unsigned v) { return __builtin_bit_cast(float, v); }

// online softmax of one tile: masks, running max / sum, P = hi + lo 16-bit parts, rescale of O when the max moved
template <typename T, bool P1>
__device__ __forceinline__ void pf2_softmax(pf32x4_t (&s)[2][4], typename PfTraits<T>::x8 (&pf)[2][2],
                                            typename PfTraits<T>::x8 (&pl)[2][2], float (&m_run)[2], pf32x4_t (&l_run)[2],
                                            pf32x4_t (&acc_o)[2][8], bool need_mask, int t0, int kv_len, int causal,
                                            int window_left, int kvoff, const int (&qidx)[2], int g, float scale_log2) {
  using elem = typename PfTraits<T>::elem;
  using x4 = typename PfTraits<T>::x4;
#ifdef XM_ABL_PF_NOSOFTMAX  /* ablation build: timing only */
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int blk = 0; blk < 4; ++blk)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pf[nb][blk >> 1][(blk & 1) * 4 + r] = (elem)s[nb][blk][r];
        pl[nb][blk >> 1][(blk & 1) * 4 + r] = (elem)s[nb][blk][r];
      }
#else
  if (need_mask) {  // wave-uniform: only the diagonal / tail / window-edge tiles of a wave
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int qpos = kvoff + qidx[nb];
#pragma unroll
      for (int blk = 0; blk < 4; ++blk)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int tok = t0 + blk * 16 + g * 4 + r;
          const bool vis = tok < kv_len && (!causal || tok <= qpos) && (window_left < 0 || tok >= qpos - window_left);
          if (!vis) s[nb][blk][r] = -INFINITY;
        }
    }
  }
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    // maximum on the raw scores (scale > 0), exponent argument by one FMA per value: p = 2^(s * scale - m)
    pf32x4_t m4 = __builtin_elementwise_max(__builtin_elementwise_max(s[nb][0], s[nb][1]),
                                            __builtin_elementwise_max(s[nb][2], s[nb][3]));
    float mx = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
#ifdef XM_ABL_PF_BPERMUTE  /* A/B build: the cross-lane maximum through ds_bpermute (LDS pipe, ~100 cycles each) */
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
#else
    {  // lanes l, l^16, l^32, l^48 hold the same query: v_permlane16_swap / v_permlane32_swap (VALU) exchange the rows.
       // swap(a, b) -> ([a0 b0 a2 b2], [a1 b1 a3 b3]) (rows of 16 / 32 lanes), so with b = a the maximum of the two results
       // is the xor-16 / xor-32 reduction (checked by tools/probe_permlane_swap.hip; the second operand is a separate copy).
      unsigned u = __builtin_bit_cast(unsigned, mx), c;
      asm volatile("v_mov_b32 %0, %1" : "=v"(c) : "v"(u));
      const auto r16 = __builtin_amdgcn_permlane16_swap(u, c, false, false);
      mx = fmaxf(as_f32(r16[0]), as_f32(r16[1]));
      u = __builtin_bit_cast(unsigned, mx);
      asm volatile("v_mov_b32 %0, %1" : "=v"(c) : "v"(u));
      const auto r32 = __builtin_amdgcn_permlane32_swap(u, c, false, false);
      mx = fmaxf(as_f32(r32[0]), as_f32(r32[1]));
    }
#endif
    // lazy rescale: the reference maximum only moves when the tile's maximum exceeds it by more than 2^8 (log2 domain), so
    // P stays <= 256 (exact in the fp32 sums, same relative precision in hi / lo) and the accumulator rescale all but vanishes
    const float mxs = mx * scale_log2;
    const float m_new = mxs > m_run[nb] + 8.0f ? mxs : m_run[nb];
    const float alpha = __builtin_amdgcn_exp2f(m_run[nb] - m_new);  // v_exp_f32: results below 2^-126 flush to 0
    m_run[nb] = m_new;
    const pf32x4_t sc4 = {scale_log2, scale_log2, scale_log2, scale_log2}, nm4 = {-m_new, -m_new, -m_new, -m_new};
    pf32x4_t l4 = l_run[nb] * alpha;
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
      const pf32x4_t e4 = __builtin_elementwise_fma(s[nb][blk], sc4, nm4);
      pf32x4_t p4;
#pragma unroll
      for (int r = 0; r < 4; ++r) p4[r] = __builtin_amdgcn_exp2f(e4[r]);
      l4 += p4;
      if constexpr (P1) {
        // one 16-bit P, rounded to nearest even (v_cvt_pk_bf16_f32 / v_cvt_pkrtz-free f16 cast): what the reference's own
        // attention kernels feed to PV (layers/cuda/flashinfer_attention.cpp:84-90 "attn @ V in bf16"); the row sum stays fp32
#pragma unroll
        for (int r = 0; r < 4; ++r) pf[nb][blk >> 1][(blk & 1) * 4 + r] = (elem)p4[r];
      } else if constexpr (__is_same(elem, __bf16)) {
        // hi = p truncated to bf16 (two values packed by one v_perm), lo = bf16(p - hi): p - hi is exact in fp32
        const pu32x4_t pb = __builtin_bit_cast(pu32x4_t, p4);
        const pu32x4_t hb = pb & 0xffff0000u;
        const pf32x4_t m1 = {-1.f, -1.f, -1.f, -1.f};
        const pf32x4_t lo4 = __builtin_elementwise_fma(__builtin_bit_cast(pf32x4_t, hb), m1, p4);  // p - hi (exact), packed
        pu32x2_t hp = {__builtin_amdgcn_perm(pb[1], pb[0], 0x07060302u), __builtin_amdgcn_perm(pb[3], pb[2], 0x07060302u)};
        const x4 h4 = __builtin_bit_cast(x4, hp);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          pf[nb][blk >> 1][(blk & 1) * 4 + r] = h4[r];
          pl[nb][blk >> 1][(blk & 1) * 4 + r] = (elem)lo4[r];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const elem hi = (elem)p4[r];
          pf[nb][blk >> 1][(blk & 1) * 4 + r] = hi;
          pl[nb][blk >> 1][(blk & 1) * 4 + r] = (elem)(p4[r] - (float)hi);
        }
      }
    }
    l_run[nb] = l4;
    // the running maximum settles after a few tiles; once no lane of the wave raised it, alpha == 1 everywhere
    // and the 32 multiplies are skipped (wave-uniform branch; multiplying by 1.0f is exact, so same bits)
    if (__any(alpha != 1.0f)) {
#pragma unroll
      for (int i = 0; i < 8; ++i) acc_o[nb][i] *= alpha;
    }
  }
#endif
}

// ---- block -> (q head, sequence, q block) of the LDS-DMA flash kernels, XCD-aware (round 6). Block b runs on XCD b % 8 (observed,
// relied on for speed only). The K / V stream of one (sequence, kv head) pair is shared by the G q heads of its group and by every
// q block: with the heads as the fastest block index the seven heads of a group sat on seven DIFFERENT XCDs and each XCD's L2
// fetched the same tiles again (587 MB of fabric reads per 2 x 4096-token launch by PMC against 91 MB pinned; Q + K + V are 75 MB). Here a pair is pinned to one XCD
// (P = n_seqs * nkv pairs dealt round robin over the 8 XCDs; P < 8 dividing 8: 8 / P XCDs share a pair's blocks), and inside an
// XCD the order stays "q block slowest and descending (heaviest causal blocks first), then pair, then head". Returns false for
// the padding blocks of the rounded-up grid.
__device__ __forceinline__ bool pf_block_coords(int nq, int nkv, int n_seqs, int n_qblocks, int& h, int& b, int& qb, int plain = 0) {
  const int G = nq / nkv, P = n_seqs * nkv;
  const int bx = blockIdx.x, x = bx & 7, j = bx >> 3;
  int pair, g, qbi;
  if (plain) {                                       // tuning arm (XLLM_MI355_PREFILL_XCD=0): the round-5 order, heads fastest
    h = bx % nq;
    b = (bx / nq) % n_seqs;
    qb = n_qblocks - 1 - bx / (nq * n_seqs);
    return qb >= 0;
  }
  if (P >= 8) {
    const int pairs_x = (P - x + 7) / 8;            // pairs x, x + 8, ... live on this XCD
    if (pairs_x <= 0) return false;
    g = j % G;
    const int t = j / G;
    pair = x + 8 * (t % pairs_x);
    qbi = t / pairs_x;
  } else if (8 % P == 0) {
    const int r = 8 / P, u = j * r + (x % r);        // the pair's blocks dealt over its r XCDs
    pair = x / r;
    g = u % G;
    qbi = u / G;
  } else {                                           // no even deal: the plain order
    const int u = bx;
    h = u % nq;
    b = (u / nq) % n_seqs;
    qb = n_qblocks - 1 - u / (nq * n_seqs);
    return qb >= 0;
  }
  if (qbi >= n_qblocks) return false;
  b = pair / nkv;
  h = (pair % nkv) * G + g;
  qb = n_qblocks - 1 - qbi;
  return true;
}
inline unsigned pf_grid_blocks(int64_t nq, int64_t nkv, int64_t n_seqs, int64_t n_qblocks) {
  const int64_t G = nq / nkv, P = n_seqs * nkv;
  if (P >= 8) return (unsigned)(8 * ((P + 7) / 8) * G * n_qblocks);
  if (8 % P == 0) { const int64_t r = 8 / P; return (unsigned)(8 * ((G * n_qblocks + r - 1) / r)); }
  return (unsigned)(nq * n_seqs * n_qblocks);
}

// NW = 8: ping-pong groups, 256 queries per workgroup, one workgroup per CU. NW = 4: one group, 128 queries per
// workgroup, two workgroups per CU (short query blocks: no second group to alternate with).
template <typename T, bool PAGED, int NW, bool MIDBAR, bool P1 = false>
__global__ __launch_bounds__(NW * 64, NW == 8 ? 1 : 2) void flash_prefill_dma_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, T* __restrict__ out,
    const int32_t* __restrict__ cu_q, const int32_t* __restrict__ cu_k, const int32_t* __restrict__ kv_lens,
    const int32_t* __restrict__ block_table, int max_blocks, int nq, int nkv, int block_size, int64_t q_stride,
    int64_t k_stride, int64_t v_stride, float scale_log2, int causal, int window_left, int n_seqs, int n_qblocks) {
  using TR = PfTraits<T>;
  using x8 = typename TR::x8;
  constexpr int D = 128, KK = D / 32, DB = D / 16;
  constexpr int ROWB = kPf2RowB, TILEB = kPf2TileB;
  constexpr int QB = NW * 32;                   // queries per workgroup
  constexpr int NDMA = 16 / NW;                 // 1 KB DMA instructions per wave, operand and tile
  __shared__ __attribute__((aligned(1024))) char lds[4 * TILEB];  // K ring [2] | V ring [2]
  typedef __attribute__((address_space(3))) char* lds_ptr_t;
  const lds_ptr_t lds3 = (lds_ptr_t)&lds[0];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = NW == 8 ? wave >> 2 : 0;
  const int p16 = lane & 15, g = lane >> 4;
  // 1-D grid, dispatched in order: the q block is the SLOWEST index and runs from the last (heaviest under a causal
  // mask) to the first, so the long workgroups of EVERY sequence start first and the short ones fill the tail
  // (with a (head, q block, sequence) grid the heaviest blocks of the last sequence started last: +12 % makespan)
  int h, b, qb;
  if (!pf_block_coords(nq, nkv, n_seqs, n_qblocks, h, b, qb)) return;
  const int q_start = cu_q[b], q_len = cu_q[b + 1] - q_start;
  const int q0 = qb * QB;
  if (q0 >= q_len) return;
  const int kv_len = PAGED ? kv_lens[b] : (cu_k[b + 1] - cu_k[b]);
  const int k_start = PAGED ? 0 : cu_k[b];
  const int G = nq / nkv, kvh = h / G;
  const int kvoff = kv_len - q_len;

  int q_hi = q0 + QB < q_len ? q0 + QB : q_len;
  int hi_tok = kv_len;
  if (causal) { int c = kvoff + q_hi; hi_tok = c < kv_len ? c : kv_len; }
  if (hi_tok < 0) hi_tok = 0;
  int lo_tok = 0;
  if (window_left >= 0) { lo_tok = kvoff + q0 - window_left; lo_tok = lo_tok > 0 ? lo_tok : 0; }
  const int tile_lo = lo_tok / kPf2Tile, tile_hi = (hi_tok + kPf2Tile - 1) / kPf2Tile;
  const int nt = tile_hi - tile_lo;

  const int32_t* bt_row = PAGED ? block_table + (int64_t)b * max_blocks : nullptr;
  const int64_t krow = PAGED ? (int64_t)nkv * D : k_stride;  // row pitch in elements
  const int64_t vrow = PAGED ? (int64_t)nkv * D : v_stride;

  x8 qf[2][KK];
  int qidx[2];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    qidx[nb] = q0 + wave * 32 + nb * 16 + p16;
    const bool ok = qidx[nb] < q_len;
    const T* qp = q + (int64_t)(q_start + (ok ? qidx[nb] : 0)) * q_stride + (int64_t)h * D;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      if (ok) qf[nb][kk] = *reinterpret_cast<const x8*>(qp + (kk * 4 + g) * 8);
      else qf[nb][kk] = x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  const int wq_lo = kvoff + q0 + wave * 32;
  int wq_hi = kvoff + (q0 + wave * 32 + 31 < q_len - 1 ? q0 + wave * 32 + 31 : q_len - 1);
  const bool wave_active = (q0 + wave * 32) < q_len;
  auto computes = [&](int i) -> bool {  // does this wave have visible keys in tile tile_lo + i ?
    const int t0 = (tile_lo + i) * kPf2Tile;
    return i >= 0 && i < nt && wave_active && (!causal || t0 <= wq_hi) && (window_left < 0 || t0 + kPf2Tile > wq_lo - window_left);
  };

  pf32x4_t acc_o[2][DB];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int i = 0; i < DB; ++i) acc_o[nb][i] = pf32x4_t{0.f, 0.f, 0.f, 0.f};
  float m_run[2] = {kPfNegBig, kPfNegBig};
  pf32x4_t l_run[2] = {pf32x4_t{0.f, 0.f, 0.f, 0.f}, pf32x4_t{0.f, 0.f, 0.f, 0.f}};  // lane-partial sums, 4 slots

  // DMA source offsets: instruction j of wave w fills LDS rows 4 (NDMA w + j) .. + 3 of the tile; lane = (row, physical chunk)
  int voff_k[4], voff_v[4];  // [NDMA] used; a template-dependent array size captured by a lambda makes hipcc drop the host stub
#pragma unroll
  for (int j = 0; j < NDMA; ++j) {
    const int row = 4 * (NDMA * wave + j) + (lane >> 4), pc = lane & 15;
    voff_k[j] = row * (int)(krow * 2) + ((pc ^ (row & 15)) << 4);
    voff_v[j] = row * (int)(vrow * 2) + ((pc ^ ((row & 7) << 1)) << 4);
  }
  auto stage = [&](int i, bool is_v) {  // tile tile_lo + i of K or V -> ring slot i & 1
    const int t0 = (tile_lo + i) * kPf2Tile;
    int rows = kv_len - t0 < kPf2Tile ? kv_len - t0 : kPf2Tile;
    rows = rows > 0 ? rows : 0;
    int64_t row0;
    if constexpr (PAGED) row0 = (int64_t)bt_row[(t0 < kv_len ? t0 : 0) / block_size] * block_size + t0 % block_size;
    else row0 = k_start + t0;
    const int64_t pitch = is_v ? vrow : krow;
    const T* src = (is_v ? v : k) + row0 * pitch + (int64_t)kvh * D;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<T*>(src), 0, rows ? (int)((rows - 1) * pitch * 2) + ROWB : 0, 0x00020000);
    const lds_ptr_t dst = lds3 + ((is_v ? 2 : 0) + (i & 1)) * TILEB + wave * (NDMA * 1024);
#pragma unroll
    for (int j = 0; j < NDMA; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, dst + j * 1024, 16, is_v ? voff_v[j] : voff_k[j], 0, 0, 0);
  };

  // fragment read offsets inside a ring slot (per lane, constant over tiles)
  const unsigned lds_base = (unsigned)(__UINTPTR_TYPE__)lds3;
  unsigned kofs[KK], vofs[DB];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) kofs[kk] = p16 * ROWB + (((kk * 4 + g) ^ p16) << 4);   // + blk * 16 rows
  {
    const int vr = 4 * g + (p16 >> 2), ft = vr & 7;
#pragma unroll
    for (int db = 0; db < DB; ++db) vofs[db] = 2 * TILEB + vr * ROWB + ((db ^ ft) << 5) + (p16 & 3) * 8;  // + 32 ks (+ 16) rows
  }

#ifdef XM_ABL_PF_TIMING
  const long long dbg_c0 = clock64(), dbg_w0 = wall_clock64();
#endif
  if (nt > 0) {
    pf32x4_t s[2][4];
    x8 pf[2][2], pl[2][2];
    // MFMA block of tile i: O += P V of tile i - 1 (P from the previous softmax), then S = K Q^T of tile i
#ifdef XM_ABL_PF_PHASES
    long long ph[4] = {0, 0, 0, 0}, ph_t = clock64();
#endif
    auto mfma_block = [&](int i) {
#if defined(XM_ABL_PF_PRIO_MFMA)
      __builtin_amdgcn_s_setprio(3);
#endif
      PF_MARK(0, m_run[0])  // barrier wait + DMA issue
      if (computes(i - 1)) {
        unsigned va[DB];
#pragma unroll
        for (int db = 0; db < DB; ++db) va[db] = lds_base + ((i - 1) & 1) * TILEB + vofs[db];
        pf2_pv<T, P1>(acc_o, pf, pl, va);
      }
      PF_MARK(1, acc_o[1][7][3])  // V reads + PV
      if (computes(i)) {
        unsigned ka[KK];
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) ka[kk] = lds_base + (i & 1) * TILEB + kofs[kk];
        pf2_qk<T>(s, ka, qf);
      }
      PF_MARK(2, s[1][3][3])  // K reads + QK^T
#if defined(XM_ABL_PF_PRIO_MFMA)
      __builtin_amdgcn_s_setprio(0);
#endif
    };
    auto softmax_block = [&](int i) {
      PF_MARK(0, m_run[0])
      if (!computes(i)) return;
      const int t0 = (tile_lo + i) * kPf2Tile;
      const bool need_mask = (t0 + kPf2Tile > kv_len) || (causal && t0 + kPf2Tile - 1 > wq_lo) ||
                             (window_left >= 0 && t0 < wq_hi - window_left);
#if defined(XM_ABL_PF_PRIO_VALU)
      __builtin_amdgcn_s_setprio(3);
#endif
      pf2_softmax<T, P1>(s, pf, pl, m_run, l_run, acc_o, need_mask, t0, kv_len, causal, window_left, kvoff, qidx, g,
                     scale_log2);
#if defined(XM_ABL_PF_PRIO_VALU)
      __builtin_amdgcn_s_setprio(0);
#endif
      PF_MARK(3, l_run[1][3])
    };
    // even step 2 i: the tiles requested two steps ago are published, K of tile i + 1 and V of tile i are requested
    // (first read at step 2 i + 2). A macro, not a lambda: hipcc drops the host stub of a kernel whose lambdas nest.
#define PF_EVEN_STEP(I_)                                                                                 \
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* this wave's slices of the requested tiles */      \
  __syncthreads();                                                                                       \
  if ((I_) + 1 < nt) stage((I_) + 1, false);                                                             \
  if ((I_) < nt) stage((I_), true);
    stage(0, false);
    // group g runs the MFMA block of tile i in step 2 i + g and the softmax of tile i in step 2 i + g + 1; each group
    // has its own straight-line loop (the same number of barriers in both)
    if (grp == 0) {
      for (int i = 0; i <= nt; ++i) {
        PF_EVEN_STEP(i)
        mfma_block(i);
        if constexpr (NW == 8 && MIDBAR) __syncthreads();
        softmax_block(i);
      }
    } else {
      for (int i = 0; i <= nt; ++i) {
        PF_EVEN_STEP(i)
        softmax_block(i - 1);
        if constexpr (MIDBAR) __syncthreads();
        mfma_block(i);
      }
    }
#undef PF_EVEN_STEP
#ifdef XM_ABL_PF_PHASES
    if (blockIdx.x == gridDim.x / 2 && lane == 0 && (wave & 3) == 0)
      for (int i = 0; i < 4; ++i) pf_dbg[4 + grp * 4 + i] = ph[i];
#endif
  }
#ifdef XM_ABL_PF_TIMING
  if (blockIdx.x == gridDim.x / 2 && tid == 0) {
    pf_dbg[0] = clock64() - dbg_c0;
    pf_dbg[1] = wall_clock64() - dbg_w0;
    pf_dbg[2] = nt;
  }
#endif

#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    float l = (l_run[nb][0] + l_run[nb][1]) + (l_run[nb][2] + l_run[nb][3]);
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (qidx[nb] >= q_len) continue;
    const float inv = l > 0.0f ? 1.0f / l : 0.0f;
    T* op = out + (int64_t)(q_start + qidx[nb]) * nq * D + (int64_t)h * D;
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      uint16_t hv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        T t = from_f32<T>(acc_o[nb][db][r] * inv);
        __builtin_memcpy(&hv[r], &t, 2);
      }
      *reinterpret_cast<uint2*>(op + db * 16 + g * 4) =
          make_uint2((uint32_t)hv[0] | ((uint32_t)hv[1] << 16), (uint32_t)hv[2] | ((uint32_t)hv[3] << 16));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Round 6: the same flash kernel on v_mfma_f32_32x32x16 with the softmax VALU work placed in the shadow of the MFMAs.
// Why: with 16x16x32 MFMAs (17 cycles each) a wave's fp32 VALU work serialises with its own matrix work (tools/coissue_bench.hip,
// profiles/r01_prefill_attention.txt: the kernel was the SUM of its MFMA and VALU issue time, 0.33 of the bf16 peak). A 32x32x16
// MFMA occupies the pipe for 32 cycles but one issue slot, so the wave can issue ~5 other instructions per MFMA
// (MI355X_MICROARCH.md, per-instruction constants) -- IF independent work sits next to it in program order. Structure:
//   * a wave owns 32 queries (one MFMA column block); S^T = K Q^T leaves lane (q = lane & 31, hi = lane >> 5) with the scores of
//     ONE query for keys 32 kb + (r & 3) + 8 (r >> 2) + 4 hi (16 of each 32-key block): the softmax is lane-local plus one
//     v_permlane32_swap for the row maximum; the row sum stays lane-partial until the epilogue;
//   * those 8-score groups ARE the B operand of O^T += V^T P^T once converted (k slot (hi, j) <-> key base + 8 (j >> 2) + 4 hi +
//     (j & 3)): no cross-lane traffic for P at all; the V^T operand is fetched with ds_read_b64_tr_b16 in exactly that key order;
//   * software pipeline inside a wave, per 64-key tile step j:  [S(j) = K(j) Q^T : 16 MFMAs  ||  max / exp / sum / convert of
//     tile j - 1]  then  [O += P(j-1) V(j-1) : 16 MFMAs  ||  the rest of the conversions, V / K fragment reads]: the MFMAs of
//     one tile never wait for the softmax of the same tile;
//   * staging, rings, swizzles, barrier protocol, masks, lazy rescale (2^8) and the single RNE-rounded 16-bit P (or hi + lo)
//     are flash_prefill_dma_kernel's: the checker's "flash" cast-point mode (64-key tiles, 2^8 threshold) describes both.
typedef float pf32x16_t __attribute__((ext_vector_type(16)));
#ifdef PF32_TRACE  /* trace build (tools/pf32_trace.py): per workgroup, 100-MHz wall clock at entry / first tile / last tile / exit + where it ran */
__device__ long long pf32_trace[16384 * 8];
#endif
#ifdef PF32_TIMING  /* timing build (tools/pf32_timing.py): shader cycles per phase of one wave, summed over its tiles */
__device__ long long pf32_dbg[16];
#define PF32_T(I_, DEP_)                                                    \
  {                                                                         \
    float dep_;                                                             \
    asm volatile("v_mov_b32 %0, %1" : "=v"(dep_) : "v"(DEP_));              \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                      \
    const long long now_ = clock64();                                       \
    tph[I_] += now_ - tph_t;                                                \
    tph_t = now_;                                                           \
  }
#define PF32_TARGS , long long (&tph)[8], long long& tph_t
#define PF32_TPASS , tph, tph_t
#else
#define PF32_T(I_, DEP_)
#define PF32_TARGS
#define PF32_TPASS
#endif
template <typename T>
struct Pf32Traits;
template <>
struct Pf32Traits<bf16_t> {
  static __device__ __forceinline__ pf32x16_t mfma(pbf16x8_t a, pbf16x8_t b, pf32x16_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <>
struct Pf32Traits<f16_t> {
  static __device__ __forceinline__ pf32x16_t mfma(pf16x8_t a, pf16x8_t b, pf32x16_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};

// one tile of a wave: S = K Q^T (16 MFMAs, K ring slot PAR), softmax, O += P V (16 MFMAs, V ring slot PAR). The ring slot is
// compile-time (the caller unrolls the tile loop by two), so every LDS offset is an immediate. The conversions of key steps 1-3
// sit between the PV MFMAs of the step before them; the row maximum and the first conversion are exposed to the wave itself and
// covered by the SIMD's other wave (two workgroups per CU, not in lockstep: each has its own barriers).
// (A two-tile pipeline -- S(j + 1) under the softmax of tile j -- needs a second score block: 32 more registers than the 256 a
// wave has at two waves per SIMD; it compiled with 400+ spilled registers and was dropped.)
template <typename T, bool P1, int PAR>
__device__ __forceinline__ void pf32_step(pf32x16_t (&acc_o)[4], float& m_run, float& l_run, const typename PfTraits<T>::x8 (&qf)[8],
                                          const unsigned (&kaddr)[8], const unsigned (&vaddr)[4], bool need_mask, int t0, int kv_len,
                                          int causal, int window_left, int qpos, int hi, float scale_log2 PF32_TARGS) {
  using x8 = typename PfTraits<T>::x8;
  using x4 = typename PfTraits<T>::x4;
  using elem = typename PfTraits<T>::elem;
  using M = Pf32Traits<T>;
  constexpr int SLOT = PAR * kPf2TileB;
  PF32_T(0, m_run)   // barrier wait + DMA issue

  pf32x16_t sc[2];
  sc[0] = pf32x16_t{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  sc[1] = sc[0];
  {
    // ---- K fragment reads: fragment I = 2 ks + kb = rows 32 kb + (lane & 31), logical chunk 2 ks + hi; eight in flight.
    // Consecutive MFMAs alternate between the two score blocks: an instruction between two MFMAs on the SAME accumulator costs
    // ~43 cycles, on different accumulators ~6 (MI355X_MICROARCH.md, per-instruction constants).
    pu32x4_t kf[8];
#define PF32_K_RD(I_) PF_DSR128(kf[(I_) & 7], kaddr[(I_) >> 1], SLOT + ((I_) & 1) * 32 * kPf2RowB);
#define PF32_K_MM(I_, WAIT_)                                                                             \
  PF_LGKM1(WAIT_, kf[(I_) & 7]);                                                                         \
  sc[(I_) & 1] = M::mfma(__builtin_bit_cast(x8, kf[(I_) & 7]), qf[(I_) >> 1], sc[(I_) & 1]);
    PF32_K_RD(0) PF32_K_RD(1) PF32_K_RD(2) PF32_K_RD(3) PF32_K_RD(4) PF32_K_RD(5) PF32_K_RD(6) PF32_K_RD(7)
    PF32_K_MM(0, 7) PF32_K_RD(8) PF32_K_MM(1, 7) PF32_K_RD(9) PF32_K_MM(2, 7) PF32_K_RD(10) PF32_K_MM(3, 7) PF32_K_RD(11)
    PF32_K_MM(4, 7) PF32_K_RD(12) PF32_K_MM(5, 7) PF32_K_RD(13) PF32_K_MM(6, 7) PF32_K_RD(14) PF32_K_MM(7, 7) PF32_K_RD(15)
    PF32_K_MM(8, 7) PF32_K_MM(9, 6) PF32_K_MM(10, 5) PF32_K_MM(11, 4) PF32_K_MM(12, 3) PF32_K_MM(13, 2) PF32_K_MM(14, 1) PF32_K_MM(15, 0)
#undef PF32_K_MM
#undef PF32_K_RD
  }
  PF32_T(1, sc[1][15])   // K reads + QK^T
  // ---- the V^T fragments of key step 0 are requested before the softmax starts
  pu32x2_t vt[8][2];   // fragment pair of (key step c, d block db) lives in slot 4 (c & 1) + db; eight pairs in flight
#define PF32_V_RD(C_, DB_)                                                                               \
  PF_DSR64TR(vt[((C_) & 1) * 4 + (DB_)][0], vaddr[DB_], 2 * kPf2TileB + SLOT + (C_) * 16 * kPf2RowB);    \
  PF_DSR64TR(vt[((C_) & 1) * 4 + (DB_)][1], vaddr[DB_], 2 * kPf2TileB + SLOT + (C_) * 16 * kPf2RowB + 8 * kPf2RowB);
  PF32_V_RD(0, 0) PF32_V_RD(0, 1) PF32_V_RD(0, 2) PF32_V_RD(0, 3) PF32_V_RD(1, 0) PF32_V_RD(1, 1) PF32_V_RD(1, 2) PF32_V_RD(1, 3)
  if (need_mask) {  // wave-uniform: only the diagonal / tail / window-edge tiles of a wave
    // (the empty asm keeps this a BRANCH: hipcc if-converted the block into ~230 compare / select instructions executed for
    // every tile, more than the whole softmax)
    asm volatile("" ::: "memory");
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int tok = t0 + 32 * kb + (r & 3) + 8 * (r >> 2) + 4 * hi;
        const bool vis = tok < kv_len && (!causal || tok <= qpos) && (window_left < 0 || tok >= qpos - window_left);
        if (!vis) sc[kb][r] = -INFINITY;
      }
  }
  // 32 scores -> 16 v_max3_f32 (as asm: hipcc puts a canonicalising v_max_f32 x, x, x in front of every fmaxf on an MFMA
  // result -- 57 instructions for this reduction instead of 17)
  float mx0 = kPfNegBig, mx1 = kPfNegBig;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 16; r += 4) {
      asm("v_max3_f32 %0, %1, %2, %3" : "=v"(mx0) : "v"(mx0), "v"(sc[kb][r]), "v"(sc[kb][r + 1]));
      asm("v_max3_f32 %0, %1, %2, %3" : "=v"(mx1) : "v"(mx1), "v"(sc[kb][r + 2]), "v"(sc[kb][r + 3]));
    }
  float mx;
  asm("v_max_f32 %0, %1, %2" : "=v"(mx) : "v"(mx0), "v"(mx1));
  {  // lanes l and l ^ 32 hold the same query: v_permlane32_swap (VALU) exchanges the halves
    unsigned u = __builtin_bit_cast(unsigned, mx), c;
    asm volatile("v_mov_b32 %0, %1" : "=v"(c) : "v"(u));
    const auto r32 = __builtin_amdgcn_permlane32_swap(u, c, false, false);
    mx = fmaxf(as_f32(r32[0]), as_f32(r32[1]));
  }
  // lazy rescale (flash_prefill_dma_kernel): the reference maximum only moves when the tile's maximum exceeds it by > 2^8
  const float mxs = mx * scale_log2;
  const float m_new = mxs > m_run + 8.0f ? mxs : m_run;
  const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
  m_run = m_new;
  x8 ph[2][2], pl[2][2];   // [kb][s1]: the B operands of the four PV key steps (hi part / lo part)
  float psum = 0.0f;
  // P of key step (kb, s1) = scores sc[kb][8 s1 .. 8 s1 + 7]: p = 2^(s * scale - m), row sum in fp32, one RNE 16-bit P (or hi + lo)
#define PF32_P_CHUNK(KB_, S1_)                                                                           \
  _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                                        \
    const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[KB_][(S1_) * 8 + j], scale_log2, -m_new));  \
    psum += p;                                                                                           \
    const elem h = (elem)p;                                                                              \
    ph[KB_][S1_][j] = h;                                                                                 \
    if constexpr (!P1) pl[KB_][S1_][j] = (elem)(p - (float)h);                                           \
  }
  PF32_P_CHUNK(0, 0)
  PF32_T(2, psum)        // mask, row maximum, first conversion

  // ---- O += P V: key step c = 2 kb + s1 (16 keys), d block db (32 columns); A = V^T by transposed reads in the k-slot key order
  if (__any(alpha != 1.0f)) {   // the running maximum settles after a few tiles (wave-uniform branch; x 1.0f is exact)
#pragma unroll
    for (int db = 0; db < 4; ++db) acc_o[db] *= alpha;
  }
#define PF32_V_MM(C_, DB_, WAIT_)                                                                        \
  {                                                                                                      \
    PF_LGKM2(WAIT_, vt[((C_) & 1) * 4 + (DB_)][0], vt[((C_) & 1) * 4 + (DB_)][1]);                       \
    const x8 v8 = __builtin_shufflevector(__builtin_bit_cast(x4, vt[((C_) & 1) * 4 + (DB_)][0]),           \
                                          __builtin_bit_cast(x4, vt[((C_) & 1) * 4 + (DB_)][1]), 0, 1, 2, 3, 4, 5, 6, 7); \
    acc_o[DB_] = M::mfma(v8, ph[(C_) >> 1][(C_) & 1], acc_o[DB_]);                                       \
    if constexpr (!P1) acc_o[DB_] = M::mfma(v8, pl[(C_) >> 1][(C_) & 1], acc_o[DB_]);                     \
  }
  PF32_V_MM(0, 0, 14) PF32_V_RD(2, 0) PF32_V_MM(0, 1, 14) PF32_V_RD(2, 1)
  PF32_P_CHUNK(0, 1)
  PF32_V_MM(0, 2, 14) PF32_V_RD(2, 2) PF32_V_MM(0, 3, 14) PF32_V_RD(2, 3)
  PF32_V_MM(1, 0, 14) PF32_V_RD(3, 0) PF32_V_MM(1, 1, 14) PF32_V_RD(3, 1)
  PF32_P_CHUNK(1, 0)
  PF32_V_MM(1, 2, 14) PF32_V_RD(3, 2) PF32_V_MM(1, 3, 14) PF32_V_RD(3, 3)
  PF32_V_MM(2, 0, 14) PF32_V_MM(2, 1, 12)
  PF32_P_CHUNK(1, 1)
  PF32_V_MM(2, 2, 10) PF32_V_MM(2, 3, 8)
  PF32_V_MM(3, 0, 6) PF32_V_MM(3, 1, 4) PF32_V_MM(3, 2, 2) PF32_V_MM(3, 3, 0)
#undef PF32_V_RD
#undef PF32_V_MM
#undef PF32_P_CHUNK
  l_run = l_run * alpha + psum;
  PF32_T(3, acc_o[3][15])   // PV + the other conversions
}

template <typename T, bool PAGED, bool P1>
__global__ __launch_bounds__(256, 2) void flash_prefill_m32_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, T* __restrict__ out,
    const int32_t* __restrict__ cu_q, const int32_t* __restrict__ cu_k, const int32_t* __restrict__ kv_lens,
    const int32_t* __restrict__ block_table, int max_blocks, int nq, int nkv, int block_size, int64_t q_stride,
    int64_t k_stride, int64_t v_stride, float scale_log2, int causal, int window_left, int n_seqs, int n_qblocks, int plain_map) {
  using TR = PfTraits<T>;
  using x8 = typename TR::x8;
  constexpr int D = 128, ROWB = kPf2RowB, TILEB = kPf2TileB, QB = 128, NDMA = 4;
  __shared__ __attribute__((aligned(1024))) char lds[4 * TILEB];  // K ring [2] | V ring [2]
  typedef __attribute__((address_space(3))) char* lds_ptr_t;
  const lds_ptr_t lds3 = (lds_ptr_t)&lds[0];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q32 = lane & 31, hi = lane >> 5;
#ifdef PF32_TRACE
  const long long tr_t0 = wall_clock64();
#endif
  int h, b, qb;
  if (!pf_block_coords(nq, nkv, n_seqs, n_qblocks, h, b, qb, plain_map)) return;
  const int q_start = cu_q[b], q_len = cu_q[b + 1] - q_start;
  const int q0 = qb * QB;
  if (q0 >= q_len) return;
  const int kv_len = PAGED ? kv_lens[b] : (cu_k[b + 1] - cu_k[b]);
  const int k_start = PAGED ? 0 : cu_k[b];
  const int G = nq / nkv, kvh = h / G;
  const int kvoff = kv_len - q_len;

  int q_hi = q0 + QB < q_len ? q0 + QB : q_len;
  int hi_tok = kv_len;
  if (causal) { int c = kvoff + q_hi; hi_tok = c < kv_len ? c : kv_len; }
  if (hi_tok < 0) hi_tok = 0;
  int lo_tok = 0;
  if (window_left >= 0) { lo_tok = kvoff + q0 - window_left; lo_tok = lo_tok > 0 ? lo_tok : 0; }
  const int tile_lo = lo_tok / kPf2Tile, tile_hi = (hi_tok + kPf2Tile - 1) / kPf2Tile;
  const int nt = tile_hi - tile_lo;

  const int32_t* bt_row = PAGED ? block_table + (int64_t)b * max_blocks : nullptr;
  const int64_t krow = PAGED ? (int64_t)nkv * D : k_stride;  // row pitch in elements
  const int64_t vrow = PAGED ? (int64_t)nkv * D : v_stride;

  // Q as the B operand: lane (n = query q32, k group hi) holds Q[q][16 ks + 8 hi .. + 7]
  x8 qf[8];
  const int qidx = q0 + wave * 32 + q32;
  {
    const bool ok = qidx < q_len;
    const T* qp = q + (int64_t)(q_start + (ok ? qidx : 0)) * q_stride + (int64_t)h * D;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      if (ok) qf[ks] = *reinterpret_cast<const x8*>(qp + ks * 16 + hi * 8);
      else qf[ks] = x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  const int wq_lo = kvoff + q0 + wave * 32;
  const int wq_hi = kvoff + (q0 + wave * 32 + 31 < q_len - 1 ? q0 + wave * 32 + 31 : q_len - 1);
  const bool wave_active = (q0 + wave * 32) < q_len;
  auto computes = [&](int i) -> bool {  // does this wave have visible keys in tile tile_lo + i ?
    const int t0 = (tile_lo + i) * kPf2Tile;
    return i >= 0 && i < nt && wave_active && (!causal || t0 <= wq_hi) && (window_left < 0 || t0 + kPf2Tile > wq_lo - window_left);
  };

  pf32x16_t acc_o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc_o[i] = pf32x16_t{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float m_run = kPfNegBig, l_run = 0.0f;

  // DMA source offsets: instruction j of wave w fills LDS rows 4 (NDMA w + j) .. + 3 of the tile; lane = (row, physical chunk)
  int voff_k[4], voff_v[4];
#pragma unroll
  for (int j = 0; j < NDMA; ++j) {
    const int row = 4 * (NDMA * wave + j) + (lane >> 4), pc = lane & 15;
    voff_k[j] = row * (int)(krow * 2) + ((pc ^ (row & 15)) << 4);
    voff_v[j] = row * (int)(vrow * 2) + ((pc ^ ((row & 3) << 2)) << 4);   // V: 32-byte units XOR 2 (row & 3), see vaddr
  }
  auto stage = [&](int i, bool is_v) {  // tile tile_lo + i of K or V -> ring slot i & 1
    const int t0 = (tile_lo + i) * kPf2Tile;
    int rows = kv_len - t0 < kPf2Tile ? kv_len - t0 : kPf2Tile;
    rows = rows > 0 ? rows : 0;
    int64_t row0;
    if constexpr (PAGED) row0 = (int64_t)bt_row[(t0 < kv_len ? t0 : 0) / block_size] * block_size + t0 % block_size;
    else row0 = k_start + t0;
    const int64_t pitch = is_v ? vrow : krow;
    const T* src = (is_v ? v : k) + row0 * pitch + (int64_t)kvh * D;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<T*>(src), 0, rows ? (int)((rows - 1) * pitch * 2) + ROWB : 0, 0x00020000);
    const lds_ptr_t dst = lds3 + ((is_v ? 2 : 0) + (i & 1)) * TILEB + wave * (NDMA * 1024);
#pragma unroll
    for (int j = 0; j < NDMA; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, dst + j * 1024, 16, is_v ? voff_v[j] : voff_k[j], 0, 0, 0);
  };

  // fragment read offsets inside ring slot 0 (per lane, constant over tiles)
  const unsigned lds_base = (unsigned)(__UINTPTR_TYPE__)lds3;
  unsigned kaddr[8], vaddr[4];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) kaddr[ks] = lds_base + q32 * ROWB + (((2 * ks + hi) ^ (q32 & 15)) << 4);   // + 32 kb rows
  {
    // V^T fragment of (key step, d block db): the 16 lanes of group (gi = d half, hi) address keys 4 hi + (p16 >> 2) (+ 8 for the
    // second read) x the four 8-byte column quads of d 32 db + 16 gi .. + 15; lane p16 receives column p16 of that 4 x 16 block
    const int p16 = lane & 15, gi = (lane >> 4) & 1;
    // (round 6: the unit swizzle was (row & 7): inside a 32-lane pass the rows are 4 hi + 0..3 and the d halves gi = 0, 1, and
    // (2 db + gi) ^ (row & 3) hits only FOUR of the eight 32-byte bank groups -- a 2-way conflict on every transposed read, 1.3
    // conflict cycles per LDS instruction by PMC (SQ_LDS_BANK_CONFLICT / SQ_INSTS_LDS); 2 (row & 3) leaves the gi bit alone: eight groups)
    const int vr = 4 * hi + (p16 >> 2), ft = 2 * (vr & 3);
#pragma unroll
    for (int db = 0; db < 4; ++db) vaddr[db] = lds_base + vr * ROWB + (((2 * db + gi) ^ ft) << 5) + (p16 & 3) * 8;   // + the V ring base
  }

#ifdef PF32_TRACE
  long long tr_t1 = 0, tr_t2 = 0;
#endif
  if (nt > 0) {
    const int qpos = kvoff + qidx;
    // step j: barrier (K(j), V(j) are published; tile j + 1 is requested into the slots tile j - 1 was read from) ; the tile
#ifdef PF32_TIMING
#define PF32_TB(I_) { const long long now_ = clock64(); tph[I_] += now_ - tph_t; tph_t = now_; }
#else
#define PF32_TB(I_)
#endif
#define PF32_BARRIER(I_)                                                                                 \
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* this wave's slices of the requested tile */       \
  PF32_TB(4)                                                                                             \
  __syncthreads();                                                                                       \
  PF32_TB(5)                                                                                             \
  if ((I_) + 1 < nt) { stage((I_) + 1, false); PF32_TB(6) stage((I_) + 1, true); PF32_TB(7) }
#define PF32_STEP(J_, PAR_)                                                                                              \
  {                                                                                                                      \
    const int j_ = (J_);                                                                                                 \
    if (computes(j_)) {                                                                                                  \
      const int t0 = (tile_lo + j_) * kPf2Tile;                                                                          \
      const bool need_mask = (t0 + kPf2Tile > kv_len) || (causal && t0 + kPf2Tile - 1 > wq_lo) ||                        \
                             (window_left >= 0 && t0 < wq_hi - window_left);                                             \
      pf32_step<T, P1, PAR_>(acc_o, m_run, l_run, qf, kaddr, vaddr, need_mask, t0, kv_len, causal, window_left, qpos, hi, \
                             scale_log2 PF32_TPASS);                                                                     \
    }                                                                                                                    \
  }
#ifdef PF32_TIMING
    long long tph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tph_t = clock64();
    const long long t_c0 = clock64(), t_w0 = wall_clock64();
#endif
#ifdef PF32_TRACE
    tr_t1 = wall_clock64();
#endif
    stage(0, false);
    stage(0, true);
    for (int j = 0; j < nt; j += 2) {
      PF32_BARRIER(j)
      PF32_STEP(j, 0)
      if (j + 1 >= nt) break;
      PF32_BARRIER(j + 1)
      PF32_STEP(j + 1, 1)
    }
#undef PF32_STEP
#undef PF32_BARRIER
#undef PF32_TB
#ifdef PF32_TRACE
    tr_t2 = wall_clock64();
#endif
#ifdef PF32_TIMING
    if (qb == n_qblocks - 4 && h == 5 && b == 0 && lane == 0 && wave == 3) {   // a long (late-query) block, its last wave
      for (int i = 0; i < 4; ++i) pf32_dbg[i] = tph[i];
      pf32_dbg[4] = clock64() - t_c0;
      pf32_dbg[5] = wall_clock64() - t_w0;
      pf32_dbg[6] = nt;
      pf32_dbg[7] = tph[4];   // of phase 0: this wave's own DMA slices landing (s_waitcnt vmcnt(0))
      pf32_dbg[8] = tph[5];   // of phase 0: the workgroup barrier
      pf32_dbg[9] = tph[6];   // of phase 0: issue of the K tile's four DMA pieces
      pf32_dbg[10] = tph[7];  // of phase 0: issue of the V tile's four DMA pieces
    }
#endif
  }

  // ---- epilogue: the two halves of a query's row sum meet, O^T -> O rows by v_permlane32_swap, 16-byte stores
  {
    unsigned u = __builtin_bit_cast(unsigned, l_run), c;
    asm volatile("v_mov_b32 %0, %1" : "=v"(c) : "v"(u));
    const auto r32 = __builtin_amdgcn_permlane32_swap(u, c, false, false);
    const float l = as_f32(r32[0]) + as_f32(r32[1]);
    const float inv = l > 0.0f ? 1.0f / l : 0.0f;
    const bool ok = qidx < q_len;
    T* op = out + (int64_t)(q_start + (ok ? qidx : 0)) * nq * D + (int64_t)h * D;
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) {
        // register group rg = 2 pr (+ 1) holds d = 32 db + 8 rg + 4 hi + 0..3: pack each to two dwords, swap the halves so that the
        // hi = 0 lane owns d 32 db + 16 pr + 0..7 and the hi = 1 lane d + 8..15
        unsigned w[2][2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int r0 = (2 * pr + e) * 4;
          uint16_t hv[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            T t = from_f32<T>(acc_o[db][r0 + r] * inv);
            __builtin_memcpy(&hv[r], &t, 2);
          }
          w[e][0] = (uint32_t)hv[0] | ((uint32_t)hv[1] << 16);
          w[e][1] = (uint32_t)hv[2] | ((uint32_t)hv[3] << 16);
        }
        // swap(a = rg even data, b = rg odd data) -> r[0] = [a_lo | b_lo] , r[1] = [a_hi | b_hi] (rows of 32 lanes):
        // hi = 0 lanes end with (a own, a partner) = d + 0..3, d + 4..7; hi = 1 lanes with (b partner, b own) = d + 8..11, d + 12..15
        const auto s0 = __builtin_amdgcn_permlane32_swap(w[0][0], w[1][0], false, false);
        const auto s1 = __builtin_amdgcn_permlane32_swap(w[0][1], w[1][1], false, false);
        if (ok)
          *reinterpret_cast<uint4*>(op + db * 32 + pr * 16 + hi * 8) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
      }
  }
#ifdef PF32_TRACE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (wave == 0 && lane == 0 && blockIdx.x < 16384) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    long long* o = pf32_trace + (size_t)blockIdx.x * 8;
    o[0] = tr_t0; o[1] = tr_t1; o[2] = tr_t2; o[3] = wall_clock64(); o[4] = nt; o[5] = hw; o[6] = xcc; o[7] = qb;
  }
#endif
}

template <typename T, int D, bool PAGED>
int launch_flash_prefill(const void* q, const void* k, const void* v, void* out, const int32_t* cu_q,
                         const int32_t* cu_k, const int32_t* kv_lens, const int32_t* block_table, int64_t max_blocks,
                         int64_t batch, int64_t nq, int64_t nkv, int64_t block_size, int64_t q_stride,
                         int64_t k_stride, int64_t v_stride, int64_t max_q_len, float scale, int causal,
                         int64_t window_left, hipStream_t s) {
  const int qblocks = (int)((max_q_len + kPfQBlock - 1) / kPfQBlock);
  if (qblocks <= 0) return XM_OK;
  const dim3 grid((unsigned)nq, (unsigned)qblocks, (unsigned)batch);
  const int wl = window_left < 0 ? -1 : (window_left > 0x3fffffff ? 0x3fffffff : (int)window_left);
  if constexpr (D == 128) {
    // LDS-DMA kernels: a 64-key tile must sit inside one page, and 64 row pitches must fit a 32-bit buffer offset
    // The register-staged kernel below stays the path of head dim 64, pages that are not 64-multiples and > 2 GiB pitches; forcing
    // it onto head dim 128 (XLLM_MI355_PREFILL_DMA=0) is a tuning arm of the -DXM_TUNING flavour. The ping-pong forms of the DMA kernel
    // (NW = 8: two wave groups alternating MFMA / softmax, round-1 negative result, profiles/r01_prefill_attention.txt) are
    // no longer instantiated in the library (round 3); the template parameter stays in the kernel for whoever revisits it.
    XM_TUNE_VAR(dma_mode, "XLLM_MI355_PREFILL_DMA", 1);
    const int64_t pitch = PAGED ? nkv * D : (k_stride > v_stride ? k_stride : v_stride);
    if (dma_mode && (!PAGED || block_size % kPf2Tile == 0) && pitch * 2 * kPf2Tile < (1ll << 31)) {
      const float sl2 = scale * 1.4426950408889634f;
      {
        // XLLM_MI355_PREFILL_P: 1 (default) = one 16-bit P per score, rounded to nearest even: the reference's semantics --
        // its eager spec casts P to the tensor dtype before PV (layers/cuda/flashinfer_attention.cpp:84-90) and its MLU decode
        // golden vector is reproduced to the last digit only with that rounding; the output is then
        // 2.1e-3 from the fp32-P result where the reference's own spec is 2.5e-3 away (profiles/r02_prefill_p.txt).
        // 2 = P = hi + lo (two MFMAs per block: fp32-P accuracy, 1e-4, at 1.34x the time)
        static int p_mode = -1;
        if (p_mode < 0) p_mode = xm_switch("XLLM_MI355_PREFILL_P", kPfDefaultPMode);   // product switch, read once
        XM_TUNE_VAR(xcd_map, "XLLM_MI355_PREFILL_XCD", 1);    // 0: heads the fastest block index (round-5 order; A/B + PMC in the tuning flavour)
        const int plain_map = xcd_map ? 0 : 1;
        const dim3 grid32(plain_map ? (unsigned)(nq * batch * qblocks) : pf_grid_blocks(nq, nkv, batch, qblocks));
        XM_TUNE_VAR(m32_mode, "XLLM_MI355_PREFILL_M32", 1);   // 0: the 16x16x32 kernel of rounds 1-5 (A/B in the tuning flavour: 293 vs 259 us)
        if (m32_mode && p_mode == 1)
          hipLaunchKernelGGL((flash_prefill_m32_kernel<T, PAGED, true>), grid32, dim3(256), 0, s,
                             (const T*)q, (const T*)k, (const T*)v, (T*)out, cu_q, cu_k, kv_lens, block_table, (int)max_blocks,
                             (int)nq, (int)nkv, (int)block_size, q_stride, k_stride, v_stride, sl2, causal, wl, (int)batch, qblocks, plain_map);
        else if (m32_mode)
          hipLaunchKernelGGL((flash_prefill_m32_kernel<T, PAGED, false>), grid32, dim3(256), 0, s,
                             (const T*)q, (const T*)k, (const T*)v, (T*)out, cu_q, cu_k, kv_lens, block_table, (int)max_blocks,
                             (int)nq, (int)nkv, (int)block_size, q_stride, k_stride, v_stride, sl2, causal, wl, (int)batch, qblocks, plain_map);
        else if (p_mode == 1)
          hipLaunchKernelGGL((flash_prefill_dma_kernel<T, PAGED, 4, false, true>), dim3(pf_grid_blocks(nq, nkv, batch, qblocks)),
                             dim3(256), 0, s, (const T*)q, (const T*)k, (const T*)v, (T*)out, cu_q, cu_k, kv_lens, block_table,
                             (int)max_blocks, (int)nq, (int)nkv, (int)block_size, q_stride, k_stride, v_stride, sl2, causal, wl,
                             (int)batch, qblocks);
        else
        hipLaunchKernelGGL((flash_prefill_dma_kernel<T, PAGED, 4, false>), dim3(pf_grid_blocks(nq, nkv, batch, qblocks)), dim3(256), 0, s,
                           (const T*)q, (const T*)k, (const T*)v, (T*)out, cu_q, cu_k, kv_lens, block_table, (int)max_blocks,
                           (int)nq, (int)nkv, (int)block_size, q_stride, k_stride, v_stride, sl2, causal, wl, (int)batch,
                           qblocks);
      }
      return hip_check_launch();
    }
  }
  hipLaunchKernelGGL((flash_prefill_kernel<T, D, PAGED>), grid, dim3(256), 0, s, (const T*)q, (const T*)k,
                     (const T*)v, (T*)out, cu_q, cu_k, kv_lens, block_table, (int)max_blocks, (int)nq, (int)nkv,
                     (int)block_size, q_stride, k_stride, v_stride, scale * 1.4426950408889634f, causal, wl);
  return hip_check_launch();
}

#define XM_INST_PREFILL(T, D, P)                                                                                   \
  template int launch_flash_prefill<T, D, P>(const void*, const void*, const void*, void*, const int32_t*,         \
                                             const int32_t*, const int32_t*, const int32_t*, int64_t, int64_t,     \
                                             int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, float, \
                                             int, int64_t, hipStream_t);
XM_INST_PREFILL(bf16_t, 128, true)
XM_INST_PREFILL(bf16_t, 128, false)
XM_INST_PREFILL(bf16_t, 64, true)
XM_INST_PREFILL(bf16_t, 64, false)
XM_INST_PREFILL(f16_t, 128, true)
XM_INST_PREFILL(f16_t, 128, false)
XM_INST_PREFILL(f16_t, 64, true)
XM_INST_PREFILL(f16_t, 64, false)

}  // namespace xm

#ifdef PF32_TIMING
extern "C" __attribute__((visibility("default"))) int xllm_mi355_debug_pf32(long long* out16) {
  return hipMemcpyFromSymbol(out16, HIP_SYMBOL(xm::pf32_dbg), 16 * sizeof(long long)) == hipSuccess ? 0 : -1;
}
#endif
#ifdef PF32_TRACE
extern "C" __attribute__((visibility("default"))) int xllm_mi355_debug_pf32_trace(long long* out, int n_blocks) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(xm::pf32_trace), (size_t)n_blocks * 8 * sizeof(long long)) == hipSuccess ? 0 : -1;
}
#endif
#ifdef XM_ABL_PF_TIMING
extern "C" __attribute__((visibility("default"))) int xllm_mi355_debug_pf(long long* out4) {
  return hipMemcpyFromSymbol(out4, HIP_SYMBOL(xm::pf_dbg), 12 * sizeof(long long)) == hipSuccess ? 0 : -1;
}
#endif

// attention_decode.hip -- paged decode attention for gfx950 (the HBM-bound 70%-of-roofline target).
//
// Reference semantics: AttentionImpl::paged_forward(is_chunked_prefill=false)
// (xllm/core/layers/dcu/flash_attention.cpp:220-288) == TorchAttentionImpl decode branch
// (layers/dcu/torch_attention.cpp:278-337): one query token per sequence, non-causal softmax over the
// kv_len cached tokens gathered page by page through the block table; GQA by kv_head = h / (nq/nkv).
//
// MI355X design (DESIGN.md "paged decode"):
//  * one WAVE owns (sequence, kv head, token range); the nq/nkv query heads of the GQA group are stacked
//    as the N dimension of the MFMA so every K/V byte is read from HBM exactly once.
//  * K is loaded straight from HBM into the MFMA A-fragment layout (16 tokens x 8 contiguous d per lane,
//    16-byte loads) -- no LDS round trip; S^T = K * Q^T ("swapped QK^T") leaves each lane with the scores
//    of ONE query head, so the online softmax is lane-local plus two cross-lane maxima per 32 tokens.
//  * V is loaded with fully coalesced 16-byte row loads, written once to a wave-private LDS tile
//    (row padded by 32 B -> conflict-free) and read back transposed with ds_read_b64_tr_b16 as the
//    A operand of O^T = V^T * P^T; the accumulator O^T keeps one query head per lane, so the rescale by
//    exp2(m_old - m_new) is lane-local too. No workgroup barrier inside the token loop.
//  * a workgroup = 4 waves = the kv heads of one token range (contiguous 1 KiB rows of the page are
//    consumed by one CU at about the same time), or 4 token sub-ranges when the rank holds < 4 kv heads
//    (TP >= 2); grid-level split-KV partials (m, l, O) are merged by a second tiny kernel.
//  * tile t+1 (16 KiB of K+V per wave) is in flight in registers while tile t is computed:
//    8 waves/CU x 16-32 KiB = 128-256 KiB outstanding per CU.
#include "common.h"
#include "attention_traits.h"

namespace xm {

constexpr int kTile = 32;         // tokens per tile (= K dim of the PV MFMA)
constexpr float kNegBig = -1e30f;  // finite "-inf" for the running max (log2 domain)

// D = head dim (K and V), UNIFORM: block_size % 32 == 0 so a tile lives in one page
// KROWS: how the K tile is fetched (see issue_loads) -- chosen by the launch plan, bit-identical results either way
// F8: the static-scale fp8 form (xllm_mi355_fp8_static.h) -- out_q takes e4m3 bytes and out_scale is READ: out_scale[0] is the
// static per-tensor scale. The one-pass epilogue stores the quantisation of the 8 values of a work item beside the 16-bit store;
// element-wise, so every plan with one grid split takes it, whatever hpw, and there is no second pass. wide_store then carries two
// flags (bit 0: 16-byte stores of out, bit 1: 8-byte stores of out_q). A template parameter, not a run-time branch, with the
// argument list unchanged: the F8 = false instantiations compile from code without it (profiles/fp8_static_decode.txt).
template <typename T, int D, bool UNIFORM, bool DEEP, bool KROWS, bool F8 = false>
__global__ __launch_bounds__(256, DEEP ? 1 : 2) void paged_decode_kernel(
    const T* __restrict__ q, const T* __restrict__ kc, const T* __restrict__ vc, T* __restrict__ out,
    float* __restrict__ part_o, float* __restrict__ part_ml, const int32_t* __restrict__ cu_q,
    const int32_t* __restrict__ kv_lens, const int32_t* __restrict__ block_table, int max_blocks, int nq,
    int nkv, int block_size, int64_t q_stride, float scale_log2, int nsplit, int hpw, int window_left,
    int8_t* __restrict__ out_q, float* __restrict__ out_scale, int part_mode, int wide_store) {
  using TR = AttnTraits<T>;
  using x8 = typename TR::x8;
  using x4 = typename TR::x4;
  using elem = typename TR::elem;
  constexpr int KK = D / 32;            // MFMA k-steps over the head dim
  constexpr int CH = D * 2 / 16;        // 16-byte chunks per K/V row
  constexpr int TPI = 64 / CH;          // V rows fetched per wave-wide load instruction
  constexpr int NV = kTile / TPI;       // V load instructions per tile
  constexpr int DB = D / 16;            // 16-wide output d blocks
  constexpr int RSB = D * 2 + 32;       // padded LDS row stride in bytes
  constexpr int WAVE_LDS = kTile * RSB; // per-wave LDS bytes (>= 16*D*4 for the epilogue)
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
  const int tile_lo = t_lo / kTile, tile_hi = (kv_len + kTile - 1) / kTile;
  const int nslots = nsplit * nsub, slot = split * nsub + sub;
  const int ntiles = tile_hi - tile_lo > 0 ? tile_hi - tile_lo : 0;
  const int per = (ntiles + nslots - 1) / nslots;
  int my_lo = tile_lo + slot * per;
  int my_hi = my_lo + per < tile_hi ? my_lo + per : tile_hi;
  my_lo = __builtin_amdgcn_readfirstlane(my_lo);
  my_hi = __builtin_amdgcn_readfirstlane(my_hi);

  const int32_t* bt_row = block_table + (int64_t)b * max_blocks;
  const int64_t row_elems = (int64_t)nkv * D;  // elements per token row of the cache
  char* my_lds = lds + wave * WAVE_LDS;

  // ---- Q as the MFMA B operand: lane (n = q head p16, k group g) holds Q[p16][(kk*4+g)*8 .. +7]
  x8 qf[KK];
  {
    const int64_t qtok = cu_q ? cu_q[b] : b;
    const T* qp = q + qtok * q_stride + (int64_t)(kvh * G + p16) * D;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      if (p16 < G) qf[kk] = *reinterpret_cast<const x8*>(qp + (kk * 4 + g) * 8);
      else qf[kk] = x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }

  f32x4_t acc_o[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i) acc_o[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m_run = kNegBig, l_run = 0.0f;

  // K/V register stages: named (never runtime-indexed) so they stay in VGPRs; native vector types so hipcc
  // emits plain 16-byte loads/stores (no memcpy allocas). DEEP: three stages = two tiles (32 KiB) in flight per
  // wave while the third is computed -- with ONE workgroup per CU (the best split count, see attention_api.hip)
  // a wave may use up to 512 registers.
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  x8 k0[2][KK], k1[2][KK], k2[2][KK];
  u32x4 v0[NV], v1[NV], v2[NV];

  // The KV stream is read exactly ONCE per launch: NON-TEMPORAL loads (global_load_dwordx4 ... nt). Round 4, tools/attn_ab.py on
  // one box, alternating libraries: 355 -> 329 us per launch at cfg3 = 6.05 -> 6.53 TB/s (0.756 -> 0.817 of 8 TB/s) -- above the
  // 6.25-6.47 TB/s "read ceiling" earlier rounds measured with ordinary loads (tools/hbm_read_bench.hip): a streaming read that
  // allocates in the L2 pays for evicting 2 GB of lines nobody will hit. -DXM_ATTN_TEMPORAL_LOADS restores the old loads (A/B).
#ifndef XM_ATTN_TEMPORAL_LOADS
#define XM_KV_LOAD(P) __builtin_nontemporal_load(P)
#else
#define XM_KV_LOAD(P) (*(P))
#endif
  auto page_of_tile = [&](int tile) -> int {  // UNIFORM only: scalar page id of a tile (clamped)
    int idx = (tile * kTile) / block_size;
    const int last = (kv_len - 1) / block_size;
    idx = idx > last ? last : idx;
    idx = idx < 0 ? 0 : idx;
    return bt_row[idx];
  };
  // every load is unconditional (tiles past the range re-load the last tile, tokens past kv_len the last token):
  // a branch around a load would make hipcc fall back to s_waitcnt vmcnt(0) and collapse the prefetch depth
  // The prefetch of the iteration that computes the wave's LAST tile asks for tile my_hi: nobody consumes it. It used to re-load
  // the whole last tile (16 KiB per wave: 0.8 % of the launch's bytes at cfg3, 6 % on a 16-tile range -- and with non-temporal
  // loads those lines are often gone from the L2 again, so they came from HBM: PMC traffic 1.007 x / 1.047 x algorithmic); now
  // every lane of such a request reads the FIRST row of that tile (one 2D-byte row, two cache lines). Still unconditional.
  auto issue_loads = [&](int tile, int page, x8 (&kr)[2][KK], u32x4 (&vr)[NV]) {
    const bool past = tile >= my_hi;            // wave-uniform
    tile = past ? my_hi - 1 : tile;
    const int t0 = tile * kTile;
    if constexpr (KROWS) {
      // K like V: an instruction fetches WHOLE head rows (64 / CH token rows x 2 D bytes) and compute_tile() re-lays the tile
      // through the wave's LDS. For a wave whose head is a strided 2D-byte slice of the token rows and whose workgroup does not
      // hold the row's other heads (hpw < nkv: small batches, DP replicas) this is the faster fetch -- round 4, alternating
      // libraries on one box (profiles/r04_attn_krows.txt): cfg2 54.5 -> 50.2 us, B = 128 / 64 / 32 at ctx 4096 177 -> 167,
      // 99.5 -> 92.5, 57.8 -> 52.4 us; with all kv heads of a row in the workgroup (hpw == nkv: the B = 256 headline, TP shards)
      // the direct operand-layout fetch below ties or wins by 0.6 %, so the plan picks per launch.
#pragma unroll
      for (int j = 0; j < 2 * KK; ++j) {
        int tok = past ? t0 : t0 + j * TPI + lane / CH;
        tok = tok < kv_len ? tok : kv_len - 1;
        int64_t rowi;
        if constexpr (UNIFORM) rowi = (int64_t)page * block_size + (tok % block_size);
        else rowi = (int64_t)bt_row[tok / block_size] * block_size + (tok % block_size);
        kr[j / KK][j % KK] = XM_KV_LOAD(reinterpret_cast<const x8*>(kc + rowi * row_elems + (int64_t)kvh * D + (lane % CH) * 8));
      }
    } else {
      // K straight into the MFMA A-operand layout: lane (p16, g) holds K[token blk*16 + p16][(kk*4+g)*8 .. +7] (64-byte pieces of
      // 16 token rows per instruction)
#pragma unroll
      for (int blk = 0; blk < 2; ++blk) {
        int tok = past ? t0 : t0 + blk * 16 + p16;
        tok = tok < kv_len ? tok : kv_len - 1;
        int64_t rowi;
        if constexpr (UNIFORM) rowi = (int64_t)page * block_size + (tok % block_size);
        else rowi = (int64_t)bt_row[tok / block_size] * block_size + (tok % block_size);
        const T* kp = kc + rowi * row_elems + (int64_t)kvh * D + g * 8;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) kr[blk][kk] = XM_KV_LOAD(reinterpret_cast<const x8*>(kp + kk * 32));
      }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      int tok = past ? t0 : t0 + i * TPI + lane / CH;
      tok = tok < kv_len ? tok : kv_len - 1;
      int64_t rowi;
      if constexpr (UNIFORM) rowi = (int64_t)page * block_size + (tok % block_size);
      else rowi = (int64_t)bt_row[tok / block_size] * block_size + (tok % block_size);
      vr[i] = XM_KV_LOAD(reinterpret_cast<const u32x4*>(vc + rowi * row_elems + (int64_t)kvh * D + (lane % CH) * 8));
    }
  };
  auto page_clamped = [&](int tile) -> int {
    if constexpr (UNIFORM) return page_of_tile(tile < my_hi ? tile : my_hi - 1);
    else return 0;
  };

  auto compute_tile = [&](int tile, const x8 (&kr)[2][KK], const u32x4 (&vr)[NV]) {
#ifdef XM_ABL_ATTN_NOCOMPUTE  /* ablation build: consume the loaded registers, no LDS / MFMA / softmax work */
    {
      unsigned fold = 0;
#pragma unroll
      for (int i = 0; i < NV; ++i) fold ^= vr[i].x ^ vr[i].y ^ vr[i].z ^ vr[i].w;
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
          u32x4 t;
          __builtin_memcpy(&t, &kr[blk][kk], 16);
          fold ^= t.x ^ t.y ^ t.z ^ t.w;
        }
      l_run += (fold == 0x12345678u) ? 1.0f : 0.0f;
      return;
    }
#endif
    const int t0 = tile * kTile;
    const bool partial = (t0 + kTile > kv_len) || (t0 < t_lo);

    // ---- KROWS: K tile -> wave-private LDS (row major, padded rows) -> MFMA A-operand fragments. The same buffer takes the V
    //      tile next: the LDS serves a wave's requests in order, so the V writes below cannot overtake these reads.
    x8 kf[2][KK];
    if constexpr (KROWS) {
#pragma unroll
      for (int j = 0; j < 2 * KK; ++j)
        *reinterpret_cast<x8*>(my_lds + (j * TPI + lane / CH) * RSB + (lane % CH) * 16) = kr[j / KK][j % KK];
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int kk = 0; kk < KK; ++kk)
          kf[blk][kk] = *reinterpret_cast<const x8*>(my_lds + (blk * 16 + p16) * RSB + (kk * 4 + g) * 16);
    } else {
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) kf[blk][kk] = kr[blk][kk];
    }

    // ---- V tile -> wave-private LDS (row major, padded rows); invalid rows zeroed (0 * NaN guard): the tail past kv_len and,
    //      in the window's edge tile, the rows below t_lo -- both meet p = 0 in the PV MFMA and may hold anything
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int r = i * TPI + lane / CH;
      u32x4 v = vr[i];
      // one unsigned range test for t_lo <= t0 + r < kv_len (t_lo <= kv_len always; a row below t_lo wraps to a huge value)
      if (partial && (unsigned)(t0 - t_lo + r) >= (unsigned)(kv_len - t_lo)) v = u32x4{0u, 0u, 0u, 0u};
      *reinterpret_cast<u32x4*>(my_lds + r * RSB + (lane % CH) * 16) = v;
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
    float mx = kNegBig;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = s[blk][r] * scale_log2;
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
    // P is fed to the matrix core as hi + lo 16-bit parts (p = hi + lo to ~2^-17 relative): the PV MFMAs
    // are idle-cheap in this HBM-bound kernel and the output then matches an fp32-P reference to rounding.
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

    // ---- O^T += V^T * P^T : A = V^T via transposed LDS reads, k slot (g, j): j<4 -> token 4g+j,
    //      j>=4 -> token 16+4g+(j-4), matching the P fragment above
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
    if constexpr (DEEP) {
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
    } else {
      int pg1 = page_clamped(my_lo + 1), pg2;
      issue_loads(my_lo, page_clamped(my_lo), k0, v0);
      while (true) {
        pg2 = page_clamped(tile + 2);
        issue_loads(tile + 1, pg1, k1, v1);
        compute_tile(tile, k0, v0);
        pg1 = pg2;
        if (++tile >= my_hi) break;
        pg2 = page_clamped(tile + 2);
        issue_loads(tile + 1, pg1, k0, v0);
        compute_tile(tile, k1, v1);
        pg1 = pg2;
        if (++tile >= my_hi) break;
      }
    }
  }

  // ---- epilogue: stage (m, l, O) of every wave in LDS, merge the sub-ranges of each head
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
  // One pass over work items (head slot h_s, live query head qq < G, 8 consecutive d): hpw * G * D / 8 of them, at most 1024, so
  // a thread takes at most 4 and padded query heads are never visited. Per item (m, l) of each contributing wave is read once,
  // m*, f = exp2(m - m*) and l are formed once per head, and O comes in as two 16-byte LDS reads per wave; the 8 values are
  // the expressions of the element-wise loop this replaces, in the same order over sb, so every exit is bit-identical to it.
  // wide_store (host, per launch): the output bases admit 16-byte (16-bit out, part_o) / 8-byte (int8) stores.
  const int64_t qtok = cu_q ? cu_q[b] : b;
  constexpr int DPI = D / 8;  // items per head
  const int nitems = hpw * G * DPI;
  __shared__ float red[32];
  float val[4][8];  // int8 form: the rounded values wait here for the row maximum
  float amax = 0.0f;
  float f8_sinv = 0.0f;
  bool wide_f8 = false;
  if constexpr (F8) {
    f8_sinv = 1.0f / out_scale[0];   // fp8_quant_kernel's reciprocal (rowwise.hip)
    wide_f8 = (wide_store & 2) != 0;
    wide_store &= 1;
  }
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int item = threadIdx.x + it * 256;
    if (item < nitems) {
      const int hq = item / DPI, d = (item % DPI) * 8;
      const int h_s = hq / G, qq = hq - h_s * G;
      float mw[4], lw[4];
      float m_star = kNegBig;
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
      if (part_mode) {  // grid-level split-KV, or a finishing kernel that wants (o, m, l) of the whole range (nsplit == 1)
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
          t[j] = from_f32<T>(l > 0.0f ? o[j] / l : 0.0f);
          uint16_t bits;
          __builtin_memcpy(&bits, &t[j], 2);
          pk[j >> 1] |= (unsigned)bits << ((j & 1) * 16);
          val[it][j] = to_f32<T>(t[j]);
          amax = fmaxf(amax, fabsf(val[it][j]));
        }
        if (out) {  // the int8 form's 16-bit copy is optional
          T* op16 = out + qtok * (int64_t)nq * D + (int64_t)head * D + d;
          if (wide_store) *reinterpret_cast<u32x4*>(op16) = pk;
          else {
#pragma unroll
            for (int j = 0; j < 8; ++j) op16[j] = t[j];
          }
        }
        if constexpr (F8) {  // static_scaled_fp8_quant of the 16-bit values above, from registers
          unsigned lo = 0u, hi = 0u;
          uint8_t f8[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            f8[j] = f32_to_e4m3_sat(val[it][j] * f8_sinv);
            const unsigned byte = (unsigned)f8[j] << ((j & 3) * 8);
            if (j < 4) lo |= byte;
            else hi |= byte;
          }
          uint8_t* oq = reinterpret_cast<uint8_t*>(out_q) + qtok * (int64_t)nq * D + (int64_t)head * D + d;
          if (wide_f8) *reinterpret_cast<uint2*>(oq) = make_uint2(lo, hi);
          else {
#pragma unroll
            for (int j = 0; j < 8; ++j) oq[j] = f8[j];
          }
        }
      }
    }
  }
  if constexpr (F8) return;
  if (!out_q) return;
  // N1 fusion: the workgroup holds ALL heads of this token (host guarantees nsplit == 1 and one head group), so the per-token
  // int8 quantisation that feeds o_proj (scaled_quantize of the 16-bit output) is done here, from the registers above.
  // Bit-identical to paged_attention -> scaled_quantize.
  amax = block_max(amax, red);
  const float qinv = (amax > 1e-10f) ? 127.0f / amax : 0.0f;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int item = threadIdx.x + it * 256;
    if (item < nitems) {
      unsigned lo = 0u, hi = 0u;
      int8_t q8[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        q8[j] = (int8_t)fmaxf(-127.0f, fminf(127.0f, rintf(val[it][j] * qinv)));
        const unsigned byte = (unsigned)(uint8_t)q8[j] << ((j & 3) * 8);
        if (j < 4) lo |= byte;
        else hi |= byte;
      }
      // item * 8 == head * D + d here: one head group (hg == 0), heads and their d chunks in item order
      int8_t* oq = out_q + qtok * (int64_t)nq * D + (int64_t)item * 8;
      if (wide_store) *reinterpret_cast<uint2*>(oq) = make_uint2(lo, hi);
      else {
#pragma unroll
        for (int j = 0; j < 8; ++j) oq[j] = q8[j];
      }
    }
  }
  if (threadIdx.x == 0) out_scale[qtok] = amax / 127.0f;
}

// merge of the grid-level split-KV partials: one workgroup (D threads) per (sequence, head)
template <typename T, int D>
__global__ void paged_decode_merge_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                          T* __restrict__ out, const int32_t* __restrict__ cu_q, int nq, int nsplit) {
  const int b = blockIdx.x / nq, head = blockIdx.x % nq;
  const int d = threadIdx.x;
  const int64_t base = ((int64_t)b * nq + head) * nsplit;
  float m_star = kNegBig;
  for (int s = 0; s < nsplit; ++s) m_star = fmaxf(m_star, part_ml[(base + s) * 2]);
  float o = 0.0f, l = 0.0f;
  for (int s = 0; s < nsplit; ++s) {
    const float f = exp2f(part_ml[(base + s) * 2] - m_star);
    o += f * part_o[(base + s) * D + d];
    l += f * part_ml[(base + s) * 2 + 1];
  }
  const int64_t qtok = cu_q ? cu_q[b] : b;
  out[qtok * (int64_t)nq * D + (int64_t)head * D + d] = from_f32<T>(l > 0.0f ? o / l : 0.0f);
}

// the same merge, emitting the static e4m3 quantisation of the 16-bit value (and the value itself when out != NULL): merge +
// static_scaled_fp8_quant in one launch, the expressions of both in their order. One query token per sequence.
template <typename T, int D>
__global__ void paged_decode_merge_fp8_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                              T* __restrict__ out, uint8_t* __restrict__ out_f8,
                                              const float* __restrict__ f8_scale, int nq, int nsplit) {
  const int b = blockIdx.x / nq, head = blockIdx.x % nq;
  const int d = threadIdx.x;
  const int64_t base = ((int64_t)b * nq + head) * nsplit;
  const float sinv = 1.0f / f8_scale[0];
  float m_star = kNegBig;
  for (int s = 0; s < nsplit; ++s) m_star = fmaxf(m_star, part_ml[(base + s) * 2]);
  float o = 0.0f, l = 0.0f;
  for (int s = 0; s < nsplit; ++s) {
    const float f = exp2f(part_ml[(base + s) * 2] - m_star);
    o += f * part_o[(base + s) * D + d];
    l += f * part_ml[(base + s) * 2 + 1];
  }
  const T v = from_f32<T>(l > 0.0f ? o / l : 0.0f);
  const int64_t at = (int64_t)b * nq * D + (int64_t)head * D + d;
  if (out) out[at] = v;
  out_f8[at] = f32_to_e4m3_sat(to_f32<T>(v) * sinv);
}

// merge + per-token int8 quantisation in one launch (N1 fusion for the plans whose workgroups do not hold a whole token:
// fewer than all kv heads per workgroup, or grid-level split-KV): one workgroup per token merges the nsplit partials of all
// nq heads exactly like paged_decode_merge_kernel, rounds to T, and quantises the row like scaled_quantize -- the bits of
// paged_attention followed by scaled_quantize, one launch and one 16-bit round trip less.
// NSP > 0 (round 6): at most NSP splits, and EVERY load of the launch -- the (m, l) pairs and all partial rows -- is requested
// before anything is consumed: the launch is one memory latency deep instead of 1 + nsplit (the round-2 form, NSP = 0, waited
// for the (m, l) pairs, then for each split's rows in turn: 12.7 us against 4.9 + 4.8 for the two launches it replaces)
template <typename T, int D, int VPT, int NSP, int NT>
__global__ __launch_bounds__(NT) void paged_decode_finish_int8_kernel(const float* __restrict__ part_o,
                                                                       const float* __restrict__ part_ml, T* __restrict__ out,
                                                                       int8_t* __restrict__ out_q, float* __restrict__ out_scale,
                                                                       int nq, int nsplit) {
  constexpr int kMaxHeads = 32, kMaxSplit = 32;     // nq <= 32 (VPT * NT / D), nsplit <= 32 (decode_num_splits)
  __shared__ float red[32];
  __shared__ float fs[kMaxHeads][kMaxSplit];        // exp2(m_s - m*) per (head, split)
  __shared__ float ls[kMaxHeads];                   // merged denominators
  const int b = blockIdx.x;
  const int n = nq * D;
  float v[VPT];
  if constexpr (NSP > 0) {
    float po[NSP][VPT];
#pragma unroll
    for (int s = 0; s < NSP; ++s)
#pragma unroll
      for (int i = 0; i < VPT; ++i) {
        const int e = threadIdx.x + i * NT;
        po[s][i] = (s < nsplit && e < n) ? part_o[(((int64_t)b * nq + e / D) * nsplit + s) * D + e % D] : 0.0f;
      }
    if ((int)threadIdx.x < nq) {
      const int head = threadIdx.x;
      const int64_t base = ((int64_t)b * nq + head) * nsplit;
      float2 ml[NSP];
#pragma unroll
      for (int s = 0; s < NSP; ++s)
        ml[s] = s < nsplit ? *reinterpret_cast<const float2*>(part_ml + (base + s) * 2) : make_float2(kNegBig, 0.0f);
      float m_star = kNegBig;
#pragma unroll
      for (int s = 0; s < NSP; ++s)
        if (s < nsplit) m_star = fmaxf(m_star, ml[s].x);
      float l = 0.0f;
#pragma unroll
      for (int s = 0; s < NSP; ++s)
        if (s < nsplit) {
          const float f = exp2f(ml[s].x - m_star);
          fs[head][s] = f;
          l += f * ml[s].y;
        }
      ls[head] = l;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < VPT; ++i) v[i] = 0.0f;
#pragma unroll
    for (int s = 0; s < NSP; ++s)
      if (s < nsplit) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
          const int e = threadIdx.x + i * NT;
          if (e < n) v[i] += fs[e / D][s] * po[s][i];
        }
      }
  } else {
    // phase A: one thread per head turns the (m, l) pairs into the split weights
    if ((int)threadIdx.x < nq) {
      const int head = threadIdx.x;
      const int64_t base = ((int64_t)b * nq + head) * nsplit;
      float m_star = kNegBig;
      for (int s = 0; s < nsplit; ++s) m_star = fmaxf(m_star, part_ml[(base + s) * 2]);
      float l = 0.0f;
      for (int s = 0; s < nsplit; ++s) {
        const float f = exp2f(part_ml[(base + s) * 2] - m_star);
        fs[head][s] = f;
        l += f * part_ml[(base + s) * 2 + 1];
      }
      ls[head] = l;
    }
    __syncthreads();
    // phase B: o = sum_s f_s * o_s in split order (the merge kernel's order), all of a thread's elements per split at once
#pragma unroll
    for (int i = 0; i < VPT; ++i) v[i] = 0.0f;
    for (int s = 0; s < nsplit; ++s) {
#pragma unroll
      for (int i = 0; i < VPT; ++i) {
        const int e = threadIdx.x + i * NT;
        if (e < n) {
          const int head = e / D, d = e % D;
          v[i] += fs[head][s] * part_o[(((int64_t)b * nq + head) * nsplit + s) * D + d];
        }
      }
    }
  }
  float amax = 0.0f;
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int e = threadIdx.x + i * NT;
    if (e < n) {
      const float l = ls[e / D];
      v[i] = r16<T>(l > 0.0f ? v[i] / l : 0.0f);
      amax = fmaxf(amax, fabsf(v[i]));
      if (out) out[(int64_t)b * n + e] = from_f32<T>(v[i]);
    }
  }
  amax = block_max(amax, red);
  const float qinv = (amax > 1e-10f) ? 127.0f / amax : 0.0f;
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int e = threadIdx.x + i * NT;
    if (e < n) out_q[(int64_t)b * n + e] = (int8_t)fmaxf(-127.0f, fminf(127.0f, rintf(v[i] * qinv)));
  }
  if (threadIdx.x == 0) out_scale[b] = amax / 127.0f;
}

int decode_num_splits(int64_t batch, int64_t nkv, int hpw, int64_t max_kv_len);
bool decode_deep_prefetch();
int decode_heads_per_wg(int64_t batch, int64_t nkv);
int decode_exclusive_cu();

template <typename T, int D>
int launch_paged_decode(const void* q, const void* kc, const void* vc, void* out, const int32_t* cu_q,
                        const int32_t* kv_lens, const int32_t* block_table, int64_t max_blocks, int64_t batch,
                        int64_t nq, int64_t nkv, int64_t block_size, int64_t q_stride, int64_t max_kv_len,
                        float scale, int64_t window_left, void* workspace, size_t ws_bytes, hipStream_t s,
                        int8_t* out_q, float* out_scale) {
  const int hpw = decode_heads_per_wg(batch, nkv);
  int nsplit = decode_num_splits(batch, nkv, hpw, max_kv_len);
  // the fused int8 epilogue needs the whole token in one workgroup; the other plans (split-KV, fewer than all kv heads per
  // workgroup) leave (o, m, l) partials in the workspace and a finishing launch merges + quantises them. Without a
  // workspace those plans are declined (the caller then runs paged_attention + scaled_quantize)
  const size_t per_split = (size_t)batch * nq * (D + 2) * sizeof(float);
  if (!workspace) ws_bytes = 0;
  // (plans with one split but fewer than all kv heads per workgroup write their 16-bit output directly: for them the
  // finishing launch would only replace scaled_quantize by a launch of the same cost -- measured -- so they are declined)
  if (out_q && nsplit == 1 && nkv / hpw != 1) return XM_ERR_UNSUPPORTED;
  const bool finish = out_q && nsplit != 1;
  if (finish && (ws_bytes < (size_t)nsplit * per_split || nq * D > 1024 * 4 || nq > 32 || cu_q)) return XM_ERR_UNSUPPORTED;
  // degrade the split count to what the caller's workspace holds (1 split needs none)
  if ((size_t)nsplit * per_split > ws_bytes) nsplit = (int)(ws_bytes / per_split);
  if (nsplit < 1) nsplit = 1;
  const int part_mode = (nsplit > 1 || finish) ? 1 : 0;
  int8_t* const kq = finish ? nullptr : out_q;          // the attention kernel's own int8 epilogue
  float* const kqs = finish ? nullptr : out_scale;
  float* part_o = reinterpret_cast<float*>(workspace);
  float* part_ml = part_o ? part_o + (size_t)batch * nq * nsplit * D : nullptr;
  const float scale_log2 = scale * 1.4426950408889634f;
  const dim3 grid((unsigned)(batch * (nkv / hpw) * nsplit));
  const int wl = window_left < 0 ? -1 : (window_left > 0x3fffffff ? 0x3fffffff : (int)window_left);
  // tuning arm (XLLM_MI355_DECODE_EXCL=1, -DXM_TUNING flavour only): grids of at most one workgroup per CU reserve enough extra LDS that two
  // workgroups cannot share a CU, so the dispatcher has to spread them over all 256
  const size_t dyn = (decode_exclusive_cu() && grid.x <= 256) ? 48 * 1024 : 0;
  // the epilogue's stores: 16 bytes per work item (16-bit out, fp32 partials) and 8 bytes (int8) when the bases allow it --
  // rows are nq * D elements with D a multiple of 64, so only the pointers decide; otherwise element-wise, same loop
  const int wide_store = (part_mode ? (uintptr_t)part_o % 16 == 0 : (uintptr_t)out % 16 == 0) && (uintptr_t)kq % 8 == 0;
  const bool krows = hpw < nkv;   // the wave's head is a strided slice of rows whose other heads are elsewhere (see issue_loads)
#define XM_DECODE_LAUNCH(UNI_, DEEP_, KROWS_, DYN_)                                                                        \
  hipLaunchKernelGGL((paged_decode_kernel<T, D, UNI_, DEEP_, KROWS_>), grid, dim3(256), DYN_, s, (const T*)q, (const T*)kc, \
                     (const T*)vc, (T*)out, part_o, part_ml, cu_q, kv_lens, block_table, (int)max_blocks, (int)nq,        \
                     (int)nkv, (int)block_size, q_stride, scale_log2, nsplit, hpw, wl, kq, kqs, part_mode, wide_store)
#ifdef XM_TUNING  /* the three-stage arm (round-1 A/B loser) exists only in the tuning flavour */
  if (block_size % kTile == 0 && decode_deep_prefetch()) XM_DECODE_LAUNCH(true, true, false, dyn);
  else
#endif
  if (block_size % kTile == 0) {
    if (krows) XM_DECODE_LAUNCH(true, false, true, dyn);
    else XM_DECODE_LAUNCH(true, false, false, dyn);
  } else {
    if (krows) XM_DECODE_LAUNCH(false, false, true, 0);
    else XM_DECODE_LAUNCH(false, false, false, 0);
  }
#undef XM_DECODE_LAUNCH
  if (finish) {
    const int vpt = (int)((nq * D + 255) / 256);
#define XM_FINISH_(V_, N_, T_)                                                                                           \
  hipLaunchKernelGGL((paged_decode_finish_int8_kernel<T, D, V_, N_, T_>), dim3((unsigned)batch), dim3(T_), 0, s, part_o,  \
                     part_ml, (T*)out, out_q, out_scale, (int)nq, nsplit)
#define XM_FINISH(V_, T_)                                                                                               \
  {                                                                                                                     \
    if (nsplit <= 2) XM_FINISH_(V_, 2, T_);                                                                             \
    else if (nsplit <= 4) XM_FINISH_(V_, 4, T_);                                                                        \
    else XM_FINISH_(V_, 0, T_);                                                                                         \
  }
    // rows beyond 1024 elements: 1024 threads (few tokens per launch there -- the launch is latency, not throughput)
    if (vpt <= 4) XM_FINISH(4, 256)
    else XM_FINISH(4, 1024)
#undef XM_FINISH
#undef XM_FINISH_
  } else if (nsplit > 1) {
    hipLaunchKernelGGL((paged_decode_merge_kernel<T, D>), dim3((unsigned)(batch * nq)), dim3(D), 0, s, part_o,
                       part_ml, (T*)out, cu_q, (int)nq, nsplit);
  }
  return hip_check_launch();
}

// the static-scale fp8 form (xllm_mi355_paged_decode_attention_fp8): the launch plan of launch_paged_decode -- hpw, the split
// count and its degradation to the caller's workspace -- so that the 16-bit values quantised here are the bits paged_attention
// writes for the same arguments. One grid split: the attention kernel's own epilogue, one launch, no workspace, for every hpw.
// Split-KV: paged_decode_kernel in part_mode + the fp8 merge, two launches instead of three.
template <typename T, int D>
int launch_paged_decode_fp8(const void* q, const void* kc, const void* vc, void* out, uint8_t* out_f8, const float* f8_scale,
                            const int32_t* kv_lens, const int32_t* block_table, int64_t max_blocks, int64_t batch, int64_t nq,
                            int64_t nkv, int64_t block_size, int64_t q_stride, int64_t max_kv_len, float scale,
                            int64_t window_left, void* workspace, size_t ws_bytes, hipStream_t s) {
  const int hpw = decode_heads_per_wg(batch, nkv);
  int nsplit = decode_num_splits(batch, nkv, hpw, max_kv_len);
  const size_t per_split = (size_t)batch * nq * (D + 2) * sizeof(float);
  if (!workspace) ws_bytes = 0;
  if ((size_t)nsplit * per_split > ws_bytes) nsplit = (int)(ws_bytes / per_split);
  if (nsplit < 1) nsplit = 1;
  float* part_o = nsplit > 1 ? reinterpret_cast<float*>(workspace) : nullptr;
  float* part_ml = part_o ? part_o + (size_t)batch * nq * nsplit * D : nullptr;
  const float scale_log2 = scale * 1.4426950408889634f;
  const dim3 grid((unsigned)(batch * (nkv / hpw) * nsplit));
  const int wl = window_left < 0 ? -1 : (window_left > 0x3fffffff ? 0x3fffffff : (int)window_left);
  const bool krows = hpw < nkv;
  const bool uniform = block_size % kTile == 0;
  if (nsplit > 1) {
    const int wide_store = (uintptr_t)part_o % 16 == 0;
#define XM_DECODE_PART8(UNI_, KROWS_)                                                                                          \
  hipLaunchKernelGGL((paged_decode_kernel<T, D, UNI_, false, KROWS_>), grid, dim3(256), 0, s, (const T*)q, (const T*)kc,        \
                     (const T*)vc, (T*)nullptr, part_o, part_ml, (const int32_t*)nullptr, kv_lens, block_table, (int)max_blocks, \
                     (int)nq, (int)nkv, (int)block_size, q_stride, scale_log2, nsplit, hpw, wl, (int8_t*)nullptr,               \
                     (float*)nullptr, 1, wide_store)
    if (uniform) {
      if (krows) XM_DECODE_PART8(true, true);
      else XM_DECODE_PART8(true, false);
    } else {
      if (krows) XM_DECODE_PART8(false, true);
      else XM_DECODE_PART8(false, false);
    }
#undef XM_DECODE_PART8
    hipLaunchKernelGGL((paged_decode_merge_fp8_kernel<T, D>), dim3((unsigned)(batch * nq)), dim3(D), 0, s, part_o, part_ml,
                       (T*)out, out_f8, f8_scale, (int)nq, nsplit);
    return hip_check_launch();
  }
  const int wide_store = ((uintptr_t)out % 16 == 0 ? 1 : 0) | ((uintptr_t)out_f8 % 8 == 0 ? 2 : 0);
#define XM_DECODE_F8(UNI_, KROWS_)                                                                                          \
  hipLaunchKernelGGL((paged_decode_kernel<T, D, UNI_, false, KROWS_, true>), grid, dim3(256), 0, s, (const T*)q, (const T*)kc, \
                     (const T*)vc, (T*)out, (float*)nullptr, (float*)nullptr, (const int32_t*)nullptr, kv_lens, block_table, \
                     (int)max_blocks, (int)nq, (int)nkv, (int)block_size, q_stride, scale_log2, 1, hpw, wl,                  \
                     reinterpret_cast<int8_t*>(out_f8), const_cast<float*>(f8_scale), 0, wide_store)
  if (uniform) {
    if (krows) XM_DECODE_F8(true, true);
    else XM_DECODE_F8(true, false);
  } else {
    if (krows) XM_DECODE_F8(false, true);
    else XM_DECODE_F8(false, false);
  }
#undef XM_DECODE_F8
  return hip_check_launch();
}

#define XM_DECODE_F8_INST(T, D)                                                                                            \
  template int launch_paged_decode_fp8<T, D>(const void*, const void*, const void*, void*, uint8_t*, const float*,         \
                                             const int32_t*, const int32_t*, int64_t, int64_t, int64_t, int64_t, int64_t,  \
                                             int64_t, int64_t, float, int64_t, void*, size_t, hipStream_t)
XM_DECODE_F8_INST(bf16_t, 128);
XM_DECODE_F8_INST(bf16_t, 64);
XM_DECODE_F8_INST(f16_t, 128);
XM_DECODE_F8_INST(f16_t, 64);
#undef XM_DECODE_F8_INST

// the suffix stage of shared-prefix decode (attention_shared_prefix.hip): the same kernel on the caller's plan (hpw, nsplit), always
// in part_mode -- (o, m, l) of every (sequence, head, split) at [(b * nq + head) * nsplit + split], log2 domain -- no window, no
// output row. A sequence of 0 tokens leaves (0, -1e30, 0).
template <typename T, int D>
int launch_paged_decode_partials(const void* q, const void* kc, const void* vc, float* part_o, float* part_ml,
                                 const int32_t* kv_lens, const int32_t* block_table, int64_t max_blocks, int64_t batch, int64_t nq,
                                 int64_t nkv, int64_t block_size, int64_t q_stride, float scale, int nsplit, int hpw, hipStream_t s) {
  const float scale_log2 = scale * 1.4426950408889634f;
  const dim3 grid((unsigned)(batch * (nkv / hpw) * nsplit));
  const int wide_store = (uintptr_t)part_o % 16 == 0;
  const bool krows = hpw < nkv;
#define XM_DECODE_PART(UNI_, KROWS_)                                                                                          \
  hipLaunchKernelGGL((paged_decode_kernel<T, D, UNI_, false, KROWS_>), grid, dim3(256), 0, s, (const T*)q, (const T*)kc,      \
                     (const T*)vc, (T*)nullptr, part_o, part_ml, (const int32_t*)nullptr, kv_lens, block_table, (int)max_blocks, \
                     (int)nq, (int)nkv, (int)block_size, q_stride, scale_log2, nsplit, hpw, -1, (int8_t*)nullptr,              \
                     (float*)nullptr, 1, wide_store)
  if (block_size % kTile == 0) {
    if (krows) XM_DECODE_PART(true, true);
    else XM_DECODE_PART(true, false);
  } else {
    if (krows) XM_DECODE_PART(false, true);
    else XM_DECODE_PART(false, false);
  }
#undef XM_DECODE_PART
  return hip_check_launch();
}

#define XM_DECODE_PART_INST(T, D)                                                                                         \
  template int launch_paged_decode_partials<T, D>(const void*, const void*, const void*, float*, float*, const int32_t*, \
                                                  const int32_t*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,   \
                                                  float, int, int, hipStream_t)
XM_DECODE_PART_INST(bf16_t, 128);
XM_DECODE_PART_INST(bf16_t, 64);
XM_DECODE_PART_INST(f16_t, 128);
XM_DECODE_PART_INST(f16_t, 64);
#undef XM_DECODE_PART_INST

template int launch_paged_decode<bf16_t, 128>(const void*, const void*, const void*, void*, const int32_t*,
                                              const int32_t*, const int32_t*, int64_t, int64_t, int64_t, int64_t,
                                              int64_t, int64_t, int64_t, float, int64_t, void*, size_t, hipStream_t, int8_t*, float*);
template int launch_paged_decode<bf16_t, 64>(const void*, const void*, const void*, void*, const int32_t*,
                                             const int32_t*, const int32_t*, int64_t, int64_t, int64_t, int64_t,
                                             int64_t, int64_t, int64_t, float, int64_t, void*, size_t, hipStream_t, int8_t*, float*);
template int launch_paged_decode<f16_t, 128>(const void*, const void*, const void*, void*, const int32_t*,
                                             const int32_t*, const int32_t*, int64_t, int64_t, int64_t, int64_t,
                                             int64_t, int64_t, int64_t, float, int64_t, void*, size_t, hipStream_t, int8_t*, float*);
template int launch_paged_decode<f16_t, 64>(const void*, const void*, const void*, void*, const int32_t*,
                                            const int32_t*, const int32_t*, int64_t, int64_t, int64_t, int64_t,
                                            int64_t, int64_t, int64_t, float, int64_t, void*, size_t, hipStream_t, int8_t*, float*);

}  // namespace xm

// attention_shared_prefix.hip -- decode attention over a KV prefix that many sequences share (DESIGN.md "shared-prefix decode").
//
// Reference semantics: the two-stage beam decode of layers/cuda/xattention.cpp:200-320 (a shared stage and an unshared stage, each
// with an LSE, combined by kernels/cuda/xattention/lse_combine.cu). Here the result is DEFINED as that of paged decode attention
// (attention_decode.hip) on the same tensors; the grouping only says which leading pages of which block-table rows are the same
// physical pages, so that they are fetched once per group instead of once per sequence.
//
// Four launches (xllm_mi355_paged_decode_attention_shared_prefix, attention_api.hip):
//  a. shared_prefix_prologue_kernel: suffix_len[b] = kv_lens[b] - P * block_size, prefix_tokens[b] = P * block_size and a block
//     table shifted left by P entries per row, so that
//  b. the suffix stage is paged_decode_kernel itself (launch_paged_decode_partials, attention_decode.hip), leaving (o, m, l);
//  c. shared_prefix_stage_kernel: per (group, kv head) the (sequence, q head) rows of the group are packed 16 to an MFMA N block
//     in the decode kernel's swapped form (S^T = K * Q^T, O^T = V^T * P^T, V through the wave's LDS tile and
//     ds_read_b64_tr_b16). A wave (= a workgroup) owns NB N blocks and one token range: every K / V fragment it fetches serves
//     all of its N blocks, and the waves of one (kv head, split) share an XCD's L2;
//  d. shared_prefix_merge_kernel: one workgroup per (sequence, head) combines the suffix partials with the shared ones.
#include "common.h"
#include "attention_traits.h"

namespace xm {

typedef unsigned sp_u32x4_t __attribute__((ext_vector_type(4)));

constexpr int kSpTile = 32;          // tokens per tile (= K dim of the PV MFMA)
constexpr float kSpNegBig = -1e30f;  // finite "-inf" of the running max (log2 domain), the decode kernel's

// ---- a. prologue: one wave per sequence. The group of b is found 64 groups at a time (one ballot per chunk).
__global__ __launch_bounds__(64) void shared_prefix_prologue_kernel(
    const int32_t* __restrict__ kv_lens, const int32_t* __restrict__ block_table, const int32_t* __restrict__ group_cu,
    const int32_t* __restrict__ group_prefix_blocks, int n_groups, int max_blocks, int block_size,
    int32_t* __restrict__ suffix_len, int32_t* __restrict__ prefix_tokens, int32_t* __restrict__ shifted) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int P = 0;
  for (int c = 0; c < n_groups; c += 64) {
    const int g = c + lane;
    const bool mine = g < n_groups && group_cu[g] <= b && b < group_cu[g + 1];
    const unsigned long long hit = __ballot(mine);
    if (hit) {
      P = group_prefix_blocks[c + __builtin_ctzll(hit)];
      break;
    }
  }
  P = P < 0 ? 0 : (P > max_blocks ? max_blocks : P);
  const int rest = kv_lens[b] - P * block_size;
  if (lane == 0) {
    suffix_len[b] = rest > 0 ? rest : 0;
    prefix_tokens[b] = P * block_size;
  }
  const int32_t* src = block_table + (int64_t)b * max_blocks;
  int32_t* dst = shifted + (int64_t)b * max_blocks;
  for (int j = lane; j < max_blocks; j += 64) dst[j] = j + P < max_blocks ? src[j + P] : 0;
}

// ---- c. the shared stage. One wave per workgroup; NB N blocks of 16 rows per wave (rows_per_tile = 16 * NB).
// Block order: u = kv head * nsplit + split names one K / V stream; with at least 8 streams, stream u lives on XCD u % 8 (block x
// runs on XCD x % 8: observed, relied on for speed only) and the row tiles of a stream follow each other there.
// UNIFORM: block_size % 32 == 0, a tile lives in one page and its table entry is one scalar load.
template <typename T, int D, int NB, bool UNIFORM>
__global__ __launch_bounds__(64) void shared_prefix_stage_kernel(
    const T* __restrict__ q, const T* __restrict__ kc, const T* __restrict__ vc, float* __restrict__ part_o,
    float* __restrict__ part_ml, const int32_t* __restrict__ block_table, const int32_t* __restrict__ group_cu,
    const int32_t* __restrict__ group_prefix_blocks, int n_groups, int max_blocks, int nq, int nkv, int block_size,
    int64_t q_stride, float scale_log2, int nsplit, int n_row_tiles) {
  using TR = AttnTraits<T>;
  using x8 = typename TR::x8;
  using x4 = typename TR::x4;
  using elem = typename TR::elem;
  constexpr int KK = D / 32;        // MFMA k-steps over the head dim
  constexpr int CH = D * 2 / 16;    // 16-byte chunks per K/V row
  constexpr int TPI = 64 / CH;      // V rows fetched per wave-wide load instruction
  constexpr int NV = kSpTile / TPI; // V load instructions per tile
  constexpr int DB = D / 16;        // 16-wide output d blocks
  constexpr int RSB = D * 2 + 32;   // padded LDS row stride in bytes
  constexpr int RPT = 16 * NB;      // rows per tile

  __shared__ __attribute__((aligned(16))) char lds[kSpTile * RSB];

  const int lane = threadIdx.x;
  const int p16 = lane & 15, g4 = lane >> 4;
  const int G = nq / nkv;

  // ---- block -> (row tile, kv head, split)
  const int U = nkv * nsplit;
  int u, rt;
  if (U >= 8) {
    const int per_x = (U + 7) / 8;
    const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
    u = x + 8 * (j % per_x);
    rt = j / per_x;
  } else {
    u = blockIdx.x % U;
    rt = blockIdx.x / U;
  }
  if (u >= U || rt >= n_row_tiles) return;
  const int kvh = u / nsplit, split = u % nsplit;

  // ---- row tile -> (group, tile of the group): groups without a prefix have no tile; 64 groups per step, a wave-wide
  //      inclusive scan of the tile counts and one ballot
  int grp = -1, lt = 0;
  {
    int base = 0;
    for (int c = 0; c < n_groups; c += 64) {
      const int g = c + lane;
      int nt = 0;
      if (g < n_groups && group_prefix_blocks[g] > 0) nt = ((group_cu[g + 1] - group_cu[g]) * G + RPT - 1) / RPT;
      int incl = nt;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
      }
      const unsigned long long hit = __ballot(nt > 0 && rt < base + incl);
      if (hit) {
        const int src = __builtin_ctzll(hit);
        grp = c + src;
        lt = rt - base - (__shfl(incl, src) - __shfl(nt, src));
        break;
      }
      base += __shfl(incl, 63);
    }
  }
  if (grp < 0) return;
  grp = __builtin_amdgcn_readfirstlane(grp);
  lt = __builtin_amdgcn_readfirstlane(lt);
  const int b0 = group_cu[grp];
  const int n_rows = (group_cu[grp + 1] - b0) * G;
  int P = group_prefix_blocks[grp];
  P = P > max_blocks ? max_blocks : P;
  const int PT = P * block_size;  // shared tokens

  const int ntiles = (PT + kSpTile - 1) / kSpTile;
  const int per = (ntiles + nsplit - 1) / nsplit;
  int my_lo = split * per;
  int my_hi = my_lo + per < ntiles ? my_lo + per : ntiles;
  my_lo = __builtin_amdgcn_readfirstlane(my_lo);
  my_hi = __builtin_amdgcn_readfirstlane(my_hi);

  const int32_t* bt_row = block_table + (int64_t)b0 * max_blocks;  // the leader's row: rows of the group agree on [0, P)
  const int64_t row_elems = (int64_t)nkv * D;

  // ---- Q as the MFMA B operand: lane (n = row p16 of N block nb, k group g4) holds Q[row][(kk*4+g4)*8 .. +7]
  x8 qf[NB][KK];
  int64_t pi[NB];      // partial index of the lane's row per N block, -1 for a padding row
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int idx = lt * RPT + nb * 16 + p16;
    const bool live = idx < n_rows;
    const int b = b0 + idx / G, qq = idx % G;
    const int head = kvh * G + qq;
    pi[nb] = live ? ((int64_t)b * nq + head) * nsplit + split : -1;
    const T* qp = q + (int64_t)b * q_stride + (int64_t)head * D;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      if (live) qf[nb][kk] = *reinterpret_cast<const x8*>(qp + (kk * 4 + g4) * 8);
      else qf[nb][kk] = x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }

  f32x4_t acc_o[NB][DB];
  float m_run[NB], l_run[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    m_run[nb] = kSpNegBig;
    l_run[nb] = 0.0f;
#pragma unroll
    for (int i = 0; i < DB; ++i) acc_o[nb][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  // ---- K straight into the MFMA A-operand layout: lane (p16, g4) holds K[token blk*16 + p16][(kk*4+g4)*8 .. +7]; V as whole
  //      rows. Token indices past the prefix are clamped to its last token (masked below), a tile past the wave's range
  //      re-loads its last tile (unconditional loads, as in the decode kernel); ordinary loads: the stream is read by every
  //      row tile of the group and should stay in the L2. Two named register stages: tile t + 1 is in flight while t is
  //      computed (a third stage spills at d = 128: 24 bytes of scratch per lane)
  x8 ka[2][KK], kb[2][KK];
  sp_u32x4_t va[NV], vb[NV];
  auto issue_loads = [&](int tile, x8 (&kf)[2][KK], sp_u32x4_t (&vr)[NV]) {
    tile = tile < my_hi ? tile : my_hi - 1;
    const int t0 = tile * kSpTile;
    int64_t page_row = 0;  // UNIFORM: first cache row of the tile's page
    if constexpr (UNIFORM) page_row = (int64_t)bt_row[t0 / block_size] * block_size;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      int tok = t0 + blk * 16 + p16;
      tok = tok < PT ? tok : PT - 1;
      const int64_t rowi = (UNIFORM ? page_row : (int64_t)bt_row[tok / block_size] * block_size) + (tok % block_size);
      const T* kp = kc + rowi * row_elems + (int64_t)kvh * D + g4 * 8;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) kf[blk][kk] = *reinterpret_cast<const x8*>(kp + kk * 32);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      int tok = t0 + i * TPI + lane / CH;
      tok = tok < PT ? tok : PT - 1;
      const int64_t rowi = (UNIFORM ? page_row : (int64_t)bt_row[tok / block_size] * block_size) + (tok % block_size);
      vr[i] = *reinterpret_cast<const sp_u32x4_t*>(vc + rowi * row_elems + (int64_t)kvh * D + (lane % CH) * 8);
    }
  };

  auto compute_tile = [&](int tile, const x8 (&kf)[2][KK], const sp_u32x4_t (&vr)[NV]) {
    const int t0 = tile * kSpTile;
    const bool partial = t0 + kSpTile > PT;
    // ---- V tile -> LDS (row major, padded rows); rows past the prefix zeroed (they meet p = 0 in the PV MFMA). The LDS serves
    //      a wave's requests in order, so these writes cannot overtake the previous tile's transposed reads
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int r = i * TPI + lane / CH;
      sp_u32x4_t v = vr[i];
      if (partial && t0 + r >= PT) v = sp_u32x4_t{0u, 0u, 0u, 0u};
      *reinterpret_cast<sp_u32x4_t*>(lds + r * RSB + (lane % CH) * 16) = v;
    }
    // ---- per N block: S^T = K * Q^T (lane holds S[row p16][token blk*16 + 4 g4 + r]), online softmax in the log2 domain,
    //      P as hi + lo 16-bit parts (attention_decode.hip: p = hi + lo to ~2^-17 relative)
    x8 pf[NB], pl[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      f32x4_t s[2];
#pragma unroll
      for (int blk = 0; blk < 2; ++blk) {
        s[blk] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) s[blk] = TR::mfma(kf[blk][kk], qf[nb][kk], s[blk]);
      }
      float mx = kSpNegBig;
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = s[blk][r] * scale_log2;
          if (partial && t0 + blk * 16 + g4 * 4 + r >= PT) v = -INFINITY;
          s[blk][r] = v;
          mx = fmaxf(mx, v);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float m_new = fmaxf(m_run[nb], mx);
      const float alpha = exp2f(m_run[nb] - m_new);
      m_run[nb] = m_new;
      float psum = 0.0f;
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = exp2f(s[blk][r] - m_new);
          psum += p;
          const elem hi = (elem)p;
          pf[nb][blk * 4 + r] = hi;
          pl[nb][blk * 4 + r] = (elem)(p - (float)hi);
        }
      l_run[nb] = l_run[nb] * alpha + psum;
#pragma unroll
      for (int i = 0; i < DB; ++i) acc_o[nb][i] *= alpha;
    }
    // ---- O^T += V^T * P^T : every transposed V fragment is read once and used by all N blocks
    const char* trb = lds + (4 * g4 + (p16 >> 2)) * RSB + (p16 & 3) * 8;
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      const x4 lo = TR::tr_read(trb + db * 32);
      const x4 hi = TR::tr_read(trb + 16 * RSB + db * 32);
      x8 vt;
      vt[0] = lo[0]; vt[1] = lo[1]; vt[2] = lo[2]; vt[3] = lo[3];
      vt[4] = hi[0]; vt[5] = hi[1]; vt[6] = hi[2]; vt[7] = hi[3];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        acc_o[nb][db] = TR::mfma(vt, pf[nb], acc_o[nb][db]);
        acc_o[nb][db] = TR::mfma(vt, pl[nb], acc_o[nb][db]);
      }
    }
  };

  if (my_lo < my_hi) {
    int tile = my_lo;
    issue_loads(tile, ka, va);
    while (true) {
      issue_loads(tile + 1, kb, vb);
      compute_tile(tile, ka, va);
      if (++tile >= my_hi) break;
      issue_loads(tile + 1, ka, va);
      compute_tile(tile, kb, vb);
      if (++tile >= my_hi) break;
    }
  }

  // ---- (o, m, l) of every live row; a split without a tile leaves (0, -1e30, 0). Lane (p16, g4) holds O[row p16][db*16 + 4 g4 ..]
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    float l = l_run[nb];
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (pi[nb] >= 0) {
      float* po = part_o + pi[nb] * D + g4 * 4;
#pragma unroll
      for (int db = 0; db < DB; ++db) *reinterpret_cast<f32x4_t*>(po + db * 16) = acc_o[nb][db];
      if (g4 == 0) *reinterpret_cast<float2*>(part_ml + pi[nb] * 2) = make_float2(m_run[nb], l);
    }
  }
}

// ---- d. merge: one workgroup (D threads) per (sequence, head); the arithmetic of paged_decode_merge_kernel over the suffix
//      partials followed by the shared ones (skipped when the sequence has no shared prefix: nothing was written for it)
template <typename T, int D>
__global__ __launch_bounds__(D) void shared_prefix_merge_kernel(const float* __restrict__ suf_o, const float* __restrict__ suf_ml,
                                                                const float* __restrict__ pre_o, const float* __restrict__ pre_ml,
                                                                const int32_t* __restrict__ prefix_tokens, T* __restrict__ out,
                                                                int nq, int suffix_nsplit, int prefix_nsplit) {
  const int b = blockIdx.x / nq, head = blockIdx.x % nq;
  const int d = threadIdx.x;
  const int64_t sbase = ((int64_t)b * nq + head) * suffix_nsplit;
  const int64_t pbase = ((int64_t)b * nq + head) * prefix_nsplit;
  const int np = prefix_tokens[b] > 0 ? prefix_nsplit : 0;
  float m_star = kSpNegBig;
  for (int s = 0; s < suffix_nsplit; ++s) m_star = fmaxf(m_star, suf_ml[(sbase + s) * 2]);
  for (int s = 0; s < np; ++s) m_star = fmaxf(m_star, pre_ml[(pbase + s) * 2]);
  float o = 0.0f, l = 0.0f;
  for (int s = 0; s < suffix_nsplit; ++s) {
    const float f = exp2f(suf_ml[(sbase + s) * 2] - m_star);
    o += f * suf_o[(sbase + s) * D + d];
    l += f * suf_ml[(sbase + s) * 2 + 1];
  }
  for (int s = 0; s < np; ++s) {
    const float f = exp2f(pre_ml[(pbase + s) * 2] - m_star);
    o += f * pre_o[(pbase + s) * D + d];
    l += f * pre_ml[(pbase + s) * 2 + 1];
  }
  out[(int64_t)b * nq * D + (int64_t)head * D + d] = from_f32<T>(l > 0.0f ? o / l : 0.0f);
}

template <typename T, int D>
int launch_paged_decode_partials(const void* q, const void* kc, const void* vc, float* part_o, float* part_ml,
                                 const int32_t* kv_lens, const int32_t* block_table, int64_t max_blocks, int64_t batch, int64_t nq,
                                 int64_t nkv, int64_t block_size, int64_t q_stride, float scale, int nsplit, int hpw, hipStream_t s);

int shared_prefix_rows_per_tile() { return 32; }

// splits of the shared stage: at most one wave per SIMD (1024: the kernel's registers leave room for one, and a second round of
// waves would only wait for the first) while every wave keeps >= 4 tiles; at most 8
int shared_prefix_num_splits(int64_t batch, int64_t nq, int64_t nkv, int64_t block_size, int64_t max_prefix_blocks) {
  const int64_t G = nq / nkv, rpt = shared_prefix_rows_per_tile();
  const int64_t waves = ((batch * G + rpt - 1) / rpt) * nkv;
  const int64_t tiles = (max_prefix_blocks * block_size + kSpTile - 1) / kSpTile;
  int64_t n = 1024 / (waves > 0 ? waves : 1);
  const int64_t by_len = tiles / 4 > 1 ? tiles / 4 : 1;
  n = n > by_len ? by_len : n;
  n = n > 8 ? 8 : n;
  return (int)(n < 1 ? 1 : n);
}

// workspace layout (bytes, every region 16-byte aligned): [suffix_len B][prefix_tokens B][shifted table B * max_blocks] int32,
// then the suffix partials (o then ml), then the shared partials (o then ml)
static inline size_t sp_align16(size_t v) { return (v + 15) / 16 * 16; }

template <typename T, int D>
int launch_shared_prefix_decode(const void* q, const void* kc, const void* vc, void* out, const int32_t* kv_lens,
                                const int32_t* block_table, int64_t max_blocks, const int32_t* group_cu,
                                const int32_t* group_prefix_blocks, int64_t n_groups, int64_t batch, int64_t nq, int64_t nkv,
                                int64_t block_size, int64_t q_stride, float scale, int suffix_hpw, int suffix_nsplit,
                                int prefix_nsplit, void* workspace, hipStream_t s) {
  constexpr int NB = 2;
  char* w = static_cast<char*>(workspace);
  int32_t* suffix_len = reinterpret_cast<int32_t*>(w);
  int32_t* prefix_tokens = suffix_len + batch;
  int32_t* shifted = prefix_tokens + batch;
  w += sp_align16((size_t)(2 * batch + batch * max_blocks) * sizeof(int32_t));
  float* suf_o = reinterpret_cast<float*>(w);
  float* suf_ml = suf_o + (size_t)batch * nq * suffix_nsplit * D;
  w += sp_align16((size_t)batch * nq * suffix_nsplit * (D + 2) * sizeof(float));
  float* pre_o = reinterpret_cast<float*>(w);
  float* pre_ml = pre_o + (size_t)batch * nq * prefix_nsplit * D;

  hipLaunchKernelGGL(shared_prefix_prologue_kernel, dim3((unsigned)batch), dim3(64), 0, s, kv_lens, block_table, group_cu,
                     group_prefix_blocks, (int)n_groups, (int)max_blocks, (int)block_size, suffix_len, prefix_tokens, shifted);
  int rc = launch_paged_decode_partials<T, D>(q, kc, vc, suf_o, suf_ml, suffix_len, shifted, max_blocks, batch, nq, nkv, block_size,
                                              q_stride, scale, suffix_nsplit, suffix_hpw, s);
  if (rc != XM_OK) return rc;
  const int G = (int)(nq / nkv);
  const int n_row_tiles = (int)((batch * G + 16 * NB - 1) / (16 * NB) + n_groups);
  const int U = (int)nkv * prefix_nsplit;
  const unsigned blocks = (unsigned)n_row_tiles * (unsigned)(U >= 8 ? (U + 7) / 8 * 8 : U);
#define XM_SP_STAGE(UNI_)                                                                                                  \
  hipLaunchKernelGGL((shared_prefix_stage_kernel<T, D, NB, UNI_>), dim3(blocks), dim3(64), 0, s, (const T*)q, (const T*)kc, \
                     (const T*)vc, pre_o, pre_ml, block_table, group_cu, group_prefix_blocks, (int)n_groups, (int)max_blocks, \
                     (int)nq, (int)nkv, (int)block_size, q_stride, scale * 1.4426950408889634f, prefix_nsplit, n_row_tiles)
  if (block_size % kSpTile == 0) XM_SP_STAGE(true);
  else XM_SP_STAGE(false);
#undef XM_SP_STAGE
  hipLaunchKernelGGL((shared_prefix_merge_kernel<T, D>), dim3((unsigned)(batch * nq)), dim3(D), 0, s, suf_o, suf_ml, pre_o, pre_ml,
                     prefix_tokens, (T*)out, (int)nq, suffix_nsplit, prefix_nsplit);
  return hip_check_launch();
}

#define XM_SP_INST(T, D)                                                                                                      \
  template int launch_shared_prefix_decode<T, D>(const void*, const void*, const void*, void*, const int32_t*, const int32_t*, \
                                                 int64_t, const int32_t*, const int32_t*, int64_t, int64_t, int64_t, int64_t,  \
                                                 int64_t, int64_t, float, int, int, int, void*, hipStream_t)
XM_SP_INST(bf16_t, 128);
XM_SP_INST(bf16_t, 64);
XM_SP_INST(f16_t, 128);
XM_SP_INST(f16_t, 64);
#undef XM_SP_INST

}  // namespace xm

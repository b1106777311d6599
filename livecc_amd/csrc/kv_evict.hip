// Sliding KV window: remove the rows [first, first + n) of ONE stream's KV arena in place (compaction).  No reference counterpart:
// ref demo/infer.py:61-180 grows `past_key_values` without bound; in HF terms this is `cat(keys[:, :, :first], keys[:, :, first + n:])`
// on every layer of a DynamicCache, on the arena layout of kernels.h:
//   K plane [Lmax][128]        : rows first + n .. L move down by n rows (256 B each);
//   V plane [Lmax/32][128][32] : key j lives in block j / 32, column j % 32, so a shift by n keys is a shift by n / 32 blocks plus a
//                                ROTATION of every 64-byte (block, channel) row by n % 32 columns across two neighbouring source blocks;
//   rows [L - n, L) become zero in both layouts (the attention kernels read whole 32-key V blocks past kv_len); rows >= L and rows
//   < first are not written (the V piece that straddles such a boundary is read-modified-written with the bytes it already holds).
// A bandwidth kernel: 16-byte global loads / stores only, no MFMA.  Both layouts are processed in units of one 32-key block (8 KB, and
// contiguous in either layout): a workgroup takes NB consecutive destination blocks of one plane per iteration, loads everything
// they need (K: into registers, V: NB + 1 source blocks into LDS), passes a barrier, and only then stores.
//
// IN-PLACE SCHEME (design (b) of the issue: one pass, ordering by workgroup ownership and by successive launches -- no scratch buffer, no
// cross-workgroup flag).  Source and destination overlap whenever the tail is longer than n.  Two launch shapes of the SAME kernel:
//   * windows: a launch covers, in every plane, destination blocks [da, db) with 32 * db <= (first row it writes) + n.  Every source row
//     it needs is then at or above block db, i.e. outside everything the launch writes, so any number of workgroups per plane may run
//     in any order.  The next window starts at db; launches on one stream are the ordering primitive.  Taken when n >= 64 and at most
//     MAX_WINDOWS launches cover the tail (the planner's case: the oldest ~half of the window is dropped, 2-3 launches).
//   * one workgroup per plane (any n, any tail): the workgroup walks its plane's destination blocks in ascending order.  Within an
//     iteration all loads complete before the barrier that precedes the stores; a later iteration reads only blocks above everything
//     written so far (source block = destination block + n / 32, + 1).  Planes are disjoint, so workgroups never meet.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace lcc {

constexpr int EV_NB = 6;            // destination blocks per workgroup iteration (V: (NB + 1) x 8 KB = 56 KB of LDS)
constexpr int EV_THREADS = 1024;
constexpr int EV_PIECES = 512;      // 16-byte pieces of one 32-key block
constexpr int EV_MAX_WINDOWS = 8;

// 16-bit elements R .. R + 8 of the 16 held by lo | hi
template <int R>
LCC_DEVICE u32x4 take8(u32x4 lo, u32x4 hi) {
  const unsigned w[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  u32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = R + 2 * i;
    o[i] = (e & 1) ? __builtin_amdgcn_alignbit(w[e / 2 + 1], w[e / 2], 16) : w[e / 2];
  }
  return o;
}
LCC_DEVICE u32x4 take8_dyn(int r, u32x4 lo, u32x4 hi) {   // r is workgroup-uniform
  switch (r) {
    case 0: return lo;
    case 1: return take8<1>(lo, hi);
    case 2: return take8<2>(lo, hi);
    case 3: return take8<3>(lo, hi);
    case 4: return take8<4>(lo, hi);
    case 5: return take8<5>(lo, hi);
    case 6: return take8<6>(lo, hi);
    default: return take8<7>(lo, hi);
  }
}

// REBASE: the 16-byte piece `w` of a K row (channels 8c .. 8c + 8 of lane `t & 15 == c`) rotated with its partner piece (channels +- 64),
// which lane t ^ 8 of the same 16-lane DPP row holds: row_ror:8 brings it over, one move per dword.  cs[e] / sn[e] = cos / sin of the
// shift angle of channel pair 8 (c & 7) + e, sn already negated in the upper half (k'[i + 64] = k[i + 64] c - k[i] s).  fp32, one RNE.
LCC_DEVICE u32x4 rebase_piece(u32x4 w, const float (&cs)[8], const float (&sn)[8]) {
  u32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned p = (unsigned)__builtin_amdgcn_update_dpp(0, (int)w[j], 0x128 /* row_ror:8 */, 0xf, 0xf, false);
    o[j] = pack2(lo2f(w[j]) * cs[2 * j] + lo2f(p) * sn[2 * j], hi2f(w[j]) * cs[2 * j + 1] + hi2f(p) * sn[2 * j + 1]);
  }
  return o;
}

// grid (G, planes): workgroup g of plane p owns destination blocks [blk_lo + g * per, min(blk_hi, blk_lo + (g + 1) * per)).
// REBASE (sliding window with positions inside the cache): every K row that moves is also rotated by the angle of -n positions,
//   k'[i] = k[i] c_i + k[i + 64] s_i,  k'[i + 64] = k[i + 64] c_i - k[i] s_i,  c_i | s_i = rot[i] | rot[64 + i] = cos | sin(n * inv_freq[i]),
// HF's `k * cos + rotate_half(k) * sin` at -n * theta_i, between the loads and the barrier; V, the zeroed rows and the launch shapes are
// those of the plain form, whose instantiation (REBASE = false) does not read `rot`.
template <bool REBASE>
__global__ __launch_bounds__(EV_THREADS) void kv_evict_kernel(bf16_t* base, KvLayout lay, int L, int first, int n, int blk_lo,
                                                              int blk_hi, int per, const float* __restrict__ rot) {
  __shared__ u32x4 lds[(EV_NB + 1) * EV_PIECES];
  const int t = threadIdx.x;
  const int plane = blockIdx.y;                       // (layer * 2 + kv) * Hkv + head: the arena order of kernels.h
  const bool is_v = (plane / lay.n_kv_heads) & 1;
  u32x4* P = reinterpret_cast<u32x4*>(base + (size_t)plane * lay.head_stride());   // 16 pieces per K row, 512 per block
  const int b0 = blk_lo + blockIdx.x * per, b1 = min(blk_hi, b0 + per);
  const int keep_to = L - n;                          // rows [first, keep_to) take row + n; rows [keep_to, L) become zero
  const u32x4 zero = {0u, 0u, 0u, 0u};
  if (!is_v) {
    float cs[8], sn[8];                               // REBASE: this thread's piece index is t & 15 in every iteration
    if constexpr (REBASE) {
      const int c = t & 15;
#pragma unroll
      for (int e = 0; e < 8; ++e) {                   // once per thread (the table is only 4-byte aligned: dword loads)
        cs[e] = rot[(c & 7) * 8 + e];
        sn[e] = c < 8 ? rot[64 + (c & 7) * 8 + e] : -rot[64 + (c & 7) * 8 + e];
      }
    }
    for (int x = b0; x < b1; x += EV_NB) {
      const int nb = min(EV_NB, b1 - x);
      u32x4 v[EV_NB * EV_PIECES / EV_THREADS];
#pragma unroll
      for (int i = 0; i < EV_NB * EV_PIECES / EV_THREADS; ++i) {
        const int o = i * EV_THREADS + t, row = x * 32 + (o >> 4);
        v[i] = zero;
        if (o < nb * EV_PIECES && row >= first && row < keep_to) v[i] = P[(size_t)(row + n) * 16 + (o & 15)];
      }
#pragma unroll
      for (int i = 0; i < EV_NB * EV_PIECES / EV_THREADS; ++i) settle_load(v[i]);   // the values are in registers before the barrier
      if constexpr (REBASE) {
#pragma unroll
        for (int i = 0; i < EV_NB * EV_PIECES / EV_THREADS; ++i) {   // every lane takes part in the DPP move; a lane and its partner share
          const int o = i * EV_THREADS + t, row = x * 32 + (o >> 4);   // the row, hence the guard.  Zeroed rows stay +0 bit for bit
          const u32x4 r = rebase_piece(v[i], cs, sn);
          if (o < nb * EV_PIECES && row >= first && row < keep_to) v[i] = r;
        }
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < EV_NB * EV_PIECES / EV_THREADS; ++i) {
        const int o = i * EV_THREADS + t, row = x * 32 + (o >> 4);
        if (o < nb * EV_PIECES && row >= first && row < L) P[(size_t)row * 16 + (o & 15)] = v[i];
      }
    }
    return;
  }
  const int q = n >> 5, s = n & 31;
  const int src_end = (L + 31) >> 5;                  // source blocks at or above this hold no cached key
  for (int x = b0; x < b1; x += EV_NB) {
    const int nb = min(EV_NB, b1 - x);
    __syncthreads();                                  // the previous iteration's LDS reads are done
    for (int o = t; o < (nb + 1) * EV_PIECES; o += EV_THREADS) {
      const int sb = x + q + o / EV_PIECES;
      if (sb < src_end) lds[o] = P[(size_t)sb * EV_PIECES + (o % EV_PIECES)];
    }
    __syncthreads();
    for (int o = t; o < nb * EV_PIECES; o += EV_THREADS) {
      const int db = o / EV_PIECES, ch = (o >> 2) & 127, p = o & 3;
      const int j0 = (x + db) * 32 + p * 8;           // first destination key of this piece
      if (j0 + 8 <= first || j0 >= L) continue;
      u32x4 r = zero;
      if (j0 < keep_to) {                             // chunks c0, c0 + 1 of the 64-column row (block db | block db + 1) of channel ch
        const int c0 = p + (s >> 3), c1 = c0 + 1;
        const u32x4 lo = lds[(db + (c0 >> 2)) * EV_PIECES + ch * 4 + (c0 & 3)];
        const u32x4 hi = lds[(db + (c1 >> 2)) * EV_PIECES + ch * 4 + (c1 & 3)];
        r = take8_dyn(s & 7, lo, hi);
      }
      u32x4* dst = P + (size_t)(x + db) * EV_PIECES + ch * 4 + p;
      if (j0 < first || j0 + 8 > keep_to) {           // a boundary piece: per key keep / shifted / zero / keep
        const u32x4 old = *dst;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int j = j0 + e;
          const unsigned m = 0xffffu << ((e & 1) * 16);
          if (j < first || j >= L) r[e >> 1] = (r[e >> 1] & ~m) | (old[e >> 1] & m);
          else if (j >= keep_to) r[e >> 1] &= ~m;
        }
      }
      *dst = r;
    }
  }
}

__global__ __launch_bounds__(256) void seen_set_slot_kernel(uint32_t* __restrict__ seen_row, const int32_t* __restrict__ ids, int n, int vocab) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int id = ids[i];
  if (id >= 0 && id < vocab) atomicOr(seen_row + (id >> 5), 1u << (id & 31));
}
int seen_set_slot(uint32_t* seen_row, const int32_t* ids, int n, int vocab, hipStream_t st) {
  if (n <= 0) return 0;
  seen_set_slot_kernel<<<dim3((n + 255) / 256), dim3(256), 0, st>>>(seen_row, ids, n, vocab);
  return 0;
}

int kv_evict_check(KvLayout lay, int kv_len, int first, int n) {
  if (lay.n_layers < 1 || lay.n_kv_heads < 1 || lay.head_dim != 128 || lay.lmax < 32 || (lay.lmax & 31)) return LCC_ERR_SHAPE;
  if (kv_len < 0 || kv_len > lay.lmax || first < 0 || n < 1 || first > kv_len || n > kv_len - first) return LCC_ERR_STATE;
  return 0;
}

// launches of kv_evict over one arena: windows of disjoint source / destination blocks, or one workgroup per plane (file header)
// rot: nullptr = plain compaction, else device fp32 [2][64] (cos | sin of the shift angle per channel pair) = compaction + re-rotation of K
int kv_evict(bf16_t* kv_base, KvLayout lay, int kv_len, int first, int n, int cu_count, hipStream_t st, const float* rot) {
  if (!kv_base || ((uintptr_t)kv_base & 15) || ((uintptr_t)rot & 3)) return LCC_ERR_ALIGN;
  if (int r = kv_evict_check(lay, kv_len, first, n)) return r;
  const int planes = lay.n_layers * 2 * lay.n_kv_heads;
  const int blk0 = first >> 5, blk_end = (kv_len + 31) >> 5, q = n >> 5;
  auto launch = [&](int lo, int hi, int G) {
    const int per = (hi - lo + G - 1) / G;
    G = (hi - lo + per - 1) / per;
    if (rot) kv_evict_kernel<true><<<dim3(G, planes), dim3(EV_THREADS), 0, st>>>(kv_base, lay, kv_len, first, n, lo, hi, per, rot);
    else kv_evict_kernel<false><<<dim3(G, planes), dim3(EV_THREADS), 0, st>>>(kv_base, lay, kv_len, first, n, lo, hi, per, nullptr);
  };
  const int w1 = std::min(blk_end, (first + n) >> 5);                     // end of the first window
  const int windows = n >= 64 ? 1 + (blk_end - w1 + q - 1) / q : EV_MAX_WINDOWS + 1;
  if (windows <= EV_MAX_WINDOWS) {
    const int g_max = std::max(1, 8 * std::max(cu_count, 1) / planes);   // about 8 workgroups per CU in flight over the launch
    for (int lo = blk0, hi = w1; lo < blk_end; lo = hi, hi = std::min(blk_end, hi + q)) {
      if (hi > lo) launch(lo, hi, std::min(g_max, (hi - lo + EV_NB - 1) / EV_NB));
    }
  } else {
    launch(blk0, blk_end, 1);
  }
  return 0;
}

}  // namespace lcc

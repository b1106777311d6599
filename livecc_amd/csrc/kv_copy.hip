// KV fork: copy the first n cached rows of ONE stream's KV arena into ANOTHER arena of the same layout.  No reference counterpart; in
// HF terms `copy.deepcopy(past_key_values)` of a DynamicCache, on the arena layout of kernels.h:
//   K plane [Lmax][128]        : rows [0, n) are copied (256 B each);
//   V plane [Lmax/32][128][32] : key j lives in block j / 32, column j % 32, so rows [0, n) are blocks [0, n / 32) whole plus the first
//                                n % 32 columns of every channel row of block n / 32;
//   rows [n, ceil32(n)) of the destination become zero in both layouts (the attention kernels read whole 32-key V blocks past kv_len;
//   kv_evict zeroes its vacated rows for the same reason); destination rows at or above ceil32(n) and the source are not written.
// A bandwidth kernel: 16-byte global loads / stores only, no LDS, no barrier.  The unit is one 32-key block (8 KB, contiguous in either
// layout), so a full block is the same straight copy in a K and in a V plane and only the last, partial block knows the layouts apart:
// a K piece (8 channels of one row) whose row is at or above n is stored as zero, a V piece (8 keys of one channel) that straddles n is
// masked in registers.  Source and destination never overlap (the callers check), every block is independent: ONE launch over a
// (G, planes) grid, workgroup g of plane p owning a contiguous range of blocks; a thread issues CP_UNROLL loads before its first store.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace lcc {

constexpr int CP_THREADS = 256;
constexpr int CP_PIECES = 512;      // 16-byte pieces of one 32-key block
constexpr int CP_UNROLL = 8;        // loads in flight per thread: CP_THREADS * CP_UNROLL pieces = 4 blocks (32 KB) per workgroup iteration
constexpr int CP_NB = CP_THREADS * CP_UNROLL / CP_PIECES;

// grid (G, planes): workgroup g of plane p owns blocks [g * per, min(n_blk, (g + 1) * per)); n_blk = ceil(n / 32)
template <bool NT>
__global__ __launch_bounds__(CP_THREADS) void kv_copy_kernel(bf16_t* __restrict__ dst_base, const bf16_t* __restrict__ src_base, KvLayout lay,
                                                             int n, int n_blk, int per) {
  const int t = threadIdx.x;
  const int plane = blockIdx.y;                       // (layer * 2 + kv) * Hkv + head: the arena order of kernels.h
  const bool is_v = (plane / lay.n_kv_heads) & 1;
  const size_t plane_off = (size_t)plane * lay.head_stride();
  const u32x4* S = reinterpret_cast<const u32x4*>(src_base + plane_off);   // 16 pieces per K row, 512 per block
  u32x4* D = reinterpret_cast<u32x4*>(dst_base + plane_off);
  const int b0 = blockIdx.x * per, b1 = min(n_blk, b0 + per);
  const int full = n >> 5;                            // blocks below this hold cached rows only
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int x = b0; x < b1; x += CP_NB) {
    const int np = min(CP_NB, b1 - x) * CP_PIECES;    // pieces of this iteration
    const size_t base = (size_t)x * CP_PIECES;
    u32x4 v[CP_UNROLL];
#pragma unroll
    for (int i = 0; i < CP_UNROLL; ++i) {
      const int o = i * CP_THREADS + t;
      v[i] = zero;
      if (o < np) {
        const int blk = x + o / CP_PIECES, w = o % CP_PIECES;
        // first key of the piece: K = its row, V = the first of its 8 keys (piece w of a V block = channel w / 4, keys 8 * (w % 4) ..)
        const int j0 = blk * 32 + (is_v ? (w & 3) * 8 : (w >> 4));
        if (blk < full || j0 < n) {
          v[i] = NT ? __builtin_nontemporal_load(S + base + o) : S[base + o];
          if (is_v && j0 + 8 > n) {                   // the V piece that straddles n: keys at or above n become zero
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (j0 + e >= n) v[i][e >> 1] &= ~(0xffffu << ((e & 1) * 16));
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < CP_UNROLL; ++i) {
      const int o = i * CP_THREADS + t;
      if (o < np) {
        if (NT) __builtin_nontemporal_store(v[i], D + base + o);
        else D[base + o] = v[i];
      }
    }
  }
}

int kv_copy_check(KvLayout lay, int n) {
  if (lay.n_layers < 1 || lay.n_kv_heads < 1 || lay.head_dim != 128 || lay.lmax < 32 || (lay.lmax & 31)) return LCC_ERR_SHAPE;
  if (n < 0 || n > lay.lmax) return LCC_ERR_STATE;
  return 0;
}

// 1: non-temporal loads and stores.  The plain form is an UNMEASURED default: neither form has been timed yet (tools/bench_kv_fork.py
// times both through lcc_debug_set_kv_copy_nt and writes profiles/kv_fork/copy.jsonl; DESIGN.md "KV fork").  Same bytes either way.
#ifndef LCC_KV_COPY_NT_DEFAULT
#define LCC_KV_COPY_NT_DEFAULT 0
#endif
static int g_kv_copy_nt = LCC_KV_COPY_NT_DEFAULT;
int set_kv_copy_nt(int on) { const int old = g_kv_copy_nt; g_kv_copy_nt = on ? 1 : 0; return old; }

int kv_copy(bf16_t* dst, const bf16_t* src, KvLayout lay, int n, int cu_count, hipStream_t st) {
  if (!dst || !src) return LCC_ERR_ARG;
  if (((uintptr_t)dst | (uintptr_t)src) & 15) return LCC_ERR_ALIGN;
  if (int r = kv_copy_check(lay, n)) return r;
  if (n == 0) return 0;
  const int planes = lay.n_layers * 2 * lay.n_kv_heads;
  const int n_blk = (n + 31) >> 5;
  // about 8 workgroups (32 waves) per CU over the launch, never less than one iteration's worth of blocks per workgroup
  int G = std::max(1, std::min(8 * std::max(cu_count, 1) / planes, (n_blk + CP_NB - 1) / CP_NB));
  const int per = ((n_blk + G - 1) / G + CP_NB - 1) / CP_NB * CP_NB;
  G = (n_blk + per - 1) / per;
  if (g_kv_copy_nt) kv_copy_kernel<true><<<dim3(G, planes), dim3(CP_THREADS), 0, st>>>(dst, src, lay, n, n_blk, per);
  else kv_copy_kernel<false><<<dim3(G, planes), dim3(CP_THREADS), 0, st>>>(dst, src, lay, n, n_blk, per);
  return 0;
}

}  // namespace lcc

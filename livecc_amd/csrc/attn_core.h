// Device building blocks of the per-wave attention kernels (swapped QK^T formulation, see attention.hip): accumulator,
// K / V fragment loads, one 32-key tile of online softmax, and the two-tile register ring.  Shared by attention.hip and the
// fused attention + o_proj decode launch of decode_v2.hip.
#pragma once
#include "common.h"
#include "kernels.h"

namespace lcc {

template <int D, int NQ>
struct AttnAcc {
  f32x4 o[D / 16][NQ];
  float m[NQ], l[NQ];
  LCC_DEVICE void init() {
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
      m[n] = -INFINITY;
      l[n] = 0.f;
#pragma unroll
      for (int d = 0; d < D / 16; ++d) o[d][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  }
};

template <int D>
struct KFrag {
  static constexpr int KS = (D + 31) / 32;
  u32x4 v[2][KS];
};

// K rows of the tile starting at key kb.  krow(key) returns the row pointer (already clamped by the caller's
// lambda to a readable row); lanes whose d-chunk lies beyond D load zeros (D = 80: chunks 10, 11).
template <int D, class RowPtr>
LCC_DEVICE void load_k(KFrag<D>& f, RowPtr krow, int kb, int li, int g) {
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int key = kb + (li >> 2) * 8 + kt * 4 + (li & 3);
    const bf16_t* p = krow(key);
#pragma unroll
    for (int ks = 0; ks < KFrag<D>::KS; ++ks) {
      const int d0 = ks * 32 + g * 8;
      f.v[kt][ks] = (d0 < D) ? ld16(p + d0) : (u32x4){0u, 0u, 0u, 0u};
    }
  }
}

template <int D>
LCC_DEVICE void load_v(u32x4 (&vf)[D / 16], const bf16_t* vt_block, int li, int g) {
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) vf[dt] = ld16(vt_block + (dt * 16 + li) * 32 + g * 8);
}

// one 32-key tile: scores, masking, online softmax, PV accumulation
// key_limit[n] : keys with index >= key_limit[n] are masked for query tile n's column of this lane
template <int D, int NQ>
LCC_DEVICE void attn_tile(AttnAcc<D, NQ>& acc, const KFrag<D>& kf, const u32x4 (&vf)[D / 16],
                          const u32x4 (&qf)[NQ][(D + 31) / 32], int kb, int g, const int (&key_limit)[NQ],
                          float scale_log2e, const int (&min_limit)[NQ]) {
  constexpr int KS = (D + 31) / 32;
  f32x4 s[2][NQ];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
      f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) a = mfma16(as_bf16x8(kf.v[kt][ks]), as_bf16x8(qf[n][ks]), a);
      s[kt][n] = a;
    }
  bf16x8 pf[NQ];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    // Row maximum over the RAW scores (scale > 0), then p = exp2(fma(s, scale, -m)): one FMA per score instead of a multiply
    // and a subtract.  Tiles that lie entirely below this wave's smallest key limit (all but the diagonal / last tile of a
    // long key range) skip the per-score compare + select.  (wave-uniform branch; the VALU work per score is what bounds
    // these kernels: 7 head-waves x 32 MFMAs per 32-key tile leave the SIMDs VALU-limited.)
    const bool masked = kb + 32 > __builtin_amdgcn_readfirstlane(min_limit[n]);
    float mx = -INFINITY;
    if (masked) {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kb + g * 8 + kt * 4 + r;
          const float v = (key < key_limit[n]) ? s[kt][n][r] : -INFINITY;
          s[kt][n][r] = v;
          mx = fmaxf(mx, v);
        }
    } else {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kt][n][r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(acc.m[n], mx * scale_log2e);
    const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
    const float alpha = exp2f(acc.m[n] - m_use);  // acc.m = -inf -> 0
    acc.m[n] = m_new;
    float p[8], psum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float e = exp2f(fmaf(s[kt][n][r], scale_log2e, -m_use));   // masked scores are -inf -> 0
        p[kt * 4 + r] = e;
        psum += e;
      }
    acc.l[n] = acc.l[n] * alpha + psum;
    // lazy rescale: once the running maximum has settled (almost every tile of a long key range) alpha is exactly 1.0 for
    // every lane and the D/16 accumulator multiplies -- the bulk of the per-tile VALU work -- are skipped.  x * 1.0f is exact,
    // so the result is bit-identical to always rescaling.  (wave-uniform branch)
    if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) acc.o[dt][n] *= alpha;
    }
    u32x4 pk = (u32x4){pack2(p[0], p[1]), pack2(p[2], p[3]), pack2(p[4], p[5]), pack2(p[6], p[7])};
    pf[n] = as_bf16x8(pk);
  }
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
    for (int n = 0; n < NQ; ++n) acc.o[dt][n] = mfma16(as_bf16x8(vf[dt]), pf[n], acc.o[dt][n]);
}

// key-tile loop [t0, t1) with a two-tile register ring: while tile t is multiplied the loads of tile t+1 are already in
// flight and those of tile t+2 are issued right after tile t's operands are consumed.  All loads are unconditional
// (tile index clamped to t1-1, so a re-load of the last tile may be issued and ignored): straight-line code, counted waits.
// wave-wide minimum of the per-lane key limits (tiles entirely below it need no mask)
template <int NQ>
LCC_DEVICE void wave_min_limits(const int (&key_limit)[NQ], int (&min_limit)[NQ]) {
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    int v = key_limit[n];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    min_limit[n] = v;
  }
}

struct NoHook { LCC_DEVICE void operator()() const {} };
// `after_first_loads` runs once the first two tiles' loads have been issued (e.g. to build the q fragments while they fly)
template <int D, int NQ, class KRow, class VBlk, class Hook = NoHook>
LCC_DEVICE void attn_loop(AttnAcc<D, NQ>& acc, KRow krow, VBlk vblk, int t0, int t1, const u32x4 (&qf)[NQ][(D + 31) / 32],
                          int li, int g, const int (&key_limit)[NQ], float scale_log2e, Hook after_first_loads = Hook()) {
  if (t0 >= t1) { after_first_loads(); return; }
  int min_limit[NQ];
  wave_min_limits<NQ>(key_limit, min_limit);
  const int tl = t1 - 1;
  KFrag<D> ka, kb;
  u32x4 va[D / 16], vb[D / 16];
  load_k<D>(ka, krow, t0 * 32, li, g);
  load_v<D>(va, vblk(t0), li, g);
  load_k<D>(kb, krow, min(t0 + 1, tl) * 32, li, g);
  load_v<D>(vb, vblk(min(t0 + 1, tl)), li, g);
  after_first_loads();
  for (int t = t0; t < t1; t += 2) {
    attn_tile<D, NQ>(acc, ka, va, qf, t * 32, g, key_limit, scale_log2e, min_limit);
    load_k<D>(ka, krow, min(t + 2, tl) * 32, li, g);
    load_v<D>(va, vblk(min(t + 2, tl)), li, g);
    if (t + 1 < t1) {
      attn_tile<D, NQ>(acc, kb, vb, qf, (t + 1) * 32, g, key_limit, scale_log2e, min_limit);
      load_k<D>(kb, krow, min(t + 3, tl) * 32, li, g);
      load_v<D>(vb, vblk(min(t + 3, tl)), li, g);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// LLM decode attention, one wave = one (stream b, KV head hk, key split): the G query heads of the KV head are the query columns,
// key tiles [split*per, (split+1)*per).  Partial (o, m, l) records go to the workspace; WT = write-through (agent-scope) stores for a
// merge by another block of the SAME launch.  The caller's wave must be a whole wave (lane = threadIdx.x & 63).
// ------------------------------------------------------------------------------------------------
template <bool DIRECT, bool WT>
__attribute__((always_inline)) LCC_DEVICE void attn_decode_body(const bf16_t* __restrict__ q, const int32_t* __restrict__ slots, const int32_t* __restrict__ kv_len,
                                 bf16_t* const* __restrict__ kv_base, const KvLayout& lay, int layer, int n_q_heads, int nsplit,
                                 float* __restrict__ ws_o, float* __restrict__ ws_ml, float scale_log2e, const AttnDirect dir, int split,
                                 int hk, int b) {
  constexpr int D = 128, KS = 4, NQ = 1;
  const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
  const int G = n_q_heads / lay.n_kv_heads;
  const int slot_id = DIRECT ? 0 : slots[b];
  // the new token's K/V were appended at index kv_len[slot] by rope_kv_append.  DIRECT: the host's count (kernels.h: AttnDirect)
  const int n = DIRECT ? (b == 0 ? dir.n[0] : (b == 1 ? dir.n[1] : (b == 2 ? dir.n[2] : dir.n[3]))) : kv_len[slot_id] + 1;
  const int ntile = (n + 31) / 32;
  const int per = (ntile + nsplit - 1) / nsplit;
  const int t0 = split * per, t1 = min(ntile, t0 + per);

  u32x4 qf[NQ][KS];
  int key_limit[NQ] = {n};
  {
    const int hq = hk * G + min(li, G - 1);
    const bf16_t* qp = q + ((size_t)b * n_q_heads + hq) * D;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[0][ks] = ld16(qp + ks * 32 + g * 8);
  }
  const bf16_t* base = (DIRECT ? (b == 0 ? dir.base[0] : (b == 1 ? dir.base[1] : (b == 2 ? dir.base[2] : dir.base[3]))) : kv_base[slot_id]) +
                       (size_t)layer * lay.layer_stride();
  const bf16_t* kbase = base + (size_t)hk * lay.head_stride();
  const bf16_t* vbase = base + lay.kv_stride() + (size_t)hk * lay.head_stride();
  auto krow = [&](int key) { return kbase + (size_t)min(key, n - 1) * D; };

  AttnAcc<D, NQ> acc;
  acc.init();
  auto vblk = [&](int t) { return vbase + (size_t)t * (D * 32); };
  attn_loop<D, NQ>(acc, krow, vblk, t0, t1, qf, li, g, key_limit, scale_log2e);
  float l = acc.l[0];
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (li < G) {
    const size_t slot = (((size_t)b * lay.n_kv_heads + hk) * nsplit + split) * 16 + li;
    float* op = ws_o + slot * D;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
      if (WT) store_sc1_f32x4(op + dt * 16 + g * 4, acc.o[dt][0]);
      else *reinterpret_cast<f32x4*>(op + dt * 16 + g * 4) = acc.o[dt][0];
    }
    if (g == 0) {
      if (WT) {
        st8_agent(ws_ml + slot * 2, (u32x2){__float_as_uint(acc.m[0]), __float_as_uint(l)});
      } else {
        ws_ml[slot * 2 + 0] = acc.m[0];
        ws_ml[slot * 2 + 1] = l;
      }
    }
  }
}

// ---- merge of the key splits (attn_decode_combine_kernel and the in-launch merge of the fused attention + o_proj kernel share the
//      arithmetic and its order: 8 groups, group q folds splits q, q+8, ... in turn, then the 8 group partials are folded in order) ----
LCC_DEVICE void split_merge_step(float& M, float& den, f32x4& num, float m, float l, f32x4 o) {
  const float Mn = fmaxf(M, m);
  const float a = (M == -INFINITY) ? 0.f : exp2f(M - Mn);
  const float w = (m == -INFINITY) ? 0.f : exp2f(m - Mn);
  num = num * a + o * w;
  den = den * a + w * l;
  M = Mn;
}
template <int NG>
LCC_DEVICE u32x2 split_merge_final(const float (&gm)[NG], const float (&gd)[NG], const f32x4 (&gn)[NG]) {
  float MM = -INFINITY;
#pragma unroll
  for (int q = 0; q < NG; ++q) MM = fmaxf(MM, gm[q]);
  float dd = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f, n3 = 0.f;
#pragma unroll
  for (int q = 0; q < NG; ++q) {
    const float m = gm[q];
    const float w = (m == -INFINITY) ? 0.f : exp2f(m - MM);
    dd += w * gd[q];
    n0 += w * gn[q][0]; n1 += w * gn[q][1]; n2 += w * gn[q][2]; n3 += w * gn[q][3];
  }
  const float inv = 1.f / dd;
  return (u32x2){pack2(n0 * inv, n1 * inv), pack2(n2 * inv, n3 * inv)};
}

}  // namespace lcc

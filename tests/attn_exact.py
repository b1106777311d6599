"""Structured attention inputs whose expected output is DERIVED, and the comparators that go with them (a plain helper module; the
kernel tests are tests/test_gpu_attn_exact.py, the proof that these comparators reject a subtly wrong kernel is
tests/test_attn_exact_ref.py, which runs without a GPU).

Counting inputs -- every key is counted exactly once.  q = 0, so every score is 0, p = exp2(0) = 1.0 exactly, the running maximum is 0
from the first tile on, and the softmax denominator is an exact integer in fp32.  The V row of key j is one-hot in channel (j + rot) % D,
so every partial sum is an exact integer and the merge weights across key splits are exactly 1 (0 for an empty split).  Rows at and
beyond the valid length are poison: K arbitrary, V = 64.0 in every channel (finite: the kernels' contract is finite bytes, 0 * 64 = 0).
Expected output: bf16(c_d / n) with c_d = #{j < n : (j + rot) % D == d}.  The only inexact operation is the final normalisation (a divide,
or a reciprocal and a multiply, then one rounding to bf16): 1 bf16 ulp.  One missing / extra / duplicated key moves its channel by about
1 / c_d relative: with c_d <= 33 (n <= 4224 at D = 128) that is >= 3 % = 7.7 ulps of 2^-8.  `rot` (a per-slot channel rotation) makes the
arenas of different slots differ, so that a row served from another stream's arena cannot give the right answer.

Needle inputs -- one chosen key per query row, any length.  K random bf16, q = 4 K[j*] (exact in bf16): the needle's score is
4 |K[j*]|^2 / sqrt(D) ~ 45 nats against N(0, 4^2) for the rest.  The test computes the fp64 softmax on the CPU and asserts ON THE REFERENCE
that the needle's weight w has 1 - w <= 2^-12.  Expected: bf16(fp64 reference); tolerance per element
max(1 bf16 ulp of the reference, (1 - w) max|V| + 2^-20).  The forbidden twin: the first invalid key gets K := K[j*] and V := 64.0 -- a mask
that lets it in halves the output towards 64.

Head dim 80 (the vision tower) -- the same helpers with dim = 80 and the gain 8: a needle's score is 8 |K|^2 / sqrt(80) ~ 72 nats against
N(0, 8^2) for the rest (gain 4 leaves 1 - w of some rows far above 2^-12 at this dim: tests/test_attn_exact_ref.py shows it).
`vit_needle_inputs` builds whole ViT segments that way -- row i of a segment looks for key perm(i) of the SAME segment, the first / last
patch of a segment is the forbidden twin (same K, V = 64.0) of a needle of the previous / next segment -- and `vit_vt` the
blocked-transposed V^T buffer [head][32-key block][80][32] the ViT kernels read, with a chosen filler in the pad columns.
"""
import math

import torch

D = 128
D_VIT = 80
POISON_V = 64.0
NEEDLE_GAIN = 4.0
NEEDLE_GAIN_VIT = 8.0                   # head dim 80: 8 x a bf16 value is exact, and 4 does not reach the weight gap below
NEEDLE_MIN_WEIGHT_GAP = 2.0 ** -12      # 1 - w of every needle, asserted on the fp64 reference
NEEDLE_ATOL = 2.0 ** -20


# ---------------------------------------------------------------------------------------------------------------------------------
# number format
# ---------------------------------------------------------------------------------------------------------------------------------
def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """fp64 -> the nearest bf16 value, returned as fp64."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """Spacing of the bf16 grid at the (normal) bf16 value x: 2^(floor(log2 |x|) - 7); 0 at x = 0 (an expected zero is exact)."""
    x = x.to(torch.float64).abs()
    e = torch.floor(torch.log2(x.clamp_min(2.0 ** -126)))
    return torch.where(x > 0, torch.exp2(e - 7), torch.zeros_like(x))


def deviation(got: torch.Tensor, ref64: torch.Tensor, atol=0.0):
    """(ok, worst): every element of `got` within max(1 bf16 ulp of bf16(ref64), atol) of bf16(ref64).  `worst` = the largest
    |got - bf16(ref)| / tolerance (0 where both are exactly equal), for the record."""
    got = got.detach().to("cpu", torch.float64)
    exp = bf16_round(ref64.detach().to("cpu", torch.float64))
    assert got.shape == exp.shape, (tuple(got.shape), tuple(exp.shape))
    if not bool(torch.isfinite(got).all()):
        return False, float("inf")
    tol = torch.maximum(bf16_ulp(exp), torch.as_tensor(atol, dtype=torch.float64).expand_as(exp))
    d = (got - exp).abs()
    rel = torch.where(d == 0, torch.zeros_like(d), d / tol.clamp_min(2.0 ** -140))
    return bool((d <= tol).all()), float(rel.max()) if rel.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# storage: [layer][K|V][Hkv][Lmax][128] arenas, V blocked-transposed [Lmax/32][128][32]
# ---------------------------------------------------------------------------------------------------------------------------------
def v_blocked(v: torch.Tensor) -> torch.Tensor:
    """Logical V rows [..., L, Dh] (L a multiple of 32) -> the blocked-transposed storage order [..., L/32, Dh, 32], flattened back to
    [..., L * Dh]: element (key j, channel d) lands at (j // 32) * Dh * 32 + d * 32 + j % 32."""
    *lead, L, dh = v.shape
    assert L % 32 == 0
    return v.reshape(*lead, L // 32, 32, dh).transpose(-1, -2).reshape(*lead, L * dh)


def write_arena(kv, slot: int, layer: int, k: torch.Tensor, v: torch.Tensor) -> None:
    """k, v: logical [Hkv, Lmax, 128] bf16 -> the slot's K rows and its blocked-transposed V rows of `layer` (the other layers are left)."""
    hkv, lmax = kv.n_kv_heads, kv.lmax
    assert k.shape == (hkv, lmax, D) and v.shape == (hkv, lmax, D)
    per = hkv * lmax * D
    o = layer * 2 * per
    kv.buf[slot, o:o + per].copy_(k.reshape(-1).to(kv.buf.dtype))
    kv.buf[slot, o + per:o + 2 * per].copy_(v_blocked(v).reshape(-1).to(kv.buf.dtype))


# ---------------------------------------------------------------------------------------------------------------------------------
# counting inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def counting_v(n_valid: int, n_rows: int, rot: int = 0, dim: int = D) -> torch.Tensor:
    """[n_rows, dim] bf16: row j < n_valid one-hot in channel (j + rot) % dim, rows >= n_valid poison (64.0 everywhere)."""
    v = torch.full((n_rows, dim), POISON_V, dtype=torch.float32)
    j = torch.arange(n_valid)
    v[:n_valid] = 0.0
    v[j, (j + rot) % dim] = 1.0
    return v.to(torch.bfloat16)


def counting_arena(n_valid: int, lmax: int, n_kv_heads: int, rot: int = 0, seed: int = 0):
    """(K, V) logical [Hkv, Lmax, 128] bf16 of one slot: K arbitrary finite bytes everywhere (q = 0 makes every score 0), V counting rows
    below n_valid and poison above."""
    g = torch.Generator().manual_seed(1000 + seed)
    k = (torch.randn(n_kv_heads, lmax, D, generator=g) * 2.0).to(torch.bfloat16)
    v = counting_v(n_valid, lmax, rot).unsqueeze(0).expand(n_kv_heads, lmax, D).contiguous()
    return k, v


def counting_expected(n: int, rot: int = 0, dim: int = D, lo: int = 0) -> torch.Tensor:
    """fp64 [dim]: c_d / (n - lo) over the keys lo <= j < n (c_d = how many of them are one-hot in channel d)."""
    j = torch.arange(lo, n)
    c = torch.bincount((j + rot) % dim, minlength=dim).to(torch.float64)
    return c / float(n - lo)


def check_counting(got: torch.Tensor, n: int, rot: int = 0, dim: int = D):
    """got [..., dim] (every leading index is a query head / row that attends to keys 0 .. n-1) -> (ok, worst deviation in ulps)."""
    exp = counting_expected(n, rot, dim)
    return deviation(got, exp.expand(got.shape))


# ---------------------------------------------------------------------------------------------------------------------------------
# needle inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def needle_gain(dim: int = D) -> float:
    """The query gain of the needle inputs at head dim `dim`."""
    return {D: NEEDLE_GAIN, D_VIT: NEEDLE_GAIN_VIT}[dim]


def needle_kv(n_valid: int, lmax: int, n_kv_heads: int, seed: int, dim: int = D):
    """(K, V) logical [Hkv, Lmax, dim] bf16: random below n_valid; above, K random and V poison."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(n_kv_heads, lmax, dim, generator=g).to(torch.bfloat16)
    v = torch.randn(n_kv_heads, lmax, dim, generator=g).to(torch.bfloat16)
    v[:, n_valid:] = POISON_V
    return k, v


def needle_q(k: torch.Tensor, needles, group: int, dim: int = D, gain=None) -> torch.Tensor:
    """q [len(needles), dim] bf16: query head h looks for key needles[h] of its KV head h // group (gain x a bf16 value is exact: the
    gain is a power of two, needle_gain(dim) unless given)."""
    assert k.shape[-1] == dim, (tuple(k.shape), dim)
    gain = needle_gain(dim) if gain is None else gain
    return torch.stack([k[h // group, j].float() * gain for h, j in enumerate(needles)]).to(torch.bfloat16)


def plant_twin(k: torch.Tensor, v: torch.Tensor, hk: int, index: int, needle: int) -> None:
    """The forbidden twin: key `index` (invalid for the row under test) of KV head hk := the needle's K, with V = 64.0."""
    k[hk, index] = k[hk, needle]
    v[hk, index] = POISON_V


def softmax_rows(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, keys, dim: int = D):
    """The plain reference in fp64: one query head q [dim] over the key list `keys` (indices into k / v [L, dim]; a list, so that a test
    can drop, repeat or add one).  Returns (output [dim], weights [len(keys)])."""
    assert q.shape[-1] == dim and k.shape[-1] == dim and v.shape[-1] == dim, (tuple(q.shape), tuple(k.shape), tuple(v.shape), dim)
    idx = torch.as_tensor(list(keys), dtype=torch.long)
    s = (k[idx].to(torch.float64) @ q.to(torch.float64)) / math.sqrt(dim)
    p = torch.exp(s - s.max())
    w = p / p.sum()
    return w @ v[idx].to(torch.float64), w


def needle_reference(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, kv_head, n_keys, needles, dim: int = D):
    """fp64 reference of needle rows: row r = one query head q[r] that attends to keys 0 .. n_keys[r]-1 of KV head kv_head[r] and looks
    for key needles[r].  Returns (ref [R, dim], 1 - w [R], max|V| over the row's valid keys [R]) and asserts, on the reference alone, that
    every needle dominates."""
    refs, gaps, vmax = [], [], []
    for r in range(q.shape[0]):
        hk, n, j = int(kv_head[r]), int(n_keys[r]), int(needles[r])
        assert 0 <= j < n
        o, w = softmax_rows(q[r], k[hk], v[hk], range(n), dim)
        gap = float(w.sum() - w[j]) if n > 1 else 0.0
        assert gap <= NEEDLE_MIN_WEIGHT_GAP, f"row {r}: needle {j} of {n} keys has 1 - w = {gap:.3g} > 2^-12: choose another seed"
        refs.append(o); gaps.append(gap); vmax.append(float(v[hk, :n].to(torch.float64).abs().max()))
    return torch.stack(refs), torch.tensor(gaps, dtype=torch.float64), torch.tensor(vmax, dtype=torch.float64)


def needle_atol(gaps: torch.Tensor, vmax: torch.Tensor) -> torch.Tensor:
    """(1 - w) max|V| + 2^-20 per row, as a column to broadcast over the channels."""
    return (gaps * vmax + NEEDLE_ATOL).unsqueeze(-1)


def check_needle(got: torch.Tensor, ref64: torch.Tensor, gaps: torch.Tensor, vmax: torch.Tensor, dim=None):
    """got [..., dim] against the fp64 reference rows (gaps, vmax: one per row, [...]) -> (ok, worst deviation in units of the tolerance).
    dim, when given, is checked against both (the comparison itself is per element: any width)."""
    assert dim is None or (got.shape[-1] == dim and ref64.shape[-1] == dim), (tuple(got.shape), tuple(ref64.shape), dim)
    return deviation(got, ref64, needle_atol(gaps, vmax).expand_as(ref64))


# ---------------------------------------------------------------------------------------------------------------------------------
# ViT segments: head dim 80, non-causal inside a segment, V^T staged per segment in blocks of 32 keys
# ---------------------------------------------------------------------------------------------------------------------------------
# The grids of tests/test_gpu_vit_exact.py: segments of 24 (under one block, 8 pads), 36 (a block + 4: every later segment starts at 4 mod 8),
# 64, 64 (exact blocks), 130 (one 128-row group + 2 rows) and 300 keys (two 256-row / three 128-row groups; P = 618 is no multiple of 8).
VIT_GRIDS = [(1, 4, 6), (1, 6, 6), (2, 8, 8), (1, 10, 13), (1, 10, 30)]


def vit_even_grids(grids):
    """every h, w rounded up to the 2 x 2 merge unit: the grids a real clip can have"""
    return [(t, h + h % 2, w + w % 2) for t, h, w in grids]


def vit_rope_tables_for(grids, cfg):
    """fp32 cos / sin [P, 40] for the kernel tests: vision_rope_tables slice by slice.  A slice with an odd h or w (10 x 13: a segment
    LENGTH the kernels must handle, not a frame the 2 x 2 merge admits -- HF's position ids and vision_rope_tables both refuse it) takes
    the first h * w rows of the table of the next even grid: real angles, one table row per patch, which is all the rope kernel sees."""
    from livecc_amd.engine import vision_rope_tables
    cs, sn = [], []
    for (t, h, w), even in zip(grids, vit_even_grids(grids)):
        c, s = vision_rope_tables([(1,) + tuple(even[1:])], cfg)
        cs += [c[:h * w]] * t
        sn += [s[:h * w]] * t
    return torch.cat(cs).contiguous(), torch.cat(sn).contiguous()


def vit_seg_lens(grids):
    """(t, h, w) grids -> the segment lengths: one segment of h * w patches per temporal slice."""
    return [h * w for t, h, w in grids for _ in range(t)]


def vit_vt_index(seg_lens, heads: int, dim: int = D_VIT):
    """(index [P, heads, dim] long, blocks): element (patch p = key kl of segment sg, head, channel d) of V lives at
    ((head * blocks + seg_blk[sg] + kl // 32) * dim + d) * 32 + kl % 32 of the V^T buffer; blocks = sum of ceil(len / 32)."""
    blk, kl, b = [], [], 0
    for n in seg_lens:
        j = torch.arange(n)
        blk.append(b + j // 32); kl.append(j % 32)
        b += (n + 31) // 32
    blk, kl = torch.cat(blk), torch.cat(kl)
    h, d = torch.arange(heads), torch.arange(dim)
    idx = ((h[None, :, None] * b + blk[:, None, None]) * dim + d[None, None, :]) * 32 + kl[:, None, None]
    return idx, b


def vit_vt(v: torch.Tensor, seg_lens, fill, guard_blocks: int = 0) -> torch.Tensor:
    """v [P, heads, dim] (any dtype) -> the flat V^T buffer of (heads * blocks + guard_blocks) * dim * 32 elements: V by plain indexing
    at vit_vt_index, `fill` everywhere else (the pad columns kl >= len % 32 of a segment's last block, and the guard)."""
    P, heads, dim = v.shape
    assert P == sum(seg_lens)
    idx, blocks = vit_vt_index(seg_lens, heads, dim)
    buf = torch.full(((heads * blocks + guard_blocks) * dim * 32,), fill, dtype=v.dtype)
    buf[idx.reshape(-1)] = v.reshape(-1)
    return buf


def vit_needle_inputs(seg_lens, heads: int, seed: int, gain: float = NEEDLE_GAIN_VIT, dim: int = D_VIT):
    """Needle inputs over whole ViT segments.  K, V random bf16 [P, heads, dim]; query row i of a segment is gain * K[perm(i)] with perm a
    fixed permutation of that segment's keys (every key is somebody's needle).  Twins: the FIRST patch of every segment after the first
    takes the K of a needle of the previous segment (its middle key) and V = 64.0; the LAST patch of every segment but the last does the
    same towards the next one.  A twin is an ordinary valid key of its own segment (and the needle of one of its rows); the reference
    admits it there and nowhere else.
    Returns dict(q, k, v [P, heads, dim] bf16; needle [P] = global index of each row's needle; twins = [(twin index, source index)];
    ref [P, heads, dim] fp64; gaps, vmax [P, heads] fp64) and asserts, on the fp64 reference alone, 1 - w <= 2^-12 for every row."""
    g = torch.Generator().manual_seed(seed)
    P = sum(seg_lens)
    k = torch.randn(P, heads, dim, generator=g).to(torch.bfloat16)
    v = torch.randn(P, heads, dim, generator=g).to(torch.bfloat16)
    starts = [sum(seg_lens[:i]) for i in range(len(seg_lens))]
    mid = [s0 + n // 2 for s0, n in zip(starts, seg_lens)]          # never a first / last patch (n >= 3): no twin is copied from a twin
    assert all(n >= 3 for n in seg_lens)
    twins = []
    for i, (s0, n) in enumerate(zip(starts, seg_lens)):
        if i > 0:
            twins.append((s0, mid[i - 1]))
        if i + 1 < len(seg_lens):
            twins.append((s0 + n - 1, mid[i + 1]))
    for t, src in twins:
        k[t] = k[src]
        v[t] = POISON_V
    needle = torch.cat([s0 + torch.randperm(n, generator=g) for s0, n in zip(starts, seg_lens)])
    q = (k[needle].float() * gain).to(torch.bfloat16)
    assert torch.equal(q.float(), k[needle].float() * gain), "gain x a bf16 value is exact"
    ref = torch.empty(P, heads, dim, dtype=torch.float64)
    gaps = torch.empty(P, heads, dtype=torch.float64)
    vmax = torch.empty(P, heads, dtype=torch.float64)
    for s0, n in zip(starts, seg_lens):
        sl = slice(s0, s0 + n)
        q64, k64, v64 = q[sl].to(torch.float64), k[sl].to(torch.float64), v[sl].to(torch.float64)
        s = torch.einsum("qhd,khd->hqk", q64, k64) / math.sqrt(dim)
        p = torch.exp(s - s.amax(-1, keepdim=True))
        w = p / p.sum(-1, keepdim=True)
        ref[sl] = torch.einsum("hqk,khd->qhd", w, v64)
        others = w.clone()                                           # 1 - w as the sum of the OTHER weights: no cancellation
        others.scatter_(2, (needle[sl] - s0)[None, :, None].expand(heads, n, 1), 0.0)
        gaps[sl] = others.sum(-1).t()
        vmax[sl] = v64.abs().amax(dim=(0, 2))[None, :].expand(n, heads)
    worst = float(gaps.max())
    assert worst <= NEEDLE_MIN_WEIGHT_GAP, f"a needle has 1 - w = {worst:.3g} > 2^-12 at gain {gain}"
    return dict(q=q, k=k, v=v, needle=needle, twins=twins, starts=starts, ref=ref, gaps=gaps, vmax=vmax)

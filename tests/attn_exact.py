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
"""
import math

import torch

D = 128
POISON_V = 64.0
NEEDLE_GAIN = 4.0
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
def needle_kv(n_valid: int, lmax: int, n_kv_heads: int, seed: int):
    """(K, V) logical [Hkv, Lmax, 128] bf16: random below n_valid; above, K random and V poison."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(n_kv_heads, lmax, D, generator=g).to(torch.bfloat16)
    v = torch.randn(n_kv_heads, lmax, D, generator=g).to(torch.bfloat16)
    v[:, n_valid:] = POISON_V
    return k, v


def needle_q(k: torch.Tensor, needles, group: int) -> torch.Tensor:
    """q [len(needles), 128] bf16: query head h looks for key needles[h] of its KV head h // group (4 x a bf16 value is exact)."""
    return torch.stack([k[h // group, j].float() * NEEDLE_GAIN for h, j in enumerate(needles)]).to(torch.bfloat16)


def plant_twin(k: torch.Tensor, v: torch.Tensor, hk: int, index: int, needle: int) -> None:
    """The forbidden twin: key `index` (invalid for the row under test) of KV head hk := the needle's K, with V = 64.0."""
    k[hk, index] = k[hk, needle]
    v[hk, index] = POISON_V


def softmax_rows(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, keys):
    """The plain reference in fp64: one query head q [128] over the key list `keys` (indices into k / v [L, 128]; a list, so that a test
    can drop, repeat or add one).  Returns (output [128], weights [len(keys)])."""
    idx = torch.as_tensor(list(keys), dtype=torch.long)
    s = (k[idx].to(torch.float64) @ q.to(torch.float64)) / math.sqrt(q.shape[-1])
    p = torch.exp(s - s.max())
    w = p / p.sum()
    return w @ v[idx].to(torch.float64), w


def needle_reference(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, kv_head, n_keys, needles):
    """fp64 reference of needle rows: row r = one query head q[r] that attends to keys 0 .. n_keys[r]-1 of KV head kv_head[r] and looks
    for key needles[r].  Returns (ref [R, 128], 1 - w [R], max|V| over the row's valid keys [R]) and asserts, on the reference alone, that
    every needle dominates."""
    refs, gaps, vmax = [], [], []
    for r in range(q.shape[0]):
        hk, n, j = int(kv_head[r]), int(n_keys[r]), int(needles[r])
        assert 0 <= j < n
        o, w = softmax_rows(q[r], k[hk], v[hk], range(n))
        gap = float(w.sum() - w[j]) if n > 1 else 0.0
        assert gap <= NEEDLE_MIN_WEIGHT_GAP, f"row {r}: needle {j} of {n} keys has 1 - w = {gap:.3g} > 2^-12: choose another seed"
        refs.append(o); gaps.append(gap); vmax.append(float(v[hk, :n].to(torch.float64).abs().max()))
    return torch.stack(refs), torch.tensor(gaps, dtype=torch.float64), torch.tensor(vmax, dtype=torch.float64)


def needle_atol(gaps: torch.Tensor, vmax: torch.Tensor) -> torch.Tensor:
    """(1 - w) max|V| + 2^-20 per row, as a column to broadcast over the channels."""
    return (gaps * vmax + NEEDLE_ATOL).unsqueeze(-1)


def check_needle(got: torch.Tensor, ref64: torch.Tensor, gaps: torch.Tensor, vmax: torch.Tensor):
    """got [R, 128] against the fp64 reference rows -> (ok, worst deviation in units of the tolerance)."""
    return deviation(got, ref64, needle_atol(gaps, vmax).expand_as(ref64))

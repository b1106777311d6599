"""Operands for the decode GEMVs (csrc/decode_v2.hip) whose correct output is UNIQUE, and the float64 references that go with them (a plain
helper module, no GPU; the kernel tests are tests/test_gpu_dgemv_exact.py, the proof that the references tell a subtly wrong kernel from a
right one is tests/test_dgemv_exact_ref.py).

Exact sums.  Activations and weights are small integers or dyadic rationals: all values multiples of 2^-s, sum_k |x_k w_k| < 2^(24-s).  Every
product and every partial sum, in any order, is then an fp32 number, so the accumulator holds the same bits whatever the wave split, the
unroll, the pipeline depth or the MFMA order (`assert_sums_exact`).  Every later step of an epilogue is ONE correctly rounded fp32 or bf16
operation on exact operands, which float64 followed by a rounding to fp32 (`f32`) or through fp32 to bf16 (`rb`) reproduces bit for bit.

  * fp8: e4m3 bytes of small integers with fp32 row scales of two or three significant bits that are not all powers of two; acc * scale is
    asserted exact in fp32, so a contraction of the scale and the bias add into one fma cannot change the result either.
  * MXFP4: codes drawn directly from the e2m1 set, block exponents spanning four octaves with neighbouring blocks of a row never equal.
  * RMSNorm prologue: row m has sum of squares c_m * K with c_m + eps a power of 4, so r_m = rsqrt(c_m + eps) is a power of two, h * r is an
    exact bf16 value, and bf16(w * bf16(h * r)) rounds (norm weights like 1 + 2^-7 against odd h * r).  Rows of one case have different r.
    With r a power of two, bf16(w * h * r) -- one rounding -- is the same number: that mutant cannot be told apart by exact operands and
    `norm_ref(mutant="single_rounded")` exists to show it; `inexact_r_rows` is the one input family with another r (3^-1/2), kept to
    values of h * r whose bf16 rounding is asserted safe against an rsqrt that is a few fp32 ulps off.
  * residual epilogue: h stays small enough that the 16-value sums of squares are exact as well (`assert_stats_exact`).
  * SwiGLU: gate rows are zero, aligned with the sign pattern of the activation rows (gate >= 32: 1 + exp(-g) == 1 in fp32, and the Newton
    step of the kernel's reciprocal returns exactly 1 for any first guess within an ulp of 1), opposed to it (gate <= -104: silu underflows
    to zero -- 1 + exp(-g) is +inf there, which a Newton step on the reciprocal turns into NaN unless it is guarded), or sparse +-1 rows
    (small gates through the transcendental: 1 bf16 ulp; draws with a silu near a rounding tie or in the denormal range are replaced).

The cases of the GPU file are listed here (RESID_CASES, NORM_CASES, SWIGLU_CASES, ROPE_CASES, CHAIN_CASES) so that the CPU file can prove
the exactness conditions and the power of the mutant references on exactly those inputs.  The GEMV_* lists are the cases of
tests/test_gpu_gemv_exact.py, which runs the weight-streaming GEMVs of csrc/gemm.hip on the same operands."""
import functools
import math

import torch

from tests.attn_exact import bf16_round, bf16_ulp, deviation  # noqa: F401  (re-exported for the two test files)

FORMATS = ("bf16", "fp8", "mxfp4")
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
FP8_SCALES_INT = (0.75, 1.25, 1.75, 0.25, 1.25, 1.75)    # with bytes 4 k: effective weights k * (3, 5, 7, 1, 5, 7), odd multiples
FP8_SCALES_FRAC = (0.75, 1.5, 0.5, 3.0, 1.0, 0.375)      # two significant bits: acc * scale stays exact for 22-bit accumulators
# 129, 133, 173, 177 / 128: their products with h * r = 1.5 (and most with 1.75, 0.75) round UP, so a truncation shows
NORM_W = (1.0078125, 1.0390625, 1.3515625, 1.3828125, 1.0, 1.5, 2.0, 3.0)
GATE_ROW_MODES = (1, 2, 2, 3, 4, 2, 1, 3)
NORM_W_PLAIN = (1.0, 1.5, 2.0, 0.75, 3.0, 0.5)           # K = 8192: keeps the activations multiples of 2^-3
QUADS = {3: ((3, 1, 1, 1), (2, 2, 2, 0)), 15: ((7, 3, 1, 1), (5, 5, 3, 1))}      # four entries with sum of squares 4 c
ROW_C = (3, 15, 3, 15)
NORM_EPS = 1.0                                            # c + eps = 4, 16: r = 1/2, 1/4
SAT_GATE = 32.0
# gates in here have a silu that is a bf16 (or intermediate fp32) denormal: flush-to-zero modes legitimately differ, no case may hold one
GATE_GRAY = (-104.0, -86.0)
POISON_BF16 = -1234.0
POISON_F32 = 12345.0
BF = torch.bfloat16
PAD = 2048


class Canary:
    """a [rows, cols] view inside a poisoned buffer: `extra_rows` rows below it, `extra_cols` columns to its right, PAD elements around"""

    def __init__(self, dev, rows, cols, dtype, init=None, extra_rows=3, extra_cols=0):
        self.poison = POISON_BF16 if dtype == BF else POISON_F32
        ld = cols + extra_cols
        self.ld = ld
        self.buf = torch.full((PAD + (rows + extra_rows) * ld + PAD,), self.poison, dtype=dtype, device=dev)
        self.view = self.buf[PAD:PAD + (rows + extra_rows) * ld].view(rows + extra_rows, ld)[:rows, :cols]
        if init is not None:
            self.view.copy_(init.to(dtype))
        self.before = self.buf.clone()

    def check(self, what):
        b = self.buf.clone()
        self.view.fill_(self.poison)
        ok = torch.equal(self.buf, torch.full_like(self.buf, self.poison))
        self.buf.copy_(b)
        assert ok, f"{what}: a store outside the result"

    def untouched(self):
        return torch.equal(self.buf, self.before)


def _dev(t64, dev, dtype=BF):
    out = t64.to(dtype)
    assert torch.equal(out.double(), t64)
    return out.contiguous().to(dev)


def gen(*key) -> torch.Generator:
    s = 0
    for k in key:
        s = (s * 1000003 + (FORMATS.index(k) + 1 if isinstance(k, str) else int(k)) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def ints(g, shape, a) -> torch.Tensor:
    """uniform integers in -a..a, float64"""
    return torch.randint(-a, a + 1, tuple(shape), generator=g).double()


def nonzero_ints(g, shape, a) -> torch.Tensor:
    """uniform over -a..-1, 1..a: no weight column is multiplied by zero"""
    mag = torch.randint(1, a + 1, tuple(shape), generator=g).double()
    return torch.where(torch.rand(tuple(shape), generator=g) < 0.5, -mag, mag)


def f32(x64: torch.Tensor) -> torch.Tensor:
    """one correctly rounded fp32 operation: the exact float64 result, rounded to fp32"""
    return x64.to(torch.float32).to(torch.float64)


def rb(x64: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16, as float64 (the argument is an fp32 value, or exact, so this is one rounding)"""
    return bf16_round(x64)


def trunc_bf16(x64: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 by dropping the low 16 bits (the mutant of a rounding)"""
    return (x64.to(torch.float32).view(torch.int32) & -65536).view(torch.float32).to(torch.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# exactness conditions
# ---------------------------------------------------------------------------------------------------------------------------------
def lsb_exp(x64: torch.Tensor) -> int:
    """smallest s >= 0 such that every element is a multiple of 2^-s"""
    for s in range(0, 48):
        y = x64 * 2.0 ** s
        if bool((y == y.round()).all()):
            return s
    raise AssertionError("not dyadic")


def assert_sums_exact(x64: torch.Tensor, w64: torch.Tensor) -> float:
    """all values multiples of 2^-s and sum_k |x w| < 2^(24-s) for every (row, column): every partial sum in any order is an fp32 number.
    Returns the head room (bound / worst sum)."""
    s = lsb_exp(x64) + lsb_exp(w64)
    worst = float((x64.abs() @ w64.abs().t()).max())
    assert worst < 2.0 ** (24 - s), f"sum |x w| = {worst} >= 2^{24 - s} (values are multiples of 2^-{s})"
    return 2.0 ** (24 - s) / max(worst, 1.0)


def assert_scaled_exact(acc64: torch.Tensor, scale64: torch.Tensor) -> None:
    p = acc64 * scale64[None, :]
    assert torch.equal(f32(p), p), "acc * scale is not an fp32 number"


def assert_stats_exact(v64: torch.Tensor) -> None:
    """v: [M, N] values the residual epilogue writes.  Per 16-value tile: the values are multiples of 2^-s and sum v^2 < 2^(24-2s), so the
    squares and all their partial sums are fp32 numbers."""
    M, N = v64.shape
    t = v64.view(M, N // 16, 16)
    s = torch.full((M, N // 16), 99, dtype=torch.int64)
    for e in range(12, -1, -1):
        y = t * 2.0 ** e
        s = torch.where((y == y.round()).all(-1), torch.full_like(s, e), s)
    assert int(s.max()) < 99, "a written value is not a multiple of 2^-12"
    ss = (t * t).sum(-1) * torch.exp2(2.0 * s.double())
    assert bool((ss < 2.0 ** 24).all()), f"tile sum of squares needs {math.log2(float(ss.max())):.1f} bits"


# ---------------------------------------------------------------------------------------------------------------------------------
# weights: the pieces in LOGICAL row order (so that a row permutation can be applied before packing) and the float64 values
# ---------------------------------------------------------------------------------------------------------------------------------
def make_weight(fmt, N, K, g, aw=15, fp8_mul=4, scales=FP8_SCALES_INT, e_lo=0, row_mode=None, sgn=None, p3=1.0, w_density=1.0, int_valued=False) -> dict:
    """row_mode [N]: 0 random signs, 1 an all-zero row, 2 signs taken from sgn [K] (so that a dot product with activations of that sign
    pattern is a sum of non-negative terms), 4 the opposite signs, 3 a sparse row of +-1 (density p3: a small dot product).  Returns q64 (the values the MFMA multiplies: bf16 weights, e4m3 values, or the dequantised
    MXFP4 weights), scale64 [N] (ones unless fp8) and the bytes to pack."""
    row_mode = torch.zeros(N, dtype=torch.int64) if row_mode is None else row_mode

    def signed(mag):
        sign = torch.where(torch.rand(N, K, generator=g) < 0.5, -1.0, 1.0).double()
        if sgn is not None:
            sign = torch.where((row_mode == 2)[:, None], sgn.double()[None, :].expand(N, K), sign)
            sign = torch.where((row_mode == 4)[:, None], -sgn.double()[None, :].expand(N, K), sign)
        one = (torch.rand(N, K, generator=g) < p3).double()
        mag = torch.where((row_mode == 3)[:, None], one, mag)
        return torch.where((row_mode == 1)[:, None], torch.zeros_like(mag), mag * sign)

    if fmt == "mxfp4":
        idx = torch.randint(0, 8, (N, K), generator=g) * (torch.rand(N, K, generator=g) < w_density)
        kb = torch.arange(K // 32)[None, :]
        e = e_lo + (kb % 2 + 2 * torch.randint(0, 2, (N, K // 32), generator=g))      # parity follows the block: neighbours differ
        if int_valued:      # 0.5 and 1.5 only in blocks whose scale makes them integers (every code still occurs)
            low = (e == 0).repeat_interleave(32, dim=1)
            idx = torch.where(low & (idx == 1), torch.full_like(idx, 2), torch.where(low & (idx == 3), torch.full_like(idx, 4), idx))
        grid = torch.tensor(E2M1, dtype=torch.float64)
        val = signed(grid[idx])
        idx = torch.where((row_mode == 3)[:, None], torch.full_like(idx, 2), idx)      # |value| 1.0 where the sparse row is not zero
        codes = (idx * (val != 0) + 8 * (val < 0)).to(torch.uint8)
        sc = (e + 127).to(torch.uint8)
        return dict(fmt=fmt, N=N, K=K, codes=codes, sc=sc, q64=dequant_mxfp4(codes, sc), scale64=torch.ones(N, dtype=torch.float64))
    k = signed(torch.randint(0, aw + 1, (N, K), generator=g).double())
    if fmt == "bf16":
        rows = k.to(torch.bfloat16)
        assert torch.equal(rows.double(), k)
        return dict(fmt=fmt, N=N, K=K, rows=rows, q64=k, scale64=torch.ones(N, dtype=torch.float64))
    q = k * fp8_mul
    by = q.to(torch.float32).to(torch.float8_e4m3fn)
    assert torch.equal(by.to(torch.float64), q), "not an e4m3 value"
    scale = torch.tensor(scales, dtype=torch.float64)[torch.arange(N) % len(scales)]
    return dict(fmt=fmt, N=N, K=K, bytes=by.view(torch.uint8), q64=q, scale64=scale)


def dequant_mxfp4(codes, sc) -> torch.Tensor:
    from livecc_amd.weights import dequantize_mxfp4_rows
    return dequantize_mxfp4_rows(codes, sc).double()


def neighbour_scale(W: dict) -> dict:
    """the mutant weight: fp8 -- every row dequantised with the scale of the row before it; MXFP4 -- every block with the scale byte of the
    block before it in its row"""
    V = dict(W)
    if W["fmt"] == "fp8":
        V["scale64"] = W["scale64"].roll(1)
    elif W["fmt"] == "mxfp4":
        V["q64"] = dequant_mxfp4(W["codes"], W["sc"].roll(1, dims=1))
    else:
        raise ValueError("bf16 weights have no scale")
    return V


def pack(W: dict, dev, perm=None):
    """-> (packed device weight, the scale keyword of the ops.dgemv_* wrappers).  perm: stored row -> logical row."""
    from livecc_amd import ops
    from livecc_amd.weights import pack_scale_mxfp4, pack_weight_fp8, pack_weight_mxfp4
    p = (lambda t: t) if perm is None else (lambda t: t[perm].contiguous())
    if W["fmt"] == "bf16":
        return ops.pack_weight(p(W["rows"])).to(dev), {}
    if W["fmt"] == "fp8":
        return pack_weight_fp8(p(W["bytes"])).to(dev), {"wscale": p(W["scale64"]).float().contiguous().to(dev)}
    return pack_weight_mxfp4(p(W["codes"])).to(dev), {"w4scale": pack_scale_mxfp4(p(W["sc"])).to(dev)}


def amplitudes(fmt, K, fp8_mul=4, target=450.0):
    """(weight amplitude, activation amplitude, activation density) that keep the standard deviation of an accumulator near `target`:
    large enough that most accumulators need a bf16 rounding, small enough that the tile sums of squares stay exact"""
    def var(a):
        return a * (a + 1) / 3.0
    def xvar(a):                                  # activations are drawn from -a..a WITHOUT zero
        return (a + 1) * (2 * a + 1) / 6.0
    wfac = {"bf16": 1.0, "fp8": (fp8_mul / 4.0) ** 2 * 26.3, "mxfp4": 1.0}[fmt]
    aw = ax = 15
    wv = (lambda: 175.0) if fmt == "mxfp4" else (lambda: wfac * var(aw))
    while K * wv() * xvar(ax) > target ** 2 and (ax > 1 or (aw > 1 and fmt != "mxfp4")):
        if ax >= aw or fmt == "mxfp4":
            ax -= 1
        else:
            aw -= 1
    px = min(1.0, target ** 2 / (K * wv() * xvar(ax)))
    return aw, ax, px


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 references, rounding points written out; `mutant` selects one deliberate mistake
# ---------------------------------------------------------------------------------------------------------------------------------
def linear64(x64, W):
    """(fp32(acc * scale), acc): the dequantised Linear output before any epilogue"""
    acc = x64 @ W["q64"].t()
    return f32(acc * W["scale64"][None, :]), acc


def resid_ref(x64, W, h0, mutant=None):
    """h = bf16(h0 + bf16(lin)); statistics = the sums of squares of every 16 WRITTEN values"""
    lin, _ = linear64(x64, W)
    v = rb(f32(h0 + lin)) if mutant == "resid_before_rounding" else rb(f32(h0 + rb(lin)))
    M, N = v.shape
    return v, (v * v).view(M, N // 16, 16).sum(-1)


def norm_ref(h64, nw64, r, mutant=None):
    """x = bf16(w * bf16(h * r)), r [M] float64"""
    if mutant == "other_row_r":
        r = r.roll(1)
    hr = f32(h64 * r[:, None])
    if mutant == "single_rounded":
        return rb(f32(nw64[None, :] * hr))
    if mutant == "truncated":
        return trunc_bf16(f32(nw64[None, :] * rb(hr)))
    return rb(f32(nw64[None, :] * rb(hr)))


def bias_ref(xn64, W, bias64=None, mutant=None):
    """bf16(acc * scale + bias)"""
    lin, _ = linear64(xn64, W)
    if bias64 is None:
        return rb(lin)
    if mutant == "bias_after_rounding":
        return rb(f32(rb(lin) + bias64[None, :]))
    return rb(f32(lin + bias64[None, :]))


def swiglu_ref(xn64, W):
    """W: rows interleaved [16 gate | 16 up] (weights.interleave_gate_up).  -> (out, gate, saturated): out = bf16(silu_bf16(g) * u) with
    g, u the bf16-rounded gate / up outputs; saturated = g == 0 or g >= 32, where the kernel's fp32 silu is exactly g (or 0)."""
    lin, _ = linear64(xn64, W)
    M, N = lin.shape
    a = lin.view(M, N // 32, 2, 16)
    g, u = rb(a[:, :, 0]).reshape(M, N // 2), rb(a[:, :, 1]).reshape(M, N // 2)
    s = rb(g / (1.0 + torch.exp(-g)))
    return rb(f32(s * u)), g, (g == 0) | (g >= SAT_GATE)


def silu_tie_margin(g64) -> torch.Tensor:
    """distance of the float64 silu(g) from the nearest bf16 rounding tie, in bf16 ulps (0.5 = as far as can be)"""
    s = g64 / (1.0 + torch.exp(-g64))
    ulp = torch.exp2(torch.floor(torch.log2(s.abs().clamp_min(2.0 ** -120))) - 7)
    t = s.abs() / ulp
    return ((t - torch.floor(t)) - 0.5).abs()


def rope_ref(xn64, W, bias64, cos64, sin64, Hq, Hkv, mutant=None):
    """W in LOGICAL row order (q heads, k heads, v heads).  y = bf16(acc * scale + bias); q and k heads:
    bf16(bf16(y * cos) + bf16(rotate_half(y) * sin)), rotate_half = (-y2, y1) (HF's op order); v heads: y.
    -> q [M, Hq * 128], k [M, Hkv, 128], v [M, Hkv, 128]"""
    y = bias_ref(xn64, W, bias64)
    M = y.shape[0]
    y = y.view(M, Hq + 2 * Hkv, 128)
    rot = y[:, :Hq + Hkv]
    y1, y2 = rot[..., :64], rot[..., 64:]
    c, s = cos64[:, None, :], sin64[:, None, :]
    sg = -1.0 if mutant == "rotate_half_sign" else 1.0
    o1 = rb(f32(rb(y1 * c) + rb(-sg * y2 * s)))
    o2 = rb(f32(rb(y2 * c) + rb(sg * y1 * s)))
    o = torch.cat([o1, o2], -1)
    return o[:, :Hq].reshape(M, Hq * 128), o[:, Hq:], y[:, Hq + Hkv:]


def k_offset(Hkv, lmax, layer, hk, pos):
    """element offset of channel 0 of K row `pos` of KV head hk inside a slot: [layer][K|V][Hkv][Lmax][128]"""
    return ((layer * 2) * Hkv + hk) * lmax * 128 + pos * 128


def v_offsets(Hkv, lmax, layer, hv, pos) -> torch.Tensor:
    """element offsets of the 128 channels of V row `pos`: blocked-transposed [Lmax/32][128][32]"""
    d = torch.arange(128)
    return ((layer * 2 + 1) * Hkv + hv) * lmax * 128 + ((pos >> 5) * 128 + d) * 32 + (pos & 31)


def place_kv(pre: torch.Tensor, Hkv, lmax, layer, tok_stream, kv_len, k64, v64) -> torch.Tensor:
    """pre: [n_slots, per_slot] bf16 pre-image of the arena -> the arena after the append of row m at kv_len[tok_stream[m]]"""
    out = pre.clone()
    for m, slot in enumerate(tok_stream):
        pos = int(kv_len[slot])
        for hk in range(Hkv):
            o = k_offset(Hkv, lmax, layer, hk, pos)
            out[slot, o:o + 128] = k64[m, hk].to(torch.bfloat16)
            out[slot, v_offsets(Hkv, lmax, layer, hk, pos)] = v64[m, hk].to(torch.bfloat16)
    return out


def arena_pattern(n_slots, per_slot) -> torch.Tensor:
    """a recognisable pre-image: bf16 bit patterns (i mod 30011) + 1, all finite, no two neighbours equal"""
    i = torch.arange(n_slots * per_slot, dtype=torch.int64)
    return ((i % 30011) + 1).to(torch.int16).view(torch.bfloat16).view(n_slots, per_slot)


# ---------------------------------------------------------------------------------------------------------------------------------
# activations
# ---------------------------------------------------------------------------------------------------------------------------------
def norm_rows(M, K, g, sgn=None, nw_set=NORM_W):
    """-> (h [M, K], norm weight [K], r [M]): row m is a shuffle, inside every 64 entries, of 16 copies of a quad with sum of squares
    4 c_m (c = 3, 15, 3, 15), so sum h^2 = c_m K while the 16-entry tile statistics vary; r_m = (c_m + 1)^-1/2 = 1/2, 1/4."""
    assert K % 64 == 0
    h = torch.empty(M, K, dtype=torch.float64)
    for m in range(M):      # rows beyond the fourth (the 17..64-row cases of gemm.hip's GEMV) repeat the four quads with shuffles of their own
        quad = torch.tensor(QUADS[ROW_C[m % 4]][(m % 4) // 2], dtype=torch.float64).repeat(16)
        blk = torch.stack([quad[torch.randperm(64, generator=g)] for _ in range(K // 64)]).reshape(K)
        sign = sgn.double() if sgn is not None else torch.where(torch.rand(K, generator=g) < 0.5, -1.0, 1.0).double()
        h[m] = blk * sign
    nw = torch.tensor(nw_set, dtype=torch.float64)[torch.randint(0, len(nw_set), (K,), generator=g)]
    r = torch.tensor([(ROW_C[m % 4] + NORM_EPS) ** -0.5 for m in range(M)], dtype=torch.float64)
    return h, nw, r


def inexact_r_rows(M, K, g):
    """rows with c = 3 and eps = 0: r = 3^-1/2, not a power of two, so h * r really rounds and one rounding differs from two.
    -> (h, norm weight, r [M], eps)"""
    h = torch.empty(M, K, dtype=torch.float64)
    for m in range(M):
        quad = torch.tensor(QUADS[3][m % 2], dtype=torch.float64).repeat(16)
        blk = torch.stack([quad[torch.randperm(64, generator=g)] for _ in range(K // 64)]).reshape(K)
        h[m] = blk * torch.where(torch.rand(K, generator=g) < 0.5, -1.0, 1.0).double()
    nw = torch.tensor(NORM_W, dtype=torch.float64)[torch.randint(0, len(NORM_W), (K,), generator=g)]
    return h, nw, torch.full((M,), 3.0 ** -0.5, dtype=torch.float64), 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_dgemv_exact.py
# ---------------------------------------------------------------------------------------------------------------------------------
RESID_K = {"bf16": (32, 96, 160, 512, 1056), "fp8": (64, 192, 1088), "mxfp4": (128, 384, 1152)}
NORM_K = {"bf16": (64, 192, 512, 1088), "fp8": (64, 192, 1088), "mxfp4": (128, 384, 1152)}
RESID_CASES = [(f, M, 80, K) for f in FORMATS for K in RESID_K[f] for M in (1, 2, 4, 5, 16)] + [("mxfp4", 2, 4112, 128)]      # 257 blocks
NORM_CASES = [(f, M, 48, K) for f in FORMATS for K in NORM_K[f] for M in (1, 2, 3, 4)] + [(f, 1, 48, 8192) for f in FORMATS]
SWIGLU_CASES = [(f, M, 96, K) for (f, M, _, K) in NORM_CASES]
HEADS_K = {(2, 1): {"bf16": 64, "fp8": 64, "mxfp4": 128}, (7, 1): {"bf16": 192, "fp8": 192, "mxfp4": 384},
           (4, 2): {"bf16": 1088, "fp8": 1088, "mxfp4": 1152}}
ROPE_CASES = [(f, M, hq, hkv, HEADS_K[(hq, hkv)][f], 128 if (M == 4 and hq == 4) else 64)
              for f in FORMATS for (hq, hkv) in HEADS_K for M in (1, 2, 3, 4)]
CHAIN_CASES = [1, 2]

# the cases of tests/test_gpu_gemv_exact.py: the weight-streaming GEMVs of csrc/gemm.hip (lcc_gemm_bf16 / _w8_bf16 / _w4_bf16, M <= 16, and the
# 17..64-row form of the bf16 kernel).  Operands: resid_case (x, W) and norm_case(swiglu=True) with x = norm_ref(h, nw, r) handed in normalised.
GEMV_CHUNK = {"bf16": 64, "fp8": 64, "mxfp4": 128}       # k per chunk: the unit the K splits are counted in


def gemv_chunks(fmt, K) -> int:
    return (K + GEMV_CHUNK[fmt] - 1) // GEMV_CHUNK[fmt]


GEMV_BIAS_CASES = [(f, M, 80, K) for f in FORMATS for K in RESID_K[f] for M in (1, 5, 16)]
# (fmt, M, N, K, nsplit): the largest K (17 chunks, 9 for MXFP4) in 1, 3 and as many splits as chunks; the smallest K (one chunk) unsplit
GEMV_SLAB_CASES = ([(f, M, 80, max(RESID_K[f]), S) for f in FORMATS for M in (1, 5, 16) for S in (1, 3, gemv_chunks(f, max(RESID_K[f])))]
                   + [(f, M, 80, min(RESID_K[f]), 1) for f in FORMATS for M in (1, 5, 16)])
GEMV_SWIGLU_CASES = SWIGLU_CASES
GEMV_MG_CASES = [("bf16", M, 80, K) for M in (17, 33, 64) for K in (192, 1088)]       # 2, 3, 4 activation groups, the last one 1 / 1 / 16 rows
GEMV_MG_SWIGLU_CASES = [("bf16", M, 96, K) for M in (17, 33, 64) for K in (192, 1088)]
GEMV_MG_SLAB_CASES = [("bf16", 33, 80, 1088, 3)]
GEMV_VARIANT_CASES = {"plain": ("bf16", 5, 80, 1056), "swiglu": ("bf16", 3, 96, 1088)}      # run under gemv_variant 0 and 2


def gemv_bias(N) -> torch.Tensor:
    """multiples of 1/4 up to 16 in magnitude: bf16 values, far below one bf16 ulp of most accumulators"""
    return ints(gen(N, 8), (N,), 64) / 4.0


def slab_ranges(fmt, K, nsplit, shift=0):
    """the k range of split s: chunks [s * cps, min(nchunk, (s + 1) * cps)), cps = ceil(nchunk / nsplit).  shift: every boundary moved by that many
    chunks (the mutant)"""
    chunk, nchunk = GEMV_CHUNK[fmt], gemv_chunks(fmt, K)
    cps = (nchunk + nsplit - 1) // nsplit
    return [(min(K, max(0, s * cps + shift) * chunk), min(K, max(0, min(nchunk, (s + 1) * cps) + shift) * chunk)) for s in range(nsplit)]


def slab_ref(x64, W, nsplit, shift=0) -> torch.Tensor:
    """[nsplit, M, N]: fp32(acc_s * scale), acc_s the exact sum over the k range of split s"""
    q, sc = W["q64"], W["scale64"]
    return torch.stack([f32((x64[:, a:b] @ q[:, a:b].t()) * sc[None, :]) for a, b in slab_ranges(W["fmt"], W["K"], nsplit, shift)])


@functools.lru_cache(maxsize=None)
def resid_case(fmt, M, N, K) -> dict:
    g = gen(fmt, M, N, K, 1)
    aw, ax, px = amplitudes(fmt, K)
    W = make_weight(fmt, N, K, g, aw=aw, int_valued=True)
    x = nonzero_ints(g, (M, K), ax) * (torch.rand(M, K, generator=g) < px)
    h0 = ints(g, (M, N), 15)
    return dict(W=W, x=x, h0=h0)


def _gates_are_safe(W, h, nw, r) -> bool:
    """no gate in the denormal range of silu, and every silu the kernel evaluates with its fp32 transcendental at least 2^-10 ulp (2^-18
    relative: far beyond the error of an fp32 exp and reciprocal) from a bf16 rounding tie -- so even those outputs are unique"""
    _, g, sat = swiglu_ref(norm_ref(h, nw, r), W)
    gu = g[~sat]
    if bool(((gu >= GATE_GRAY[0]) & (gu <= GATE_GRAY[1])).any()):
        return False
    return bool((silu_tie_margin(gu[gu > GATE_GRAY[1]]) > 2.0 ** -10).all())


@functools.lru_cache(maxsize=None)
def norm_case(fmt, M, N, K, swiglu=False) -> dict:
    big = K >= 8192
    for salt in range(64):      # SwiGLU: a draw that puts a silu next to a rounding tie is replaced by the next one, not tolerated
        g = gen(fmt, M, N, K, 3 if swiglu else 2, salt)
        sgn = torch.where(torch.rand(K, generator=g) < 0.5, -1.0, 1.0) if swiglu else None
        h, nw, r = norm_rows(M, K, g, sgn=sgn, nw_set=NORM_W_PLAIN if big else NORM_W)
        row_mode = None
        if swiglu:      # of every 8 gate rows: 2 zero, 3 aligned with the activations' signs (gate >= 32), 1 opposed (gate <= -104), 2 small; up rows random
            n = torch.arange(N)
            gate = (n % 32) < 16
            row_mode = torch.where(gate, torch.tensor(GATE_ROW_MODES)[n % 8], torch.zeros(N, dtype=torch.int64))
        p3 = min(1.0, 100.0 / (K * {"bf16": 1.0, "fp8": 3.0, "mxfp4": 21.0}[fmt]))
        W = make_weight(fmt, N, K, g, aw=7 if big else 5 if K >= 1024 else 15, fp8_mul=1, scales=FP8_SCALES_FRAC, row_mode=row_mode, sgn=sgn, p3=p3,
                        w_density=0.4 if (fmt == "mxfp4" and K >= 1024) else 1.0)
        bias = ints(g, (N,), 64) / 4.0
        if not swiglu or _gates_are_safe(W, h, nw, r):
            return dict(W=W, h=h, nw=nw, r=r, eps=NORM_EPS, bias=bias)
    raise AssertionError("no safe draw")


def rope_positions(case_index, M, lmax):
    """the cache positions of the M streams: a window of (0, 31, 32, 63, lmax - 1) that moves with the case, so every one is written"""
    ring = (0, 31, 32, 63, lmax - 1)
    return [ring[(case_index + m + (4 if lmax > 64 else 0)) % 5] for m in range(M)] if lmax == 64 else [lmax - 1, 0, 32, 63, 31][:M]


@functools.lru_cache(maxsize=None)
def rope_case(fmt, M, Hq, Hkv, K, lmax) -> dict:
    g = gen(fmt, M, Hq, Hkv, K, 4)
    N = (Hq + 2 * Hkv) * 128
    h, nw, r = norm_rows(M, K, g)
    W = make_weight(fmt, N, K, g, aw=5 if K >= 1024 else 15, fp8_mul=1, scales=FP8_SCALES_FRAC, w_density=0.4 if (fmt == "mxfp4" and K >= 1024) else 1.0)
    bias = ints(g, (N,), 64) / 4.0
    n_slots = M + 1
    tok_stream = [(2 * m + 1) % n_slots for m in range(M)] if M > 1 else [1]      # distinct (n_slots and 2 coprime or M small), never the identity
    if len(set(tok_stream)) != M:
        tok_stream = list(range(M, 0, -1))
    idx = ROPE_CASES.index((fmt, M, Hq, Hkv, K, lmax))
    kv_len = [7] * n_slots                                     # the unused slot keeps a length of its own
    for m, p in enumerate(rope_positions(idx, M, lmax)):
        kv_len[tok_stream[m]] = p
    pos3 = torch.tensor([[5 + 11 * m for m in range(M)], [77 + 3 * m for m in range(M)], [1234 - 7 * m for m in range(M)]], dtype=torch.int32)
    return dict(W=W, h=h, nw=nw, r=r, eps=NORM_EPS, bias=bias, n_slots=n_slots, tok_stream=tok_stream, kv_len=kv_len, pos3=pos3, layer=1,
                n_layers=2)


@functools.lru_cache(maxsize=None)
def chain_case(M) -> dict:
    """down_proj + q|k|v in one launch: x is one-hot per row, so the Linear output of row m is ONE column of the down weight, chosen such
    that h0 + column is a norm row (sum of squares c K): the residual stream the consumer normalises is exact by construction."""
    H, I, Hq, Hkv = 256, 512, 2, 1
    g = gen("bf16", M, H, I, 5)
    h1, nw, r = norm_rows(M, H, g)
    h0 = ints(g, (M, H), 3)
    Wd = make_weight("bf16", H, I, g)
    cols = [37, 300][:M]
    x = torch.zeros(M, I, dtype=torch.float64)
    for m, c in enumerate(cols):
        x[m, c] = 1.0
        Wd["q64"][:, c] = h1[m] - h0[m]
    Wd["rows"] = Wd["q64"].to(torch.bfloat16)
    assert torch.equal(Wd["rows"].double(), Wd["q64"])
    Wq = make_weight("bf16", (Hq + 2 * Hkv) * 128, H, g)
    bias = ints(g, ((Hq + 2 * Hkv) * 128,), 64) / 4.0
    pos3 = torch.tensor([[9 + m for m in range(M)], [40 + m for m in range(M)], [700 + m for m in range(M)]], dtype=torch.int32)
    return dict(Wd=Wd, Wq=Wq, x=x, h0=h0, h1=h1, nw=nw, r=r, eps=NORM_EPS, bias=bias, Hq=Hq, Hkv=Hkv, H=H, I=I, pos3=pos3,
                tok_stream=list(range(M)), kv_len=[31, 32][:M], lmax=64)


@functools.lru_cache(maxsize=None)
def inexact_case(M) -> dict:
    """RMSNorm + Linear with r = 3^-1/2 (bf16 weights, K = 192): the one case where bf16(h * r) really rounds"""
    K, N = 192, 48
    h, nw, r, eps = inexact_r_rows(M, K, gen(M, K, 6))
    r = torch.rsqrt(torch.full((M,), 3.0, dtype=torch.float32)).double()
    return dict(W=make_weight("bf16", N, K, gen(M, 7)), h=h, nw=nw, r=r, eps=eps, N=N, K=K)


def qkv_perm(Hq, Hkv, K):
    from livecc_amd.config import LiveCCConfig
    from livecc_amd.weights import qkv_decode_row_permutation
    return qkv_decode_row_permutation(LiveCCConfig(num_attention_heads=Hq, num_key_value_heads=Hkv, hidden_size=K))


def hf_mrope_rows(pos3: torch.Tensor, theta=1e6):
    """CPU restatement of the M-RoPE table rows (sections 16, 24, 24), bf16 -> float64 [S, 64]: stands in for ops.mrope_table where no GPU
    is present (the GPU tests read the real table back)"""
    inv = 1.0 / (theta ** (torch.arange(0, 128, 2, dtype=torch.float) / 128))
    fr = pos3.float()[:, :, None] * inv[None, None, :]
    sec = [16, 24, 24]
    cos, sin = fr.cos().to(torch.bfloat16), fr.sin().to(torch.bfloat16)
    cs = torch.cat([m[i % 3] for i, m in enumerate(cos.split(sec, dim=-1))], -1)
    sn = torch.cat([m[i % 3] for i, m in enumerate(sin.split(sec, dim=-1))], -1)
    return cs.double(), sn.double(), inv

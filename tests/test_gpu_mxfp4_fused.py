"""-m gpu: the 8-wave tile GEMMs staging MXFP4 weights themselves (csrc/gemm.hip: W4Fused -- gemm_big_kernel, gemm_vh_kernel and gemm_tall_kernel
with PACKED4 fragments and e8m0 scale bytes DMA'd straight from the arena and expanded behind the LDS read).  The expanded operand is the bf16
weight itself and the MFMA stream is the bf16 kernel's, so the oracle everywhere is the bf16 operator on pack_weight(dequantised weight),
compared with torch.equal.  Every call also shows that no dequantisation pass ran: the caller's scratch keeps its sentinel, the launch counter
`gemm_w4_fused` rises by one and `gemm_w4_dequant` does not move.

Shapes are the smallest at which each thing can go wrong: K = 128 (one fragment: ring prologue only), 384 (three fragments = six k-tiles: the
rings wrap, the last fragment is used in two halves, and two splits start in the middle of a fragment), 1024; N = 256 (one column tile) and
272 (ragged second tile: clamped fragment row, a half-fragment pair across the clamp), 320 / 336 for the 160-column tiles of the tall
kernel; M per family at a wave pair without rows, a ragged last row tile and more than one row tile."""
import pytest
import torch

from tests.test_gpu_mxfp4 import _w4
from tests.test_gpu_ops import _rand

pytestmark = pytest.mark.gpu

SENTINEL = 0x7B5A      # bit pattern the scratch is filled with (a finite bf16 no kernel here produces in bulk)
_CACHE = {}


@pytest.fixture
def force():
    """force(variant): lcc_debug_set_gemm_variant for the test, the default routing afterwards."""
    from livecc_amd import ops
    yield ops.set_gemm_variant
    ops.set_gemm_variant(ops.GEMM_DEFAULT_VARIANT)
    ops.set_w4_fused(True)


def _weights(dev, N, K):
    """(PACKED4 bytes, scale bytes, packed bf16 twin) of a seeded [N, K] matrix, made once per shape and never written."""
    from livecc_amd import ops
    if (N, K) not in _CACHE:
        w4, s4, wd, _, _ = _w4(dev, N, K, 2, 0.05)
        _CACHE[(N, K)] = (w4, s4, ops.pack_weight(wd.to(torch.bfloat16)))
    return _CACHE[(N, K)]


def _scratch(dev, N, K):
    return torch.full((N * K,), SENTINEL, dtype=torch.int16, device=dev).view(torch.bfloat16)


def _fused_call(dev, M, N, K, code, epi=0, nsplit=0, weights=None, x=None, with_bias=True):
    """One lcc_gemm_w4_bf16 call that must take the fused route on tile `code`; returns (got, want)."""
    from livecc_amd import ops
    w4, s4, wp = weights if weights is not None else _weights(dev, N, K)
    assert ops.gemm_w4_plan(M, N, K, epi, nsplit) == (code, 1), (M, N, K, epi, nsplit, ops.gemm_w4_plan(M, N, K, epi, nsplit))
    x = _rand((M, K), dev, 1.0, 1) if x is None else x
    bias = _rand((N,), dev, 0.1, 3) if (epi == 0 and nsplit == 0 and with_bias) else None
    res = _rand((M, N), dev, 1.0, 4) if epi == 3 else None
    dq = _scratch(dev, N, K)
    before = ops.launch_counts()
    got = ops.linear_w4(x, w4, s4, bias, epi, res, nsplit=nsplit, dq_scratch=dq)
    after = ops.launch_counts()
    want = ops.linear_partial(x, wp, nsplit, packed_shape=(N, K)) if nsplit else ops.linear(x, wp, bias, epi, res, packed_shape=(N, K))
    what = (M, N, K, code, epi, nsplit)
    assert after["gemm_w4_fused"] == before["gemm_w4_fused"] + 1 and after["gemm_w4_dequant"] == before["gemm_w4_dequant"], (what, before, after)
    assert bool((dq.view(torch.int16) == SENTINEL).all()), (what, "the dequantisation scratch was written")
    assert got.shape == want.shape and torch.equal(got, want), (what, int((got != want).sum()))
    return got, want


def _cases(N, K, slabs=True):
    """(epilogue, nsplit): bias, residual, SwiGLU where N pairs 32 rows, and the slab form with two split counts per K."""
    out = [(0, 0), (3, 0)] + ([(4, 0)] if N % 32 == 0 else [])
    if slabs:
        out += [(0, s) for s in {128: (1, 2), 384: (2, 3), 1024: (2, 4)}[K]]      # 384 / 2: an odd k-tile count per split -> split 1 starts mid-fragment
    return out


@pytest.mark.parametrize("K", [128, 384, 1024])
@pytest.mark.parametrize("variant,code", [(3, 256), (13, 192), (4, 128)])
def test_big_tiles(dev, force, variant, code, K):
    """gemm_big_kernel, BM 256 / 192 / 128.  M = 130: the second row tile of the 128-row form holds two rows (its upper wave pair has none),
    386: ragged last tile of every height."""
    force(variant)
    for M in (130, 386):
        for N in (256, 272):
            for epi, ns in _cases(N, K):
                _fused_call(dev, M, N, K, code, epi, ns)


@pytest.mark.parametrize("K", [128, 384, 1024])
def test_variable_height_tiles(dev, force, K):
    """gemm_vh_kernel, large class: M = 272 is one tile of 17 fragments (the extra activation slot is live), 544 two of them."""
    force(14)
    for M in (272, 544):
        for N in (256, 272):
            for epi, ns in _cases(N, K):
                _fused_call(dev, M, N, K, 272, epi, ns)


@pytest.mark.parametrize("K", [128, 384, 1024])
def test_small_variable_height_tiles(dev, force, K):
    """gemm_vh_kernel, small class (slabs only; three-stage ring with the counted wait): M = 144 is one tile of 9 fragments, 386 = 9 + 8 + 8."""
    force(15)
    for M in (144, 386):
        for N in (256, 272):
            for epi, ns in _cases(N, K):
                if ns:
                    _fused_call(dev, M, N, K, 144, epi, ns)


@pytest.mark.parametrize("K", [128, 384, 1024])
def test_tall_tile(dev, force, K):
    """gemm_tall_kernel (no slab form): 160-column tiles, N = 320 two full ones, 336 a ragged third; M = 257 (the third M-wave holds 33 rows: its
    four-row-tile path, the fourth none), 386 (a streaming chunk), 448 (every row of the block tile)."""
    force(8)
    for M in (257, 386, 448):
        for N in (320, 336):
            for epi, ns in _cases(N, K, slabs=False):
                _fused_call(dev, M, N, K, 448, epi, ns)


# ---- key-exact layout: the `keyed` fixture of tests/test_gpu_mxfp4.py at a fused shape ----
_KX_N, _KX_K = 256, 384
_KX_COLS = list(range(128)) + [256, 383]      # every k of fragment 0 + the first and the last k of the last fragment


@pytest.fixture(scope="module")
def keyed(dev):
    """A 256 x 384 weight whose every 32-block has its own octave, the 130 one-hot activation rows that read its columns, and those columns of
    the CPU-dequantised weight."""
    from livecc_amd import ops
    from livecc_amd.weights import dequantize_mxfp4_rows, quantize_mxfp4_rows
    g = torch.Generator().manual_seed(5)
    octave = torch.randint(-9, 6, (_KX_N, _KX_K // 32), generator=g)
    w = torch.randn(_KX_N, _KX_K, generator=g) * torch.exp2(octave.float()).repeat_interleave(32, dim=1)
    codes, sc = quantize_mxfp4_rows(w)
    assert len(torch.unique(sc)) >= 8, "the scales must differ between blocks"
    wd = dequantize_mxfp4_rows(codes, sc)
    w4, s4 = ops.quantize_mxfp4(w.to(dev))
    x = torch.zeros(len(_KX_COLS), _KX_K, dtype=torch.bfloat16)
    x[torch.arange(len(_KX_COLS)), torch.tensor(_KX_COLS)] = 1.0
    want = wd.t()[torch.tensor(_KX_COLS)]      # [rows, N] fp32: row m = column k_m; every value is a bf16
    assert torch.equal(want.to(torch.bfloat16).float(), want)
    return (w4, s4, ops.pack_weight(wd.to(torch.bfloat16).to(dev))), x.to(dev), want


@pytest.mark.parametrize("variant,code,rows,nsplit", [(4, 128, 130, 0), (3, 256, 130, 0), (13, 192, 130, 0), (14, 272, 272, 0), (15, 144, 130, 2), (8, 448, 130, 0)])
def test_one_hot_rows_read_the_dequantised_columns_bit_for_bit(dev, force, keyed, variant, code, rows, nsplit):
    """x[m, k_m] = 1: output row m is ONE exact product plus exact zeros, so it equals column k_m of the CPU-dequantised weight -- a wrong dword,
    half fragment, scale byte or lane pairing changes a value that random data could hide behind equal sums.  Once per kernel family (the large
    variable-height class needs 16 row fragments: the 130 rows are followed by zero rows; the small class exists for slabs: their sum is exact)."""
    weights, x, want = keyed
    force(variant)
    if rows > x.shape[0]:
        x = torch.cat([x, torch.zeros(rows - x.shape[0], _KX_K, dtype=torch.bfloat16, device=dev)])
    got, _ = _fused_call(dev, rows, _KX_N, _KX_K, code, 0, nsplit, weights=weights, x=x, with_bias=False)
    got = (got.sum(0) if nsplit else got.float()).cpu()
    n = len(_KX_COLS)
    assert torch.equal(got[:n], want), int((got[:n] != want).sum())
    assert not bool(got[n:].any())


# ---- the engine ----
def test_engine_prefill_on_the_fused_route_equals_the_dequantising_route(dev, force):
    """A 69-row prefill + 4 decode steps of a seeded tiny model with MXFP4 weights, the 128-row 8-wave tiles forced so that its four Linears reach a
    fused route (the default scores send shapes this small to the 4-wave tiles): same logits and tokens with the knob on and off, the prefill
    on the fused kernels with the knob on and on the dequantising route with it off; a bf16 model built afterwards reproduces its own tokens."""
    from livecc_amd import ops, protocol
    from livecc_amd.config import tiny
    from livecc_amd.modeling import LiveCCForConditionalGeneration
    cfg = tiny()
    ids = protocol.TurnBuilder(cfg, seed=5).turn_ids(0, protocol.num_video_tokens(protocol.grid_of(10, 56, 84, cfg), cfg))
    frames = torch.from_numpy(protocol.synth_frames(10, 56, 84, seed=5, layout="TCHW"))
    S, H, I = len(ids), cfg.hidden_size, cfg.intermediate_size
    qd = cfg.num_attention_heads * 128
    qkvd = qd + 2 * cfg.num_key_value_heads * 128
    assert S > 64
    force(4)
    for N, K, epi in ((qkvd, H, 0), (H, qd, 3), (2 * I, H, 4), (H, I, 3)):
        assert ops.gemm_plan(S, N, K, w_fp8=True)[1] == 1, "the engine would ask for slabs here"
        assert ops.gemm_w4_plan(S, N, K, epi) == (128, 1), (S, N, K, epi)

    def greedy(model):
        r = model.generate(input_ids=torch.from_numpy(ids).view(1, -1), frames=frames, max_new_tokens=5, min_new_tokens=5, output_logits=True)
        out = (r.sequences[0, len(ids):].tolist(), r.logits.clone())
        r.past_key_values.release()
        return out

    def counted(model):
        before = ops.launch_counts()
        out = greedy(model)
        after = ops.launch_counts()
        return out, after["gemm_w4_fused"] - before["gemm_w4_fused"], after["gemm_w4_dequant"] - before["gemm_w4_dequant"]
    kw = dict(max_streams=1, max_kv_len=1024, max_new_rows=512, max_patches=2048, max_history=16)
    mx = LiveCCForConditionalGeneration.from_config(cfg, dev, seed=2, llm_weights="mxfp4", **kw)
    (toks_on, logits_on), fused, dequant = counted(mx)
    assert len(toks_on) == 5 and fused == 4 * cfg.num_hidden_layers and dequant == 0, (fused, dequant)
    ops.set_w4_fused(False)
    (toks_off, logits_off), fused, dequant = counted(mx)
    assert fused == 0 and dequant == 4 * cfg.num_hidden_layers, (fused, dequant)
    assert toks_on == toks_off and torch.equal(logits_on, logits_off)
    ops.set_w4_fused(True)
    bf = LiveCCForConditionalGeneration.from_config(cfg, dev, seed=2, **kw)
    toks, logits = greedy(bf)
    toks2, logits2 = greedy(bf)
    assert toks2 == toks and torch.equal(logits2, logits)

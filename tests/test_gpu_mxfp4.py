"""-m gpu: MXFP4 weights (OCP e2m1 elements, one e8m0 scale per 32 consecutive k of a row) through the C-ABI.  MX scales are powers of two, so the
expanded weight is exact in bf16 and every oracle here is "the bf16 operator on the dequantised weight": the same arithmetic class as the fp8 path
(exactly expanded weights, bf16 MFMA, fp32 sums), hence the tolerances of the corresponding fp8 tests, unchanged."""
import math

import pytest
import torch

from tests.test_gpu_decode_v2 import _rmsnorm_ref, _staged, resid_waves  # noqa: F401  (resid_waves: fixture)
from tests.test_gpu_ops import _hf_mrope_ref, _rand, _ref_linear
from tests.util import assert_bf16_close

pytestmark = pytest.mark.gpu


def _w4(dev, N, K, seed, std=0.03):
    """(PACKED4 bytes, packed scale bytes, dequantised fp32 weight, codes, scales) of a seeded matrix, quantised on the GPU."""
    from livecc_amd import ops
    from livecc_amd.weights import dequantize_mxfp4_rows, pack_scale_mxfp4, pack_weight_mxfp4, quantize_mxfp4_rows
    w = _rand((N, K), dev, std, seed).float()
    codes, sc = quantize_mxfp4_rows(w)
    w4, s4 = ops.quantize_mxfp4(w)
    assert torch.equal(w4, pack_weight_mxfp4(codes)) and torch.equal(s4, pack_scale_mxfp4(sc))
    return w4, s4, dequantize_mxfp4_rows(codes, sc), codes, sc


def test_mxfp4_quantiser_gives_the_same_bytes_on_the_gpu_as_on_the_cpu(dev):
    """The arena quantises on the GPU, an oracle on the CPU: same codes and same scale bytes (the rule is integer operations, exact power-of-two
    products and comparisons only).  The shape / std pairs of the fp8 byte test."""
    from livecc_amd.weights import quantize_mxfp4_rows
    g = torch.Generator().manual_seed(11)
    for shape, std in (((1024, 4096), 0.02), ((256, 8192), 1.0), ((64, 512), 1e-4)):
        w = (torch.randn(*shape, generator=g) * std).to(torch.bfloat16)
        cc, sc = quantize_mxfp4_rows(w)
        cg, sg = quantize_mxfp4_rows(w.to(dev))
        assert torch.equal(sc, sg.cpu()), shape
        assert torch.equal(cc, cg.cpu()), (shape, int((cc != cg.cpu()).sum()))


# ---- key-exact layout test: nibble order, k -> MFMA slot, scale lookup and the scale semantics of the conversion instruction in one go ----
_KX_N, _KX_K = 48, 384
_KX_COLS = list(range(128)) + [256, 383]      # every position of one fragment + the first and the last k of the last fragment


@pytest.fixture(scope="module")
def keyed(dev):
    """A weight whose blocks span several octaves (every block has its own scale) and the one-hot activation rows that read its columns."""
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
    want = wd.t()[torch.tensor(_KX_COLS)].to(torch.bfloat16)      # [rows, N]: row m = column k_m; lossless (every value is a bf16)
    assert torch.equal(want.float(), wd.t()[torch.tensor(_KX_COLS)])
    return w4, s4, x.to(dev), want


@pytest.mark.parametrize("route,rows", [("gemv", 16), ("dequantise", 17), ("dgemv_resid", 4)])
def test_one_hot_rows_read_the_dequantised_columns_bit_for_bit(dev, keyed, route, rows):
    """x[m, k_m] = 1: output row m is ONE exact product (w[n, k_m] x 1.0) plus exact zeros, so it must equal column k_m of the CPU-dequantised
    weight exactly -- a wrong nibble, MFMA slot, scale byte or exponent bias changes a value.  (Equality of values: the sums cannot produce -0.)"""
    from livecc_amd import ops
    w4, s4, x, want = keyed
    for r0 in range(0, x.shape[0], rows):
        xs = x[r0:r0 + rows].contiguous()
        if route == "dgemv_resid":
            got = torch.zeros(xs.shape[0], _KX_N, dtype=torch.bfloat16, device=dev)
            ops.dgemv_resid_(w4, xs, got, (_KX_N, _KX_K), w4scale=s4)
        else:
            got = ops.linear_w4(xs, w4, s4)
        assert torch.equal(got.cpu(), want[r0:r0 + rows]), (route, r0, int((got.cpu() != want[r0:r0 + rows]).sum()))


# ---- M > 16: exact dequantisation + the bf16 route ----
_DQ_SHAPES = [(17, 272, 128), (40, 512, 256), (386, 1536, 1024)]


@pytest.mark.parametrize("M,N,K,epi", [(m, n, k, e) for (m, n, k) in _DQ_SHAPES for e in (0, 3, 4) if e != 4 or n % 32 == 0])      # SwiGLU pairs 32 rows
def test_dequantise_route_is_bit_identical_to_the_bf16_gemm_on_the_dequantised_weight(dev, M, N, K, epi):
    from livecc_amd import ops
    w4, s4, wd, _, _ = _w4(dev, N, K, 2, 0.05)
    wp = ops.pack_weight(wd.to(torch.bfloat16))
    x, b = _rand((M, K), dev, 1.0, 1), (_rand((N,), dev, 0.1, 3) if epi == 0 else None)
    res = _rand((M, N), dev, 1.0, 4) if epi == 3 else None
    got = ops.linear_w4(x, w4, s4, b, epi, res)
    want = ops.linear(x, wp, b, epi, res, packed_shape=(N, K))
    assert torch.equal(got, want), int((got != want).sum())
    if epi == 0:
        part, pref = ops.linear_w4(x, w4, s4, nsplit=2), ops.linear_partial(x, wp, 2, packed_shape=(N, K))
        assert torch.equal(part, pref)


# ---- M <= 16: the weight-streaming GEMV ----
@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("N,K", [(16, 128), (272, 896), (4608, 3584), (3584, 18944)])
def test_gemv_w4(dev, M, N, K):
    """Plain (+ bias) and split-K slabs against the bf16 linear of the dequantised weight; tolerances of test_gemv_w8_fp8_weights."""
    from livecc_amd import ops
    x, b = _rand((M, K), dev, 1.0, 1), _rand((N,), dev, 0.1, 3)
    w4, s4, wd, _, _ = _w4(dev, N, K, 2)
    got = ops.linear_w4(x, w4, s4, b)
    ref, atol = _ref_linear(x, wd, b, with_atol=True)
    assert_bf16_close(got, ref, f"gemv_w4[{M}x{N}x{K}]", max_ulp=1.0, max_frac=5e-3, atol=atol)
    S = min(ops.gemv_num_splits(N, K), K // 128)
    part = ops.linear_w4(x, w4, s4, nsplit=S)
    r32 = x.float() @ wd.t()
    err = (part.sum(0) - r32).abs().max().item()
    print(f"gemv_w4 slabs [{M}x{N}x{K}] S={S}: err {err:.3e}")
    assert err <= 2e-5 * float(r32.abs().max()) * math.sqrt(K / 256) + 1e-5, f"mxfp4 split-K slabs: {err}"


@pytest.mark.parametrize("M,I,K", [(1, 512, 256), (8, 2432, 896)])
def test_gemv_w4_swiglu(dev, M, I, K):
    from livecc_amd import ops
    x = _rand((M, K), dev, 1.0, 1)
    w4, s4, wd, _, _ = _w4(dev, 2 * I, K, 2, 0.05)
    got = ops.linear_w4(x, w4, s4, None, ops.EPI_SWIGLU)
    ref, atol = _ref_linear(x, wd, None, 4, with_atol=True)
    assert_bf16_close(got, ref, f"gemv_w4_swiglu[{M}x{I}x{K}]", max_ulp=1.0, max_frac=5e-3, atol=atol)


# ---- pipeline-v2 GEMVs: tolerances of the test_fp8_* tests of tests/test_gpu_decode_v2.py ----
@pytest.mark.parametrize("M,N,K", _staged([1, 2, 4], [(1024, 256), (37888, 3584)]) + [(1, 1024, 128), (2, 1024, 896)])      # one fragment; ragged across waves
def test_w4_norm_swiglu_gemv(dev, M, N, K):
    from livecc_amd import ops
    h, nw = _rand((M, K), dev, 2.0, 1), (1.0 + 0.1 * _rand((K,), dev, 1.0, 3).float()).to(torch.bfloat16)
    w4, s4, wd, _, _ = _w4(dev, N, K, 2)
    got = ops.dgemv_norm_linear(w4, h, ops.tile_stats(h), nw, 1e-6, (N, K), swiglu=True, w4scale=s4)
    ref, atol = _ref_linear(_rmsnorm_ref(h, nw, 1e-6).to(torch.bfloat16), wd, None, 4, with_atol=True)
    assert_bf16_close(got, ref, f"dgemv_w4_norm_swiglu[{M}x{N}x{K}]", max_ulp=1.0, max_frac=1e-2, atol=atol)


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N,K", [(2048, 256), (152064, 3584)])
def test_w4_norm_linear_gemv_lm_head(dev, M, N, K):
    from livecc_amd import ops
    h, nw = _rand((M, K), dev, 2.0, 4), (1.0 + 0.1 * _rand((K,), dev, 1.0, 6).float()).to(torch.bfloat16)
    w4, s4, wd, _, _ = _w4(dev, N, K, 5)
    got = ops.dgemv_norm_linear(w4, h, ops.tile_stats(h), nw, 1e-6, (N, K), w4scale=s4)
    ref, atol = _ref_linear(_rmsnorm_ref(h, nw, 1e-6).to(torch.bfloat16), wd, None, with_atol=True)
    assert_bf16_close(got, ref, f"dgemv_w4_norm_linear[{M}x{N}x{K}]", max_ulp=1.0, max_frac=1e-2, atol=atol)


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N,K", [(256, 512), (3584, 3584), (3584, 18944), (256, 128), (256, 896)])      # 128: seven of eight waves idle; 896: ragged
def test_w4_residual_gemv_and_tile_statistics(dev, M, N, K, resid_waves):
    from livecc_amd import ops
    x, h0 = _rand((M, K), dev, 1.0, 7), _rand((M, N), dev, 2.0, 9)
    w4, s4, wd, _, _ = _w4(dev, N, K, 8)
    h = h0.clone()
    stats = ops.dgemv_resid_(w4, x, h, (N, K), w4scale=s4)
    ref, atol = _ref_linear(x, wd, None, 3, h0, with_atol=True)
    assert_bf16_close(h, ref, f"dgemv_w4_resid[{M}x{N}x{K}]", max_ulp=1.0, max_frac=1e-2, atol=atol)
    assert torch.allclose(stats, ops.tile_stats(h), rtol=1e-6, atol=1e-6)


def test_w4_residual_gemv_on_a_grid_of_more_than_one_block_per_cu(dev):
    """N / 16 > 256 blocks takes the two-chunks-per-stage instantiation (72B-like hidden size, short K)."""
    from livecc_amd import ops
    M, N, K = 2, 8192, 1024
    x, h0 = _rand((M, K), dev, 1.0, 7), _rand((M, N), dev, 2.0, 9)
    w4, s4, wd, _, _ = _w4(dev, N, K, 8)
    h = h0.clone()
    stats = ops.dgemv_resid_(w4, x, h, (N, K), w4scale=s4)
    ref, atol = _ref_linear(x, wd, None, 3, h0, with_atol=True)
    assert_bf16_close(h, ref, f"dgemv_w4_resid[{M}x{N}x{K}]", max_ulp=1.0, max_frac=1e-2, atol=atol)
    assert torch.allclose(stats, ops.tile_stats(h), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("Hq,Hkv,K", [(2, 1, 256), (28, 4, 3584)])
@pytest.mark.parametrize("M", [1, 2])
def test_w4_qkv_gemv_with_rope_and_kv_append(dev, Hq, Hkv, K, M):
    """The MXFP4 decode copy (code rows AND scale rows permuted) in one launch against the chain on the un-permuted weight: RMSNorm -> MXFP4
    split-K GEMV slabs (lcc_gemm_w4_bf16) -> rope_kv_append.  The same codes and scales on both sides: only the fp32 summation order differs."""
    from livecc_amd import ops
    from livecc_amd.config import LiveCCConfig
    from livecc_amd.weights import pack_scale_mxfp4, pack_weight_mxfp4, qkv_decode_row_permutation
    N = (Hq + 2 * Hkv) * 128
    cfg = LiveCCConfig(num_attention_heads=Hq, num_key_value_heads=Hkv, hidden_size=K)
    h, b = _rand((M, K), dev, 2.0, 11), _rand((N,), dev, 0.2, 13)
    nw = (1.0 + 0.1 * _rand((K,), dev, 1.0, 14).float()).to(torch.bfloat16)
    w4, s4, _, codes, sc = _w4(dev, N, K, 12)
    perm = qkv_decode_row_permutation(cfg).to(dev)
    w4_dec, s4_dec = pack_weight_mxfp4(codes[perm].contiguous()), pack_scale_mxfp4(sc[perm].contiguous())
    lens = [37, 100][:M]
    kv_a, kv_b = ops.KvArena(M, 1, Hkv, 256, dev), ops.KvArena(M, 1, Hkv, 256, dev)
    slots = torch.arange(M, dtype=torch.int32, device=dev)
    kv_len = torch.tensor(lens, dtype=torch.int32, device=dev)
    pos3 = torch.tensor([[l + 3 for l in lens]] * 3, dtype=torch.int32)
    _, _, inv = _hf_mrope_ref(pos3)
    c, s_ = ops.mrope_table(pos3.to(dev), inv.to(dev), [16, 24, 24])
    q_got = ops.dgemv_qkv_rope(w4_dec, h, ops.tile_stats(h), nw, 1e-6, b, c, s_, slots, kv_len, kv_a, 0, Hq, w4scale=s4_dec)
    xn = _rmsnorm_ref(h, nw, 1e-6).to(torch.bfloat16)
    part = ops.linear_w4(xn, w4, s4, nsplit=min(8, ops.gemv_num_splits(N, K), K // 128))
    q_ref = ops.rope_kv_append(None, c, s_, slots, None, kv_b, 0, Hq, partial=part, bias=b, kv_len=kv_len)
    assert_bf16_close(q_got, q_ref, f"dgemv_w4_qkv_rope.q[{Hq},{Hkv},{K},M{M}]", max_ulp=2.0, max_frac=2e-2, atol=2e-2)
    assert_bf16_close(kv_a.buf, kv_b.buf, "dgemv_w4_qkv_rope.kv", max_ulp=2.0, max_frac=2e-2, atol=2e-2)


def test_the_two_scale_keywords_exclude_each_other(dev):
    from livecc_amd import ops
    w4, s4, _, _, _ = _w4(dev, 16, 128, 1)
    x, h = _rand((1, 128), dev, 1.0, 2), _rand((1, 16), dev, 1.0, 3)
    with pytest.raises(ValueError):
        ops.dgemv_resid_(w4, x, h, (16, 128), wscale=torch.ones(16, device=dev), w4scale=s4)


# ---- the engine with an MXFP4 arena ----
def _fake_quantize_llm_mxfp4(model) -> None:
    """Every weight of the quantised set (q/k/v/o, gate/up/down, lm_head) replaced by its MXFP4 dequantisation: the values the native path
    computes with.  Lossless in fp32 AND in bf16 (MX scales are powers of two), so both oracles hold the same numbers."""
    from livecc_amd.weights import dequantize_mxfp4_rows, quantize_mxfp4_rows
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.dim() != 2 or "visual" in n or "embed_tokens" in n:
                continue
            if not any(k in n for k in ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj", "lm_head")):
                continue
            p.copy_(dequantize_mxfp4_rows(*quantize_mxfp4_rows(p.float())).to(p.dtype))


@pytest.fixture(scope="module")
def mx_models(dev):
    from livecc_amd.config import tiny
    from livecc_amd.modeling import LiveCCForConditionalGeneration
    from oracle import hf_oracle as O
    cfg = tiny()
    hf32 = O.build_hf_model(cfg, dtype=torch.float32, seed=3, init_scale=2.0)
    _fake_quantize_llm_mxfp4(hf32)
    hf16 = O.build_hf_model(cfg, dtype=torch.float32, seed=3, init_scale=2.0)
    _fake_quantize_llm_mxfp4(hf16)
    hf16.to(torch.bfloat16)
    native = LiveCCForConditionalGeneration.from_hf_model(hf32, cfg, dev, llm_weights="mxfp4", max_streams=3, max_kv_len=2048, max_new_rows=1024,
                                                          max_patches=4096, max_history=32)
    return cfg, hf16, hf32, native


def test_streaming_generate_mxfp4_llm_weights_matches_oracle(dev, mx_models):
    """Three streaming turns of one stream: rms error against the fp32 truth on the same quantised values <= 1.05 x the bf16 oracle's own (the
    project's bound), with the decode steps on the pipeline-v2 GEMVs (launch counter slot 5), not on the fallback sequence."""
    from livecc_amd import ops, protocol
    from tests.test_gpu_e2e import _compare_stream, _replay_native
    cfg, hf16, hf32, native = mx_models
    assert native.weights.llm_weights == "mxfp4" and not native.weights.llm_fp8
    assert native.weights.view("llm.0.qkv_w").dtype == torch.uint8 and native.weights.view("llm.0.qkv_w.scale").dtype == torch.uint8
    frames = torch.from_numpy(protocol.synth_frames(10, 56, 84, seed=77, layout="TCHW"))
    before = ops.launch_counts()["dgemv_v2"]
    turns = _replay_native(native, cfg, frames, protocol.TurnBuilder(cfg, seed=77), max_new_tokens=8, repetition_penalty=1.05, max_turns=3)
    assert ops.launch_counts()["dgemv_v2"] > before, "decode did not take the pipeline-v2 GEMVs"
    _compare_stream(cfg, hf16, hf32, turns, frames, "stream_tiny_mxfp4_weights", 1.05)


def test_three_co_scheduled_streams_match_their_batch_1_runs(dev, mx_models):
    """3 streams in one call = the skinny sequence on gemv_wq_kernel; each stream, teacher-forced to its own batch-1 tokens, reproduces the logits of
    its batch-1 run (pipeline v2) up to the fp32 summation order -- the bound of the existing batched-vs-alone comparison (tests/test_gpu_e2e.py)."""
    from livecc_amd import ops, protocol
    cfg, _, _, native = mx_models
    ids = protocol.TurnBuilder(cfg, seed=21).turn_ids(0, protocol.num_video_tokens(protocol.grid_of(6, 56, 84, cfg), cfg))
    clips = [torch.from_numpy(protocol.synth_frames(6, 56, 84, seed=s, layout="TCHW")) for s in (21, 22, 23)]
    alone = []
    for f in clips:
        r = native.generate(input_ids=torch.from_numpy(ids).view(1, -1), frames=f, max_new_tokens=6, min_new_tokens=6, output_logits=True)
        alone.append((r.sequences[0, len(ids):].tolist(), r.logits.float().cpu()))
        r.past_key_values.release()
    before = ops.launch_counts()["dgemv_v2"]
    outs = native.generate_batch([dict(input_ids=torch.from_numpy(ids), frames=f) for f in clips], max_new_tokens=6, force_length=True,
                                 output_logits=True, teacher_tokens=[a[0] for a in alone])
    assert ops.launch_counts()["dgemv_v2"] == before, "three streams are not a pipeline-v2 batch"
    for o, (toks, logits) in zip(outs, alone):
        assert o.sequences[0, len(ids):].tolist() == toks
        d = (o.logits.float().cpu() - logits).abs().max().item()
        print(f"mxfp4 batched vs alone: max |dlogit| {d:.4f} of scale {logits.abs().max().item():.3f}")
        assert d <= 6e-2 * logits.abs().max().item(), d
        o.past_key_values.release()


def test_a_bf16_model_reproduces_its_tokens_after_an_mxfp4_model_is_destroyed(dev):
    """No routing state leaks from one weight format to the next."""
    import gc
    from livecc_amd import protocol
    from livecc_amd.config import tiny
    from livecc_amd.modeling import LiveCCForConditionalGeneration
    cfg = tiny()
    ids = protocol.TurnBuilder(cfg, seed=5).turn_ids(0, protocol.num_video_tokens(protocol.grid_of(6, 56, 84, cfg), cfg))
    frames = torch.from_numpy(protocol.synth_frames(6, 56, 84, seed=5, layout="TCHW"))

    def greedy(model):
        r = model.generate(input_ids=torch.from_numpy(ids).view(1, -1), frames=frames, max_new_tokens=8, min_new_tokens=8, output_logits=True)
        out = (r.sequences[0, len(ids):].tolist(), r.logits.clone())
        r.past_key_values.release()
        return out
    kw = dict(max_streams=1, max_kv_len=1024, max_new_rows=512, max_patches=2048, max_history=16)
    bf = LiveCCForConditionalGeneration.from_config(cfg, dev, seed=2, **kw)
    toks, logits = greedy(bf)
    mx = LiveCCForConditionalGeneration.from_config(cfg, dev, seed=2, llm_weights="mxfp4", **kw)
    toks_mx, _ = greedy(mx)
    assert len(toks_mx) == 8
    del mx
    gc.collect()
    toks2, logits2 = greedy(bf)
    assert toks2 == toks and torch.equal(logits2, logits)


def test_seventeen_co_scheduled_streams_take_the_dequantise_route_and_match_batch_1(dev, mx_models):
    """More than 16 rows per decode step: every Linear is dequantised into the scratch and runs the bf16 route, lm_head in vocabulary slices.
    Functional, not fast -- and it must still be the same model: each stream, teacher-forced to its batch-1 tokens, reproduces its batch-1 logits
    within the bound of the batched-vs-alone comparison."""
    from livecc_amd import protocol
    from livecc_amd.modeling import LiveCCForConditionalGeneration
    cfg, _, hf32, _ = mx_models
    native = LiveCCForConditionalGeneration.from_hf_model(hf32, cfg, dev, llm_weights="mxfp4", max_streams=17, max_kv_len=512, max_new_rows=4096,
                                                          max_patches=8192, max_history=8)
    ids = protocol.TurnBuilder(cfg, seed=21).turn_ids(0, protocol.num_video_tokens(protocol.grid_of(2, 56, 84, cfg), cfg))
    clips = [torch.from_numpy(protocol.synth_frames(2, 56, 84, seed=30 + s, layout="TCHW")) for s in range(2)]
    alone = []
    for f in clips:
        r = native.generate(input_ids=torch.from_numpy(ids).view(1, -1), frames=f, max_new_tokens=4, min_new_tokens=4, output_logits=True)
        alone.append((r.sequences[0, len(ids):].tolist(), r.logits.float().cpu()))
        r.past_key_values.release()
    outs = native.generate_batch([dict(input_ids=torch.from_numpy(ids), frames=clips[i % 2]) for i in range(17)], max_new_tokens=4, force_length=True,
                                 output_logits=True, teacher_tokens=[alone[i % 2][0] for i in range(17)])
    for i, o in enumerate(outs):
        toks, logits = alone[i % 2]
        assert o.sequences[0, len(ids):].tolist() == toks
        d = (o.logits.float().cpu() - logits).abs().max().item()
        assert d <= 6e-2 * logits.abs().max().item(), (i, d)
        o.past_key_values.release()

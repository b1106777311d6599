"""CPU tier: the MXFP4 weight format (OCP e2m1 elements, one e8m0 scale per 32 consecutive k of a row) -- the quantisation rule against an
independent restatement, exactness of the dequantised values in bf16, the PACKED4 byte order of include/livecc_amd.h, the weight arena and the
loaders, and the argument validation of the four C-ABI entry points (host logic: no device needed)."""
import ctypes
import json
import math
import struct

import pytest
import torch

from livecc_amd import weights as W
from livecc_amd.config import tiny

GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def _floor_log2_from_bits(x: float) -> int:
    """floor(log2(x)) of a normal fp32 value, read from its exponent field (zero / subnormal values: -127)."""
    return ((struct.unpack("<I", struct.pack("<f", x))[0] >> 23) & 0xFF) - 127


def _rule(w):
    """The rule of the issue, restated as a plain loop over blocks and elements (python floats hold fp32 values and their power-of-two multiples exactly)."""
    N, K = w.shape
    codes, scales = [[0] * K for _ in range(N)], [[0] * (K // 32) for _ in range(N)]
    for n in range(N):
        for b in range(K // 32):
            blk = [float(w[n, b * 32 + i]) for i in range(32)]
            amax = max(abs(v) for v in blk)
            s = 0 if amax == 0.0 else min(120, max(-120, _floor_log2_from_bits(amax) - 2))
            scales[n][b] = s + 127
            for i, v in enumerate(blk):
                a = abs(v) * 2.0 ** -s
                if a >= 6.0:
                    c = 7                                   # saturate
                else:
                    lo = max(j for j in range(8) if GRID[j] <= a)
                    hi = min(lo + 1, 7)
                    dl, dh = a - GRID[lo], GRID[hi] - a
                    c = lo if (dl < dh or hi == lo) else hi if dh < dl else (lo if lo % 2 == 0 else hi)      # tie: the even code
                if v < 0 and c != 0:
                    c |= 8
                codes[n][b * 32 + i] = c
    return torch.tensor(codes, dtype=torch.uint8), torch.tensor(scales, dtype=torch.uint8)


def _hand_made_matrix():
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    below = [math.nextafter(t, 0.0) for t in ties]
    above = [math.nextafter(t, 10.0) for t in ties]
    f32 = lambda v: struct.unpack("<f", struct.pack("<f", v))[0]
    rows = []

    def block(vals, top):       # 32 values whose maximum `top` pins the scale
        v = list(vals) + [0.0] * (31 - len(vals)) + [top]
        assert len(v) == 32
        return v
    # s = 0 (block maximum 4.0 -> [4, 8)): the ties, both signs, and their fp32 neighbours on either side
    near = [f32(t * (1 - 2.0 ** -23)) for t in ties] + [f32(t * (1 + 2.0 ** -23)) for t in ties]
    assert all(a < t < b for a, t, b in zip(below, ties, above))
    rows.append(block(ties + [-t for t in ties] + near, 4.0) + block([-v for v in near] + ties, -4.0) +
                # the same ties scaled by 2^-7 under a block maximum of 4 * 2^-7; a block maximum at 2^n and just below 2^n
                block([t * 2.0 ** -7 for t in ties] + [-t * 2.0 ** -7 for t in ties], 4.0 * 2.0 ** -7) + block([0.3, -0.9, 0.0, -0.0], 8.0))
    rows.append(block([1.0, -3.0, 0.1], f32(8.0 * (1 - 2.0 ** -24))) + block([], 0.0) +                   # just below 2^3; an all-zero block
                block([2.0 ** -125, -(2.0 ** -122), 2.0 ** -127], 2.0 ** -119) +                           # maximum below 2^-118: scale clamp at -120
                block([7.9 * 2.0 ** 120, -(7.0 * 2.0 ** 120), 2.0 ** 119], 2.0 ** 125))                    # scale clamp at +120: 7.9 * 2^s saturates to 6 * 2^s
    rows.append(block([-0.0, 0.0, -0.1, 0.1, -0.2499], 1.0) + block([0.02, -0.013, 0.007], -0.031) +
                block([3.0, 6.0, -6.0, 5.5, -5.5, 4.5, -4.5], 7.0) + block([1e-30, -1e-30], 1e-20))
    return torch.tensor(rows, dtype=torch.float32)


def test_the_quantiser_equals_an_independent_restatement_of_the_rule():
    w = _hand_made_matrix()
    codes, scales = W.quantize_mxfp4_rows(w)
    want_c, want_s = _rule(w)
    assert torch.equal(scales, want_s), (scales, want_s)
    assert torch.equal(codes, want_c), (codes != want_c).nonzero().tolist()
    assert int((codes == 8).sum()) == 0, "negative zero is canonicalised"
    # the listed ties, by value: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4 (row 0, block 0: s = 0)
    dq = W.dequantize_mxfp4_rows(codes, scales)
    assert dq[0, :7].tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0] and dq[0, 7:14].tolist() == [-0.0, -1.0, -1.0, -2.0, -2.0, -4.0, -4.0]
    assert scales[1].tolist() == [127, 127, 7, 247]      # maximum just below 2^3 (s = 0, where 2^3 itself gives s = 1), zero block, both clamps
    assert dq[1, 96].item() == 6.0 * 2.0 ** 120 and dq[1, 97].item() == -6.0 * 2.0 ** 120      # 7.9 * 2^s and -7 * 2^s saturate
    assert scales[0, 3] == 128 and scales[0, 0] == 127                                 # maxima 8.0 and 4.0
    for bad in (float("nan"), float("inf"), -float("inf")):
        w2 = w.clone()
        w2[1, 5] = bad
        with pytest.raises(ValueError):
            W.quantize_mxfp4_rows(w2)


@pytest.mark.parametrize("std", [0.02, 1.0, 1e-4])
def test_dequantised_values_are_exact_in_bf16_and_requantise_to_themselves(std):
    g = torch.Generator().manual_seed(3)
    w = torch.randn(96, 1024, generator=g) * std
    codes, scales = W.quantize_mxfp4_rows(w)
    assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8 and int(codes.max()) <= 15 and scales.shape == (96, 32)
    dq = W.dequantize_mxfp4_rows(codes, scales)
    assert dq.dtype == torch.float32 and torch.equal(dq.to(torch.bfloat16).float(), dq)
    c2, s2 = W.quantize_mxfp4_rows(dq)
    assert torch.equal(c2, codes) and torch.equal(s2, scales)
    c3, s3 = W.quantize_mxfp4_rows(dq.to(torch.bfloat16))
    assert torch.equal(c3, codes) and torch.equal(s3, scales)
    err = (w - dq).view(96, 32, 32).abs().amax(dim=2)
    assert bool((err <= w.view(96, 32, 32).abs().amax(dim=2) / 4).all())


def test_pack_round_trip_and_the_byte_order_of_the_header():
    N, K = 32, 256
    n, k = torch.meshgrid(torch.arange(N), torch.arange(K), indexing="ij")
    codes = ((n * 7 + k * 5 + k // 32) % 16).to(torch.uint8)                    # index-coded: neighbours in n and k differ
    scales = ((n[:, ::32] * 3 + (k[:, ::32] // 32) * 11) % 251).to(torch.uint8)
    p, ps = W.pack_weight_mxfp4(codes), W.pack_scale_mxfp4(scales)
    assert p.shape == (N, K // 2) and ps.shape == (N, K // 32)
    assert torch.equal(W.unpack_weight_mxfp4(p), codes) and torch.equal(W.unpack_scale_mxfp4(ps), scales)
    flat, sflat = p.reshape(-1), ps.reshape(-1)
    for nt in range(N // 16):
        for kb in range(K // 128):
            for g in range(4):
                for row in range(16):
                    lane = g * 16 + row
                    base = ((nt * (K // 128) + kb) * 64 + lane) * 16            # [N/16][K/128][4 g][16 rows][16 bytes]
                    for byte in range(16):
                        k0 = kb * 128 + g * 32 + 2 * byte
                        v = int(flat[base + byte])
                        assert (v & 15, v >> 4) == (int(codes[nt * 16 + row, k0]), int(codes[nt * 16 + row, k0 + 1]))      # lower k: low nibble
                    assert int(sflat[(nt * (K // 128) + kb) * 64 + lane]) == int(scales[nt * 16 + row, kb * 4 + g])        # one byte per lane, lane order


def test_arena_stores_the_quantised_set_as_packed4_bytes_and_scales():
    cfg = tiny()
    from oracle import hf_oracle as O
    hf = O.build_hf_model(cfg, dtype=torch.bfloat16, seed=4)
    a = W.from_hf_model(hf, cfg, "cpu", llm_weights="mxfp4")
    assert a.llm_weights == "mxfp4" and a.llm_fp8 is False
    sd = {W._normalise_hf_key(k): v for k, v in hf.state_dict().items()}
    quantised = W.fp8_weight_names(cfg)
    assert "lm_head" in quantised and "llm.0.qkv_w_dec" in quantised
    for name in quantised:
        N, K = a.offsets[name][2]
        v, s = a.view(name), a.view(name + ".scale")
        assert v.dtype == torch.uint8 and s.dtype == torch.uint8 and v.numel() == N * K // 2 and s.numel() == N * K // 32
        assert v.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 0
        assert name + ".scale" in a.names() and a.is_mxfp4(name)
    assert "llm.0.in_norm.scale" not in a.names() and a.view("embed").dtype == torch.bfloat16

    def dq(t):
        return W.dequantize_mxfp4_rows(*W.quantize_mxfp4_rows(t.float()))
    assert torch.equal(a.logical("llm.0.o_w"), dq(sd["language_model.layers.0.self_attn.o_proj.weight"]))
    assert torch.equal(a.logical("llm.1.down_w"), dq(sd["language_model.layers.1.mlp.down_proj.weight"]))
    assert torch.equal(a.logical("lm_head"), dq(sd["lm_head.weight"] if not cfg.tie_word_embeddings else sd["language_model.embed_tokens.weight"]))
    gu = W.interleave_gate_up(sd["language_model.layers.0.mlp.gate_proj.weight"], sd["language_model.layers.0.mlp.up_proj.weight"])
    assert torch.equal(a.logical("llm.0.gate_up_w"), dq(gu))
    # the decode copy = permuted code rows + permuted scale rows of the same quantisation
    perm = W.qkv_decode_row_permutation(cfg)
    codes = W.unpack_weight_mxfp4(a.view("llm.0.qkv_w"))
    scales = W.unpack_scale_mxfp4(a.view("llm.0.qkv_w.scale"))
    assert torch.equal(W.unpack_weight_mxfp4(a.view("llm.0.qkv_w_dec")), codes[perm])
    assert torch.equal(W.unpack_scale_mxfp4(a.view("llm.0.qkv_w_dec.scale")), scales[perm])
    # fill_random: the same relation, and the values of a quantised weight are on the grid
    r = W.WeightArena(cfg, "cpu", llm_weights="mxfp4").fill_random(1)
    assert torch.equal(r.logical("llm.1.qkv_w_dec"), r.logical("llm.1.qkv_w")[perm])
    d = r.logical("llm.0.down_w")
    assert torch.equal(W.dequantize_mxfp4_rows(*W.quantize_mxfp4_rows(d)), d) and 0.015 < float(d.std()) < 0.025


def test_llm_fp8_still_builds_the_fp8_arena_with_the_same_offsets():
    cfg = tiny()
    old, new, bf = W.WeightArena(cfg, "cpu", llm_fp8=True), W.WeightArena(cfg, "cpu", llm_weights="fp8"), W.WeightArena(cfg, "cpu")
    assert old.llm_fp8 and new.llm_fp8 and old.llm_weights == "fp8" and bf.llm_weights == "bf16" and not bf.llm_fp8
    assert old.offsets == new.offsets and old.numel == new.numel and old.names() == new.names()
    # the layout rule of the fp8 arena, restated: N*K bytes + 4 N bytes of row scales, every entry padded to 256 bytes
    total = 0
    for name, shp in W.weight_shapes(cfg):
        n = math.prod(shp)
        units = n // 2 if name in W.fp8_weight_names(cfg) else n
        assert old.offsets[name] == (total, units, shp), name
        total += (units + 127) // 128 * 128
        if name in W.fp8_weight_names(cfg):
            assert old.offsets[name + ".scale"] == (total, 2 * shp[0], (shp[0],))
            total += (2 * shp[0] + 127) // 128 * 128
    assert total == old.numel
    with pytest.raises(ValueError):
        W.WeightArena(cfg, "cpu", llm_fp8=True, llm_weights="mxfp4")
    with pytest.raises(ValueError):
        W.WeightArena(cfg, "cpu", llm_weights="int4")


def test_from_pretrained_equals_from_hf_model_byte_for_byte(tmp_path):
    from safetensors.torch import save_file
    from oracle import hf_oracle as O
    cfg = tiny()
    hf = O.build_hf_model(cfg, dtype=torch.bfloat16, seed=4)
    sd = {k: v.contiguous() for k, v in hf.state_dict().items()}
    keys = sorted(sd)
    d = tmp_path / "ckpt"
    d.mkdir()
    save_file({k: sd[k] for k in keys[: len(keys) // 2]}, str(d / "model-00001-of-00002.safetensors"))
    save_file({k: sd[k] for k in keys[len(keys) // 2:]}, str(d / "model-00002-of-00002.safetensors"))
    (d / "config.json").write_text(json.dumps(cfg.to_hf().to_dict(), default=str))
    got = W.from_pretrained(str(d), cfg, "cpu", llm_weights="mxfp4")
    ref = W.from_hf_model(hf, cfg, "cpu", llm_weights="mxfp4")
    assert got.llm_weights == "mxfp4" and got.names() == ref.names()
    for name in ref.names():
        assert torch.equal(got.view(name), ref.view(name)), name


def test_the_four_entry_points_validate_before_any_device_work(built_lib):
    """K % 128 / N % 16 -> LCC_ERR_SHAPE, null weight / scale or a missing dq_scratch at M > 16 -> LCC_ERR_ARG, unaligned -> LCC_ERR_ALIGN: refused on
    the host (this tier has no GPU: a call that got past validation would fail differently)."""
    from livecc_amd import _lib
    lib = built_lib
    SHAPE, ARG, ALIGN = -2, -1, -3
    hdr = open(_lib.HEADER_PATH).read()
    for name, val in (("LCC_ERR_ARG", ARG), ("LCC_ERR_SHAPE", SHAPE), ("LCC_ERR_ALIGN", ALIGN)):
        assert f"{name} = {val}" in hdr or f"{name}  = {val}" in hdr or f"{name}={val}" in hdr, name
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    lay = _lib.KvLayout(1, 1, 64, 128)

    def gemm(W4=p, S=p, M=1, N=16, K=128, dq=None, A=p):
        return lib.lcc_gemm_w4_bf16(A, K, W4, S, None, None, 0, p, N, M, N, K, 0, None, 0, dq, None)

    def norm(W4=p, S=p, N=16, K=128):
        return lib.lcc_dgemv_norm_linear_w4(W4, S, p, p, p, 1e-6, None, p, N, 1, N, K, 0, None)

    def resid(W4=p, S=p, N=16, K=128):
        return lib.lcc_dgemv_resid_w4(W4, S, p, K, p, p, 1, N, K, None)

    def qkv(W4=p, S=p, K=128):
        return lib.lcc_dgemv_qkv_rope_w4(W4, S, p, p, p, 1e-6, p, p, p, p, p, p, lay, 0, p, 1, 1, K, None)

    for call in (gemm, norm, resid, qkv):
        assert call(K=192) == SHAPE and b"128" in lib.lcc_last_error()
        assert call(W4=None) == ARG and call(S=None) == ARG
        assert call(W4=p + 8) == ALIGN and call(S=p + 4) == ALIGN
    for call in (gemm, norm, resid):
        assert call(N=24) == SHAPE
    assert gemm(M=17) == ARG and b"dq_scratch" in lib.lcc_last_error()
    assert gemm(M=17, dq=p + 2) == ALIGN and gemm(A=p + 2) == ALIGN

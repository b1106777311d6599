"""Weight arena of the native engine.

All parameters live in ONE flat bf16 HBM arena (plus a tiny fp32 tail for `inv_freq`); every named weight
is a view into it.  That is what makes the multi-GPU start-up a single RCCL broadcast over xGMI
(`distributed.broadcast_weights`) instead of every data-parallel worker re-reading the checkpoint from disk
as the reference does (ref evaluation/livesports3kcc/distributed_generate_livecc.py:46).

Layout decisions (engine names -> shapes):
  vit.patch_embed [E,1176]           Conv3d weight [E,3,2,14,14] flattened (c,t,y,x) = patch feature order
  vit.{i}.qkv_w [3E,E] ...           as HF
  vit.{i}.qkv_w_rope / qkv_b_rope    the same rows in the rotation-pair order (vit_qkv_rope_row_permutation): RoPE + V transpose run in
                                     the projection's epilogue
  llm.{i}.qkv_w [Hq*128+2*Hkv*128, H] q_proj|k_proj|v_proj rows concatenated (one GEMM)
  llm.{i}.gate_up_w [2I, H]          rows interleaved in blocks of 16: [16 gate rows | 16 up rows] so that
                                     the GEMM epilogue holds gate and up of the same column in one lane
  lm_head [V,H]                      tied checkpoints (2B) alias `embed`
HF parameter names follow HF models/qwen2_vl/modeling_qwen2_vl.py (5.x: `model.visual.*`,
`model.language_model.*`; 4.5x checkpoints: `visual.*`, `model.layers.*`) -- both are accepted.
"""
from __future__ import annotations

import re
from typing import Callable, Dict, Iterable, List, Tuple

import torch

from .config import LiveCCConfig


def qkv_decode_row_permutation(cfg: LiveCCConfig) -> torch.Tensor:
    """Row order of the DECODE copy of the fused q|k|v weight (`llm.{i}.qkv_w_dec`): inside every 128-row head, stored row
    j*16 + half*8 + i holds logical row half*64 + j*8 + i, i.e. each 16-row MFMA tile carries 8 channels and their 8 M-RoPE
    rotation partners (d, d + 64) -- the decode GEMV then applies bias + RoPE + KV append from registers (csrc/decode_v2.hip)."""
    heads = cfg.qkv_dim // 128
    j, half, i = torch.meshgrid(torch.arange(8), torch.arange(2), torch.arange(8), indexing="ij")
    inner = (half * 64 + j * 8 + i).reshape(-1)                     # stored position (j, half, i) -> logical channel
    return (torch.arange(heads)[:, None] * 128 + inner[None, :]).reshape(-1)


def vit_qkv_rope_row_permutation(cfg: LiveCCConfig) -> torch.Tensor:
    """Row order of the copy of the vision q|k|v weight / bias whose GEMM epilogue applies the 2-D RoPE and writes V transposed
    (`vit.{i}.qkv_w_rope`, `vit.{i}.qkv_b_rope`; csrc/gemm.hip: vit_qkv_epilogue): stored row -> logical row.  Inside q and inside k
    every 32 stored rows are [16 first-half channels | their 16 rotation partners (+40)], first-half channels enumerated head-major
    (f = head * 40 + c, c < 40), so the two 16-column MFMA tiles of a lane hold (x[c], x[c + 40]) of one head; V rows keep their order."""
    E, hd = cfg.vit_embed_dim, cfg.vit_head_dim
    assert hd == 80 and E % 32 == 0, (E, hd)
    f = torch.arange(E // 2).view(-1, 16)                                    # [E/32 groups, 16]
    first = (f // 40) * 80 + f % 40
    qk = torch.stack([first, first + 40], dim=1).reshape(-1)                 # [E]: 16 first-half | 16 partners | ...
    return torch.cat([qk, E + qk, 2 * E + torch.arange(E)])


def has_vit_rope_copies(cfg: LiveCCConfig) -> bool:
    return cfg.vit_head_dim == 80 and cfg.vit_embed_dim % 32 == 0


def weight_shapes(cfg: LiveCCConfig, decode_copies: bool = True) -> List[Tuple[str, Tuple[int, ...]]]:
    E, H, I = cfg.vit_embed_dim, cfg.hidden_size, cfg.intermediate_size
    M = cfg.vit_mlp_dim
    out: List[Tuple[str, Tuple[int, ...]]] = [("vit.patch_embed", (E, cfg.patch_dim))]
    for i in range(cfg.vit_depth):
        p = f"vit.{i}."
        out += [(p + "ln1_w", (E,)), (p + "ln1_b", (E,)), (p + "qkv_w", (3 * E, E)), (p + "qkv_b", (3 * E,)),
                (p + "proj_w", (E, E)), (p + "proj_b", (E,)), (p + "ln2_w", (E,)), (p + "ln2_b", (E,)),
                (p + "fc1_w", (M, E)), (p + "fc1_b", (M,)), (p + "fc2_w", (E, M)), (p + "fc2_b", (E,))]
        if decode_copies and has_vit_rope_copies(cfg):      # +0.16 GB at 7B: one launch per tower block (RoPE + V transpose in the GEMM epilogue)
            out += [(p + "qkv_w_rope", (3 * E, E)), (p + "qkv_b_rope", (3 * E,))]
    out += [("merger.ln_w", (E,)), ("merger.ln_b", (E,)), ("merger.fc1_w", (4 * E, 4 * E)), ("merger.fc1_b", (4 * E,)),
            ("merger.fc2_w", (H, 4 * E)), ("merger.fc2_b", (H,)), ("embed", (cfg.vocab_size, H))]
    for i in range(cfg.num_hidden_layers):
        p = f"llm.{i}."
        out += [(p + "in_norm", (H,)), (p + "qkv_w", (cfg.qkv_dim, H)), (p + "qkv_b", (cfg.qkv_dim,)),
                (p + "o_w", (H, cfg.q_dim)), (p + "post_norm", (H,)), (p + "gate_up_w", (2 * I, H)),
                (p + "down_w", (H, I))]
        if decode_copies:      # +7 % of a layer's bytes (33 MB of 466 MB at 7B) buys three launches per decode layer
            out += [(p + "qkv_w_dec", (cfg.qkv_dim, H))]
    out += [("final_norm", (H,)), ("lm_head", (cfg.vocab_size, H))]   # tied checkpoints: a packed copy of `embed`
    return out


# matrices kept row-major: the Conv3d-as-GEMM weight (K = 1176 is not a multiple of 32) and the embedding table (gathered by
# row).  Every other 2-D weight is stored PACKED in MFMA fragment order (ops.pack_weight / include/livecc_amd.h) so that
# the weight-streaming decode kernels read linear 1-KB bursts.
ROW_MAJOR = ("vit.patch_embed", "embed")


def pack_weight(w: torch.Tensor) -> torch.Tensor:
    N, K = w.shape
    assert N % 16 == 0 and K % 32 == 0, (N, K)
    return w.view(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().view(N, K)


FP8_MAX = 448.0   # largest finite OCP e4m3 value


def quantize_fp8_rows(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[N,K] float -> (q uint8 [N,K] = OCP e4m3 bit patterns, scale fp32 [N]) with w ~= q * scale[:, None]; per-output-row
    absmax scaling (the row's largest weight maps to +-448), round-to-nearest-even.

    The rule is spelled out in operations that are exact, or correctly rounded, on every device, so a CPU process (the oracle) and the
    GPU arena quantise the same checkpoint to the SAME bytes: scale = fp32(fp64(absmax) / 448) (`tensor / 448.0` in fp32 is a multiply by
    the reciprocal on the GPU and a division on the CPU), x = fp32(fp64(w) / fp64(scale)), then x rounded to its e4m3 grid
    by frexp / ldexp / round-half-even (the devices' own float -> float8 casts disagree on ~0.15 % of the elements: measured,
    tools/probes/fp8_quantiser_cpu_vs_gpu.py) and only then cast, which is exact for a value already on the grid."""
    wf = w.float()
    scale = (wf.abs().amax(dim=1).double() / FP8_MAX).float().clamp_min(1e-12)
    x = (wf.double() / scale.double()[:, None]).float().clamp_(-FP8_MAX, FP8_MAX)
    _, e = torch.frexp(x)                                   # |x| = m * 2^e, m in [0.5, 1): the leading bit is 2^(e-1)
    ulp_exp = (e - 4).clamp_(min=-9)                        # 3 mantissa bits below the leading one; subnormal step 2^-9 below 2^-6
    q = torch.ldexp(torch.round(torch.ldexp(x, -ulp_exp)), ulp_exp).clamp_(-FP8_MAX, FP8_MAX)
    return q.to(torch.float8_e4m3fn).view(torch.uint8), scale


def dequantize_fp8_rows(q_u8: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    return q_u8.view(torch.float8_e4m3fn).float() * scale[:, None].float()


def pack_weight_fp8(q_u8: torch.Tensor) -> torch.Tensor:
    """PACKED8 order of include/livecc_amd.h: [N/16][K/64][4 g][16 rows][16 k] bytes."""
    N, K = q_u8.shape
    assert N % 16 == 0 and K % 64 == 0, (N, K)
    return q_u8.view(N // 16, 16, K // 64, 4, 16).permute(0, 2, 3, 1, 4).contiguous().view(N, K)


def unpack_weight_fp8(p_u8: torch.Tensor) -> torch.Tensor:
    N, K = p_u8.shape
    return p_u8.reshape(N // 16, K // 64, 4, 16, 16).permute(0, 3, 1, 2, 4).reshape(N, K)


# ---- OCP MXFP4: e2m1 elements (grid below, plus a sign bit) in blocks of 32 consecutive k of one row that share one e8m0 scale ----
MXFP4_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
MXFP4_BLOCK = 32


def _pow2_f32(e: torch.Tensor) -> torch.Tensor:
    """2^e as fp32 built from the exponent bits (e in [-126, 127]): no exp2 / ldexp, the same bits on every device."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def quantize_mxfp4_rows(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[N,K] float -> (codes uint8 [N,K], one e2m1 code 0..15 per byte: bit 3 = sign, bits 0-2 = index into MXFP4_GRID;
    scale_e8m0 uint8 [N,K/32] = s + 127) with w ~= sign * grid[code & 7] * 2^s over every block of 32 consecutive k of a row.

    s = clamp(floor(log2(absmax of the block)) - 2, -120, 120): the block maximum lands in [4, 8) and rounds to 4 or 6.  floor(log2) is
    read from the exponent bits of the fp32 value and every step is an integer operation, an exact power-of-two product or a comparison,
    so a CPU process (the oracle) and the GPU arena produce the SAME bytes by construction.  An all-zero block gets s = 0.  The magnitude
    is rounded to the nearest grid value, ties to the even code (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4),
    and saturates at 6 (only a clamped scale can leave more).  -0.0 is canonicalised: code 8 is never produced.  The clamp keeps every
    dequantised value a normal bf16, so dequantize_mxfp4_rows is exact and its `.to(bfloat16)` lossless.  Non-finite weights raise."""
    wf = w.float()
    N, K = wf.shape
    assert K % MXFP4_BLOCK == 0, (N, K)
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_mxfp4_rows: non-finite weight")
    b = wf.reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = b.abs().amax(dim=2).contiguous()
    e = ((amax.view(torch.int32) >> 23) & 0xFF) - 127                     # floor(log2(amax)) of a normal fp32 (zero / subnormal: -127, clamped next)
    s = torch.where(amax == 0, torch.zeros_like(e), (e - 2).clamp(-120, 120))
    a = (b * _pow2_f32(-s)[:, :, None]).abs()                             # exact: a power-of-two factor, |result| < 2^9
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8) + (a >= 1.75).to(torch.uint8) +
            (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8) + (a > 5.0).to(torch.uint8))
    code = code + (((b < 0) & (code != 0)).to(torch.uint8) << 3)
    return code.reshape(N, K), (s + 127).to(torch.uint8)


def dequantize_mxfp4_rows(codes: torch.Tensor, scale_e8m0: torch.Tensor) -> torch.Tensor:
    """(codes [N,K], scale_e8m0 [N,K/32]) -> fp32 [N,K], exact (and exactly representable in bf16)."""
    N, K = codes.shape
    grid = torch.tensor(MXFP4_GRID, dtype=torch.float32, device=codes.device)
    mag = grid[(codes & 7).long()]
    val = torch.where((codes & 8) != 0, -mag, mag).reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    return (val * _pow2_f32(scale_e8m0.to(torch.int32) - 127)[:, :, None]).reshape(N, K)


def pack_weight_mxfp4(codes: torch.Tensor) -> torch.Tensor:
    """PACKED4 order of include/livecc_amd.h: codes [N,K] -> bytes [N,K/2] stored [N/16][K/128][4 g][16 rows][16 bytes]; a byte holds
    two codes, the lower k in the low nibble; the 16 bytes of lane (g, row) are the 32 consecutive k = kb*128 + g*32 .. +31."""
    N, K = codes.shape
    assert N % 16 == 0 and K % 128 == 0, (N, K)
    by = codes[:, 0::2] | (codes[:, 1::2] << 4)
    return by.reshape(N // 16, 16, K // 128, 4, 16).permute(0, 2, 3, 1, 4).contiguous().view(N, K // 2)


def unpack_weight_mxfp4(p_u8: torch.Tensor) -> torch.Tensor:
    N, K2 = p_u8.shape
    by = p_u8.reshape(N // 16, K2 // 64, 4, 16, 16).permute(0, 3, 1, 2, 4).reshape(N, K2)
    return torch.stack([by & 15, by >> 4], dim=2).reshape(N, 2 * K2)


def pack_scale_mxfp4(scale_e8m0: torch.Tensor) -> torch.Tensor:
    """scale bytes [N,K/32] -> [N/16][K/128][4 g][16 rows]: one byte per lane of a PACKED4 fragment, in lane order."""
    N, KB = scale_e8m0.shape
    assert N % 16 == 0 and KB % 4 == 0, (N, KB)
    return scale_e8m0.reshape(N // 16, 16, KB // 4, 4).permute(0, 2, 3, 1).contiguous().view(N, KB)


def unpack_scale_mxfp4(p_u8: torch.Tensor) -> torch.Tensor:
    N, KB = p_u8.shape
    return p_u8.reshape(N // 16, KB // 4, 4, 16).permute(0, 3, 1, 2).reshape(N, KB)


LLM_WEIGHT_FORMATS = ("bf16", "fp8", "mxfp4")


def resolve_llm_weights(llm_weights=None, llm_fp8: bool = False) -> str:
    """The one spelling of the LLM weight format: `llm_weights` ("bf16" | "fp8" | "mxfp4"); llm_fp8=True is the older way to say "fp8"."""
    if llm_weights is None:
        return "fp8" if llm_fp8 else "bf16"
    if llm_weights not in LLM_WEIGHT_FORMATS:
        raise ValueError(f"llm_weights must be one of {LLM_WEIGHT_FORMATS}, got {llm_weights!r}")
    if llm_fp8 and llm_weights != "fp8":
        raise ValueError(f"llm_fp8=True contradicts llm_weights={llm_weights!r}")
    return llm_weights


def fp8_weight_names(cfg: LiveCCConfig) -> List[str]:
    """The LLM Linear weights (q|k|v and its decode copy, o, gate/up, down of every layer, and lm_head) stored quantised when the arena is built
    with llm_weights="fp8" or "mxfp4": one rule for both formats (ViT, embeddings, norms stay bf16)."""
    out = []
    for i in range(cfg.num_hidden_layers):
        out += [f"llm.{i}.qkv_w", f"llm.{i}.qkv_w_dec", f"llm.{i}.o_w", f"llm.{i}.gate_up_w", f"llm.{i}.down_w"]
    return out + ["lm_head"]


def interleave_gate_up(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """[I,H],[I,H] -> [2I,H] with rows [16 gate | 16 up | 16 gate | ...]."""
    I, H = gate.shape
    assert I % 16 == 0
    return torch.stack([gate.view(I // 16, 16, H), up.view(I // 16, 16, H)], dim=1).reshape(2 * I, H)


class WeightArena:
    def __init__(self, cfg: LiveCCConfig, device, llm_fp8: bool = False, llm_weights=None):
        """llm_weights (llm_fp8=True means "fp8"): how the LLM Linear weights + lm_head (fp8_weight_names) are stored.
        "fp8": OCP e4m3 bytes (PACKED8 order) followed by their fp32 row scales (`<name>.scale`) -- 1 byte per parameter instead of 2
        (72B: 73 GB instead of 147 GB; BASELINE configs[4]).
        "mxfp4": OCP MXFP4, e2m1 codes in the PACKED4 order (N*K/2 bytes) followed by the e8m0 block scales (`<name>.scale`, N*K/32 bytes,
        one per 32 consecutive k of a row, packed in lane order) -- 4.25 bits per parameter (72B: about 39 GB)."""
        self.cfg, self.device = cfg, torch.device(device)
        self.llm_weights = resolve_llm_weights(llm_weights, llm_fp8)
        self.llm_fp8 = self.llm_weights == "fp8"
        self.shapes = weight_shapes(cfg, decode_copies=True)           # round 3: the fp8 arena carries the decode copies too (pipeline v2)
        self.fp8 = set(fp8_weight_names(cfg)) if self.llm_fp8 else set()
        self.mx4 = set(fp8_weight_names(cfg)) if self.llm_weights == "mxfp4" else set()
        offs, total = {}, 0          # offsets / sizes in bf16 (2-byte) units
        for name, shp in self.shapes:
            n = 1
            for s in shp:
                n *= s
            if name in self.mx4 and (shp[0] % 16 or shp[1] % 128):
                raise ValueError(f"mxfp4 weights need N % 16 == 0 and K % 128 == 0: {name} is {shp}")
            units = n // 4 if name in self.mx4 else (n // 2 if name in self.fp8 else n)
            offs[name] = (total, units, shp)
            total += (units + 127) // 128 * 128          # keep every weight 256-byte aligned
            if name in self.mx4:
                offs[name + ".scale"] = (total, n // 64, (shp[0], shp[1] // MXFP4_BLOCK))
                total += (n // 64 + 127) // 128 * 128
            if name in self.fp8:
                offs[name + ".scale"] = (total, 2 * shp[0], (shp[0],))
                total += (2 * shp[0] + 127) // 128 * 128
        self.offsets, self.numel = offs, total
        self.flat = torch.empty(total, dtype=torch.bfloat16, device=self.device)
        hd = cfg.head_dim
        # HF Qwen2VLRotaryEmbedding.compute_default_rope_parameters (modeling_qwen2_vl.py:129-146), fp32 on CPU
        self.inv_freq = (1.0 / (cfg.rope_theta ** (torch.arange(0, hd, 2, dtype=torch.float) / hd))).to(self.device)

    def is_fp8(self, name: str) -> bool:
        return name in self.fp8

    def is_mxfp4(self, name: str) -> bool:
        return name in self.mx4

    def view(self, name: str) -> torch.Tensor:
        """Storage view [N,K]-shaped; for packed weights the bytes are in fragment order (use `logical` to read values).
        fp8 weights: uint8 [N,K] in the PACKED8 order; `<name>.scale`: fp32 [N].
        mxfp4 weights: uint8 [N,K/2] in the PACKED4 order; `<name>.scale`: uint8 [N,K/32], e8m0 bytes in lane order (pack_scale_mxfp4)."""
        o, n, shp = self.offsets[name]
        if name.endswith(".scale") and name[:-6] in self.mx4:
            return self.flat[o:o + n].view(torch.uint8).view(*shp)
        if name in self.mx4:
            return self.flat[o:o + n].view(torch.uint8).view(shp[0], shp[1] // 2)
        if name.endswith(".scale"):
            return self.flat[o:o + n].view(torch.float32)
        if name in self.fp8:
            return self.flat[o:o + n].view(torch.uint8).view(*shp)
        return self.flat[o:o + n].view(*shp)

    def is_packed(self, name: str) -> bool:
        return len(self.offsets[name][2]) == 2 and name not in ROW_MAJOR

    def logical(self, name: str) -> torch.Tensor:
        """Row-major [N,K] values of a (possibly packed / fp8) weight (tests / export); fp8 weights come back dequantised (fp32)."""
        v = self.view(name)
        if name in self.fp8:
            return dequantize_fp8_rows(unpack_weight_fp8(v), self.view(name + ".scale"))
        if name in self.mx4:
            return dequantize_mxfp4_rows(unpack_weight_mxfp4(v), unpack_scale_mxfp4(self.view(name + ".scale")))
        if not self.is_packed(name):
            return v
        N, K = v.shape
        return v.reshape(N // 16, K // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(N, K)

    def _store_mxfp4(self, name: str, rows_of: Callable[[int, int], torch.Tensor]) -> None:
        """Quantise + pack an mxfp4 weight in row blocks (rows_of(r0, r1) -> float [r1 - r0, K] on the arena's device): a PACKED4 fragment
        covers 16 whole rows, so blocks of a multiple of 16 rows pack independently and the fp32 staging stays small at 72B shapes."""
        N, K = self.offsets[name][2]
        pv = self.view(name).view(N // 16, K // 128, 4, 16, 16)
        sv = self.view(name + ".scale").view(N // 16, K // 128, 4, 16)
        rows = max(16, (1 << 26) // K // 16 * 16)
        for r0 in range(0, N, rows):
            r1 = min(N, r0 + rows)
            codes, sc = quantize_mxfp4_rows(rows_of(r0, r1))
            pv[r0 // 16:r1 // 16].copy_(pack_weight_mxfp4(codes).view((r1 - r0) // 16, K // 128, 4, 16, 16))
            sv[r0 // 16:r1 // 16].copy_(pack_scale_mxfp4(sc).view((r1 - r0) // 16, K // 128, 4, 16))

    def store(self, name: str, t: torch.Tensor) -> None:
        if name in self.mx4:
            assert tuple(t.shape) == tuple(self.offsets[name][2]), f"{name}: {tuple(t.shape)} vs {self.offsets[name][2]}"
            self._store_mxfp4(name, lambda r0, r1: t[r0:r1].to(self.device))
            return
        v = self.view(name)
        assert tuple(t.shape) == tuple(v.shape), f"{name}: {tuple(t.shape)} vs {tuple(v.shape)}"
        if name in self.fp8:
            q, scale = quantize_fp8_rows(t.to(self.device))
            v.copy_(pack_weight_fp8(q))
            self.view(name + ".scale").copy_(scale)
            return
        t = t.to(self.device, dtype=torch.bfloat16)
        v.copy_(pack_weight(t) if self.is_packed(name) else t)

    def names(self) -> List[str]:
        out = []
        for s in self.shapes:
            out.append(s[0])
            if s[0] in self.fp8 or s[0] in self.mx4:
                out.append(s[0] + ".scale")
        return out

    def nbytes(self) -> int:
        return self.flat.numel() * 2

    # ---- fillers ----
    @torch.no_grad()
    def fill_random(self, seed: int = 0, std: float = 0.02) -> "WeightArena":
        """Random weights generated directly in HBM (no checkpoints offline): N(0, std) matrices, norm weights
        1 + 0.1 N(0,1), biases 0.05 N(0,1).  Throughput is data-independent; used by bench.py at 7B shapes."""
        g = torch.Generator(device=self.device).manual_seed(seed)
        for name, shp in self.shapes:
            v = self.view(name)
            if name in self.mx4 and name.endswith("qkv_w_dec"):
                # block quantisation is per row, so it commutes with the row permutation: permuted code rows + permuted scale rows
                perm = qkv_decode_row_permutation(self.cfg).to(self.device)
                src = name[:-4]
                v.copy_(pack_weight_mxfp4(unpack_weight_mxfp4(self.view(src))[perm].contiguous()))
                self.view(name + ".scale").copy_(pack_scale_mxfp4(unpack_scale_mxfp4(self.view(src + ".scale"))[perm].contiguous()))
            elif name in self.mx4:
                K = shp[1]
                self._store_mxfp4(name, lambda r0, r1: torch.randn((r1 - r0, K), generator=g, device=self.device, dtype=torch.float32).mul_(std))
            elif name in self.fp8 and name.endswith("qkv_w_dec"):
                # row quantisation commutes with the row permutation: the decode copy = permuted fp8 rows + permuted scales
                perm = qkv_decode_row_permutation(self.cfg).to(self.device)
                src = name[:-4]
                v.copy_(pack_weight_fp8(unpack_weight_fp8(self.view(src))[perm].contiguous()))
                self.view(name + ".scale").copy_(self.view(src + ".scale")[perm])
            elif name in self.fp8:   # quantised in row blocks so that the fp32 staging stays below ~1 GB at 72B shapes
                N, K = shp
                rows = max(16, (1 << 27) // K // 16 * 16)
                sc = self.view(name + ".scale")
                pv = v.view(N // 16, K // 64, 4, 16, 16)
                for r0 in range(0, N, rows):
                    r1 = min(N, r0 + rows)
                    q, s_ = quantize_fp8_rows(torch.randn((r1 - r0, K), generator=g, device=self.device, dtype=torch.float32).mul_(std))
                    pv[r0 // 16:r1 // 16].copy_(pack_weight_fp8(q).view((r1 - r0) // 16, K // 64, 4, 16, 16))
                    sc[r0:r1].copy_(s_)
            elif name.endswith("qkv_w_rope"):  # the vision q|k|v weight in the rotation-pair row order
                self.store(name, self.logical(name[:-5])[vit_qkv_rope_row_permutation(self.cfg).to(self.device)])
            elif name.endswith("qkv_b_rope"):
                v.copy_(self.view(name[:-5])[vit_qkv_rope_row_permutation(self.cfg).to(self.device)])
            elif name.endswith("qkv_w_dec"):   # the same matrix as qkv_w, rows permuted (both packed)
                self.store(name, self.logical(name[:-4])[qkv_decode_row_permutation(self.cfg).to(self.device)])
            elif name.endswith("qkv_w"):       # kept logical -> packed so that the decode copy can be derived from it
                self.store(name, torch.randn(shp, generator=g, device=self.device, dtype=torch.float32).mul_(std))
            elif len(shp) >= 2:   # i.i.d. values: the packed order of a random matrix is a random matrix
                v.copy_(torch.randn(shp, generator=g, device=self.device, dtype=torch.float32).mul_(std))
            elif name.endswith("_b"):
                v.copy_(torch.randn(shp, generator=g, device=self.device, dtype=torch.float32).mul_(0.05))
            else:
                v.copy_(1.0 + 0.1 * torch.randn(shp, generator=g, device=self.device, dtype=torch.float32))
        return self

    @torch.no_grad()
    def fill_tiled(self, seed: int = 0, variant: str = "tiled") -> "WeightArena":
        """Seeded synthetic weights that a CPU process can reproduce bit for bit WITHOUT a large RNG run: every HF parameter
        is a window of one seeded 4,194,301-element (prime) bf16 block (`tiled_param`).  bench.py uses it so that the CPU
        reference leg (oracle/cpu_baseline.py, HF model filled by the same function) computes with the SAME weights as the
        MI355X arena and the two can be compared logit by logit at the full 7B shapes."""
        shapes = hf_param_shapes(self.cfg)
        dev = self.device
        return self.load_state_dict(lambda name: synthetic_param(name, shapes, seed, dev, variant))

    @torch.no_grad()
    def load_state_dict(self, sd_get: Callable[[str], torch.Tensor]) -> "WeightArena":
        """Fill from an HF state dict accessor (tensor by HF name; any float dtype; CPU or GPU)."""
        cfg = self.cfg

        put = self.store

        put("vit.patch_embed", sd_get("visual.patch_embed.proj.weight").reshape(cfg.vit_embed_dim, -1))
        for i in range(cfg.vit_depth):
            s, p = f"visual.blocks.{i}.", f"vit.{i}."
            for a, b in (("norm1.weight", "ln1_w"), ("norm1.bias", "ln1_b"), ("attn.qkv.weight", "qkv_w"),
                         ("attn.qkv.bias", "qkv_b"), ("attn.proj.weight", "proj_w"), ("attn.proj.bias", "proj_b"),
                         ("norm2.weight", "ln2_w"), ("norm2.bias", "ln2_b"), ("mlp.fc1.weight", "fc1_w"),
                         ("mlp.fc1.bias", "fc1_b"), ("mlp.fc2.weight", "fc2_w"), ("mlp.fc2.bias", "fc2_b")):
                put(p + b, sd_get(s + a))
            if (p + "qkv_w_rope") in self.offsets:
                perm = vit_qkv_rope_row_permutation(cfg)
                w, bq = sd_get(s + "attn.qkv.weight"), sd_get(s + "attn.qkv.bias")
                put(p + "qkv_w_rope", w[perm.to(w.device)])
                put(p + "qkv_b_rope", bq[perm.to(bq.device)])
        for a, b in (("ln_q.weight", "ln_w"), ("ln_q.bias", "ln_b"), ("mlp.0.weight", "fc1_w"), ("mlp.0.bias", "fc1_b"),
                     ("mlp.2.weight", "fc2_w"), ("mlp.2.bias", "fc2_b")):
            put("merger." + b, sd_get("visual.merger." + a))
        put("embed", sd_get("language_model.embed_tokens.weight"))
        for i in range(cfg.num_hidden_layers):
            s, p = f"language_model.layers.{i}.", f"llm.{i}."
            put(p + "in_norm", sd_get(s + "input_layernorm.weight"))
            qkv = torch.cat([sd_get(s + f"self_attn.{x}_proj.weight") for x in "qkv"], dim=0)
            put(p + "qkv_w", qkv)
            if (p + "qkv_w_dec") in self.offsets:
                put(p + "qkv_w_dec", qkv[qkv_decode_row_permutation(cfg).to(qkv.device)])
            put(p + "qkv_b", torch.cat([sd_get(s + f"self_attn.{x}_proj.bias") for x in "qkv"], dim=0))
            put(p + "o_w", sd_get(s + "self_attn.o_proj.weight"))
            put(p + "post_norm", sd_get(s + "post_attention_layernorm.weight"))
            put(p + "gate_up_w", interleave_gate_up(sd_get(s + "mlp.gate_proj.weight"), sd_get(s + "mlp.up_proj.weight")))
            put(p + "down_w", sd_get(s + "mlp.down_proj.weight"))
        put("final_norm", sd_get("language_model.norm.weight"))
        put("lm_head", sd_get("language_model.embed_tokens.weight") if cfg.tie_word_embeddings else sd_get("lm_head.weight"))
        return self


TILE_PERIOD = 4194301      # prime: gcd with every row length is 1, so no two rows of any weight matrix are equal
_TILE_BLOCKS: Dict[Tuple[int, str], torch.Tensor] = {}


def _tile_block(seed: int, device) -> torch.Tensor:
    key = (int(seed), str(device))
    if key not in _TILE_BLOCKS:
        g = torch.Generator(device="cpu").manual_seed(1000003 * int(seed) + 17)      # CPU generator: identical on every machine
        _TILE_BLOCKS[key] = torch.randn(TILE_PERIOD, generator=g, dtype=torch.float32).to(device)
    return _TILE_BLOCKS[key]


# "decisive" variant of the seeded synthetic model (greedy token identity becomes a hard test): with i.i.d. Gaussian weights the
# top-1/top-2 logit gap (~sigma/4.9 over 152k ids) is the size of bf16's own noise, so "token-id exact under greedy" (BASELINE.json
# north_star) is undecidable on most steps.  Here the embedding table is scaled from 0.02 to sqrt(hidden)/30 (2.0 at LiveCC-7B, 1.3 at
# Qwen2-VL-2B: the current token's embedding then stays a component of the residual stream comparable to the sum of the 2 x n_layers
# layer outputs, whose rms grows like sqrt(hidden) with 0.02-scale weights) and lm_head row v is a scaled copy of embedding row
# (A v + B) mod V: the logit of the ONE id whose row matches the current token's embedding is ~|E|^2 / rms(h) while every other id sees
# a random projection.  Measured with HF on CPU (oracle/cpu_baseline.py --weights decisive:0): top-1 margin 36-60 % of the logit
# scale on every step at 7B and 2B shapes = 10-15 x the bf16 logit noise (~4 % of scale), and the generated sequence walks the
# permutation v -> A^-1 (v - B) instead of being decided by rounding.  The layers still matter: the layer outputs make up more than
# half of the final hidden state's norm.
DECISIVE_A, DECISIVE_B = 48271, 7919


def decisive_embed_scale(hidden_size: int) -> float:
    return round(float(hidden_size) ** 0.5 / 30.0, 2)


def synthetic_param(name: str, shapes: Dict[str, Tuple[int, ...]], seed: int, device, variant: str = "tiled", dtype=torch.bfloat16) -> torch.Tensor:
    """Parameter `name` of the seeded synthetic model, variant "tiled" (i.i.d. N(0, 0.02) matrices) or "decisive" (above)."""
    if variant == "tiled":
        return tiled_param(name, shapes[name], seed, device, dtype)
    if variant != "decisive":
        raise ValueError(f"unknown synthetic weight variant {variant!r}")
    emb_name = "language_model.embed_tokens.weight"
    es = decisive_embed_scale(shapes[emb_name][1])
    if name == emb_name:
        return tiled_param(name, shapes[name], seed, device, dtype, scale=es)
    if name == "lm_head.weight":
        V = shapes[name][0]
        emb = tiled_param(emb_name, shapes[emb_name], seed, device, dtype, scale=es)
        perm = (torch.arange(V, dtype=torch.int64, device=emb.device) * DECISIVE_A + DECISIVE_B) % V
        return (emb[perm].float() * (0.02 / es)).to(dtype)
    return tiled_param(name, shapes[name], seed, device, dtype)


def tiled_param(name: str, shape, seed: int, device, dtype=torch.bfloat16, scale: float = None) -> torch.Tensor:
    """Parameter `name` (normalised HF name: visual.* / language_model.* / lm_head.weight) of the seeded synthetic model:
    flat[i] = f(block[(offset(name) + i) mod TILE_PERIOD]) with f = 0.02 x for matrices, 1 + 0.1 x for norm weights and
    0.05 x for biases (the scales of `fill_random` / HF's initializer_range), rounded to bf16.  Built from slice copies."""
    import zlib
    blk = _tile_block(seed, device)
    n = 1
    for d in shape:
        n *= int(d)
    off = zlib.crc32(name.encode()) % TILE_PERIOD
    if len(shape) >= 2:
        scale, shift = (0.02 if scale is None else float(scale)), 0.0
    elif name.endswith("bias"):
        scale, shift = 0.05, 0.0
    else:
        scale, shift = 0.1, 1.0
    res = torch.empty(n, dtype=dtype, device=device)
    pos = 0
    while pos < n:                      # windows of the block, transformed piecewise (bounded fp32 staging)
        k = min(TILE_PERIOD - off, n - pos)
        seg = blk[off:off + k]
        res[pos:pos + k] = (seg * scale + shift) if shift else (seg * scale)
        pos += k
        off = 0
    return res.view(*[int(d) for d in shape])


def hf_param_shapes(cfg: LiveCCConfig) -> Dict[str, Tuple[int, ...]]:
    """Shapes of the HF `Qwen2VLForConditionalGeneration` parameters under the normalised names `load_state_dict` reads."""
    E, H, I, M = cfg.vit_embed_dim, cfg.hidden_size, cfg.intermediate_size, cfg.vit_mlp_dim
    out: Dict[str, Tuple[int, ...]] = {"visual.patch_embed.proj.weight": (E, cfg.in_channels, cfg.temporal_patch_size, cfg.patch_size, cfg.patch_size)}
    for i in range(cfg.vit_depth):
        p = f"visual.blocks.{i}."
        out.update({p + "norm1.weight": (E,), p + "norm1.bias": (E,), p + "attn.qkv.weight": (3 * E, E), p + "attn.qkv.bias": (3 * E,),
                    p + "attn.proj.weight": (E, E), p + "attn.proj.bias": (E,), p + "norm2.weight": (E,), p + "norm2.bias": (E,),
                    p + "mlp.fc1.weight": (M, E), p + "mlp.fc1.bias": (M,), p + "mlp.fc2.weight": (E, M), p + "mlp.fc2.bias": (E,)})
    out.update({"visual.merger.ln_q.weight": (E,), "visual.merger.ln_q.bias": (E,), "visual.merger.mlp.0.weight": (4 * E, 4 * E),
                "visual.merger.mlp.0.bias": (4 * E,), "visual.merger.mlp.2.weight": (H, 4 * E), "visual.merger.mlp.2.bias": (H,),
                "language_model.embed_tokens.weight": (cfg.vocab_size, H)})
    for i in range(cfg.num_hidden_layers):
        p = f"language_model.layers.{i}."
        out.update({p + "input_layernorm.weight": (H,), p + "post_attention_layernorm.weight": (H,),
                    p + "self_attn.q_proj.weight": (cfg.q_dim, H), p + "self_attn.q_proj.bias": (cfg.q_dim,),
                    p + "self_attn.k_proj.weight": (cfg.kv_dim, H), p + "self_attn.k_proj.bias": (cfg.kv_dim,),
                    p + "self_attn.v_proj.weight": (cfg.kv_dim, H), p + "self_attn.v_proj.bias": (cfg.kv_dim,),
                    p + "self_attn.o_proj.weight": (H, cfg.q_dim), p + "mlp.gate_proj.weight": (I, H), p + "mlp.up_proj.weight": (I, H),
                    p + "mlp.down_proj.weight": (H, I)})
    out["language_model.norm.weight"] = (H,)
    if not cfg.tie_word_embeddings:
        out["lm_head.weight"] = (cfg.vocab_size, H)
    return out


def fill_hf_model_tiled(hf_model, cfg: LiveCCConfig, seed: int = 0, variant: str = "tiled") -> None:
    """Fill an instantiated (possibly `to_empty`) HF model with the weights of `WeightArena.fill_tiled(seed)` -- used by the CPU
    reference leg of bench.py and by the full-shape parity tests (test infrastructure calls this; the product never does)."""
    shapes = hf_param_shapes(cfg)
    with torch.no_grad():
        for k, p_ in hf_model.named_parameters():
            name = _normalise_hf_key(k)
            if name not in shapes:
                raise KeyError(f"unexpected HF parameter {k}")
            assert tuple(p_.shape) == tuple(shapes[name]), (k, tuple(p_.shape), shapes[name])
            p_.copy_(synthetic_param(name, shapes, seed, p_.device, variant).to(p_.dtype))


def _normalise_hf_key(k: str) -> str:
    """Map 5.x and 4.5x parameter names onto one scheme: visual.* / language_model.* / lm_head.weight."""
    k = re.sub(r"^model\.visual\.", "visual.", k)
    k = re.sub(r"^model\.language_model\.", "language_model.", k)
    k = re.sub(r"^model\.(layers|embed_tokens|norm)\.", r"language_model.\1.", k)
    return k


def from_hf_model(hf_model, cfg: LiveCCConfig, device, llm_fp8: bool = False, llm_weights=None) -> WeightArena:
    sd = {_normalise_hf_key(k): v for k, v in hf_model.state_dict().items()}
    return WeightArena(cfg, device, llm_fp8=llm_fp8, llm_weights=llm_weights).load_state_dict(lambda n: sd[n])


def from_pretrained(path: str, cfg: LiveCCConfig, device, llm_fp8: bool = False, llm_weights=None) -> WeightArena:
    """safetensors checkpoint directory -> arena (what `from_pretrained` does at ref demo/infer.py:43-47)."""
    import glob
    import os
    from safetensors import safe_open
    index: Dict[str, Tuple[str, str]] = {}
    files = sorted(glob.glob(os.path.join(path, "*.safetensors")))
    if not files:
        raise FileNotFoundError(f"no *.safetensors under {path}")
    handles = {f: safe_open(f, framework="pt", device="cpu") for f in files}
    for f, h in handles.items():
        for k in h.keys():
            index[_normalise_hf_key(k)] = (f, k)

    def get(name):
        if name not in index:
            raise KeyError(f"{name} missing from checkpoint {path}")
        f, k = index[name]
        return handles[f].get_tensor(k)

    return WeightArena(cfg, device, llm_fp8=llm_fp8, llm_weights=llm_weights).load_state_dict(get)

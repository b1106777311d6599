"""-m gpu: exact tests of the vision tower's rope / V^T staging kernel and of the ViT attention kernels' key selection.
  (a) lcc_vit_rope_vt_bf16 rotates q and k to HF's bits (apply_rotary_pos_emb_vision run on the CPU, and a three-line fp32 restatement of
      it: separate fp32 products, no contraction, one rounding to bf16) and leaves the V third alone;
  (b) its V^T staging is a pure permutation into [head][32-key block][80][32] that writes nothing else: every other element of a
      sentinel-filled buffer, pads and a guard plane included, keeps the sentinel;
  (c) needle segments at head dim 80 (tests/attn_exact.py: vit_needle_inputs): every query finds its own key, through every attention
      variant and group size, with poison in the pad columns of V^T (64.0, and -64.0 in a second pass: see _needles) and forbidden twins
      on the segment edges;
  (d) the counting inputs (q = k = 0) with poisoned pads: a pad let in shows in the numerator as well as in the denominator;
  (e) vit_attention's defaults equal the two stages called separately.
The grids give segments of 24, 36, 64, 64, 130 and 300 keys (P = 618): under one block; a block + 4, after which every segment starts at 4
mod 8 (the ragged V path, V groups and query groups that straddle two segments); exact blocks; one 128-row group + 2 rows; several groups
and a last V group cut by the end of P.  (10 x 13 is a segment length, not a frame: tests/attn_exact.py, vit_rope_tables_for.)  The comparators are proven on the CPU in tests/test_attn_exact_ref.py."""
import pytest
import torch

from tests import attn_exact as X
from tests.util import record

pytestmark = pytest.mark.gpu

GRIDS = X.VIT_GRIDS
SEG_LENS = X.vit_seg_lens(GRIDS)
P = sum(SEG_LENS)
DV = X.D_VIT
# After the 36-key segment every V group of 8 patches starts at 4 mod 8 of its segment: GRIDS runs the register-transpose path of the
# V^T staging on 7 groups, all in a segment's first block.  These segments (64, 64, 140 keys; P = 268) start at 0 mod 8: the aligned path in
# every block of a segment, and a last group that the end of P cuts.  Used by the rope / V^T tests only.
ALIGNED_GRIDS = [(2, 8, 8), (1, 10, 14)]
ROPE_CASES = [pytest.param(GRIDS, 2, id="heads2"), pytest.param(GRIDS, 3, id="heads3"), pytest.param(GRIDS, 16, id="heads16"),
              pytest.param(ALIGNED_GRIDS, 3, id="aligned_heads3")]
SENTINEL = 0x7B5A          # a bf16 bit pattern (~1.1e36) that no staged V holds
_WORST = {}
_CACHE = {}


def _note(family, worst):
    """worst observed deviation of a family (in units of its tolerance), kept in the parity report"""
    _WORST[family] = max(_WORST.get(family, 0.0), worst)
    record(f"vit_exact/{family}", dict(worst_deviation_in_tolerances=_WORST[family]))


@pytest.fixture(params=[0, 1, 2, 3], ids=["attn_per_wave", "attn_prefill_shared", "attn_lds_shared_default", "attn_prefill_mfma32"])
def attn_variant(request):
    from livecc_amd import ops
    ops.set_attn_variant(request.param)
    yield request.param
    ops.set_attn_variant(ops.ATTN_DEFAULT_VARIANT)


def _group_rows(attn_variant):
    return (256, 128) if attn_variant == 3 else (256,)


def _tables(grids=GRIDS):
    from livecc_amd.config import tiny
    key = ("tables", tuple(grids))
    if key not in _CACHE:
        _CACHE[key] = X.vit_rope_tables_for(grids, tiny())
    return _CACHE[key]


def _rope_inputs(heads, n_patches=P):
    g = torch.Generator().manual_seed(40 + heads)
    return (torch.randn(n_patches, 3 * heads * DV, generator=g) * 1.5).to(torch.bfloat16)


def _rope_run(dev, grids, heads):
    """One ops.vit_rope_vt call per case, shared by (a) and (b): (qkv before, qkv after, vt after as int16 bits, blocks), all on the
    CPU.  vt goes in filled with the sentinel and one block plane longer than the kernel may touch."""
    from livecc_amd import ops
    key = ("rope", tuple(grids), heads)
    if key not in _CACHE:
        assert SEG_LENS == [24, 36, 64, 64, 130, 300] and P == 618
        seg_lens = X.vit_seg_lens(grids)
        cos, sin = _tables(grids)
        qkv0 = _rope_inputs(heads, sum(seg_lens))
        blocks = sum((n + 31) // 32 for n in seg_lens)
        vt = torch.full(((heads * blocks + 1) * DV * 32,), SENTINEL, dtype=torch.int16).view(torch.bfloat16).to(dev)
        qkv = qkv0.clone().to(dev)
        got = ops.vit_rope_vt(qkv, cos.to(dev), sin.to(dev), grids, heads, vt=vt)
        assert got.data_ptr() == vt.data_ptr(), "the caller's buffer is the one that is staged and returned"
        torch.cuda.synchronize()
        _CACHE[key] = (qkv0, qkv.cpu(), vt.cpu().view(torch.int16), blocks)
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) rope
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grids,heads", ROPE_CASES)
def test_rope_is_hfs_arithmetic_bit_for_bit(dev, grids, heads):
    from transformers.models.qwen2_vl.modeling_qwen2_vl import apply_rotary_pos_emb_vision
    E = heads * DV
    cos, sin = _tables(grids)
    qkv0, qkv1, _, _ = _rope_run(dev, grids, heads)
    P = qkv0.shape[0]
    q0, k0, v0 = [x.reshape(P, heads, DV) for x in qkv0.split(E, dim=1)]
    q1, k1, v1 = [x.reshape(P, heads, DV) for x in qkv1.split(E, dim=1)]
    hf_q, hf_k = apply_rotary_pos_emb_vision(q0, k0, torch.cat([cos, cos], -1), torch.cat([sin, sin], -1))
    assert hf_q.dtype == torch.bfloat16 and hf_q.shape == q0.shape

    def restated(x, dtype):
        x1, x2 = x[..., :40].to(dtype), x[..., 40:].to(dtype)
        c, s = cos[:, None, :].to(dtype), sin[:, None, :].to(dtype)
        return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)     # separate products, then one add / subtract: no FMA on the CPU

    my_q, my_k = restated(q0, torch.float32).to(torch.bfloat16), restated(k0, torch.float32).to(torch.bfloat16)
    assert torch.equal(my_q, hf_q) and torch.equal(my_k, hf_k), "the fp32 restatement is HF's function (CPU against CPU)"
    n64 = 0
    for got, x in ((q1, q0), (k1, k0)):
        n64 += int((got != restated(x, torch.float64).to(torch.float32).to(torch.bfloat16)).sum())
    record(f"vit_exact/rope_vs_fp64_rounded_once[P{P},heads{heads}]", dict(mismatches=n64, elements=2 * P * E))
    for name, got, want in (("q", q1, hf_q), ("k", k1, hf_k)):
        bad = (got != want).nonzero()
        assert bad.numel() == 0, (f"{name}: {bad.shape[0]} of {got.numel()} elements differ from HF; first (patch, head, channel) = "
                                  f"{bad[:8].tolist()}")
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{name}: bit pattern (signed zeros)"
    assert torch.equal(v1.view(torch.int16), v0.view(torch.int16)), "the V third of qkv is left alone"


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) V^T staging
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grids,heads", ROPE_CASES)
def test_vt_staging_is_a_pure_permutation_and_writes_nothing_else(dev, grids, heads):
    E = heads * DV
    qkv0, _, vt, blocks = _rope_run(dev, grids, heads)
    seg_lens = X.vit_seg_lens(grids)
    P = sum(seg_lens)
    v_bits = qkv0[:, 2 * E:].reshape(P, heads, DV).contiguous().view(torch.int16)
    assert int((v_bits == SENTINEL).sum()) == 0, "the sentinel is not a value of V"
    want = X.vit_vt(v_bits, seg_lens, SENTINEL, guard_blocks=1)
    assert want.numel() == vt.numel() == (heads * blocks + 1) * DV * 32
    if not torch.equal(vt, want):
        idx, _ = X.vit_vt_index(seg_lens, heads)
        placed = vt[idx.reshape(-1)].reshape(P, heads, DV) != v_bits
        rest = torch.ones(vt.numel(), dtype=torch.bool)
        rest[idx.reshape(-1)] = False
        over = (rest & (vt != SENTINEL)).nonzero().flatten()
        pytest.fail(f"V^T: {int(placed.sum())} keys' elements misplaced, first (patch, head, channel) = {placed.nonzero()[:8].tolist()}; "
                    f"{over.numel()} pad / guard elements overwritten, first flat offsets = {over[:8].tolist()} "
                    f"(guard starts at {heads * blocks * DV * 32})")


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) needles
# ---------------------------------------------------------------------------------------------------------------------------------
def _needles(dev, heads):
    """inputs + fp64 reference, built once per head count and left unchanged: qkv [P, 3E] already 'rotated' (rope=False), vt staged on the
    CPU by plain indexing with POISON_V in the pad columns"""
    key = ("needle", heads)
    if key not in _CACHE:
        c = X.vit_needle_inputs(SEG_LENS, heads, seed=17 + heads)
        E = heads * DV
        c["qkv"] = torch.cat([c["q"].reshape(P, E), c["k"].reshape(P, E), c["v"].reshape(P, E)], dim=1).contiguous().to(dev)
        # pad columns: 64.0, and -64.0 in a second copy -- the last key of a segment with a successor is a twin (V = 64.0), and a +64 pad
        # under that key's K (the row a kernel may clamp its pads' K to) would change nothing
        c["vt"] = {fill: X.vit_vt(c["v"], SEG_LENS, fill).to(dev) for fill in (X.POISON_V, -X.POISON_V)}
        _CACHE[key] = c
    return _CACHE[key]


@pytest.mark.parametrize("heads", [2, 16])
def test_every_query_finds_its_own_key_and_nothing_outside_its_segment(dev, heads, attn_variant):
    from livecc_amd import ops
    c = _needles(dev, heads)
    qkv0, vt0 = c["qkv"].clone(), {f: t.clone() for f, t in c["vt"].items()}
    outs = []
    for group_rows, fill in [(g, f) for f in c["vt"] for g in _group_rows(attn_variant)]:
        before = ops.launch_counts()["attn_vit32"]
        got = ops.vit_attention(c["qkv"], None, None, GRIDS, heads, group_rows=group_rows, vt=c["vt"][fill], rope=False)
        assert ops.launch_counts()["attn_vit32"] == before + (1 if attn_variant == 3 else 0)
        outs.append(got)
        got = got.view(P, heads, DV).cpu()
        ok, worst = X.check_needle(got, c["ref"], c["gaps"], c["vmax"], DV)
        print(f"vit needles[heads {heads}, variant {attn_variant}, group_rows {group_rows}, pads {fill}]: worst deviation {worst:.3f} tolerances, "
              f"worst 1 - w {float(c['gaps'].max()):.3g}")
        _note(f"vit_needle[group_rows{group_rows}]" if attn_variant == 3 else "vit_needle", worst)
        if not ok:
            exp = X.bf16_round(c["ref"])
            tol = torch.maximum(X.bf16_ulp(exp), X.needle_atol(c["gaps"], c["vmax"]).expand_as(exp))
            bad = ((got.double() - exp).abs() > tol).any(-1).nonzero()
            pytest.fail(f"vit_attention[heads {heads}, variant {attn_variant}, group_rows {group_rows}, pads {fill}]: off by {worst:.2f} tolerances; "
                        f"{bad.shape[0]} (patch, head) rows wrong, first {bad[:8].tolist()}; segments start at {c['starts']}")
    assert torch.equal(c["qkv"], qkv0) and all(torch.equal(c["vt"][f], vt0[f]) for f in vt0), "rope=False reads qkv and vt, it writes neither"
    for other in outs[1:]:
        assert torch.equal(outs[0], other), "a query row's arithmetic depends neither on the group size nor on what the pads hold"


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) counting, pads poisoned
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [2, 16])
def test_vit_attention_counts_every_key_of_its_segment_once_with_poisoned_pads(dev, heads, attn_variant):
    """q = k = 0, V one-hot in channel local % 40 of the lower half for even segments and of the upper half for odd ones: bf16(c_d / len) in
    the segment's half, EXACT zeros in the other.  The pad columns of V^T hold 64.0: a pad let in adds 64 / (len + 1) to every channel."""
    from livecc_amd import ops
    E = heads * DV
    vv = torch.zeros(P, heads, DV)
    exp = torch.zeros(P, heads, DV, dtype=torch.float64)
    off = 0
    for sg, n in enumerate(SEG_LENS):
        half = (sg % 2) * 40
        local = torch.arange(n)
        vv[off + local, :, half + local % 40] = 1.0
        exp[off:off + n, :, half:half + 40] = X.counting_expected(n, 0, 40)
        off += n
    vv = vv.to(torch.bfloat16)
    qkv = torch.zeros(P, 3 * E, dtype=torch.bfloat16)
    qkv[:, 2 * E:] = vv.view(P, E)
    qkv = qkv.to(dev)
    vt = X.vit_vt(vv, SEG_LENS, X.POISON_V).to(dev)
    assert int((vt == X.POISON_V).sum()) == heads * DV * sum(-n % 32 for n in SEG_LENS)
    for group_rows in _group_rows(attn_variant):
        got = ops.vit_attention(qkv, None, None, GRIDS, heads, group_rows=group_rows, vt=vt, rope=False)
        ok, worst = X.deviation(got.view(P, heads, DV), exp)
        _note("vit_counting_poisoned_pads", worst)
        assert ok, f"vit_attention[heads {heads}, variant {attn_variant}, group_rows {group_rows}]: off by {worst:.2f} ulp"


# ---------------------------------------------------------------------------------------------------------------------------------
# (e) the two stages are the one call
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [2, 16])
def test_rope_true_and_the_two_stages_agree(dev, heads):
    from livecc_amd import ops
    cos, sin = [t.to(dev) for t in _tables()]
    qkv0 = _rope_inputs(heads).to(dev)
    one_qkv = qkv0.clone()
    one = ops.vit_attention(one_qkv, cos, sin, GRIDS, heads)
    two_qkv = qkv0.clone()
    vt = ops.vit_rope_vt(two_qkv, cos, sin, GRIDS, heads)
    blocks = sum((n + 31) // 32 for n in SEG_LENS)
    assert vt.shape == (heads * blocks * DV * 32,) and vt.dtype == torch.bfloat16
    staged = two_qkv.clone()
    two = ops.vit_attention(two_qkv, None, None, GRIDS, heads, vt=vt, rope=False)
    assert torch.equal(two_qkv, staged), "rope=False does not rotate again"
    assert torch.equal(one_qkv, two_qkv), "both forms leave the same rotated qkv"
    assert torch.isfinite(one.float()).all() and torch.equal(one, two)
    given = torch.zeros_like(vt)
    three = ops.vit_attention(qkv0.clone(), cos, sin, GRIDS, heads, vt=given)
    assert torch.equal(three, one) and torch.equal(given, vt), "a caller's vt is the buffer that is staged"
    with pytest.raises(ValueError):
        ops.vit_attention(qkv0.clone(), cos, sin, GRIDS, heads, rope=False)
    with pytest.raises(ValueError):
        ops.vit_rope_vt(qkv0.clone(), cos, sin, GRIDS, heads, vt=vt[:-1])

"""-m gpu: key-exact tests of the attention kernels -- masks, key splits, tile boundaries, the by-value decode path, multi-stream prefill
and ViT segment isolation -- on the structured inputs of tests/attn_exact.py, whose expected outputs are derived (not measured) and whose
comparators are proven on the CPU to reject one dropped / duplicated / leaked key (tests/test_attn_exact_ref.py).  Tolerances: 1 bf16 ulp
for counting inputs, max(1 ulp, (1 - w) max|V| + 2^-20) for needles."""
import pytest
import torch

from tests import attn_exact as X
from tests.util import record

pytestmark = pytest.mark.gpu

D = 128
HEADS = [(7, 1), (28, 4), (2, 1)]
LAYER = 1
_WORST = {}


def _note(family, worst):
    """worst observed deviation of a family (in units of its tolerance), kept in the parity report"""
    _WORST[family] = max(_WORST.get(family, 0.0), worst)
    record(f"attn_exact/{family}", dict(worst_deviation_in_tolerances=_WORST[family]))


@pytest.fixture(params=[0, 1, 2, 3], ids=["attn_per_wave", "attn_prefill_shared", "attn_lds_shared_default", "attn_prefill_mfma32"])
def attn_variant(request):
    from livecc_amd import ops
    ops.set_attn_variant(request.param)
    yield request.param
    ops.set_attn_variant(ops.ATTN_DEFAULT_VARIANT)


def _rot(slot):
    return 5 * slot          # per-slot channel rotation of the counting rows: another stream's arena gives another answer


# ---------------------------------------------------------------------------------------------------------------------------------
# decode, counting
# ---------------------------------------------------------------------------------------------------------------------------------
LENS = [0, 31, 32, 33, 500, 991]          # cached keys per stream before the new token
SLOTS = [3, 0, 5, 1, 6, 2]                # batch row -> slot (a permutation; slot 4 stays unused: all poison)
LMAX = 1024
NSPLITS = [1, 2, 3, 8, 16, 33]            # 33 > the tile count of every stream: empty splits, m = -inf records
_ARENAS = {}


def _decode_arena(dev, Hkv):
    """(arena with every stream's n = cached + 1 counting rows, the same arena before the new token's append) -- built once per KV head
    count and never written by a test (the fused test works on a copy)."""
    from livecc_amd import ops
    if Hkv not in _ARENAS:
        after, before = ops.KvArena(7, 2, Hkv, LMAX, dev), ops.KvArena(7, 2, Hkv, LMAX, dev)
        for slot in range(7):
            n = LENS[SLOTS.index(slot)] + 1 if slot in SLOTS else 0
            k, v = X.counting_arena(n, LMAX, Hkv, _rot(slot), seed=slot)
            if n:
                k[:, n - 1] = 0.0                      # the new token's K as the fused kernel appends it from zero slabs
            X.write_arena(after, slot, LAYER, k, v)
            if n:
                k[:, n - 1] = 7.0
                v[:, n - 1] = X.POISON_V
            X.write_arena(before, slot, LAYER, k, v)
        _ARENAS[Hkv] = (after, before)
    return _ARENAS[Hkv]


def _decode_state(dev):
    slots = torch.tensor(SLOTS, dtype=torch.int32, device=dev)
    kv_len = torch.zeros(7, dtype=torch.int32, device=dev)
    kv_len[slots.long()] = torch.tensor(LENS, dtype=torch.int32, device=dev)
    return slots, kv_len


def _check_decode_counting(out, Hq, rows, family, what):
    for i, b in enumerate(rows):
        ok, worst = X.check_counting(out[i].view(Hq, D), LENS[b] + 1, _rot(SLOTS[b]))
        _note(family, worst)
        assert ok, f"{what}: stream {b} ({LENS[b]} cached keys, slot {SLOTS[b]}) off by {worst:.2f} ulp"


@pytest.mark.parametrize("nsplit", NSPLITS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_decode_counts_every_key_once(dev, Hq, Hkv, nsplit):
    """attn_decode, B = 6 on permuted slots, index path: every head of stream b gives bf16(c_d / n_b) within 1 ulp."""
    from livecc_amd import ops
    kv, _ = _decode_arena(dev, Hkv)
    slots, kv_len = _decode_state(dev)
    q = torch.zeros(len(LENS), Hq * D, dtype=torch.bfloat16, device=dev)
    out = ops.attn_decode(q, kv, LAYER, slots, kv_len, Hq, nsplit)
    _check_decode_counting(out, Hq, range(len(LENS)), "decode_counting", f"attn_decode[Hq{Hq},nsplit{nsplit}]")


@pytest.mark.parametrize("nsplit", NSPLITS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_decode_by_value_is_bit_identical_to_the_index_path(dev, Hq, Hkv, nsplit):
    """The DIRECT instantiation (arena pointers and key counts as kernel arguments), batches of <= 4: the same bits as the index path and
    the counting check on its own.  The device-side kv_len handed to the by-value call is all zeros: only a kernel that takes its counts
    from the arguments can pass."""
    from livecc_amd import ops
    kv, _ = _decode_arena(dev, Hkv)
    slots, kv_len = _decode_state(dev)
    q = torch.zeros(len(LENS), Hq * D, dtype=torch.bfloat16, device=dev)
    ref = ops.attn_decode(q, kv, LAYER, slots, kv_len, Hq, nsplit)
    for rows in ([0, 1, 2, 3], [4, 5], [5, 2, 0]):
        sl = slots[rows].contiguous()
        got = ops.attn_decode(q[rows].contiguous(), kv, LAYER, sl, torch.zeros_like(kv_len), Hq, nsplit, direct_n=[LENS[b] + 1 for b in rows])
        _check_decode_counting(got, Hq, rows, "decode_counting_by_value", f"attn_decode direct[Hq{Hq},nsplit{nsplit}]")
        assert torch.equal(got, ref[rows]), f"by-value and index decode differ (rows {rows}, nsplit {nsplit})"


def test_decode_by_value_refuses_more_than_four_streams_and_counts_outside_the_arena(dev):
    from livecc_amd import _lib, ops
    kv, _ = _decode_arena(dev, 1)
    slots, kv_len = _decode_state(dev)
    q = torch.zeros(len(LENS), 7 * D, dtype=torch.bfloat16, device=dev)
    with pytest.raises(_lib.LccError, match="1..4 streams"):
        ops.attn_decode(q[:5].contiguous(), kv, LAYER, slots[:5].contiguous(), kv_len, 7, 2, direct_n=[1] * 5)
    for bad in (0, LMAX + 1):
        with pytest.raises(_lib.LccError):
            ops.attn_decode(q[:1].contiguous(), kv, LAYER, slots[:1].contiguous(), kv_len, 7, 2, direct_n=[bad])


@pytest.mark.parametrize("nsplit", NSPLITS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_fused_decode_counts_every_key_once_and_appends_what_it_was_fed(dev, Hq, Hkv, nsplit):
    """attn_decode_fused with zero q / k slabs and zero bias (RoPE of 0 is 0); the v part of the slab is the new key's one-hot row.  The
    new key must be counted (it is appended by the same launch) and the arena afterwards is exactly the fed rows, nothing else touched."""
    from livecc_amd import ops
    after, before = _decode_arena(dev, Hkv)
    kv = ops.KvArena(7, 2, Hkv, LMAX, dev)
    kv.buf.copy_(before.buf)
    slots, kv_len = _decode_state(dev)
    B, qkv_dim = len(LENS), (Hq + 2 * Hkv) * D
    part = torch.zeros(1, B, Hq + 2 * Hkv, D, dtype=torch.float32)
    for b in range(B):
        part[0, b, Hq + Hkv:, (LENS[b] + _rot(SLOTS[b])) % D] = 1.0
    part = part.view(1, B, qkv_dim).to(dev)
    bias = torch.zeros(qkv_dim, dtype=torch.bfloat16, device=dev)
    cos = torch.full((B, 64), 0.75, dtype=torch.bfloat16, device=dev)
    sin = torch.full((B, 64), 0.5, dtype=torch.bfloat16, device=dev)
    got, counters = ops.attn_decode_fused(part, bias, cos, sin, kv, LAYER, slots, kv_len, Hq, nsplit)
    assert int(counters.abs().sum()) == 0, "arrival counters must be left at zero"
    assert torch.equal(kv.buf, after.buf), "the appended K / V rows are not bit-exact to what was fed (or another row was written)"
    _check_decode_counting(got, Hq, range(B), "decode_fused_counting", f"attn_decode_fused[Hq{Hq},nsplit{nsplit}]")


# ---------------------------------------------------------------------------------------------------------------------------------
# the fused attention + o_proj launch, counting
# ---------------------------------------------------------------------------------------------------------------------------------
def _nsplit(n_keys):
    """The engine's rule (lcc_llm_decode): 4 key tiles of 32 keys per split, at most 64 splits."""
    return max(1, min(64, ((n_keys + 31) // 32 + 3) // 4))


@pytest.mark.parametrize("Hq,Hkv,H,lens", [(7, 1, 896, (4095,)), (7, 1, 896, (4096, 4000)), (28, 4, 3584, (500, 260))],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_attn_o_launch_counts_every_key_once(dev, request, Hq, Hkv, H, lens):
    """lcc_dgemv_attn_o (attn_o_kernel): the returned attention rows against the derived counts -- an independent reference where
    test_gpu_attn_o_fused.py has attn_decode -- through the index path and by value (device kv_len zeroed), bit-identical to each other.
    4096 cached keys are n = 4097: channel 0 holds 33 keys, one key more or less is still 1 / 33 = 3 % = 3.9 ulps at the least."""
    from livecc_amd import _lib, ops
    from tests.test_gpu_ops import _rand
    lens, M = list(lens), len(lens)
    lmax = (max(lens) + 1 + 31) // 32 * 32 + 32                  # room for a poison row behind the longest stream
    nsplit = _nsplit(max(lens) + 1)
    assert M * Hkv * nsplit + H // 16 <= torch.cuda.get_device_properties(dev).multi_processor_count, "case does not fit one block per CU"
    old_mode = _lib.load().lcc_debug_set_resid_waves(0)
    request.addfinalizer(lambda: _lib.load().lcc_debug_set_resid_waves(old_mode))
    kv = ops.KvArena(M, 2, Hkv, lmax, dev)
    slots = torch.arange(M, dtype=torch.int32, device=dev).flip(0).contiguous()           # row m -> slot M-1-m
    slot_of = [M - 1 - m for m in range(M)]
    for m in range(M):
        X.write_arena(kv, slot_of[m], LAYER, *X.counting_arena(lens[m] + 1, lmax, Hkv, _rot(slot_of[m]), seed=m))
    kv_len = torch.zeros(M, dtype=torch.int32, device=dev)
    kv_len[slots.long()] = torch.tensor(lens, dtype=torch.int32, device=dev)
    K = Hq * D
    w_o = ops.pack_weight(_rand((H, K), dev, 0.03, 51))
    q, h0 = torch.zeros(M, K, dtype=torch.bfloat16, device=dev), _rand((M, H), dev, 2.0, 200)
    tickets, counter, err = (torch.zeros(256, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                             torch.zeros(1, dtype=torch.int32, device=dev))
    ops.launch_counts(reset=True)
    outs = []
    for i, (kl, direct_n) in enumerate(((kv_len, None), (torch.zeros_like(kv_len), [n + 1 for n in lens]))):
        h = h0.clone()
        attn, _ = ops.dgemv_attn_o_(q, kv, LAYER, slots, kl, Hq, nsplit, w_o, h, tickets, counter, i * M * Hkv, err, direct_n=direct_n)
        assert int(err[0]) == 0 and int(counter[0]) == (i + 1) * M * Hkv
        for m in range(M):
            ok, worst = X.check_counting(attn[m].view(Hq, D), lens[m] + 1, _rot(slot_of[m]))
            _note("attn_o_counting", worst)
            assert ok, f"{'by value' if direct_n else 'index'}: stream {m} ({lens[m]} cached keys) off by {worst:.2f} ulp"
        outs.append((attn, h))
    assert ops.launch_counts()["attn_o_fused"] == 2
    assert int(tickets.abs().sum()) == 0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "by-value and index launches differ"


# ---------------------------------------------------------------------------------------------------------------------------------
# decode, needle, long caches
# ---------------------------------------------------------------------------------------------------------------------------------
NEEDLE_HQ, NEEDLE_HKV, NEEDLE_LMAX = 28, 4, 32768


def _decode_needles(n):
    """one needle per query head: the first keys, both sides of a tile boundary, both sides of a split boundary of the 16- and the 64-split
    launch, the last two keys, the rest spread over the middle; dealt so that every KV head gets a mix"""
    ntile = (n + 31) // 32
    b16, b64 = 5 * ((ntile + 15) // 16) * 32, 37 * ((ntile + 63) // 64) * 32
    fixed = [0, 31, 32, b16 - 1, b16, b64 - 1, b64, n - 2, n - 1]
    assert max(b16, b64) < n - 2 and len(set(fixed)) == len(fixed)
    mid = [(i + 1) * n // 21 + 7 for i in range(NEEDLE_HQ - len(fixed))]
    pos = fixed + mid
    assert len(set(pos)) == NEEDLE_HQ and all(0 <= p < n for p in pos)
    return [pos[(h * 11) % NEEDLE_HQ] for h in range(NEEDLE_HQ)]


@pytest.fixture(scope="module", params=[4096, 32736], ids=lambda n: f"n{n}")
def long_needles(request, dev):
    """arena, q and the fp64 reference of one cache length, computed once and shared by every split count"""
    from livecc_amd import ops
    n, G = request.param, NEEDLE_HQ // NEEDLE_HKV
    needles = _decode_needles(n)
    k, v = X.needle_kv(n, NEEDLE_LMAX, NEEDLE_HKV, seed=n)
    for hk in range(NEEDLE_HKV):
        X.plant_twin(k, v, hk, n, needles[hk * G])          # the forbidden twin at index n (of the group's first head)
    q = X.needle_q(k, needles, G)
    ref, gaps, vmax = X.needle_reference(q, k, v, [h // G for h in range(NEEDLE_HQ)], [n] * NEEDLE_HQ, needles)
    kv = ops.KvArena(1, 1, NEEDLE_HKV, NEEDLE_LMAX, dev)
    X.write_arena(kv, 0, 0, k, v)
    return n, kv, q.view(1, NEEDLE_HQ * D).to(dev), ref, gaps, vmax


@pytest.mark.parametrize("nsplit", [1, 16, 64])
def test_decode_finds_the_needle_in_a_long_cache_and_never_its_twin(dev, long_needles, nsplit):
    from livecc_amd import ops
    n, kv, q, ref, gaps, vmax = long_needles
    slots = torch.zeros(1, dtype=torch.int32, device=dev)
    kv_len = torch.tensor([n - 1], dtype=torch.int32, device=dev)
    got = ops.attn_decode(q, kv, 0, slots, kv_len, NEEDLE_HQ, nsplit)
    ok, worst = X.check_needle(got.view(NEEDLE_HQ, D), ref, gaps, vmax)
    _note("decode_needle", worst)
    assert ok, f"attn_decode[n{n},nsplit{nsplit}]: {worst:.3g} x the tolerance"
    by_value = ops.attn_decode(q, kv, 0, slots, torch.zeros_like(kv_len), NEEDLE_HQ, nsplit, direct_n=[n])
    ok, worst = X.check_needle(by_value.view(NEEDLE_HQ, D), ref, gaps, vmax)
    _note("decode_needle_by_value", worst)
    assert ok, f"attn_decode direct[n{n},nsplit{nsplit}]: {worst:.3g} x the tolerance"
    assert torch.equal(by_value, got)


# ---------------------------------------------------------------------------------------------------------------------------------
# prefill
# ---------------------------------------------------------------------------------------------------------------------------------
def _tilings(Hq, Hkv):
    """(tile_rows, nsplit) of the random-input prefill test, with the engine's own tile height under variant 3"""
    from livecc_amd import ops
    tall = ops.attn_tile_rows(Hq, Hkv)
    return ((32, 1), (16, 1), (16, 3), (32, 2)) + (((tall, 1), (tall, 2)) if tall > 32 else ())


def _prefill_counting_expected(segments, Hq):
    rows = []
    for slot, n_new, past in segments:
        rows += [X.counting_expected(past + i + 1, _rot(slot)) for i in range(n_new)]
    return torch.stack(rows).unsqueeze(1).expand(len(rows), Hq, D)


def _prefill_counting_arena(dev, segments, Hkv, lmax):
    from livecc_amd import ops
    kv = ops.KvArena(max(s for s, _, _ in segments) + 1, 2, Hkv, lmax, dev)
    for slot in range(kv.buf.shape[0]):
        valid = max([past + n_new for s, n_new, past in segments if s == slot] or [0])
        X.write_arena(kv, slot, LAYER, *X.counting_arena(valid, lmax, Hkv, _rot(slot), seed=slot))
    return kv


MULTI = [(2, 1, 0), (0, 37, 100), (1, 70, 31), (3, 32, 0)]          # (slot, new rows, cached keys): ragged, partial tiles mid-table


@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_multi_stream_prefill_counts_every_key_once_and_equals_per_stream_launches(dev, Hq, Hkv, attn_variant):
    """One tile table over four ragged streams (what lcc_llm_prefill builds): row i of a stream = bf16(c_d / (past + i + 1)), and the launch is
    bit-identical, row for row, to four single-segment launches -- a tile's arithmetic does not depend on its index in the table."""
    from livecc_amd import ops
    kv = _prefill_counting_arena(dev, MULTI, Hkv, 256)
    S = sum(n for _, n, _ in MULTI)
    q = torch.zeros(S, Hq * D, dtype=torch.bfloat16, device=dev)
    exp = _prefill_counting_expected(MULTI, Hq)
    for tr, ns in _tilings(Hq, Hkv):
        got = ops.attn_prefill(q, kv, LAYER, MULTI, Hq, tile_rows=tr, nsplit=ns)
        ok, worst = X.deviation(got.view(S, Hq, D), exp)
        _note("prefill_counting_multi_stream", worst)
        assert ok, f"attn_prefill multi-stream[Hq{Hq},rows{tr},split{ns}]: off by {worst:.2f} ulp"
        row = 0
        for seg in MULTI:
            one = ops.attn_prefill(q[row:row + seg[1]].contiguous(), kv, LAYER, [seg], Hq, tile_rows=tr, nsplit=ns)
            assert torch.equal(one, got[row:row + seg[1]]), f"stream {seg} alone differs from its rows of the shared table (rows{tr},split{ns})"
            row += seg[1]


@pytest.mark.parametrize("past", [0, 70, 1000])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_prefill_counts_every_key_once(dev, Hq, Hkv, past, attn_variant):
    from livecc_amd import ops
    S = 70
    seg = [(0, S, past)]
    kv = _prefill_counting_arena(dev, seg, Hkv, (past + S + 1 + 31) // 32 * 32)
    q = torch.zeros(S, Hq * D, dtype=torch.bfloat16, device=dev)
    exp = _prefill_counting_expected(seg, Hq)
    for tr, ns in _tilings(Hq, Hkv):
        got = ops.attn_prefill(q, kv, LAYER, seg, Hq, tile_rows=tr, nsplit=ns)
        ok, worst = X.deviation(got.view(S, Hq, D), exp)
        _note("prefill_counting", worst)
        assert ok, f"attn_prefill[Hq{Hq},past{past},rows{tr},split{ns}]: off by {worst:.2f} ulp"


ROW_SETS = ([0, 16, 32, 36, 69], [15, 31, 35, 67])          # pairwise non-adjacent: a row's twin sits where the next row's key is
_PREFILL_NEEDLES = {}


def _prefill_needle_case(Hq, Hkv, past, which):
    """K, V, q and the fp64 reference of one row set (independent of the kernel variant: computed once).  Every tested row r looks for its
    own diagonal key past + r -- the last valid one -- and its twin sits at past + r + 1, the first invalid one."""
    key = (Hq, Hkv, past, which)
    if key not in _PREFILL_NEEDLES:
        S, G, rows = 70, Hq // Hkv, ROW_SETS[which]
        lmax = (past + S + 1 + 31) // 32 * 32
        k, v = X.needle_kv(past + S, lmax, Hkv, seed=100 * past + 10 * Hq + which)
        for r in rows:
            for hk in range(Hkv):
                X.plant_twin(k, v, hk, past + r + 1, past + r)
        g = torch.Generator().manual_seed(7 + which)
        q = (torch.randn(S, Hq, D, generator=g) * 0.5).to(torch.bfloat16)          # the untested rows: ordinary queries
        for r in rows:
            q[r] = X.needle_q(k, [past + r] * Hq, G)
        qt = q[rows].reshape(len(rows) * Hq, D)
        heads = [h // G for _ in rows for h in range(Hq)]
        nk = [past + r + 1 for r in rows for _ in range(Hq)]
        ref, gaps, vmax = X.needle_reference(qt, k, v, heads, nk, [n - 1 for n in nk])
        _PREFILL_NEEDLES[key] = (k, v, lmax, q.view(S, Hq * D), ref, gaps, vmax)
    return _PREFILL_NEEDLES[key]


@pytest.mark.parametrize("past", [0, 33, 1000])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_prefill_finds_the_diagonal_needle_and_never_the_key_behind_it(dev, Hq, Hkv, past, attn_variant):
    """Both sides of the causal mask at once: the needle is the row's last valid key, its twin (same K, V = 64) the first masked one."""
    from livecc_amd import ops
    S = 70
    for which, rows in enumerate(ROW_SETS):
        k, v, lmax, q, ref, gaps, vmax = _prefill_needle_case(Hq, Hkv, past, which)
        kv = ops.KvArena(1, 2, Hkv, lmax, dev)
        X.write_arena(kv, 0, LAYER, k, v)
        qd = q.to(dev)
        for tr, ns in _tilings(Hq, Hkv):
            got = ops.attn_prefill(qd, kv, LAYER, [(0, S, past)], Hq, tile_rows=tr, nsplit=ns)
            ok, worst = X.check_needle(got.view(S, Hq, D)[rows].reshape(-1, D), ref, gaps, vmax)
            _note("prefill_needle", worst)
            assert ok, f"attn_prefill[Hq{Hq},past{past},rows{tr},split{ns}] row set {rows}: {worst:.3g} x the tolerance"


# ---------------------------------------------------------------------------------------------------------------------------------
# ViT: segment isolation
# ---------------------------------------------------------------------------------------------------------------------------------
VIT_GRIDS = [(2, 4, 8), (1, 6, 6), (3, 8, 8), (1, 4, 6)]          # segments of 32, 32, 36, 64, 64, 64, 24 keys


def test_vit_attention_stays_inside_its_segment(dev, attn_variant):
    """q = k = 0, V one-hot in channel local % 40 for even segments and 40 + local % 40 for odd ones: bf16(c_d / seg_len) in the segment's
    half, EXACT zeros in the other.  A pad key let in (36 = a block + 4 keys and 28 pads; 24 = 8 pads) shows in the denominator, a key of
    the neighbouring segment in the wrong half."""
    from livecc_amd import ops
    heads, Dv = 2, 80
    E = heads * Dv
    seg_lens = [h * w for t, h, w in VIT_GRIDS for _ in range(t)]
    assert seg_lens == [32, 32, 36, 64, 64, 64, 24]
    P = sum(seg_lens)
    vv = torch.zeros(P, heads, Dv)
    exp = torch.zeros(P, heads, Dv, dtype=torch.float64)
    off = 0
    for sg, n in enumerate(seg_lens):
        half = (sg % 2) * 40
        local = torch.arange(n)
        vv[off + local, :, half + local % 40] = 1.0
        exp[off:off + n, :, half:half + 40] = X.counting_expected(n, 0, 40)
        off += n
    qkv = torch.zeros(P, 3 * E)
    qkv[:, 2 * E:] = vv.view(P, E)
    qkv = qkv.to(torch.bfloat16).to(dev)
    cos = torch.full((P, 40), 0.8, dtype=torch.float32, device=dev)
    sin = torch.full((P, 40), 0.6, dtype=torch.float32, device=dev)
    for group_rows in ((256, 128) if attn_variant == 3 else (256,)):
        got = ops.vit_attention(qkv.clone(), cos, sin, VIT_GRIDS, heads, group_rows=group_rows)
        ok, worst = X.deviation(got.view(P, heads, Dv), exp)
        _note("vit_counting", worst)
        assert ok, f"vit_attention[variant {attn_variant}, group_rows {group_rows}]: off by {worst:.2f} ulp"

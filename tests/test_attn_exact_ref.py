"""Sensitivity proof of tests/attn_exact.py (no GPU, no kernel): each comparator is fed the plain fp64 reference, rounded to bf16 as a
kernel's output would be, once unmutated (must be accepted) and once with one of the mistakes attention kernels make (must be rejected):
  (a) one key removed, (b) one key counted twice, (c) the key at index n (the first invalid one) admitted, (d) the causal limit off by +-1,
at the boundary positions 0, 31, 32, n-1 and on both sides of a key-split boundary.  This is how the GPU tests of
tests/test_gpu_attn_exact.py are shown to fail on a subtly wrong kernel without ever breaking one."""
import pytest
import torch

from tests import attn_exact as X

D = X.D


def _as_kernel_output(ref64):
    return ref64.to(torch.float32).to(torch.bfloat16)


def _split_boundary(n, nsplit):
    """first key of split 1 as the decode kernels cut the range: ceil(ceil(n / 32) / nsplit) tiles of 32 keys per split"""
    ntile = (n + 31) // 32
    return (ntile + nsplit - 1) // nsplit * 32


def _positions(n, nsplit):
    b = _split_boundary(n, nsplit)
    return sorted({p for p in (0, 31, 32, n - 1, b - 1, b, b + 1) if 0 <= p < n})


# ---------------------------------------------------------------------------------------------------------------------------------
# the number-format helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_one_ulp_is_accepted_two_are_rejected_and_an_expected_zero_is_exact():
    ref = torch.tensor([1.0, 0.75, 2.0 ** -8, 0.0, 33.0 / 4097.0], dtype=torch.float64)
    exp = X.bf16_round(ref)
    ulp = X.bf16_ulp(exp)
    assert ulp[0] == 2.0 ** -7 and ulp[1] == 2.0 ** -8 and ulp[2] == 2.0 ** -15 and ulp[3] == 0.0
    assert X.deviation(exp.to(torch.bfloat16), ref) == (True, 0.0)
    for i in range(len(ref)):
        for sign in (1.0, -1.0):
            one, two = exp.clone(), exp.clone()
            one[i] += sign * ulp[i]
            two[i] += sign * 2 * ulp[i]
            if ulp[i] > 0:
                assert X.deviation(one, ref)[0], (i, sign)
                assert not X.deviation(two, ref)[0], (i, sign)
    tiny = exp.clone(); tiny[3] = 2.0 ** -30
    assert not X.deviation(tiny, ref)[0], "a value where an exact zero is expected"
    nan = exp.clone(); nan[0] = float("nan")
    assert not X.deviation(nan, ref)[0]


def test_blocked_v_layout_is_what_the_arena_view_gathers():
    from livecc_amd import ops
    hkv, lmax = 2, 96
    kv = ops.KvArena(2, 2, hkv, lmax, torch.device("cpu"))
    g = torch.Generator().manual_seed(3)
    k = torch.randn(hkv, lmax, D, generator=g).to(torch.bfloat16)
    v = torch.randn(hkv, lmax, D, generator=g).to(torch.bfloat16)
    X.write_arena(kv, 1, 1, k, v)
    assert torch.equal(kv.k_view(1, 1), k) and torch.equal(kv.v_view(1, 1), v)
    assert int((kv.buf[0] != 0).sum()) == 0 and int((kv.k_view(1, 0) != 0).sum()) == 0, "other slots / layers are left alone"
    # element (key j, channel d) of a head at (j // 32) * 128 * 32 + d * 32 + j % 32
    flat = X.v_blocked(v[0])
    for j, d in ((0, 0), (31, 127), (32, 5), (95, 64)):
        assert flat[(j // 32) * D * 32 + d * 32 + j % 32] == v[0, j, d]


# ---------------------------------------------------------------------------------------------------------------------------------
# counting family
# ---------------------------------------------------------------------------------------------------------------------------------
def _counting_rows(n, lmax, rot):
    k, v = X.counting_arena(n, lmax, 1, rot, seed=n)
    return torch.zeros(D, dtype=torch.bfloat16), k[0], v[0]


COUNTING_CASES = [(1, 1, 0), (32, 2, 0), (33, 2, 5), (34, 3, 0), (501, 8, 10), (992, 3, 15), (4096, 16, 0), (4097, 33, 5)]


@pytest.mark.parametrize("n,nsplit,rot", COUNTING_CASES)
def test_counting_accepts_the_reference_and_rejects_every_one_key_mistake(n, nsplit, rot):
    lmax = (n + 1 + 31) // 32 * 32
    q, k, v = _counting_rows(n, lmax, rot)
    clean, w = X.softmax_rows(q, k, v, range(n))
    assert torch.equal(w, torch.full((n,), 1.0 / n, dtype=torch.float64)), "q = 0: every key weighs 1 / n"
    assert torch.allclose(clean, X.counting_expected(n, rot), rtol=1e-12, atol=0), "the derived value is the softmax reference"
    ok, worst = X.check_counting(_as_kernel_output(clean), n, rot)
    assert ok and worst == 0.0
    keys = list(range(n))
    for p in _positions(n, nsplit):
        if n == 1:          # attention over one key is that key's V however often it is counted, and without it there is no output at all
            continue
        out, _ = X.softmax_rows(q, k, v, keys[:p] + keys[p + 1:])                      # (a) key p missing
        assert not X.check_counting(_as_kernel_output(out), n, rot)[0], f"key {p} of {n} removed"
        out, _ = X.softmax_rows(q, k, v, keys[:p] + [p] + keys[p:])                    # (b) key p twice
        assert not X.check_counting(_as_kernel_output(out), n, rot)[0], f"key {p} of {n} duplicated"
    out, _ = X.softmax_rows(q, k, v, keys + [n])                                       # (c) the poison row at index n let in
    assert not X.check_counting(_as_kernel_output(out), n, rot)[0], f"key {n} (invalid) admitted"


@pytest.mark.parametrize("past,row,S", [(0, 0, 70), (0, 15, 70), (0, 31, 70), (0, 32, 70), (33, 35, 70), (70, 36, 70), (1000, 69, 70), (100, 36, 37),
                                        (31, 0, 70), (0, 31, 32)])
def test_counting_rejects_a_causal_limit_off_by_one(past, row, S):
    """prefill: the arena holds past + S valid keys, row r attends to past + r + 1 of them.  Limit + 1 admits the next row's key (a valid
    one-hot row, or the poison behind the last row); limit - 1 drops the diagonal."""
    n_valid, n = past + S, past + row + 1
    lmax = (n_valid + 1 + 31) // 32 * 32
    q, k, v = _counting_rows(n_valid, lmax, 0)
    clean, _ = X.softmax_rows(q, k, v, range(n))
    assert X.check_counting(_as_kernel_output(clean), n)[0]
    out, _ = X.softmax_rows(q, k, v, range(n + 1))
    assert not X.check_counting(_as_kernel_output(out), n)[0], "limit + 1"
    if n > 1:
        out, _ = X.softmax_rows(q, k, v, range(n - 1))
        assert not X.check_counting(_as_kernel_output(out), n)[0], "limit - 1"


@pytest.mark.parametrize("seg_len", [24, 32, 36, 64])
def test_vit_counting_rejects_a_pad_key_and_a_neighbours_key(seg_len):
    """ViT segments (head dim 80, q = k = 0): V one-hot in channel local % 40 of one half; the other half is exactly zero.  A pad key (V = 0)
    shows up in the denominator, a neighbour's key in the other half."""
    for half in (0, 1):
        exp = torch.zeros(80, dtype=torch.float64)
        exp[half * 40:half * 40 + 40] = X.counting_expected(seg_len, 0, 40)
        assert X.deviation(_as_kernel_output(exp), exp) == (True, 0.0)
        pad = exp * seg_len / (seg_len + 1)                       # one pad key in the denominator
        assert not X.deviation(_as_kernel_output(pad), exp)[0]
        nb = exp * seg_len / (seg_len + 1)                        # one key of the neighbouring segment (the other half)
        nb[(1 - half) * 40] = 1.0 / (seg_len + 1)
        assert not X.deviation(_as_kernel_output(nb), exp)[0]
        nb_only = exp.clone(); nb_only[(1 - half) * 40 + 7] = 2.0 ** -20
        assert not X.deviation(_as_kernel_output(nb_only), exp)[0], "anything at all in the other half"


# ---------------------------------------------------------------------------------------------------------------------------------
# needle family
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(1000, 8), (4096, 16), (32736, 64)], ids=lambda p: f"n{p[0]}")
def needle_case(request):
    n, nsplit = request.param
    lmax = (n + 1 + 31) // 32 * 32
    k, v = X.needle_kv(n, lmax, 1, seed=11 + n)
    return n, nsplit, k, v


def test_needle_accepts_the_reference_and_rejects_a_lost_needle_the_twin_and_a_shifted_limit(needle_case):
    n, nsplit, k0, v0 = needle_case
    for p in _positions(n, nsplit):
        k, v = k0.clone(), v0.clone()
        X.plant_twin(k, v, 0, n, p)
        q = X.needle_q(k, [p], 1)
        ref, gaps, vmax = X.needle_reference(q, k, v, [0], [n], [p])
        assert float(gaps[0]) <= 2.0 ** -12
        ok, worst = X.check_needle(_as_kernel_output(ref), ref, gaps, vmax)
        assert ok and worst == 0.0
        keys = list(range(n))
        out, _ = X.softmax_rows(q[0], k[0], v[0], keys[:p] + keys[p + 1:])             # (a) the needle itself missing
        assert not X.check_needle(_as_kernel_output(out)[None], ref, gaps, vmax)[0], f"needle {p} of {n} removed"
        out, _ = X.softmax_rows(q[0], k[0], v[0], keys + [n])                          # (c) / (d, +1) the twin at index n let in
        assert not X.check_needle(_as_kernel_output(out)[None], ref, gaps, vmax)[0], f"twin of needle {p} admitted"
        assert float((out - ref[0]).abs().max()) > 25.0, "the twin pulls the output half-way to 64"
        if p == n - 1:                                                                 # (d, -1) the limit one short: the diagonal key is gone
            out, _ = X.softmax_rows(q[0], k[0], v[0], keys[:-1])
            assert not X.check_needle(_as_kernel_output(out)[None], ref, gaps, vmax)[0], "limit - 1"


def test_a_key_counted_twice_is_the_counting_familys_to_find(needle_case):
    """(b) on needle inputs: a duplicated needle doubles numerator and denominator alike and a duplicated bystander weighs nothing, so the
    needle comparator cannot see either -- by construction, not by tolerance.  The counting inputs reject a duplicate at every one of these
    positions (test_counting_accepts_the_reference_and_rejects_every_one_key_mistake); the GPU tests run both families."""
    n, nsplit, k, v = needle_case
    p = _split_boundary(n, nsplit)
    q = X.needle_q(k, [p], 1)
    ref, gaps, vmax = X.needle_reference(q, k, v, [0], [n], [p])
    keys = list(range(n))
    out, _ = X.softmax_rows(q[0], k[0], v[0], keys + [p])
    assert X.check_needle(_as_kernel_output(out)[None], ref, gaps, vmax)[0]
    if n <= 4224:
        qc, kc, vc = _counting_rows(n, k.shape[1], 0)
        out, _ = X.softmax_rows(qc, kc, vc, keys + [p])
        assert not X.check_counting(_as_kernel_output(out), n)[0]


def test_needle_tolerance_is_the_derived_one():
    gaps, vmax = torch.tensor([2.0 ** -12, 0.0]), torch.tensor([4.0, 3.0])
    assert torch.equal(X.needle_atol(gaps, vmax), torch.tensor([[2.0 ** -10 + 2.0 ** -20], [2.0 ** -20]], dtype=torch.float64))
    ref = torch.tensor([[1.0, 2.0 ** -22], [0.5, 0.0]], dtype=torch.float64)
    got = X.bf16_round(ref)
    got[1, 1] = 2.0 ** -20                                        # inside the floor
    assert X.check_needle(got, ref, gaps, vmax)[0]
    got[1, 1] = 2.0 ** -19
    assert not X.check_needle(got, ref, gaps, vmax)[0]
    got[1, 1] = 0.0; got[0, 0] = 1.0 + 2.0 ** -6                  # 2 ulps of 1.0 = 2^-6 > 2^-10 + 2^-20
    assert not X.check_needle(got, ref, gaps, vmax)[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# head dim 80: the ViT needle segments (tests/test_gpu_vit_exact.py)
# ---------------------------------------------------------------------------------------------------------------------------------
VIT_GRIDS = X.VIT_GRIDS
DV = X.D_VIT


@pytest.fixture(scope="module")
def vit_case():
    seg_lens = X.vit_seg_lens(VIT_GRIDS)
    assert seg_lens == [24, 36, 64, 64, 130, 300]
    return seg_lens, X.vit_needle_inputs(seg_lens, 2, seed=5)


def _vit_row(c, row, h, keys, k=None, v=None):
    """fp64 attention of query (row, head h) over the global key list `keys`, as [1, 80] for the comparator"""
    k, v = (c["k"] if k is None else k), (c["v"] if v is None else v)
    out, _ = X.softmax_rows(c["q"][row, h], k[:, h], v[:, h], keys, DV)
    return _as_kernel_output(out)[None]


def _vit_check(c, got, row, h):
    return X.check_needle(got, c["ref"][row, h][None], c["gaps"][row, h][None], c["vmax"][row, h][None], DV)[0]


def test_vit_needles_cover_every_key_and_the_twins_sit_on_the_segment_edges(vit_case):
    seg_lens, c = vit_case
    P = sum(seg_lens)
    assert sorted(c["needle"].tolist()) == list(range(P)), "every key is somebody's needle"
    for s0, n in zip(c["starts"], seg_lens):
        assert bool(((c["needle"][s0:s0 + n] >= s0) & (c["needle"][s0:s0 + n] < s0 + n)).all()), "inside its own segment"
    assert len(c["twins"]) == 2 * (len(seg_lens) - 1)
    ends = {s0 for s0 in c["starts"][1:]} | {s0 + n - 1 for s0, n in zip(c["starts"][:-1], seg_lens[:-1])}
    assert {t for t, _ in c["twins"]} == ends
    for t, src in c["twins"]:
        assert torch.equal(c["k"][t], c["k"][src]) and bool((c["v"][t] == X.POISON_V).all()) and src not in ends
    assert float(c["gaps"].max()) <= X.NEEDLE_MIN_WEIGHT_GAP
    ok, worst = X.check_needle(_as_kernel_output(c["ref"]), c["ref"], c["gaps"], c["vmax"], DV)
    assert ok and worst == 0.0, "the comparator accepts the reference"


@pytest.mark.parametrize("seg", [1, 4], ids=["len36", "len130"])
def test_vit_needle_rejects_a_lost_needle_a_neighbours_twin_a_poison_pad_and_a_swapped_vt_order(vit_case, seg):
    seg_lens, c = vit_case
    s0, n = c["starts"][seg], seg_lens[seg]
    keys = list(range(s0, s0 + n))
    needle, P = c["needle"], sum(seg_lens)
    row_of = {int(needle[r]): r for r in keys}                       # key -> the row of this segment that looks for it
    for h in range(2):
        for row in (s0, s0 + 31, s0 + n - 1):
            assert _vit_check(c, _vit_row(c, row, h, keys), row, h)
            j = int(needle[row])
            assert not _vit_check(c, _vit_row(c, row, h, [x for x in keys if x != j]), row, h), f"needle {j} of row {row} lost"
        # the neighbours' twins: K of this segment's middle key, V = 64, planted on the last patch before and the first patch after it
        leaks = [t for t, src in c["twins"] if src == s0 + n // 2]
        assert sorted(leaks) == [s0 - 1, s0 + n], "one twin on either side"
        row = row_of[s0 + n // 2]
        for t in leaks:
            out = _vit_row(c, row, h, keys + [t])
            assert not _vit_check(c, out, row, h), f"twin {t} of the neighbouring segment admitted"
            assert float((out[0].double() - c["ref"][row, h]).abs().max()) > 25.0, "the twin pulls the output half-way to 64"
        # a pad column of the last block: V = the filler under whatever K row the kernel pairs it with (the kernels clamp K to a row of
        # the segment; which one is theirs to choose) -- here the middle key's and the last key's.  The last key of a segment with a
        # successor is a twin, V = 64.0 already: a +64 pad under ITS K changes nothing, which is why the GPU test also runs a -64 filler.
        for fill in (X.POISON_V, -X.POISON_V):
            vp = torch.cat([c["v"], torch.full_like(c["v"][:1], fill)])
            for echoed in (s0 + n // 2, s0 + n - 1):
                kp = torch.cat([c["k"], c["k"][echoed:echoed + 1]])
                row = row_of[echoed]
                seen = not _vit_check(c, _vit_row(c, row, h, keys + [P], kp, vp), row, h)
                hidden = fill == X.POISON_V and bool((c["v"][echoed] == X.POISON_V).all())
                assert seen != hidden, f"a {fill} pad under the K of key {echoed}"
        assert not hidden or echoed in {t for t, _ in c["twins"]}
        lone = _vit_row(c, s0, h, keys + [P], torch.cat([c["k"], torch.zeros_like(c["k"][:1])]), vp)     # K = 0: weight ~ e^-72, unseen --
        assert _vit_check(c, lone, s0, h), "a pad nobody looks for weighs nothing: the counting inputs are the ones that see it"
        # two keys swapped in the vt order: K read in one order, V^T in another
        a, b = s0 + 3, s0 + 35
        vs = c["v"].clone()
        vs[[a, b]] = vs[[b, a]]
        for key in (a, b):
            row = row_of[key]
            assert not _vit_check(c, _vit_row(c, row, h, keys, v=vs), row, h), f"keys {a} and {b} swapped in the V^T order"


def test_vit_vt_layout_is_the_blocked_transpose_per_segment_with_the_filler_in_the_pads():
    seg_lens, heads = [24, 36, 64], 3
    P = sum(seg_lens)
    v = torch.arange(P * heads * DV, dtype=torch.int32).reshape(P, heads, DV)
    buf = X.vit_vt(v, seg_lens, -1, guard_blocks=1)
    blocks = 1 + 2 + 2
    assert buf.numel() == (heads * blocks + 1) * DV * 32
    seg_blk, starts = [0, 1, 3], [0, 24, 60]
    seen = 0
    for sg, n in enumerate(seg_lens):
        for kl in (0, 7, 23, 31, 32, 35, n - 1):
            if kl >= n:
                continue
            for h, d in ((0, 0), (2, 79), (1, 40)):
                assert buf[((h * blocks + seg_blk[sg] + kl // 32) * DV + d) * 32 + kl % 32] == v[starts[sg] + kl, h, d]
                seen += 1
    assert seen > 40
    assert int((buf == -1).sum()) == buf.numel() - P * heads * DV, "V is placed once each, everything else is the filler"
    assert bool((buf[heads * blocks * DV * 32:] == -1).all())


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_weight_gap_fails_at_gain_4_and_holds_at_gain_8_at_head_dim_80(seed):
    """Why NEEDLE_GAIN_VIT exists: 4 |K|^2 / sqrt(80) ~ 36 nats against N(0, 4^2 |K|^2 / 80) scores -- over the 1456 keys of a 28 x 52 frame
    some row's runner-up comes within 8 nats of it."""
    seg_lens = [24, 36, 130, 28 * 52]
    c = X.vit_needle_inputs(seg_lens, 2, seed)
    assert float(c["gaps"].max()) <= X.NEEDLE_MIN_WEIGHT_GAP and X.needle_gain(DV) == X.NEEDLE_GAIN_VIT == 8.0
    with pytest.raises(AssertionError, match="1 - w"):
        X.vit_needle_inputs(seg_lens, 2, seed, gain=X.NEEDLE_GAIN)


def test_needle_helpers_at_head_dim_80_and_their_default_of_128():
    k, v = X.needle_kv(70, 96, 1, seed=4, dim=DV)
    assert k.shape == (1, 96, DV) and bool((v[:, 70:] == X.POISON_V).all())
    q = X.needle_q(k, [33], 1, dim=DV)
    assert torch.equal(q[0].float(), k[0, 33].float() * 8.0)
    X.plant_twin(k, v, 0, 70, 33)
    ref, gaps, vmax = X.needle_reference(q, k, v, [0], [70], [33], dim=DV)
    assert X.check_needle(_as_kernel_output(ref), ref, gaps, vmax, dim=DV) == (True, 0.0)
    out, _ = X.softmax_rows(q[0], k[0], v[0], range(71), dim=DV)
    assert not X.check_needle(_as_kernel_output(out)[None], ref, gaps, vmax, dim=DV)[0], "the twin at index n admitted"
    k128, _ = X.needle_kv(8, 32, 1, seed=4)
    assert k128.shape == (1, 32, 128) and torch.equal(X.needle_q(k128, [3], 1)[0].float(), k128[0, 3].float() * 4.0)
    with pytest.raises(AssertionError):
        X.needle_q(k, [3], 1)                                        # a dim-80 K under the default dim


# ---------------------------------------------------------------------------------------------------------------------------------
# vision_rope_tables against the tables of HF's own vision model
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hf_visual():
    from livecc_amd.config import tiny
    from oracle import hf_oracle as O
    return O.build_hf_model(tiny(), dtype=torch.float32).model.visual


def _hf_tables(hf_visual, grids):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)               # rot_pos_emb: deprecated by name, still what the tower's forward computes
        with torch.no_grad():
            freqs = hf_visual.rot_pos_emb(torch.tensor(grids, dtype=torch.long))
    assert freqs.dtype == torch.float32
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos(), emb.sin()


@pytest.mark.parametrize("grids", [X.vit_even_grids(VIT_GRIDS), [(3, 4, 6), (1, 10, 14), (2, 6, 8)]], ids=["test_grids", "multi_clip_t3"])
def test_vision_rope_tables_are_hf_tables(hf_visual, grids):
    """The 10 x 13 grid of VIT_GRIDS is a segment length for the kernels, not a frame: HF refuses it as vision_rope_tables does (2 x 2
    merge), so the table comparison runs on the even grids (10 x 14 in its place) and on a multi-clip list with t > 1."""
    from livecc_amd.config import tiny
    from livecc_amd.engine import vision_rope_tables
    cos, sin = vision_rope_tables(grids, tiny())
    P = sum(t * h * w for t, h, w in grids)
    assert cos.shape == sin.shape == (P, 40) and cos.dtype == sin.dtype == torch.float32
    hf_cos, hf_sin = _hf_tables(hf_visual, grids)
    assert hf_cos.shape == (P, 80)
    assert torch.equal(torch.cat([cos, cos], -1), hf_cos) and torch.equal(torch.cat([sin, sin], -1), hf_sin)


def test_an_odd_grid_is_refused_by_hf_and_by_vision_rope_tables_and_the_kernel_tests_take_rows_of_the_even_one(hf_visual):
    from livecc_amd.config import tiny
    from livecc_amd.engine import vision_rope_tables
    with pytest.raises(RuntimeError):
        vision_rope_tables([(1, 10, 13)], tiny())
    with pytest.raises(RuntimeError):
        _hf_tables(hf_visual, [(1, 10, 13)])
    cos, sin = X.vit_rope_tables_for(VIT_GRIDS, tiny())
    assert cos.shape == sin.shape == (618, 40) and cos.is_contiguous() and sin.is_contiguous()
    hf_cos, hf_sin = _hf_tables(hf_visual, X.vit_even_grids(VIT_GRIDS))
    keep = torch.cat([torch.arange(0, 188 + 130), torch.arange(188 + 140, 628)])          # the 10 x 14 slice loses its last 10 rows
    assert torch.equal(torch.cat([cos, cos], -1), hf_cos[keep]) and torch.equal(torch.cat([sin, sin], -1), hf_sin[keep])

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

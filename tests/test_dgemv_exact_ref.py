"""Proof of tests/dgemv_exact.py (no GPU, no kernel).  For every case tests/test_gpu_dgemv_exact.py runs: the exactness conditions hold
(sums, scaled accumulators, tile statistics, normalised rows), and every mutant reference -- one deliberate mistake at a rounding point or
an index -- differs from the true reference in at least 5 % of the elements, so a kernel that made that mistake would fail torch.equal.
Plus the layout helpers: K / V placement against KvArena's own views, and the q|k|v row permutation."""
import pytest
import torch

from tests import dgemv_exact as X

MIN_SHARE = 0.05


def _share(a, b):
    return float((a != b).double().mean())


def _id(c):
    return "-".join(str(v) for v in c)


# ---------------------------------------------------------------------------------------------------------------------------------
# number-format helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rounding_helpers():
    x = torch.tensor([257.0, 258.0, 259.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1000.5], dtype=torch.float64)
    assert X.rb(x).tolist() == [256.0, 258.0, 260.0, 1.0, 1.015625, -1000.0]           # ties to even
    assert X.trunc_bf16(x).tolist() == [256.0, 258.0, 258.0, 1.0, 1.0078125, -1000.0]
    assert X.lsb_exp(torch.tensor([1.0, 0.375, -6.0], dtype=torch.float64)) == 3
    X.assert_sums_exact(torch.full((1, 4), 15.0, dtype=torch.float64), torch.full((2, 4), 15.0, dtype=torch.float64))
    with pytest.raises(AssertionError):
        X.assert_sums_exact(torch.full((1, 4), 2.0 ** 12 + 1, dtype=torch.float64), torch.full((1, 4), 2.0 ** 11 + 1, dtype=torch.float64))
    with pytest.raises(AssertionError):                                                 # 4097^2 + 1 does not fit 24 bits
        X.assert_stats_exact(torch.tensor([[4097.0, 1.0] + [0.0] * 14], dtype=torch.float64))


def test_weight_builders_hold_what_they_say():
    from livecc_amd.weights import unpack_scale_mxfp4, unpack_weight_fp8, unpack_weight_mxfp4
    g = X.gen(1)
    W8 = X.make_weight("fp8", 32, 128, g)
    assert torch.equal(W8["bytes"].view(torch.float8_e4m3fn).double(), W8["q64"])
    sc = W8["scale64"]
    assert bool((sc != sc.roll(1)).all()) and bool((torch.log2(sc) != torch.log2(sc).round()).any()), "row scales: neighbours differ, not all powers of two"
    w_eff = W8["q64"] * sc[:, None]
    assert torch.equal(w_eff, w_eff.round())
    W4 = X.make_weight("mxfp4", 32, 256, g)
    assert not bool((W4["codes"] == 8).any()) and int(W4["sc"].max()) - int(W4["sc"].min()) == 3
    assert bool((W4["sc"][:, 1:] != W4["sc"][:, :-1]).all()), "neighbouring blocks of a row never share a scale"
    p, kw = X.pack(W4, "cpu")
    assert torch.equal(unpack_weight_mxfp4(p), W4["codes"]) and torch.equal(unpack_scale_mxfp4(kw["w4scale"]), W4["sc"])
    p8, kw8 = X.pack(W8, "cpu")
    assert torch.equal(unpack_weight_fp8(p8), W8["bytes"]) and kw8["wscale"].dtype == torch.float32
    for fmt in ("fp8", "mxfp4"):
        W = X.make_weight(fmt, 32, 256, g)
        x = X.ints(g, (2, 256), 3)
        assert _share(X.linear64(x, W)[0], X.linear64(x, X.neighbour_scale(W))[0]) > 0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# residual epilogue
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.RESID_CASES, ids=_id)
def test_residual_cases_are_exact_and_tell_the_mutants_apart(case):
    c = X.resid_case(*case)
    W, x, h0 = c["W"], c["x"], c["h0"]
    X.assert_sums_exact(x, W["q64"])
    lin, acc = X.linear64(x, W)
    X.assert_scaled_exact(acc, W["scale64"])
    v, stats = X.resid_ref(x, W, h0)
    X.assert_stats_exact(v)
    assert torch.equal(stats.float().double(), stats)
    assert bool((x != 0).all()) or X.amplitudes(case[0], case[3])[2] < 1, "every column of the weight is multiplied by a non-zero activation in every row"
    assert _share(v, X.resid_ref(x, W, h0, mutant="resid_before_rounding")[0]) >= MIN_SHARE
    if W["fmt"] != "bf16":
        assert _share(v, X.resid_ref(x, X.neighbour_scale(W), h0)[0]) >= MIN_SHARE


# ---------------------------------------------------------------------------------------------------------------------------------
# RMSNorm prologue + bf16 / SwiGLU epilogues
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_norm_rows(c):
    h, nw, r, eps = c["h"], c["nw"], c["r"], c["eps"]
    M, K = h.shape
    hb = h.to(torch.bfloat16)
    assert torch.equal(hb.double(), h)
    stats = hb.float().pow(2).view(M, K // 16, 16).sum(-1)                  # what ops.tile_stats computes
    assert len(torch.unique(stats)) > 1 or K < 128, "the tile statistics vary along a row"
    ms = stats.double().sum(-1) / K + eps
    assert torch.equal(ms.float().double(), ms)
    assert torch.equal(torch.rsqrt(ms.float()).double(), r), "fp32 rsqrt of the mean square + eps is the exact power of two"
    assert M == 1 or len(torch.unique(r)) > 1, "rows of one case have different r"
    hr = h * r[:, None]
    assert torch.equal(X.rb(hr), hr), "h * r is a bf16 value"
    for off in (-2, 2):                                                     # an rsqrt a few fp32 ulps off still rounds to it
        r_off = (r.float().view(torch.int32) + off).view(torch.float32).double()
        assert torch.equal(X.rb(X.f32(h * r_off[:, None])), hr)
    xn = X.norm_ref(h, nw, r)
    assert torch.equal(X.norm_ref(h, nw, r, mutant="single_rounded"), xn), "with r a power of two one rounding equals two"
    return xn


@pytest.mark.parametrize("case", X.NORM_CASES, ids=_id)
def test_norm_linear_cases_are_exact_and_tell_the_mutants_apart(case):
    c = X.norm_case(*case)
    W, h, nw, r, bias = c["W"], c["h"], c["nw"], c["r"], c["bias"]
    xn = _check_norm_rows(c)
    X.assert_sums_exact(xn, W["q64"])
    lin, acc = X.linear64(xn, W)
    X.assert_scaled_exact(acc, W["scale64"])
    assert torch.equal(bias.to(torch.bfloat16).double(), bias)
    y = X.bias_ref(xn, W, bias)
    assert _share(y, X.bias_ref(xn, W, bias, mutant="bias_after_rounding")) >= MIN_SHARE
    plain = X.bias_ref(xn, W)
    if case[3] < 8192:                                                      # the one long-K case keeps norm weights that never round
        assert _share(xn, X.norm_ref(h, nw, r, mutant="truncated")) >= MIN_SHARE
        assert _share(plain, X.bias_ref(X.norm_ref(h, nw, r, mutant="truncated"), W)) >= MIN_SHARE
    # eps: without it r = c^-1/2
    c_row = torch.tensor([X.ROW_C[m] for m in range(h.shape[0])], dtype=torch.float64)
    assert _share(plain, X.bias_ref(X.norm_ref(h, nw, c_row ** -0.5), W)) >= MIN_SHARE
    if h.shape[0] > 1:
        assert _share(plain, X.bias_ref(X.norm_ref(h, nw, r, mutant="other_row_r"), W)) >= MIN_SHARE
    if W["fmt"] != "bf16":
        assert _share(plain, X.bias_ref(xn, X.neighbour_scale(W))) >= MIN_SHARE


@pytest.mark.parametrize("case", X.SWIGLU_CASES, ids=_id)
def test_swiglu_cases_are_exact_and_mostly_saturated(case):
    c = X.norm_case(*case, swiglu=True)
    W = c["W"]
    xn = _check_norm_rows(c)
    X.assert_sums_exact(xn, W["q64"])
    lin, acc = X.linear64(xn, W)
    X.assert_scaled_exact(acc, W["scale64"])
    out, g, sat = X.swiglu_ref(xn, W)
    assert float(sat.double().mean()) >= 0.5, "at least half of the gates are 0 or >= 32"
    assert float((g >= X.SAT_GATE).double().mean()) >= 0.25 and float((g == 0).double().mean()) >= 0.2
    assert float((g < X.GATE_GRAY[0]).double().mean()) >= 0.1, "gates whose silu underflows to zero"
    assert bool((~sat).any()), "some gates go through the transcendental"
    gu = g[~sat]
    assert not bool(((gu >= X.GATE_GRAY[0]) & (gu <= X.GATE_GRAY[1])).any()), "a gate whose silu is a denormal"
    small = gu[gu > X.GATE_GRAY[1]]
    assert bool((X.silu_tie_margin(small) > 2.0 ** -10).all()), "a silu within 2^-18 (relative) of a bf16 rounding tie"
    assert torch.equal(out[g >= X.SAT_GATE], X.rb(X.f32(g * X.rb(lin.view(g.shape[0], -1, 2, 16)[:, :, 1]).reshape(g.shape)))[g >= X.SAT_GATE])
    if W["fmt"] != "bf16":
        assert _share(out, X.swiglu_ref(xn, X.neighbour_scale(W))[0]) >= MIN_SHARE


def test_inexact_r_rows_round_safely_and_tell_one_rounding_from_two():
    """r = 3^-1/2: h * r needs a rounding; every h * r is far enough from a bf16 tie that an rsqrt 4 fp32 ulps off rounds alike"""
    for M in (1, 2):
        c = X.inexact_case(M)
        h, nw, r, W = c["h"], c["nw"], c["r"], c["W"]
        ms = (h * h).sum(-1) / c["K"] + c["eps"]
        assert torch.equal(ms, torch.full_like(ms, 3.0))
        want = X.rb(X.f32(h * r[:, None]))
        for off in (-4, -1, 1, 4):
            r_off = (r.float().view(torch.int32) + off).view(torch.float32).double()
            assert torch.equal(X.rb(X.f32(h * r_off[:, None])), want)
        xn = X.norm_ref(h, nw, r)
        assert _share(xn, X.norm_ref(h, nw, r, mutant="single_rounded")) >= MIN_SHARE
        assert _share(X.bias_ref(xn, W), X.bias_ref(X.norm_ref(h, nw, r, mutant="single_rounded"), W)) >= MIN_SHARE
        X.assert_sums_exact(xn, W["q64"])


# ---------------------------------------------------------------------------------------------------------------------------------
# the GEMVs of csrc/gemm.hip (tests/test_gpu_gemv_exact.py): bias, split-K slabs, SwiGLU, 17..64 rows
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.GEMV_BIAS_CASES + X.GEMV_MG_CASES, ids=_id)
def test_gemv_bias_cases_are_exact_and_tell_the_mutants_apart(case):
    fmt, M, N, K = case
    c = X.resid_case(*case)
    W, x, bias = c["W"], c["x"], X.gemv_bias(N)
    assert x.shape == (M, K) and torch.equal(x.to(torch.bfloat16).double(), x) and torch.equal(bias.to(torch.bfloat16).double(), bias)
    X.assert_sums_exact(x, W["q64"])
    X.assert_scaled_exact(X.linear64(x, W)[1], W["scale64"])
    y = X.bias_ref(x, W, bias)
    assert _share(y, X.bias_ref(x, W, bias, mutant="bias_after_rounding")) >= MIN_SHARE
    assert _share(y, X.bias_ref(x, W)) >= MIN_SHARE, "the bias shows"
    if fmt != "bf16":
        assert _share(X.bias_ref(x, W), X.bias_ref(x, X.neighbour_scale(W))) >= MIN_SHARE


@pytest.mark.parametrize("case", X.GEMV_SLAB_CASES + X.GEMV_MG_SLAB_CASES, ids=_id)
def test_gemv_slab_cases_are_exact_per_split_and_tell_a_shifted_boundary(case):
    fmt, M, N, K, S = case
    c = X.resid_case(fmt, M, N, K)
    W, x = c["W"], c["x"]
    ranges = X.slab_ranges(fmt, K, S)
    assert ranges[0][0] == 0 and ranges[-1][1] == K and all(a < b for a, b in ranges), "every split owns at least one chunk"
    assert all(ranges[s][1] == ranges[s + 1][0] for s in range(S - 1))
    for a, b in ranges:
        X.assert_sums_exact(x[:, a:b], W["q64"][:, a:b])
        X.assert_scaled_exact(x[:, a:b] @ W["q64"][:, a:b].t(), W["scale64"])
    slabs = X.slab_ref(x, W, S)
    assert slabs.shape == (S, M, N) and torch.equal(X.f32(slabs.sum(0)), X.linear64(x, W)[0]), "the slabs add up to the Linear output, exactly"
    for shift in (-1, 1):
        moved = X.slab_ref(x, W, S, shift=shift)
        assert all(_share(slabs[s], moved[s]) >= MIN_SHARE for s in range(S)), "every split tells a boundary that is one chunk off"
    if fmt != "bf16":
        assert _share(slabs, X.slab_ref(x, X.neighbour_scale(W), S)) >= MIN_SHARE


@pytest.mark.parametrize("case", X.GEMV_MG_SWIGLU_CASES, ids=_id)
def test_gemv_swiglu_cases_of_17_to_64_rows_are_exact_and_mostly_saturated(case):
    """norm_rows beyond four rows: the same proof as for SWIGLU_CASES (whose operands the M <= 16 SwiGLU cases of the GEMV file use as they are)"""
    assert X.GEMV_SWIGLU_CASES is X.SWIGLU_CASES
    test_swiglu_cases_are_exact_and_mostly_saturated(case)
    c = X.norm_case(*case, swiglu=True)
    xn = X.norm_ref(c["h"], c["nw"], c["r"])
    assert xn.shape == (case[1], case[3]) and torch.equal(xn.to(torch.bfloat16).double(), xn)


def test_gemv_variant_cases_are_among_the_proven_ones():
    assert X.GEMV_VARIANT_CASES["plain"] in X.GEMV_BIAS_CASES and X.GEMV_VARIANT_CASES["swiglu"] in X.GEMV_SWIGLU_CASES


# ---------------------------------------------------------------------------------------------------------------------------------
# bias + M-RoPE + KV append
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.ROPE_CASES, ids=_id)
def test_rope_cases_are_exact_and_tell_the_mutants_apart(case):
    fmt, M, Hq, Hkv, K, lmax = case
    c = X.rope_case(*case)
    W, h, nw, r, bias = c["W"], c["h"], c["nw"], c["r"], c["bias"]
    xn = _check_norm_rows(c)
    X.assert_sums_exact(xn, W["q64"])
    lin, acc = X.linear64(xn, W)
    X.assert_scaled_exact(acc, W["scale64"])
    cos, sin, _ = X.hf_mrope_rows(c["pos3"])
    assert bool((sin.abs() > 0).any(-1).all())
    q, k, v = X.rope_ref(xn, W, bias, cos, sin, Hq, Hkv)
    qm, km, _ = X.rope_ref(xn, W, bias, cos, sin, Hq, Hkv, mutant="rotate_half_sign")
    assert _share(q, qm) >= MIN_SHARE and _share(k, km) >= MIN_SHARE
    y = X.bias_ref(xn, W, bias)
    assert _share(y, X.bias_ref(xn, W, bias, mutant="bias_after_rounding")) >= MIN_SHARE
    if fmt != "bf16":
        qs, ks, vs = X.rope_ref(xn, X.neighbour_scale(W), bias, cos, sin, Hq, Hkv)
        assert min(_share(q, qs), _share(k, ks), _share(v, vs)) >= MIN_SHARE
    # streams: distinct slots, not the identity, positions from the ring
    ts, kl = c["tok_stream"], c["kv_len"]
    assert len(set(ts)) == M and ts != list(range(M)) and all(0 <= s < c["n_slots"] for s in ts)
    assert all(kl[s] in (0, 31, 32, 63, lmax - 1) for s in ts)


def test_every_ring_position_is_appended_under_every_format_and_both_arena_lengths():
    seen = {}
    for case in X.ROPE_CASES:
        c = X.rope_case(*case)
        seen.setdefault((case[0], case[5]), set()).update(c["kv_len"][s] for s in c["tok_stream"])
    for fmt in X.FORMATS:
        assert seen[(fmt, 64)] >= {0, 31, 32, 63}, (fmt, seen[(fmt, 64)])
        assert 127 in seen[(fmt, 128)], (fmt, seen[(fmt, 128)])


@pytest.mark.parametrize("Hkv,lmax,layer", [(1, 64, 0), (2, 128, 1)])
def test_reference_kv_placement_agrees_with_the_arena_views(Hkv, lmax, layer):
    from livecc_amd import ops
    kv = ops.KvArena(3, 2, Hkv, lmax, "cpu")
    pre = X.arena_pattern(3, kv.per_slot)
    assert len(torch.unique(pre.view(torch.int16))) > 30000 and bool(torch.isfinite(pre.float()).all())
    tok_stream, kv_len = [2, 0], [lmax - 1, 7, 32]
    k = (torch.arange(2 * Hkv * 128, dtype=torch.float64).view(2, Hkv, 128) * 7) % 251 + 1      # bf16 values, rows differ
    v = -k
    kv.buf.copy_(X.place_kv(pre, Hkv, lmax, layer, tok_stream, kv_len, k, v))
    changed = kv.buf.view(torch.int16) != pre.view(torch.int16)
    assert int(changed.sum()) == 2 * 2 * Hkv * 128 and not bool(changed[1].any())
    for m, slot in enumerate(tok_stream):
        pos = kv_len[slot]
        assert torch.equal(kv.k_view(slot, layer)[:, pos].double(), k[m])
        assert torch.equal(kv.v_view(slot, layer)[:, pos].double(), v[m])
        other = 1 - layer
        assert torch.equal(kv.k_view(slot, other).reshape(-1).view(torch.int16),
                           pre[slot].view(torch.int16)[other * 2 * Hkv * lmax * 128:(other * 2 + 1) * Hkv * lmax * 128])


@pytest.mark.parametrize("Hq,Hkv", list(X.HEADS_K))
def test_qkv_row_permutation_round_trips(Hq, Hkv):
    perm = X.qkv_perm(Hq, Hkv, 64)
    N = (Hq + 2 * Hkv) * 128
    assert sorted(perm.tolist()) == list(range(N))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(N)
    w = torch.arange(N)
    assert torch.equal(w[perm][inv], w)
    # stored tile t of head hd: rows 0-7 = channels j*8 .. +7, rows 8-15 = their rotation partners (+64): what the epilogue assumes
    st = perm.view(-1, 8, 2, 8)
    hd = torch.arange(N // 128)[:, None, None]
    j = torch.arange(8)[None, :, None]
    i = torch.arange(8)[None, None, :]
    assert torch.equal(st[:, :, 0], hd * 128 + j * 8 + i) and torch.equal(st[:, :, 1], hd * 128 + 64 + j * 8 + i)


# ---------------------------------------------------------------------------------------------------------------------------------
# chained launch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", X.CHAIN_CASES)
def test_chain_cases_hand_over_an_exact_norm_row(M):
    c = X.chain_case(M)
    X.assert_sums_exact(c["x"], c["Wd"]["q64"])
    v, stats = X.resid_ref(c["x"], c["Wd"], c["h0"])
    assert torch.equal(v, c["h1"])
    X.assert_stats_exact(v)
    xn = _check_norm_rows(dict(h=v, nw=c["nw"], r=c["r"], eps=c["eps"]))
    X.assert_sums_exact(xn, c["Wq"]["q64"])

"""-m gpu: the decode GEMVs (csrc/decode_v2.hip: two prologues, four epilogues, three weight formats, the chained launch) on the operands of
tests/dgemv_exact.py, whose sums are exact in fp32 in ANY order -- so the expected output is unique and every assertion is torch.equal against
a float64 reference with the rounding points written out.  The one exception: SwiGLU outputs whose gate goes through the fp32 transcendental
(neither 0 nor >= 32) are held to 1 bf16 ulp.  tests/test_dgemv_exact_ref.py proves on the CPU that these inputs are exact and that a kernel
with one misplaced rounding, scale index or rotation sign would differ in >= 5 % of the elements.

Every output lives in a view inside a larger poisoned buffer (rows beyond M, columns beyond N, 4 KB on either side): a store outside the
result is seen.  Shapes are tiny (N <= 1152, one grid of 257 blocks for the MXFP4 N/16 > 256 branch); K covers one fragment, the odd half chunk
of the bf16 format (K % 64 == 32), fewer chunks than waves and counts ragged across 8 and 16 waves."""
import functools

import pytest
import torch

from tests import dgemv_exact as X
from tests.dgemv_exact import BF, Canary, _dev
from tests.test_gpu_decode_v2 import resid_waves  # noqa: F401  (fixture: both block shapes of lcc_dgemv_resid)

pytestmark = pytest.mark.gpu


def _id(c):
    return "-".join(str(v) for v in c)


@functools.lru_cache(maxsize=None)
def _resid_expected(case):
    c = X.resid_case(*case)
    return X.resid_ref(c["x"], c["W"], c["h0"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. h += Linear(x), tile statistics
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.RESID_CASES, ids=_id)
def test_residual_gemv_is_bit_exact(dev, case, resid_waves):
    from livecc_amd import ops
    fmt, M, N, K = case
    c = X.resid_case(*case)
    wp, kw = X.pack(c["W"], dev)
    h = Canary(dev, M, N, BF, init=c["h0"])
    st = Canary(dev, M, N // 16, torch.float32)
    ops.dgemv_resid_(wp, _dev(c["x"], dev), h.view, (N, K), stats_out=st.view, **kw)
    v, stats = _resid_expected(case)
    got = h.view.cpu().double()
    assert torch.equal(got, v), (case, int((got != v).sum()), (got != v).nonzero()[:4].tolist())
    assert torch.equal(st.view.cpu().double(), stats), case
    h.check("h"), st.check("stats_out")


@pytest.mark.parametrize("fmt,K", [("bf16", 96), ("fp8", 192), ("mxfp4", 384)])
def test_residual_gemv_reads_x_at_its_row_stride(dev, fmt, K):
    """ldx > K: rows of x lie 64 elements further apart, the gap holds 64.0 (finite: a read of it changes the sums)"""
    from livecc_amd import ops
    M, N = 5, 80
    c = X.resid_case(fmt, M, N, K)
    wp, kw = X.pack(c["W"], dev)
    xw = torch.full((M, K + 64), 64.0, dtype=BF, device=dev)
    xw[:, :K] = _dev(c["x"], dev)
    h = Canary(dev, M, N, BF, init=c["h0"])
    st = Canary(dev, M, N // 16, torch.float32)
    ops.dgemv_resid_(wp, xw, h.view, (N, K), stats_out=st.view, ldx=K + 64, **kw)
    v, stats = _resid_expected((fmt, M, N, K))
    assert torch.equal(h.view.cpu().double(), v) and torch.equal(st.view.cpu().double(), stats)
    h.check("h"), st.check("stats_out")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. RMSNorm + Linear (+ bias) and RMSNorm + gate/up + SwiGLU
# ---------------------------------------------------------------------------------------------------------------------------------
def _norm_inputs(c, dev):
    from livecc_amd import ops
    h = _dev(c["h"], dev)
    return h, ops.tile_stats(h), _dev(c["nw"], dev)


@pytest.mark.parametrize("with_bias", [False, True], ids=["plain", "bias"])
@pytest.mark.parametrize("case", X.NORM_CASES, ids=_id)
def test_norm_linear_gemv_is_bit_exact(dev, case, with_bias):
    from livecc_amd import ops
    fmt, M, N, K = case
    c = X.norm_case(*case)
    wp, kw = X.pack(c["W"], dev)
    h, stats, nw = _norm_inputs(c, dev)
    assert torch.equal(stats.cpu().double(), (c["h"] ** 2).view(M, K // 16, 16).sum(-1))
    out = Canary(dev, M, N, BF, extra_cols=24)
    ops.dgemv_norm_linear(wp, h, stats, nw, c["eps"], (N, K), bias=_dev(c["bias"], dev) if with_bias else None, out=out.view, **kw)
    want = X.bias_ref(X.norm_ref(c["h"], c["nw"], c["r"]), c["W"], c["bias"] if with_bias else None)
    got = out.view.cpu().double()
    assert torch.equal(got, want), (case, int((got != want).sum()), (got != want).nonzero()[:4].tolist())
    out.check("out")


@pytest.mark.parametrize("M", [1, 2])
def test_norm_linear_gemv_with_an_r_that_is_not_a_power_of_two(dev, M):
    """r = 3^-1/2 and eps = 0: bf16(h * r) really rounds (every value asserted safe against an rsqrt 4 fp32 ulps off), so
    bf16(w * bf16(h * r)) and the single-rounded bf16(w * h * r) differ"""
    from livecc_amd import ops
    c = X.inexact_case(M)
    wp, kw = X.pack(c["W"], dev)
    h, stats, nw = _norm_inputs(c, dev)
    out = Canary(dev, M, c["N"], BF, extra_cols=24)
    ops.dgemv_norm_linear(wp, h, stats, nw, c["eps"], (c["N"], c["K"]), out=out.view, **kw)
    assert torch.equal(out.view.cpu().double(), X.bias_ref(X.norm_ref(c["h"], c["nw"], c["r"]), c["W"]))
    out.check("out")


@pytest.mark.parametrize("case", X.SWIGLU_CASES, ids=_id)
def test_norm_swiglu_gemv_is_bit_exact_where_the_gate_saturates(dev, case):
    from livecc_amd import ops
    fmt, M, N, K = case
    c = X.norm_case(*case, swiglu=True)
    wp, kw = X.pack(c["W"], dev)
    h, stats, nw = _norm_inputs(c, dev)
    out = Canary(dev, M, N // 2, BF, extra_cols=24)
    ops.dgemv_norm_linear(wp, h, stats, nw, c["eps"], (N, K), swiglu=True, out=out.view, **kw)
    want, g, sat = X.swiglu_ref(X.norm_ref(c["h"], c["nw"], c["r"]), c["W"])
    got = out.view.cpu().double()
    print(f"swiglu {case}: {int(sat.sum())} saturated gates, {int((~sat).sum())} through exp; differing: {int((got != want).sum())}")
    assert bool(torch.isfinite(got).all()), (case, "non-finite outputs at gates", g[~torch.isfinite(got)][:8].tolist())
    assert torch.equal(got[sat], want[sat]), (case, int((got[sat] != want[sat]).sum()))
    ok, worst = X.deviation(got[~sat], want[~sat])
    assert ok, (case, worst)
    out.check("out")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. RMSNorm + q|k|v + bias + M-RoPE + KV append
# ---------------------------------------------------------------------------------------------------------------------------------
def _rope_tables(pos3, dev):
    from livecc_amd import ops
    _, _, inv = X.hf_mrope_rows(pos3)
    cos, sin = ops.mrope_table(pos3.to(dev), inv.to(dev), [16, 24, 24])
    return cos, sin


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("case", X.ROPE_CASES, ids=_id)
def test_qkv_rope_gemv_is_bit_exact_and_appends_exactly_one_row(dev, case):
    from livecc_amd import ops
    fmt, M, Hq, Hkv, K, lmax = case
    c = X.rope_case(*case)
    wp, kw = X.pack(c["W"], dev, X.qkv_perm(Hq, Hkv, K))
    h, stats, nw = _norm_inputs(c, dev)
    cos, sin = _rope_tables(c["pos3"], dev)
    kv = ops.KvArena(c["n_slots"], c["n_layers"], Hkv, lmax, dev)
    pre = X.arena_pattern(c["n_slots"], kv.per_slot)
    kv.buf.copy_(pre)
    q = Canary(dev, M, Hq * 128, BF)
    ops.dgemv_qkv_rope(wp, h, stats, nw, c["eps"], _dev(c["bias"], dev), cos, sin, _i32(c["tok_stream"], dev), _i32(c["kv_len"], dev), kv,
                       c["layer"], Hq, q_out=q.view, **kw)
    xn = X.norm_ref(c["h"], c["nw"], c["r"])
    q_ref, k_ref, v_ref = X.rope_ref(xn, c["W"], c["bias"], cos.cpu().double(), sin.cpu().double(), Hq, Hkv)
    got_q = q.view.cpu().double()
    assert torch.equal(got_q, q_ref), (case, int((got_q != q_ref).sum()), (got_q != q_ref).nonzero()[:4].tolist())
    q.check("q_out")
    for m, slot in enumerate(c["tok_stream"]):
        pos = c["kv_len"][slot]
        gk, gv = kv.k_view(slot, c["layer"])[:, pos].cpu().double(), kv.v_view(slot, c["layer"])[:, pos].cpu().double()
        assert torch.equal(gk, k_ref[m]), (case, "K row", m, slot, pos, int((gk != k_ref[m]).sum()))
        assert torch.equal(gv, v_ref[m]), (case, "V column", m, slot, pos, int((gv != v_ref[m]).sum()))
    # the pattern holds neither zero nor NaN, so equality of values is identity of the bytes outside the appended rows
    want = X.place_kv(pre, Hkv, lmax, c["layer"], c["tok_stream"], c["kv_len"], k_ref, v_ref)
    assert torch.equal(kv.buf.cpu(), want), (case, "the arena differs from its pre-image outside the appended rows")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the chained launch against the CPU reference
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", X.CHAIN_CASES)
def test_chained_down_qkv_launch_is_bit_exact(dev, M):
    from livecc_amd import ops
    c = X.chain_case(M)
    Hq, Hkv, H, I, lmax = c["Hq"], c["Hkv"], c["H"], c["I"], c["lmax"]
    wd, _ = X.pack(c["Wd"], dev)
    wq, _ = X.pack(c["Wq"], dev, X.qkv_perm(Hq, Hkv, H))
    cos, sin = _rope_tables(c["pos3"], dev)
    kv = ops.KvArena(M, 1, Hkv, lmax, dev)
    pre = X.arena_pattern(M, kv.per_slot)
    kv.buf.copy_(pre)
    h = Canary(dev, M, H, BF, init=c["h0"])
    counter, err = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    try:
        st, q = ops.dgemv_down_qkv_(wd, _dev(c["x"], dev), h.view, I, wq, _dev(c["nw"], dev), c["eps"], _dev(c["bias"], dev), cos, sin,
                                    _i32(c["tok_stream"], dev), _i32(c["kv_len"], dev), kv, 0, Hq, counter, 0, err)
    except RuntimeError as e:
        if "(-5)" in str(e):
            pytest.skip(f"the two grids ({H // 16} + {(Hq + 2 * Hkv) * 8} blocks) do not fit this chip at once: {e}")
        raise
    assert int(err[0]) == 0, "a consumer block gave up waiting"
    assert int(counter[0]) == H // 16
    v, stats = X.resid_ref(c["x"], c["Wd"], c["h0"])
    assert torch.equal(h.view.cpu().double(), v) and torch.equal(st.cpu().double(), stats)
    h.check("h")
    q_ref, k_ref, v_ref = X.rope_ref(X.norm_ref(v, c["nw"], c["r"]), c["Wq"], c["bias"], cos.cpu().double(), sin.cpu().double(), Hq, Hkv)
    assert torch.equal(q.cpu().double(), q_ref)
    assert torch.equal(kv.buf.cpu(), X.place_kv(pre, Hkv, lmax, 0, c["tok_stream"], c["kv_len"], k_ref, v_ref))


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. refusals: an error, no launch -- the outputs keep their bytes
# ---------------------------------------------------------------------------------------------------------------------------------
def _zeros_weight(fmt, N, K, dev):
    if fmt == "bf16":
        return torch.zeros(N * ((K + 31) // 32) * 32, dtype=BF, device=dev), {}
    if fmt == "fp8":
        return torch.zeros(N, K, dtype=torch.uint8, device=dev), {"wscale": torch.ones(N, dtype=torch.float32, device=dev)}
    return torch.zeros(N, K // 2, dtype=torch.uint8, device=dev), {"w4scale": torch.full((N, K // 32), 127, dtype=torch.uint8, device=dev)}


@pytest.mark.parametrize("fmt,M,K", [("bf16", 1, 48), ("fp8", 1, 96), ("mxfp4", 1, 64), ("bf16", 17, 64)],
                         ids=["k_not_32", "fp8_k_not_64", "mxfp4_k_not_128", "m_17"])
def test_residual_gemv_refuses(dev, fmt, M, K):
    from livecc_amd import _lib, ops
    N = 16
    wp, kw = _zeros_weight(fmt, N, K, dev)
    h, st = Canary(dev, M, N, BF, init=torch.ones(M, N)), Canary(dev, M, 1, torch.float32)
    with pytest.raises(_lib.LccError):
        ops.dgemv_resid_(wp, torch.ones(M, K, dtype=BF, device=dev), h.view, (N, K), stats_out=st.view, **kw)
    torch.cuda.synchronize()
    assert h.untouched() and st.untouched()


def test_residual_gemv_refuses_zero_rows(dev):
    """M = 0 through the C ABI (an empty tensor has no address to pass through ops)"""
    from livecc_amd import _lib
    N, K = 16, 32
    wp, _ = _zeros_weight("bf16", N, K, dev)
    x = torch.ones(1, K, dtype=BF, device=dev)
    h, st = Canary(dev, 1, N, BF, init=torch.ones(1, N)), Canary(dev, 1, 1, torch.float32)
    rc = _lib.load().lcc_dgemv_resid(wp.data_ptr(), None, x.data_ptr(), K, h.view.data_ptr(), st.view.data_ptr(), 0, N, K,
                                     torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and h.untouched() and st.untouched()


@pytest.mark.parametrize("M,N,K,swiglu", [(5, 16, 64, False), (3, 16, 5504, False), (1, 48, 64, True)], ids=["m_5", "rows_past_lds", "swiglu_n_not_32"])
def test_norm_linear_gemv_refuses(dev, M, N, K, swiglu):
    from livecc_amd import _lib, ops
    wp, _ = _zeros_weight("bf16", N, K, dev)
    hrow = torch.ones(M, K, dtype=BF, device=dev)
    out = Canary(dev, M, N // 2 if swiglu else N, BF, extra_cols=8)
    with pytest.raises(_lib.LccError):
        ops.dgemv_norm_linear(wp, hrow, ops.tile_stats(hrow), torch.ones(K, dtype=BF, device=dev), 1e-6, (N, K), swiglu=swiglu, out=out.view)
    torch.cuda.synchronize()
    assert out.untouched()

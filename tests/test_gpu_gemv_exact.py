"""-m gpu: the weight-streaming GEMVs of csrc/gemm.hip (gemv_skinny_kernel for bf16 weights and up to 64 rows, the quantised-weight GEMV for
fp8 and MXFP4 weights and up to 16 rows; three output forms: fp32 split-K slabs, bf16 + bias, SwiGLU) on the operands of tests/dgemv_exact.py,
whose sums are exact in fp32 in ANY order -- the expected output is unique and every assertion is torch.equal against a float64 reference with
the rounding points written out.  The one exception, as in tests/test_gpu_dgemv_exact.py: SwiGLU outputs whose gate goes through the fp32
transcendental are held to 1 bf16 ulp; saturated gates are exact and every output is finite.  tests/test_dgemv_exact_ref.py proves on the CPU
that the GEMV_* cases are exact (per split for the slabs) and that a misplaced bias rounding, scale index or split boundary would show.

The kernels are reached through the C ABI (lcc_gemm_bf16 / lcc_gemm_w8_bf16 / lcc_gemm_w4_bf16) because ops.linear* allocate their own outputs:
here every output is a view inside a poisoned buffer with rows below it and columns to its right.  (The slab form has no leading dimension of
its own -- a slab row is N floats -- so a slab canary has the rows below and the padding around only.)  Shapes are tiny: N = 80 / 96, the
largest grid is 5 blocks x 17 splits."""
import functools

import pytest
import torch

from tests import dgemv_exact as X
from tests.dgemv_exact import BF, Canary, _dev

pytestmark = pytest.mark.gpu

EPI_NONE, EPI_SWIGLU = 0, 4


def _id(v):
    return "-".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


def _with_layouts(cases):
    """bf16 weights exist row-major and packed; the quantised formats in their packed order only"""
    return [(c, lay) for c in cases for lay in (("packed", "rows") if c[0] == "bf16" else ("packed",))]


def _weight(W, dev, layout):
    """-> (device weight, w_layout of lcc_gemm_bf16, scale pointer holder)"""
    if layout == "rows":
        return W["rows"].contiguous().to(dev), 0, {}
    wp, kw = X.pack(W, dev)
    return wp, 1, kw


def _gemm(dev, W, layout, x, M, out=None, ldc=0, bias=None, epi=EPI_NONE, slab=None, nsplit=0, weight=None):
    """one call of the C ABI; returns the error code (0 = launched)"""
    from livecc_amd import _lib
    lib = _lib.load()
    fmt, N, K = W["fmt"], W["N"], W["K"]
    wp, w_layout, kw = weight if weight is not None else _weight(W, dev, layout)
    st = torch.cuda.current_stream(dev).cuda_stream
    C = out.data_ptr() if out is not None else None
    b = bias.data_ptr() if bias is not None else None
    P = slab.data_ptr() if slab is not None else None
    if fmt == "bf16":
        rc = lib.lcc_gemm_bf16(x.data_ptr(), K, wp.data_ptr(), K, w_layout, b, None, 0, C, ldc, M, N, K, epi, P, nsplit, st)
    elif fmt == "fp8":
        rc = lib.lcc_gemm_w8_bf16(x.data_ptr(), K, wp.data_ptr(), kw["wscale"].data_ptr(), b, None, 0, C, ldc, M, N, K, epi, P, nsplit, None, st)
    else:
        rc = lib.lcc_gemm_w4_bf16(x.data_ptr(), K, wp.data_ptr(), kw["w4scale"].data_ptr(), b, None, 0, C, ldc, M, N, K, epi, P, nsplit, None, st)
    torch.cuda.synchronize()
    return rc


def _equal(got, want, what):
    assert torch.equal(got, want), (what, int((got != want).sum()), (got != want).nonzero()[:4].tolist())


@functools.lru_cache(maxsize=None)
def _bias_expected(case, with_bias):
    c = X.resid_case(*case)
    return X.bias_ref(c["x"], c["W"], X.gemv_bias(case[2]) if with_bias else None)


@functools.lru_cache(maxsize=None)
def _slab_expected(case):
    fmt, M, N, K, S = case
    c = X.resid_case(fmt, M, N, K)
    return X.slab_ref(c["x"], c["W"], S)


@functools.lru_cache(maxsize=None)
def _swiglu_expected(case):
    c = X.norm_case(*case, swiglu=True)
    xn = X.norm_ref(c["h"], c["nw"], c["r"])
    return (xn,) + X.swiglu_ref(xn, c["W"])


# ---------------------------------------------------------------------------------------------------------------------------------
# bf16 + bias (MODE 1): M <= 16 in all three formats, 17..64 rows (2, 3, 4 activation groups) with bf16 weights
# ---------------------------------------------------------------------------------------------------------------------------------
def _run_bias(dev, case, layout, with_bias):
    fmt, M, N, K = case
    c = X.resid_case(*case)
    out = Canary(dev, M, N, BF, extra_cols=24)
    rc = _gemm(dev, c["W"], layout, _dev(c["x"], dev), M, out=out.view, ldc=out.ld, bias=_dev(X.gemv_bias(N), dev) if with_bias else None)
    assert rc == 0, (case, rc)
    _equal(out.view.cpu().double(), _bias_expected(case, with_bias), case)
    out.check("C")


@pytest.mark.parametrize("with_bias", [False, True], ids=["plain", "bias"])
@pytest.mark.parametrize("case,layout", _with_layouts(X.GEMV_BIAS_CASES), ids=_id)
def test_gemv_bf16_output_is_bit_exact(dev, case, layout, with_bias):
    _run_bias(dev, case, layout, with_bias)


@pytest.mark.parametrize("with_bias", [False, True], ids=["plain", "bias"])
@pytest.mark.parametrize("case,layout", _with_layouts(X.GEMV_MG_CASES), ids=_id)
def test_gemv_of_17_to_64_rows_is_bit_exact_and_stores_no_absent_row(dev, case, layout, with_bias):
    """M = 17 and 33 leave 15 of the last group's 16 rows empty: the rows below the result keep their poison"""
    _run_bias(dev, case, layout, with_bias)


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 split-K slabs (MODE 0)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,layout", _with_layouts(X.GEMV_SLAB_CASES + X.GEMV_MG_SLAB_CASES), ids=_id)
def test_gemv_slabs_are_bit_exact_per_split(dev, case, layout):
    fmt, M, N, K, S = case
    c = X.resid_case(fmt, M, N, K)
    slab = Canary(dev, S * M, N, torch.float32)
    rc = _gemm(dev, c["W"], layout, _dev(c["x"], dev), M, ldc=N, slab=slab.view, nsplit=S)
    assert rc == 0, (case, rc)
    _equal(slab.view.cpu().double().view(S, M, N), _slab_expected(case), case)
    slab.check("partial")


# ---------------------------------------------------------------------------------------------------------------------------------
# SwiGLU (MODE 2): the activation is handed in normalised
# ---------------------------------------------------------------------------------------------------------------------------------
def _run_swiglu(dev, case, layout, slab=None, nsplit=0):
    fmt, M, N, K = case
    c = X.norm_case(*case, swiglu=True)
    xn, want, g, sat = _swiglu_expected(case)
    out = Canary(dev, M, N // 2, BF, extra_cols=24)
    rc = _gemm(dev, c["W"], layout, _dev(xn, dev), M, out=out.view, ldc=out.ld, epi=EPI_SWIGLU, slab=slab, nsplit=nsplit)
    assert rc == 0, (case, rc)
    got = out.view.cpu().double()
    print(f"swiglu {case} {layout}: {int(sat.sum())} saturated gates, {int((~sat).sum())} through exp; differing: {int((got != want).sum())}")
    assert bool(torch.isfinite(got).all()), (case, "non-finite outputs at gates", g[~torch.isfinite(got)][:8].tolist())
    _equal(got[sat], want[sat], case)
    ok, worst = X.deviation(got[~sat], want[~sat])
    assert ok, (case, worst)
    out.check("C")


@pytest.mark.parametrize("case,layout", _with_layouts(X.GEMV_SWIGLU_CASES), ids=_id)
def test_gemv_swiglu_is_bit_exact_where_the_gate_saturates(dev, case, layout):
    _run_swiglu(dev, case, layout)


@pytest.mark.parametrize("case,layout", _with_layouts(X.GEMV_MG_SWIGLU_CASES), ids=_id)
def test_gemv_swiglu_of_17_to_64_rows_is_bit_exact_where_the_gate_saturates(dev, case, layout):
    _run_swiglu(dev, case, layout)


@pytest.mark.parametrize("fmt,K", [("bf16", 192), ("fp8", 192), ("mxfp4", 384)])
def test_gemv_swiglu_wins_over_a_slab_pointer_exactly(dev, fmt, K):
    """SwiGLU with `partial` set is the SwiGLU GEMV into C; the slab buffer keeps its bytes"""
    M, N = 3, 96
    slab = Canary(dev, 2 * M, N, torch.float32)
    _run_swiglu(dev, (fmt, M, N, K), "packed", slab=slab.view, nsplit=2)
    assert slab.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------
# the two other loop forms of the bf16 kernel (gemv_variant 0: two chunks per stage, one stage; 2: two chunks per stage, two stages)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 2])
def test_gemv_variants_are_bit_exact(dev, variant):
    from livecc_amd import ops
    ops.set_gemv_variant(variant)
    try:
        for layout in ("packed", "rows"):
            _run_bias(dev, X.GEMV_VARIANT_CASES["plain"], layout, True)
            _run_swiglu(dev, X.GEMV_VARIANT_CASES["swiglu"], layout)
    finally:
        ops.set_gemv_variant(ops.GEMV_DEFAULT_VARIANT)


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: an error, no launch -- the outputs keep their bytes
# ---------------------------------------------------------------------------------------------------------------------------------
def _zeros_weight(fmt, N, K, dev):
    if fmt == "bf16":
        return torch.zeros(N * ((K + 31) // 32) * 32, dtype=BF, device=dev), 1, {}
    if fmt == "fp8":
        return torch.zeros(N, K, dtype=torch.uint8, device=dev), 1, {"wscale": torch.ones(N, dtype=torch.float32, device=dev)}
    return torch.zeros(N, K // 2, dtype=torch.uint8, device=dev), 1, {"w4scale": torch.full((N, K // 32), 127, dtype=torch.uint8, device=dev)}


@pytest.mark.parametrize("fmt,K,nsplit", [("fp8", 96, 0), ("mxfp4", 192, 0), ("bf16", 96, 3), ("fp8", 128, 3), ("mxfp4", 256, 3)],
                         ids=["fp8_k_not_64", "mxfp4_k_not_128", "bf16_more_splits_than_chunks", "fp8_more_splits_than_chunks",
                              "mxfp4_more_splits_than_chunks"])
def test_gemv_refuses(dev, fmt, K, nsplit):
    M, N = 5, 80
    out = Canary(dev, M, N, BF, extra_cols=24)
    slab = Canary(dev, max(nsplit, 1) * M, N, torch.float32)
    x = torch.ones(M, K, dtype=BF, device=dev)
    rc = _gemm(dev, dict(fmt=fmt, N=N, K=K), "packed", x, M, out=out.view, ldc=out.ld, slab=slab.view if nsplit else None, nsplit=nsplit,
               weight=_zeros_weight(fmt, N, K, dev))
    assert rc != 0 and out.untouched() and slab.untouched()

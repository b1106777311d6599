"""CPU tier: which GEMM calls with MXFP4 weights are served by a tile kernel that stages the PACKED4 bytes itself (csrc/gemm.hip: W4Fused) and
which still dequantise into the scratch first.  Host logic only, through lcc_debug_gemm_w4_plan -- the decision lcc_gemm_w4_bf16 launches from.
The rule: the bf16 twin (the launch lcc_gemm_bf16 makes for the dequantised packed weight) decides; an 8-wave tile kernel reads the 4-bit bytes,
every other route dequantises."""
import pytest

from tests import test_gemm_routes as R

FUSED_CODES = {448, 272, 144, 256, 192, 128}      # tall, variable-height (big / small class), the 8-wave tile heights
SWIGLU = 4


@pytest.fixture
def knobs(built_lib):
    from livecc_amd import ops
    yield ops
    ops.set_gemm_variant(ops.GEMM_DEFAULT_VARIANT)
    ops.set_skinny_rows(64)
    ops.set_w4_fused(True)


def _grid():
    """Every (M, N, K, epilogue, nsplit) of the route table's grid that MXFP4 weights can have (whole 128-k fragments)."""
    return [(m, n, k, e, s) for m in R.MS for n, k in R.NKS if k % 128 == 0 for e, s in R.cases(n)]


@pytest.mark.parametrize("variant,rows", [tuple(k) for k in R.KNOBS])
def test_the_plan_is_the_bf16_twins_and_fused_exactly_on_the_8_wave_tile_kernels(knobs, variant, rows):
    ops = knobs
    ops.set_gemm_variant(variant)
    ops.set_skinny_rows(rows)
    seen = set()
    for m, n, k, e, s in _grid():
        code = ops.gemm_plan(m, n, k, e, nsplit=s)[0]
        got = ops.gemm_w4_plan(m, n, k, e, nsplit=s)
        if code == 0:
            assert got == (0, -1), (m, n, k, e, s, got)
            continue
        assert got[0] == code, (m, n, k, e, s, code, got)
        assert got[1] == (1 if code in FUSED_CODES else 0), (m, n, k, e, s, code, got)
        assert code in FUSED_CODES or code == 64 or code == 16, code
        seen.add((code, got[1]))
    if variant == 2 and rows == 64:
        assert {c for c, f in seen if f == 1} == FUSED_CODES and (64, 0) in seen and (16, 0) in seen      # every family occurs on the grid


def test_named_7b_shapes(knobs):
    ops = knobs
    assert ops.gemm_w4_plan(386, 37888, 3584, SWIGLU) == (448, 1)                    # gate|up of one streaming chunk: the tall kernel
    splits = ops.gemm_plan(386, 3584, 18944)[1]                                      # what the engine asks for with packed bf16 weights
    assert splits == 6 and ops.gemm_w4_plan(386, 3584, 18944, nsplit=splits) == (144, 1)      # down: the small variable-height class
    # the engine asks for the 128-row rule's split count with MXFP4 weights (as with fp8): those slabs are the 128-row tiles', fused as well
    s4 = ops.gemm_plan(386, 3584, 18944, w_fp8=True)[1]
    assert s4 == 4 and ops.gemm_w4_plan(386, 3584, 18944, nsplit=s4) == (128, 1)
    assert ops.gemm_w4_plan(3088, 37888, 3584, SWIGLU) == (272, 1)                   # gate|up of 8 chunks: variable-height tiles
    assert ops.gemm_w4_plan(40, 3584, 3584) == (16, 0)                               # 17..64 rows: the bf16 GEMV on the dequantised weight
    assert ops.gemm_w4_plan(8, 3584, 3584) == (16, 0)                                # M <= 16: gemv_wq_kernel, no scratch either
    assert ops.gemm_w4_plan(8, 3584, 3584, nsplit=4) == (16, 0)
    assert ops.gemm_w4_plan(8, 3584, 3584, nsplit=29) == (0, -1)                     # more splits than 128-k fragments
    assert ops.gemm_w4_plan(386, 3584, 3584 + 64) == (0, -1)                         # K % 128 != 0: LCC_ERR_SHAPE
    assert ops.gemm_w4_plan(386, 3584 + 8, 3584) == (0, -1)                          # N % 16 != 0


def test_the_knob_turns_every_fused_route_into_the_dequantising_one_and_leaves_the_tiles_alone(knobs):
    ops = knobs
    grid = [c for c in _grid() if c[0] in (8, 40, 386, 1131, 3088)]
    on = [ops.gemm_w4_plan(m, n, k, e, nsplit=s) for m, n, k, e, s in grid]
    assert any(f == 1 for _, f in on)
    ops.set_w4_fused(False)
    off = [ops.gemm_w4_plan(m, n, k, e, nsplit=s) for m, n, k, e, s in grid]
    assert [t for t, _ in off] == [t for t, _ in on]
    assert all(f == (-1 if t == 0 else 0) for t, f in off)
    ops.set_w4_fused(True)
    assert [ops.gemm_w4_plan(m, n, k, e, nsplit=s) for m, n, k, e, s in grid] == on


def test_abi_of_the_new_symbols(built_lib):
    import ctypes as C
    from livecc_amd import _lib, ops
    lib = built_lib
    out = (C.c_int32 * 2)()
    p0, p1 = C.addressof(out), C.addressof(out) + 4
    assert lib.lcc_debug_gemm_w4_plan(386, 3584, 3584, 0, 0, None, p1) == _LCC_ERR_ARG
    assert lib.lcc_debug_gemm_w4_plan(386, 3584, 3584, 0, 0, p0, None) == _LCC_ERR_ARG
    assert b"lcc_debug_gemm_w4_plan" in lib.lcc_last_error()
    assert lib.lcc_debug_gemm_w4_plan(0, 3584, 3584, 0, 0, p0, p1) == _LCC_ERR_ARG
    assert lib.lcc_debug_gemm_w4_plan(386, 37888, 3584, SWIGLU, 0, p0, p1) == 0 and (out[0], out[1]) == (448, 1)
    # the knob is process-global routing state like its siblings: the same signature, 0 when no model-level call is in flight (a refusal is
    # LCC_ERR_STATE from the guard they share: tests/test_gpu_server.py exercises that guard under load)
    sig = lib._lcc_signatures
    assert sig["lcc_debug_set_w4_fused"] == sig["lcc_debug_set_gemm_variant"]
    assert lib.lcc_debug_set_w4_fused(0) == 0 and lib.lcc_debug_set_w4_fused(1) == 0
    assert ops.LAUNCH_COUNTERS[17:19] == ("gemm_w4_fused", "gemm_w4_dequant") and len(ops.LAUNCH_COUNTERS) == 19
    counts = ops.launch_counts()
    assert counts["gemm_w4_fused"] >= 0 and counts["gemm_w4_dequant"] >= 0
    big = (C.c_int64 * 20)()
    assert lib.lcc_debug_launch_counts(C.addressof(big), 19, 0) == 0
    assert lib.lcc_debug_launch_counts(C.addressof(big), 20, 0) == _LCC_ERR_ARG      # there are 19 counters
    assert "lcc_debug_gemm_w4_plan" in _lib.declared_symbols() and "lcc_debug_set_w4_fused" in _lib.declared_symbols()


_LCC_ERR_ARG = -1

"""CPU tier: which decode calls take the fused attention + key-split merge + o_proj launch (csrc/decode_v2.hip: attn_o_kernel).  Host logic
only, through lcc_debug_attn_o_plan -- the same predicate lcc_llm_decode decides with (there the block capacity comes from the runtime's
occupancy query; here it is one 512-thread block per CU of the `cu_count` given)."""
import pytest

from livecc_amd import ops

B7 = dict(n_q_heads=28, n_kv_heads=4, head_dim=128, hidden=3584)          # LiveCC-7B
B2 = dict(n_q_heads=12, n_kv_heads=2, head_dim=128, hidden=1536)          # 2B-like
B72 = dict(n_q_heads=64, n_kv_heads=8, head_dim=128, hidden=8192)         # 72B: 8 query heads per KV head


@pytest.fixture
def fused_on():
    old = ops.set_attn_o_fused(True)
    assert old in (0, 1)
    yield
    ops.set_attn_o_fused(bool(old))


@pytest.mark.parametrize("max_kv,want", [(1, 1), (128, 1), (129, 2), (4096, 32), (4097, 33), (6000, 47), (8192, 64), (8193, 64), (20000, 64)])
def test_key_splits_follow_the_cache_length(fused_on, max_kv, want):
    """4 key tiles of 32 keys per split, at most 64 splits (the defaults of LCC_ATTN_TPS / LCC_ATTN_MAXSPLIT)."""
    assert ops.attn_o_plan(1, max_kv=max_kv, **B7)[1] == want


@pytest.mark.parametrize("name,kw,want", [
    ("7B one stream, 1,000 keys: 4 x 8 + 224 = 256 blocks, one per CU", dict(n_streams=1, max_kv=1000, **B7), True),
    ("7B one stream, 1,100 keys: 4 x 9 + 224 > 256", dict(n_streams=1, max_kv=1100, **B7), False),
    ("7B one stream, 6k keys (the benchmark's cache): 188 + 224 blocks do not fit", dict(n_streams=1, max_kv=6000, **B7), False),
    ("7B two streams, 500 keys: 2 x 4 x 4 + 224", dict(n_streams=2, max_kv=500, **B7), True),
    ("three streams keep the round-1 sequence", dict(n_streams=3, max_kv=500, **B7), False),
    ("fp8 weights", dict(n_streams=1, max_kv=1000, w_fp8=True, **B7), False),
    ("parity taps bound", dict(n_streams=1, max_kv=1000, taps_bound=True, **B7), False),
    ("72B: 8 query heads per KV head, 7 merging waves", dict(n_streams=1, max_kv=500, **B72), False),
    ("2B-like, one stream, 6k keys: 2 x 47 + 96", dict(n_streams=1, max_kv=6000, **B2), True),
    ("2B-like, two streams, 6k keys: 188 + 96 > 256", dict(n_streams=2, max_kv=6000, **B2), False),
    ("half the chip: the 224 o_proj blocks alone exceed 128", dict(n_streams=1, max_kv=100, cu_count=128, **B7), False),
])
def test_fused_route_eligibility(fused_on, name, kw, want):
    assert ops.attn_o_plan(**kw)[0] is want, name


def test_switch_off_means_three_launches():
    old = ops.set_attn_o_fused(False)
    try:
        assert ops.attn_o_plan(1, max_kv=1000, **B7) == (False, 8)
        assert ops.set_attn_o_fused(True) == 0
        assert ops.attn_o_plan(1, max_kv=1000, **B7) == (True, 8)
    finally:
        ops.set_attn_o_fused(bool(old))


def test_resid_waves_mode_2_keeps_the_three_launches(fused_on):
    """16-wave o_proj blocks for every call = another fp32 summation order than the fused launch's 8-wave o_proj part."""
    from livecc_amd import _lib
    old = _lib.load().lcc_debug_set_resid_waves(2)
    try:
        assert ops.attn_o_plan(1, max_kv=1000, **B7)[0] is False
        _lib.load().lcc_debug_set_resid_waves(1)
        assert ops.attn_o_plan(1, max_kv=1000, **B7)[0] is True
    finally:
        _lib.load().lcc_debug_set_resid_waves(old)


def test_launch_counter_is_exposed():
    assert ops.LAUNCH_COUNTERS[16] == "attn_o_fused" and ops.launch_counts()["attn_o_fused"] >= 0

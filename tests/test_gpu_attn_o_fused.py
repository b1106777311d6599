"""-m gpu: the fused decode launch (attention + key-split merge + o_proj, csrc/decode_v2.hip: attn_o_kernel) against the three launches
it replaces.  Same wave-level arithmetic in the same order, so every comparison is exact equality."""
import pytest
import torch

from tests.test_gpu_ops import _rand

pytestmark = pytest.mark.gpu


def _nsplit(n_keys):
    """The engine's rule (lcc_llm_decode): 4 key tiles of 32 keys per split, at most 64 splits."""
    return max(1, min(64, ((n_keys + 31) // 32 + 3) // 4))


# cached keys per stream, one entry per stream (the new token is one more key).  A block owns a CU, so streams x KV heads x splits + H/16
# must stay within the CU count: the long caches run at the small shape (7 query heads on 1 KV head, H = 896: 56 o_proj blocks), where
# 4095 | 4096 cached keys are 32 | 33 splits (the merge's second pass over its 8 groups has 0 | 1 live group in the last round) and 12.5k keys
# are 64 splits of 7 key tiles; 7B shapes run up to 8 splits for one stream (32 + 224 blocks), the 2B-like shape at 47 and 2 x 18.
CASES = [
    (7, 1, 896, (4095,)), (7, 1, 896, (4096,)), (7, 1, 896, (12500,)), (7, 1, 896, (4095, 37)), (7, 1, 896, (4096, 4000)), (7, 1, 896, (12500, 300)),
    (7, 1, 896, (300, 37)), (28, 4, 3584, (37,)), (28, 4, 3584, (1000,)), (28, 4, 3584, (700,)), (28, 4, 3584, (37, 100)), (28, 4, 3584, (500, 260)),
    (12, 2, 1536, (6000,)), (12, 2, 1536, (2200, 700)), (2, 1, 256, (1000, 5)),
]


@pytest.mark.parametrize("Hq,Hkv,H,lens", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fused_launch_is_bit_identical_to_attention_combine_and_o_proj(dev, request, Hq, Hkv, H, lens):
    """attn rows, residual stream after o_proj and its tile statistics of lcc_dgemv_attn_o == lcc_attn_decode_bf16 + lcc_dgemv_resid, one and
    two streams, on both sides of a split-count change (32 | 33) and at 64 splits of 7 tiles (> 12k keys) at the small shape, up to 8 splits
    at 7B shapes.  20 launches on ONE monotonic counter with fresh q / h each time (an o_proj block that read a stale or half-published
    head row would reproduce other values); the tickets end at zero, the counter at its target, the error word stays clear.  Every case
    must RUN the kernel: a case that does not fit the chip fails here (the refusal has its own test below)."""
    from livecc_amd import _lib, ops
    lens, M = list(lens), len(lens)
    lmax = (max(lens) + 1 + 31) // 32 * 32
    nsplit = _nsplit(max(lens) + 1)
    assert M * Hkv * nsplit + H // 16 <= torch.cuda.get_device_properties(dev).multi_processor_count, "case does not fit one block per CU"
    old_mode = _lib.load().lcc_debug_set_resid_waves(0)         # o_proj of the fused launch = the 8-wave block shape
    request.addfinalizer(lambda: _lib.load().lcc_debug_set_resid_waves(old_mode))
    state = dict(tickets=torch.zeros(256, dtype=torch.int32, device=dev), counter=torch.zeros(1, dtype=torch.int32, device=dev),
                 err=torch.zeros(1, dtype=torch.int32, device=dev), before=0)
    ops.launch_counts(reset=True)
    for it in range(20):
        _run_once(dev, ops, Hq, Hkv, H, lens, lmax, nsplit, it, state)
    c = ops.launch_counts()
    assert c["attn_o_fused"] == 20 and c["last_decode_nsplit"] == nsplit
    assert int(state["tickets"].abs().sum()) == 0, "the last-arriving block leaves its ticket counter at zero"


@pytest.mark.parametrize("Hq,Hkv,H,lens,mode", [(28, 4, 3584, (4095,), 0), (28, 4, 3584, (1000, 900), 0), (12, 2, 1536, (6000, 6000), 0),
                                                (7, 1, 896, (300,), 2)])
def test_operator_refuses_what_the_engine_sends_to_the_three_launches(dev, request, Hq, Hkv, H, lens, mode):
    """LCC_ERR_STATE, nothing launched: attention + o_proj blocks beyond one per CU (7B at 32 splits, 7B two streams at 8, 2B-like two streams
    at 47), and resid-waves mode 2 (the stand-alone o_proj then has 16-wave blocks and another summation order than the fused launch's)."""
    from livecc_amd import _lib, ops
    old_mode = _lib.load().lcc_debug_set_resid_waves(mode)
    request.addfinalizer(lambda: _lib.load().lcc_debug_set_resid_waves(old_mode))
    lens = list(lens)
    ops.launch_counts(reset=True)
    with pytest.raises(RuntimeError, match=r"\(-5\)"):
        _run_once(dev, ops, Hq, Hkv, H, lens, (max(lens) + 32) // 32 * 32, _nsplit(max(lens) + 1), 0, None)
    assert ops.launch_counts()["attn_o_fused"] == 0


def _run_once(dev, ops, Hq, Hkv, H, lens, lmax, nsplit, it, state):
    M, K = len(lens), Hq * 128
    if state is None or it == 0:
        kv = ops.KvArena(M, 2, Hkv, lmax, dev)
        g = torch.Generator(device=dev).manual_seed(5)
        kv.buf.copy_((torch.randn(kv.buf.shape, generator=g, device=dev) * 0.5).to(torch.bfloat16))
        w_o = ops.pack_weight(_rand((H, K), dev, 0.03, 51))
        if state is None:
            state = dict(tickets=torch.zeros(256, dtype=torch.int32, device=dev), counter=torch.zeros(1, dtype=torch.int32, device=dev),
                         err=torch.zeros(1, dtype=torch.int32, device=dev), before=0)
        state["kv"], state["w_o"] = kv, w_o
    kv, w_o = state["kv"], state["w_o"]
    slots = torch.arange(M, dtype=torch.int32, device=dev).flip(0).contiguous()           # row m -> slot M-1-m
    kv_len = torch.zeros(M, dtype=torch.int32, device=dev)
    kv_len[slots.long()] = torch.tensor(lens, dtype=torch.int32, device=dev)
    q, h0 = _rand((M, K), dev, 1.0, 100 + it), _rand((M, H), dev, 2.0, 200 + it)
    layer = 1
    # the three launches
    attn_ref = ops.attn_decode(q, kv, layer, slots, kv_len, Hq, nsplit)
    h_ref = h0.clone()
    st_ref = ops.dgemv_resid_(w_o, attn_ref, h_ref, (H, K))
    # the fused launch
    h = h0.clone()
    attn, st = ops.dgemv_attn_o_(q, kv, layer, slots, kv_len, Hq, nsplit, w_o, h, state["tickets"], state["counter"], state["before"], state["err"])
    state["before"] += M * Hkv
    assert int(state["err"][0]) == 0, "an o_proj block gave up waiting"
    assert int(state["counter"][0]) == state["before"]
    assert torch.equal(attn, attn_ref), f"iteration {it}: merged attention rows differ"
    assert torch.equal(h, h_ref), f"iteration {it}: residual stream after o_proj differs (stale head row?)"
    assert torch.equal(st, st_ref), f"iteration {it}: tile statistics differ"


@pytest.fixture(scope="module")
def small_native(dev):
    from livecc_amd.config import small
    from livecc_amd.modeling import LiveCCForConditionalGeneration
    from oracle import hf_oracle as O
    cfg = small()
    hf16 = O.build_hf_model(cfg, dtype=torch.bfloat16, seed=4, init_scale=1.5)
    return cfg, LiveCCForConditionalGeneration.from_hf_model(hf16, cfg, dev, max_streams=4, max_kv_len=4096, max_new_rows=2048,
                                                             max_patches=8192, max_history=64)


def test_two_turn_generate_is_bit_identical_with_the_switch_on_and_off(dev, small_native):
    """Small config (7 query heads per KV head), two streaming turns per run, the switch 0 / 1 / 1 / 0 on ONE engine: tokens and raw logits
    of every step are equal, the fused kernel ran exactly when it was switched on (once per layer and decode step), and no call failed
    on the hand-off error word (lcc_slot_read_tokens checks it after every generate)."""
    from livecc_amd import ops, protocol
    from tests.test_gpu_e2e import _replay_native
    cfg, native = small_native
    frames = torch.from_numpy(protocol.synth_frames(8, 56, 84, seed=77, layout="TCHW"))
    n_tok, L = 8, cfg.num_hidden_layers
    outs = []
    old = ops.set_attn_o_fused(False)
    try:
        for on in (0, 1, 1, 0):
            ops.set_attn_o_fused(bool(on))
            ops.launch_counts(reset=True)
            outs.append(_replay_native(native, cfg, frames, protocol.TurnBuilder(cfg, seed=77), max_new_tokens=n_tok, repetition_penalty=1.05,
                                       max_turns=2))
            c = ops.launch_counts(reset=True)
            turns = len(outs[-1])
            assert turns == 2
            assert c["attn_o_fused"] == (turns * (n_tok - 1) * L if on else 0), (on, c)
            assert c["attn_decode_combine"] == (0 if on else turns * (n_tok - 1) * L), (on, c)
    finally:
        ops.set_attn_o_fused(bool(old))
    for o in outs[1:]:
        for ta, tb in zip(outs[0], o):
            assert ta["new_tokens"] == tb["new_tokens"]
            assert torch.equal(ta["logits"], tb["logits"]), "fused and separate launches must be bit-identical"

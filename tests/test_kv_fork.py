"""KV fork, host side (CPU tier): the numpy statement of the copy contract (the expected-value generator of
tests/test_gpu_kv_fork.py), the error paths of `lcc_kv_copy_bf16` (argument validation comes before any device work), and
`StreamState.fork` / `LiveCCDemoInfer.mcq_predict_many` / `LiveCCDemoInfer.ask` over stand-in models that record what reaches the
engine."""
import threading

import numpy as np
import pytest
import torch

from livecc_amd import infer as I, protocol
from livecc_amd.config import tiny
from livecc_amd.modeling import GenerateOutput, StreamState
from tests.test_kv_window import v_blocked, v_natural


# ---- 1. the contract in numpy ---------------------------------------------------------------------------------------------------
def fork_arena_numpy(src: np.ndarray, dst: np.ndarray, layers: int, hkv: int, lmax: int, n: int) -> np.ndarray:
    """Expected destination arena (uint16 bit patterns, [layer][K|V][Hkv][lmax * 128]) after copying the first n rows of `src` into
    `dst`: in every K and V plane rows [0, n) are the source's, rows [n, ceil32(n)) are zero, rows at or above ceil32(n) stay."""
    s = src.reshape(layers, 2, hkv, lmax * 128)
    d = dst.reshape(layers, 2, hkv, lmax * 128).copy()
    up = (n + 31) // 32 * 32
    for l in range(layers):
        for h in range(hkv):
            k = d[l, 0, h].reshape(lmax, 128)
            k[:n] = s[l, 0, h].reshape(lmax, 128)[:n]
            k[n:up] = 0
            nat = v_natural(d[l, 1, h].reshape(lmax // 32, 128, 32))
            nat[:n] = v_natural(s[l, 1, h].reshape(lmax // 32, 128, 32))[:n]
            nat[n:up] = 0
            d[l, 1, h] = v_blocked(nat).reshape(-1)
    return d.reshape(dst.shape)


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 31, 32, 33, 64])
def test_fork_arena_numpy_states_the_contract(n):
    rng = np.random.default_rng(n)
    layers, hkv, lmax = 2, 2, 64
    numel = layers * 2 * hkv * lmax * 128
    src = rng.integers(1, 65536, numel).astype(np.uint16)
    dst = rng.integers(1, 65536, numel).astype(np.uint16)
    src0, dst0 = src.copy(), dst.copy()
    out = fork_arena_numpy(src, dst, layers, hkv, lmax, n)
    assert np.array_equal(src, src0) and np.array_equal(dst, dst0), "the inputs are not written"
    up = (n + 31) // 32 * 32
    o4, s4, d4 = (x.reshape(layers, 2, hkv, lmax * 128) for x in (out, src0, dst0))
    for l in range(layers):
        for h in range(hkv):
            for kv, nat in ((0, lambda x: x.reshape(lmax, 128)), (1, lambda x: v_natural(x.reshape(lmax // 32, 128, 32)))):
                o, s, d = nat(o4[l, kv, h]), nat(s4[l, kv, h]), nat(d4[l, kv, h])
                assert np.array_equal(o[:n], s[:n]) and not o[n:up].any() and np.array_equal(o[up:], d[up:])
    # stated on the BLOCKED V layout, index by index: key j = (block j // 32, column j % 32)
    vb_o, vb_s = o4[1, 1, 1].reshape(lmax // 32, 128, 32), s4[1, 1, 1].reshape(lmax // 32, 128, 32)
    for j in range(up):
        want = vb_s[j // 32, :, j % 32] if j < n else 0
        assert np.array_equal(vb_o[j // 32, :, j % 32], np.broadcast_to(want, (128,)))


# ---- 2. lcc_kv_copy_bf16: every refusal, without a GPU ----------------------------------------------------------------------------
def test_kv_copy_error_codes_without_a_gpu(built_lib):
    from livecc_amd import _lib
    lib = built_lib
    ARG, SHAPE, ALIGN, STATE = -1, -2, -3, -5
    ok = _lib.KvLayout(2, 1, 256, 128)
    bytes_ = 2 * 2 * 1 * 256 * 128 * 2
    A, B = 1 << 30, (1 << 30) + bytes_          # dummy aligned addresses of two adjacent arenas: nothing may be dereferenced
    cases = [
        (None, A, ok, 10, ARG), (A, None, ok, 10, ARG),
        (B + 2, A, ok, 10, ALIGN), (B, A + 8, ok, 10, ALIGN),
        (B, A, _lib.KvLayout(2, 1, 256, 64), 10, SHAPE), (B, A, _lib.KvLayout(2, 1, 250, 128), 10, SHAPE),
        (B, A, _lib.KvLayout(2, 1, 0, 128), 0, SHAPE), (B, A, _lib.KvLayout(0, 1, 256, 128), 10, SHAPE),
        (B, A, _lib.KvLayout(2, 0, 256, 128), 10, SHAPE),
        (B, A, ok, -1, STATE), (B, A, ok, 257, STATE),
        (A, A, ok, 10, ARG), (A + 16, A, ok, 10, ARG), (A, A + bytes_ - 16, ok, 10, ARG), (B - 16, A, ok, 0, ARG),
    ]
    for dst, src, lay, n, code in cases:
        assert lib.lcc_kv_copy_bf16(dst, src, lay, n, None) == code, (dst, src, n, code)
        assert lib.lcc_last_error() != b""
    assert lib.lcc_kv_copy_bf16(B, A, ok, 0, None) == 0, "n_rows == 0 succeeds and launches nothing"
    assert lib.lcc_kv_copy_bf16(A, B, ok, 0, None) == 0


# ---- stand-in model: records what reaches the engine ------------------------------------------------------------------------------
class _Engine:
    max_history = 512

    def __init__(self, max_slots):
        self.max_slots = max_slots
        self.len = {s: 0 for s in range(max_slots)}
        self.forks = []
        self.fail_fork = False

    def slot_length(self, slot):
        return self.len[slot], 0

    def fork_slot(self, src, dst):
        if self.fail_fork:
            raise RuntimeError("fork_slot failed")
        self.forks.append((src, dst))
        self.len[dst] = self.len[src]


class ForkModel:
    DECODE_GROUP = 64

    def __init__(self, cfg=None, max_streams=4):
        self.cfg = cfg or tiny()
        self.device = torch.device("cpu")
        self.engine = _Engine(max_streams)
        self._free_slots = list(range(max_streams - 1, -1, -1))
        self._lock = threading.RLock()
        self.eos_token_ids = [self.cfg.eos_token_id]
        self.generation_config = {}
        self.calls = []                  # one entry per generate_batch call: a list of per-request records
        self.fail_batches_of = None      # raise in a generate_batch call of this many requests

    def new_stream(self):
        if not self._free_slots:
            raise RuntimeError(f"all {self.engine.max_slots} stream slots are in use (raise max_streams)")
        st = StreamState(self, self._free_slots.pop())
        self.engine.len[st.slot] = 0
        return st

    def generate_batch(self, requests, max_new_tokens=16, output_logits=False, **kw):
        if self.fail_batches_of == len(requests):
            raise RuntimeError("generate_batch failed")
        outs, rec = [], []
        for rq in requests:
            st = rq.get("state") or self.new_stream()
            assert not st.released
            ids = torch.as_tensor(rq["input_ids"]).reshape(-1)
            past = st.get_seq_length()
            assert len(ids) > past
            seq = torch.cat([ids, torch.arange(max_new_tokens) + 7])
            self.engine.len[st.slot] = len(seq) - 1
            rec.append(dict(ids=ids.numpy().copy(), past=past, frames=rq.get("frames"), slot=st.slot, kw=dict(kw, max_new_tokens=max_new_tokens,
                                                                                                           output_logits=output_logits)))
            lg = None
            if output_logits:
                lg = torch.zeros(max_new_tokens, self.cfg.vocab_size)
                lg[0, int(ids.sum()) % self.cfg.vocab_size] = 1.0
            outs.append(GenerateOutput(sequences=seq.view(1, -1), past_key_values=st, logits=lg))
        self.calls.append(rec)
        return outs

    def generate(self, input_ids=None, frames=None, past_key_values=None, max_new_tokens=16, output_logits=False, frames_layout="TCHW", **kw):
        return self.generate_batch([dict(input_ids=input_ids[0], frames=frames, state=past_key_values)], max_new_tokens=max_new_tokens,
                                   output_logits=output_logits, **kw)[0]


# ---- 3. StreamState.fork ------------------------------------------------------------------------------------------------------------
def test_stream_state_fork_slot_accounting():
    m = ForkModel(max_streams=3)
    a = m.new_stream()
    a.rope_delta = -37
    m.engine.len[a.slot] = 100
    b = a.fork()
    assert isinstance(b, StreamState) and b.slot != a.slot and not b.released and b.model is m
    assert m.engine.forks == [(a.slot, b.slot)] and b.rope_delta == -37 and b.get_seq_length() == 100
    assert sorted(m._free_slots + [a.slot, b.slot]) == [0, 1, 2] and len(m._free_slots) == 1
    c = b.fork()                                         # a fork of a fork; the last slot
    assert m.engine.forks[-1] == (b.slot, c.slot) and m._free_slots == []
    with pytest.raises(RuntimeError, match="stream slots are in use"):
        a.fork()                                         # no free slot: the error of new_stream, nothing leaked, nothing forked
    assert m._free_slots == [] and len(m.engine.forks) == 2
    c.release()
    assert m._free_slots == [c.slot]
    with pytest.raises(ValueError):
        c.fork()                                         # a released source
    assert m._free_slots == [c.slot] and len(m.engine.forks) == 2
    m.engine.fail_fork = True
    with pytest.raises(RuntimeError, match="fork_slot failed"):
        a.fork()                                         # a failing fork_slot gives the slot back
    assert m._free_slots == [c.slot] and not a.released and a.rope_delta == -37
    b.release(); a.release()
    assert sorted(m._free_slots) == [0, 1, 2]


# ---- 4. mcq_predict_many ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text_cfg(tmp_path_factory):
    import dataclasses
    from livecc_amd.text import TextFrontEnd
    from tests.test_text import make_tokenizer_dir
    fe0 = TextFrontEnd(make_tokenizer_dir(tmp_path_factory.mktemp("tok_fork")))
    tk = fe0.tokenizer
    cfg = dataclasses.replace(tiny(), video_token_id=fe0.video_token_id, eos_token_id=fe0.eos_token_id,
                              image_token_id=tk.convert_tokens_to_ids("<|image_pad|>"),
                              vision_start_token_id=tk.convert_tokens_to_ids("<|vision_start|>"),
                              vision_end_token_id=tk.convert_tokens_to_ids("<|vision_end|>"),
                              bos_token_id=tk.convert_tokens_to_ids("<|endoftext|>"))
    return tk, cfg


ITEMS = [("what is happening now?", ["A. system", "B. user", "C. assistant", "D. video"]),
         ("now?", ["A. 0", "B. 1", "C. 2", "D. 3"], "Time=0.0-3.0s livecc ... Time=12.5-13.5s user"),
         ("Please describe the video. what is happening now? ...", ["A. a helpful assistant", "B. livecc", "C. =-.", "D. 0123456789"])]


def _one_shot_ids(infer, clip, item):
    """The ids `mcq_predict` sends for one question, read off the stand-in."""
    m = infer.model
    before = len(m.calls)
    infer.mcq_predict(clip, item[0], item[1], subtitles=item[2] if len(item) == 3 else None)
    assert len(m.calls) == before + 1 and len(m.calls[-1]) == 1
    return m.calls[-1][0]["ids"]


@pytest.mark.parametrize("max_streams", [4, 3, 2])
def test_mcq_predict_many_prefills_the_clip_once_and_forks_per_question(text_cfg, max_streams):
    from livecc_amd.text import TextFrontEnd
    tk, cfg = text_cfg
    m = ForkModel(cfg, max_streams=max_streams)
    infer = I.LiveCCDemoInfer(model=m, text=TextFrontEnd(tk, cfg))
    clip = torch.zeros(4, 3, 56, 84, dtype=torch.uint8)
    want_ids = [_one_shot_ids(infer, clip, it) for it in ITEMS]
    assert len({len(x) for x in want_ids}) == 3, "three questions of different lengths"
    assert sorted(m._free_slots) == list(range(max_streams))
    m.calls.clear()
    res = infer.mcq_predict_many(clip, ITEMS)
    assert len(res) == 3 and all(0 <= c < 4 and lg.shape == (4,) for c, lg in res)
    with_frames = [r for call in m.calls for r in call if r["frames"] is not None]
    assert len(with_frames) == 1 and m.calls[0] == [with_frames[0]], "exactly one call carries frames: the first, alone"
    prefix = with_frames[0]["ids"]
    assert prefix[-1] == cfg.vision_end_token_id and with_frames[0]["past"] == 0 and with_frames[0]["kw"]["max_new_tokens"] == 1
    base_slot = with_frames[0]["slot"]
    assert len(m.engine.forks) == 3 and all(s == base_slot and d != base_slot for s, d in m.engine.forks)
    tails = m.calls[1:]
    waves = -(-3 // (max_streams - 1))
    assert len(tails) == waves, "one batched tail call per wave of free slots (one call when every question has a slot)"
    recs = [r for call in tails for r in call]
    assert len(recs) == 3 and all(r["frames"] is None and r["past"] == len(prefix) for r in recs)
    assert all(r["kw"]["max_new_tokens"] == 1 and r["kw"]["output_logits"] and r["kw"]["repetition_penalty"] == 1.0 for r in recs)
    assert [r["slot"] for r in recs] == [d for _, d in m.engine.forks]
    for r, want in zip(recs, want_ids):
        assert np.array_equal(r["ids"], want), "prefix + tail are the ids mcq_predict sends"
        assert np.array_equal(r["ids"][:len(prefix)], prefix) and len(r["ids"]) > len(prefix)
    assert sorted(m._free_slots) == list(range(max_streams)), "every fork and the prefix stream are released"
    # the restricted logits are those of the question's own output, in item order
    letter_ids = [tk(f": {x}").input_ids[-1] for x in "ABCD"]
    for (c, lg), want in zip(res, want_ids):
        hot = int(want.sum()) % cfg.vocab_size
        assert lg.tolist() == [1.0 if t == hot else 0.0 for t in letter_ids]


def test_mcq_predict_many_releases_everything_when_the_tail_call_raises(text_cfg):
    from livecc_amd.text import TextFrontEnd
    tk, cfg = text_cfg
    m = ForkModel(cfg, max_streams=4)
    infer = I.LiveCCDemoInfer(model=m, text=TextFrontEnd(tk, cfg))
    clip = torch.zeros(4, 3, 56, 84, dtype=torch.uint8)
    m.fail_batches_of = 3
    with pytest.raises(RuntimeError, match="generate_batch failed"):
        infer.mcq_predict_many(clip, ITEMS)
    assert sorted(m._free_slots) == [0, 1, 2, 3] and len(m.engine.forks) == 3
    m.fail_batches_of = 1                                    # ... and when the prefix prefill itself raises
    with pytest.raises(RuntimeError, match="generate_batch failed"):
        infer.mcq_predict_many(clip, ITEMS)
    assert sorted(m._free_slots) == [0, 1, 2, 3]
    m.fail_batches_of = None
    assert infer.mcq_predict_many(clip, []) == []


def test_mcq_predict_many_needs_a_slot_to_fork_into(text_cfg):
    from livecc_amd.text import TextFrontEnd
    tk, cfg = text_cfg
    m = ForkModel(cfg, max_streams=1)
    infer = I.LiveCCDemoInfer(model=m, text=TextFrontEnd(tk, cfg))
    clip = torch.zeros(4, 3, 56, 84, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="max_streams"):
        infer.mcq_predict_many(clip, ITEMS)
    assert m._free_slots == [0] and m.calls == []
    with pytest.raises(ValueError):
        infer.mcq_predict_many(None, ITEMS)
    with pytest.raises(ValueError):
        I.LiveCCDemoInfer(model=ForkModel(cfg)).mcq_predict_many(clip, ITEMS)      # no tokenizer


# ---- 5. ask -------------------------------------------------------------------------------------------------------------------------
def _snapshot(state):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] is b[k] or a[k] == b[k], k


@pytest.mark.parametrize("mode", ["synthetic", "text"])
def test_ask_leaves_the_state_alone_and_releases_the_fork(text_cfg, mode):
    from livecc_amd.text import TextFrontEnd
    tk, cfg = text_cfg
    if mode == "synthetic":
        cfg = tiny()                       # (the synthetic builder draws its text ids below the special ids of the model config)
    m = ForkModel(cfg, max_streams=2)
    infer = I.LiveCCDemoInfer(model=m, text=TextFrontEnd(tk, cfg) if mode == "text" else None)
    state = {}
    clip = torch.zeros(8, 3, 56, 84, dtype=torch.uint8)
    for _ in infer.live_cc_clip(clip, state, max_new_tokens=4, message="what is happening now?" if mode == "text" else None):
        pass
    assert state["turn_index"] == 2 and len(m._free_slots) == 1
    before = _snapshot(state)
    src_len = m.engine.len[state["past_key_values"].slot]
    builder = (infer.turn_builder.query_len, infer.turn_builder._rng.get_state()[1].copy())
    n_calls, n_gen = len(m.calls), len(infer.last_generated)
    resp = infer.ask("and now?" if mode == "text" else 16, state, max_new_tokens=5)
    assert isinstance(resp, str)
    _same(before, state)
    assert state["past_key_values"] is before["past_key_values"] and not state["past_key_values"].released
    assert m.engine.len[state["past_key_values"].slot] == src_len and len(m._free_slots) == 1, "the fork is released, the stream is not"
    assert infer.turn_builder.query_len == builder[0] and np.array_equal(infer.turn_builder._rng.get_state()[1], builder[1])
    assert len(m.calls) == n_calls + 1
    r = m.calls[-1][0]
    fork_slot = m.engine.forks[-1][1]
    assert m.engine.forks == [(state["past_key_values"].slot, fork_slot)] and r["slot"] == fork_slot and r["frames"] is None
    assert r["past"] == len(state["past_ids"]) and np.array_equal(r["ids"][:r["past"]], state["past_ids"]) and r["kw"]["max_new_tokens"] == 5
    tail = r["ids"][r["past"]:]
    assert tail[0] == cfg.eos_token_id and cfg.video_token_id not in tail, "the continuing text turn: '<|im_end|>\\n' + the turn, no video"
    if mode == "text":
        assert tk.decode(tail.tolist(), skip_special_tokens=False) == "<|im_end|>\n<|im_start|>user\nand now?<|im_end|>\n<|im_start|>assistant\n"
    else:
        assert len(tail) == 2 + 3 + 10 + 16 + 5
    assert len(infer.last_generated) == n_gen + 1 and infer.last_generated[-1]["tokens"] == [7, 8, 9, 10, 11]
    assert np.array_equal(infer.last_generated[-1]["prompt_ids"], tail)
    # a failing generate still releases the fork and leaves the state alone
    m.fail_batches_of = 1
    with pytest.raises(RuntimeError, match="generate_batch failed"):
        infer.ask("and now?" if mode == "text" else 16, state)
    _same(before, state)
    assert len(m._free_slots) == 1
    state["past_key_values"].release()


def test_ask_needs_a_cache():
    infer = I.LiveCCDemoInfer(model=ForkModel(tiny()))
    with pytest.raises(ValueError):
        infer.ask(16, {})
    with pytest.raises(ValueError):
        infer.ask(16, {"past_ids": np.arange(5), "past_key_values": None})
    st = infer.model.new_stream()
    with pytest.raises(ValueError):
        infer.ask("a string without a tokenizer", {"past_ids": np.arange(5), "past_key_values": st})
    assert len(infer.model._free_slots) == 3 and infer.model.engine.forks == [], "refused before anything was forked"
    st.release()

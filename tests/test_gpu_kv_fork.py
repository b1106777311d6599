"""-m gpu: the KV fork -- the copy kernel (csrc/kv_copy.hip) bit for bit against the numpy statement of the arena layout
(tests/test_kv_fork.py), its refusals, `StreamState.fork` against the engine itself (same kernels on the same bytes: every
comparison is `torch.equal`), `mcq_predict_many` against the HF oracle under the bound of the one-question test, and `ask` on the
side of a commentary stream."""
import numpy as np
import pytest
import torch

from tests.test_gpu_kv_window import _Replay
from tests.test_kv_fork import ITEMS, fork_arena_numpy
from tests.test_kv_window import v_natural

pytestmark = pytest.mark.gpu


# ---- A. kernel, bit-exact -----------------------------------------------------------------------------------------------------------
LAYOUTS = {"tiny": (2, 1), "gqa2": (3, 2), "7b": (28, 4)}      # (n_layers, n_kv_heads) of the arena
KERNEL_CASES = [("tiny", 256, n) for n in (1, 7, 8, 9, 31, 32, 33)] + [
    ("tiny", 1024, 1024),      # n == lmax: the last block is full
    ("gqa2", 256, 250),        # two KV heads, a partial last block that is also the arena's last
    ("7b", 4096, 4001),        # 224 planes, several blocks per workgroup
    ("tiny", 256, 0),          # nothing to copy: nothing launched
]


def _arena(lay, lmax, dev, seed, guard):
    """[guard | arena | guard] of random bf16 bit patterns (NaN / inf / denormal patterns included: the op is a copy)."""
    n = lay[0] * 2 * lay[1] * lmax * 128
    g = torch.Generator(device=dev).manual_seed(seed)
    buf = torch.randint(-32768, 32768, (guard + n + guard,), dtype=torch.int32, device=dev, generator=g).to(torch.int16)
    return buf, n


@pytest.mark.parametrize("name,lmax,n", KERNEL_CASES)
def test_kv_copy_kernel_is_a_bit_exact_copy(dev, name, lmax, n):
    from livecc_amd import _lib
    lib = _lib.load()
    lay = LAYOUTS[name]
    guard = lay[0] * 2 * lay[1] * lmax * 128 if name != "7b" else 4 << 20
    sbuf, numel = _arena(lay, lmax, dev, seed=1000 + n, guard=guard)
    dbuf, _ = _arena(lay, lmax, dev, seed=2000 + n, guard=guard)
    assert sbuf.data_ptr() % 256 == 0 and dbuf.data_ptr() % 256 == 0 and (guard * 2) % 256 == 0
    s0, d0 = sbuf.cpu().numpy().view(np.uint16), dbuf.cpu().numpy().view(np.uint16)
    assert np.isnan(torch.from_numpy(s0[guard:guard + 4096].view(np.int16).copy()).view(torch.bfloat16).float().numpy()).any()
    want = d0.copy()
    want[guard:guard + numel] = fork_arena_numpy(s0[guard:guard + numel], d0[guard:guard + numel], lay[0], lay[1], lmax, n)
    kl = _lib.KvLayout(lay[0], lay[1], lmax, 128)
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.lcc_kv_copy_bf16(dbuf.data_ptr() + guard * 2, sbuf.data_ptr() + guard * 2, kl, n, st), "lcc_kv_copy_bf16")
    torch.cuda.synchronize(dev)
    got = dbuf.cpu().numpy().view(np.uint16)
    assert np.array_equal(sbuf.cpu().numpy().view(np.uint16), s0), "the source (or its neighbours) was written"
    assert np.array_equal(got[:guard], d0[:guard]) and np.array_equal(got[guard + numel:], d0[guard + numel:]), "a neighbouring arena was written"
    shape4 = (lay[0], 2, lay[1], lmax * 128)
    g4, s4, b4 = (x[guard:guard + numel].reshape(shape4) for x in (got, s0, d0))
    up = (n + 31) // 32 * 32
    for l, h in ((0, 0), (lay[0] - 1, lay[1] - 1)):      # readable messages on two planes, then everything at once
        for kv, nat in ((0, lambda x: x.reshape(lmax, 128)), (1, lambda x: v_natural(x.reshape(lmax // 32, 128, 32)))):
            a, s, b = nat(g4[l, kv, h]), nat(s4[l, kv, h]), nat(b4[l, kv, h])
            tag = f"layer {l} {'KV'[kv]} head {h}"
            assert np.array_equal(a[:n], s[:n]), f"{tag}: copied rows are not bit-identical"
            assert not a[n:up].any(), f"{tag}: rows [n, ceil32(n)) are not zero"
            assert np.array_equal(a[up:], b[up:]), f"{tag}: rows at or above ceil32(n) were written"
    assert np.array_equal(got, want)


def test_kv_copy_kernel_past_2_to_the_31_bytes(dev):
    """7B layout, lmax 65536: 3.76 GB per arena, so the last planes start past 2^31 BYTES and past 2^31 / 2 elements.  Compared on
    the device.  In both layouts the first 96 rows of a plane are its first 96 * 128 elements (K: 96 rows; V: 3 blocks of 128 x 32)."""
    from livecc_amd import _lib
    lib = _lib.load()
    L, H, lmax, n, rows = 28, 4, 65536, 70, 96
    planes, per_plane = L * 2 * H, lmax * 128
    assert planes * per_plane * 2 > 2 ** 31 + 2 ** 30
    SENT = 0x5A5A
    src = torch.zeros(planes * per_plane, dtype=torch.int16, device=dev)
    dst = torch.zeros(planes * per_plane, dtype=torch.int16, device=dev).fill_(SENT)
    g = torch.Generator(device=dev).manual_seed(7)
    head = torch.randint(-32768, 32768, (planes, rows * 128), dtype=torch.int32, device=dev, generator=g).to(torch.int16)
    s2, d2 = src.view(planes, per_plane), dst.view(planes, per_plane)
    s2[:, :rows * 128] = head
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.lcc_kv_copy_bf16(dst.data_ptr(), src.data_ptr(), _lib.KvLayout(L, H, lmax, 128), n, st), "lcc_kv_copy_bf16")
    torch.cuda.synchronize(dev)

    def natural(x, is_v):      # [planes', rows * 128] -> [planes', rows, 128]
        return x.view(-1, rows // 32, 128, 32).permute(0, 1, 3, 2).reshape(-1, rows, 128) if is_v else x.view(-1, rows, 128)
    is_v = ((torch.arange(planes, device=dev) // H) & 1).bool()
    for tag, sel in (("first plane (K)", [0]), ("last plane (V)", [planes - 1])):
        v = bool(is_v[sel[0]])
        a, s = natural(d2[sel, :rows * 128], v), natural(head[sel], v)
        assert torch.equal(a[:, :n], s[:, :n]), f"{tag}: copied rows differ"
        assert not bool(a[:, n:].any()), f"{tag}: rows 70-95 are not zero"
        assert bool((d2[sel, rows * 128:] == SENT).all()), f"{tag}: rows at or above 96 were written"
    for v in (False, True):
        a, s = natural(d2[:, :rows * 128][is_v == v], v), natural(head[is_v == v], v)
        assert torch.equal(a[:, :n], s[:, :n]) and not bool(a[:, n:].any())
    assert bool((d2[:, rows * 128:] == SENT).all()), "everything else in dst is still the sentinel"
    assert torch.equal(s2[:, :rows * 128], head) and not bool(s2[:, rows * 128:].any()), "src was written"


# ---- B. refusals write nothing ------------------------------------------------------------------------------------------------------
def test_kv_copy_refusals_write_nothing(dev):
    from livecc_amd import _lib
    lib = _lib.load()
    sbuf, numel = _arena((2, 1), 256, dev, seed=1, guard=0)
    dbuf, _ = _arena((2, 1), 256, dev, seed=2, guard=0)
    big, _ = _arena((2, 1), 256, dev, seed=3, guard=numel // 2)        # two arenas' worth: room for overlapping placements
    s0, d0, b0 = sbuf.clone(), dbuf.clone(), big.clone()
    st = torch.cuda.current_stream(dev).cuda_stream
    ok = _lib.KvLayout(2, 1, 256, 128)
    ARG, SHAPE, ALIGN, STATE = -1, -2, -3, -5
    S, D, B = sbuf.data_ptr(), dbuf.data_ptr(), big.data_ptr()
    for dst, src, kl, n, code in ((None, S, ok, 10, ARG), (D, None, ok, 10, ARG), (D + 2, S, ok, 10, ALIGN), (D, S + 8, ok, 10, ALIGN),
                                  (D, S, _lib.KvLayout(2, 1, 256, 64), 10, SHAPE), (D, S, _lib.KvLayout(2, 1, 250, 128), 10, SHAPE),
                                  (D, S, _lib.KvLayout(2, 1, 0, 128), 0, SHAPE), (D, S, _lib.KvLayout(0, 1, 256, 128), 10, SHAPE),
                                  (D, S, _lib.KvLayout(2, 0, 256, 128), 10, SHAPE), (D, S, ok, -1, STATE), (D, S, ok, 257, STATE),
                                  (D, D, ok, 10, ARG), (B + 16, B, ok, 10, ARG), (B, B + numel * 2 - 16, ok, 10, ARG),
                                  (B + numel, B, ok, 256, ARG)):
        assert lib.lcc_kv_copy_bf16(dst, src, kl, n, st) == code, (n, code)
        assert lib.lcc_last_error() != b""
    torch.cuda.synchronize(dev)
    assert torch.equal(sbuf, s0) and torch.equal(dbuf, d0) and torch.equal(big, b0)


# ---- C. engine ----------------------------------------------------------------------------------------------------------------------
def _build(cfg, dev, seed=0, init_scale=1.0):
    """tests/test_gpu_e2e.py::_build (the bf16 oracle's weights behind the native model; max_streams=4)."""
    from livecc_amd.modeling import LiveCCForConditionalGeneration
    from oracle import hf_oracle as O
    hf16 = O.build_hf_model(cfg, dtype=torch.bfloat16, seed=seed, init_scale=init_scale)
    native = LiveCCForConditionalGeneration.from_hf_model(hf16, cfg, dev, max_streams=4, max_kv_len=4096,
                                                          max_new_rows=2048, max_patches=8192, max_history=64)
    return hf16, native


@pytest.fixture(scope="module")
def tiny_native(dev):
    from livecc_amd.config import tiny
    return _build(tiny(), dev, seed=0, init_scale=2.0)[1]


def _replay(native, seed=11, n_turns=4):
    """A stream with every turn's prompt ids built up front (forks and controls then share them whatever the call order)."""
    from livecc_amd import protocol
    frames = torch.from_numpy(protocol.synth_frames(6 + 2 * (n_turns - 1), 56, 84, seed=seed, layout="TCHW"))
    rp = _Replay(native, native.cfg, frames, protocol.TurnBuilder(native.cfg, seed=seed))
    for ti in range(n_turns):              # one by one: `request` sizes the ids it builds by the grid of the turn it is asked for
        rp.request(ti)
    return rp


def _fork(rp):
    f = _Replay(rp.native, rp.cfg, rp.frames, rp.builder)
    f.turn_ids = rp.turn_ids
    f.state, f.past_ids, f.spans = rp.state.fork(), rp.past_ids.copy(), list(rp.spans)
    return f


def _same(ra, rb):
    return torch.equal(ra.sequences, rb.sequences) and torch.equal(ra.logits, rb.logits)


def _used_slot(native, seed, n_turns):
    """A LONGER stream with other content runs and is released: its slot is the next one handed out."""
    junk = _replay(native, seed=seed, n_turns=n_turns)
    for ti in range(n_turns):
        junk.turn(ti, repetition_penalty=1.3)
    slot, length = junk.state.slot, junk.state.get_seq_length()
    junk.state.release()
    return slot, length


def test_fork_continues_exactly_like_its_source_and_like_an_unforked_stream(tiny_native):
    eng = tiny_native.engine
    free0 = sorted(tiny_native._free_slots)
    src, ctl = _replay(tiny_native), _replay(tiny_native)
    for ti in range(2):
        assert _same(src.turn(ti), ctl.turn(ti))
    slot, junk_len = _used_slot(tiny_native, seed=57, n_turns=4)
    fk = _fork(src)
    assert fk.state.slot == slot and junk_len > src.state.get_seq_length(), "the destination held a longer, released stream"
    assert fk.state.get_seq_length() == src.state.get_seq_length() == len(src.past_ids)
    assert eng.slot_length(fk.state.slot) == eng.slot_length(src.state.slot) and fk.state.rope_delta == src.state.rope_delta
    r_src = src.turn(2)
    r_fk = fk.turn(2)                      # a separate call
    r_ctl = ctl.turn(2)
    assert _same(r_src, r_fk), "the fork's next turn differs from the source's"
    assert _same(r_src, r_ctl), "forking changed the source"
    assert bool(torch.isfinite(r_fk.logits.float()).all())
    assert eng.slot_length(fk.state.slot) == eng.slot_length(src.state.slot)
    # ... and one turn further, source and fork batched in ONE call
    (ia, ca), (ib, cb) = src.request(3), fk.request(3)
    outs = tiny_native.generate_batch([dict(input_ids=torch.from_numpy(ia), frames=ca, frames_layout="TCHW", state=src.state),
                                       dict(input_ids=torch.from_numpy(ib), frames=cb, frames_layout="TCHW", state=fk.state)],
                                      repetition_penalty=1.05, max_new_tokens=4, force_length=True, output_logits=True)
    assert _same(outs[0], outs[1]) and _same(outs[0], ctl.turn(3))
    for s in (src, ctl, fk):
        s.state.release()
    assert sorted(tiny_native._free_slots) == free0


def test_fork_copies_the_repetition_penalty_bitmap(tiny_native):
    PEN = 1.3
    src = _replay(tiny_native, seed=23)
    for ti in range(2):
        src.turn(ti, repetition_penalty=PEN)
    slot, _ = _used_slot(tiny_native, seed=58, n_turns=4)          # the destination's bitmap row holds another stream's ids
    fk = _fork(src)
    assert fk.state.slot == slot
    r_src = src.turn(2, max_new_tokens=1, repetition_penalty=PEN, output_scores=True)
    r_fk = fk.turn(2, max_new_tokens=1, repetition_penalty=PEN, output_scores=True)
    assert _same(r_src, r_fk) and torch.equal(r_src.scores, r_fk.scores), "the processed scores of the fork differ from the source's"
    assert not torch.equal(r_src.scores.float(), r_src.logits[0].float()), "the penalty is at work in this comparison"
    src.state.release(); fk.state.release()


def test_advancing_a_fork_leaves_the_source_alone(tiny_native):
    from livecc_amd import protocol
    src, ctl = _replay(tiny_native, seed=31), _replay(tiny_native, seed=31)
    for ti in range(2):
        assert _same(src.turn(ti), ctl.turn(ti))
    fk = src.state.fork()
    other = torch.from_numpy(protocol.synth_frames(2, 56, 84, seed=99, layout="TCHW"))
    tb = protocol.TurnBuilder(tiny_native.cfg, seed=99)
    tb.query_len = 9
    new = tb.turn_ids(2, protocol.num_video_tokens(protocol.grid_of(2, 56, 84, tiny_native.cfg), tiny_native.cfg), with_query=True)
    ids = np.concatenate([src.past_ids, new])
    r = tiny_native.generate(input_ids=torch.from_numpy(ids).view(1, -1), frames=other, frames_layout="TCHW", past_key_values=fk, do_sample=True,
                             seed=3, repetition_penalty=1.2, max_new_tokens=6, min_new_tokens=6)
    assert fk.get_seq_length() == len(ids) + 5 and src.state.get_seq_length() == len(src.past_ids)
    assert r.sequences.shape[1] == len(ids) + 6
    assert _same(src.turn(2), ctl.turn(2)), "the fork's turn reached the source's cache, bitmap, counters or positions"
    for s in (src.state, ctl.state, fk):
        s.release()


def test_fork_copies_the_rng_counter(tiny_native):
    """Draws are keyed by (seed, slot, counter): two forks of one state into the SAME slot, sampled with the same seed, draw the same
    tokens only if each fork starts from the source's counter and not from what the slot's last user left behind."""
    src = _replay(tiny_native, seed=41)
    for ti in range(2):
        src.turn(ti)
    ids, clip = src.request(2)

    def sample(st):
        r = tiny_native.generate(input_ids=torch.from_numpy(ids).view(1, -1), frames=clip, frames_layout="TCHW", past_key_values=st, do_sample=True,
                                 seed=5, temperature=1.5, top_k=0, repetition_penalty=1.05, max_new_tokens=8, min_new_tokens=8, output_logits=True)
        return r.sequences[0, len(ids):].tolist(), r.logits[0].clone()
    f1 = src.state.fork()
    slot = f1.slot
    t1, l1 = sample(f1)
    f1.release()
    f2 = src.state.fork()
    assert f2.slot == slot, "the second fork did not get the first fork's slot: the comparison below needs it"
    t2, l2 = sample(f2)
    f2.release()
    assert torch.equal(l1, l2) and t1 == t2
    assert len(set(t1)) > 1, "eight draws at temperature 1.5 from a flat tiny-model distribution"
    src.state.release()


def test_fork_refusals(tiny_native):
    from livecc_amd import _lib
    src = _replay(tiny_native, seed=43)
    src.turn(0)
    eng = tiny_native.engine
    for a, b in ((src.state.slot, src.state.slot), (-1, 0), (0, eng.max_slots), (eng.max_slots, 0)):
        with pytest.raises(_lib.LccError):
            eng.fork_slot(a, b)
    st = src.state
    st.release()
    with pytest.raises(ValueError):
        st.fork()


# ---- D. mcq_predict_many against the HF oracle ----------------------------------------------------------------------------------
def test_mcq_predict_many_matches_the_oracle_and_runs_the_tower_once(dev, tmp_path):
    """The setup and the bound of tests/test_gpu_e2e.py::test_mcq_prefill_only_scoring_matches_oracle, restated: per question one
    oracle forward on the full ids; |native - oracle| <= 6e-2 x the logit scale on the restricted logits, and the choice is the
    oracle's wherever its margin exceeds twice the error.  The vision tower runs once for the three questions."""
    import dataclasses
    from livecc_amd import ops, protocol
    from livecc_amd.config import tiny
    from livecc_amd.infer import LiveCCDemoInfer
    from livecc_amd.modeling import LiveCCForConditionalGeneration
    from livecc_amd.text import TextFrontEnd
    from oracle import hf_oracle as O
    from tests.test_text import make_tokenizer_dir
    fe0 = TextFrontEnd(make_tokenizer_dir(tmp_path))
    tk = fe0.tokenizer
    cfg = dataclasses.replace(tiny(), video_token_id=fe0.video_token_id, eos_token_id=fe0.eos_token_id,
                              image_token_id=tk.convert_tokens_to_ids("<|image_pad|>"),
                              vision_start_token_id=tk.convert_tokens_to_ids("<|vision_start|>"),
                              vision_end_token_id=tk.convert_tokens_to_ids("<|vision_end|>"),
                              bos_token_id=tk.convert_tokens_to_ids("<|endoftext|>"))
    hf16 = O.build_hf_model(cfg, dtype=torch.bfloat16, seed=8, init_scale=2.0)
    native = LiveCCForConditionalGeneration.from_hf_model(hf16, cfg, dev, max_streams=4, max_kv_len=2048, max_new_rows=1024,
                                                          max_patches=4096, max_history=8)
    infer = LiveCCDemoInfer(model=native, text=TextFrontEnd(tk, cfg))
    frames = torch.from_numpy(protocol.synth_frames(4, 56, 84, seed=4, layout="TCHW"))
    VIT = ("attn_vit32", "gemm_vit_qkv")
    tower_calls, orig_vit = [], native._vit_encode

    def spy(clips, stream=None):
        tower_calls.append(len(clips))
        return orig_vit(clips, stream=stream)
    native._vit_encode = spy
    try:
        c0 = ops.launch_counts()
        one = infer.mcq_predict(frames, ITEMS[0][0], ITEMS[0][1])
        c1, n_one = ops.launch_counts(), len(tower_calls)
        res = infer.mcq_predict_many(frames, ITEMS)
        c2, n_many = ops.launch_counts(), len(tower_calls) - n_one
    finally:
        native._vit_encode = orig_vit
    assert len(res) == 3 and one[1].shape == (4,) and sorted(native._free_slots) == [0, 1, 2, 3]
    assert n_one == 1 and n_many == 1, f"the vision tower ran {n_many} times for three questions ({n_one} for one)"
    # the vision-tower launch counters that move for the single call move by the same amount for the three questions (at this tiny
    # clip the tower may be served by kernels without a counter: then the call count above is the whole statement)
    d_one, d_many = {k: c1[k] - c0[k] for k in VIT}, {k: c2[k] - c1[k] for k in VIT}
    print("vision-tower launch counters of one mcq_predict:", d_one, " of mcq_predict_many:", d_many)
    for k in VIT:                          # every tower counter, moved or not: a tower that ran per question would move it three times as far
        assert d_many[k] == d_one[k], f"{k}: the tower ran {d_many[k]} launches for three questions, {d_one[k]} for one"
    fe = infer.text
    letter_ids = [tk(f": {x}").input_ids[-1] for x in "ABCD"]
    grid = protocol.grid_of(4, 56, 84, cfg)
    pv, g = O.patchify_normalize_ref(frames, cfg)
    lens = set()
    for qi, (item, (choice, lg)) in enumerate(zip(ITEMS, res)):
        query = item[0] + "\n" + "\n".join(item[1]) + "\nPlease select the correct answer."
        if len(item) == 3:
            query = f"This video's subtitles are listed below:\n{item[2]}\nAccording to the video and subtitles, " + query
        ids = fe.encode(fe.qa_text(query, continuing=False, with_video=True) + "Answer:", [grid])
        assert fe.decode(ids, skip_special_tokens=False).endswith("<|im_start|>assistant\nAnswer:")
        lens.add(len(ids))
        ro = O.OracleStream(hf16, cfg).turn(ids, pv, g, max_new_tokens=1, repetition_penalty=1.0)
        ref = ro["logits"][0][letter_ids]
        err, scale = (lg - ref).abs().max().item(), ro["logits"][0].abs().max().item()
        print(f"question {qi}: {len(ids)} ids, |native - oracle| = {err:.4g}, logit scale {scale:.4g}, choice {choice}")
        assert lg.shape == (4,) and 0 <= choice < 4
        assert err <= 6e-2 * scale, f"question {qi}"
        margin = torch.topk(ref, 2).values
        if (margin[0] - margin[1]).item() > 2 * err:
            assert choice == int(torch.argmax(ref)), f"question {qi}"
    assert len(lens) == 3, "three questions of different lengths"


# ---- E. ask -------------------------------------------------------------------------------------------------------------------------
def test_ask_on_the_side_leaves_the_commentary_stream_bit_identical(tiny_native):
    from livecc_amd import protocol
    from livecc_amd.infer import LiveCCDemoInfer

    class FixedIds(protocol.TurnBuilder):          # per-turn ids independent of call order and of the builder's history
        def turn_ids(self, turn_index, n_video_tokens, with_query=None):
            self._rng = np.random.RandomState(1000 + turn_index)
            return super().turn_ids(turn_index, n_video_tokens, with_query)
    frames = torch.from_numpy(protocol.synth_frames(10, 56, 84, seed=61, layout="TCHW"))
    kw = dict(max_new_tokens=4, force_length=True, output_logits=True)

    class Stream:
        def __init__(self):
            self.infer = LiveCCDemoInfer(model=tiny_native, turn_builder=FixedIds(tiny_native.cfg))
            self.state, self.outs = {}, []

        def chunks(self, clip):
            orig = tiny_native.generate

            def spy(*a, **k):
                r = orig(*a, **k)
                self.outs.append(r)
                return r
            tiny_native.generate = spy
            try:
                for _ in self.infer.live_cc_clip(clip, self.state, **kw):
                    pass
            finally:
                tiny_native.generate = orig
    A, B, C = Stream(), Stream(), Stream()
    for s in (A, B, C):
        s.chunks(frames[:8])                                   # two chunks: 6 + 2 frames
        assert s.state["turn_index"] == 2
    before = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in A.state.items()}
    len_before = tiny_native.engine.slot_length(A.state["past_key_values"].slot)
    free_before = len(tiny_native._free_slots)
    resp = A.infer.ask(16, A.state, max_new_tokens=4, force_length=True)
    assert isinstance(resp, str) and len(tiny_native._free_slots) == free_before
    assert A.state.keys() == before.keys() and all(
        np.array_equal(A.state[k], before[k]) if isinstance(before[k], np.ndarray) else A.state[k] is before[k] or A.state[k] == before[k]
        for k in before)
    assert tiny_native.engine.slot_length(A.state["past_key_values"].slot) == len_before and len_before[0] == len(A.state["past_ids"])
    A.chunks(frames[8:])
    B.chunks(frames[8:])
    assert len(A.outs) == len(B.outs) == 3
    assert _same(A.outs[2], B.outs[2]), "the question reached the commentary stream"
    assert np.array_equal(A.state["past_ids"], B.state["past_ids"])
    # the answer is the one a destructive video_qa turn gives on an identically built stream
    C.infer.video_qa(16, [], C.state, max_new_tokens=4, force_length=True)
    asked, destructive = A.infer.last_generated[-2], C.infer.last_generated[-1]
    assert asked["span"] is None and np.array_equal(asked["prompt_ids"], destructive["prompt_ids"])
    assert asked["tokens"] == destructive["tokens"] and len(asked["tokens"]) == 4
    for s in (A, B, C):
        s.state["past_key_values"].release()

"""-m gpu: the sliding KV window -- the in-place compaction kernel (csrc/kv_evict.hip) bit for bit against the numpy statement of the
arena layout (tests/test_kv_window.py), `StreamState.evict` against HF with the same rows cut out of its DynamicCache, against the
engine itself, its repetition-penalty bitmap, batch invariance, and `StreamServer(window_policy="slide")` end to end."""
import numpy as np
import pytest
import torch

from tests.test_kv_window import evict_arena_numpy, hf_cut, v_natural

pytestmark = pytest.mark.gpu

# bounds of tests/test_gpu_e2e.py::_compare_stream (the multi-turn stream bound at the tiny / small configs), restated
GROSS_REL = 6e-2                 # |native - bf16 oracle| <= 6e-2 x logit scale per step
ERR_RATIO, ERR_ABS_REL = 1.5, 1e-3 + 2.0 ** -7      # |native - fp32| <= 1.5 x |bf16 oracle - fp32| + (1e-3 + one bf16 ulp) x scale


# ---- 5. kernel, bit-exact -------------------------------------------------------------------------------------------------------
LAYOUTS = {"tiny": (2, 1), "small": (4, 1), "gqa2": (3, 2), "7b": (28, 4)}      # (n_layers, n_kv_heads) of the arena
KERNEL_CASES = [
    # layout, lmax, kv_len, first, n                      n%32  first%32  tail vs n              launch shape
    ("tiny", 1024, 1000, 64, 64),          #               0     0         much longer            one workgroup per plane
    ("tiny", 1024, 1000, 60, 62),          #               30    28        much longer            one workgroup per plane
    ("tiny", 1024, 900, 450, 225),         #               1     2         equal                  windows
    ("tiny", 1024, 901, 450, 300),         #               12    2         shorter                windows
    ("tiny", 1024, 1024, 33, 95),          #               31    1         longer, kv_len == lmax  one workgroup per plane (15 windows > 8)
    ("tiny", 1024, 700, 600, 100),         #               4     24        none: truncate + zero
    ("tiny", 1024, 1024, 3, 31),           #               31    3         n below one block
    ("tiny", 1024, 777, 0, 1),             #               1     0         first == 0, one row
    ("gqa2", 256, 250, 40, 96),            #               0     8         longer, two KV heads   windows
    ("gqa2", 256, 256, 17, 239),           #               15    17        none, kv_len == lmax
    ("small", 2048, 2048, 450, 799),       #               31    2         equal, kv_len == lmax  windows
    ("small", 2048, 2000, 130, 400),       #               16    2         much longer (overlap)  windows (5 launches)
    ("small", 2048, 2000, 130, 160),       #               0     2         much longer            one workgroup per plane
    ("7b", 32768, 32700, 450, 16125),      #               29    2         equal, near 32k        windows (the planner's case)
]


def _arena(lay, lmax, dev, seed, guard):
    """[guard | arena | guard] of random bf16 bit patterns (NaN / inf / denormal patterns included: the op is a copy)."""
    n = lay[0] * 2 * lay[1] * lmax * 128
    g = torch.Generator(device=dev).manual_seed(seed)
    buf = torch.randint(-32768, 32768, (guard + n + guard,), dtype=torch.int32, device=dev, generator=g).to(torch.int16)
    return buf, n


@pytest.mark.parametrize("name,lmax,L,first,n", KERNEL_CASES)
def test_kv_evict_kernel_is_a_bit_exact_compaction(dev, name, lmax, L, first, n):
    from livecc_amd import _lib
    lib = _lib.load()
    lay = LAYOUTS[name]
    # the neighbours stand for the other slots' arenas: whole arenas at the small layouts, 8-MB bands next to the 1.9-GB 7B arena
    guard = lay[0] * 2 * lay[1] * lmax * 128 if name != "7b" else 4 << 20
    buf, numel = _arena(lay, lmax, dev, seed=first * 131 + n, guard=guard)
    assert buf.data_ptr() % 256 == 0 and (guard * 2) % 256 == 0
    before = buf.cpu().numpy().view(np.uint16)
    assert np.isnan(torch.from_numpy(before[guard:guard + 4096].view(np.int16).copy()).view(torch.bfloat16).float().numpy()).any()
    want = before.copy()
    want[guard:guard + numel] = evict_arena_numpy(before[guard:guard + numel], lay[0], lay[1], lmax, L, first, n)
    kl = _lib.KvLayout(lay[0], lay[1], lmax, 128)
    assert lib.lcc_kv_evict_scratch_bytes(kl, L, first, n) == 0
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.lcc_kv_evict_bf16(buf.data_ptr() + guard * 2, kl, L, first, n, None, 0, st), "lcc_kv_evict_bf16")
    torch.cuda.synchronize(dev)
    got = buf.cpu().numpy().view(np.uint16)
    assert np.array_equal(got[:guard], before[:guard]) and np.array_equal(got[guard + numel:], before[guard + numel:]), "a neighbouring arena was written"
    g4, b4 = got[guard:guard + numel].reshape(lay[0], 2, lay[1], lmax * 128), before[guard:guard + numel].reshape(lay[0], 2, lay[1], lmax * 128)
    for l, h in ((0, 0), (lay[0] - 1, lay[1] - 1)):      # readable messages on two planes, then everything at once
        for kv, nat in ((0, lambda x: x.reshape(lmax, 128)), (1, lambda x: v_natural(x.reshape(lmax // 32, 128, 32)))):
            a, b = nat(g4[l, kv, h]), nat(b4[l, kv, h])
            tag = f"layer {l} {'KV'[kv]} head {h}"
            assert np.array_equal(a[:first], b[:first]), f"{tag}: rows below first changed"
            assert np.array_equal(a[first:L - n], b[first + n:L]), f"{tag}: kept rows are not bit-identical"
            assert not a[L - n:L].any(), f"{tag}: vacated rows are not zero"
            assert np.array_equal(a[L:], b[L:]), f"{tag}: rows at or above kv_len were written"
    assert np.array_equal(got, want)


def test_kv_evict_refuses_bad_ranges_and_writes_nothing(dev):
    from livecc_amd import _lib
    lib = _lib.load()
    buf, numel = _arena((2, 1), 256, dev, seed=1, guard=0)
    before = buf.clone()
    st = torch.cuda.current_stream(dev).cuda_stream
    ok = _lib.KvLayout(2, 1, 256, 128)
    STATE, ARG, SHAPE, ALIGN = -5, -1, -2, -3
    for kl, L, first, n, code in ((ok, 200, -1, 10, STATE), (ok, 200, 10, 0, STATE), (ok, 200, 150, 51, STATE), (ok, 200, 201, 1, STATE),
                                  (ok, 257, 0, 10, STATE), (ok, -1, 0, 1, STATE), (ok, 200, 10, -5, STATE),
                                  (_lib.KvLayout(2, 1, 256, 64), 200, 10, 10, SHAPE), (_lib.KvLayout(2, 1, 250, 128), 200, 10, 10, SHAPE),
                                  (_lib.KvLayout(0, 1, 256, 128), 200, 10, 10, SHAPE)):
        assert lib.lcc_kv_evict_bf16(buf.data_ptr(), kl, L, first, n, None, 0, st) == code, (L, first, n)
        assert lib.lcc_last_error() != b""
    assert lib.lcc_kv_evict_bf16(None, ok, 200, 10, 10, None, 0, st) == ARG
    assert lib.lcc_kv_evict_bf16(buf.data_ptr() + 2, ok, 200, 10, 10, None, 0, st) == ALIGN
    torch.cuda.synchronize(dev)
    assert torch.equal(buf, before)


# ---- shared: a stream replayed turn by turn ---------------------------------------------------------------------------------------
class _Replay:
    """One native stream driven like the reference does (cat(past_ids, new_ids), KV carry), with the turn table an evicting caller keeps."""

    def __init__(self, native, cfg, frames, builder):
        from livecc_amd import protocol
        self.native, self.cfg, self.frames, self.builder = native, cfg, frames, builder
        self.chunks = protocol.split_clip(frames.shape[0])
        self.state, self.past_ids, self.spans, self.turn_ids = None, None, [], []

    def request(self, ti):
        from livecc_amd import protocol
        a, b = self.chunks[ti]
        clip = self.frames[a:b]
        grid = protocol.grid_of(clip.shape[0], clip.shape[2], clip.shape[3], self.cfg)
        while len(self.turn_ids) <= ti:
            self.turn_ids.append(self.builder.turn_ids(len(self.turn_ids), protocol.num_video_tokens(grid, self.cfg)))
        new = self.turn_ids[ti]
        ids = new if self.past_ids is None else np.concatenate([self.past_ids, new])
        return ids, clip

    def turn(self, ti, teacher=None, max_new_tokens=4, repetition_penalty=1.05, **kw):
        ids, clip = self.request(ti)
        r = self.native.generate(input_ids=torch.from_numpy(ids).view(1, -1), frames=clip, frames_layout="TCHW", past_key_values=self.state,
                                 do_sample=False, repetition_penalty=repetition_penalty, max_new_tokens=max_new_tokens,
                                 min_new_tokens=max_new_tokens, output_logits=True, teacher_tokens=teacher, **kw)
        self.absorb(r, len(ids))
        return r

    def absorb(self, r, n_in):
        self.state = r.past_key_values
        seq = r.sequences[0].cpu().numpy()
        self.spans.append((0 if self.past_ids is None else len(self.past_ids), len(seq) - 1))
        self.past_ids = seq[:-1]
        return seq[n_in:].tolist()

    def evict_turns(self, t0, t1):
        first, n = self.spans[t0][0], self.spans[t1][1] - self.spans[t0][0]
        kept = np.concatenate([self.past_ids[:first], self.past_ids[first + n:]])
        self.state.evict(first, n, kept)
        self.past_ids = kept
        self.spans = self.spans[:t0] + [(b - n, e - n) for b, e in self.spans[t1 + 1:]]
        return first, n


@pytest.fixture(scope="module")
def tiny_native(dev):
    from livecc_amd.config import tiny
    from livecc_amd.modeling import LiveCCForConditionalGeneration
    return LiveCCForConditionalGeneration.from_config(tiny(), dev, seed=0, max_streams=4, max_kv_len=2048, max_new_rows=1024,
                                                      max_patches=4096, max_history=16)


def _tiny_replay(native, seed=11, n_turns=5):
    from livecc_amd import protocol
    frames = torch.from_numpy(protocol.synth_frames(6 + 2 * (n_turns - 1), 56, 84, seed=seed, layout="TCHW"))
    return _Replay(native, native.cfg, frames, protocol.TurnBuilder(native.cfg, seed=seed))


# ---- 6. engine against HF -------------------------------------------------------------------------------------------------------
def test_evicted_stream_matches_hf_with_the_same_rows_cut_out_of_its_cache(dev):
    """small() config (GQA group 7), HF live on the host: 4 turns, turns 1-2 evicted on both sides (native: StreamState.evict, HF:
    tests/test_kv_window.py::hf_cut), 2 more turns, every native step teacher-forced on the bf16 oracle's tokens.  Bound: the one
    tests/test_gpu_e2e.py::_compare_stream enforces for a multi-turn stream at this config -- |native - bf16 oracle| <= 6e-2 x logit
    scale, and |native - fp32 oracle| <= 1.5 x |bf16 oracle - fp32 oracle| + (1e-3 + 2^-7) x scale -- the SAME for the turns after the
    eviction as for the turns before it."""
    from livecc_amd import protocol
    from livecc_amd.config import small
    from livecc_amd.modeling import LiveCCForConditionalGeneration
    from oracle import hf_oracle as O
    from tests.util import record
    cfg = small()
    hf16 = O.build_hf_model(cfg, dtype=torch.bfloat16, seed=1, init_scale=1.5)
    hf32 = O.build_hf_model(cfg, dtype=torch.float32, seed=1, init_scale=1.5)
    native = LiveCCForConditionalGeneration.from_hf_model(hf16, cfg, dev, max_streams=1, max_kv_len=2048, max_new_rows=1024, max_patches=4096,
                                                          max_history=16)
    frames = torch.from_numpy(protocol.synth_frames(6 + 2 * 5, 112, 140, seed=77, layout="TCHW"))
    rp = _Replay(native, cfg, frames, protocol.TurnBuilder(cfg, seed=77))
    s16, s32 = O.OracleStream(hf16, cfg), O.OracleStream(hf32, cfg)
    PEN, NEW = 1.15, 4
    worst = {"before": [0.0, 0.0], "after": [0.0, 0.0]}
    for ti in range(6):
        if ti == 4:
            L, pos = native.engine.slot_length(rp.state.slot)
            delta = rp.state.rope_delta
            first, n = rp.evict_turns(1, 2)
            assert native.engine.slot_length(rp.state.slot) == (L - n, pos) and rp.state.rope_delta == delta + n
            assert first == rp.spans[0][1] and n > 64 and n % 32 != 0
            for s in (s16, s32):
                hf_cut(s, first, n)
            assert np.array_equal(s16.past_ids[0].numpy(), rp.past_ids)
        ids, clip = rp.request(ti)
        pv, grid = O.patchify_normalize_ref(clip, cfg)
        r16 = s16.turn(rp.turn_ids[ti], pv, grid, max_new_tokens=NEW, repetition_penalty=PEN)
        toks = r16["new_tokens"]
        r32 = s32.turn(rp.turn_ids[ti], pv, grid, max_new_tokens=NEW, repetition_penalty=PEN, teacher_tokens=toks)
        rn = rp.turn(ti, teacher=toks, max_new_tokens=NEW, repetition_penalty=PEN)
        assert rn.sequences[0, -NEW:].tolist() == toks == r32["new_tokens"]
        w = worst["after" if ti >= 4 else "before"]
        for k in range(NEW):
            ln, l16, l32 = rn.logits[k].float().cpu(), r16["logits"][k], r32["logits"][k]
            scale = l32.abs().max().item()
            d16, en, eo = (ln - l16).abs().max().item(), (ln - l32).abs().max().item(), (l16 - l32).abs().max().item()
            w[0], w[1] = max(w[0], d16 / scale), max(w[1], en / (eo + 1e-3 * scale))
            print(f"turn {ti} step {k}: |native-bf16|/scale {d16 / scale:.4f}  native err {en:.4g}  bf16-oracle err {eo:.4g}  scale {scale:.3g}")
            assert d16 <= GROSS_REL * scale, f"turn {ti} step {k}: |native - bf16 oracle| = {d16:.4g} (scale {scale:.3g})"
            assert en <= ERR_RATIO * eo + ERR_ABS_REL * scale, f"turn {ti} step {k}: native error vs fp32 {en:.4g} > 1.5 x bf16-oracle error {eo:.4g}"
    record("kv_window_small_vs_hf", dict(worst_rel_dlogit_before=worst["before"][0], worst_err_ratio_before=worst["before"][1],
                                         worst_rel_dlogit_after=worst["after"][0], worst_err_ratio_after=worst["after"][1]))
    rp.state.release()


# ---- 7. engine against itself ---------------------------------------------------------------------------------------------------
def test_evicting_the_last_turn_equals_truncation(tiny_native):
    """Rows of the LAST cached turn evicted (first + n == kv_len) == `set_slot_length(first, next_pos)`: the next turn's raw logits are
    bit-identical between the two routes (teacher-forced, so the seen-id bitmap, which only the truncation route leaves stale, plays
    no part).  The kernel has no separate n % 32 == 0 path (the rotation by 0 columns runs the same code), so there is no second
    route to compare arena bytes with; its two launch shapes are both checked against numpy above."""
    a, b = _tiny_replay(tiny_native), _tiny_replay(tiny_native)
    for ti in range(3):
        ra, rb = a.turn(ti), b.turn(ti)
        assert torch.equal(ra.sequences, rb.sequences) and torch.equal(ra.logits, rb.logits)
    eng = tiny_native.engine
    (L, pos), first = eng.slot_length(a.state.slot), a.spans[2][0]
    n = L - first
    a.evict_turns(2, 2)
    eng.set_slot_length(b.state.slot, first, pos)
    b.state.rope_delta += n
    b.past_ids, b.spans = b.past_ids[:first], b.spans[:2]
    assert eng.slot_length(a.state.slot) == eng.slot_length(b.state.slot) == (first, pos) and np.array_equal(a.past_ids, b.past_ids)
    forced = [5, 6, 7, 8]
    ra, rb = a.turn(3, teacher=forced), b.turn(3, teacher=forced)
    assert torch.equal(ra.logits, rb.logits) and bool(torch.isfinite(ra.logits.float()).all())
    ra, rb = a.turn(4, repetition_penalty=1.0), b.turn(4, repetition_penalty=1.0)
    assert torch.equal(ra.logits, rb.logits) and torch.equal(ra.sequences, rb.sequences)
    a.state.release(); b.state.release()


def test_stream_state_evict_refuses_bad_calls(tiny_native):
    a = _tiny_replay(tiny_native)
    a.turn(0); a.turn(1)
    L, pos = tiny_native.engine.slot_length(a.state.slot)
    with pytest.raises(ValueError):
        a.state.evict(0, L, [])                               # nothing kept
    with pytest.raises(ValueError):
        a.state.evict(10, L, a.past_ids[:10])                 # outside the cached length
    with pytest.raises(ValueError):
        a.state.evict(10, 0, a.past_ids)
    with pytest.raises(ValueError):
        a.state.evict(10, 5, a.past_ids)                      # kept ids do not match the rows that remain
    assert tiny_native.engine.slot_length(a.state.slot) == (L, pos)
    st = a.state
    st.release()
    with pytest.raises(ValueError):
        st.evict(10, 5, np.concatenate([a.past_ids[:10], a.past_ids[15:]]))


# ---- 8. repetition penalty ------------------------------------------------------------------------------------------------------
def test_repetition_penalty_forgets_evicted_ids_only(tiny_native):
    """X occurs only in the evicted turn, Y also in a kept one: after the eviction X's processed score is its raw logit again while Y
    stays penalised (HF's processor sees input_ids = kept ids + new ids); without the eviction both are penalised."""
    PEN = 1.3
    runs = {}
    for evict in (True, False):
        rp = _tiny_replay(tiny_native, seed=23)
        for ti in range(4):
            rp.request(ti)                                   # builds every turn's prompt ids up front
        used = set(np.concatenate(rp.turn_ids[:4]).tolist())
        free = [t for t in range(100, 400) if t not in used]
        X, Y = free[0], free[1]
        forced = [free[10:14], [X, Y, free[14], free[15]], [Y, free[16], free[17], free[18]]]
        for ti in range(3):
            rp.turn(ti, teacher=forced[ti], repetition_penalty=PEN)
        if evict:
            rp.evict_turns(1, 1)
            assert X not in rp.past_ids and Y in rp.past_ids
        r = rp.turn(3, max_new_tokens=1, repetition_penalty=PEN, output_scores=True)
        runs[evict] = (r.logits[0].float().cpu(), r.scores.float().cpu(), X, Y)
        rp.state.release()

    def penalised(l):
        return l / PEN if l > 0 else l * PEN
    for evict, (lg, sc, X, Y) in runs.items():
        assert lg[X] != 0 and lg[Y] != 0
        assert sc[Y].item() == pytest.approx(penalised(lg[Y].item()), rel=1e-5) and sc[Y] != lg[Y]
        if evict:
            assert sc[X].item() == lg[X].item(), "an id that only occurred in the evicted turn is still penalised"
        else:
            assert sc[X].item() == pytest.approx(penalised(lg[X].item()), rel=1e-5) and sc[X] != lg[X]


# ---- 9. batch invariance ----------------------------------------------------------------------------------------------------------
def test_a_stream_batched_with_a_freshly_slid_stream_equals_itself_alone(tiny_native):
    a, b, alone = _tiny_replay(tiny_native, seed=31), _tiny_replay(tiny_native, seed=32), _tiny_replay(tiny_native, seed=32)
    for ti in range(3):
        a.turn(ti)
    for ti in range(2):
        b.turn(ti); alone.turn(ti)
    a.evict_turns(1, 1)
    (ia, ca), (ib, cb) = a.request(3), b.request(2)
    kw = dict(repetition_penalty=1.05, max_new_tokens=4, force_length=True, output_logits=True)
    outs = tiny_native.generate_batch([dict(input_ids=torch.from_numpy(ia), frames=ca, frames_layout="TCHW", state=a.state),
                                       dict(input_ids=torch.from_numpy(ib), frames=cb, frames_layout="TCHW", state=b.state)], **kw)
    solo = tiny_native.generate_batch([dict(input_ids=torch.from_numpy(ib), frames=cb, frames_layout="TCHW", state=alone.state)], **kw)[0]
    assert torch.equal(outs[1].sequences, solo.sequences) and torch.equal(outs[1].logits, solo.logits)
    assert bool(torch.isfinite(outs[0].logits.float()).all())
    # ... and the slid stream itself is served the same in the batch as alone
    a2 = _tiny_replay(tiny_native, seed=31)
    for ti in range(3):
        a2.turn(ti)
    a2.evict_turns(1, 1)
    ra2 = a2.turn(3)
    assert torch.equal(outs[0].sequences, ra2.sequences) and torch.equal(outs[0].logits, ra2.logits)
    for s in (a, b, alone, a2):
        s.state.release()


# ---- 10. server end to end ---------------------------------------------------------------------------------------------------------
def test_slide_server_streams_three_windows_without_end(dev):
    """small() model, a 256-row KV slot, a 40-s clip (more than 3 x the window in rows): no window_full, no error, >= 2 evictions, and
    a short neighbour stream yields exactly the tokens it yields alone.  KV bound: the engine's own rule is `cached + new rows +
    max_history <= max_kv_len` BEFORE generation, so every call's prompt is <= max_kv_len - max_history rows and the up to
    max_new_tokens - 1 rows that generation appends stay inside the max_history headroom (<= max_kv_len)."""
    from livecc_amd import protocol
    from livecc_amd.config import small
    from livecc_amd.infer import LiveCCDemoInfer
    from livecc_amd.modeling import LiveCCForConditionalGeneration
    from livecc_amd.server import StreamServer
    MAXKV, HIST, NEW = 256, 8, 4
    native = LiveCCForConditionalGeneration.from_config(small(), dev, seed=3, max_streams=2, max_kv_len=MAXKV, max_new_rows=512,
                                                        max_patches=2048, max_history=HIST)

    class FixedIds(protocol.TurnBuilder):          # per-turn ids independent of call order (the streams share one builder)
        def turn_ids(self, turn_index, n_video_tokens, with_query=None):
            self._rng = np.random.RandomState(1000 + turn_index)
            return super().turn_ids(turn_index, n_video_tokens, with_query)

    def video(seed, n_frames):
        g = torch.Generator().manual_seed(seed)
        return torch.randint(0, 256, (n_frames, 60, 90, 3), dtype=torch.uint8, generator=g).to(dev), np.arange(n_frames) / 30.0

    def serve(vids):
        srv = StreamServer(LiveCCDemoInfer(model=native, turn_builder=FixedIds(native.cfg)), max_new_tokens=NEW, force_length=True,
                           window_policy="slide")
        for sid, v in vids.items():
            srv.add_stream(sid, *v, t_start=0.0, max_pixels=4 * 28 * 28)
        prompts, orig = [], native.generate_batch

        def spy(reqs, **kw):
            prompts.extend(int(r["input_ids"].numel()) for r in reqs)
            return orig(reqs, **kw)
        native.generate_batch = spy
        lengths = []
        try:
            out = srv.run(realtime=False, on_result=lambda sid, span, text, st: lengths.append(
                (sid, len(st["past_ids"]), native.engine.slot_length(st["past_key_values"].slot)[0]) if st.get("past_key_values") else None))
        finally:
            native.generate_batch = orig
        for sid in list(vids):
            srv.remove_stream(sid)
        return out, prompts, lengths
    long_v, short_v = video(1, 1200), video(2, 150)
    out, prompts, lengths = serve({"long": long_v, "short": short_v})
    by = {}
    for sid, span, text, st in out:
        by.setdefault(sid, []).append((span, text, st))
    assert not any(st.get("window_full") or "error" in st or st.get("restarted") for _, _, st in by["long"] + by["short"])
    assert by["long"][-1][0][1] >= 39.0 and len(by["long"]) == 38
    slid = [st for _, _, st in by["long"] if st.get("slid")]
    assert len(slid) >= 2 and [st["evictions"] for st in slid] == list(range(1, len(slid) + 1)) and all(st["evicted_turns"] >= 1 for st in slid)
    assert not any(st.get("slid") for _, _, st in by["short"])
    assert max(prompts) <= MAXKV - HIST, "a call's cached + new rows respect the engine's rule"
    assert all(x is not None and x[1] == x[2] <= MAXKV - HIST + NEW - 1 for x in lengths), "past_ids and the device KV length agree and stay inside the slot"
    # the scenario: every turn appends >= 24 prompt rows, so the long stream went through more than 3 windows of rows
    assert 24 * len(by["long"]) > 3 * MAXKV
    solo, _, _ = serve({"short": short_v})
    assert [(s, t) for s, t, _ in by["short"]] == [(span, text) for _, span, text, _ in solo] and len(solo) == 3
    assert all(t != "" for _, t, _ in by["short"] + by["long"])


# ---- live_cc(kv_window="slide"): the single-stream generator --------------------------------------------------------------------------
def test_live_cc_slides_where_the_reference_behaviour_runs_out_of_cache(dev):
    from livecc_amd import _lib
    from livecc_amd.config import tiny
    from livecc_amd.infer import LiveCCDemoInfer
    from livecc_amd.modeling import LiveCCForConditionalGeneration
    from livecc_amd.video import DecodedVideo
    native = LiveCCForConditionalGeneration.from_config(tiny(), dev, seed=0, max_streams=1, max_kv_len=256, max_new_rows=512, max_patches=2048,
                                                        max_history=8)
    g = torch.Generator().manual_seed(5)
    frames, pts = torch.randint(0, 256, (600, 60, 90, 3), dtype=torch.uint8, generator=g).to(dev), np.arange(600) / 30.0     # 20 s

    def play(kv_window):
        infer = LiveCCDemoInfer(model=native)
        state, spans = {"video_path": DecodedVideo(frames, pts, 30.0)}, []
        try:
            for wall in np.arange(0.0, 21.0, 0.5):
                state["video_timestamp"] = float(wall)
                for span, text, state in infer.live_cc(None, state, max_pixels=4 * 28 * 28, max_new_tokens=4, force_length=True, do_sample=False,
                                                      kv_window=kv_window):
                    spans.append(span)
                    assert len(state["past_ids"]) == native.engine.slot_length(state["past_key_values"].slot)[0] <= 256
        finally:
            if state.get("past_key_values") is not None:
                state["past_key_values"].release()
        return spans, state
    spans, state = play("slide")
    assert spans[0] == (0.0, 3.0) and spans[-1][1] >= 19.5 and state.get("evictions", 0) >= 2
    assert state["turn_spans"][0][0] == 0 and state["turn_spans"][-1][1] == len(state["past_ids"])
    with pytest.raises(_lib.LccError):
        play(None)                                   # today's behaviour: the engine refuses the prefill that does not fit
    with pytest.raises(ValueError):
        next(LiveCCDemoInfer(model=native).live_cc(None, {"video_path": DecodedVideo(frames, pts, 30.0)}, kv_window="ring"))

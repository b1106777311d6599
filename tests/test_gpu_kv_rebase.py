"""-m gpu: the sliding KV window with positions inside the cache ("rebase") -- the re-rotating form of the compaction kernel
(csrc/kv_evict.hip, REBASE) against the numpy statement of tests/test_kv_rebase.py, `StreamState.evict(rebase=True)` against HF with
the same rows cut and the same keys rotated in its DynamicCache, against the engine itself, batch invariance, fork, and
`StreamServer(window_policy="slide_rebase")` / `live_cc(kv_window="slide_rebase")` end to end."""
import numpy as np
import pytest
import torch

from tests.test_kv_rebase import bf16_to_f64, hf_cut_rebase, rebase_arena_numpy, rot_table, rotate_rows_f64

pytestmark = pytest.mark.gpu

# bounds of tests/test_gpu_kv_window.py (those of tests/test_gpu_e2e.py::_compare_stream), restated
GROSS_REL = 6e-2                 # |native - bf16 oracle| <= 6e-2 x logit scale per step
ERR_RATIO, ERR_ABS_REL = 1.5, 1e-3 + 2.0 ** -7      # |native - fp32| <= 1.5 x |bf16 oracle - fp32| + (1e-3 + one bf16 ulp) x scale
STATE, ARG, SHAPE, ALIGN = -5, -1, -2, -3


# ---- 4. kernel against the oracle -------------------------------------------------------------------------------------------------
LAYOUTS = {"tiny": (2, 1), "small": (4, 1), "gqa2": (3, 2), "7b_planes": (28, 4)}      # (n_layers, n_kv_heads) of the arena
KERNEL_CASES = [
    # layout, lmax, kv_len, first, n                      n%32  tail                     launch shape
    ("tiny", 1024, 1000, 64, 64),          #               0     much longer              one workgroup per plane
    ("tiny", 1024, 1000, 60, 62),          #               30    much longer              one workgroup per plane
    ("tiny", 1024, 900, 450, 225),         #               1     equal                    windows
    ("tiny", 1024, 1024, 33, 95),          #               31    longer, kv_len == lmax   one workgroup per plane
    ("tiny", 1024, 700, 600, 100),         #               4     none: nothing to rotate
    ("tiny", 1024, 777, 0, 1),             #               1     first == 0, one row
    ("gqa2", 256, 256, 17, 239),           #               15    none, kv_len == lmax
    ("small", 2048, 2000, 130, 400),       #               16    much longer (overlap)    windows (5 launches)
    ("7b_planes", 1024, 1000, 450, 275),   #               19    equal, 224 planes        windows
]


def _finite_k(shape, seed):
    """bf16 bit patterns of finite keys [..., rows, 128]: normal draws at scales 1e-3, 1 and 1e3 in different rows, some exact zeros
    and some bf16 denormals."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    rows = torch.arange(shape[-2]).view(-1, 1)
    x = x * torch.tensor([1e-3, 1.0, 1e3])[rows % 3]
    u = torch.rand(shape, generator=g)
    bits = x.to(torch.bfloat16).view(torch.int16).clone()
    bits[u < 0.01] = 0
    den = torch.randint(1, 128, shape, generator=g, dtype=torch.int32) | (torch.randint(0, 2, shape, generator=g, dtype=torch.int32) << 15)
    den = torch.where(den >= 32768, den - 65536, den).to(torch.int16)                 # 0x0001 .. 0x007f with either sign
    sel = (u >= 0.01) & (u < 0.02)
    bits[sel] = den[sel]
    return bits


def _arena(lay, lmax, dev, seed, guard):
    """[guard | arena | guard]: random bf16 bit patterns everywhere (NaN / inf patterns included), finite keys in the K planes."""
    n = lay[0] * 2 * lay[1] * lmax * 128
    g = torch.Generator(device=dev).manual_seed(seed)
    buf = torch.randint(-32768, 32768, (guard + n + guard,), dtype=torch.int32, device=dev, generator=g).to(torch.int16)
    buf[guard:guard + n].view(lay[0], 2, lay[1], lmax, 128)[:, 0] = _finite_k((lay[0], lay[1], lmax, 128), seed).to(dev)
    return buf, n


@pytest.mark.parametrize("name,lmax,L,first,n", KERNEL_CASES)
def test_kv_evict_rebase_kernel_matches_the_float64_formula(dev, name, lmax, L, first, n):
    """Everything but the rotated K elements bit for bit; every rotated element within half a bf16 ulp of the float64 value plus
    three fp32 roundings of products bounded by |a| + |b|: |got - x| <= 2^-8 |x| + 2^-21 (|a| + |b|) + 2^-133."""
    from livecc_amd import _lib
    lib = _lib.load()
    lay = LAYOUTS[name]
    numel = lay[0] * 2 * lay[1] * lmax * 128
    guard = numel if numel <= (8 << 20) else 4 << 20
    buf, numel = _arena(lay, lmax, dev, seed=first * 131 + n, guard=guard)
    assert buf.data_ptr() % 256 == 0 and (guard * 2) % 256 == 0
    before = buf.cpu().numpy().view(np.uint16)
    b5 = before[guard:guard + numel].reshape(lay[0], 2, lay[1], lmax, 128)
    assert np.isnan(bf16_to_f64(b5[:, 1])).any() and np.isfinite(bf16_to_f64(b5[:, 0])).all()
    cos, sin = rot_table(n)                                           # theta = 1e6, float64, rounded to fp32
    rot = torch.from_numpy(np.concatenate([cos, sin])).to(dev)
    want = before.copy()
    want[guard:guard + numel] = rebase_arena_numpy(before[guard:guard + numel], lay[0], lay[1], lmax, L, first, n, cos, sin)
    kl = _lib.KvLayout(lay[0], lay[1], lmax, 128)
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.lcc_kv_evict_rebase_bf16(buf.data_ptr() + guard * 2, kl, L, first, n, rot.data_ptr(), st), "lcc_kv_evict_rebase_bf16")
    torch.cuda.synchronize(dev)
    got = buf.cpu().numpy().view(np.uint16)
    assert np.array_equal(got[:guard], before[:guard]) and np.array_equal(got[guard + numel:], before[guard + numel:]), "a neighbouring arena was written"
    g5 = got[guard:guard + numel].reshape(lay[0], 2, lay[1], lmax, 128)
    w5 = want[guard:guard + numel].reshape(lay[0], 2, lay[1], lmax, 128)
    assert np.array_equal(g5[:, 1], w5[:, 1]), "V planes are compacted bit for bit"
    assert np.array_equal(g5[:, 0, :, :first], b5[:, 0, :, :first]), "K rows below first changed"
    assert not g5[:, 0, :, L - n:L].any(), "vacated K rows are not zero"
    assert np.array_equal(g5[:, 0, :, L:], b5[:, 0, :, L:]), "K rows at or above kv_len were written"
    masked = got.copy()
    masked[guard:guard + numel].reshape(lay[0], 2, lay[1], lmax, 128)[:, 0, :, first:L - n] = w5[:, 0, :, first:L - n]
    assert np.array_equal(masked, want), "something outside the rotated K rows differs from the oracle"
    if L - n <= first:
        return                                                        # no tail: the whole arena was compared bit for bit
    src = b5[:, 0, :, first + n:L]
    x = rotate_rows_f64(src, cos.astype(np.float64), sin.astype(np.float64))
    k = np.abs(bf16_to_f64(src))
    ab = np.concatenate([k[..., :64] + k[..., 64:]] * 2, axis=-1)
    y = bf16_to_f64(g5[:, 0, :, first:L - n])
    err, bound = np.abs(y - x), 2.0 ** -8 * np.abs(x) + 2.0 ** -21 * ab + 2.0 ** -133
    worst = float((err / bound).max())
    exact = float((g5[:, 0, :, first:L - n] == w5[:, 0, :, first:L - n]).mean())
    print(f"{name} lmax {lmax} L {L} first {first} n {n}: worst err / bound {worst:.3f}, {exact:.4%} of the rotated elements equal the float64 RNE value")
    assert np.isfinite(y).all() and (err <= bound).all(), f"worst err / bound = {worst:.3f}"
    assert (g5[:, 0, :, first:L - n] != src).any(), "a plain copy: nothing was rotated"


# ---- 5. refusals write nothing -------------------------------------------------------------------------------------------------------
def test_kv_evict_rebase_refuses_bad_calls_and_writes_nothing(dev):
    from livecc_amd import _lib
    lib = _lib.load()
    buf, numel = _arena((2, 1), 256, dev, seed=1, guard=0)
    before = buf.clone()
    rot = torch.from_numpy(np.concatenate(rot_table(10))).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    ok = _lib.KvLayout(2, 1, 256, 128)
    for kl, L, first, n, code in ((ok, 200, -1, 10, STATE), (ok, 200, 10, 0, STATE), (ok, 200, 150, 51, STATE), (ok, 200, 201, 1, STATE),
                                  (ok, 257, 0, 10, STATE), (ok, -1, 0, 1, STATE), (ok, 200, 10, -5, STATE),
                                  (_lib.KvLayout(2, 1, 256, 64), 200, 10, 10, SHAPE), (_lib.KvLayout(2, 1, 250, 128), 200, 10, 10, SHAPE),
                                  (_lib.KvLayout(0, 1, 256, 128), 200, 10, 10, SHAPE)):
        assert lib.lcc_kv_evict_rebase_bf16(buf.data_ptr(), kl, L, first, n, rot.data_ptr(), st) == code, (L, first, n)
        assert lib.lcc_last_error() != b""
    assert lib.lcc_kv_evict_rebase_bf16(None, ok, 200, 10, 10, rot.data_ptr(), st) == ARG
    assert lib.lcc_kv_evict_rebase_bf16(buf.data_ptr(), ok, 200, 10, 10, None, st) == ARG
    assert lib.lcc_kv_evict_rebase_bf16(buf.data_ptr() + 2, ok, 200, 10, 10, rot.data_ptr(), st) == ALIGN
    assert lib.lcc_kv_evict_rebase_bf16(buf.data_ptr(), ok, 200, 10, 10, rot.data_ptr() + 2, st) == ALIGN
    torch.cuda.synchronize(dev)
    assert torch.equal(buf, before)


# ---- shared: a stream replayed turn by turn (the _Replay of tests/test_gpu_kv_window.py with `rebase=`) ---------------------------
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
        self.state = r.past_key_values
        seq = r.sequences[0].cpu().numpy()
        self.spans.append((0 if self.past_ids is None else len(self.past_ids), len(seq) - 1))
        self.past_ids = seq[:-1]
        return r

    def evict_rows(self, first, n, rebase):
        kept = np.concatenate([self.past_ids[:first], self.past_ids[first + n:]])
        self.state.evict(first, n, kept, rebase=rebase)
        self.past_ids = kept

    def evict_turns(self, t0, t1, rebase):
        first, n = self.spans[t0][0], self.spans[t1][1] - self.spans[t0][0]
        self.evict_rows(first, n, rebase)
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


def test_slot_evict_rebase_refuses_a_shift_below_position_zero(tiny_native):
    eng = tiny_native.engine
    a = _tiny_replay(tiny_native)
    a.turn(0); a.turn(1)
    slot = a.state.slot
    L, pos = eng.slot_length(slot)
    eng.set_slot_length(slot, L, 9)                              # a stream whose next position is below the shift asked for
    torch.cuda.synchronize()
    arena = eng._kv[slot].clone()
    first, n = a.spans[1][0], 10
    kept = np.ascontiguousarray(np.concatenate([a.past_ids[:first], a.past_ids[first + n:]]), dtype=np.int32)
    assert eng.lib.lcc_slot_evict_rebase(eng.h, slot, first, n, kept.ctypes.data, len(kept), eng._stream()) == STATE
    assert b"position" in eng.lib.lcc_last_error()
    assert eng.lib.lcc_slot_evict_rebase(eng.h, slot, first, L, kept.ctypes.data, len(kept), eng._stream()) == STATE     # range, as lcc_slot_evict
    assert eng.lib.lcc_slot_evict_rebase(eng.h, slot, first, n, kept.ctypes.data, len(kept) - 1, eng._stream()) == ARG
    torch.cuda.synchronize()
    assert eng.slot_length(slot) == (L, 9) and torch.equal(eng._kv[slot], arena)
    eng.set_slot_length(slot, L, pos)
    with pytest.raises(ValueError):
        a.state.evict(first, L, kept, rebase=True)
    assert eng.slot_length(slot) == (L, pos) and torch.equal(eng._kv[slot], arena)
    a.state.release()


# ---- 6. engine against HF ---------------------------------------------------------------------------------------------------------
def test_rebased_stream_matches_hf_with_the_same_rows_cut_and_keys_rotated(dev):
    """small() config, HF live on the host (bf16 and fp32): 7 turns, turn 1 evicted before turn 4 and turn 2 before turn 6, both with
    rebase=True natively and tests/test_kv_rebase.py::hf_cut_rebase on both oracles -- turn 3's keys are rotated twice, turns 4-5
    once.  Every native step is teacher-forced on the bf16 oracle's tokens.  Bounds: those of tests/test_gpu_kv_window.py, the same
    before and after the evictions (the bf16 oracle re-rounds its own keys the same way, so its error carries the same term)."""
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
    frames = torch.from_numpy(protocol.synth_frames(6 + 2 * 6, 112, 140, seed=77, layout="TCHW"))
    rp = _Replay(native, cfg, frames, protocol.TurnBuilder(cfg, seed=77))
    s16, s32 = O.OracleStream(hf16, cfg), O.OracleStream(hf32, cfg)
    PEN, NEW = 1.15, 4
    worst = {"before": [0.0, 0.0], "after": [0.0, 0.0]}
    for ti in range(7):
        if ti in (4, 6):
            L, pos = native.engine.slot_length(rp.state.slot)
            delta = rp.state.rope_delta
            first, n = rp.evict_turns(1, 1, rebase=True)        # the oldest turn after the head: original turn 1, then original turn 2
            assert native.engine.slot_length(rp.state.slot) == (L - n, pos - n) and rp.state.rope_delta == delta
            assert first == rp.spans[0][1] and n >= 1
            for s in (s16, s32):
                hf_cut_rebase(s, first, n, cfg)
                assert s.past_key_values.get_seq_length() + int(s.rope_deltas) == pos - n
            assert np.array_equal(s16.past_ids[0].numpy(), rp.past_ids) and np.array_equal(s32.past_ids[0].numpy(), rp.past_ids)
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
    record("kv_rebase_small_vs_hf", dict(worst_rel_dlogit_before=worst["before"][0], worst_err_ratio_before=worst["before"][1],
                                         worst_rel_dlogit_after=worst["after"][0], worst_err_ratio_after=worst["after"][1]))
    rp.state.release()


# ---- 7. engine against itself -----------------------------------------------------------------------------------------------------
def test_rebased_eviction_of_the_last_turn_equals_truncation(tiny_native):
    """Rows of the LAST cached turn evicted with rebase=True (no tail: nothing to rotate) == `set_slot_length(first, pos - n)` with
    `rope_delta` unchanged: the next two turns' logits and sequences are bit-identical between the two routes."""
    a, b = _tiny_replay(tiny_native), _tiny_replay(tiny_native)
    for ti in range(3):
        ra, rb = a.turn(ti), b.turn(ti)
        assert torch.equal(ra.sequences, rb.sequences) and torch.equal(ra.logits, rb.logits)
    eng = tiny_native.engine
    (L, pos), first = eng.slot_length(a.state.slot), a.spans[2][0]
    n, delta = L - first, a.state.rope_delta
    a.evict_turns(2, 2, rebase=True)
    eng.set_slot_length(b.state.slot, first, pos - n)
    b.past_ids, b.spans = b.past_ids[:first], b.spans[:2]
    assert eng.slot_length(a.state.slot) == eng.slot_length(b.state.slot) == (first, pos - n) and np.array_equal(a.past_ids, b.past_ids)
    assert a.state.rope_delta == b.state.rope_delta == delta
    forced = [5, 6, 7, 8]
    ra, rb = a.turn(3, teacher=forced), b.turn(3, teacher=forced)
    assert torch.equal(ra.logits, rb.logits) and bool(torch.isfinite(ra.logits.float()).all())
    ra, rb = a.turn(4, repetition_penalty=1.0), b.turn(4, repetition_penalty=1.0)
    assert torch.equal(ra.logits, rb.logits) and torch.equal(ra.sequences, rb.sequences)
    a.state.release(); b.state.release()


# ---- 8. every key moves: invisible ------------------------------------------------------------------------------------------------
def test_rebasing_every_kept_key_is_invisible(tiny_native):
    """Rows [0, 37) evicted before turn 3, once plainly and once rebased: every kept key moves down by 37, every relative position
    stays, so the next turn's logits (teacher-forced) agree up to one more bf16 rounding of K: within 6e-2 x the logit scale (HF in
    bf16 shows 1.3e-2 x)."""
    from tests.util import record
    eng = tiny_native.engine
    a, b = _tiny_replay(tiny_native), _tiny_replay(tiny_native)
    for ti in range(2):
        ra, rb = a.turn(ti), b.turn(ti)
        assert torch.equal(ra.logits, rb.logits)
    assert a.spans[0][1] > 37
    (L, pos), da, db = eng.slot_length(a.state.slot), a.state.rope_delta, b.state.rope_delta
    a.evict_rows(0, 37, rebase=False)
    b.evict_rows(0, 37, rebase=True)
    assert eng.slot_length(a.state.slot) == (L - 37, pos) and a.state.rope_delta == da + 37
    assert eng.slot_length(b.state.slot) == (L - 37, pos - 37) and b.state.rope_delta == db
    forced = [5, 6, 7, 8]
    ra, rb = a.turn(2, teacher=forced), b.turn(2, teacher=forced)
    la, lb = ra.logits.float().cpu(), rb.logits.float().cpu()
    scale = la.abs().max().item()
    d = (la - lb).abs().max().item()
    print(f"plain vs rebased eviction of rows [0, 37): worst |dlogit| {d:.4g} at logit scale {scale:.3g} ({d / scale:.3e} x)")
    record("kv_rebase_tiny_invisible", dict(worst_abs_dlogit=d, logit_scale=scale, rel=d / scale))
    assert bool(torch.isfinite(lb).all()) and d <= GROSS_REL * scale
    a.state.release(); b.state.release()


# ---- 9. batch invariance and fork -------------------------------------------------------------------------------------------------
def test_batch_invariance_and_fork_after_a_rebase(tiny_native):
    a, b, alone = _tiny_replay(tiny_native, seed=31), _tiny_replay(tiny_native, seed=32), _tiny_replay(tiny_native, seed=32)
    for ti in range(3):
        a.turn(ti)
    for ti in range(2):
        b.turn(ti); alone.turn(ti)
    a.evict_turns(1, 1, rebase=True)
    (ia, ca), (ib, cb) = a.request(3), b.request(2)
    kw = dict(repetition_penalty=1.05, max_new_tokens=4, force_length=True, output_logits=True)
    outs = tiny_native.generate_batch([dict(input_ids=torch.from_numpy(ia), frames=ca, frames_layout="TCHW", state=a.state),
                                       dict(input_ids=torch.from_numpy(ib), frames=cb, frames_layout="TCHW", state=b.state)], **kw)
    solo = tiny_native.generate_batch([dict(input_ids=torch.from_numpy(ib), frames=cb, frames_layout="TCHW", state=alone.state)], **kw)[0]
    assert torch.equal(outs[1].sequences, solo.sequences) and torch.equal(outs[1].logits, solo.logits), "the neighbour equals itself alone"
    for s in (a, b, alone):
        s.state.release()
    # the rebased stream is served the same in the batch as alone; a fork taken right after the rebase equals its source
    a2 = _tiny_replay(tiny_native, seed=31)
    for ti in range(3):
        a2.turn(ti)
    a2.evict_turns(1, 1, rebase=True)
    fork = a2.state.fork()
    eng = tiny_native.engine
    assert eng.slot_length(fork.slot) == eng.slot_length(a2.state.slot) and fork.rope_delta == a2.state.rope_delta
    ids, clip = a2.request(3)
    toks = outs[0].sequences[0, -4:].tolist()
    gen = dict(input_ids=torch.from_numpy(ids).view(1, -1), frames=clip, frames_layout="TCHW", do_sample=False, repetition_penalty=1.05,
               max_new_tokens=4, min_new_tokens=4, output_logits=True)
    rf = tiny_native.generate(past_key_values=fork, teacher_tokens=toks, **gen)
    ra2 = tiny_native.generate(past_key_values=a2.state, **gen)
    assert torch.equal(outs[0].sequences, ra2.sequences) and torch.equal(outs[0].logits, ra2.logits), "the rebased stream equals itself alone"
    assert torch.equal(rf.logits, ra2.logits) and bool(torch.isfinite(rf.logits.float()).all()), "fork and source agree bit for bit"
    fork.release(); a2.state.release()


# ---- 10. server and live_cc end to end --------------------------------------------------------------------------------------------
def test_slide_rebase_server_keeps_positions_inside_the_slot(dev):
    """The scenario of tests/test_gpu_kv_window.py::test_slide_server_streams_three_windows_without_end (small() model, a 256-row KV
    slot, a 40-s clip) under "slide_rebase": no window_full, no error, >= 2 evictions, the short neighbour's tokens are those it
    yields alone, and after every result the next rope position is inside the slot.  The same run under "slide" ends above
    3 x the slot: the difference this mode exists for."""
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

    def serve(vids, policy):
        srv = StreamServer(LiveCCDemoInfer(model=native, turn_builder=FixedIds(native.cfg)), max_new_tokens=NEW, force_length=True,
                           window_policy=policy)
        for sid, v in vids.items():
            srv.add_stream(sid, *v, t_start=0.0, max_pixels=4 * 28 * 28)
        seen = []
        out = srv.run(realtime=False, on_result=lambda sid, span, text, st: seen.append(
            (sid, len(st["past_ids"]), native.engine.slot_length(st["past_key_values"].slot), st["past_key_values"].rope_delta)
            if st.get("past_key_values") else None))
        for sid in list(vids):
            srv.remove_stream(sid)
        return out, seen
    long_v, short_v = video(1, 1200), video(2, 150)
    out, seen = serve({"long": long_v, "short": short_v}, "slide_rebase")
    by = {}
    for sid, span, text, st in out:
        by.setdefault(sid, []).append((span, text, st))
    assert not any(st.get("window_full") or "error" in st or st.get("restarted") for _, _, st in by["long"] + by["short"])
    assert by["long"][-1][0][1] >= 39.0 and len(by["long"]) == 38
    slid = [st for _, _, st in by["long"] if st.get("slid")]
    assert len(slid) >= 2 and [st["evictions"] for st in slid] == list(range(1, len(slid) + 1))
    assert all(st["evicted_turns"] >= 1 and st.get("rebased") is True for st in slid)
    assert not any(st.get("slid") or st.get("rebased") for _, _, st in by["short"])
    assert all(x is not None for x in seen)
    assert all(n_ids == kv for _, n_ids, (kv, _), _ in seen), "past_ids and the device KV length agree"
    assert all(pos <= MAXKV for _, _, (_, pos), _ in seen), "the next rope position stays inside the slot"
    assert all(pos == kv + delta for _, _, (kv, pos), delta in seen), "next position = kv_len + rope_delta, always"
    assert len({delta for sid, _, _, delta in seen if sid == "long"}) == 1, "rope_delta never changes after the first turn"
    solo, _ = serve({"short": short_v}, "slide_rebase")
    assert [(s, t) for s, t, _ in by["short"]] == [(span, text) for _, span, text, _ in solo] and len(solo) == 3
    assert all(t != "" for _, t, _ in by["short"] + by["long"])
    # the plain slide keeps the cache inside the slot and lets the positions run away
    out_s, seen_s = serve({"long": long_v}, "slide")
    last = [x for x in seen_s if x[0] == "long"][-1]
    assert len(out_s) == 38 and last[2][0] <= MAXKV and last[2][1] > 3 * MAXKV, f"'slide' ended at position {last[2][1]}"
    assert not any("rebased" in st for _, _, _, st in out_s)


def test_live_cc_slide_rebase_keeps_positions_inside_the_slot(dev):
    from livecc_amd.config import tiny
    from livecc_amd.infer import LiveCCDemoInfer
    from livecc_amd.modeling import LiveCCForConditionalGeneration
    from livecc_amd.video import DecodedVideo
    native = LiveCCForConditionalGeneration.from_config(tiny(), dev, seed=0, max_streams=1, max_kv_len=256, max_new_rows=512, max_patches=2048,
                                                        max_history=8)
    g = torch.Generator().manual_seed(5)
    frames, pts = torch.randint(0, 256, (600, 60, 90, 3), dtype=torch.uint8, generator=g).to(dev), np.arange(600) / 30.0     # 20 s
    infer = LiveCCDemoInfer(model=native)
    state, spans, deltas = {"video_path": DecodedVideo(frames, pts, 30.0)}, [], []
    try:
        for wall in np.arange(0.0, 21.0, 0.5):
            state["video_timestamp"] = float(wall)
            for span, text, state in infer.live_cc(None, state, max_pixels=4 * 28 * 28, max_new_tokens=4, force_length=True, do_sample=False,
                                                  kv_window="slide_rebase"):
                spans.append(span)
                kv, pos = native.engine.slot_length(state["past_key_values"].slot)
                assert len(state["past_ids"]) == kv <= 256 and pos <= 256 and pos == kv + state["past_key_values"].rope_delta
                deltas.append(state["past_key_values"].rope_delta)
    finally:
        if state.get("past_key_values") is not None:
            state["past_key_values"].release()
    assert spans[0] == (0.0, 3.0) and spans[-1][1] >= 19.5 and state.get("evictions", 0) >= 2
    assert state["turn_spans"][0][0] == 0 and state["turn_spans"][-1][1] == len(state["past_ids"])
    assert len(set(deltas)) == 1, "rope_delta is the first turn's for ever"
    with pytest.raises(ValueError):
        next(LiveCCDemoInfer(model=native).live_cc(None, {"video_path": DecodedVideo(frames, pts, 30.0)}, kv_window="ring"))

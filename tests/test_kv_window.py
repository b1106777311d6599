"""Sliding KV window, host side (CPU tier): the eviction planner, the numpy statement of the blocked-transposed V index map (the
expected-value generator of tests/test_gpu_kv_window.py), `StreamServer(window_policy="slide")` over the stand-in models of
tests/test_server_logic.py, and HF's own statement of the contract (rows cut out of its DynamicCache, `rope_deltas` raised by n)."""
import functools

import numpy as np
import pytest
import torch

from livecc_amd import protocol, server
from tests.test_server_logic import CapModel, FakeInfer, _video


# ---- 1. planner -----------------------------------------------------------------------------------------------------------------
def _random_spans(rng, n_turns, lo=20, hi=120):
    ends = np.cumsum(rng.integers(lo, hi, n_turns))
    return [(int(b), int(e)) for b, e in zip(np.concatenate([[0], ends[:-1]]), ends)]


@pytest.mark.parametrize("seed", range(40))
def test_plan_eviction_properties(seed):
    rng = np.random.default_rng(seed)
    spans = _random_spans(rng, int(rng.integers(1, 30)))
    kv_len = spans[-1][1]
    need = int(rng.integers(1, 150))
    cap = int(rng.integers(max(need, 50), kv_len + need + 200))
    keep = int(rng.integers(0, 3))
    low = float(rng.choice([0.25, 0.5, 0.75, 1.0]))
    plan = protocol.plan_eviction(spans, kv_len, need, cap, keep_head_turns=keep, low_water=low)
    if kv_len + need <= cap:
        assert plan is None, "no eviction while the next turn fits"
        return
    droppable = spans[keep:]
    all_n = droppable[-1][1] - droppable[0][0] if droppable else 0
    if kv_len - all_n + need > cap:
        assert plan is None, "even dropping everything but the head makes no room"
        return
    first, n, k = plan
    assert 1 <= k <= len(droppable) and n >= 1
    assert first == droppable[0][0] and first + n == droppable[k - 1][1], "one contiguous, turn-aligned range right after the head"
    assert first >= (spans[keep - 1][1] if keep else 0), "head turns are never dropped"
    assert kv_len - n + need <= cap
    reachable = kv_len - all_n + need <= low * cap
    if reachable:
        assert kv_len - n + need <= low * cap
        if k > 1:   # ... and no more turns than that takes
            assert kv_len - (droppable[k - 2][1] - first) + need > low * cap
    else:
        assert k == len(droppable), "low-water mark out of reach: everything droppable goes"


def test_plan_eviction_7b_cadence_and_bad_tables():
    """7B shapes: ~400-row turns in a 32k window -> one eviction frees about half the window, i.e. ~40 turns until the next."""
    spans, pos = [], 0
    for t in range(81):
        n = 1200 if t == 0 else 402
        spans.append((pos, pos + n))
        pos += n
    cap = 32768
    assert pos + 402 > cap
    first, n, k = protocol.plan_eviction(spans, pos, 402, cap)
    assert first == 1200 and n == k * 402
    assert pos - n + 402 <= 0.5 * cap < pos - n + 402 + 402, "as few turns as reach the low-water mark"
    assert 38 <= (cap - (pos - n)) // 402 <= 42, "turns until the window is full again"
    with pytest.raises(ValueError):
        protocol.plan_eviction([(0, 10), (12, 20)], 20, 5, 22)          # a gap
    with pytest.raises(ValueError):
        protocol.plan_eviction([(0, 10), (10, 20)], 25, 5, 22)          # does not cover the cache
    assert protocol.plan_eviction([(0, 10)], 10, 20, 22) is None        # only the head is cached


# ---- 2. the arena layout in numpy: expected values of the kernel test ---------------------------------------------------------
def blocked(j):
    """Key j of a V plane [Lmax/32][128][32] lives in block j // 32, column j % 32 (csrc/kernels.h KvLayout)."""
    return j // 32, j % 32


def v_natural(plane_blocked: np.ndarray) -> np.ndarray:
    """[Lmax/32][128][32] -> [Lmax][128] (key-major, as the K plane)."""
    nb = plane_blocked.shape[0]
    return plane_blocked.transpose(0, 2, 1).reshape(nb * 32, 128)


def v_blocked(plane_natural: np.ndarray) -> np.ndarray:
    lmax = plane_natural.shape[0]
    return np.ascontiguousarray(plane_natural.reshape(lmax // 32, 32, 128).transpose(0, 2, 1))


def evict_rows(nat: np.ndarray, L: int, first: int, n: int) -> np.ndarray:
    """The contract on a key-major plane: rows first + n .. L move down by n, rows [L - n, L) become zero, everything else stays."""
    out = nat.copy()
    out[first:L - n] = nat[first + n:L]
    out[L - n:L] = 0
    return out


def evict_v_blocked_indexwise(vb: np.ndarray, L: int, first: int, n: int) -> np.ndarray:
    """The same contract stated on the BLOCKED layout, index by index: destination (block d, column c) of key j' = 32 d + c takes
    source key j = j' + n = (block j // 32, column j % 32)."""
    out = vb.copy()
    for jd in range(first, L):
        d, c = blocked(jd)
        if jd < L - n:
            sb, sc = blocked(jd + n)
            out[d, :, c] = vb[sb, :, sc]
        else:
            out[d, :, c] = 0
    return out


def evict_arena_numpy(arena: np.ndarray, n_layers: int, n_kv_heads: int, lmax: int, L: int, first: int, n: int) -> np.ndarray:
    """Expected arena (uint16 bit patterns, [layer][K|V][Hkv][lmax * 128]) after evicting rows [first, first + n) of L cached rows."""
    a = arena.reshape(n_layers, 2, n_kv_heads, lmax * 128).copy()
    for l in range(n_layers):
        for h in range(n_kv_heads):
            a[l, 0, h] = evict_rows(a[l, 0, h].reshape(lmax, 128), L, first, n).reshape(-1)
            nat = v_natural(a[l, 1, h].reshape(lmax // 32, 128, 32))
            a[l, 1, h] = v_blocked(evict_rows(nat, L, first, n)).reshape(-1)
    return a.reshape(arena.shape)


@pytest.mark.parametrize("s", range(32))
def test_v_index_map_round_trips_for_every_column_rotation(s):
    rng = np.random.default_rng(s)
    lmax = 256
    vb = rng.integers(1, 65536, (lmax // 32, 128, 32)).astype(np.uint16)
    assert np.array_equal(v_blocked(v_natural(vb)), vb)
    for j in (0, 31, 32, 77, lmax - 1):
        b, c = blocked(j)
        assert np.array_equal(v_natural(vb)[j], vb[b, :, c])
    for L, first, n in ((lmax, 5, 32 + s), (200, 64, 64 + s), (lmax - 3, 33, max(s, 1)), (150, 150 - max(s, 1), max(s, 1))):
        assert n % 32 == s % 32 or s == 0
        want = v_blocked(evict_rows(v_natural(vb), L, first, n))
        assert np.array_equal(evict_v_blocked_indexwise(vb, L, first, n), want)
        nat = v_natural(want)
        assert not nat[L - n:L].any() and np.array_equal(nat[L:], v_natural(vb)[L:]) and np.array_equal(nat[:first], v_natural(vb)[:first])


def test_evict_arena_numpy_touches_k_and_v_of_every_plane():
    rng = np.random.default_rng(0)
    nl, hk, lmax = 2, 2, 64
    arena = rng.integers(1, 65536, nl * 2 * hk * lmax * 128).astype(np.uint16)
    out = evict_arena_numpy(arena, nl, hk, lmax, 60, 10, 7).reshape(nl, 2, hk, lmax * 128)
    src = arena.reshape(nl, 2, hk, lmax * 128)
    for l in range(nl):
        for h in range(hk):
            k0, k1 = src[l, 0, h].reshape(lmax, 128), out[l, 0, h].reshape(lmax, 128)
            assert np.array_equal(k1[10:53], k0[17:60]) and not k1[53:60].any() and np.array_equal(k1[60:], k0[60:])
            v0, v1 = v_natural(src[l, 1, h].reshape(2, 128, 32)), v_natural(out[l, 1, h].reshape(2, 128, 32))
            assert np.array_equal(v1[10:53], v0[17:60]) and not v1[53:60].any() and np.array_equal(v1[60:], v0[60:])


# ---- 3. StreamServer(window_policy="slide") over the stand-in models ------------------------------------------------------------
class SlideModel(CapModel):
    """CapModel whose KV handles can `evict`; checks on its side that every range is turn-aligned, spares the head turn, and that
    the ids sent after a slide are the kept past ids + the new turn."""

    def __init__(self, cfg, max_kv_len, max_history=3):
        super().__init__(cfg, max_kv_len, max_history)
        self.evicts, self.spans, self.kept, self.checked_after_slide = [], {}, {}, 0
        self.engine.max_kv_len, self.engine.max_history = max_kv_len, max_history

    def _evict(self, kv, first, n, kept_ids):
        spans = self.spans[kv.slot]
        begins, ends = [b for b, _ in spans], [e for _, e in spans]
        assert first in begins and first + n in ends, f"[{first}, {first + n}) is not turn-aligned in {spans}"
        assert first >= spans[0][1], "the head turn is never evicted"
        assert len(kept_ids) == self.lengths[kv.slot] - n
        i, j = begins.index(first), ends.index(first + n)
        self.spans[kv.slot] = spans[:i] + [(b - n, e - n) for b, e in spans[j + 1:]]
        self.lengths[kv.slot] -= n
        self.kept[kv.slot] = np.asarray(kept_ids).copy()
        self.evicts.append((kv.slot, first, n))

    def generate_batch(self, reqs, **kw):
        for r in reqs:
            st = r["state"]
            if st is not None and st.slot in self.kept:
                kept, ids = self.kept.pop(st.slot), r["input_ids"].numpy()
                assert len(ids) > len(kept) and np.array_equal(ids[:len(kept)], kept), "ids after a slide = kept past ids + new turn"
                self.checked_after_slide += 1
        before = {r["state"].slot: self.lengths.get(r["state"].slot, 0) for r in reqs if r["state"] is not None}
        outs = super().generate_batch(reqs, **kw)
        for o in outs:
            kv = o.past_key_values
            if not hasattr(kv, "evict"):
                kv.evict = functools.partial(self._evict, kv)
            self.spans.setdefault(kv.slot, []).append((before.get(kv.slot, 0), self.lengths[kv.slot]))
        return outs


def _slide_server(monkeypatch, max_kv_len, **kw):
    def fake_clip(frames, h, w, ts, pts, index_from, layout="THWC"):
        from livecc_amd import resize as R
        idxs, kept = R.select_clip_frames(ts, pts, index_from)
        return (torch.zeros(len(idxs), 3, h, w, dtype=torch.uint8) if idxs else None), kept, idxs
    monkeypatch.setattr(server.R, "get_smart_resized_clip", fake_clip)
    inf = FakeInfer()
    inf.model = SlideModel(inf.cfg, max_kv_len)
    return server.StreamServer(inf, max_new_tokens=3, **kw)


def _by_stream(out):
    by = {}
    for sid, span, text, state in out:
        by.setdefault(sid, []).append((span, text, state))
    return by


def test_slide_policy_streams_without_end(monkeypatch):
    srv = _slide_server(monkeypatch, max_kv_len=160, window_policy="slide")
    srv.add_stream("long", *_video(1800), t_start=0.0, max_pixels=4 * 28 * 28)      # 60 s: many times the 160-row window
    srv.add_stream("short", *_video(150), t_start=0.0, max_pixels=4 * 28 * 28)
    out = srv.run(realtime=False)
    m, by = srv.model, _by_stream(out)
    spans = [s for s, _, _ in by["long"]]
    assert spans[0] == (0.0, 3.0) and spans[-1][1] >= 59.0 and all(b - a == 1.0 for a, b in spans[1:]), "every chunk was served"
    assert not any(st.get("window_full") or "error" in st or st.get("restarted") for _, _, st in by["long"] + by["short"])
    assert all(t != "" for _, t, _ in by["long"])
    slid = [st for _, _, st in by["long"] if st.get("slid")]
    assert len(slid) >= 3 and [st["evictions"] for st in slid] == list(range(1, len(slid) + 1))
    assert all(st["evicted_turns"] >= 1 for st in slid) and srv.streams["long"].evictions == len(slid) == len(m.evicts)
    assert m.checked_after_slide == len(slid)
    assert not any(st.get("slid") for _, _, st in by["short"]) and [s for s, _, _ in by["short"]] == [(0.0, 3.0), (3.0, 4.0), (4.0, 5.0)]
    # hysteresis: an eviction goes down to half the window, so slides are several turns apart (not one per turn)
    assert len(slid) <= len(by["long"]) // 2
    long_slot = m.evicts[0][0]
    assert m.lengths[long_slot] + m.engine.max_history <= 160


def test_slide_uses_the_exact_turn_length(monkeypatch):
    """The slide is decided on the built turn's length -- neither one chunk early (the `+ 64` estimate of the other policies) nor late:
    every call the engine sees satisfies its own rule, and no slide happens while the exact turn still fits."""
    srv = _slide_server(monkeypatch, max_kv_len=160, window_policy="slide")
    srv.add_stream("v", *_video(900), t_start=0.0, max_pixels=4 * 28 * 28)
    m = srv.model
    sizes = []
    orig = m.generate_batch

    def spy(reqs, **kw):
        sizes.append((len(m.evicts), int(reqs[0]["input_ids"].numel())))
        return orig(reqs, **kw)
    m.generate_batch = spy
    srv.run(realtime=False)
    assert len(m.evicts) >= 2
    cap = 160 - m.engine.max_history
    assert all(n <= cap for _, n in sizes)
    for i in range(1, len(sizes)):
        if sizes[i][0] > sizes[i - 1][0]:           # a slide happened right before call i: without it the turn would not have fitted
            slot, first, n = m.evicts[sizes[i][0] - 1]
            assert sizes[i][1] + n > cap


def test_end_and_restart_policies_never_evict(monkeypatch):
    for policy in ("end", "restart"):
        srv = _slide_server(monkeypatch, max_kv_len=160, window_policy=policy)
        srv.add_stream("v", *_video(600), t_start=0.0, max_pixels=4 * 28 * 28)
        out = srv.run(realtime=False)
        assert srv.model.evicts == [] and not any(st.get("slid") for _, _, _, st in out)
        if policy == "end":
            assert out[-1][3].get("window_full") is True and srv.streams["v"].window_full
        else:
            assert len([1 for _, _, _, st in out if st.get("restarted")]) >= 2 and out[-1][1][1] >= 19.0
    with pytest.raises(ValueError):
        server.StreamServer(FakeInfer(), window_policy="ring")


def test_slide_falls_back_to_window_full_when_nothing_can_be_dropped(monkeypatch):
    srv = _slide_server(monkeypatch, max_kv_len=160, window_policy="slide", slide_keep_head_turns=1000)
    srv.add_stream("v", *_video(600), t_start=0.0, max_pixels=4 * 28 * 28)
    out = srv.run(realtime=False)
    assert out[-1][3].get("window_full") is True and srv.model.evicts == []
    assert not any("error" in st for _, _, _, st in out)


# ---- 4. HF's own statement of the contract ---------------------------------------------------------------------------------------
def hf_cut(stream, first: int, n: int) -> None:
    """Evict rows [first, first + n) from an `oracle.hf_oracle.OracleStream` through its public attributes: the rows leave every
    layer of the DynamicCache, the same entries leave `past_ids`, and `rope_deltas` grows by n (cached keys keep their positions)."""
    for layer in stream.past_key_values.layers:
        layer.keys = torch.cat([layer.keys[:, :, :first], layer.keys[:, :, first + n:]], dim=2)
        layer.values = torch.cat([layer.values[:, :, :first], layer.values[:, :, first + n:]], dim=2)
    stream.past_ids = torch.cat([stream.past_ids[:, :first], stream.past_ids[:, first + n:]], dim=1)
    stream.rope_deltas = stream.rope_deltas + n


def test_hf_positions_continue_after_a_cache_cut():
    from livecc_amd.config import tiny
    from oracle import hf_oracle as O
    cfg = tiny()
    hf = O.build_hf_model(cfg, torch.bfloat16, 3, 2.0)
    frames = torch.from_numpy(protocol.synth_frames(6 + 2 * 4, 56, 84, seed=5, layout="TCHW"))
    chunks = protocol.split_clip(frames.shape[0])
    seen_pos = []
    hook = hf.model.language_model.register_forward_pre_hook(
        lambda mod, args, kwargs: seen_pos.append(kwargs["position_ids"].clone()) if kwargs.get("position_ids") is not None else None,
        with_kwargs=True)

    def run(cut_before=None):
        b, st = protocol.TurnBuilder(cfg, seed=7), O.OracleStream(hf, cfg)
        spans, outs, first_pos = [], [], []
        for ti, (a, e) in enumerate(chunks):
            pv, grid = O.patchify_normalize_ref(frames[a:e], cfg)
            ids = b.turn_ids(ti, protocol.num_video_tokens(grid, cfg))
            if ti == cut_before:
                lo, hi = spans[1][0], spans[2][1]
                next_pos = st.past_key_values.get_seq_length() + int(st.rope_deltas)
                hf_cut(st, lo, hi - lo)
                assert st.past_key_values.get_seq_length() + int(st.rope_deltas) == next_pos
                assert st.past_ids.shape[1] == st.past_key_values.get_seq_length() == spans[-1][1] - (hi - lo)
                first_pos.append(next_pos)
            n_before = 0 if st.past_ids is None else st.past_ids.shape[1]
            del seen_pos[:]
            outs.append(st.turn(ids, pv, grid, max_new_tokens=3, repetition_penalty=1.05))
            if ti == cut_before:
                p = seen_pos[0]                              # the prefill's position ids as HF computed them
                assert int(p.reshape(-1, p.shape[-1])[0, 0]) == first_pos[0], "HF continues at the old next position"
                assert p.shape[-1] == len(ids)
            spans.append((n_before, st.past_ids.shape[1]))
        return outs, spans
    try:
        full, spans = run()
        cut, _ = run(cut_before=4)
    finally:
        hook.remove()
    for ti in range(4):
        assert all(torch.equal(x, y) for x, y in zip(full[ti]["logits"], cut[ti]["logits"])), "turns before the cut are unchanged"
    assert not all(torch.equal(x, y) for x, y in zip(full[4]["logits"], cut[4]["logits"])), "the evicted context is gone"
    assert len(cut[4]["new_tokens"]) == 3

"""Sliding KV window with positions inside the cache ("rebase"), host side (CPU tier): the numpy statement of the re-rotation on the
arena layout (the expected-value generator of tests/test_gpu_kv_rebase.py), HF's own statement of the contract (rows cut out of its
DynamicCache, the kept keys rotated back by n positions, `rope_deltas` left alone), and `StreamServer(window_policy="slide_rebase")`
over the stand-in models of tests/test_kv_window.py."""
import numpy as np
import pytest
import torch

from livecc_amd import protocol, server
from tests.test_kv_window import SlideModel, _by_stream, evict_arena_numpy, hf_cut
from tests.test_server_logic import FakeInfer, _video


# ---- 1. the re-rotation in numpy: expected values of the kernel test ---------------------------------------------------------------
def bf16_to_f64(bits: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):                  # (signalling-NaN patterns of the V planes and guards)
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def f64_to_bf16_rne(x: np.ndarray) -> np.ndarray:
    """float64 -> bf16 bit patterns with ONE round-to-nearest-even (no intermediate fp32 rounding decides a tie)."""
    mag = np.abs(x)
    with np.errstate(over="ignore"):
        b32 = mag.astype(np.float32).view(np.uint32)
    down = b32 & np.uint32(0xFFFF0000)                   # a bf16 neighbour of |x| (the one below, unless the fp32 cast rounded up onto it)
    up = down + np.uint32(0x10000)
    d_lo, d_hi = mag - down.view(np.float32).astype(np.float64), up.view(np.float32).astype(np.float64) - mag
    even = (down >> 16) & 1 == 0
    pick = np.where((d_lo < d_hi) | ((d_lo == d_hi) & even), down, up)
    return ((pick >> 16).astype(np.uint16) | (np.signbit(x).astype(np.uint16) << 15)).astype(np.uint16)


def rotate_rows_f64(rows: np.ndarray, cos: np.ndarray, sin: np.ndarray) -> np.ndarray:
    """The formula of include/livecc_amd.h (lcc_kv_evict_rebase_bf16) in float64 on K rows [..., 128] of bf16 bit patterns:
    k'[i] = k[i] c_i + k[i + 64] s_i, k'[i + 64] = k[i + 64] c_i - k[i] s_i."""
    k = bf16_to_f64(rows)
    c, s = np.asarray(cos, dtype=np.float64), np.asarray(sin, dtype=np.float64)
    lo, hi = k[..., :64], k[..., 64:]
    return np.concatenate([lo * c + hi * s, hi * c - lo * s], axis=-1)


def rebase_arena_numpy(arena: np.ndarray, n_layers: int, n_kv_heads: int, lmax: int, L: int, first: int, n: int, cos, sin) -> np.ndarray:
    """Expected arena (uint16 bit patterns) after evicting rows [first, first + n) of L cached rows WITH the re-rotation:
    tests/test_kv_window.py::evict_arena_numpy, then K rows [first, L - n) of every K plane replaced by the float64 evaluation of
    the formula, rounded RNE to bf16."""
    a = evict_arena_numpy(arena, n_layers, n_kv_heads, lmax, L, first, n).reshape(n_layers, 2, n_kv_heads, lmax, 128).copy()
    if L - n > first:
        a[:, 0, :, first:L - n] = f64_to_bf16_rne(rotate_rows_f64(a[:, 0, :, first:L - n], cos, sin))
    return a.reshape(arena.shape)


def rot_table(n: int, theta: float = 1e6):
    """cos | sin of n * theta^(-i / 64), i in 0..63: float64, rounded to fp32 (what lcc_slot_evict_rebase ships)."""
    ang = n * (1.0 / theta ** (np.arange(64, dtype=np.float64) / 64.0))
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def test_f64_to_bf16_rne_is_torch_rounding_on_fp32_values_and_breaks_ties_to_even():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.normal(0, s, 4096) for s in (1e-3, 1.0, 1e3)] + [[0.0, -0.0, 2.0 ** -133, 3 * 2.0 ** -134, 2.0 ** -134, 1e-40]])
    x = x.astype(np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(f64_to_bf16_rne(x.astype(np.float64)), want)
    # ties decided on the float64 value: 1 + 2^-8 is halfway between bf16 1.0 (even) and 1.0078125; a hair above goes up
    assert f64_to_bf16_rne(np.array([1 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -40, 1 + 3 * 2.0 ** -8])).tolist() == [0x3F80, 0x3F81, 0x3F82]


def test_rebase_arena_numpy_only_changes_the_kept_k_rows():
    rng = np.random.default_rng(1)
    nl, hk, lmax, L, first, n = 2, 2, 64, 60, 10, 7
    arena = rng.integers(1, 65536, nl * 2 * hk * lmax * 128).astype(np.uint16)
    k = arena.reshape(nl, 2, hk, lmax, 128)[:, 0]
    k[...] = torch.from_numpy(rng.normal(0, 1, k.shape).astype(np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    plain = evict_arena_numpy(arena, nl, hk, lmax, L, first, n)
    cos, sin = rot_table(n)
    got = rebase_arena_numpy(arena, nl, hk, lmax, L, first, n, cos, sin)
    g5, p5 = got.reshape(nl, 2, hk, lmax, 128), plain.reshape(nl, 2, hk, lmax, 128)
    assert np.array_equal(g5[:, 1], p5[:, 1]), "V planes are only compacted"
    assert np.array_equal(g5[:, 0, :, :first], p5[:, 0, :, :first]) and np.array_equal(g5[:, 0, :, L - n:], p5[:, 0, :, L - n:])
    moved = g5[:, 0, :, first:L - n] != p5[:, 0, :, first:L - n]
    assert moved.mean() > 0.5, "the kept K rows are rotated"
    # the rotation keeps every pair's norm, to bf16 rounding
    a, b = bf16_to_f64(g5[:, 0, :, first:L - n]), bf16_to_f64(p5[:, 0, :, first:L - n])
    na, nb = np.hypot(a[..., :64], a[..., 64:]), np.hypot(b[..., :64], b[..., 64:])
    assert np.all(np.abs(na - nb) <= 2.0 ** -7 * nb + 1e-30)
    # a zero angle reproduces the plain eviction entirely
    assert np.array_equal(rebase_arena_numpy(arena, nl, hk, lmax, L, first, n, np.ones(64), np.zeros(64)), plain)
    # a cut with no tail has nothing to rotate
    assert np.array_equal(rebase_arena_numpy(arena, nl, hk, lmax, L, 40, 20, cos, sin), evict_arena_numpy(arena, nl, hk, lmax, L, 40, 20))


# ---- 2. HF states the contract -------------------------------------------------------------------------------------------------------
def hf_cut_rebase(stream, first: int, n: int, cfg, direction: int = 1) -> None:
    """Evict rows [first, first + n) from an `oracle.hf_oracle.OracleStream` with positions inside the cache: the rows leave every
    layer of the DynamicCache and `past_ids`, the keys at or above `first` are rotated back by n positions -- HF's
    `k * cos + rotate_half(k) * sin` at angle -n * inv_freq, in fp32, stored back in the cache dtype -- and `rope_deltas` stays.
    `direction=-1` rotates the wrong way (what the tests must be able to tell apart)."""
    d = stream.past_key_values.layers[0].keys.shape[-1]
    inv_freq = 1.0 / (cfg.rope_theta ** (torch.arange(0, d, 2, dtype=torch.float) / d))
    ang = torch.cat([inv_freq, inv_freq]).double() * (-n * direction)
    cos, sin = ang.cos().float(), ang.sin().float()
    for layer in stream.past_key_values.layers:
        keys = torch.cat([layer.keys[:, :, :first], layer.keys[:, :, first + n:]], dim=2)
        k = keys[:, :, first:].float()
        rot = torch.cat([-k[..., d // 2:], k[..., :d // 2]], dim=-1)
        keys[:, :, first:] = (k * cos + rot * sin).to(keys.dtype)
        layer.keys = keys
        layer.values = torch.cat([layer.values[:, :, :first], layer.values[:, :, first + n:]], dim=2)
    stream.past_ids = torch.cat([stream.past_ids[:, :first], stream.past_ids[:, first + n:]], dim=1)


@pytest.fixture(scope="module")
def hf_runs():
    """tiny(), fp32 HF, 4 turns; rows cut before turn 3 (index 2) in several ways.  Returns a function run(kind) -> (outs, info)."""
    from livecc_amd.config import tiny
    from oracle import hf_oracle as O
    cfg = tiny()
    hf = O.build_hf_model(cfg, torch.float32, 3, 2.0)
    frames = torch.from_numpy(protocol.synth_frames(6 + 2 * 3, 56, 84, seed=5, layout="TCHW"))
    chunks = protocol.split_clip(frames.shape[0])
    cache = {}

    def run(kind):
        if kind in cache:
            return cache[kind]
        seen_pos = []
        hook = hf.model.language_model.register_forward_pre_hook(
            lambda mod, args, kwargs: seen_pos.append(kwargs["position_ids"].clone()) if kwargs.get("position_ids") is not None else None,
            with_kwargs=True)
        try:
            b, st = protocol.TurnBuilder(cfg, seed=7), O.OracleStream(hf, cfg)
            spans, outs, info = [], [], {}
            for ti, (a, e) in enumerate(chunks):
                pv, grid = O.patchify_normalize_ref(frames[a:e], cfg)
                ids = b.turn_ids(ti, protocol.num_video_tokens(grid, cfg))
                if ti == 2 and kind != "full":
                    first, n = (0, 37) if kind.startswith("sys") else (spans[1][0], spans[1][1] - spans[1][0])
                    assert spans[0][1] > 37, "rows [0, 37) are inside the first turn's system prompt and query"
                    old_next = st.past_key_values.get_seq_length() + int(st.rope_deltas)
                    delta = int(st.rope_deltas)
                    if kind.endswith("plain"):
                        hf_cut(st, first, n)
                    else:
                        hf_cut_rebase(st, first, n, cfg, direction=-1 if kind.endswith("wrong") else 1)
                        assert int(st.rope_deltas) == delta
                        assert st.past_key_values.get_seq_length() + int(st.rope_deltas) == old_next - n
                    info.update(old_next=old_next, n=n, first=first)
                n_before = 0 if st.past_ids is None else st.past_ids.shape[1]
                del seen_pos[:]
                teacher = cache["full"][0][ti]["new_tokens"] if "full" in cache else None
                outs.append(st.turn(ids, pv, grid, max_new_tokens=3, repetition_penalty=1.05, teacher_tokens=teacher))
                if ti == 2:
                    p = seen_pos[0]
                    info["prefill_start"], info["prefill_len"] = int(p.reshape(-1, p.shape[-1])[0, 0]), (p.shape[-1], len(ids))
                spans.append((n_before, st.past_ids.shape[1]))
        finally:
            hook.remove()
        cache[kind] = (outs, info)
        return cache[kind]
    run("full")
    return run


def _dlogit(x, y, turns):
    worst, scale = 0.0, 0.0
    for ti in turns:
        for a, b in zip(x[ti]["logits"], y[ti]["logits"]):
            worst, scale = max(worst, (a.double() - b.double()).abs().max().item()), max(scale, b.abs().max().item())
    return worst, scale


def test_hf_prefill_starts_n_positions_lower_after_a_rebased_cut(hf_runs):
    for kind in ("sys_rebase", "turn1_rebase"):
        _, info = hf_runs(kind)
        assert info["prefill_start"] == info["old_next"] - info["n"], "HF continues n positions below the old next position"
        assert info["prefill_len"][0] == info["prefill_len"][1]
    _, info = hf_runs("sys_plain")
    assert info["prefill_start"] == info["old_next"], "(the plain cut continues at the old position)"


def test_hf_rebase_is_invisible_when_every_kept_key_moves(hf_runs):
    """Rows [0, 37) cut: every kept key moves down by 37, every relative position is what it was, so the next two turns' logits
    are those of the plain cut -- within 1e-4 x the logit scale in fp32 (measured 6e-7 x); the wrong direction gives ~0.15 x."""
    plain, _ = hf_runs("sys_plain")
    reb, _ = hf_runs("sys_rebase")
    worst, scale = _dlogit(reb, plain, (2, 3))
    print(f"rebase vs plain cut of rows [0, 37): worst |dlogit| {worst:.3g} at logit scale {scale:.3g} ({worst / scale:.2e} x)")
    assert worst <= 1e-4 * scale
    for ti in (0, 1):
        assert all(torch.equal(a, b) for a, b in zip(reb[ti]["logits"], plain[ti]["logits"]))
    wrong, _ = hf_runs("sys_wrong")
    w, s = _dlogit(wrong, plain, (2, 3))
    print(f"wrong direction: {w / s:.3g} x")
    assert w > 1e-2 * s, "a rotation in the wrong direction is visible"


def test_hf_rebase_moves_the_head_closer_when_it_stays(hf_runs):
    plain, _ = hf_runs("turn1_plain")
    reb, _ = hf_runs("turn1_rebase")
    worst, scale = _dlogit(reb, plain, (2, 3))
    print(f"first = start of turn 1: |dlogit| {worst:.3g} at scale {scale:.3g}")
    assert worst > 1e-3 * scale, "the head is n positions closer: the logits differ"


# ---- 3. StreamServer(window_policy="slide_rebase") over the stand-in model -----------------------------------------------------------
class RebaseModel(SlideModel):
    """SlideModel whose KV handles take `rebase=` and carry a `rope_delta` the way StreamState does: += n on a plain eviction,
    unchanged on a rebased one."""

    def __init__(self, cfg, max_kv_len, max_history=3):
        super().__init__(cfg, max_kv_len, max_history)
        self.rebase_flags, self.deltas = [], {}

    def _evict(self, kv, first, n, kept_ids, rebase=False):
        super()._evict(kv, first, n, kept_ids)
        self.rebase_flags.append(bool(rebase))
        if not rebase:
            kv.rope_delta += n

    def generate_batch(self, reqs, **kw):
        outs = super().generate_batch(reqs, **kw)
        for o in outs:
            kv = o.past_key_values
            if not hasattr(kv, "rope_delta"):
                kv.rope_delta = -17                      # what the first turn's video rows leave behind
            self.deltas.setdefault(kv.slot, []).append(kv.rope_delta)
        return outs


def _server(monkeypatch, max_kv_len, **kw):
    def fake_clip(frames, h, w, ts, pts, index_from, layout="THWC"):
        from livecc_amd import resize as R
        idxs, kept = R.select_clip_frames(ts, pts, index_from)
        return (torch.zeros(len(idxs), 3, h, w, dtype=torch.uint8) if idxs else None), kept, idxs
    monkeypatch.setattr(server.R, "get_smart_resized_clip", fake_clip)
    inf = FakeInfer()
    inf.model = RebaseModel(inf.cfg, max_kv_len)
    return server.StreamServer(inf, max_new_tokens=3, **kw)


def _serve(monkeypatch, policy):
    srv = _server(monkeypatch, max_kv_len=160, window_policy=policy)
    srv.add_stream("long", *_video(1800), t_start=0.0, max_pixels=4 * 28 * 28)
    srv.add_stream("short", *_video(150), t_start=0.0, max_pixels=4 * 28 * 28)
    return srv, _by_stream(srv.run(realtime=False))


def test_slide_rebase_policy_rebases_every_eviction_and_keeps_rope_delta(monkeypatch):
    srv, by = _serve(monkeypatch, "slide_rebase")
    m = srv.model
    assert len(m.evicts) >= 3 and m.rebase_flags == [True] * len(m.evicts), "every eviction is made with rebase=True"
    long_slot = m.evicts[0][0]
    assert set(m.deltas[long_slot]) == {-17}, "rope_delta never changes after the first turn"
    slid = [st for _, _, st in by["long"] if st.get("slid")]
    assert len(slid) == len(m.evicts) and all(st.get("rebased") is True and st["evicted_turns"] >= 1 for st in slid)
    assert [st["evictions"] for st in slid] == list(range(1, len(slid) + 1))
    assert not any(st.get("rebased") for _, _, st in by["long"] if not st.get("slid")) and not any(st.get("rebased") for _, _, st in by["short"])
    assert not any(st.get("window_full") or "error" in st or st.get("restarted") for _, _, st in by["long"] + by["short"])
    assert m.checked_after_slide == len(slid) and m.lengths[long_slot] + m.engine.max_history <= 160
    spans = [s for s, _, _ in by["long"]]
    assert spans[0] == (0.0, 3.0) and spans[-1][1] >= 59.0 and all(b - a == 1.0 for a, b in spans[1:]), "every chunk was served"


def test_slide_is_served_exactly_as_before_and_shares_the_plan(monkeypatch):
    srv_r, by_r = _serve(monkeypatch, "slide_rebase")
    srv_s, by_s = _serve(monkeypatch, "slide")
    ms, mr = srv_s.model, srv_r.model
    assert ms.rebase_flags == [False] * len(ms.evicts) and len(ms.evicts) >= 3, "'slide' never rebases"
    assert ms.evicts == mr.evicts, "both policies share the planner and the turn table"
    assert not any("rebased" in st for sid in by_s for _, _, st in by_s[sid])
    d = ms.deltas[ms.evicts[0][0]]
    assert d[-1] == -17 + sum(n for _, _, n in ms.evicts) and sorted(d) == d, "'slide': rope_delta grows by every n"
    for sid in by_s:
        assert [(s, t) for s, t, _ in by_s[sid]] == [(s, t) for s, t, _ in by_r[sid]]
        strip = lambda st: {k: v for k, v in st.items() if k not in ("rebased", "past_key_values", "past_ids")}
        assert [strip(st) for _, _, st in by_s[sid]] == [strip(st) for _, _, st in by_r[sid]]


def test_unknown_window_policies_still_raise():
    for bad in ("ring", "nope", "rebase", "slide-rebase"):
        with pytest.raises(ValueError):
            server.StreamServer(FakeInfer(), window_policy=bad)
    assert server.StreamServer(FakeInfer(), window_policy="slide_rebase").window_policy == "slide_rebase"


def test_live_cc_refuses_unknown_windows_before_touching_the_video():
    from livecc_amd.infer import LiveCCDemoInfer
    inf = LiveCCDemoInfer.__new__(LiveCCDemoInfer)
    for bad in ("ring", "rebase"):
        with pytest.raises(ValueError):
            next(inf.live_cc(None, {"video_path": "x"}, kv_window=bad))
    assert list(inf.live_cc(None, {"video_path": None}, kv_window="slide_rebase")) == []

#!/usr/bin/env python
"""Weight formats of the LLM Linears on MI355X, three formats: bf16, fp8 (e4m3 + row scales), mxfp4 (e2m1 + e8m0 block scales).

(a) GEMV time: microseconds per launch of the four decode GEMVs of pipeline v2 (q|k|v + RoPE + KV append, o_proj + residual, gate/up + SwiGLU,
    down_proj + residual) for ONE stream at LiveCC-7B shapes, and gate/up + down at Qwen2-VL-72B shapes.  Method: a hipEvent pair around a window
    of back-to-back launches (the dispatch of launch i+1 hides under kernel i), each launch on ANOTHER copy of the weight, enough copies that a round
    streams more than 1 GB (cold: the 256-MB last-level cache never holds the weight a launch reads); per-launch time = window / launches; median,
    min and max over the windows after warm-up.  The legs alternate window by window, so they see the same machine.
(b) Decode step: milliseconds per step of a one-stream engine at LiveCC-7B shapes (random weights generated in HBM), a 386-token text prompt and 64
    generated tokens, from the engine's own step events (lcc_engine_profile_read_steps), late steps only.
(c) Chunk prefill: milliseconds of one generate call over a 386-row prompt with one new token (prefill + lm_head + sampler + host; no vision tower),
    event pair around the call, median of the repeats.

(d) Prefill GEMMs: microseconds per call of the four LLM Linears at LiveCC-7B shapes with M = 386 (one streaming chunk) and M = 3088 (eight), in the
    form the engine's prefill calls them (epilogue and split count per weight format), for bf16, mxfp4 on the PACKED4-staging tile kernels ("fused")
    and mxfp4 through the dequantisation scratch ("dequant": lcc_debug_set_w4_fused(0), the only mxfp4 route of a tree without that switch).  Windows
    as in (a): back-to-back calls, another weight copy per call, the three legs alternating window by window in one process.

The bf16 and fp8 legs use only operators that exist without MXFP4 support: run on such a tree the mxfp4 leg reports "unavailable", and those figures
are the baseline.  `--baseline FILE` embeds an earlier output (the parent tree's) and adds the ratios mxfp4 / baseline fp8.  Prints ONE JSON line and
writes it to --out (default profiles/mxfp4/bench_mxfp4.json)."""
import argparse
import gc
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from livecc_amd import ops  # noqa: E402
from livecc_amd.config import livecc_7b  # noqa: E402

HAVE_W4 = hasattr(ops, "linear_w4")
LEGS = ("bf16", "fp8", "mxfp4")
SHAPES_7B = dict(hidden=3584, inter=18944, hq=28, hkv=4)
SHAPES_72B = dict(hidden=8192, inter=29568, hq=64, hkv=8)


def weight_bytes(fmt, N, K):
    return {"bf16": 2 * N * K, "fp8": N * K + 4 * N, "mxfp4": N * K // 2 + N * K // 32}[fmt]


def make_weight(fmt, N, K, dev, seed):
    """Weight bytes of the right size and a legal value range, generated in HBM: the kernels' time does not depend on the values."""
    g = torch.Generator(device=dev).manual_seed(seed)
    if fmt == "bf16":
        return dict(w=(torch.randn(N * K, generator=g, device=dev, dtype=torch.float32) * 0.02).to(torch.bfloat16))
    if fmt == "fp8":
        w = torch.randint(0, 256, (N, K), generator=g, device=dev, dtype=torch.uint8) & 0x77      # never the NaN patterns
        return dict(w=w, wscale=torch.full((N,), 1e-3, device=dev))
    w = torch.randint(0, 256, (N, K // 2), generator=g, device=dev, dtype=torch.uint8)
    return dict(w=w, w4scale=torch.randint(118, 123, (N, K // 32), generator=g, device=dev, dtype=torch.uint8))


def gemv_cases(sh, dev, which):
    """name -> (N, K, launch(weight dict)) for one stream (M = 1)."""
    H, I, hq, hkv = sh["hidden"], sh["inter"], sh["hq"], sh["hkv"]
    nw = torch.ones(H, dtype=torch.bfloat16, device=dev)
    h = (torch.randn(1, H, device=dev) * 2).to(torch.bfloat16)
    stats = ops.tile_stats(h)
    x_i, x_q = torch.randn(1, I, device=dev).to(torch.bfloat16), torch.randn(1, hq * 128, device=dev).to(torch.bfloat16)
    hres = h.clone()
    out = {}

    def kw(w):
        return {k: v for k, v in w.items() if k != "w"}
    if "gate_up" in which:
        out["gate_up"] = (2 * I, H, lambda w: ops.dgemv_norm_linear(w["w"], h, stats, nw, 1e-6, (2 * I, H), swiglu=True, **kw(w)))
    if "down" in which:
        out["down"] = (H, I, lambda w: ops.dgemv_resid_(w["w"], x_i, hres, (H, I), **kw(w)))
    if "o" in which:
        out["o"] = (H, hq * 128, lambda w: ops.dgemv_resid_(w["w"], x_q, hres, (H, hq * 128), **kw(w)))
    if "qkv" in which:
        N = (hq + 2 * hkv) * 128
        kv = ops.KvArena(1, 1, hkv, 256, dev)
        bias = torch.zeros(N, dtype=torch.bfloat16, device=dev)
        slots, kv_len = torch.zeros(1, dtype=torch.int32, device=dev), torch.full((1,), 37, dtype=torch.int32, device=dev)
        inv = (1.0 / (1e6 ** (torch.arange(0, 128, 2, dtype=torch.float) / 128))).to(dev)
        c, s = ops.mrope_table(torch.full((3, 1), 40, dtype=torch.int32, device=dev), inv, [16, 24, 24])
        out["qkv"] = (N, H, lambda w: ops.dgemv_qkv_rope(w["w"], h, stats, nw, 1e-6, bias, c, s, slots, kv_len, kv, 0, hq, **kw(w)))
    return out


def bench_gemvs(sh, dev, which, windows, warmup, legs):
    res = {}
    for name, (N, K, launch) in gemv_cases(sh, dev, which).items():
        copies = {f: [make_weight(f, N, K, dev, 7 * i + 1) for i in range(max(2, -(-(1 << 30) // weight_bytes(f, N, K))))] for f in legs}
        # launches per window: fixed by the shape alone (the copies the SMALLEST format needs), so that a tree without the mxfp4 leg times windows of
        # the same length -- a window's fixed cost (event records, the first dispatch) is shared by its launches
        per = max(2, -(-(1 << 30) // weight_bytes("mxfp4", N, K)))
        times = {f: [] for f in legs}
        for it in range(warmup + windows):
            for f in legs:                                            # alternating legs
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                for i in range(per):
                    launch(copies[f][i % len(copies[f])])
                ev1.record()
                ev1.synchronize()
                if it >= warmup:
                    times[f].append(ev0.elapsed_time(ev1) * 1e3 / per)
        res[name] = dict(N=N, K=K, launches_per_window=per)
        for f in legs:
            t = np.asarray(times[f])
            res[name][f] = dict(us_median=round(float(np.median(t)), 2), us_min=round(float(t.min()), 2), us_max=round(float(t.max()), 2),
                                weight_bytes=weight_bytes(f, N, K), copies=len(copies[f]),
                                TB_per_s=round(weight_bytes(f, N, K) / (float(np.median(t)) * 1e-6) / 1e12, 3))
        del copies
        gc.collect()
        torch.cuda.empty_cache()
    return res


def prefill_gemm_cases(M, sh, max_new_rows=4096):
    """name -> (N, K, {leg format: (epilogue, nsplit)}) as csrc/engine_llm.hip run_layers calls the Linears of an M-row prefill: o / down as split-K
    slabs where gemm_tiled_num_splits says so (packed bf16 weights may get the small variable-height class's count, the quantised formats the
    128-row rule's), else with the residual epilogue; q|k|v as slabs for bf16 weights of a short prefill, with its bias otherwise; gate/up SwiGLU."""
    H, I, hq, hkv = sh["hidden"], sh["inter"], sh["hq"], sh["hkv"]
    qd, qkvd = hq * 128, (hq + 2 * hkv) * 128

    def slab_or(N, K, epi):
        s16, s4 = ops.gemm_plan(M, N, K)[1], ops.gemm_plan(M, N, K, w_fp8=True)[1]
        return {"bf16": (0, s16) if s16 > 1 else (epi, 0), "mxfp4": (0, s4) if s4 > 1 else (epi, 0)}
    qkv16 = ops.gemm_plan(M, qkvd, H)[1] if 6 * min(max_new_rows, 4096) * H >= 8 * M * qkvd else 1
    return {"qkv": (qkvd, H, {"bf16": (0, qkv16) if qkv16 > 1 else (0, 0), "mxfp4": (0, 0)}),
            "o": (H, qd, slab_or(H, qd, ops.EPI_RESIDUAL)),
            "gate_up": (2 * I, H, {"bf16": (ops.EPI_SWIGLU, 0), "mxfp4": (ops.EPI_SWIGLU, 0)}),
            "down": (H, I, slab_or(H, I, ops.EPI_RESIDUAL))}


def bench_prefill_gemms(sh, dev, Ms, windows, warmup):
    have_knob = hasattr(ops, "set_w4_fused")
    legs = ["bf16"] + (["mxfp4_fused", "mxfp4_dequant"] if have_knob else ["mxfp4_dequant"]) if HAVE_W4 else ["bf16"]
    res = {}
    try:
        for M in Ms:
            res[f"M{M}"] = {}
            for name, (N, K, forms) in prefill_gemm_cases(M, sh).items():
                n16 = min(16, max(2, -(-(1 << 30) // weight_bytes("bf16", N, K))))
                n4 = min(16, max(2, -(-(1 << 30) // weight_bytes("mxfp4", N, K))))
                w16 = [make_weight("bf16", N, K, dev, 7 * i + 1)["w"] for i in range(n16)]
                w4 = [make_weight("mxfp4", N, K, dev, 7 * i + 2) for i in range(n4)] if HAVE_W4 else []
                x = torch.randn(M, K, device=dev).to(torch.bfloat16)
                bias, resid = torch.zeros(N, dtype=torch.bfloat16, device=dev), torch.randn(M, N, device=dev).to(torch.bfloat16)
                dq = torch.empty(N * K, dtype=torch.bfloat16, device=dev) if HAVE_W4 else None
                dq_kw = dict(dq_scratch=dq) if have_knob else {}      # (a tree without the switch allocates its scratch per call)

                def call(leg, i):
                    epi, ns = forms["bf16" if leg == "bf16" else "mxfp4"]
                    b, r = (bias if epi == 0 and ns == 0 else None), (resid if epi == ops.EPI_RESIDUAL else None)
                    if leg == "bf16":
                        w = w16[i % n16]
                        return ops.linear_partial(x, w, ns, packed_shape=(N, K)) if ns else ops.linear(x, w, b, epi, r, packed_shape=(N, K))
                    w = w4[i % n4]
                    return ops.linear_w4(x, w["w"], w["w4scale"].view(-1), b, epi, r, nsplit=ns, **dq_kw)
                per, times = n4, {f: [] for f in legs}
                for it in range(warmup + windows):
                    for f in legs:                                        # alternating legs
                        if have_knob and f != "bf16":
                            ops.set_w4_fused(f == "mxfp4_fused")
                        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        ev0.record()
                        for i in range(per):
                            call(f, i)
                        ev1.record()
                        ev1.synchronize()
                        if it >= warmup:
                            times[f].append(ev0.elapsed_time(ev1) * 1e3 / per)
                d = dict(N=N, K=K, calls_per_window=per, form={k: dict(epilogue=e, nsplit=s) for k, (e, s) in forms.items()},
                         tile_rows=dict(bf16=ops.gemm_plan(M, N, K, forms["bf16"][0], forms["bf16"][1])[0]))
                if have_knob:
                    ops.set_w4_fused(True)
                    d["tile_rows"]["mxfp4"], d["mxfp4_fused_by_default"] = ops.gemm_w4_plan(M, N, K, forms["mxfp4"][0], forms["mxfp4"][1])
                for f in legs:
                    t = np.asarray(times[f])
                    d[f] = dict(us_median=round(float(np.median(t)), 2), us_min=round(float(t.min()), 2), us_max=round(float(t.max()), 2))
                res[f"M{M}"][name] = d
                del w16, w4, dq
                gc.collect()
                torch.cuda.empty_cache()
            res[f"M{M}"]["sum_us_median"] = {f: round(sum(v[f]["us_median"] for k, v in res[f"M{M}"].items() if isinstance(v, dict) and f in v), 2) for f in legs}
    finally:
        if have_knob:
            ops.set_w4_fused(True)
    return res


def bench_engine(fmt, dev, steps, prefill_reps):
    from livecc_amd.modeling import LiveCCForConditionalGeneration
    cfg = livecc_7b()
    kw = dict(max_streams=1, max_kv_len=2048, max_new_rows=1024, max_patches=1024, max_history=steps)
    if fmt == "bf16":
        m = LiveCCForConditionalGeneration.from_config(cfg, dev, seed=0, **kw)
    elif fmt == "fp8":
        m = LiveCCForConditionalGeneration.from_config(cfg, dev, seed=0, llm_fp8=True, **kw)
    else:
        m = LiveCCForConditionalGeneration.from_config(cfg, dev, seed=0, llm_weights="mxfp4", **kw)
    ids = torch.from_numpy(np.random.RandomState(1).randint(1000, 100000, 386).astype(np.int64)).view(1, -1)
    out = dict(arena_GB=round(m.weights.nbytes() / 1e9, 3))
    ts = []
    for it in range(prefill_reps + 1):                                # (c) one 386-row prefill call; the first call is warm-up
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        r = m.generate(input_ids=ids, max_new_tokens=1, min_new_tokens=1)
        ev1.record()
        ev1.synchronize()
        r.past_key_values.release()
        if it:
            ts.append(ev0.elapsed_time(ev1))
    out["prefill_386_call_ms"] = dict(median=round(float(np.median(ts)), 3), min=round(min(ts), 3), max=round(max(ts), 3), calls=len(ts))
    r = m.generate(input_ids=ids, max_new_tokens=steps, min_new_tokens=steps)      # warm-up of the decode path
    r.past_key_values.release()
    m.engine.profile(True)
    r = m.generate(input_ids=ids, max_new_tokens=steps, min_new_tokens=steps)      # (b)
    torch.cuda.synchronize(dev)
    st = np.asarray(m.engine.profile_read_steps(), dtype=np.float64)
    m.engine.profile(False)
    r.past_key_values.release()
    late = st[len(st) // 2:] if len(st) >= 4 else st
    out["decode_step_ms"] = dict(median=round(float(np.median(late)), 4), min=round(float(late.min()), 4), max=round(float(late.max()), 4),
                                 sampled_steps=int(len(late)))
    del m, r
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--prefill-reps", type=int, default=5)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--skip-72b", action="store_true")
    ap.add_argument("--skip-gemv", action="store_true")
    ap.add_argument("--skip-prefill-gemms", action="store_true")
    ap.add_argument("--baseline", default=None, help="an earlier output of this tool (the parent tree's run) to embed and compare against")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mxfp4", "bench_mxfp4.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mxfp4 needs the MI355X: no GPU, no number")
    dev = torch.device("cuda:0")
    legs = [f for f in LEGS if f != "mxfp4" or HAVE_W4]
    res = dict(tool="bench_mxfp4", mxfp4="available" if HAVE_W4 else "unavailable", windows=a.windows, warmup_windows=a.warmup,
               method="event pair around a window of back-to-back launches, one weight copy per launch (> 1 GB per round: cold), per-launch = window / launches")
    if not a.skip_gemv:
        res["gemv_7b_us"] = bench_gemvs(SHAPES_7B, dev, ("qkv", "o", "gate_up", "down"), a.windows, a.warmup, legs)
    if not a.skip_prefill_gemms:
        res["prefill_gemm_7b_us"] = bench_prefill_gemms(SHAPES_7B, dev, (386, 3088), a.windows, a.warmup)
    if not a.skip_72b and not a.skip_gemv:
        res["gemv_72b_us"] = bench_gemvs(SHAPES_72B, dev, ("gate_up", "down"), a.windows, a.warmup, legs)
    if not a.skip_engine:
        res["engine_7b"] = {f: bench_engine(f, dev, a.steps, a.prefill_reps) for f in legs}
    if a.baseline:
        with open(a.baseline) as f:
            base = json.loads(f.readline())
        res["parent"] = base
        if HAVE_W4:
            ratios = {}
            for grp in ("gemv_7b_us", "gemv_72b_us"):
                for name, d in res.get(grp, {}).items():
                    b = base.get(grp, {}).get(name, {}).get("fp8")
                    if b:
                        ratios[f"{grp}.{name}"] = round(d["mxfp4"]["us_median"] / b["us_median"], 3)
            res["mxfp4_over_parent_fp8"] = ratios
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""A/B of the decode seam attention -> split merge -> o_proj at operator level: the three launches (lcc_attn_decode_bf16 + lcc_dgemv_resid)
against the fused launch (lcc_dgemv_attn_o, csrc/decode_v2.hip: attn_o_kernel), at shapes where the fused launch is eligible.

One pass = `layers` decoder layers' worth of the seam, every layer with its own KV rows and its own o_proj weight (so K / V and weights
come from HBM as in a decode step, not from a cache warmed by the previous iteration).  A pass of each route is captured as a graph and
replayed; the time per layer is (events around `reps` replays) / (reps * layers): it contains the gaps between the kernels of a pass, which
a kernel trace does not show.  Rounds alternate three / fused.  Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats -- python
tools/bench_attn_o.py ...` the same run gives the per-kernel times (attn_decode_kernel, attn_decode_combine_kernel, dgemv_kernel vs
attn_o_kernel).  LCC_ATTN_O_DELAY_US in the environment sets the o_proj blocks' silent wait before their first poll.

    python tools/bench_attn_o.py --shape 7b --keys 1000 [--streams 1] [--layers 28] [--reps 20] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = {"7b": (28, 4, 3584), "2b": (12, 2, 1536), "small": (7, 1, 896)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="7b")
    ap.add_argument("--keys", type=int, default=1000)
    ap.add_argument("--streams", type=int, default=1)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    from livecc_amd import ops
    dev = torch.device("cuda:0")
    Hq, Hkv, H = SHAPES[a.shape]
    M, K, L = a.streams, Hq * 128, a.layers
    n = a.keys
    nsplit = max(1, min(64, ((n + 31) // 32 + 3) // 4))
    lmax = (n + 31) // 32 * 32
    g = torch.Generator(device=dev).manual_seed(1)
    kv = ops.KvArena(M, L, Hkv, lmax, dev)
    kv.buf.copy_((torch.randn(kv.buf.shape, generator=g, device=dev) * 0.5).to(torch.bfloat16))
    w = [ops.pack_weight((torch.randn(H, K, generator=g, device=dev) * 0.03).to(torch.bfloat16)) for _ in range(L)]
    q = (torch.randn(M, K, generator=g, device=dev)).to(torch.bfloat16)
    h0 = (torch.randn(M, H, generator=g, device=dev) * 2).to(torch.bfloat16)
    slots = torch.arange(M, dtype=torch.int32, device=dev)
    kv_len = torch.full((M,), n - 1, dtype=torch.int32, device=dev)          # the new token is key n - 1
    tickets = torch.zeros(256, dtype=torch.int32, device=dev)
    counter, err = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    h = {"three": h0.clone(), "fused": h0.clone()}

    def three():
        for l in range(L):
            attn = ops.attn_decode(q, kv, l, slots, kv_len, Hq, nsplit)
            ops.dgemv_resid_(w[l], attn, h["three"], (H, K))

    def fused():
        counter.zero_()                      # the hand-off targets below are baked into the captured launches: every replay starts from 0
        for l in range(L):
            ops.dgemv_attn_o_(q, kv, l, slots, kv_len, Hq, nsplit, w[l], h["fused"], tickets, counter, l * M * Hkv, err)

    routes = {"three": three, "fused": fused}
    graphs = {}
    for name, fn in routes.items():
        h[name].copy_(h0)
        fn()                                  # eager pass: first-use setup outside the capture; also the parity check below
        torch.cuda.synchronize()
    same = bool(torch.equal(h["three"], h["fused"]))
    for name, fn in routes.items():
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            fn()
        graphs[name] = gr
    times = {k: [] for k in routes}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name in routes:
        graphs[name].replay()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name in ("three", "fused"):
            ev0.record()
            for _ in range(a.reps):
                graphs[name].replay()
            ev1.record()
            torch.cuda.synchronize()
            times[name].append(round(ev0.elapsed_time(ev1) * 1e3 / (a.reps * L), 3))
    out = dict(shape=a.shape, heads=[Hq, Hkv], hidden=H, streams=M, keys=n, nsplit=nsplit, layers=L, reps=a.reps,
               blocks=dict(attention=M * Hkv * nsplit, o_proj=H // 16), delay_us=os.environ.get("LCC_ATTN_O_DELAY_US", "default(6)"),
               bit_identical=same, err_word=int(err[0]), us_per_layer={k: v for k, v in times.items()},
               median_us_per_layer={k: statistics.median(v) for k, v in times.items()})
    out["fused_minus_three_us"] = round(out["median_us_per_layer"]["fused"] - out["median_us_per_layer"]["three"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What a KV fork costs and what it saves on MI355X, at the LiveCC-7B shapes (28 layers x 4 KV heads, 57,344 B per cached row).

`--what copy` (profiles/kv_fork/copy.jsonl): `lcc_kv_copy_bf16` (csrc/kv_copy.hip) between two 32,768-row arenas for n in {1k, 6.5k,
24k, 32k} rows, in both store forms (plain / non-temporal, `lcc_debug_set_kv_copy_nt`), against the yardstick measured in the same
run: a plain `torch` device-to-device `copy_` of the same number of bytes (the runtime's own copy, not the code under test).  Method:
a device event pair around every call on the launch stream, the three alternating call by call, warm-up first, the MEDIAN of --iters
calls.  `bytes_per_s` is bytes read + written (2 x n x 57,344) over that time.  A 1k-row copy (59 MB) fits the 256-MiB Infinity Cache,
so its repeated calls run cache-warm; the larger ones do not fit.

`--what mcq` (profiles/kv_fork/mcq.jsonl): `LiveCCDemoInfer.mcq_predict_many` with three questions against three `mcq_predict`
calls (the one-question path, one vision tower + one full prefill each) in the same process, on a 60-frame 392x728 clip and a
480-frame 280x280 clip, synthetic weights, a byte-level tokenizer built on the fly (no tokenizer files exist offline).  Host clock
around work that ends in a device synchronise, the two alternating, warm-up first, median of --reps.

One JSON line per measurement; needs the GPU (no GPU, no number)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from livecc_amd import _lib  # noqa: E402
from livecc_amd.config import livecc_7b  # noqa: E402

PEAK_BPS = 8.0e12
ROWS = (1024, 6656, 24576, 32768)
QUESTIONS = [("what is happening now?", ["A. system", "B. user", "C. assistant", "D. video"]),
             ("now?", ["A. 0", "B. 1", "C. 2", "D. 3"]),
             ("Please describe the video. what is happening now? ...", ["A. a helpful assistant", "B. livecc", "C. =-.", "D. 0123456789"])]


def bench_copy(a, dev, out_path):
    lib = _lib.load()
    c = livecc_7b()
    lmax = 32768
    kl = _lib.KvLayout(c.num_hidden_layers, c.num_key_value_heads, lmax, 128)
    row_bytes = c.num_hidden_layers * 2 * c.num_key_value_heads * 128 * 2
    total = row_bytes * lmax
    src = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev)
    dst = torch.zeros(total, dtype=torch.uint8, device=dev)
    ysrc, ydst = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev), torch.zeros(total, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    default_nt = lib.lcc_debug_set_kv_copy_nt(0)
    lines = []
    for n in ROWS:
        nbytes = n * row_bytes

        def kernel():
            _lib.check(lib.lcc_kv_copy_bf16(dst.data_ptr(), src.data_ptr(), kl, n, st), "lcc_kv_copy_bf16")
        calls = {"kernel_plain": kernel, "kernel_nt": kernel, "torch_copy": lambda: ydst[:nbytes].copy_(ysrc[:nbytes])}
        times = {k: [] for k in calls}
        for it in range(a.warmup + a.iters):
            for k, fn in calls.items():
                lib.lcc_debug_set_kv_copy_nt(int(k == "kernel_nt"))      # outside the timed span
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    times[k].append(e0.elapsed_time(e1) * 1e3)
        us = {k: statistics.median(v) for k, v in times.items()}
        line = dict(what="kv_copy", layout="7b (28 layers x 4 KV heads)", lmax=lmax, n_rows=n, bytes_copied=nbytes, iters=a.iters,
                    default_store="nt" if default_nt else "plain",
                    kernel_plain_us=round(us["kernel_plain"], 2), kernel_nt_us=round(us["kernel_nt"], 2), torch_copy_us=round(us["torch_copy"], 2),
                    kernel_plain_bytes_per_s=2 * nbytes / (us["kernel_plain"] * 1e-6), kernel_nt_bytes_per_s=2 * nbytes / (us["kernel_nt"] * 1e-6),
                    torch_copy_bytes_per_s=2 * nbytes / (us["torch_copy"] * 1e-6),
                    kernel_plain_min_max_us=[round(min(times["kernel_plain"]), 2), round(max(times["kernel_plain"]), 2)],
                    kernel_nt_min_max_us=[round(min(times["kernel_nt"]), 2), round(max(times["kernel_nt"]), 2)],
                    torch_copy_min_max_us=[round(min(times["torch_copy"]), 2), round(max(times["torch_copy"]), 2)],
                    hbm_peak_bytes_per_s=PEAK_BPS)
        lines.append(line)
        print(json.dumps(line), flush=True)
    lib.lcc_debug_set_kv_copy_nt(default_nt)
    _write(out_path, lines)


def bench_mcq(a, dev, out_path):
    import dataclasses
    from livecc_amd import protocol
    from livecc_amd.infer import LiveCCDemoInfer
    from livecc_amd.modeling import LiveCCForConditionalGeneration
    from livecc_amd.text import TextFrontEnd
    from livecc_amd.weights import WeightArena
    from tests.test_text import make_tokenizer_dir       # the byte-level tokenizer the text tests build (none ships offline)
    with tempfile.TemporaryDirectory() as td:
        tk = TextFrontEnd(make_tokenizer_dir(td)).tokenizer
    ids = {k: tk.convert_tokens_to_ids(v) for k, v in (("video_token_id", "<|video_pad|>"), ("eos_token_id", "<|im_end|>"),
                                                        ("image_token_id", "<|image_pad|>"), ("vision_start_token_id", "<|vision_start|>"),
                                                        ("vision_end_token_id", "<|vision_end|>"), ("bos_token_id", "<|endoftext|>"))}
    cfg = dataclasses.replace(livecc_7b(), **ids)
    arena = WeightArena(cfg, dev).fill_random(0)
    lines = []
    for name, (T, H, W) in (("configs[1] clip: 60 frames 392x728", (60, 392, 728)), ("configs[3] clip: 480 frames 280x280", (480, 280, 280))):
        grid = protocol.grid_of(T, H, W, cfg)
        rows = protocol.num_video_tokens(grid, cfg) + 512
        model = LiveCCForConditionalGeneration(cfg, arena, dev, max_streams=4, max_kv_len=(rows + 31) // 32 * 32 + 64, max_new_rows=4096,
                                               max_patches=16384, max_history=16)
        infer = LiveCCDemoInfer(model=model, text=TextFrontEnd(tk, cfg))
        clip = torch.from_numpy(protocol.synth_frames(T, H, W, seed=1234, layout="TCHW")).to(dev)

        def three_single():
            return [infer.mcq_predict(clip, q, o) for q, o in QUESTIONS]

        def many():
            return infer.mcq_predict_many(clip, QUESTIONS)
        calls = {"three_mcq_predict": three_single, "mcq_predict_many": many}
        times = {k: [] for k in calls}
        res = {}
        for it in range(1 + a.reps):
            for k, fn in calls.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                res[k] = fn()
                torch.cuda.synchronize(dev)
                if it >= 1:
                    times[k].append(time.perf_counter() - t0)
        s = {k: statistics.median(v) for k, v in times.items()}
        worst = max((x[1] - y[1]).abs().max().item() for x, y in zip(res["three_mcq_predict"], res["mcq_predict_many"]))
        line = dict(what="mcq three questions", clip=name, visual_rows=int(protocol.num_video_tokens(grid, cfg)), questions=len(QUESTIONS), reps=a.reps,
                    three_mcq_predict_s=round(s["three_mcq_predict"], 4), mcq_predict_many_s=round(s["mcq_predict_many"], 4),
                    ratio=round(s["three_mcq_predict"] / s["mcq_predict_many"], 3),
                    three_mcq_predict_min_max_s=[round(min(times["three_mcq_predict"]), 4), round(max(times["three_mcq_predict"]), 4)],
                    mcq_predict_many_min_max_s=[round(min(times["mcq_predict_many"]), 4), round(max(times["mcq_predict_many"]), 4)],
                    same_choices=[x[0] for x in res["three_mcq_predict"]] == [y[0] for y in res["mcq_predict_many"]],
                    worst_abs_logit_difference=worst, weights="synthetic (seed 0)")
        lines.append(line)
        print(json.dumps(line), flush=True)
        del infer, model
        torch.cuda.empty_cache()
    _write(out_path, lines)


def _write(path, lines):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["copy", "mcq", "both"], default="both")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "kv_fork"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kv_fork needs the MI355X: no GPU, no number")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if a.what in ("copy", "both"):
        bench_copy(a, dev, os.path.join(a.out_dir, "copy.jsonl"))
    if a.what in ("mcq", "both"):
        bench_mcq(a, dev, os.path.join(a.out_dir, "mcq.jsonl"))


if __name__ == "__main__":
    main()

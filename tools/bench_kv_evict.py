#!/usr/bin/env python
"""Cost of one sliding-window eviction on MI355X at the LiveCC-7B KV layout (28 layers x 4 KV heads, 32768 rows, 57,344 B per row):
`lcc_slot_evict` (the compaction kernel of csrc/kv_evict.hip + the seen-id bitmap rebuild) with kv_len = 32768, dropping the oldest
half after a 450-row head (n % 32 != 0, the general column rotation of the blocked-transposed V planes).

Method: a hipEvent pair around every call on the launch stream, >= 20 timed calls after warm-up, the arena re-filled and the slot
length restored between calls OUTSIDE the timed region.  Yardstick measured in the same run, alternating with the calls under test:
one `hipMemcpyAsync` device-to-device of the same payload (the bytes of the rows that move).  Rates are payload / time; traffic is
read + write of the payload (+ the zero fill), quoted as a fraction of the 8 TB/s HBM peak.  The operator-level entry
(`lcc_kv_evict_bf16`, kernel launches only) is timed the same way, so the difference to `lcc_slot_evict` is the bitmap rebuild and
the id upload.  --rebase: the same alternating loop also times the re-rotating forms (`lcc_kv_evict_rebase_bf16` with a fixed table,
`lcc_slot_evict_rebase`: the same bytes moved, the K rows rotated on their way through registers) and the default --out becomes
bench_kv_evict_rebase.json; their yardstick is kernel_only / slot_evict of the same run.  Prints ONE JSON line and writes it to --out (default profiles/kv_evict/bench_kv_evict.json).  Needs no weights: the
engine is created bare through the C-ABI."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from livecc_amd import _lib  # noqa: E402
from livecc_amd.config import livecc_7b  # noqa: E402

PEAK_BPS = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--kv-len", type=int, default=32768)
    ap.add_argument("--head", type=int, default=450)
    ap.add_argument("--rebase", action="store_true", help="also time lcc_kv_evict_rebase_bf16 and lcc_slot_evict_rebase")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kv_evict",
                             "bench_kv_evict_rebase.json" if a.rebase else "bench_kv_evict.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_kv_evict needs the MI355X: no GPU, no number")
    lib, dev = _lib.load(), torch.device("cuda:0")
    hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    c = livecc_7b()
    lmax = (a.kv_len + 31) // 32 * 32
    mc = _lib.ModelConfig(c.vocab_size, c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads,
                          c.num_key_value_heads, 128, 1e-6, 16, 24, 24, c.vit_depth, c.vit_embed_dim, c.vit_num_heads, c.vit_mlp_dim, 1176, 2, 0)
    lim = _lib.EngineLimits(1, lmax, 4096, 16384, 32)
    e = lib.lcc_engine_create(C.byref(mc), C.byref(lim))
    assert e, lib.lcc_last_error()
    ws = torch.empty(lib.lcc_engine_workspace_bytes(e), dtype=torch.uint8, device=dev)
    state = torch.zeros(lib.lcc_engine_state_bytes(e), dtype=torch.uint8, device=dev)
    mb = lib.lcc_engine_meta_bytes(e)
    meta_d, meta_h = torch.empty(mb, dtype=torch.uint8, device=dev), torch.empty(mb, dtype=torch.uint8).pin_memory()
    _lib.check(lib.lcc_engine_bind_buffers(e, ws.data_ptr(), ws.numel(), state.data_ptr(), state.numel(), meta_d.data_ptr(), meta_h.data_ptr(), mb))
    kvb = lib.lcc_engine_kv_bytes_per_slot(e)
    kv = torch.zeros(kvb, dtype=torch.uint8, device=dev)
    _lib.check(lib.lcc_engine_bind_kv(e, 0, kv.data_ptr(), kvb))
    fill = torch.randint(0, 256, (kvb,), dtype=torch.uint8, device=dev)
    L, first = a.kv_len, a.head
    n = (L - first) // 2
    n += 1 if n % 32 == 0 else 0
    row_bytes = kvb // lmax
    payload = (L - first - n) * row_bytes
    zero_bytes = n * row_bytes
    kept = np.random.RandomState(0).randint(0, c.vocab_size, L - n).astype(np.int32)
    kl = _lib.KvLayout(c.num_hidden_layers, c.num_key_value_heads, lmax, 128)
    src, dst = torch.empty(payload, dtype=torch.uint8, device=dev), torch.empty(payload, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def slot_evict():
        _lib.check(lib.lcc_slot_evict(e, 0, first, n, kept.ctypes.data, len(kept), st), "lcc_slot_evict")

    def kernel_only():
        _lib.check(lib.lcc_kv_evict_bf16(kv.data_ptr(), kl, L, first, n, None, 0, st), "lcc_kv_evict_bf16")

    def memcpy():
        assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), payload, 3, st) == 0       # 3 = hipMemcpyDeviceToDevice

    variants = [("slot_evict", slot_evict), ("kernel_only", kernel_only), ("memcpy", memcpy)]
    if a.rebase:
        inv_freq = (1.0 / (c.rope_theta ** (torch.arange(0, 128, 2, dtype=torch.float) / 128))).to(dev)
        _lib.check(lib.lcc_engine_set_weight(e, b"inv_freq", inv_freq.data_ptr(), inv_freq.numel()), "inv_freq")
        ang = n * inv_freq.double().cpu().numpy()
        rot = torch.from_numpy(np.concatenate([np.cos(ang), np.sin(ang)]).astype(np.float32)).to(dev)     # a fixed table: the shift by n

        def slot_evict_rebase():
            _lib.check(lib.lcc_slot_evict_rebase(e, 0, first, n, kept.ctypes.data, len(kept), st), "lcc_slot_evict_rebase")

        def kernel_only_rebase():
            _lib.check(lib.lcc_kv_evict_rebase_bf16(kv.data_ptr(), kl, L, first, n, rot.data_ptr(), st), "lcc_kv_evict_rebase_bf16")
        variants += [("slot_evict_rebase", slot_evict_rebase), ("kernel_only_rebase", kernel_only_rebase)]
    times = {name: [] for name, _ in variants}
    for it in range(a.warmup + a.iters):
        for name, fn in variants:                                                                       # alternating, same conditions
            kv.copy_(fill)                                                                          # un-timed: arena as before an eviction
            _lib.check(lib.lcc_slot_set_length(e, 0, L, L, st), "lcc_slot_set_length")
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            fn()
            ev1.record()
            ev1.synchronize()
            if it >= a.warmup:
                times[name].append(ev0.elapsed_time(ev1))
    res = dict(tool="bench_kv_evict", layout="livecc-7b: 28 layers x 4 KV heads x 128, bf16", lmax=lmax, kv_len=L, first=first, n=n, n_mod_32=n % 32,
               rows_moved=L - first - n, payload_bytes=payload, zero_fill_bytes=zero_bytes, timed_calls=a.iters, warmup_calls=a.warmup,
               hbm_peak_bytes_per_s=PEAK_BPS)
    for name, ts in times.items():
        ts = np.asarray(ts)
        med = float(np.median(ts))
        traffic = 2 * payload + (zero_bytes if name != "memcpy" else 0)
        res[name] = dict(ms_median=round(med, 4), ms_min=round(float(ts.min()), 4), ms_max=round(float(ts.max()), 4),
                         payload_TB_per_s=round(payload / (med * 1e-3) / 1e12, 3),
                         traffic_fraction_of_peak=round(traffic / (med * 1e-3) / PEAK_BPS, 3))
    res["kernel_vs_memcpy_time"] = round(res["kernel_only"]["ms_median"] / res["memcpy"]["ms_median"], 3)
    res["slot_evict_vs_memcpy_time"] = round(res["slot_evict"]["ms_median"] / res["memcpy"]["ms_median"], 3)
    if a.rebase:      # the plain forms of the same run are the yardstick; their own min-to-max spread says what a difference means
        for reb, plain in (("kernel_only_rebase", "kernel_only"), ("slot_evict_rebase", "slot_evict")):
            res[f"{reb}_minus_{plain}_ms_median"] = round(res[reb]["ms_median"] - res[plain]["ms_median"], 4)
            res[f"{plain}_spread_ms"] = round(res[plain]["ms_max"] - res[plain]["ms_min"], 4)
    lib.lcc_engine_destroy(e)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

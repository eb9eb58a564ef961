#!/usr/bin/env python3
"""Modulus switching (csrc/modswitch.hip) on resident data, in one process, alternating with fhe_add on the same batch.
(a) Kernel.  4096 size-2 ciphertexts per case: the P8192 primes 4 -> 3, 2, 1; the P4096 primes 3 -> 2; the eight SEAL23_16384 primes at
n = 16384, 8 -> 4 and 8 -> 1.  Reported per case: the time, (bytes in + bytes out) / time as a share of the 8 TB/s HBM roofline (DESIGN.md
section 5), the same for fhe_add on the same batch (two operands in, one out: the yardstick of a streaming kernel here), their ratio, and
the Shoup products per byte moved.  No target: the deep drops may be instruction-bound, the ratio is recorded with its reason.
(b) End to end.  server_resize_plain `src` x `src` -> `dst` x `dst`, three channels, at the P8192 preset over files in a tmpfs, with and
without out_primes in the same run (second pass of each; the first locks and allocates pages): output bytes and wall seconds.
Device events, two warm-up runs, three alternating rounds per variant of at least `window_s` each, the spread reported.  One JSON line per
case to stdout and to profiles/modswitch_bench.json.  Secondary measurement, not bench.py's.
Usage: bench_modswitch.py [window_s=0.5] [out=profiles/modswitch_bench.json] [count=4096] [src=128] [dst=64] [out_primes=2] [dir=/dev/shm]"""
import json, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fhip_amd as fhe

arg = lambda i, d: sys.argv[i] if len(sys.argv) > i else d
window_s, out_path, COUNT = float(arg(1, "0.5")), arg(2, os.path.join(ROOT, "profiles", "modswitch_bench.json")), int(arg(3, "4096"))
SRC, DST, OUT_PRIMES, DIR = int(arg(4, "128")), int(arg(5, "64")), int(arg(6, "2")), arg(7, "/dev/shm")
ROUNDS = 3
HBM_PEAK = 8e12
CASES = [("P8192", (3, 2, 1)), ("P4096", (2,)), ("SEAL23_16384", (4, 1))]


def window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def steps_for(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    return max(1, int(window_s * 1e3 / window(fn, 1)) + 1)


def measure(fns):
    steps = {name: steps_for(fn) for name, fn in fns.items()}
    rounds = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            rounds[name].append(window(fn, steps[name]))
    ms = {name: statistics.median(r) for name, r in rounds.items()}
    return steps, rounds, ms, {name: (max(r) - min(r)) / ms[name] for name, r in rounds.items()}


lines = []
for preset, outs in CASES:
    ctx = fhe.SEALContext.preset(preset)
    ev = fhe.Evaluator(ctx)
    k, n = ctx.k, ctx.n
    ct = ctx.random_ct(COUNT, seed=fhe.SEED)
    other = ctx.random_ct(COUNT, seed=fhe.SEED + 1)
    total = ctx.empty(COUNT)
    bufs = {k_out: ctx.level(k_out).empty(COUNT) for k_out in outs}
    fns = {"add": lambda: ev.add(ct, other, out=total)}
    for k_out in outs:
        fns["%d->%d" % (k, k_out)] = lambda k_out=k_out: ev.mod_switch(ct, k_out, out=bufs[k_out])
    steps, rounds, ms, spread = measure(fns)
    word_bytes = COUNT * 2 * n * 8
    add_share = 3 * k * word_bytes / ms["add"] * 1e3 / HBM_PEAK
    for k_out in outs:
        name = "%d->%d" % (k, k_out)
        moved = (k + k_out) * word_bytes
        share = moved / ms[name] * 1e3 / HBM_PEAK
        products = sum(range(k_out, k))                               # one per (drop, kept prime) and coefficient
        line = {"workload": "mod_switch %s on %d size-2 ciphertexts, %s primes (n=%d k=%d)" % (name, COUNT, preset, n, k), "lazy_products": max(q.bit_length() for q in ctx.q) <= 58,
                "rounds": ROUNDS, "steps": {x: steps[x] for x in (name, "add")}, "ms": ms[name], "ms_rounds": rounds[name], "spread": spread[name], "bytes_in_plus_out": moved,
                "share_of_hbm_roofline": share, "add_ms": ms["add"], "add_ms_rounds": rounds["add"], "add_bytes": 3 * k * word_bytes, "add_share_of_hbm_roofline": add_share,
                "ratio_to_add_share": share / add_share, "shoup_products_per_coefficient": products, "bytes_per_coefficient": (k + k_out) * 8,
                "ciphertext_bytes_in": 2 * k * n * 8, "ciphertext_bytes_out": 2 * k_out * n * 8}
        print(json.dumps(line), flush=True)
        lines.append(line)
    del ct, other, total, bufs, fns
    torch.cuda.empty_cache()

# (b) server_resize_plain with and without out_primes, same process, same input file
ctx = fhe.SEALContext.preset("P8192")
fin, fout = os.path.join(DIR, "fhe_ms_in.ct"), os.path.join(DIR, "fhe_ms_out.ct")
rec = fhe.server.RECORD_HEADER + 2 * ctx.k * ctx.n * 8
try:
    row = torch.empty((SRC, 3, 2, ctx.k, ctx.n), dtype=torch.int64).pin_memory()
    sin = fhe.server.StreamFile(fin, write=True, size=SRC * SRC * 3 * rec)
    for r in range(SRC):
        row.copy_(ctx.random_ct(SRC, 3, size=2, seed=fhe.SEED, first_index=r * SRC * 3 * 2 * ctx.k * ctx.n))
        sin.transfer(r * SRC * 3, SRC * 3, 2, ctx, row, 8)
    sin.close()
    result = {}
    for out_primes in (None, OUT_PRIMES):
        k_out = ctx.k if out_primes is None else out_primes
        sin = fhe.server.StreamFile(fin)
        sout = fhe.server.StreamFile(fout, write=True, size=DST * DST * 3 * (fhe.server.RECORD_HEADER + 2 * k_out * ctx.n * 8))
        seconds = []
        for _ in range(2):                                             # the first pass locks and allocates pages
            stats = {}
            t0 = time.time()
            fhe.server.server_resize_plain(ctx, sin, sout, SRC, SRC, DST, DST, "catmull_rom", rows_per_step=4, io_threads=16, stats=stats, out_primes=out_primes)
            torch.cuda.synchronize()
            seconds.append(time.time() - t0)
        sin.close()
        sout.close()
        os.remove(fout)
        result["k_out=%d" % k_out] = {"out_primes": out_primes, "bytes_out": stats["bytes_out"], "seconds": seconds[1], "first_pass_seconds": seconds[0],
                                      "file_read_seconds": stats["file_read_seconds"], "file_write_seconds": stats["file_write_seconds"]}
    a, b = result["k_out=%d" % ctx.k], result["k_out=%d" % OUT_PRIMES]
    line = {"workload": "server_resize_plain %dx%d -> %dx%d catmull_rom, three channels, P8192, files in %s" % (SRC, SRC, DST, DST, DIR), "bytes_in": SRC * SRC * 3 * rec,
            "runs": result, "bytes_out_ratio": b["bytes_out"] / a["bytes_out"], "seconds_ratio": b["seconds"] / a["seconds"]}
    print(json.dumps(line), flush=True)
    lines.append(line)
finally:
    for p in (fin, fout):
        if os.path.exists(p):
            os.remove(p)

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    for line in lines:
        fh.write(json.dumps(line) + "\n")

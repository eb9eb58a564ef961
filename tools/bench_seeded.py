#!/usr/bin/env python3
"""Seeded symmetric encryption (csrc/encrypt.hip k_seed_expand / k_enc_sym_fused), in one process.
(a) fhe_expand_seeded on resident data at the P4096 and P8192 primes, 256 and 4,096 ciphertexts: microseconds per ciphertext and
    (bytes read + bytes written) / time as a share of the 8 TB/s HBM roofline -- the kernel is expected to be
    bound by instruction issue (a ChaCha20 block per 32 bytes written), not by memory; the share says how far below the roofline that is.
(b) fhe_encrypt_symmetric_batch beside fhe_encrypt_batch on the same plaintext batch, alternating.
(c) server_jpeg end to end over `blocks` colour blocks in a tmpfs: the same c0 records read as a seeded stream and, expanded and stored as
    full records, as an ordinary one; alternating passes after one warm-up pass each (the first locks and allocates pages): bytes_in,
    wall seconds and device compute seconds of each.
Device events, two warm-up runs, three alternating rounds per variant of at least `window_s` each, the spread reported.  One JSON line per
case to stdout and to the output file.  Secondary measurement, not bench.py's.
Usage: bench_seeded.py [window_s=0.5] [out=profiles/seeded_bench.json] [blocks_p4096=32] [blocks_p8192=12] [dir=/dev/shm]"""
import json, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fhip_amd as fhe

arg = lambda i, d: sys.argv[i] if len(sys.argv) > i else d
window_s, out_path = float(arg(1, "0.5")), arg(2, os.path.join(ROOT, "profiles", "seeded_bench.json"))
BLOCKS, DIR = {"P4096": int(arg(3, "32")), "P8192": int(arg(4, "12"))}, arg(5, "/dev/shm")
ROUNDS, PASSES = 3, 3
HBM_PEAK = 8e12
COUNTS = (256, 4096)
A_KEY, N_KEY = bytes(range(32)), bytes(range(100, 132))


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


def emit(line):
    print(json.dumps(line), flush=True)
    lines.append(line)


for preset in ("P4096", "P8192"):
    ctx = fhe.SEALContext.preset(preset)
    ev = fhe.Evaluator(ctx)
    k, n = ctx.k, ctx.n
    kg = fhe.KeyGenerator(ctx, seed=1)
    for count in COUNTS:
        # (a) expansion
        c0 = ctx.random_ct(count, size=1, seed=fhe.SEED)[:, 0].contiguous()
        full = ctx.empty(count)
        steps, rounds, ms, spread = measure({"expand": lambda: ev.expand_seeded(c0, A_KEY, 0, out=full)})
        moved = 3 * count * k * n * 8                                   # c0 read, c0 and a written
        emit({"workload": "fhe_expand_seeded on %d ciphertexts, %s primes (n=%d k=%d)" % (count, preset, n, k), "rounds": ROUNDS, "steps": steps["expand"],
              "ms": ms["expand"], "ms_rounds": rounds["expand"], "spread": spread["expand"], "us_per_ciphertext": ms["expand"] * 1e3 / count,
              "bytes_read_plus_written": moved, "share_of_hbm_roofline": moved / ms["expand"] * 1e3 / HBM_PEAK,
              "regenerated_bytes_per_second": count * k * n * 8 / ms["expand"] * 1e3, "cipher_blocks": count * k * n // 4})
        # (b) the client's encryption beside the public-key one, same plaintexts
        plain = (ctx.random_ct(count, size=1, seed=fhe.SEED + 2)[:, 0, 0] % ctx.t).contiguous()
        sym = fhe.SymmetricEncryptor(ctx, kg.secret_key(), a_key=A_KEY, noise_key=N_KEY, reproducible=True)
        pke = fhe.DeviceEncryptor(ctx, kg.public_key(), key=N_KEY, reproducible=True)

        def run_sym():
            sym.seek(0)
            sym.encrypt_plains(plain)

        def run_pk():
            pke.seek(0)
            pke.encrypt_plains(plain)

        steps, rounds, ms, spread = measure({"symmetric": run_sym, "public_key": run_pk})
        emit({"workload": "fhe_encrypt_symmetric_batch beside fhe_encrypt_batch, %d plaintexts, %s primes (n=%d k=%d)" % (count, preset, n, k), "rounds": ROUNDS,
              "steps": steps, "symmetric_ms": ms["symmetric"], "symmetric_ms_rounds": rounds["symmetric"], "symmetric_spread": spread["symmetric"],
              "symmetric_us_per_ciphertext": ms["symmetric"] * 1e3 / count, "public_key_ms": ms["public_key"], "public_key_ms_rounds": rounds["public_key"],
              "public_key_spread": spread["public_key"], "public_key_us_per_ciphertext": ms["public_key"] * 1e3 / count,
              "symmetric_over_public_key": ms["symmetric"] / ms["public_key"], "bytes_out_symmetric": count * k * n * 8, "bytes_out_public_key": 2 * count * k * n * 8,
              "includes": "output allocation (torch.empty) in both"})
        del c0, full, plain, sym, pke
        torch.cuda.empty_cache()

    # (c) server_jpeg over the same blocks, seeded and unseeded, alternating
    blocks = BLOCKS[preset]
    lib = fhe._lib.load()
    rec1, rec2 = lib.fhe_io_record_bytes(1, k, n), lib.fhe_io_record_bytes(2, k, n)
    fseed, ffull, fout = (os.path.join(DIR, "fhe_seeded_%s_%s.ct" % (preset, x)) for x in ("c0", "full", "out"))
    try:
        one = torch.empty((192, 1, k, n), dtype=torch.int64).pin_memory()
        two = torch.empty((192, 2, k, n), dtype=torch.int64).pin_memory()
        sseed = fhe.server.StreamFile(fseed, write=True, size=blocks * 192 * rec1)
        sfull = fhe.server.StreamFile(ffull, write=True, size=blocks * 192 * rec2)
        for b in range(blocks):
            c0 = ctx.random_ct(192, size=1, seed=fhe.SEED, first_index=b * 192 * k * n)
            one.copy_(c0)
            two.copy_(ev.expand_seeded(c0[:, 0].contiguous(), A_KEY, b * 192))
            torch.cuda.synchronize()
            sseed.transfer(b * 192, 192, 1, ctx, one, 8)
            sfull.transfer(b * 192, 192, 2, ctx, two, 8)
        sseed.close()
        sfull.close()
        sout = fhe.server.StreamFile(fout, write=True, size=blocks * 192 * rec2)
        runs = {"seeded": [], "unseeded": []}
        quant = list(fhe.YQT)
        for p in range(PASSES + 1):                                      # pass 0 warms up: pages, pinned buffers, plans
            for name, path, seeded in (("seeded", fseed, (A_KEY, 0)), ("unseeded", ffull, None)):
                sin = fhe.server.StreamFile(path)
                stats = {}
                t0 = time.time()
                fhe.server.server_jpeg(ctx, sin, sout, blocks, wave_blocks=8, quant=quant, io_threads=16, stats=stats, seeded=seeded)
                torch.cuda.synchronize()
                wall = time.time() - t0
                sin.close()
                if p:
                    runs[name].append({"bytes_in": stats["bytes_in"], "bytes_out": stats["bytes_out"], "seconds": stats["seconds"], "wall_seconds": wall,
                                       "device_compute_seconds": stats["device_compute_seconds"], "file_read_seconds": stats["file_read_seconds"],
                                       "file_write_seconds": stats["file_write_seconds"]})
        sout.close()
        med = {name: statistics.median(r["seconds"] for r in rs) for name, rs in runs.items()}
        dev = {name: statistics.median(r["device_compute_seconds"] for r in rs) for name, rs in runs.items()}
        emit({"workload": "server_jpeg %d colour blocks with quantisation, %s (n=%d k=%d), files in %s, wave_blocks=8" % (blocks, preset, n, k, DIR), "passes": PASSES,
              "runs": runs, "seconds": med, "device_compute_seconds": dev, "bytes_in": {name: rs[0]["bytes_in"] for name, rs in runs.items()},
              "spread": {name: (max(r["seconds"] for r in rs) - min(r["seconds"] for r in rs)) / med[name] for name, rs in runs.items()},
              "bytes_in_ratio": runs["seeded"][0]["bytes_in"] / runs["unseeded"][0]["bytes_in"], "seconds_ratio": med["seeded"] / med["unseeded"],
              "device_compute_ratio": dev["seeded"] / dev["unseeded"]})
    finally:
        for path in (fseed, ffull, fout):
            if os.path.exists(path):
                os.remove(path)
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    for line in lines:
        fh.write(json.dumps(line) + "\n")

#!/usr/bin/env python3
"""The fused weighted sum of hoisted special-prime rotations (fhe_rotate_sum_sp, csrc/rotsum.hip; circuits.packed_filter2d(fused=True))
beside the op-by-op composition with the SAME special keys (packed_filter2d(fused=False): one fhe_apply_galois_sp, one multiply_plain and
one add per tap -- the path that exists without this feature), on resident data, in one process, alternating:
  box 3x3 (9 taps, 8 rotations) and Gauss 5x5 (25 taps, 24 rotations) over 64-wide tiles, `count` ciphertexts, at the P8192 primes
  (n = 8192) and the P4096 primes (n = 4096), t = 65537, a key for every tap's element.
Per case: ms per call of both, the ratio, output pixels per second (the slots where the window stays inside its tile), the budget left
by both on real encryptions (whole bits from decrypt_batch, beside circuits.rotate_sum_budget), that both decrypt to the same slots, the
transform counts and the launch counts per call (from the code; `trace` lets a kernel trace confirm them).
Device events, two warm-up runs, three alternating rounds per variant.  One JSON line per case to stdout and to
profiles/rotsum_bench.json.  Secondary measurement, not bench.py's.  `trace` as the first argument runs every variant three times and
measures nothing (for `rocprofv3 --kernel-trace --stats`, in a run of its own).
Usage: bench_rotsum.py [mode=bench|trace] [count=256] [window_s=1.0] [out=profiles/rotsum_bench.json]"""
import json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fhip_amd as fhe

arg = lambda i, d: sys.argv[i] if len(sys.argv) > i else d
mode, count, window_s, out_path = arg(1, "bench"), int(arg(2, "256")), float(arg(3, "1.0")), arg(4, os.path.join(ROOT, "profiles", "rotsum_bench.json"))
ROUNDS = 3
T_BATCH = 65537
TILE_W = 64
FILTERS = {"box3x3": (np.ones((3, 3), dtype=np.int64), 3), "gauss5x5": (np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1]), 5)}


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


lines = []
for preset in ("P8192", "P4096"):
    pr = fhe.PRESETS[preset]
    parent = fhe.SEALContext(pr["n"], pr["q"], T_BATCH)
    n, k = parent.n, parent.k
    level = parent.level(k - 1)
    pm = (fhe._lib.load().fhe_arith_path(parent.h) & 3) != 0
    kg = fhe.KeyGenerator(parent, seed=2)
    sk = kg.secret_key()[:level.k].contiguous()
    kgl = fhe.KeyGenerator(level, seed=3, secret_key=sk)
    ev, be = fhe.Evaluator(level), fhe.BatchEncoder(level)
    enc, dec = fhe.DeviceEncryptor(level, kgl.public_key()), fhe.Decryptor(level, sk)
    th = n // 2 // TILE_W
    tiles = np.random.default_rng(1).integers(0, 256, size=(4, 2, th, TILE_W))
    real = enc.encrypt_plains(be.encode(tiles.reshape(4, n).astype(np.uint64)))
    fresh = dec.decrypt_batch(real, with_budget=True)[1]
    resident = level.random_ct(count, seed=fhe.SEED)
    for kind, (w, ksz) in FILTERS.items():
        elts, ws = fhe.circuits.packed_filter_taps(n, T_BATCH, TILE_W, w, ksz, ksz)
        gk = kg.generate_special_galois_keys([g for g in elts if g != 1])
        taps, rot = len(elts), sum(g != 1 for g in elts)
        fns = {"fused": lambda: fhe.circuits.packed_filter2d(ev, gk, resident, TILE_W, w, ksz, ksz, fused=True),
               "op_by_op": lambda: fhe.circuits.packed_filter2d(ev, gk, resident, TILE_W, w, ksz, ksz)}
        if mode == "trace":
            for fn in fns.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            continue
        # the same slots, and the budgets, on real encryptions
        mask = fhe.circuits.packed_filter_valid_mask(n, TILE_W, ksz, ksz)
        pf, bf = dec.decrypt_batch(fhe.circuits.packed_filter2d(ev, gk, real, TILE_W, w, ksz, ksz, fused=True), with_budget=True)
        po, bo = dec.decrypt_batch(fhe.circuits.packed_filter2d(ev, gk, real, TILE_W, w, ksz, ksz), with_budget=True)
        assert np.array_equal(be.decode(pf)[:, mask], be.decode(po)[:, mask]), "the fused filter and the op-by-op filter decrypt to different slots"
        steps = {name: steps_for(fn) for name, fn in fns.items()}
        rounds = {name: [] for name in fns}
        for _ in range(ROUNDS):
            for name, fn in fns.items():
                rounds[name].append(window(fn, steps[name]))
        ms = {name: statistics.median(r) for name, r in rounds.items()}
        L = k - 1
        line = {"workload": "packed_filter2d %s (%d taps, %d rotations), %d ciphertexts of 2 x %d x %d pixels, %s primes (n=%d, level of %d primes + special prime), t=%d"
                            % (kind, taps, rot, count, th, TILE_W, preset, n, L, T_BATCH),
                "path": "pseudo-Mersenne" if pm else "general (FP64 transforms)",
                "rounds": ROUNDS, "steps": steps, "ms": ms, "ms_rounds": rounds, "spread": {name: (max(r) - min(r)) / ms[name] for name, r in rounds.items()},
                "op_by_op_over_fused": ms["op_by_op"] / ms["fused"],
                "valid_pixels_per_ciphertext": int(mask.sum()),
                "output_pixels_per_s": {name: count * int(mask.sum()) / ms[name] * 1e3 for name in ms},
                "transforms_per_ciphertext": {"fused": L * k + 2 * k, "op_by_op": rot * (L * k + 2 * k)},
                "launches_per_call_from_the_code": {"fused": 4 if pm else 6, "op_by_op": rot * (4 if pm else 6) + taps + (taps - 1)},
                "budget_bits": {"fresh": fresh, "fused": bf, "op_by_op": bo,
                                "rotate_sum_budget_of_fresh": fhe.circuits.rotate_sum_budget(parent, min(fresh), ws)}}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del gk
        torch.cuda.empty_cache()

if mode != "trace":
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")

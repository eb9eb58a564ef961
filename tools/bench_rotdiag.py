#!/usr/bin/env python3
"""The diagonal linear map under one key switch (fhe_rotate_diag_sum_sp, csrc/rotdiag.hip; circuits.packed_filter2d(border="zero"))
beside two baselines with the SAME special keys, on resident data, in one process, alternating:
  (a) each_mul_add   Evaluator.rotate_each, then one multiply_plain by the tap's encoded diagonal (prepared once) and one add per tap: the
                     composition DESIGN.md 3.15 names for per-slot weights -- the path that exists without this feature;
  (b) fused_scalar   packed_filter2d(fused=True): scalar weights, wrong at the tile border -- what the per-slot table costs over them.
Cases: box 3x3 and Gauss 5x5 over 64-wide tiles, `count` ciphertexts, at the P8192 primes (n = 8192) and the P4096 primes (n = 4096),
t = 65537, a key for every tap's element.  Per case: ms per call of the three, the ratios, that `diag` and (a) decrypt to the same slots
on EVERY slot and agree with (b) inside the valid mask, the budgets on real encryptions beside circuits.rotate_diag_budget, and the
transform and launch counts per call (from the code; `trace` lets a kernel trace confirm them).
Device events, two warm-up runs, three alternating rounds per variant.  One JSON line per case to stdout and to
profiles/rotdiag_bench.json.  Secondary measurement, not bench.py's.  `trace` as the first argument runs every variant three times and
measures nothing (for a kernel trace, in a run of its own).
Usage: bench_rotdiag.py [mode=bench|trace] [count=256] [window_s=1.0] [out=profiles/rotdiag_bench.json]"""
import json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fhip_amd as fhe

arg = lambda i, d: sys.argv[i] if len(sys.argv) > i else d
mode, count, window_s, out_path = arg(1, "bench"), int(arg(2, "256")), float(arg(3, "1.0")), arg(4, os.path.join(ROOT, "profiles", "rotdiag_bench.json"))
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
        elts, diags = fhe.circuits.packed_filter_diagonals(n, T_BATCH, TILE_W, w, ksz, ksz, border="zero")
        gk = kg.generate_special_galois_keys([g for g in elts if g != 1])
        taps, rot = len(elts), sum(g != 1 for g in elts)
        plan = fhe.RotDiagPlan(level, gk, elts, diags)
        each_plan = fhe.RotSumPlan(level, gk, elts)
        prepared = [fhe.PreparedPlain(level, p) for p in plan.plains]

        def diag(ct=None):
            return ev.rotate_diag_sum(resident if ct is None else ct, plan)

        def each_mul_add(ct=None):
            each = ev.rotate_each(resident if ct is None else ct, each_plan)
            acc = ev.multiply_plain(each[0], prepared[0])
            for j in range(1, taps):
                ev.add(acc, ev.multiply_plain(each[j], prepared[j]), out=acc)
            return acc

        def fused_scalar(ct=None):
            return fhe.circuits.packed_filter2d(ev, gk, resident if ct is None else ct, TILE_W, w, ksz, ksz, fused=True)

        fns = {"diag": diag, "each_mul_add": each_mul_add, "fused_scalar": fused_scalar}
        if mode == "trace":
            for fn in fns.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            continue
        # the same slots, and the budgets, on real encryptions
        mask = fhe.circuits.packed_filter_valid_mask(n, TILE_W, ksz, ksz)
        pd, bd = dec.decrypt_batch(diag(real), with_budget=True)
        pa, ba = dec.decrypt_batch(each_mul_add(real), with_budget=True)
        pb, bb = dec.decrypt_batch(fused_scalar(real), with_budget=True)
        want = np.stack([np.stack([fhe.circuits.packed_filter_border_model(tiles[c, r], w, ksz, ksz, T_BATCH) for r in range(2)]).reshape(n) for c in range(4)])
        same = {"diag_is_the_zero_padded_model": bool(np.array_equal(be.decode(pd), want.astype(np.uint64))),
                "diag_is_each_mul_add": bool(np.array_equal(be.decode(pd), be.decode(pa))),
                "diag_is_fused_scalar_inside_the_valid_mask": bool(np.array_equal(be.decode(pd)[:, mask], be.decode(pb)[:, mask]))}
        if min(bd) > 0 and min(ba) > 0 and min(bb) > 0:                 # with budget left, a difference is a bug; without, it is the parameters'
            assert all(same.values()), same
        steps = {name: steps_for(fn) for name, fn in fns.items()}
        rounds = {name: [] for name in fns}
        for _ in range(ROUNDS):
            for name, fn in fns.items():
                rounds[name].append(window(fn, steps[name]))
        ms = {name: statistics.median(r) for name, r in rounds.items()}
        L = k - 1
        gen = 7                                                        # general path: stage c_0, its transforms, the digits, their transforms, accumulate, inverse transforms, drop
        line = {"workload": "packed_filter2d %s border=zero (%d taps, %d rotations), %d ciphertexts of 2 x %d x %d pixels, %s primes (n=%d, level of %d primes + special prime), t=%d"
                            % (kind, taps, rot, count, th, TILE_W, preset, n, L, T_BATCH),
                "path": "pseudo-Mersenne" if pm else "general (FP64 transforms)",
                "rounds": ROUNDS, "steps": steps, "ms": ms, "ms_rounds": rounds, "spread": {name: (max(r) - min(r)) / ms[name] for name, r in rounds.items()},
                "each_mul_add_over_diag": ms["each_mul_add"] / ms["diag"], "diag_over_fused_scalar": ms["diag"] / ms["fused_scalar"],
                "pixels_per_ciphertext": n, "output_pixels_per_s": {name: count * (int(mask.sum()) if name == "fused_scalar" else n) / ms[name] * 1e3 for name in ms},
                "transforms_per_ciphertext": {"diag": L * k + L + 2 * k, "each_mul_add": L * k + rot * 2 * k + taps * 4 * L, "fused_scalar": L * k + 2 * k},
                "launches_per_call_from_the_code": {"diag": 4 if pm else gen, "fused_scalar": 4 if pm else 6},
                "same_slots": same,
                "budget_bits": {"fresh": fresh, "diag": bd, "each_mul_add": ba, "fused_scalar": bb,
                                "rotate_diag_budget_of_fresh": fhe.circuits.rotate_diag_budget(parent, min(fresh), plan.plains)}}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del gk, plan, each_plan, prepared
        torch.cuda.empty_cache()

if mode != "trace":
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")

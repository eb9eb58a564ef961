#!/usr/bin/env python3
"""Galois rotations (fhe_apply_galois, csrc/galois.hip) on resident data, in one process, alternating:
  (a) one rotation of a batch of `count` size-2 ciphertexts: the fused path (default), the fused path with the digit kernel's permuted loads
      taken through LDS (FHE_GALOIS_GATHER_LDS=1), the staged path (FHE_GALOIS_STAGED=1), and fhe_relinearize_to on the same batch -- the
      same key switch without the permutation; ratio = fused / relinearize is the figure of merit, fused <= staged the adoption rule;
  (b) circuits.packed_filter2d (box 3x3, 64x64 tiles, two per ciphertext at n = 8192) beside fhe_filter2d on a 64x64 image of one
      ciphertext per pixel: output pixels / s of both, their ratio and the bytes per pixel of both representations;
  (d) the noise budget one rotation consumes at dbc 30 and 60 (t = 65537), from decrypt_batch(with_budget=True).
Device events, two warm-up runs, three alternating rounds per variant of at least a second each.  One JSON line per case to stdout and to
profiles/galois_bench.json.  Secondary measurement, not bench.py's.  `trace` as the first argument runs every variant of (a) five times
and measures nothing (for a kernel trace).
Usage: bench_galois.py [parts=abd|trace] [count=256] [window_s=1.0] [out=profiles/galois_bench.json]"""
import ctypes as C, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fhip_amd as fhe

arg = lambda i, d: sys.argv[i] if len(sys.argv) > i else d
parts, count, window_s, out_path = arg(1, "abd"), int(arg(2, "256")), float(arg(3, "1.0")), arg(4, os.path.join(ROOT, "profiles", "galois_bench.json"))
ROUNDS = 3
T_BATCH = 65537
L = fhe._lib.load()
p = lambda t: C.c_void_p(t.data_ptr())


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


def rotation_cases():
    for preset, dbcs in (("P8192", (30, 60)), ("P4096", (30, 60))):
        pr = fhe.PRESETS[preset]
        ctxs = {"fused": fhe.SEALContext.preset(preset), "fused_lds_gather": fhe.SEALContext.preset(preset, switches={"FHE_GALOIS_GATHER_LDS": "1"}),
                "staged": fhe.SEALContext.preset(preset, switches={"FHE_GALOIS_STAGED": "1"})}
        ctx = ctxs["fused"]
        n, k, kn = ctx.n, ctx.k, ctx.k * ctx.n
        g = fhe.galois_element(n, 1)
        ct = ctx.random_ct(count, seed=fhe.SEED)
        ct3 = ctx.random_ct(count, size=3, seed=fhe.SEED + 1)
        out = ctx.empty(count)
        for dbc in dbcs:
            words = L.fhe_evk_words(ctx.h, dbc)
            key = torch.empty(words, dtype=torch.int64, device=ctx.device)
            fhe._lib.call("fhe_fill_random", ctx.h, p(key), words // kn, 7, 0, None)          # any reduced residues time like a key
            nbytes = max(L.fhe_apply_galois_scratch_bytes(ctx.h, dbc, count), L.fhe_relinearize_scratch_bytes(ctx.h, dbc, count))
            scr = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=ctx.device)

            def rot(c):
                return lambda: fhe._lib.call("fhe_apply_galois", c.h, p(ct), 2 * kn, p(out), 2 * kn, count, g, p(key), dbc, p(scr), nbytes, None)

            def relin():
                fhe._lib.call("fhe_relinearize_to", ctx.h, p(ct3), 3 * kn, p(out), 2 * kn, count, p(key), dbc, p(scr), nbytes, None)

            fns = dict({name: rot(c) for name, c in ctxs.items()}, relinearize_to=relin)
            ref = None
            for name in ctxs:                                   # the three paths give the same bits
                fns[name]()
                ref = out.clone() if ref is None else ref
                assert torch.equal(out, ref), name
            yield preset, ctx, dbc, fns
        del ct, ct3, out, ctxs
        torch.cuda.empty_cache()


lines = []
if parts == "trace":
    for preset, ctx, dbc, fns in rotation_cases():
        for fn in fns.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
    sys.exit(0)

if "a" in parts:
    for preset, ctx, dbc, fns in rotation_cases():
        steps = {name: steps_for(fn) for name, fn in fns.items()}
        rounds = {name: [] for name in fns}
        for _ in range(ROUNDS):
            for name, fn in fns.items():
                rounds[name].append(window(fn, steps[name]))
        ms = {name: statistics.median(r) for name, r in rounds.items()}
        line = {"workload": "apply_galois g=3, %d ciphertexts, %s (n=%d k=%d) dbc=%d" % (count, preset, ctx.n, ctx.k, dbc), "arith_path": L.fhe_arith_path(ctx.h),
                "digits": L.fhe_evk_digits(ctx.h, dbc), "rounds": ROUNDS, "steps": steps, "ms": ms, "ms_rounds": rounds,
                "spread": {name: (max(r) - min(r)) / ms[name] for name, r in rounds.items()},
                "ratio_fused_to_relinearize": ms["fused"] / ms["relinearize_to"], "ratio_staged_to_relinearize": ms["staged"] / ms["relinearize_to"],
                "ratio_fused_to_staged": ms["fused"] / ms["staged"], "rotations_per_s": count / ms["fused"] * 1e3}
        print(json.dumps(line), flush=True)
        lines.append(line)

Q4 = fhe.PRESETS["P8192"]["q"]
if "b" in parts:
    ctx = fhe.SEALContext(8192, Q4, T_BATCH)
    ev, kg = fhe.Evaluator(ctx), fhe.KeyGenerator(ctx, seed=1)
    tw, cts = 64, 8
    w = np.ones((3, 3), dtype=np.int64)
    hops = kg.generate_galois_keys(30)
    direct = kg.generate_galois_keys(30, elements=[fhe.galois_element(ctx.n, dy * tw + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx])
    packed = ctx.random_ct(cts, seed=3)
    valid = int(fhe.circuits.packed_filter_valid_mask(ctx.n, tw, 3, 3).sum())
    side = 64
    src = ctx.random_ct(side * side, seed=4)
    plan = fhe.FilterPlan(ctx, np.full((3, 3), 1.0))
    taps = fhe.filter_tap_plan(side, side, 3, 3)[0]
    out = ctx.empty(side * side)
    fns = {"packed_default_keys": lambda: fhe.circuits.packed_filter2d(ev, hops, packed, tw, w, 3, 3),
           "packed_direct_keys": lambda: fhe.circuits.packed_filter2d(ev, direct, packed, tw, w, 3, 3),
           "filter2d_per_pixel": lambda: ev.filter2d(plan, src, taps, out=out)}
    steps = {name: steps_for(fn) for name, fn in fns.items()}
    rounds = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            rounds[name].append(window(fn, steps[name]))
    ms = {name: statistics.median(r) for name, r in rounds.items()}
    ct_bytes = 2 * ctx.k * ctx.n * 8
    pps = {"packed_default_keys": cts * valid / ms["packed_default_keys"] * 1e3, "packed_direct_keys": cts * valid / ms["packed_direct_keys"] * 1e3,
           "filter2d_per_pixel": side * side / ms["filter2d_per_pixel"] * 1e3}
    line = {"workload": "box 3x3: packed_filter2d on %d ciphertexts of two 64x64 tiles vs fhe_filter2d on a 64x64 image, P8192 primes, t=65537, dbc 30" % cts,
            "rotations_per_ciphertext": {"packed_default_keys": sum(len(ev.rotation_plan(dy * tw + dx, hops)) for dy in (-1, 0, 1) for dx in (-1, 0, 1)), "packed_direct_keys": 8},
            "valid_pixels_per_ciphertext": valid, "ms": ms, "ms_rounds": rounds, "steps": steps, "output_pixels_per_s": pps,
            "ratio_packed_direct_to_per_pixel": pps["packed_direct_keys"] / pps["filter2d_per_pixel"],
            "ratio_packed_default_to_per_pixel": pps["packed_default_keys"] / pps["filter2d_per_pixel"],
            "bytes_per_pixel": {"packed": ct_bytes / ctx.n, "per_pixel": ct_bytes}}
    print(json.dumps(line), flush=True)
    lines.append(line)
    del packed, src, out, hops, direct
    torch.cuda.empty_cache()

if "d" in parts:
    for preset in ("P4096", "P8192"):
        pr = fhe.PRESETS[preset]
        ctx = fhe.SEALContext(pr["n"], pr["q"], T_BATCH)
        ev, kg, be = fhe.Evaluator(ctx), fhe.KeyGenerator(ctx, seed=2), fhe.BatchEncoder(ctx)
        enc, dec = fhe.DeviceEncryptor(ctx, kg.public_key()), fhe.Decryptor(ctx, kg.secret_key())
        slots = np.random.default_rng(1).integers(0, T_BATCH, size=(4, ctx.n), dtype=np.uint64)
        ct = enc.encrypt_plains(be.encode(slots))
        fresh = dec.decrypt_batch(ct, with_budget=True)[1]
        for dbc in (30, 60):
            keys = kg.generate_galois_keys(dbc, elements=[3, 2 * ctx.n - 1])
            plain, rows = dec.decrypt_batch(ev.rotate_rows(ct, 1, keys), with_budget=True)
            assert np.array_equal(be.decode(plain).reshape(4, 2, -1), np.roll(slots.reshape(4, 2, -1), -1, axis=2))
            cols = dec.decrypt_batch(ev.rotate_columns(ct, keys), with_budget=True)[1]
            line = {"workload": "noise budget of one rotation, %s primes, t=65537, dbc=%d" % (preset, dbc), "fresh_bits": fresh, "after_rotate_rows_bits": rows,
                    "after_rotate_columns_bits": cols, "consumed_bits": min(fresh) - min(min(rows), min(cols))}
            print(json.dumps(line), flush=True)
            lines.append(line)

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    for line in lines:
        fh.write(json.dumps(line) + "\n")

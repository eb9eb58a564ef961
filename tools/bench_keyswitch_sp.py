#!/usr/bin/env python3
"""The key switch with a special prime (fhe_apply_galois_sp / fhe_relinearize_sp_poly, csrc/keyswitch_sp.hip) beside SEAL 2.3's bit
decomposition (fhe_apply_galois / fhe_relinearize_to), on resident data, in one process, alternating:
  (a) one rotation (g = 3) and one relinearisation step of `count` ciphertexts at the P8192 and P4096 primes:
        special      special-prime keys: ciphertexts on the first k - 1 primes, the last prime is the special one
        level_dbc30  the bit decomposition at dbc 30 at the SAME level (the same ciphertext bytes)
        level_dbc60  the same at dbc 60
        full_dbc30   the bit decomposition on all k primes (what a user runs today)
        full_dbc60
      milliseconds, ratios to `special`, and the algorithmic bytes (ciphertexts read and written once, the key read once) over the time,
      against the 8 TB/s roofline;
  (d) the noise budget one rotation leaves with each kind of key at the same level and on all k primes (t = 65537, the presets' own n).
Device events, two warm-up runs, three alternating rounds per variant.  One JSON line per case to stdout and to
profiles/keyswitch_sp_bench.json.  Secondary measurement, not bench.py's.  `trace` as the first argument runs every variant of (a) five
times and measures nothing (for a kernel trace).
Usage: bench_keyswitch_sp.py [parts=ad|trace] [count=256] [window_s=1.0] [out=profiles/keyswitch_sp_bench.json]"""
import ctypes as C, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fhip_amd as fhe

arg = lambda i, d: sys.argv[i] if len(sys.argv) > i else d
parts, count, window_s, out_path = arg(1, "ad"), int(arg(2, "256")), float(arg(3, "1.0")), arg(4, os.path.join(ROOT, "profiles", "keyswitch_sp_bench.json"))
ROUNDS = 3
T_BATCH = 65537
HBM_BYTES_PER_S = 8e12
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


def random_words(ctx, words):
    key = torch.empty(words, dtype=torch.int64, device=ctx.device)
    fhe._lib.call("fhe_fill_random", ctx.h, p(key), words // (ctx.k * ctx.n), 7, 0, None)      # any reduced residues time like a key
    return key


def cases():
    """(preset, operation, {variant: (call, algorithmic bytes)}) with every buffer resident"""
    for preset in ("P8192", "P4096"):
        parent = fhe.SEALContext.preset(preset)
        level = parent.level(parent.k - 1)
        n = parent.n
        for op in ("rotation", "relinearise"):
            size = 2 if op == "rotation" else 3
            fns, keep = {}, []
            # special-prime keys: the call goes to the parent's handle, the ciphertexts are the level's
            kl = level.k * n
            ct, out = level.random_ct(count, size=size, seed=fhe.SEED), level.empty(count)
            key = random_words(parent, L.fhe_ksk_sp_words(parent.h))
            nbytes = L.fhe_key_switch_sp_scratch_bytes(parent.h, count)
            scr = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=parent.device)
            keep += [ct, out, key, scr]
            if op == "rotation":
                call = lambda ct=ct, out=out, key=key, scr=scr, nbytes=nbytes, kl=kl: fhe._lib.call("fhe_apply_galois_sp", parent.h, p(ct), 2 * kl, p(out), 2 * kl, count, 3, p(key), p(scr), nbytes, None)
            else:
                call = lambda ct=ct, out=out, key=key, scr=scr, nbytes=nbytes, kl=kl: fhe._lib.call("fhe_relinearize_sp_poly", parent.h, p(ct), 3 * kl, 2, p(out), 2 * kl, count, p(key), p(scr), nbytes, None)
            fns["special"] = (call, (count * (size + 2) * kl + key.numel()) * 8)
            for where, ctx in (("level", level), ("full", parent)):
                kn = ctx.k * n
                ct, out = ctx.random_ct(count, size=size, seed=fhe.SEED), ctx.empty(count)
                keep += [ct, out]
                for dbc in (30, 60):
                    key = random_words(ctx, L.fhe_evk_words(ctx.h, dbc))
                    nbytes = max(L.fhe_apply_galois_scratch_bytes(ctx.h, dbc, count), L.fhe_relinearize_scratch_bytes(ctx.h, dbc, count))
                    scr = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=ctx.device)
                    keep += [key, scr]
                    if op == "rotation":
                        call = lambda ctx=ctx, ct=ct, out=out, key=key, scr=scr, nbytes=nbytes, kn=kn, dbc=dbc: fhe._lib.call(
                            "fhe_apply_galois", ctx.h, p(ct), 2 * kn, p(out), 2 * kn, count, 3, p(key), dbc, p(scr), nbytes, None)
                    else:
                        call = lambda ctx=ctx, ct=ct, out=out, key=key, scr=scr, nbytes=nbytes, kn=kn, dbc=dbc: fhe._lib.call(
                            "fhe_relinearize_to", ctx.h, p(ct), 3 * kn, p(out), 2 * kn, count, p(key), dbc, p(scr), nbytes, None)
                    fns["%s_dbc%d" % (where, dbc)] = (call, (count * (size + 2) * kn + key.numel()) * 8)
            yield preset, parent, op, fns
            del fns, keep
            torch.cuda.empty_cache()


lines = []
if parts == "trace":
    for preset, parent, op, fns in cases():
        for fn, _ in fns.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
    sys.exit(0)

if "a" in parts:
    for preset, parent, op, fns in cases():
        steps = {name: steps_for(fn) for name, (fn, _) in fns.items()}
        rounds = {name: [] for name in fns}
        for _ in range(ROUNDS):
            for name, (fn, _) in fns.items():
                rounds[name].append(window(fn, steps[name]))
        ms = {name: statistics.median(r) for name, r in rounds.items()}
        k = parent.k
        line = {"workload": "%s, %d ciphertexts, %s primes (n=%d, k=%d; special-prime and level variants on %d primes)" % (op, count, preset, parent.n, k, k - 1),
                "forward_transforms_per_ciphertext": {"special": (k - 1) * k, "level_dbc30": (k - 1) ** 2 * L.fhe_evk_digits(parent.level(k - 1).h, 30),
                                                      "level_dbc60": (k - 1) ** 2 * L.fhe_evk_digits(parent.level(k - 1).h, 60),
                                                      "full_dbc30": k * k * L.fhe_evk_digits(parent.h, 30), "full_dbc60": k * k * L.fhe_evk_digits(parent.h, 60)},
                "inverse_transforms_per_ciphertext": {"special": 2 * k, "level_dbc30": 2 * (k - 1), "level_dbc60": 2 * (k - 1), "full_dbc30": 2 * k, "full_dbc60": 2 * k},
                "rounds": ROUNDS, "steps": steps, "ms": ms, "ms_rounds": rounds, "spread": {name: (max(r) - min(r)) / ms[name] for name, r in rounds.items()},
                "ratio_to_special": {name: ms[name] / ms["special"] for name in ms},
                "algorithmic_bytes": {name: b for name, (_, b) in fns.items()},
                "algorithmic_GB_per_s": {name: b / ms[name] / 1e6 for name, (_, b) in fns.items()},
                "share_of_8TBps_roofline": {name: b / (ms[name] * 1e-3) / HBM_BYTES_PER_S for name, (_, b) in fns.items()},
                "key_switches_per_s": {name: count / ms[name] * 1e3 for name in ms}}
        print(json.dumps(line), flush=True)
        lines.append(line)

if "d" in parts:
    for preset in ("P4096", "P8192"):
        pr = fhe.PRESETS[preset]
        parent = fhe.SEALContext(pr["n"], pr["q"], T_BATCH)
        level = parent.level(parent.k - 1)
        kg = fhe.KeyGenerator(parent, seed=2)
        sk = kg.secret_key()
        slots = np.random.default_rng(1).integers(0, T_BATCH, size=(4, parent.n), dtype=np.uint64)
        budgets = {}
        for where, ctx, s in (("level", level, sk[:level.k].contiguous()), ("full", parent, sk)):
            kgc = kg if ctx is parent else fhe.KeyGenerator(ctx, seed=3, secret_key=s)
            ev, be = fhe.Evaluator(ctx), fhe.BatchEncoder(ctx)
            enc, dec = fhe.DeviceEncryptor(ctx, kgc.public_key()), fhe.Decryptor(ctx, s)
            ct = enc.encrypt_plains(be.encode(slots))
            budgets["%s_fresh" % where] = dec.decrypt_batch(ct, with_budget=True)[1]
            variants = [("%s_dbc%d" % (where, dbc), kgc.generate_galois_keys(dbc, elements=[3])) for dbc in (30, 60)]
            if ctx is level:
                variants.append(("special", kg.generate_special_galois_keys([3])))
            for name, keys in variants:
                plain, left = dec.decrypt_batch(ev.rotate_rows(ct, 1, keys), with_budget=True)
                if min(left) > 0:
                    assert np.array_equal(be.decode(plain).reshape(4, 2, -1), np.roll(slots.reshape(4, 2, -1), -1, axis=2)), name
                budgets[name] = left
        fresh = {"special": "level_fresh", "level_dbc30": "level_fresh", "level_dbc60": "level_fresh", "full_dbc30": "full_fresh", "full_dbc60": "full_fresh"}
        line = {"workload": "noise budget after one rotation, %s primes (n=%d), t=65537" % (preset, parent.n), "budget_bits": budgets,
                "consumed_bits": {name: min(budgets[f]) - min(budgets[name]) for name, f in fresh.items()},
                "bound_bits_special": fhe.circuits.special_key_switch_budget(parent, min(budgets["level_fresh"]))}
        print(json.dumps(line), flush=True)
        lines.append(line)

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    for line in lines:
        fh.write(json.dumps(line) + "\n")

#!/usr/bin/env python3
"""The baby-step / giant-step linear map in one call (fhe_rotate_bsgs_sp, csrc/rotbsgs.hip; Evaluator.rotate_bsgs) beside what exists without
it, on resident data, in one process, alternating:
  (a) diag_chunks   the map cut into chunks of at most 64 diagonals, each one Evaluator.rotate_diag_sum with a key PER DIAGONAL, added;
  (b) op_by_op      the same baby / giant split from existing entry points with the SAME keys: rotate_each over the baby steps, one
                    multiply_plain (plaintexts prepared once) and add per present pair, apply_galois per non-identity giant step, add;
  (c) separable     (the DCT only) the pair of rotate_diag_sum calls, 15 diagonals each: D along the block's rows, then down its columns.
Cases: the 64 x 64 matrix D (x) D of the 2-D 8 x 8 DCT (bits = 4) as 16 x 8 steps at the P8192 primes (n = 8192) and the P4096 primes
(n = 4096), and one dense map of 256 diagonals (steps 0 .. 255, random slot values) as 16 x 16 steps at the P8192 primes; t = 65537.
Per case: ms per call, the ratios, that all variants decrypt to the same slots on real encryptions (and the DCT to B @ x), the budgets
beside circuits.rotate_bsgs_budget, keys and key bytes, transforms per ciphertext (from the code).
Device events, two warm-up runs, three alternating rounds per variant.  One JSON line per case to stdout and to
profiles/rotbsgs_bench.json.  Secondary measurement, not bench.py's.
Usage: bench_rotbsgs.py [count=256] [window_s=1.0] [out=profiles/rotbsgs_bench.json]"""
import json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fhip_amd as fhe

arg = lambda i, d: sys.argv[i] if len(sys.argv) > i else d
count, window_s, out_path = int(arg(1, "256")), float(arg(2, "1.0")), arg(3, os.path.join(ROOT, "profiles", "rotbsgs_bench.json"))
ROUNDS = 3
T_BATCH = 65537
BABY = 16
c = fhe.circuits


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
for preset, kind in (("P8192", "dct2d"), ("P4096", "dct2d"), ("P8192", "dense256")):
    pr = fhe.PRESETS[preset]
    parent = fhe.SEALContext(pr["n"], pr["q"], T_BATCH)
    n, k = parent.n, parent.k
    L = k - 1
    level = parent.level(L)
    pm = (fhe._lib.load().fhe_arith_path(parent.h) & 3) != 0
    kg = fhe.KeyGenerator(parent, seed=2)
    sk = kg.secret_key()[:level.k].contiguous()
    kgl = fhe.KeyGenerator(level, seed=3, secret_key=sk)
    ev, be = fhe.Evaluator(level), fhe.BatchEncoder(level)
    enc, dec = fhe.DeviceEncryptor(level, kgl.public_key()), fhe.Decryptor(level, sk)
    rng = np.random.default_rng(1)
    x = rng.integers(0, 16, size=(2, n))
    real = enc.encrypt_plains(be.encode(x.astype(np.uint64)))
    fresh = dec.decrypt_batch(real, with_budget=True)[1]
    resident = level.random_ct(count, seed=fhe.SEED)
    if kind == "dct2d":
        B = c.block_dct2d_matrix(4)
        elts, diags = c.block_matvec_diagonals(n, T_BATCH, B)
        step_of = {fhe.galois_element(n, s): s for s in range(-63, 64)}
        steps_all = [step_of[g] for g in elts]
        want = np.stack([(np.einsum("ab,gb->ga", B.astype(object), row.reshape(n // 64, 64).astype(object)) % T_BATCH).reshape(n) for row in x]).astype(np.uint64)
    else:
        steps_all = list(range(256))
        diags = rng.integers(0, T_BATCH, size=(256, n), dtype=np.uint64)
        elts = [fhe.galois_element(n, s) for s in steps_all]
        want = None
    bs, gs, split = c.bsgs_split(n, steps_all, diags, BABY)
    bsgs_keys = kg.generate_special_galois_keys([fhe.galois_element(n, s) for s in bs + gs if s])
    plan = fhe.RotBsgsPlan(level, bsgs_keys, bs, gs, split, steps=True)
    each_plan = fhe.RotSumPlan(level, bsgs_keys, plan.baby)
    prepared = [[fhe.PreparedPlain(level, p) if p.any() else None for p in row] for row in plan.plains]
    diag_keys = kg.generate_special_galois_keys([g for g in elts if g != 1])
    chunks = [fhe.RotDiagPlan(level, diag_keys, elts[i:i + 64], diags[i:i + 64]) for i in range(0, len(elts), 64)]

    def fused(ct=None):
        return ev.rotate_bsgs(resident if ct is None else ct, plan)

    def op_by_op(ct=None):
        rot = ev.rotate_each(resident if ct is None else ct, each_plan)
        out = None
        for h, row in zip(plan.giant, prepared):
            inner = None
            for j, p in enumerate(row):
                if p is None:
                    continue
                term = ev.multiply_plain(rot[j], p)
                inner = term if inner is None else ev.add(inner, term, out=inner)
            if h != 1:
                inner = ev.apply_galois(inner, h, bsgs_keys)
            out = inner if out is None else ev.add(out, inner, out=out)
        return out

    def diag_chunks(ct=None):
        src = resident if ct is None else ct
        out = ev.rotate_diag_sum(src, chunks[0])
        for p in chunks[1:]:
            ev.add(out, ev.rotate_diag_sum(src, p), out=out)
        return out

    fns = {"fused": fused, "op_by_op": op_by_op, "diag_chunks": diag_chunks}
    sep_keys = None
    if kind == "dct2d":
        D = c.dct8_matrix(4)
        e1, d1 = c.block_matvec_diagonals(n, T_BATCH, np.kron(np.eye(8, dtype=np.int64), D))
        e2, d2 = c.block_matvec_diagonals(n, T_BATCH, np.kron(D, np.eye(8, dtype=np.int64)))
        sep_keys = kg.generate_special_galois_keys([g for g in e1 + e2 if g != 1])
        p1, p2 = fhe.RotDiagPlan(level, sep_keys, e1, d1), fhe.RotDiagPlan(level, sep_keys, e2, d2)

        def separable(ct=None):
            return ev.rotate_diag_sum(ev.rotate_diag_sum(resident if ct is None else ct, p1), p2)

        fns["separable"] = separable
    # the same slots, and the budgets, on real encryptions
    dec_of = {name: dec.decrypt_batch(fn(real), with_budget=True) for name, fn in fns.items()}
    slots = {name: be.decode(v[0]) for name, v in dec_of.items()}
    budgets = {name: v[1] for name, v in dec_of.items()}
    same = {"fused_is_" + name: bool(np.array_equal(slots["fused"], slots[name])) for name in fns if name != "fused"}
    if want is not None:
        same["fused_is_B_at_x"] = bool(np.array_equal(slots["fused"], want))
    for name in fns:                                                    # with budget left, a difference is a bug; without, it is the parameters'
        if name != "fused" and min(budgets[name]) > 0 and min(budgets["fused"]) > 0:
            assert same["fused_is_" + name], (preset, kind, name)
    if want is not None and min(budgets["fused"]) > 0:
        assert same["fused_is_B_at_x"], (preset, kind)
    steps = {name: steps_for(fn) for name, fn in fns.items()}
    rounds = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            rounds[name].append(window(fn, steps[name]))
    ms = {name: statistics.median(r) for name, r in rounds.items()}
    G1, G2 = len(bs), len(gs)
    pairs = int(plan.plains.any(axis=2).sum())
    rb, rg = sum(g != 1 for g in plan.baby), sum(g != 1 for g in plan.giant)
    key_words = L * 2 * k * n
    transforms = {"fused": (L * k + L) + G2 * (1 + L + L * k) + 2 + 2 * L,
                  "op_by_op": L * k + rb * 2 * k + pairs * 4 * L + rg * (L * k + 2 * k),
                  "diag_chunks": len(chunks) * (L * k + L + 2 * k)}
    keys = {"fused": rb + rg, "op_by_op": rb + rg, "diag_chunks": len(diag_keys.elements())}
    if sep_keys is not None:
        transforms["separable"] = 2 * (L * k + L + 2 * k)
        keys["separable"] = len(sep_keys.elements())
    line = {"workload": "%s: %d diagonals as %d baby x %d giant steps (%d present pairs), %d ciphertexts, %s primes (n=%d, level of %d primes + special prime), t=%d"
                        % ("2-D 8x8 DCT (bits=4) on blocks of 64 slots" if kind == "dct2d" else "dense map, steps 0..255", len(steps_all), G1, G2, pairs, count, preset, n, L, T_BATCH),
            "path": "pseudo-Mersenne" if pm else "general (FP64 transforms)", "count": count, "window_s": window_s,
            "rounds": ROUNDS, "steps": steps, "ms": ms, "ms_rounds": rounds, "spread": {name: (max(r) - min(r)) / ms[name] for name, r in rounds.items()},
            "over_fused": {name: ms[name] / ms["fused"] for name in ms if name != "fused"},
            "keys": keys, "key_bytes": {name: v * key_words * 8 for name, v in keys.items()},
            "transforms_per_ciphertext": transforms,
            "scratch_bytes_per_ciphertext_fused": plan.scratch_bytes(1),
            "same_slots": same,
            "budget_bits": dict(budgets, fresh=fresh, rotate_bsgs_budget_of_fresh=c.rotate_bsgs_budget(parent, min(fresh), plan.plains, plan.baby, plan.giant))}
    print(json.dumps(line), flush=True)
    lines.append(line)
    del plan, each_plan, prepared, chunks, bsgs_keys, diag_keys, sep_keys, fns, resident
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    for line in lines:
        fh.write(json.dumps(line) + "\n")

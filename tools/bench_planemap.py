#!/usr/bin/env python3
"""Sparse integer maps across position-packed ciphertexts (csrc/planemap.hip) on resident data, in one process, alternating.  Cases, each
at the P4096 and P8192 primes with t = 4295294977, on one frame set (ciphertext p holds pixel p of n frames: 4096 ciphertexts of input fill
the device):
  resize   64x64 -> 32x32 Catmull-Rom, both passes (circuits.packed_resize_plans, 8-bit weights);
  box3     box 3x3 over 64x64 tiles (circuits.packed_tile_filter_plan);
  chroma   the 4:2:0 average, 2x2 at stride 2, over 64x64 tiles.
Variants on the same batch: the windowed kernel with window 16, 32 and 64, the direct kernel (a context created with FHE_PLANEMAP_DIRECT=1),
and the op-by-op composition -- per slot p one Evaluator.multiply_plain of the gathered sources with a prepared one-coefficient plaintext and
one Evaluator.add (the gathers are torch index_selects and are part of its time).  Reported per case: the times, (bytes in + bytes out) /
time of each pass as a share of the 8 TB/s HBM roofline, source_reads amplification per window, output pixels/s with
ciphertext bytes per pixel, beside Evaluator.resize_plain on one 64x64 image of one ciphertext per pixel (resize) and circuits.packed_filter2d
with direct Galois keys on slot-packed tiles (box3).
Adoption rule, written before measuring: the windowed kernel is the default only if it is not slower than the direct kernel in every case;
the default window is the fastest of 16, 32, 64 on the resize case; fused must beat the composition in every case.
Device events, two warm-up runs, three alternating rounds per variant of at least `window_s` each, the spread reported.  One JSON line per
case to stdout and to profiles/planemap_bench.json.  Secondary measurement, not bench.py's.
Usage: bench_planemap.py [cases=resize,box3,chroma] [window_s=0.5] [out=profiles/planemap_bench.json] [presets=P4096,P8192]"""
import json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fhip_amd as fhe

arg = lambda i, d: sys.argv[i] if len(sys.argv) > i else d
cases, window_s, out_path, presets = arg(1, "resize,box3,chroma").split(","), float(arg(2, "0.5")), arg(3, os.path.join(ROOT, "profiles", "planemap_bench.json")), arg(4, "P4096,P8192").split(",")
ROUNDS = 3
T33 = 4295294977
HBM_PEAK = 8e12
SIDE = 64
L = fhe._lib.load()
circuits = fhe.circuits


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


def passes_of(case, ctx, window):
    if case == "resize":
        return list(circuits.packed_resize_plans(ctx, SIDE, SIDE, SIDE // 2, SIDE // 2, window=window))
    f = circuits.packed_filter_integer("box3" if case == "box3" else "chroma420")
    kh, kw = f["weights"].shape
    return [circuits.packed_tile_filter_plan(ctx, SIDE, SIDE, f["weights"], kw, kh, anchor=f["anchor"], stride=f["stride"], window=window)]


def composed_fn(ctx, ev, passes, ct):
    """multiply_plain / add per slot on gathered batches; every slot column of these plans has one weight"""
    prep, idx = {}, []
    for pl in passes:
        cols = []
        for p in range(pl.taps.shape[1]):
            w = set(int(v) for v in pl.weights[:, p])
            assert len(w) == 1 and 0 not in w, "the composition here expects one weight per slot column"
            w = w.pop() % ctx.t
            prep.setdefault(w, fhe.PreparedPlain(ctx, np.array([w], dtype=np.uint64)))
            cols.append((torch.from_numpy(pl.taps[:, p].astype(np.int64)).to(ctx.device), prep[w]))
        idx.append(cols)

    def run():
        x = ct[0]
        for cols in idx:
            acc = None
            for gather, plain in cols:
                term = ev.multiply_plain(x.index_select(0, gather), plain)
                acc = term if acc is None else ev.add(acc, term, out=acc)
            x = acc
        return x
    return run


lines = []
for preset in presets:
    pr = fhe.PRESETS[preset]
    ctx = fhe.SEALContext(pr["n"], pr["q"], T33)
    dctx = fhe.SEALContext(pr["n"], pr["q"], T33, switches={"FHE_PLANEMAP_DIRECT": "1"})
    ev, dev = fhe.Evaluator(ctx), fhe.Evaluator(dctx)
    ct_bytes = 2 * ctx.k * ctx.n * 8
    ct = ctx.random_ct(1, SIDE * SIDE, seed=fhe.SEED)
    for case in cases:
        plans = {("w%d" % w): (ev, passes_of(case, ctx, w)) for w in (16, 32, 64)}
        plans["direct"] = (dev, passes_of(case, dctx, 0))
        bufs = [ctx.empty(1, pl.n_out) for pl in plans["w16"][1]]

        def runner(e, passes):
            def run():
                x = ct
                for pl, buf in zip(passes, bufs):
                    x = e.plane_map(pl.plan, x, out=buf)
                return x
            return run
        fns = {name: runner(e, passes) for name, (e, passes) in plans.items()}
        fns["composed"] = composed_fn(ctx, ev, plans["w16"][1], ct)
        want = fns["direct"]().clone()
        for name, fn in fns.items():
            got = fn()
            assert torch.equal(got.reshape(want.shape), want), "%s differs from the direct kernel" % name
        per_pass = {}
        for i, pl in enumerate(plans["w16"][1]):                          # each pass alone, for the roofline share
            src = ct if i == 0 else bufs[i - 1]
            one = {name: (lambda e=e, p=passes[i], s=src, b=bufs[i]: e.plane_map(p.plan, s, out=b)) for name, (e, passes) in plans.items()}
            _, _, ms1, _ = measure(one)
            moved = (pl.n_in + pl.n_out) * ct_bytes
            used = len(set(int(t) for t, w in zip(pl.taps.reshape(-1), pl.weights.reshape(-1)) if w))
            per_pass["pass%d" % i] = {"n_in": pl.n_in, "n_out": pl.n_out, "T": int(pl.taps.shape[1]), "ms": ms1, "bytes_in_plus_out": moved,
                                      "share_of_hbm_roofline": {name: moved / v * 1e3 / HBM_PEAK for name, v in ms1.items()},
                                      "groups": {name: passes[i].plan.groups for name, (_, passes) in plans.items()},
                                      "source_reads_amplification": {name: passes[i].plan.source_reads / used for name, (_, passes) in plans.items()}}
        steps, rounds, ms, spread = measure(fns)
        last = plans["w16"][1][-1]
        best = min(("w16", "w32", "w64"), key=lambda k: ms[k])
        line = {"workload": "%s on one frame set of %dx%d position-packed planes, %s primes (n=%d k=%d), t=%d" % (case, SIDE, SIDE, preset, ctx.n, ctx.k, T33),
                "arith_path": L.fhe_arith_path(ctx.h), "rounds": ROUNDS, "steps": steps, "ms": ms, "ms_rounds": rounds, "spread": spread, "passes": per_pass,
                "fastest_window": best, "windowed_not_slower_than_direct": {k: ms[k] <= ms["direct"] for k in ("w16", "w32", "w64")},
                "ratio_composed_to_fused": {k: ms["composed"] / ms[k] for k in ("w16", "w32", "w64", "direct")},
                "fused_faster_than_composed": all(ms[k] < ms["composed"] for k in ("w16", "w32", "w64", "direct")),
                "output_pixels_per_s": {k: last.n_out * ctx.n / ms[k] * 1e3 for k in ms}, "ciphertext_bytes_per_pixel": ct_bytes / ctx.n}
        del fns, plans, bufs, want, got
        torch.cuda.empty_cache()
        if case == "resize":                                               # one ciphertext per pixel: Evaluator.resize_plain on one 64x64 image
            plan = circuits.resize_plan(SIDE, SIDE, SIDE // 2, SIDE // 2, weight_bits=8)
            tables = [fhe.WeightTable(ctx, p["values"]) for p in plan["passes"]]
            src = ct[0]
            out = ctx.empty((SIDE // 2) ** 2)
            fn = lambda: ev.resize_plain(plan, src, tables=tables, out=out)
            _, r, m, _ = measure({"resize_plain": fn})
            line["per_pixel_resize_plain"] = {"ms": m["resize_plain"], "ms_rounds": r["resize_plain"], "output_pixels_per_s": (SIDE // 2) ** 2 / m["resize_plain"] * 1e3,
                                              "ciphertext_bytes_per_pixel": ct_bytes}
            del tables, out
        if case == "box3":                                                 # slot-packed tiles and rotations: circuits.packed_filter2d, direct keys
            kg = fhe.KeyGenerator(ctx, seed=1)
            keys = kg.generate_galois_keys(30, elements=[fhe.galois_element(ctx.n, dy * SIDE + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx])
            cts = 8
            packed = ctx.random_ct(cts, seed=3)
            valid = int(circuits.packed_filter_valid_mask(ctx.n, SIDE, 3, 3).sum())
            fn = lambda: circuits.packed_filter2d(ev, keys, packed, SIDE, np.ones((3, 3), dtype=np.int64), 3, 3)
            _, r, m, _ = measure({"packed_filter2d": fn})
            line["rotations_packed_filter2d"] = {"ciphertexts": cts, "valid_pixels_per_ciphertext": valid, "ms": m["packed_filter2d"], "ms_rounds": r["packed_filter2d"],
                                                 "output_pixels_per_s": cts * valid / m["packed_filter2d"] * 1e3, "ciphertext_bytes_per_pixel": ct_bytes / ctx.n,
                                                 "noise": "eight key switches per output; plane_map has none"}
            del keys, packed
        torch.cuda.empty_cache()
        print(json.dumps(line), flush=True)
        lines.append(line)
    del ct
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    for line in lines:
        fh.write(json.dumps(line) + "\n")

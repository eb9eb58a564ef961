#!/usr/bin/env python3
"""Integer linear maps across slot-packed ciphertexts (csrc/packed.hip) on resident data, in one process, alternating:
  (a) fhe_block8x8_scalar with the default forward plan (circuits.packed_dct_plan: 8-bit DCT, 8-bit reciprocals of the luminance table) on
      `groups` groups of 64 size-2 ciphertexts at P4096 and P8192 (t = 4295294977), beside the op-by-op composition it replaces --
      Evaluator.multiply_plain with prepared one-coefficient plaintexts and Evaluator.add, each call on the `groups` ciphertexts of one
      position -- on the same batch; time, ratio, (bytes in + bytes out) / time, its share of the 8 TB/s HBM roofline
      and blocks/s = n * groups / time IN THE PACKED FIXED-POINT REPRESENTATION (not bench.py's metric: another circuit, another encoding);
  (b) fhe_channel_mix, 3 x 3 (circuits.packed_rgb_to_ycc) with bias, on the same batch sizes, likewise.
Adoption rule, written before measuring: the fused kernels ship only if they are faster than the composition in every case of (a) and (b).
Device events, two warm-up runs, three alternating rounds per variant of at least `window_s` each, the spread reported.  One JSON line per
case to stdout and to profiles/packed_bench.json.  Secondary measurement, not bench.py's.  `trace` as the first argument runs every fused
call five times and measures nothing (for a kernel trace).
Usage: bench_packed.py [parts=ab|trace] [groups=16] [window_s=1.0] [out=profiles/packed_bench.json]"""
import json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fhip_amd as fhe

arg = lambda i, d: sys.argv[i] if len(sys.argv) > i else d
parts, groups, window_s, out_path = arg(1, "ab"), int(arg(2, "16")), float(arg(3, "1.0")), arg(4, os.path.join(ROOT, "profiles", "packed_bench.json"))
ROUNDS = 3
T33 = 4295294977
HBM_PEAK = 8e12
L = fhe._lib.load()


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


def block_case(preset):
    pr = fhe.PRESETS[preset]
    ctx = fhe.SEALContext(pr["n"], pr["q"], T33)
    ev = fhe.Evaluator(ctx)
    plan = fhe.circuits.packed_dct_plan(ctx)
    ct = ctx.random_ct(groups, 64, seed=fhe.SEED)
    out = torch.empty_like(ct)
    by_pos = ct.transpose(0, 1).contiguous()                            # [64][groups]: one contiguous batch per position for the composition
    prep = {}

    def scal(a, w):
        w = int(w) % ctx.t
        if w not in prep:
            prep[w] = fhe.PreparedPlain(ctx, np.array([w], dtype=np.uint64))
        return ev.multiply_plain(a, prep[w])

    def wsum(terms):
        acc = None
        for w, a in terms:
            if int(w):
                term = scal(a, w)
                acc = term if acc is None else ev.add(acc, term, out=acc)
        return acc

    def composed():
        Lm, Rm, post = plan.L, plan.R, plan.post
        cols = [[wsum([(Lm[u][i], by_pos[8 * i + y]) for i in range(8)]) for y in range(8)] for u in range(8)]
        return [scal(wsum([(Rm[v][j], cols[u][j]) for j in range(8)]), post[u][v]) for u in range(8) for v in range(8)]

    fused = lambda: ev.block8x8_scalar(plan.plan, ct, out=out)
    fused()
    assert torch.equal(out.transpose(0, 1), torch.stack(composed())), "fused and composed differ"
    return ctx, {"fused": fused, "composed": composed}, ct


def mix_case(preset):
    pr = fhe.PRESETS[preset]
    ctx = fhe.SEALContext(pr["n"], pr["q"], T33)
    ev = fhe.Evaluator(ctx)
    M, bias = fhe.circuits.packed_rgb_to_ycc(8), [-(128 << 8), 77, -5]
    planes = ctx.random_ct(3, groups * 64, seed=fhe.SEED + 2)
    out = torch.empty_like(planes)
    prep = {int(w) % ctx.t: fhe.PreparedPlain(ctx, np.array([int(w) % ctx.t], dtype=np.uint64)) for w in M.reshape(-1)}
    bp = [np.array([b % ctx.t], dtype=np.uint64) for b in bias]

    def composed():
        res = []
        for i in range(3):
            acc = None
            for j in range(3):
                term = ev.multiply_plain(planes[j], prep[int(M[i][j]) % ctx.t])
                acc = term if acc is None else ev.add(acc, term, out=acc)
            res.append(ev.add_plain(acc, bp[i]))
        return res

    fused = lambda: ev.channel_mix(M, planes, bias=bias, out=out)
    fused()
    assert torch.equal(out, torch.stack(composed())), "fused and composed differ"
    return ctx, {"fused": fused, "composed": composed}, planes


lines = []
if parts == "trace":
    for preset in ("P4096", "P8192"):
        for case in (block_case, mix_case):
            ctx, fns, _ = case(preset)
            for _ in range(5):
                fns["fused"]()
            torch.cuda.synchronize()
            del fns
            torch.cuda.empty_cache()
    sys.exit(0)

for part, case, what in (("a", block_case, "fhe_block8x8_scalar, default forward plan (packed_dct_plan 8, 8)"), ("b", mix_case, "fhe_channel_mix 3x3 with bias")):
    if part not in parts:
        continue
    for preset in ("P4096", "P8192"):
        ctx, fns, data = case(preset)
        steps, rounds, ms, spread = measure(fns)
        moved = 2 * data.numel() * 8
        line = {"workload": "%s, %d groups of 64 size-2 ciphertexts%s, %s primes (n=%d k=%d), t=%d" % (what, groups, " per plane" if part == "b" else "", preset, ctx.n, ctx.k, T33),
                "arith_path": L.fhe_arith_path(ctx.h), "rounds": ROUNDS, "steps": steps, "ms": ms, "ms_rounds": rounds, "spread": spread,
                "ratio_composed_to_fused": ms["composed"] / ms["fused"], "bytes_in_plus_out": moved, "fused_bytes_per_s": moved / ms["fused"] * 1e3,
                "fused_share_of_hbm_roofline": moved / ms["fused"] * 1e3 / HBM_PEAK, "fused_faster_than_composed": ms["fused"] < ms["composed"]}
        if part == "a":
            line["packed_fixed_point_blocks_per_s"] = ctx.n * groups / ms["fused"] * 1e3
        print(json.dumps(line), flush=True)
        lines.append(line)
        del fns, data
        torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    for line in lines:
        fh.write(json.dumps(line) + "\n")

#!/usr/bin/env python3
"""Evaluator.resize_plain (fhe_remap) against the op-by-op composition and the ct x ct resize, on resident data, in one process, alternating:
  (a) Evaluator.resize_plain in circuits.resize_plan's default pass order: two fhe_remap passes, the intermediate in NTT form (one forward and one inverse transform per ciphertext);
  (b) the same two passes op by op through the batched Evaluator, as a host had them before fhe_remap: per slot and per distinct
      weight of that slot a gather of the sources, Evaluator.multiply_plain, a scatter of the terms, and Evaluator.add per slot;
  (c) circuits.resize_bicubic_shared (the reference's ResizeImage / SampleBicubic with encrypted offsets, size-6 outputs) for the first
      shape -- NOT the same ciphertexts: it is the circuit (a) replaces when the geometry is public.
One channel, Catmull-Rom, 128x128 -> 64x64 and 64x64 -> 128x128, presets P8192 and P4096; device events, two warm-up runs, three
alternating rounds per variant of at least a second each.  One JSON line per case to stdout and to profiles/resample_bench.json: ms
(median of the rounds), output pixels / s, fhe_remap_path, the ratio b / a, the run-to-run spread of (a), (a) with the sources already
transformed (src_is_ntt: the share of the forward pass), (a) in the other pass order, and (c).  Secondary measurement, not bench.py's.
Usage: bench_resample.py [presets=P8192,P4096] [shapes=128x64,64x128] [kernel=catmull_rom] [window_s=1.0] [out=profiles/resample_bench.json]"""
import json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fhip_amd as fhe

arg = lambda i, d: sys.argv[i] if len(sys.argv) > i else d
presets = arg(1, "P8192,P4096").split(",")
shapes = [tuple(int(v) for v in s.split("x")) for s in arg(2, "128x64,64x128").split(",")]
kernel, window_s, out_path = arg(3, "catmull_rom"), float(arg(4, "1.0")), arg(5, os.path.join(ROOT, "profiles", "resample_bench.json"))
ROUNDS = 3


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


def stepwise_pass(ctx, ev, enc, p):
    """one remap pass as batched Evaluator calls: [(slot, [(plain, source indices, output indices)])]"""
    slots = []
    for s in range(p["taps"].shape[1]):
        groups = []
        for wid in np.unique(p["wids"][:, s]):
            if wid == fhe.REMAP_SKIP:
                continue
            plain = enc.encode(float(p["values"][wid]))
            if not np.any(plain):
                continue
            outs = np.flatnonzero(p["wids"][:, s] == wid)
            groups.append((fhe.PreparedPlain(ctx, plain), torch.as_tensor(p["taps"][outs, s].astype("int64"), device=ctx.device),
                           torch.as_tensor(outs.astype("int64"), device=ctx.device), len(outs) == p["count"]))
        slots.append(groups)
    return slots


lines = []
for preset in presets:
    ctx = fhe.SEALContext.preset(preset)
    ev, enc = fhe.Evaluator(ctx), fhe.FractionalEncoder(ctx)
    for case, (side, dst) in enumerate(shapes):
        src = ctx.random_ct(side * side, seed=fhe.SEED)
        src_ntt = ev.ntt_forward(src)
        plan = fhe.resize_plan(side, side, dst, dst, kernel)
        other = fhe.resize_plan(side, side, dst, dst, kernel, order="vh" if plan["order"] == "hv" else "hv")
        tables = [fhe.WeightTable(ctx, p["values"]) for p in plan["passes"]]
        tables_other = [fhe.WeightTable(ctx, p["values"]) for p in other["passes"]]
        count = dst * dst
        o = ctx.empty(count)
        n_mid = plan["passes"][0]["count"]
        work = max(n_mid, count)
        mid, g, t = ctx.empty(n_mid), ctx.empty(work), ctx.empty(work)
        a2 = ctx.empty(count)
        passes = [stepwise_pass(ctx, ev, enc, p) for p in plan["passes"]]

        def fused():
            ev.resize_plain(plan, src, tables=tables, out=o)

        def fused_resident():
            ev.resize_plain(plan, src_ntt, tables=tables, out=o, src_is_ntt=True)

        def fused_other_order():
            ev.resize_plain(other, src, tables=tables_other, out=o)

        def run_pass(slots, source, acc, n_out, gather_only=False):
            first = True
            for groups in slots:
                if not groups:
                    continue
                dst_t = acc if first else t[:n_out]
                for pl, si, oi, whole in groups:
                    gg = g[:si.numel()]
                    torch.index_select(source, 0, si, out=gg)
                    if gather_only:
                        continue
                    if whole:
                        ev.multiply_plain(gg, pl, out=dst_t)
                    else:
                        dst_t.index_copy_(0, oi, ev.multiply_plain(gg, pl, out=gg))
                if not first and not gather_only:
                    ev.add(acc, t[:n_out], out=acc)
                first = False

        def op_by_op():
            run_pass(passes[0], src, mid, n_mid)
            run_pass(passes[1], mid, a2, count)

        def gathers():
            run_pass(passes[0], src, mid, n_mid, gather_only=True)
            run_pass(passes[1], mid, a2, count, gather_only=True)

        op_by_op()
        fused()
        assert torch.equal(o, a2), "fused and op-by-op results differ"
        fused_other_order()
        assert torch.equal(o, a2), "the two pass orders differ"
        sa, sb = steps_for(fused), steps_for(op_by_op)
        ra, rb = [], []
        for _ in range(ROUNDS):
            ra.append(window(fused, sa))
            rb.append(window(op_by_op, sb))
        ms_a, ms_b = statistics.median(ra), statistics.median(rb)
        ms_res = window(fused_resident, steps_for(fused_resident))
        ms_other = window(fused_other_order, steps_for(fused_other_order))
        ms_g = window(gathers, steps_for(gathers))
        line = {"workload": "resize_plain %s %dx%d -> %dx%d, 1 channel, %s (n=%d k=%d)" % (kernel, side, side, dst, dst, preset, ctx.n, ctx.k),
                "remap_path": fhe._lib.load().fhe_remap_path(ctx.h), "order": plan["order"], "taps": [int(p["taps"].shape[1]) for p in plan["passes"]],
                "distinct_weights": [tb.distinct for tb in tables], "steps": sa, "baseline_steps": sb, "rounds": ROUNDS,
                "ms": ms_a, "pixels_per_s": count / ms_a * 1e3, "spread": (max(ra) - min(ra)) / ms_a, "ms_rounds": ra,
                "baseline_ms": ms_b, "baseline_ms_rounds": rb, "baseline_gather_ms": ms_g, "ratio": ms_b / ms_a,
                "ratio_without_gather": (ms_b - ms_g) / ms_a, "ms_src_is_ntt": ms_res, "forward_share": 1.0 - ms_res / ms_a,
                "ms_other_pass_order": ms_other}
        if case == 0 and dst >= 2:
            pc = fhe.circuits.PlainCache(ctx)
            xf, yf = ctx.random_ct(dst, seed=11), ctx.random_ct(dst, seed=12)

            def ctct():
                fhe.circuits.resize_bicubic_shared(ev, pc, src, side, side, dst, dst, xf, yf, consume=lambda first, band: None)

            rc = [window(ctct, steps_for(ctct)) for _ in range(ROUNDS)]
            line.update(ctct_shared_ms=statistics.median(rc), ctct_shared_ms_rounds=rc, ratio_ctct=statistics.median(rc) / ms_a)
            del pc, xf, yf
        print(json.dumps(line), flush=True)
        lines.append(line)
        del src, src_ntt, o, mid, g, t, a2, passes, tables, tables_other
        torch.cuda.empty_cache()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    for line in lines:
        fh.write(json.dumps(line) + "\n")

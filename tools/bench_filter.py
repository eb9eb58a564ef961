#!/usr/bin/env python3
"""fhe_filter2d against the op-by-op composition, on resident data, in one process, alternating:
  (a) Evaluator.filter2d (one forward transform per source, gather + lazy sums + inverse transform per output);
  (b) per non-zero tap: gather of the tap's sources, Evaluator.multiply_plain, Evaluator.add -- the batched calls a host had before.
      The gather is what lets (b) run as batched calls at all; it is timed on its own too, so the ratio is given with and without it.
Single channel, 64x64 and 128x128, kernels box3 and gauss5, presets P8192 and P4096; device events, two warm-up runs, three
alternating rounds per variant of at least a second each.  One JSON line per case to stdout and to profiles/filter_bench.json:
ms (median of the rounds), output pixels / s, fhe_filter_path, algorithmic bytes (sources read once + outputs written once), the
ratio b / a, the run-to-run spread of (a), (a) with the sources already transformed (src_is_ntt: the share of the forward pass),
and (a) with FHE_FILTER_XCD=0 (workgroups in plain order).  Secondary measurement, not bench.py's.
Usage: bench_filter.py [presets=P8192,P4096] [sizes=64,128] [kernels=box3,gauss5] [window_s=1.0] [out=profiles/filter_bench.json]"""
import json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fhip_amd as fhe

arg = lambda i, d: sys.argv[i] if len(sys.argv) > i else d
presets, sizes, kernels = arg(1, "P8192,P4096").split(","), [int(x) for x in arg(2, "64,128").split(",")], arg(3, "box3,gauss5").split(",")
window_s, out_path = float(arg(4, "1.0")), arg(5, os.path.join(ROOT, "profiles", "filter_bench.json"))
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


lines = []
for preset in presets:
    ctx = fhe.SEALContext.preset(preset)
    plain_order = fhe.SEALContext.preset(preset, switches={"FHE_FILTER_XCD": "0"})
    ev, ev_plain, enc = fhe.Evaluator(ctx), fhe.Evaluator(plain_order), fhe.FractionalEncoder(ctx)
    for side in sizes:
        src = ctx.random_ct(side * side, seed=fhe.SEED)
        src_ntt = ev.ntt_forward(src)
        out, gathered, term, acc = (torch.empty_like(src) for _ in range(4))
        for name in kernels:
            f = fhe.FILTERS[name]
            w = f["weights"]
            kh, kw = w.shape
            taps, dw, dh = fhe.filter_tap_plan(side, side, kw, kh, anchor=f["anchor"], stride=f["stride"])
            plan, plan_plain = fhe.FilterPlan(ctx, w), fhe.FilterPlan(plain_order, w)
            live = [p for p in range(kw * kh) if w.reshape(-1)[p] != 0.0]
            idx = [torch.as_tensor(taps[:, p].astype("int64"), device=ctx.device) for p in live]
            plains = [fhe.PreparedPlain(ctx, enc.encode(float(w.reshape(-1)[p]))) for p in live]
            count = taps.shape[0]
            o, g, t, a = out[:count], gathered[:count], term[:count], acc[:count]

            def fused():
                ev.filter2d(plan, src, taps, out=o)

            def fused_resident():
                ev.filter2d(plan, src_ntt, taps, out=o, src_is_ntt=True)

            def fused_plain_order():
                ev_plain.filter2d(plan_plain, src, taps, out=o)

            def gathers():
                for i in idx:
                    torch.index_select(src, 0, i, out=g)

            def op_by_op():
                for j, (i, pl) in enumerate(zip(idx, plains)):
                    torch.index_select(src, 0, i, out=g)
                    if j == 0:
                        ev.multiply_plain(g, pl, out=a)
                    else:
                        ev.multiply_plain(g, pl, out=t)
                        ev.add(a, t, out=a)

            op_by_op()
            ref = a.clone()
            fused()
            assert torch.equal(o, ref), "fused and op-by-op results differ"
            sa, sb = steps_for(fused), steps_for(op_by_op)
            ra, rb = [], []
            for _ in range(ROUNDS):
                ra.append(window(fused, sa))
                rb.append(window(op_by_op, sb))
            ms_a, ms_b = statistics.median(ra), statistics.median(rb)
            ms_res = window(fused_resident, steps_for(fused_resident))
            ms_plain = window(fused_plain_order, steps_for(fused_plain_order))
            ms_g = window(gathers, steps_for(gathers))
            by = (src.numel() + o.numel()) * 8
            line = {"workload": "filter2d %s %dx%d -> %dx%d, 1 channel, %s (n=%d k=%d)" % (name, side, side, dw, dh, preset, ctx.n, ctx.k),
                    "filter_path": fhe._lib.load().fhe_filter_path(ctx.h), "taps": plan.taps, "steps": sa, "baseline_steps": sb, "rounds": ROUNDS,
                    "ms": ms_a, "pixels_per_s": count / ms_a * 1e3, "algorithmic_bytes": by, "algorithmic_GB_per_s": by / ms_a / 1e6,
                    "spread": (max(ra) - min(ra)) / ms_a, "ms_rounds": ra,
                    "baseline_ms": ms_b, "baseline_ms_rounds": rb, "baseline_gather_ms": ms_g, "ratio": ms_b / ms_a,
                    "ratio_without_gather": (ms_b - ms_g) / ms_a, "ms_src_is_ntt": ms_res, "forward_share": 1.0 - ms_res / ms_a,
                    "ms_plain_workgroup_order": ms_plain}
            print(json.dumps(line), flush=True)
            lines.append(line)
        del src, src_ntt, out, gathered, term, acc
        torch.cuda.empty_cache()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    for line in lines:
        fh.write(json.dumps(line) + "\n")

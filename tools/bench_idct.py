#!/usr/bin/env python3
"""Throughput of fhe_idct8x8_dequant (dequantisation + 8x8 inverse DCT, the inverse of bench.py's fused DCT + quant) on
resident ciphertexts at the headline shape: blocks/s and algorithmic GB/s (64 size-2 ciphertexts in + 64 out per block,
bench.py's algorithmic bytes per block).  The forward pair on the same blocks is measured beside it for the ratio.
Secondary measurement, not bench.py's.  Usage: bench_idct.py [blocks=1024] [preset=P4096] [steps=10]"""
import json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fhip_amd as fhe
nb = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
preset = sys.argv[2] if len(sys.argv) > 2 else "P4096"
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
ctx = fhe.SEALContext.preset(preset)
ev = fhe.Evaluator(ctx)
blocks = ctx.random_ct(nb, 64, seed=fhe.SEED)
out = torch.empty_like(blocks)
iplan, fplan = fhe.IdctPlan(ctx, fhe.YQT), fhe.DctPlan(ctx, fhe.YQT)


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


ms_inv = timed(lambda: ev.idct8x8_dequant(iplan, blocks, out=out))
ms_fwd = timed(lambda: ev.dct8x8_quant(fplan, blocks, out=out))
by = 128 * 2 * ctx.k * ctx.n * 8
print(json.dumps({"workload": "idct8x8_dequant (YQT), %s (n=%d k=%d)" % (preset, ctx.n, ctx.k), "blocks": nb, "steps": steps,
                  "idct_path": "fused: k_idct_rows + k_idct_cols" if fhe._lib.load().fhe_dct_path(ctx.h) == 1 else
                  "general: k_ntt_fwd + %s + k_ntt_inv" % ("k_idct_lines_pm x2" if fhe._lib.load().fhe_arith_path(ctx.h) & 3 == 1 else "k_idct_slots"),
                  "ms": ms_inv, "blocks_per_s": nb / ms_inv * 1e3, "algorithmic_bytes_per_block": by,
                  "algorithmic_GB_per_s": nb * by / ms_inv / 1e6, "forward_dct_path": fhe._lib.load().fhe_dct_path(ctx.h),
                  "forward_ms": ms_fwd, "forward_blocks_per_s": nb / ms_fwd * 1e3, "inverse_over_forward": ms_fwd / ms_inv}))

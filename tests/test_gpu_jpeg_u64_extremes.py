"""GPU: the integer JPEG kernels at their exits and arithmetic edges -- k_idct_lines_pm<false / true> and k_idct_slots, k_dct_lines_pm<false /
true> and k_dct_slots, k_rgb_ntt_pm + k_rgb_combine_pm on both pseudo-Mersenne classes, k_rgb2ycc and k_ycc2rgb.  tests/jpeg_u64_craft.py
builds the inputs and restates the kernels as value models; tests/test_jpeg_u64_craft_cpu.py proves in those models what the inputs reach
(every canon_pm exit takes and skips its subtraction thousands of times and meets fold_pm == q; the canonical kernels meet sums of exactly q,
differences of exactly 0 and (q-1) + (q-1); each wrong variant changes a model's output).  Here the same blocks go through the kernels.

Bases (n = 1024, t = 2^14): SEAL's 54/55-bit primes (class A; the line kernels -- the inverse by default, the forward direction with
FHE_DCT_FORCE_U64=1), the same with FHE_NTT_NOPM=1 (the slot and one-launch kernels), a 58-bit base (class B: colour on PmB, DCT on the slot
kernels), a 61-bit base (Shoup everywhere) and the class-A base with the widest delta fhe_build_base admits.  The colour kernels are
templated on the transform size and run once more at n = 8192.

Families: Z constant blocks (all-zero among them), E prescribed outputs at the exits, T the ties of slot_craft's F1 - F3, G one random
block; C the colour blocks.  The words a line or slot kernel stores are not returned: an inverse transform runs on them.  A stored q + r
changes a ciphertext only where the transform's first butterfly X - Y + q meets X < r, so E holds such pairs (X = 0 beside r = 1 .. delta - 1
at the two slots w and -w of output (0, 0)): a line kernel without its exit subtraction fails E here, which the library built that way
showed; a stored q (`>` for `>=`) can show in no ciphertext and is caught in the models' stored words only.  Per base and direction ONE call on the whole batch: bit for bit the CPU oracle, fhe_count_unreduced == 0, the
inverse DCT in place equals out of place, and on SEAL's primes the default context gives the same bytes as the FHE_NTT_NOPM=1 context."""
import ctypes as C

import numpy as np
import pytest

import idct_oracle as io
import jpeg_u64_craft as jc

pytestmark = pytest.mark.gpu

DCT_FAMILIES = ("Z", "E", "T", "G")
CASES = [(b, jc.N, w) for b in jc.bases() for w in ("inv", "fwd", "ycc", "rgb")] + [(b, 8192, w) for b in jc.bases(8192) for w in ("ycc", "rgb")]


def _grouped(cases):
    """cases that share (n, primes) next to each other: their crafted batches are built once"""
    groups = {}
    for b, n, w in cases:
        groups.setdefault((n, tuple(jc.bases(n)[b][1])), []).append((b, n, w))
    return [c for cs in groups.values() for c in cs]


def _family(name):
    return "G" if name == "random" else name.split("-")[0]


@pytest.fixture(scope="module")
def crafted(oracle_mod):
    """(n, primes, what) -> the crafted batch with the oracle's outputs; the slot model of one (n, primes) is kept at a time"""
    state = {"key": None, "sm": None, "col": None, "data": {}}

    def get(n, q, what):
        if state["key"] != (n, tuple(q)):
            state.update(key=(n, tuple(q)), sm=jc.slot_model(oracle_mod, n, q), col=None, data={})
        sm = state["sm"]
        if what not in state["data"]:
            if what in ("inv", "fwd"):
                names, blocks, G, ok = jc.craft_batch(sm, what)
                ops = io.OracleOps(sm.orc)
                want = np.stack([ops.idct_block(b, oracle_mod.YQT) if what == "inv" else sm.orc.dct_quant(b, oracle_mod.YQT) for b in blocks])
                state["data"][what] = dict(names=names, blocks=blocks, want=want, G=G, ok=ok, sm=sm)
            else:
                state["col"] = state["col"] or jc.Colour(sm)
                pres = jc.prescribed_pixels(n)
                if what == "ycc":
                    blk = jc.craft_ycc(state["col"], pres)[0]
                    want = io.OracleOps(sm.orc).ycc_to_rgb_block(blk)
                else:
                    blk = jc.craft_rgb(state["col"], pres)[0]
                    want = np.empty_like(blk)
                    for p in range(64):
                        want[0, p], want[1, p], want[2, p] = sm.orc.rgb_to_ycc(blk[0, p], blk[1, p], blk[2, p])
                state["data"][what] = dict(names=["C"], blocks=blk[None], want=want[None], sm=sm)
        return state["data"][what]
    return get


def _unreduced(fhe, ctx, t):
    import torch
    cnt = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    fhe._lib.call("fhe_count_unreduced", ctx.h, C.c_void_p(t.data_ptr()), t.numel() // ctx.n // ctx.k, C.c_void_p(cnt.data_ptr()), None)
    return int(cnt.cpu()[0])


def _context(fhe, n, q, switches, dct_path=None):
    """the context, with the path the library reports asserted against the rule restated in dct_u64_craft.classify"""
    ctx = fhe.SEALContext(n, q, jc.T_PLAIN, switches=dict(switches) or None)
    path, arith = jc.expected_paths(n, q, switches)
    assert fhe._lib.call("fhe_arith_path", ctx.h) & 3 == arith, "fhe_arith_path"
    assert fhe._lib.call("fhe_dct_path", ctx.h) == path, "fhe_dct_path"
    if dct_path is not None:
        assert path == dct_path, "the DCT must take the general path: forward transform, line or slot kernels, inverse transform"
    return ctx, arith


def _call(fhe, ctx, what, dev):
    ev = fhe.Evaluator(ctx)
    if what == "inv":
        return ev.idct8x8_dequant(fhe.IdctPlan(ctx, fhe.YQT), dev)
    if what == "fwd":
        return ev.dct8x8_quant(fhe.DctPlan(ctx, fhe.YQT), dev)
    out = dev.clone()
    return ev.ycc_to_rgb_blocks(out) if what == "ycc" else ev.rgb_to_ycc_blocks(out)


@pytest.fixture(scope="module")
def runs(fhe, crafted):
    """(base, n, what) -> one call on the whole crafted batch and what was compared; the last run is kept"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    state = {"key": None, "run": None}

    def get(base, n, what):
        if state["key"] == (base, n, what):
            return state["run"]
        _, q, sw, cls = jc.bases(n)[base]
        data = crafted(n, q, what)
        switches = dict(sw, **jc.FORCE_U64) if what == "fwd" else dict(sw)
        ctx, arith = _context(fhe, n, q, switches, 0 if what in ("inv", "fwd") else None)
        assert arith == {"A": 1, "B": 2, None: 0}[cls]
        dev = fhe.to_device(data["blocks"], ctx.device)
        before = dev.clone()
        got = _call(fhe, ctx, what, dev)
        torch.cuda.synchronize()
        run = dict(data, got=fhe.to_host(got), unreduced=_unreduced(fhe, ctx, got), untouched=bool(torch.equal(dev, before)), same_in_place=None, same_nopm=None)
        if what == "inv":
            again = dev.clone()
            fhe.Evaluator(ctx).idct8x8_dequant(fhe.IdctPlan(ctx, fhe.YQT), again, out=again)
            run["same_in_place"] = bool(torch.equal(again, got))
        if base == "pmA":                                    # SEAL's primes: the pseudo-Mersenne kernels against the Shoup ones
            other, _ = _context(fhe, n, q, dict(switches, **jc.NOPM))
            run["same_nopm"] = bool(torch.equal(_call(fhe, other, what, dev), got))
        torch.cuda.synchronize()
        state["key"], state["run"] = (base, n, what), run
        return run
    return get


@pytest.mark.parametrize("base,n,what,family", [(b, n, w, f) for b, n, w in _grouped(CASES) for f in (DCT_FAMILIES if w in ("inv", "fwd") else ("C",))])
def test_crafted_family_is_bit_for_bit_the_oracle(runs, base, n, what, family):
    """the first family of a batch also carries the whole-batch checks: no output word at or above its prime, the input unchanged, the
    inverse DCT in place equals out of place, the default context equals the FHE_NTT_NOPM=1 context on SEAL's primes"""
    run = runs(base, n, what)
    names, got, want = run["names"], run["got"], run["want"]
    if family in ("Z", "C"):
        assert run["unreduced"] == 0
        assert run["untouched"] or what in ("ycc", "rgb")
        assert run["same_in_place"] in (None, True) and (what == "inv") == (run["same_in_place"] is not None)
        assert run["same_nopm"] in (None, True) and (base == "pmA") == (run["same_nopm"] is not None)
        assert len(names) <= 12
    mine = [b for b, nm in enumerate(names) if _family(nm) == family]
    assert mine
    for b in mine:
        assert np.array_equal(got[b], want[b]), names[b]
    if family == "Z":
        assert not got[names.index("Z-zero")].any()
    if family == "E":                                        # the prescribed residues, at the slots, where the solver found them
        sm, e = run["sm"], names.index("E")
        slots = jc.to_slots(sm, got[e]).reshape(8, 8, 2, sm.k, sm.n)
        assert np.array_equal(np.where(run["ok"], slots, 0), np.where(run["ok"], run["G"], 0))

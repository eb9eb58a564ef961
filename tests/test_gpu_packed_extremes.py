"""GPU: the packed integer maps at their arithmetic edges -- fhe_block8x8_scalar, fhe_channel_mix (csrc/packed.hip) and fhe_plane_map
(csrc/planemap.hip) on the operands of tests/packed_craft.py, bit for bit the direct specification (tests/packed_oracle.py,
tests/planemap_oracle.py; never the model).  tests/test_packed_craft_cpu.py proves in the integer model what the operands reach: every
excess and every canon() interval the reach table allows, sums of eight terms at the largest excess, outputs exactly 0
and q - 1 in the highest interval their last product can return, eight canonical products of q - 1 in one sum -- and that a canon() with
one subtraction, a ninth term, a 16-term plane-map chunk, a plane map without its per-chunk reduction and lazy sums beyond the gate each
leave the specification on them.

Bases, all at n = 1024 with the 33-bit t (and the 54/55-bit primes once with t = 65537, where (t - 1) / 2 is the scalar limit):

  base    primes                                        arithmetic (packed_arith.h lazy_ok)       families
  Q3      36/37 bit                                     lazy                                      S, X
  Q4      54/55 bit                                     lazy                                      S, X
  Q58     the two largest 58-bit primes                 lazy (the only base with excess 3)        S, X
  shoup   Q4 with FHE_NTT_NOPM=1                        canonical, small primes                   C
  Q60     the largest 60-bit prime and a 55-bit one     canonical: lazy sums would wrap           C, and S as a lazy kernel would need it
  Q61     the largest 61-bit prime and a 55-bit one     canonical at its own bound (8 q - 8)      C, and S as a lazy kernel would need it

The kernel instantiations and the cases that run them:

  k_block8x8<true,  true >     test_block8x8[Q3 | Q4 | Q58 - pre - *], [Q58 - pre - post - size 3], [Q4 - t = 65537]
  k_block8x8<true,  false>     test_block8x8[Q3 | Q4 | Q58 - nopre - *]
  k_block8x8<false, true >     test_block8x8[shoup | Q60 | Q61 - pre - *], test_the_gate_from_its_far_side[Q60 | Q61 - block]
  k_block8x8<false, false>     test_block8x8[shoup | Q60 | Q61 - nopre - *]
  k_channel_mix<true>          test_channel_mix[Q3 | Q4 | Q58 - m], [Q4 - t = 65537]
  k_channel_mix<false>         test_channel_mix[shoup | Q60 | Q61 - m], test_the_gate_from_its_far_side[Q60 | Q61 - mix]
  k_plane_map<true,  16>       test_plane_map[Q3 | Q4 | Q58]: the plan with window 16 (its groups of at most 16 sources)
  k_plane_map<true,  32>       test_plane_map[Q3 | Q4 | Q58]: the plans with windows 16 and 32 (groups of 17 .. 32 sources)
  k_plane_map<true,  64>       test_plane_map[Q3 | Q4 | Q58]: every windowed plan (the 64-source outputs)
  k_plane_map<false, 16 | 32 | 64>   the same plans of test_plane_map[shoup | Q60 | Q61], test_the_gate_from_its_far_side[Q60 | Q61 - pm]
  k_plane_map_direct<true>     test_plane_map[Q3 | Q4 | Q58]: the default plan and the FHE_PLANEMAP_DIRECT=1 context
  k_plane_map_direct<false>    test_plane_map[shoup | Q60 | Q61]: the same two

(* = with and without post: the last product is post[u][v] or the pair for 1.)  Every call also asserts fhe_count_unreduced == 0, the
input unchanged and, where the entry point allows it, in place == out of place."""
import numpy as np
import pytest

import packed_craft as pc
import packed_oracle as po
import planemap_oracle as pmo
from test_gpu_galois import _unreduced

pytestmark = pytest.mark.gpu

BASES = pc.bases()
_cache = {}


def _ctx(fhe, base, t=po.T33, direct=False):
    if (base, t, direct) not in _cache:
        q, sw = BASES[base]
        sw = dict(sw, FHE_PLANEMAP_DIRECT="1") if direct else dict(sw)
        ctx = fhe.SEALContext(pc.N, q, t, switches=sw or None)
        _cache[(base, t, direct)] = (ctx, fhe.Evaluator(ctx))
    return _cache[(base, t, direct)]


def _report(fhe, ctx, base, kind, case, what):
    big, hist = pc.describe(kind, case)
    if BASES[base][1].get("FHE_NTT_NOPM"):                                 # fhe_arith_path reports the transforms' arithmetic, not the packed maps'; it does
        assert fhe._lib.load().fhe_arith_path(ctx.h) == 0, "FHE_NTT_NOPM=1 did not reach the context: lazy_ok would hold"      # show whether the switch the gate reads arrived
    print("\n[%s %s %s] arith path %d, widest prime %d bits, restated gate: %s; the model's largest sum %d q; words per canon() interval %s"
          % (kind, base, what, fhe._lib.load().fhe_arith_path(ctx.h), max(p.bit_length() for p in ctx.q), "lazy" if pc.gate(*BASES[base]) else "canonical", big, hist))


def _checked(fhe, ctx, dev, host, out, want, what):
    import torch
    assert np.array_equal(fhe.to_host(out), want), what
    assert _unreduced(fhe, ctx, out) == 0, what
    assert torch.equal(dev, fhe.to_device(host, ctx.device)), "the input was written"


def _block(fhe, base, case, t, what):
    import torch
    ctx, ev = _ctx(fhe, base, t)
    assert list(ctx.q) == case.A.q
    _report(fhe, ctx, base, "block", case, what)
    host, want = pc.to_ct(case.X, case.size)[None], pc.spec_block(case)[None]
    plan = fhe.Block8x8Plan(ctx, *case.plan)
    dev = fhe.to_device(host, ctx.device)
    out = ev.block8x8_scalar(plan, dev)
    _checked(fhe, ctx, dev, host, out, want, what)
    buf = dev.clone()
    assert ev.block8x8_scalar(plan, buf, out=buf) is buf and torch.equal(buf, out), "in place differs"


BLOCK = [(b, pre, post, 2, po.T33) for b in BASES for pre in (True, False) for post in (True, False)] + [("Q58", True, True, 3, po.T33), ("Q4", True, True, 2, pc.T_SMALL)]


@pytest.mark.parametrize("base,pre,post,size,t", BLOCK, ids=["%s-%s-%s-size%d-t%d" % (b, "pre" if p0 else "nopre", "post" if p1 else "nopost", s, t.bit_length()) for b, p0, p1, s, t in BLOCK])
def test_block8x8(fhe, base, pre, post, size, t):
    """one group of 64 ciphertexts: families S and X on the lazy bases, C on the canonical ones"""
    q, sw = BASES[base]
    _block(fhe, base, pc.craft("block", q, pc.gate(q, sw), (pre, post), size=size, t=t), t, "pre=%d post=%d size=%d" % (pre, post, size))


def _mix(fhe, base, case, t, what, aimed=True):
    import torch
    ctx, ev = _ctx(fhe, base, t)
    _report(fhe, ctx, base, "mix", case, what)
    M = case.plan
    m = M.shape[0]
    lim = po.scalar_limit(t)
    host = pc.to_ct(case.X, case.size)[:, None]                            # [8, 1, size, k, n]
    bias = np.array([-lim, 5, lim, 0, 1, -1, 77, -(lim // 3)][:m], dtype=np.int64)
    assert bias[pc.O0] != 0
    dev = fhe.to_device(host, ctx.device)
    for b in (None, bias):
        want = pc.spec_mix(case, b, t)[:, None]
        if b is None:
            plain = want
            assert not aimed or all(int(want[pc.O0, 0, 0, i, 0]) == p - 1 for i, p in enumerate(ctx.q)), "coefficient 0 of c0 of output O0 is crafted to q - 1"
        else:                                                              # (q - 1) + constant wraps past q on every prime
            add = po.add_plain_constant(ctx.q, t, int(bias[pc.O0]) % t)
            assert not aimed or all(0 < a and int(want[pc.O0, 0, 0, i, 0]) == a - 1 for i, a in enumerate(add))
            assert np.array_equal(want[:, :, 1:], plain[:, :, 1:]) and np.array_equal(want[..., 1:], plain[..., 1:])
        out = ev.channel_mix(M, dev, bias=b)
        _checked(fhe, ctx, dev, host, out, want, (what, b is None))
        if m == 8:
            buf = dev.clone()
            assert ev.channel_mix(M, buf, bias=b, out=buf) is buf and torch.equal(buf, out), "in place differs"


MIX = [(b, m, po.T33) for b in BASES for m in (8, 3)] + [("Q4", 8, pc.T_SMALL)]


@pytest.mark.parametrize("base,m,t", MIX, ids=["%s-m%d-t%d" % (b, m, t.bit_length()) for b, m, t in MIX])
def test_channel_mix(fhe, base, m, t):
    """(c, m) = (8, 8) and (8, 3), without and with a bias (the output aimed at q - 1 wraps at coefficient 0 of c0), in place when m == c"""
    q, sw = BASES[base]
    _mix(fhe, base, pc.craft("mix", q, pc.gate(q, sw), (m,), t=t), t, "c=8 m=%d" % m)


def _plane_map(fhe, base, case, t, what):
    import torch
    ctx, ev = _ctx(fhe, base, t)
    dctx, dev_ev = _ctx(fhe, base, t, direct=True)
    _report(fhe, ctx, base, "pm", case, what)
    taps, w, order = case.plan
    host = np.stack([pc.to_ct(case.X, case.size), pc.to_ct(np.ascontiguousarray(case.X[:, :, ::-1]), case.size)])      # count 2: the positions once more, reversed
    want = pmo.plane_map_direct(ctx.q, host, taps, w)
    assert np.array_equal(want[0], pc.spec_pm(case))
    plans = [(ev, fhe.PlaneMapPlan(ctx, pc.PM_IN, taps, w, order=order, window=win)) for win in (16, 32, 64)]
    plans.append((dev_ev, fhe.PlaneMapPlan(dctx, pc.PM_IN, taps, w, order=order)))
    plans.append((ev, fhe.PlaneMapPlan(ctx, pc.PM_IN, taps, w, order=order)))
    assert [p.window for _, p in plans[:3]] == [16, 32, 64] and plans[0][1].groups >= plans[1][1].groups >= plans[2][1].groups > 1
    dev = fhe.to_device(host, ctx.device)
    outs = []
    for e, plan in plans:
        out = e.plane_map(plan, dev)
        assert tuple(out.shape) == (2, len(taps), case.size, ctx.k, ctx.n)
        _checked(fhe, e.ctx, dev, host, out, want, (what, plan.window, e is dev_ev))
        outs.append(out)
    assert all(torch.equal(outs[0], o) for o in outs[1:])


PM = [(b, po.T33) for b in BASES] + [("Q4", pc.T_SMALL)]


@pytest.mark.parametrize("base,t", PM, ids=["%s-t%d" % (b, t.bit_length()) for b, t in PM])
def test_plane_map(fhe, base, t):
    """70 planes -> 9 outputs of 64, 8, 8 (one source eight times), 1, 9, 16, 17, 64 and 23 terms, count 2: windows 16, 32, 64, the default
    plan and an FHE_PLANEMAP_DIRECT=1 context"""
    q, sw = BASES[base]
    _plane_map(fhe, base, pc.craft("pm", q, pc.gate(q, sw), (), t=t), t, "windows 16 32 64, default, direct")


@pytest.mark.parametrize("kind", ["block", "mix", "pm"])
@pytest.mark.parametrize("base", ["Q60", "Q61"])
def test_the_gate_from_its_far_side(fhe, base, kind):
    """family S as a lazy kernel would need it -- eight terms of excess 2 on residues in the top sixteenth -- at 60 and 61 bits, where the
    lazy model wraps on thousands of words (test_variant_lazy_sums_beyond_the_gate): the library must take its canonical kernels there"""
    q, sw = BASES[base]
    assert not pc.gate(q, sw)
    args = {"block": (True, True), "mix": (8,), "pm": ()}[kind]
    case = pc.craft(kind, q, True, args, emax={s: [2] * len(q) for s in pc.SITES})
    want = pc.spec(kind, case)
    assert (pc.to_ct(pc.run_model(kind, case)[0], case.size) != want)[:, :, 0].sum() >= 8, "the lazy model does not wrap on this data"
    case = pc.Case(case, A=pc.Arith(q, False))                            # what is printed is the arithmetic the gate chooses
    {"block": _block, "mix": lambda *a: _mix(*a, aimed=False), "pm": _plane_map}[kind](fhe, base, case, po.T33, "family S beyond the gate")

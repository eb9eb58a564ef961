"""CPU: the integer restatement of the packed integer maps (tests/packed_craft.py: k_block8x8<LAZY, PRE>, k_channel_mix<LAZY>, pm_output<LAZY>)
equals the specification (tests/packed_oracle.py, tests/planemap_oracle.py) on random and on crafted inputs, on every base and every
instantiation; the reach table is the one DESIGN.md 3.12.1 records; the crafted operands reach -- in the model's traces, as conditions --
what they are aimed at; and every wrong variant of the model leaves the specification on them.  tests/test_gpu_packed_extremes.py runs
the same operands through the kernels.

Run with -s for the tables.  Every figure printed here comes from the integer model on a CPU; no kernel runs."""
import os
import re
import time

import numpy as np
import pytest

import packed_craft as pc
import packed_oracle as po
import planemap_oracle as pmo

T0 = time.time()
BASES = pc.bases()
LAZY = [b for b, (q, sw) in BASES.items() if pc.gate(q, sw)]
CANONICAL = [b for b in BASES if b not in LAZY]
CASES = [(b, kind, args) for b in BASES for kind, args in pc.instances()]
MIN_POSITIONS = 8
# (base, kind, arguments, target) the seeded budget does not bring to MIN_POSITIONS positions on every prime: nothing is claimed for them
UNREACHED = set()
_runs = {}


def _run(base, kind, args):
    """the crafted case of a base in the arithmetic its gate chooses: (case, out, trace, sums, canon_in, the specification)"""
    key = (base, kind, args)
    if key not in _runs:
        q, sw = BASES[base]
        case = pc.craft(kind, q, pc.gate(q, sw), args)
        _runs[key] = (case,) + pc.run_model(kind, case) + (pc.spec(kind, case),)
    return _runs[key]


def test_the_gate_and_the_bases():
    assert LAZY == ["Q3", "Q4", "Q58"] and CANONICAL == ["shoup", "Q60", "Q61"]
    widths = {b: [p.bit_length() for p in q] for b, (q, _) in BASES.items()}
    assert widths["Q3"] == [36, 36, 37] and widths["Q4"] == [55, 55, 54, 54] and widths["Q58"] == [58, 58] and widths["Q60"] == [60, 55] and widths["Q61"] == [61, 55]
    assert BASES["Q58"][0][0] == pc.WITNESS[0] and BASES["Q61"][0][0] == 0x1FFFFFFFFFFFD801
    assert all(p % 2048 == 1 for q, _ in BASES.values() for p in q)
    assert pc.gate([pc.prime_below(58)]) and not pc.gate([pc.prime_below(59)]) and not pc.gate([pc.prime_below(58)], pc.NOPM)


def test_the_witness_has_excess_3():
    """modarith.h said {0, 1, 2} q, packed_arith.h {0 .. 3} q: the operand 0x78b2b578c230fce6 (above 8 q) times -474698375 modulo the largest
    58-bit prime returns 3 q + (x w mod q)"""
    assert pc.witness() == 3


def test_the_products_of_the_model_are_the_exact_ones():
    """mul_lazy4 is congruent to x w and below 4 q, mul_shoup is x w mod q, for any 64-bit operand, against Python integers"""
    rng = np.random.default_rng(1)
    for q in (BASES["Q3"][0], BASES["Q58"][0], BASES["Q61"][0]):
        W = pc.reach_weights(rng, po.W_MAX, 16)
        x = rng.integers(0, 1 << 64, size=(16, len(q), 64), dtype=np.uint64)
        pw = pc.pairs(W, q)
        with np.errstate(over="ignore"):
            lazy, exact = pc.Arith(q, True).mul(x, pw), pc.Arith(q, False).mul(x, pw)
        for j, w in enumerate(W):
            for i, p in enumerate(q):
                want = [int(v) * (int(w) % p) % p for v in x[j, i]]
                assert [int(v) for v in exact[j, i]] == want
                if p.bit_length() <= 58:
                    assert [int(v) % p for v in lazy[j, i]] == want and int(lazy[j, i].max()) < 4 * p


@pytest.mark.parametrize("base,kind,args", CASES)
def test_model_equals_the_specification_on_the_crafted_inputs(base, kind, args):
    case, out, _, sums, canon_in, want = _run(base, kind, args)
    lim = po.scalar_limit(po.T33)
    weights = np.concatenate([np.asarray(a).reshape(-1) for a in (case.plan if kind == "block" else [case.plan] if kind == "mix" else case.plan[:2][1:]) if a is not None])
    assert (case.X < case.A.qa).all(), "an input is not a canonical residue"
    assert np.abs(weights).max() == lim and weights.min() == -lim and weights.max() == lim, "both ends of the scalar range"
    if kind != "pm":
        assert (weights != 0).all(), "the aimed plans are dense"
    assert np.array_equal(pc.to_ct(out, case.size), want)
    assert case.A.lazy == pc.gate(*BASES[base])
    if case.A.lazy:
        assert int(case.A.units(canon_in).max()) < 4 and all(int(case.A.units(s).max()) < 32 for s in sums.values())


@pytest.mark.parametrize("base", list(BASES))
def test_model_equals_the_specification_on_random_inputs(base):
    """the plans of the existing GPU tests (zeros inside L and R, dead slots, repeated sources, the term counts 1, 8, 9, 16, 17, 64), random residues"""
    q, sw = BASES[base]
    A = pc.Arith(q, pc.gate(q, sw))
    rng = np.random.default_rng(len(base))
    k, size = len(q), 2
    with np.errstate(over="ignore"):
        for pre, post in ((True, True), (True, False), (False, True), (False, False)):
            plan = po.random_plan(rng, po.T33, pre, post)
            X = pc._uniform(rng, A, (64, k, 256))
            out, _ = pc.block_model(A, X, pc.block_tab(q, *plan))
            assert np.array_equal(pc.to_ct(out, size), po.block8x8_direct(q, pc.to_ct(X, size), *plan)), (pre, post)
        for c, m in ((1, 1), (3, 3), (8, 8), (8, 3), (1, 8)):
            M = rng.integers(-po.W_MAX, po.W_MAX + 1, size=(m, c), dtype=np.int64)
            M[0, 0] = M[0, 0] or 1
            if c > 1:
                M[m - 1, 1] = 0
            X = pc._uniform(rng, A, (c, k, 256))
            out, _ = pc.mix_model(A, X, pc.pairs(M, q))
            assert np.array_equal(pc.to_ct(out, size), po.channel_mix_direct(q, po.T33, M, pc.to_ct(X, size))), (c, m)
        taps, w, _ = pmo.random_plan(rng, po.T33, 70, 41, 64, pmo.EDGE_TERMS)
        X = pc._uniform(rng, A, (70, k, 256))
        out, trs = pc.pm_model(A, X, pc.pm_tab(q, taps, w))
        assert np.array_equal(pc.to_ct(out, size), pmo.plane_map_direct(q, pc.to_ct(X, size), taps, w))
        assert sorted({len(tp) // 4 for tp, _, _ in pc.pm_tab(q, taps, w)} & {1, 2, 3, 4, 5, 16}) == [1, 2, 3, 4, 5, 16], "1, 8, 9, 16, 17 and 64 terms are 1, 2, 3, 4, 5 and 16 quads"


# ---- the reach table -------------------------------------------------------------------------------------------------------------------
SUM_SITES = ("col", "post", "one_block", "one_mix", "one_chunk", "one_total")


def reach_rows():
    """per prime of the lazy bases: the largest excess per site (the seeded search) and the largest operand of the sum sites in units of q
    (the crafted families)"""
    rows = []
    for base in LAZY:
        q, _ = BASES[base]
        e = pc.reach_excess(q)
        big = {s: np.zeros(len(q), dtype=np.int64) for s in SUM_SITES}
        for kind, args in pc.instances():
            case, _, _, sums, _, _ = _run(base, kind, args)
            for s, v in sums.items():
                big[s] = np.maximum(big[s], case.A.units(v).reshape(-1, len(q), v.shape[-1]).max(axis=(0, 2)).astype(np.int64))
        for i, p in enumerate(q):
            rows.append([base, "0x%x" % p] + [str(e[s][i]) for s in pc.SITES] + [str(int(big[s][i])) for s in SUM_SITES])
    return rows


def test_reach_table_is_the_one_in_design_md():
    rows = reach_rows()
    head = ["base", "prime"] + list(pc.SITES) + ["sum " + s for s in SUM_SITES]
    print("\n| " + " | ".join(head) + " |\n|" + "---|" * len(head))
    for r in rows:
        print("| " + " | ".join("`%s`" % c if j < 2 else c for j, c in enumerate(r)) + " |")
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    section = text[text.index("#### 3.12.1"):]
    section = section[:section.index("\n### ")]
    found = [[c.strip().strip("`") for c in line.strip().strip("|").split("|")] for line in section.splitlines() if re.match(r"\| `Q(3|4|58)` \| `0x", line)]
    assert found == rows
    # what the table says, as the comments of modarith.h and packed_arith.h now state it
    byp = {(r[0], r[1]): dict(zip(pc.SITES, map(int, r[2:]))) for r in rows}
    assert all(max(v.values()) <= 3 for v in byp.values())
    assert all(v["pre"] == v["row"] == v["row_pre"] == 2 for v in byp.values()), "a canonical operand, or one below 4 q, reaches excess 2 and never 3"
    assert all((v["col"], v["post"]) == ((3, 3) if b == "Q58" else (2, 2)) for (b, _), v in byp.items()), "excess 3 needs a 58-bit prime and an operand from 8 q on"
    assert all(v["one_mix"] == v["one_chunk"] == v["one_total"] == v["one_block"] == (1 if b == "Q3" else 0) for (b, _), v in byp.items())


def test_the_product_by_1_returns_q_at_every_multiple_of_q():
    """the random search finds the product by 1 of a value below 32 q canonical on the 54- to 58-bit primes; at the 31 multiples of q it is
    exactly q on every prime, so canon() behind it does subtract: whenever an output is 0"""
    for base in LAZY:
        A = pc.Arith(BASES[base][0], True)
        x = np.array([[j * p for j in range(1, 32)] for p in A.q], dtype=np.uint64)
        with np.errstate(over="ignore"):
            assert (A.mul(x, A.one) == A.qa).all() and (A.mul(x - np.uint64(1), A.one) == A.qa - np.uint64(1)).all()
            assert (pc.exit_hi(A, A.one, 0) == 1).all() and (pc.exit_hi(A, A.one, 1) == 0).all()


# ---- what the families reach -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,kind,args", CASES)
def test_every_target_is_met_at_eight_positions_on_every_prime(base, kind, args):
    case, out, tr, _, _, _ = _run(base, kind, args)
    counts = pc.count(kind, case, tr, out)
    print("\n[%s %s %r] %s" % (base, kind, args, counts))
    assert {n for n in counts if not n.startswith("site_")} == set(case.names) - {"random"}, "a target without its condition"
    if case.A.lazy and kind == "block":
        assert ("site_pre" in counts) == args[0]
    short = {n for n, c in counts.items() if any(0 <= v < MIN_POSITIONS for v in c)}
    assert short == {t for b, kd, a, t in UNREACHED if (b, kd, a) == (base, kind, args)}, counts
    if case.A.lazy:                                                   # every interval the table allows at this exit, and none above it
        site = {"block": "post" if args and args[-1] else "one_block", "mix": "one_mix", "pm": "one_total"}[kind]
        assert [n for n in counts if re.fullmatch(r"X_\d", n)] == ["X_%d" % j for j in range(max(case.emax[site]) + 1)]


@pytest.mark.parametrize("base", CANONICAL)
def test_family_c_sums_are_8q_minus_8(base):
    """the targeted sums of the canonical path, exactly: eight products of q - 1"""
    q, _ = BASES[base]
    qa = np.array(q, dtype=np.uint64)[:, None]
    want = np.uint64(8) * (qa - np.uint64(1))
    assert [int(v) for v in want[:, 0]] == [8 * p - 8 for p in q] and 8 * max(q) - 8 < 1 << 64
    for pre, post in ((True, True), (False, False)):
        case, _, tr, _, _, _ = _run(base, "block", (pre, post))
        assert (tr["mid"][:, pc.V0][:, :, case.tgt == case.names.index("C_row")] == want[None, :, :]).all()
        assert (tr["o"][pc.U0][:, :, case.tgt == case.names.index("C_col")] == want[None, :, :]).all()
    case, _, tr, _, _, _ = _run(base, "mix", (8,))
    assert (tr["acc"][pc.O0][:, case.tgt == case.names.index("C_sum")] == want).all() and (tr["terms"][pc.O0][:, :, case.tgt == 0] == qa[None] - np.uint64(1)).all()
    case, _, trs, _, _, _ = _run(base, "pm", ())
    for c in pc.PM_CHUNKS:
        assert (trs[pc.PM_WIDE]["acc"][c][:, case.tgt == case.names.index("C_chunk%d" % c)] == want).all()
    assert (trs[pc.PM_WIDE]["total"][:, case.tgt == case.names.index("C_values")] == want).all(), "eight reduced chunks of q - 1"
    if base == "Q61":
        print("\n[Q61] q = 0x%x: 8 q - 8 is %d below 2^64" % (q[0], (1 << 64) - (8 * q[0] - 8)))
        assert (1 << 64) - (8 * q[0] - 8) == 81920


# ---- the wrong variants ----------------------------------------------------------------------------------------------------------------
def _differs(kind, case, want, A=None, **variant):
    """the positions per prime at which a variant of the model leaves the specification"""
    out = pc.run_model(kind, case, A, **variant)[0]
    return (pc.to_ct(out, case.size) != want).sum(axis=(0, 1, 3))


@pytest.mark.parametrize("base", LAZY)
def test_variant_canon_with_one_subtraction(base):
    """csub(x, q) alone is wrong from 2 q on: behind post (every block8x8 plan with one) on family X.  Behind the product by 1 the value
    stays below 2 q, so there the variant is right and the one WITHOUT any subtraction is the wrong one: it fails on every output 0."""
    q, _ = BASES[base]
    for kind, args in pc.instances():
        case, _, _, _, canon_in, want = _run(base, kind, args)
        once, none = pc.Arith(q, True, canon_once=True), pc.Arith(q, True, canon_once=True)
        none.canon = lambda y: y
        d1, d0 = _differs(kind, case, want, once), _differs(kind, case, want, none)
        print("\n[%s %s %r] one subtraction: %s words differ, none: %s" % (base, kind, args, d1, d0))
        if kind == "block" and args[1]:
            assert (d1 >= MIN_POSITIONS).all()
        else:
            assert (d1 == 0).all() and int(case.A.units(canon_in).max()) < 2
        assert (d0 >= MIN_POSITIONS).all()


@pytest.mark.parametrize("bits,wraps", [(59, False), (60, True), (61, True)])
def test_variant_lazy_sums_beyond_the_gate(bits, wraps):
    """family S in lazy arithmetic where the gate forbids it: at 60 and 61 bits the sums wrap and the outputs leave the specification; at
    59 bits 32 q < 2^64 still holds and nothing wraps -- the gate is conservative by one bit"""
    q = [pc.prime_below(bits) if bits != 61 else BASES["Q61"][0][0], BASES["Q4"][0][0]]
    assert not pc.gate(q) and (32 * q[0] < 1 << 64) == (not wraps)
    emax = {s: [2, 2] for s in pc.SITES}
    for kind, args in (("block", (True, True)), ("block", (False, False)), ("mix", (8,)), ("pm", ())):
        case = pc.craft(kind, q, True, args, emax=emax)
        want = pc.spec(kind, case)
        d = _differs(kind, case, want)
        sums = pc.run_model(kind, case)[2]
        print("\n[%d bits, %s %r] lazy: %s words differ; largest sum %s q" % (bits, kind, args, d, max(int(case.A.units(s)[..., 0, :].max()) for s in sums.values())))
        assert d[1] == 0, "the 55-bit prime beside it"
        assert (d[0] >= MIN_POSITIONS) == wraps and (wraps or d[0] == 0)
        assert (_differs(kind, case, want, pc.Arith(q, False)) == 0).all(), "the canonical arithmetic the gate chooses"


def test_variant_nine_terms_and_sixteen_term_chunks():
    """family C at the 61-bit prime: a ninth product of q - 1 on a sum of eight, or a plane-map chunk of sixteen terms, passes 2^64; on
    the 55-bit primes of the same data the variants are the same sums, regrouped, and change nothing"""
    for base in ("Q61", "shoup"):
        q, _ = BASES[base]
        A = pc.Arith(q, False)
        case, out, _, _, _, want = _run(base, "mix", (8,))
        sel = case.tgt == case.names.index("C_sum")
        nine = pc.run_model("mix", case, extra_term=True)[0][pc.O0][:, sel]
        exact = (out[pc.O0][:, sel] + (A.qa - np.uint64(1))) % A.qa          # the ninth term is the first again: q - 1
        wrong = (nine != exact).sum(axis=1)
        case, _, _, _, _, want = _run(base, "pm", ())
        d = _differs("pm", case, want, chunk=16)
        print("\n[%s] nine terms: %s positions wrong; 16-term chunks: %s words differ" % (base, wrong, d))
        if base == "Q61":
            assert wrong[0] == sel.sum() and wrong[1] == 0 and d[0] >= MIN_POSITIONS and d[1] == 0
        else:
            assert (wrong == 0).all() and (d == 0).all()


def test_variant_plane_map_without_the_chunk_reduction():
    """pm_output summing unreduced chunks: 64 lazy terms reach 2^64 on the 58-bit primes (family S); on the 37-bit primes they do not"""
    for base in ("Q58", "Q3"):
        case, _, _, _, _, want = _run(base, "pm", ())
        d = _differs("pm", case, want, reduce_chunks=False)
        print("\n[%s] no per-chunk reduction: %s words differ" % (base, d))
        assert (d >= MIN_POSITIONS).all() if base == "Q58" else (d == 0).all()


def test_small_batching_prime_and_size_3():
    """t = 65537: (t - 1) / 2 = 32768 is the scalar limit and both ends are in the plans; size 3 on Q58.  The model equals the
    specification; what these reach is printed, not claimed (weights that small give a canonical operand no excess 2)"""
    q, sw = BASES["Q4"]
    for kind, args in pc.instances():
        case = pc.craft(kind, q, True, args, t=pc.T_SMALL)
        out, tr, _, _ = pc.run_model(kind, case)
        weights = np.concatenate([np.asarray(a).reshape(-1) for a in (case.plan if kind == "block" else [case.plan] if kind == "mix" else [case.plan[1]]) if a is not None])
        assert weights.min() == -32768 and weights.max() == 32768
        assert np.array_equal(pc.to_ct(out, 2), pc.spec(kind, case, **({"t": pc.T_SMALL} if kind == "mix" else {})))
        print("\n[Q4 t=65537 %s %r] %s" % (kind, args, pc.count(kind, case, tr, out)))
    case = pc.craft("block", BASES["Q58"][0], True, (True, True), size=3)
    out, tr, _, _ = pc.run_model("block", case)
    assert np.array_equal(pc.to_ct(out, 3), pc.spec_block(case))
    counts = pc.count("block", case, tr, out)
    assert all(v >= MIN_POSITIONS for c in counts.values() for v in c), counts


def test_wall_time():
    print("\n[test_packed_craft_cpu] %.0f s since the module was imported" % (time.time() - T0))

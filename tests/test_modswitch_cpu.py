"""CPU: the specification of modulus switching (tests/modswitch_oracle.py) -- its big-integer, residue and 64-bit-register forms agree on
every base the GPU tests use; operands built backwards reach every prescribed remainder, result and wrap; the wrong variants of the
kernel's arithmetic are caught by them; the noise bound of circuits.mod_switch_budget holds on a toy BFV in Python integers."""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

import modswitch_oracle as mo
import packed_oracle as po

BASES = mo.bases(1024)


def _specials(q):
    Q, h = mo.prod(q), q[-1] // 2
    return [0, 1, Q - 1, Q - 2, Q // 2, h, h + 1, Q - h, Q - h - 1]


@pytest.mark.parametrize("name", list(BASES))
def test_the_forms_of_the_specification_agree(name):
    """residue form (vectorised) == 64-bit-register form == big-integer form at every level: 300 random coefficients, the special values
    of the issue and every residue at q_i - 1"""
    q = BASES[name]
    k = len(q)
    rng = np.random.default_rng(len(name) + k)
    ops = [[int(rng.integers(0, qi)) for qi in q] for _ in range(300)] + [[c % qi for qi in q] for c in _specials(q)] + [[qi - 1 for qi in q]]
    x = np.array(ops, dtype=np.uint64).T.copy()                       # [k, count]
    levels = mo.switch_residues_levels(x, q)
    assert sorted(levels) == list(range(1, k))
    for k_out in range(1, k):
        assert levels[k_out].shape == (k_out, len(ops))
        for j, res in enumerate(ops):
            want = mo.switch_big(res, q, k_out)
            assert mo.switch_model(res, q, k_out) == want, (name, k_out, res)
            assert [int(v) for v in levels[k_out][:, j]] == want, (name, k_out, res)
            assert all(w < qi for w, qi in zip(want, q))


@pytest.mark.parametrize("name", list(BASES))
def test_crafted_operands_reach_every_target(name):
    """built backwards, an operand prescribes the rounded remainder of every drop and, by CRT on the last level, every final residue: all
    of r in {0, 1, h-1, h, h+1, p-2, p-1} at every drop x final residues all 0, 1, q_i-2, q_i-1 are reached in the model, and c = 0,
    c = q - 1 and both sides of the wrap at q - h give what the definition gives"""
    q = BASES[name]
    k = len(q)
    for k_out in range(1, k):
        reached = set()
        for res, what in mo.craft(q, k_out, seed=k_out):
            trace = []
            got = mo.switch_model(res, q, k_out, trace=trace)
            assert got == mo.switch_big(res, q, k_out)
            assert all(0 <= v < qi for v, qi in zip(res, q))
            if what[0] == "r":
                _, m, rt, ct = what
                assert trace[k - 1 - m] == mo._r_value(rt, q[m]), (name, k_out, what)
                assert got == [mo._c_value(ct, q[i]) for i in range(k_out)], (name, k_out, what)
            reached.add(what)
        assert {w for w in reached if w[0] == "r"} == {("r", m, rt, ct) for m in range(k_out, k) for rt in mo.R_TARGETS for ct in mo.C_TARGETS}
        assert {"c=0", "c=q-1", "c=q-h-1", "c=q-h"} <= {w[0] for w in reached}
    Q, h = mo.prod(q), q[-1] // 2
    below, at = [(Q - h - 1) % qi for qi in q], [(Q - h) % qi for qi in q]
    assert mo.switch_big(at, q, k - 1) == [0] * (k - 1)                                  # c + h = q: floor(q / p) = q / p = 0 (mod q / p)
    assert mo.switch_big(below, q, k - 1) == [qi - 1 for qi in q[:-1]]                   # c + h = q - 1: q / p - 1


def _caught(q, k_out, variant, ops):
    n = 0
    for res in ops:
        try:
            n += mo.switch_model(res, q, k_out, variant=variant) != mo.switch_model(res, q, k_out)
        except AssertionError:                                         # the variant left its registers' range
            n += 1
    return n


def test_wrong_variants_are_caught_by_the_crafted_operands():
    """Which wrong variants of the kernel's arithmetic the crafted set (37 operands of a two-prime base, k_out = 1) catches, and how many of
    10^5 random coefficients do (seed 1):
         gt_final (`>` for `>=` in the last conditional subtraction of a product; the 58-bit pair): crafted 13 of 37 (every operand whose
                  result is 0: the lazy Shoup product of a non-zero multiple of q_i is exactly q_i), random 0 of 100000;
         gt_r     (`>` for `>=` reducing c_m + h; the 58-bit pair): crafted 6 of 37 (the operands with r = 0, and c = q - h), random 0 of 100000;
         raw_r    (r used as if below q_i; Q61 reversed, the 61-bit prime dropped over the 55-bit one): crafted 27 of 37, random 97659 of
                  100000 -- and none on Q61 itself, where the dropped prime is the smaller one (crafted 0, random 0): the reversed base
                  is what makes the trap a test."""
    rng = np.random.default_rng(1)
    report = {}
    for variant, name, want_crafted in (("gt_final", "Q58", True), ("gt_r", "Q58", True), ("raw_r", "Q61R", True), ("raw_r", "Q61", False)):
        q = BASES[name]
        crafted = [r for r, _ in mo.craft(q, 1, seed=1)]
        rand = [[int(rng.integers(0, qi)) for qi in q] for _ in range(100000)]
        report[(variant, name)] = (_caught(q, 1, variant, crafted), len(crafted), _caught(q, 1, variant, rand))
        assert (report[(variant, name)][0] > 0) == want_crafted, (variant, name, report)
    print("\n[mod_switch wrong variants] (variant, base): (crafted caught, crafted, random caught of 100000) = %r" % report)
    assert report[("gt_final", "Q58")][2] == 0 and report[("gt_r", "Q58")][2] == 0          # random operands do not find the boundary cases
    assert report[("raw_r", "Q61R")][2] > 90000 and report[("raw_r", "Q61")][2] == 0


def _exact_budget(Q, worst):
    """-log2(2 ||v||), ||v|| = worst / Q"""
    return math.log2(Q) - math.log2(worst) - 1 if worst else float("inf")


def _worst(polys, s, Q, t):
    n, acc = len(s), [0] * len(s)
    for c in reversed(polys):
        acc = [(u + v) % Q for u, v in zip(mo.negacyclic_mul(acc, s, Q), c)]
    out, plain = 0, []
    for x in acc:
        m = (t * x + Q // 2) // Q
        out = max(out, abs(t * x - m * Q))
        plain.append(m % t)
    return out, plain


@pytest.mark.parametrize("name,t,size", [("Q3", 65537, 2), ("Q3", 65537, 3), ("Q4", po.T33, 2), ("Q4", 65537, 3)])
def test_noise_bound_holds_on_a_toy_bfv(fhe, name, t, size):
    """n = 32, a ternary secret, a ciphertext of `size` polynomials with a noise of 2^20: after the iterated drops to every level the
    plaintext is unchanged and the exact budget -log2(2 ||v||) is at least mod_switch_budget of the exact budget before"""
    q, n = BASES[name], 32
    ctx = SimpleNamespace(n=n, t=t, q=q, k=len(q))
    rng = np.random.default_rng(size)
    Q = mo.prod(q)
    s = [int(v) - 1 for v in rng.integers(0, 3, size=n)]
    m = [int(v) for v in rng.integers(0, t, size=n)]
    rnd = lambda: [int.from_bytes(rng.bytes(64), "little") % Q for _ in range(n)]
    tail = [rnd() for _ in range(size - 1)]                                               # c_1 .. c_(size-1) uniform
    mask, spow = [0] * n, [1] + [0] * (n - 1)
    for c in tail:
        spow = mo.negacyclic_mul(spow, s, Q)
        mask = [(u + v) % Q for u, v in zip(mask, mo.negacyclic_mul(c, spow, Q))]
    e = [int(v) for v in rng.integers(-(1 << 20), (1 << 20) + 1, size=n)]
    polys = [[(Q // t * mi + ei - mk) % Q for mi, ei, mk in zip(m, e, mask)]] + tail
    worst, plain = _worst(polys, s, Q, t)
    assert plain == m
    before = _exact_budget(Q, worst)
    lines = []
    base = list(q)
    while len(base) > 1:
        polys = [[mo.drop_big(c, base) for c in p] for p in polys]
        base.pop()
        Ql = mo.prod(base)
        bound = fhe.circuits.mod_switch_budget(ctx, before, len(base), size=size)
        if bound <= 0:
            break                                                                          # nothing is promised below zero bits
        worst, plain = _worst(polys, [v % Ql for v in s], Ql, t)
        after = _exact_budget(Ql, worst)
        lines.append("%d primes: %.1f bits, bound %.1f" % (len(base), after, bound))
        assert plain == m, (name, len(base))
        assert after >= bound - 1e-9, (name, size, lines)
    print("\n[toy BFV %s t=%d size=%d n=%d] %.1f bits before; %s" % (name, t, size, n, before, "; ".join(lines)))
    assert lines, "no level was checked"


def test_budget_formula_and_the_choice_of_primes(fhe):
    c = fhe.circuits
    for q, n, t in ((BASES["Q4"], 8192, 1 << 14), (BASES["Q3"], 4096, 65537), (BASES["S16K"], 16384, po.T33)):
        ctx = SimpleNamespace(n=n, t=t, q=q, k=len(q))
        k = len(q)
        for size in (2, 3):
            S = sum(n ** j for j in range(size))
            for B in (20, 100, 140):
                assert c.mod_switch_budget(ctx, B, k, size) == pytest.approx(B)            # no drop: the budget itself
                total = Fraction(1, 1 << B)
                for k_out in range(k - 1, 0, -1):
                    total += Fraction(t * S, mo.prod(q[:k_out]))
                    got = c.mod_switch_budget(ctx, B, k_out, size)
                    assert got == pytest.approx(-math.log2(total), abs=1e-6)
                    assert got <= c.mod_switch_budget(ctx, B, k_out + 1, size) <= B + 1e-9 # fewer primes keep no more (equal in double precision when the sum is far below 2^-B)
            for B in (30, 140):
                picks = [c.mod_switch_primes(ctx, B, keep, size) for keep in range(0, B + 8)]
                assert picks == sorted(picks) and picks[0] >= 1 and picks[-1] == k         # monotone in keep_bits
                for keep, k_out in zip(range(0, B + 8), picks):
                    if k_out < k:
                        assert c.mod_switch_budget(ctx, B, k_out, size) >= keep
                    assert k_out == 1 or c.mod_switch_budget(ctx, B, k_out - 1, size) < keep
                one_drop = c.mod_switch_budget(ctx, B, k - 1, size)
                assert c.mod_switch_primes(ctx, B, math.floor(one_drop) + 1, size) == k    # a single drop already falls short: no switch
                assert c.mod_switch_primes(ctx, B, math.floor(one_drop), size) <= k - 1     # and it qualifies where its bound does
    with pytest.raises(ValueError):
        c.mod_switch_budget(SimpleNamespace(n=1024, t=65537, q=BASES["Q3"]), 50, 0)

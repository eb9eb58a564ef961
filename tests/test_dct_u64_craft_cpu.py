"""What tests/dct_u64_craft.py's value model of the fused u64 DCT pair (csrc/dct_u64.hip) proves, on the CPU (no GPU, no library).  Run with
-s for the tables that DESIGN.md section 3.2.2 quotes.

  validation  in every context of the GPU file: the model's canonical outputs equal the CPU oracle's dct_quant on the sampled work units --
              every unit of the X block at n = 2048; elsewhere, per block, both halves of one column (G-random, G-top, X, W: of an even and an
              odd column) for every polynomial and prime, with the eight row units each of them needs -- and no range assertion of the model
              fires (no 64-bit wrap, no operand above its static bound, every lazy4 result below 4q, every mul_pm operand within PmA::LIM)
  bounds      the static conditions 4 Bn q < 2^64 and 128 q < 2^64 at the largest prime each class admits, and that the class rule is what
              keeps them at the next prime size up
  exits       per (body, L, target) the histogram of the multiple of q with which the zeros of Z and the 0 / q - 1 targets of X reach the
              exit.  Shoup exit csub(csub(x, 2q), q): every cell non-empty.  Pseudo-Mersenne exit csub(fold_pm(x), q): a zero folds to
              exactly q; fold_pm's result is below 2^b + 2^(64-b) delta < q + (q - 1), so q - 1 cannot arrive as 2q - 1: that cell must be EMPTY
  variants    deliberately wrong kernels, in the model only; each must raise or change crafted outputs, except the dropped exit folds of the
              pseudo-Mersenne inverse, which no family reaches (a stated gap); 100 000 random outputs beside it
  reach       static bound beside the largest operand per site (sixteenths of q) for W / X / random / all-(q - 1); no threshold
"""
import time
from collections import Counter

import numpy as np
import pytest

import dct_u64_craft as dc
import ntt_craft as nc
import slot_craft as sc

_CACHE = {}
TWO_COLUMNS = ("G-random", "G-top", "X", "W")


def _units(k, cols):
    return [(i, p, c, h) for i in range(k) for p in range(2) for c in cols for h in range(2)]


def analyse(oracle_mod, name):
    """the batch of one context through the model on the sampled units; asserts the validation; keeps the lazy values of the prescribed
    outputs, the reach per block and the time"""
    if name in _CACHE:
        return _CACHE[name]
    n, q, t, sw, (body, pm) = dc.CONTEXTS[name]
    t0 = time.time()
    sm = dc.slot_model(oracle_mod, n, q, t)
    m = dc.Model(sm)
    names, blocks, tg = dc.craft_batch(sm)
    res = dict(body=body, pm=pm, q=q, n=n, reach={}, zero=Counter(), x0=Counter(), xtop=Counter(), units=0, names=names)
    for b, nm in enumerate(names):
        want = sm.orc.dct_quant(blocks[b], oracle_mod.YQT)
        if nm == "X" and n == 2048:
            units = None
        else:
            units = _units(len(q), ((b % 8, (b + 1) % 8) if nm in TWO_COLUMNS else (b % 8,)))
        out, lazy, reach = m.run(blocks[b], body, pm, units)
        res["reach"][nm] = reach
        res["units"] += len(out)
        for u, got in out.items():
            i, p, c, h = u
            exp = m.expected(want, u)
            assert np.array_equal(got, exp), "%s %s unit %s: the model differs from the oracle" % (name, nm, u)
            assert (lazy[u] % np.uint64(q[i]) == exp).all()
            mult = (lazy[u] // np.uint64(q[i])).astype(np.int64)
            if nm.startswith("Z-") or nm == "G-zero":
                for mi in range(4):
                    if 8 * (2 * mi + h) + c != 0:                    # every output but the DC one is exactly zero
                        assert not exp[mi].any()
                        res["zero"].update(mult[mi].tolist())
            if nm == "X":
                for mi in range(4):
                    tgt = tg[8 * (2 * mi + h) + c, i]
                    tgt = tgt if p == 0 else (np.uint64(q[i]) - tgt) % np.uint64(q[i])
                    assert np.array_equal(exp[mi], tgt), "the oracle's output is not the prescribed target"
                    res["x0"].update(mult[mi][exp[mi] == 0].tolist())
                    res["xtop"].update(mult[mi][exp[mi] == q[i] - 1].tolist())
    res["seconds"] = time.time() - t0
    _CACHE[name] = res
    return res


# ---- the pieces the model stands on -------------------------------------------------------------------------------------------------------------
def test_widened_modular_product_matches_python_integers(oracle_mod):
    """slot_craft.SlotModel's limb product and inverse at 55-, 56- and 57-bit primes (6-bit limbs at 57 bits)"""
    rng = np.random.default_rng(3)
    for q in (dc.PRESET, dc.LAZY56, dc.NOLAZY57):
        m = dc.slot_model(oracle_mod, 2048, q)
        a = rng.integers(0, 1 << 62, size=(m.k, m.n), dtype=np.int64).astype(np.uint64) % m.P
        b = rng.integers(0, 1 << 62, size=(m.k, m.n), dtype=np.int64).astype(np.uint64) % m.P
        a[:, 0], b[:, 0], a[:, 1], b[:, 1] = m.P[:, 0] - np.uint64(1), m.P[:, 0] - np.uint64(1), m.H[:, 0], m.H[:, 0] + np.uint64(1)
        prod, (inv, nz) = m.mul(a, b), m.inv(a)
        for i, p in enumerate(q):
            assert [int(x) for x in prod[i]] == [int(x) * int(y) % p for x, y in zip(a[i], b[i])]
            assert all(int(x) * int(y) % p == 1 for x, y, z in zip(a[i], inv[i], nz[i]) if z)


def test_array_primitives_equal_the_scalar_models():
    """lazy4 / mul_pm / fold_pm on arrays against ntt_craft.mul_shoup_lazy4 and test_pm_arithmetic_model.mul_pm / fold_pm in Python
    integers, element by element: any 64-bit operand for lazy4 and fold_pm, up to 128 q for mul_pm; twiddles 1, q - 1, q / 2, random"""
    import random
    rng = random.Random(8)
    for q in dc.PRESET + dc.LAZY56 + dc.NOLAZY57 + dc.LOW48:
        xs = [nc.M64, 128 * q - 1, 0, 1, q, q - 1, 4 * q, 1 << 63, (1 << 32) - 1, 1 << 32] + [rng.randrange(1 << 64) for _ in range(500)]
        ws = [1, q - 1, q // 2, 2] + [rng.randrange(q) for _ in range(4)]
        X = np.array(xs, dtype=np.uint64)
        for w in ws:
            wp = (w << 64) // q
            r = dc.lazy4(X, np.uint64(w), np.uint64(wp), q)
            assert [int(v) for v in r] == [nc.mul_shoup_lazy4(x, w, wp, q) for x in xs]
            acc = np.array([rng.randrange(4 * q) for _ in xs], dtype=np.uint64)
            ra = dc.lazy4(X, np.uint64(w), np.uint64(wp), q, acc=acc)
            assert [int(v) for v in ra] == [nc.mul_shoup_lazy4(x, w, wp, q, int(a)) for x, a in zip(xs, acc)]
        if q.bit_length() <= 55 and dc.pm_class([q]) == 1:
            m = dc.Pm(q)
            lim = dc.PMA["LIM"] * q // 16
            xm = [lim, lim - 1, 0, 1, q, q - 1, (1 << 31) - 1, 1 << 31] + [rng.randrange(lim + 1) for _ in range(500)]
            Xm = np.array(xm, dtype=np.uint64)
            for w in ws:
                r = dc.mul_pm(Xm, np.uint64(w), np.uint64((w << 31) % q), m)
                assert [int(v) for v in r] == [dc.mul_pm_int(x, w, m) for x in xm]
            assert [int(v) for v in dc.fold_pm(X, m)] == [dc.fold_pm_int(x, m) for x in xs]
    big = np.array([1 << 63, 5], dtype=np.uint64)
    for bad in (lambda: dc.add(big, big), lambda: dc.sub_off(np.array([1], dtype=np.uint64), np.array([9], dtype=np.uint64), np.uint64(7)), lambda: dc.shl1(big)):
        with pytest.raises(AssertionError):
            bad()


def test_context_primes_classes_and_instantiations():
    """the primes are what the searches find; the class rule gives each context the body the issue expects; k takes 1, 2 and 3; the
    contexts launch all nine row and six column instantiations"""
    assert dc.LAZY56 == [nc.largest_primes(56, 8192, 1)[0], nc.largest_primes(55, 8192, 1)[0]]
    assert dc.NOLAZY57 == [nc.largest_primes(57, 8192, 1)[0], nc.largest_primes(56, 8192, 1)[0]]
    assert dc.LOW48[0] == sc.search_prime(1 << 47, +1) and dc.LOW48[1] == sc.search_prime(dc.LOW48[0] - 1 + (1 << 14), +1)
    for q in (dc.PRESET3, dc.LAZY56, dc.NOLAZY57, dc.LOW48):
        assert all(sc.is_prime(p) and p % (1 << 14) == 1 for p in q) and len(set(q)) == len(q)
    assert [p.bit_length() for p in dc.LAZY56 + dc.NOLAZY57 + dc.LOW48] == [56, 55, 57, 56, 48, 48]
    want = {"pmA": ("pm", True), "shoup55": ("lazy", False), "lazy56": ("lazy", False), "nolazy57": ("nolazy", False), "low48": ("lazy", False)}
    for name, (n, q, t, sw, exp) in dc.CONTEXTS.items():
        assert exp == want[name.split("-")[0]], name
        assert dc.classify(n, q, sw)[0] == 2 and dc.classify(n, q, dict(sw, FHE_DCT_FORCE_U64=1))[0] == 0
    assert {len(c[1]) for c in dc.CONTEXTS.values()} == {1, 2, 3}
    assert dc.instantiations() == dc.ALL_INSTANTIATIONS and len(dc.ALL_INSTANTIATIONS) == 15
    # what the suite launched before this file, by the same rule: tests/test_gpu_parity.py at the presets (all three n) and at the largest
    # 56- and 57-bit primes (n = 4096 only), and tests/test_gpu_dct_slot_extremes.py in its contexts n4096-above47 and n8192-above47, whose
    # 48-bit prime takes the DCT off the FP64 pair and onto this one (that file asserts only that the path is not 1)
    earlier = [(n, dc.PRESET, {}) for n in (2048, 4096, 8192)] + [(4096, [nc.largest_primes(b, 4096, 1)[0], nc.largest_primes(b - 1, 4096, 1)[0]], {}) for b in (56, 57)]
    earlier += [(n, q, sw) for n, q, sw, _ in sc.GPU_CONTEXTS.values()]
    before, slot_file = set(), set()
    for n, q, sw in earlier:
        path, body, pm, _ = dc.classify(n, q, sw)
        if path == 2:
            L = n.bit_length() - 1
            before |= {("rows", L, body != "nolazy", body == "pm"), ("cols", L, pm)}
            if q[0] == sc.P_ABOVE_47:
                slot_file |= {("rows", L, body != "nolazy", body == "pm"), ("cols", L, pm)}
    assert slot_file == {("rows", 12, True, False), ("cols", 12, False), ("rows", 13, True, False), ("cols", 13, False)}
    assert [nm for nm, c in sc.GPU_CONTEXTS.items() if dc.classify(c[0], c[1], c[2])[0] == 2] == ["n4096-above47", "n8192-above47"]
    # of the six instantiations the issue lists, two were reached there; four were launched by no test
    assert dc.ALL_INSTANTIATIONS - before == {("rows", 11, True, False), ("rows", 11, False, False), ("rows", 13, False, False), ("cols", 11, False)}
    assert dc.classify(4096, [sc.P_BELOW_47, sc.Q46[0]])[0] == 1 and dc.classify(4096, nc.largest_primes(58, 8192))[0] == 0


def test_static_bounds_at_the_admission_thresholds():
    """the largest prime each class admits keeps 4 Bn q and 128 q below 2^64 at L = 13 (and so at 11 and 12); one prime size up the bound
    would fail for that body, and the class rule (57 bits -> not LAZY, 56 -> not PM, 58 -> not supported) is what sends the prime elsewhere"""
    top = {b: nc.largest_primes(b, 8192, 1)[0] for b in (55, 56, 57, 58)}
    print()
    for body, bits in (("pm", 55), ("lazy", 56), ("nolazy", 57)):
        q = top[bits]
        for L in (11, 12, 13):
            assert dc.static_bounds_hold(L, body, q)
        print("%-6s %d bits: 4 Bn q = %.4f x 2^64, 128 q = %.4f x 2^64" % (body, bits, 4 * dc.bn(13, body) * q / 2.0 ** 64, 128 * q / 2.0 ** 64))
    assert not dc.static_bounds_hold(13, "pm", top[56]) and dc.classify(8192, [top[56], top[55]])[1] == "lazy"
    assert not dc.static_bounds_hold(13, "lazy", top[57]) and dc.classify(8192, [top[57], top[56]])[1] == "nolazy"
    assert not dc.static_bounds_hold(11, "lazy", top[57])
    assert not dc.static_bounds_hold(13, "nolazy", top[58]) and dc.classify(8192, [top[58], top[57]])[0] == 0
    assert dc.classify(8192, [top[57], top[56]], lazy_limit=57)[1] == "lazy"           # the wrong rule, for the variants below
    assert 128 * top[57] == (1 << 64) - 128 * ((1 << 57) - top[57]) and 32 + (12 << 7) <= dc.PMA["LIM"]
    for L in (11, 12, 13):                                     # the range plans: no inv_stage bound above 32 q before a stage, 64 q after it
        for P in range(dc.n_passes(L)):
            assert max(dc.inv_bd(L, P, r, u) for r in range(8) for u in range(1, dc.p_stages(L, P) + 1)) <= 32
            assert max(dc.inv_bd(L, P, r, 0) for r in range(8)) <= 64
            assert dc.pm3_plan(L, P)[3] == 0                    # at these sizes pm3_plan never asks for a fold_y / fold_x: only exit folds


@pytest.mark.parametrize("name", list(dc.CONTEXTS))
def test_model_equals_the_oracle_and_no_range_assertion_fires(oracle_mod, name):
    res = analyse(oracle_mod, name)
    print("\n%s: %d column units (and the row units they need) in %.1f s" % (name, res["units"], res["seconds"]))
    assert set(res["names"]) == {"G-random", "G-top", "G-zero", "Z-one", "Z-half-", "Z-half+", "Z-top", "X", "W"}
    if res["n"] == 2048:
        assert res["units"] >= 2 * len(res["q"]) * 16


@pytest.mark.parametrize("name", list(dc.CONTEXTS))
def test_exit_cells(oracle_mod, name):
    res = analyse(oracle_mod, name)
    L = res["n"].bit_length() - 1
    print("\n%s (%s, L = %d) multiple of q in front of the exit: count   zeros of Z %s   X target 0 %s   X target q-1 %s"
          % (name, "pm exit" if res["pm"] else "Shoup exit", L, dict(sorted(res["zero"].items())), dict(sorted(res["x0"].items())), dict(sorted(res["xtop"].items()))))
    lazy = lambda h: sum(c for k, c in h.items() if k >= 1)
    assert lazy(res["zero"]) > 0 and lazy(res["x0"]) > 0
    if res["pm"]:
        assert set(res["zero"]) <= {0, 1} and set(res["x0"]) <= {0, 1}      # a zero folds to exactly q (or is 0)
        assert lazy(res["xtop"]) == 0 and res["xtop"][0] > 0                # 2q - 1 is above fold_pm's range: the cell must be empty
    else:
        assert lazy(res["xtop"]) > 0 and max(list(res["zero"]) + list(res["x0"]) + list(res["xtop"])) <= 3
        if min(res["q"]).bit_length() >= 55:                    # 0 as exactly 2q: the one value that tells `>=` from `>` in csub(., 2q)
            assert res["zero"][2] > 0 and res["x0"][2] > 0


# ---- deliberately wrong variants -----------------------------------------------------------------------------------------------------------------
VARIANTS = [("shoup55-n2048", "exit > (2q)", {"exit_gt": 0}), ("shoup55-n2048", "exit > (q)", {"exit_gt": 1}), ("pmA-n2048", "pm exit >", {"exit_gt": 0}),
            ("shoup55-n2048", "end-of-pass csub(32q) dropped, pass 2", {"drop_csub": (2, 0)}), ("shoup55-n2048", "end-of-pass csub(16q) dropped, pass 2", {"drop_csub": (2, 1)}),
            ("shoup55-n2048", "end-of-pass csub(8q) dropped, pass 2", {"drop_csub": (2, 2)}), ("shoup55-n2048", "end-of-pass csub(8q) dropped, pass 3", {"drop_csub": (3, 2)}),
            ("shoup55-n2048", "off one class too small at bound 8q", {"off_small": 8}), ("shoup55-n2048", "off one class too small at bound 16q", {"off_small": 16}),
            ("shoup55-n2048", "off one class too small at bound 32q", {"off_small": 32}),
            ("shoup55-n2048", "RED04 omitted (lazy rows)", {"no_red04": True}), ("pmA-n2048", "RED04 omitted (pm rows)", {"no_red04": True}),
            ("nolazy57-n2048", "RED04 omitted (non-lazy rows)", {"no_red04": True}),
            ("nolazy57-n2048", "LAZY taken at 57 bits", {"body": "lazy", "skip_static": True}),
            ("pmA-n2048", "exit fold of register 0 dropped, pass 2", {"drop_fold": (2, 0)}), ("pmA-n2048", "exit fold of register 1 dropped, pass 1", {"drop_fold": (1, 1)}),
            ("pmA-n2048", "exit fold of register 4 dropped, pass 3", {"drop_fold": (3, 4)})]


def _count(m, blocks, names, picks, body, pm, var):
    """(changed outputs, outputs, raised) of the wrong variant against the right model on the picked (block name, units)"""
    rights = [(blocks[names.index(nm)] if isinstance(nm, str) else nm, units) for nm, units in picks]
    rights = [(blk, units, m.run(blk, body, pm, units)[0]) for blk, units in rights]
    total, changed = sum(v.size for _, _, right in rights for v in right.values()), 0
    for blk, units, right in rights:
        try:
            wrong = m.run(blk, var.get("body", body), pm, units, var)[0]
        except AssertionError as e:
            return changed, total, str(e) or "assertion"
        changed += sum(int((wrong[u] != right[u]).sum()) for u in right)
    return changed, total, None


@pytest.fixture(scope="module")
def small(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            n, q, t, sw, (body, pm) = dc.CONTEXTS[name]
            sm = dc.slot_model(oracle_mod, n, q, t)
            names, blocks, _ = dc.craft_batch(sm)
            rnd = [sm.orc.random_ct(64, seed=500 + r) for r in range(2)]
            cache[name] = (dc.Model(sm), names, blocks, rnd, body, pm)
        return cache[name]
    return get


@pytest.mark.parametrize("ctx,label,var", VARIANTS, ids=[v[1] for v in VARIANTS])
def test_wrong_variants_are_caught_by_the_crafted_families(small, ctx, label, var):
    """crafted: per family the units (prime, polynomial) x columns 0 and 1 x both halves of one block (Z-one, X, W, G-zero); random: 16 column
    units of two random blocks = 131 072 outputs.  A variant is caught when the model raises or a crafted output changes."""
    m, names, blocks, rnd, body, pm = small(ctx)
    k = m.k
    crafted = [(nm, _units(k, (0, 1))) for nm in ("Z-one", "X", "W", "G-zero")]
    random_picks = [(rnd[r], [(i, p, c, 0) for i in range(min(k, 2)) for p in range(2) for c in (2 * r, 2 * r + 1)] + [(0, p, 5 + r, 1) for p in range(2)] + [(k - 1, 0, 7, r), (k - 1, 1, 6, r)]) for r in range(2)]
    cc, ct, craised = _count(m, blocks, names, crafted, body, pm, var)
    rc, rt, rraised = _count(m, blocks, names, random_picks, body, pm, var)
    print("\n%-46s crafted: %s   random: %s" % (label, "raises (%s)" % craised if craised else "%d of %d outputs change" % (cc, ct),
                                                 "raises (%s)" % rraised if rraised else "%d of %d outputs change" % (rc, rt)))
    assert rt >= 100000
    if "drop_fold" in var:
        # pm3_plan holds no fold_y / fold_x at n = 2048 .. 8192 (asserted above): the variant the plan does have is a dropped inv_exit_pm
        # fold.  A fold changes no residue, so the variant can only show as a wrap, a negative difference or a product operand above LIM.
        #   pass 3 at n = 2048 (registers 0 and 4, bound 16 q = the next pass's offset): not needed for ANY legal input, shown statically
        #   elsewhere (bounds 96 q and 24 q against an offset of 16 q): needed by the static bounds, which rest on RQ = 6 q per product;
        #   mul_pm returns less than 2^b + 2^32 delta, about 2.5 q at these primes and 1.0 q on almost all data, so no input tried comes
        #   near: the counts are a measurement, and the fold stays a condition of the static proof, not of any output seen
        P, r = var["drop_fold"]
        needed = dc.pm3_exit_fold_needed(m.L, P, r)
        print("%-46s static: %s" % ("", needed or "not needed: every later difference stays non-negative and within LIM"))
        assert (needed is None) == (P == 3)
        if needed is None:
            assert not craised and not rraised and cc == 0 and rc == 0
        return
    assert craised or cc > 0, "the variant is not caught by any crafted family"
    if "exit" in label and "fold" not in label:
        assert not rraised and rc == 0                          # the exits: only prescribed values can tell


def test_w_search_and_reach_table(oracle_mod):
    """the bounded search of family W at n = 2048 in each body, and W_CHOICE against it; then per context and site the static bound beside
    what W, X, the random block and the all-(q - 1) block reach (sixteenths of q).  A measurement: its only condition is that no operand
    passes its bound, which the model asserts as it runs."""
    print()
    total = {}
    searched = [(name,) + dc.CONTEXTS[name][:2] + dc.CONTEXTS[name][4] for name in ("pmA-n2048", "shoup55-n2048", "lazy56-n2048", "nolazy57-n2048")]
    for name, n, q, body, pm in searched + [("low48 at n = 2048", 2048, dc.LOW48, "lazy", False)]:
        m = dc.Model(dc.slot_model(oracle_mod, n, q))
        scores = dc.search_w(m, body, pm)
        bits = max(p.bit_length() for p in q)
        for nm, s in scores.items():
            key = nm.replace("X^%d" % (n - 1), "X^%d")
            total.setdefault(bits, Counter())[key] += sum(s)
        top = sorted(scores, key=lambda nm: -sum(scores[nm]))[:3]
        print("%s: W search over %d candidates, best three (share of the row, column, inverse-difference bound): %s"
              % (name, len(scores), "; ".join("%s %.2f %.2f %.2f" % ((nm,) + scores[nm]) for nm in top)))
    for bits, tally in total.items():
        assert dc.W_CHOICE[bits] == max(tally, key=lambda nm: tally[nm]), (bits, tally.most_common(3))
    sites = ("rows fwd out", "rows tmp12+tmp13", "rows out 0", "rows out 4", "rows z3+z4", "cols tmp12+tmp13", "cols out 0", "cols out 4", "cols z3+z4",
             "inv difference, bound 64 q", "inv sum, bound 64 q", "inv difference (pm)")
    for name in dc.CONTEXTS:
        res = analyse(oracle_mod, name)
        print("%s (%s)   site: bound | W  X  random  all-(q-1)" % (name, res["body"] + ("/pm" if res["pm"] else "")))
        for s in sites:
            cells = [res["reach"][b].get(s) for b in ("W", "X", "G-random", "G-top")]
            if any(cells):
                bound = [c[0] for c in cells if c][0]
                print("   %-28s %5d | %s" % (s, bound, "  ".join("%5d" % (c[1] if c else 0) for c in cells)))
                assert all(c is None or c[1] <= bound for c in cells)

"""What tests/ntt_craft.py's integer models of the transform kernels prove, on the CPU (no GPU, no library).  Run with -s for the tables.

  pinning     every crafted and structured operand and 20 random ones per base: the model's canonical output equals the exact transform
              and none of the model's range assertions fires (pm_fwd_bound / pm_inv_plan on real values, mul_shoup_lazy4 below 4q on the
              operands a transform really produces, canon_below_64q's estimate in {Q - 1, Q})
  hits        per base, operation and target value: the prescribed outputs that reach the canonicalisation in a NON-canonical form
              (a non-zero multiple of q for target 0, r + q or more for the others), as a histogram of the multiple.  None may be empty --
              where the range in front of the canonicalisation admits one at all: a target r can only appear as r + q when r + q lies below
              that range's bound (ntt_craft.exit_bound, from the kernels' own range statements).  A class-B inverse output is a mul_pm
              result below 2^b + 2^32 delta, about (1 + 2^-10) q, so only 0, 1 and 2 can be lazy there; such cells must be EMPTY.
  variants    deliberately wrong last steps, applied in the model to the lazy values: `>` for `>=` in canon_pm, canon_rq_pm, each of the
              three conditional subtractions of the non-lazy forward exit and the two of the inverse exit; canon_below_64q without its
              (1 - 2^-17) factor at the largest 55- and 58-bit primes; `<=` for `<` in the FP64 exit.  Each must change a crafted output
              and none of 10^5 random ones.
  reach       per stage the static bound beside the largest operand reached by the crafted, the random and the all-(q - 1) inputs: a
              measurement without a threshold (its only condition is that no range assertion fires)
"""
import functools
import random
from collections import Counter

import numpy as np
import pytest

import ntt_craft as nc

N = 1024
CASES = [("pm-A", 1024), ("pm-B", 1024), ("pm-A", 2048), ("pm-B", 2048), ("shoup-lazy-A", 1024), ("shoup-lazy-B", 1024), ("shoup-small", 1024),
         ("shoup-nolazy-61", 1024), ("shoup-nolazy-A", 1024), ("shoup-nolazy-33", 1024)]
OPS = ("fwd", "inv", "mp")


def _ints(a):
    return [int(v) for v in a]


@functools.lru_cache(maxsize=None)
def analyse(name, n):
    """all crafted, structured and 20 random operands of one base through the models; asserts the pinning, returns the lazy values of the
    prescribed outputs, the hit histograms and the reach table"""
    q, t, _, _, fam, tf_lazy, mp_lazy = nc.base(name, n)
    cr = nc.crafted_by_model(name, n)
    res = dict(lazy={op: [] for op in OPS}, hits={}, reach={}, q=q, fam=fam, tf_lazy=tf_lazy, mp_lazy=mp_lazy)

    def note(run, op, kind, i, want, pat):
        assert run.out == want, "%s %s prime %d: the model's output differs from the exact transform" % (name, op, i)
        assert max(run.out) < q[i]
        for label, bd, top in run.reach:
            cell = res["reach"].setdefault((op, label), dict(bound=bd, crafted=0, random=0, qm1=0))
            assert cell["bound"] == bd
            cell[kind] = max(cell[kind], top)
        if pat is not None:
            res["lazy"][op].append((i, run.lazy, pat))

    rng = random.Random("random/%s/%d" % (name, n))
    for i in range(len(q)):
        fwd, inv, mp = nc.model(fam, nc.tables(q[i], n), tf_lazy, mp_lazy)
        kind = lambda nm: "qm1" if nm == "all q-1" else "crafted"
        for j, nm in enumerate(cr.F_names):
            note(fwd(cr.F[j][i]), "fwd", kind(nm), i, _ints(cr.F_slots[j][i]), _ints(cr.F_pat[nm][i]) if nm in cr.F_pat else None)
        for j, nm in enumerate(cr.I_names):
            note(inv(cr.I[j][i]), "inv", kind(nm), i, _ints(cr.I_out[j][i]), _ints(cr.F_pat[nm][i]) if nm in cr.F_pat else None)
        for j, nm in enumerate(cr.M_names):
            note(mp(cr.M[j][i], cr.P_slots[i]), "mp", kind(nm), i, _ints(cr.M_out[j][i]), _ints(cr.M_pat[nm][i]) if nm.startswith("out") else None)
    for r in range(20):
        i, T = r % len(q), nc.tables(q[r % len(q)], n)
        fwd, inv, mp = nc.model(fam, T, tf_lazy, mp_lazy)
        a = [rng.randrange(q[i]) for _ in range(n)]
        op = OPS[(r // len(q)) % 3]
        if op == "fwd":
            note(fwd(a), op, "random", i, nc.exact_fwd(a, T), None)
        elif op == "inv":
            note(inv(a), op, "random", i, nc.exact_inv(a, T), None)
        else:
            w = _ints(cr.P_slots[i])
            note(mp(a, w), op, "random", i, nc.exact_inv([x * y % q[i] for x, y in zip(nc.exact_fwd(a, T), w)], T), None)
    for op in OPS:
        for i, lazy, pat in res["lazy"][op]:
            V = nc.targets(q[i])
            for v, r in zip(lazy, pat):
                if r in V:
                    assert v % q[i] == r
                    h = res["hits"].setdefault((op, i, V.index(r)), Counter())
                    if v != r:
                        h[v // q[i]] += 1
    return res


@pytest.mark.parametrize("name,n", CASES)
def test_models_equal_the_exact_transforms_and_stay_inside_their_ranges(name, n):
    res = analyse(name, n)
    assert all(res["lazy"][op] for op in OPS)


def test_lazy4_product_at_its_extreme_operands():
    """mul_shoup_lazy4 for ANY 64-bit x: 2^64 - 1, 32q - 1, the twiddles q - 1 and 1 (reduce_lazy4), with and without the accumulator"""
    rng = random.Random(4)
    for q in nc.Q4 + nc.Q3 + nc.largest_primes(58, N) + nc.largest_primes(61, N, 1) + nc.largest_primes(33, N, 1):
        for w in (1, q - 1, q // 2, 2, rng.randrange(q)):
            wp = (w << 64) // q
            for x in [nc.M64, 32 * q - 1 if 32 * q <= nc.M64 else 8 * q - 1, q, q - 1, 4 * q, 0, 1 << 63, (1 << 32) - 1, 1 << 32] + [rng.randrange(1 << 64) for _ in range(300)]:
                r = nc.mul_shoup_lazy4(x, w, wp, q)
                assert r % q == x * w % q and r < 4 * q
                acc = rng.randrange(4 * q)
                assert nc.mul_shoup_lazy4(x, w, wp, q, acc) == acc + r


def _reachable(res, op, i, r, L):
    lazy = res["mp_lazy"] if op == "mp" else res["tf_lazy"]
    return r + res["q"][i] < nc.exit_bound(res["fam"], "fwd" if op == "fwd" else "inv", res["q"][i], L, lazy)


@pytest.mark.parametrize("name,n", CASES)
def test_every_target_reaches_the_canonicalisation_in_lazy_form(name, n):
    res, L = analyse(name, n), n.bit_length() - 1
    q = res["q"]
    print("\n%s n=%d: prescribed outputs in lazy form, multiple of q: count" % (name, n))
    for op in OPS:
        for ti, tn in enumerate(("0", "1", "2", "q/2", "q/2+1", "q-2", "q-1")):
            tot, can, cannot = Counter(), False, False
            for i in range(len(q)):
                h = res["hits"][(op, i, ti)]
                if _reachable(res, op, i, nc.targets(q[i])[ti], L):
                    can = True
                    tot.update(h)
                else:
                    cannot = True
                    assert not h, "a lazy value above the range the kernel states"
            print("  %-3s %-6s %s%s" % (op, tn, dict(sorted(tot.items())) if can else "not reachable: r + q is above the exit range", " (some primes only)" if can and cannot else ""))
            assert not can or sum(tot.values()) > 0, "%s %s target %s: no prescribed output is lazy" % (name, op, tn)


# ---- the deliberately wrong variants -------------------------------------------------------------------------------------------------------
def _variants(res, op, i):
    """name -> (right, wrong) last steps for the lazy values of operation `op` modulo prime i"""
    q, fam = res["q"][i], res["fam"]
    if fam in ("A", "B"):
        m, RQ = nc.Pm(q), nc.CLASSES[fam]["RQ"]
        if op == "fwd":
            return {"canon_pm >": (lambda v: nc.canon_pm(v, m), lambda v: nc.canon_pm(v, m, True))}
        return {"canon_rq_pm >": (lambda v: nc.canon_rq_pm(v, m, RQ), lambda v: nc.canon_rq_pm(v, m, RQ, True))}
    if op == "fwd" and res["tf_lazy"]:
        c, cw = nc.canon_scale(q), nc.canon_scale(q, False)
        return {"canon_below_64q without (1 - 2^-17)": (lambda v: nc.canon_below_64q(v, q, c), lambda v: nc.canon_below_64q(v, q, cw, strict=False))}
    if op == "fwd":
        return {"forward exit > (%s)" % s: (lambda v: nc.exit_fwd_nolazy(v, q), lambda v, g=g: nc.exit_fwd_nolazy(v, q, g)) for g, s in enumerate(("4q", "2q", "q"))}
    return {"inverse exit > (%s)" % s: (lambda v: nc.exit_inv(v, q), lambda v, g=g: nc.exit_inv(v, q, g)) for g, s in enumerate(("2q", "q"))}


@functools.lru_cache(maxsize=None)
def random_lazy(name, op, primes, count=100000):
    """lazy values of `count` outputs of random transforms (round-robin over `primes`, indices into the base)"""
    q, _, _, _, fam, tf_lazy, mp_lazy = nc.base(name, N)
    rng, out = random.Random("variants/%s/%s" % (name, op)), []
    w = nc.crafted_by_model(name, N).P_slots
    for r in range(-(-count // N)):
        i = primes[r % len(primes)]
        fwd, inv, mp = nc.model(fam, nc.tables(q[i], N), tf_lazy, mp_lazy)
        a = [rng.randrange(q[i]) for _ in range(N)]
        run = fwd(a) if op == "fwd" else inv(a) if op == "inv" else mp(a, _ints(w[i]))
        out.append((i, run.lazy))
    return out


# (base, operation): the last steps the issue names, each on the base whose kernels have it
VARIANT_CASES = [("pm-A", "fwd"), ("pm-A", "inv"), ("pm-A", "mp"), ("pm-B", "fwd"), ("pm-B", "inv"), ("shoup-nolazy-A", "fwd"), ("shoup-nolazy-61", "inv"),
                 ("shoup-lazy-A", "inv"), ("shoup-lazy-A", "fwd"), ("shoup-lazy-B", "fwd")]


@pytest.mark.parametrize("name,op", VARIANT_CASES)
def test_wrong_last_steps_change_crafted_outputs_and_no_random_one(name, op):
    res = analyse(name, N)
    q = res["q"]
    only0 = res["tf_lazy"] and op == "fwd"                  # the constant is tested at the largest prime of the base: 55 and 58 bits
    assert not only0 or (q[0] == max(q) and q[0].bit_length() in (55, 58))
    primes = (0,) if only0 else tuple(range(len(q)))
    crafted, rnd = Counter(), Counter()
    for src, tally in ((res["lazy"][op], crafted), (random_lazy(name, op, primes), rnd)):
        for item in src:
            i, lazy = item[0], item[1]
            if i not in primes:
                continue
            for vn, (right, wrong) in _variants(res, op, i).items():
                tally[vn] += sum(1 for v in lazy if right(v) != wrong(v))
                tally[vn + " of"] += len(lazy)
    print()
    for vn in [v for v in crafted if not v.endswith(" of")]:
        print("%s %s: %-40s changes %d of %d crafted and %d of %d random outputs" % (name, op, vn, crafted[vn], crafted[vn + " of"], rnd[vn], rnd[vn + " of"]))
        assert crafted[vn] > 0 and rnd[vn] == 0 and rnd[vn + " of"] >= 100000


@pytest.mark.parametrize("q", [nc.Q4[0], nc.largest_primes(58, N, 1)[0], nc.Q3[0], nc.largest_primes(34, N, 1)[0]])
def test_canon_below_64q_on_the_grid_of_lazy_values(q):
    """k q + r, k = 0 .. 62, r in the targets: the kernel's constant is right everywhere; the constant without the safety factor is wrong
    on residues just below q at the wide primes (the estimate rounds up to the next integer) and nowhere at 34 - 37 bits, which is why
    all-(q - 1) inputs on small primes could not catch it"""
    c, cw = nc.canon_scale(q), nc.canon_scale(q, False)
    grid = [k * q + r for k in range(63) for r in nc.targets(q)]
    assert all(nc.canon_below_64q(v, q, c) == v % q for v in grid)
    wrong = [v for v in grid if nc.canon_below_64q(v, q, cw, strict=False) != v % q]
    print("\nq of %d bits: without the factor %d of %d grid values are wrong" % (q.bit_length(), len(wrong), len(grid)))
    assert all(v % q >= q - 2 for v in wrong)
    assert bool(wrong) == (q.bit_length() >= 55)


def test_fp64_exit_variant():
    """the last step of k_poly_f64 on the centred value: `<=` for `<` turns every 0 into p; random residues have no 0"""
    rng = random.Random(9)
    for q in nc.Q3:
        crafted = nc.pattern(q, N, "mixed", nc.SEED) + nc.pattern(q, N, "dense", nc.SEED)
        assert all(nc.f64_exit(nc.centred(r, q), q) == r for r in crafted + [0, q - 1, q // 2, q // 2 + 1])
        bad = sum(1 for r in crafted if nc.f64_exit(nc.centred(r, q), q, True) != r)
        rnd = sum(1 for _ in range(100000) if (lambda r: nc.f64_exit(nc.centred(r, q), q, True) != r)(rng.randrange(q)))
        neg = Counter(nc.targets(q).index(r) for r in crafted if r in nc.targets(q) and nc.centred(r, q) < 0)
        print("\nFP64 exit, q = %#x: `<=` changes %d of %d crafted and %d of 100000 random outputs; negative centred targets (index: count) %s" % (q, bad, len(crafted), rnd, dict(neg)))
        assert bad > 0 and rnd == 0 and set(neg) == {4, 5, 6}


def test_reach_table():
    """static bound beside the largest operand (sixteenths of q) the crafted, random and all-(q - 1) inputs reach; no threshold"""
    print()
    for name, n in CASES:
        res = analyse(name, n)
        print("%s n=%d      stage: bound | crafted  random  all-(q-1)" % (name, n))
        for (op, label), c in res["reach"].items():
            print("  %-3s %-7s %5d | %5d %5d %5d" % (op, label, c["bound"], c["crafted"], c["random"], c["qm1"]))
            assert max(c["crafted"], c["random"], c["qm1"]) <= c["bound"]

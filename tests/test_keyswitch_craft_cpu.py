"""CPU: the one-slot restatement of the key switch (tests/keyswitch_craft.py) equals the C oracle on the crafted operands, and the
operands reach -- in the model, as conditions -- what they are aimed at.  tests/test_gpu_keyswitch_extremes.py runs the same operands
through the kernels of csrc/behz.hip and csrc/galois.hip.

Run with -s for the tables: the largest lazy product found per prime against the documented bound of mulvv_pm, the largest crafted
and random 20-term sums in units of q, and the share of slots whose folded sum enters the inverse transform at or above q.
Every figure printed here comes from the integer model on a CPU; no kernel runs."""
import random

import numpy as np
import pytest

import galois_oracle as go
import keyswitch_craft as kc
from test_pm_arithmetic_model import CLASSES, Pm, cls_of, mulvv_pm

N = 1024
N_RANDOM = 10 ** 5
PM_BASES = {"A": kc.BASES["A"][1], "B": kc.BASES["B"][1]}
FULL_SIZE = {"A": 7, "B": 12}                  # k x powers = 20 at dbc 60: 4 x 5 and 2 x 10
M32 = np.uint64(0xFFFFFFFF)


def mulvv_np(a, b, m):
    """mulvv_pm on uint64 arrays, limb for limb (every intermediate of the scalar model fits 64 bits, which its u64() assertions establish);
    used for the random measurement only and checked against the scalar model below"""
    S = np.uint64
    al, ah, bl, bh = a & M32, a >> S(32), b & M32, b >> S(32)
    P0 = al * bl
    mid = ah * bl + (al * bh + (P0 >> S(32)))
    top = ah * bh + (mid >> S(32))
    sh, mb, delta = S(m.sh), S(m.mb), S(m.delta)
    zh_lo = ((((top & M32) << S(32)) | (mid & M32)) >> sh) & M32
    zh_hi = (top >> sh) & M32
    zl = (P0 & M32) | (((mid & M32) & mb) << S(32))
    F = zh_lo * delta + zl
    G = zh_hi * delta + (F >> S(32))
    zh2 = (G >> sh) & M32
    lo = (F & M32) | (((G & M32) & mb) << S(32))
    return zh2 * delta + lo


@pytest.fixture(scope="module")
def oracles(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = oracle_mod.Oracle(N, PM_BASES[name], kc.T_PLAIN)
        return cache[name]
    return get


def _with_addends(orc, run, q, shape):
    """c0 / c1 complementing what `run(c01)` adds to zero c0 / c1"""
    return kc.final_addends(run(np.zeros(shape, dtype=np.uint64)), q)


@pytest.mark.parametrize("kind", kc.Uniform.KINDS)
@pytest.mark.parametrize("name,dbc", [("A", 60), ("A", 27), ("A", 11), ("B", 60), ("B", 30), ("B", 6)])
def test_model_equals_oracle_relinearize_and_galois(oracles, name, dbc, kind):
    """one key switch of family U: the model's per-slot values through the oracle's inverse transform and addition == Oracle.relinearize and
    galois_oracle.apply_galois, bit for bit, with c0 / c1 at the edges of the final addition"""
    orc, q = oracles(name), PM_BASES[name]
    u = kc.Uniform(q, N, dbc, 1, pm=True)
    assert kc.gate(u.k, u.nd) and u.k * u.nd <= kc.MAX_TERMS and not u.zero_digits
    key = u.key(kind)
    assert all(int(key[0, :, :, :, ii].max()) < q[ii] for ii in range(u.k))
    relin = lambda c01: orc.relinearize(u.ct(3, c01), key[0], dbc)
    c01 = _with_addends(orc, relin, q, (2, u.k, N))
    want = relin(c01)
    assert np.array_equal(u.model_relinearize(orc, key, c01), want)
    if kind == "zero1":
        assert np.array_equal(want[1], c01[1])                       # the accumulator of polynomial 1 is exactly zero
    # the final addition's four cases occur: results 0 and q - 1 where they were aimed at
    for ii in range(u.k):
        assert not want[:, ii, 2::4].any() and (want[:, ii, 3::4] == q[ii] - 1).all()
    for g, _, _ in go.elements(N):
        # sigma_g leaves the constant c1 alone; c0 is chosen so that sigma_g(c0) is the addend
        src = np.zeros((2, u.k, N), dtype=np.uint64)
        src[1, :, 0] = u.src
        assert np.array_equal(go.sigma(src, g, q), src)
        src[0] = go.sigma(c01[0], pow(g, -1, 2 * N), q)
        got = go.apply_galois(orc, src, g, key[0], dbc)
        assert np.array_equal(got, u.model_relinearize(orc, key, np.stack([c01[0], np.zeros_like(c01[0])])))


@pytest.mark.parametrize("name,size", [("A", 4), ("A", 7), ("A", 8), ("B", 4), ("B", 12), ("B", 13)])
def test_model_equals_oracle_relinearize_n(oracles, name, size):
    """evaluator.relinearize of a size-`size` ciphertext at dbc 60, pass by pass as fhe_relinearize_n groups them == Oracle.relinearize_n"""
    orc, q = oracles(name), PM_BASES[name]
    u = kc.Uniform(q, N, 60, size - 2, pm=True)
    key = u.key("crafted")
    relin = lambda c01: orc.relinearize_n(u.ct(size, c01), key, 60)
    c01 = _with_addends(orc, relin, q, (2, u.k, N))
    want = relin(c01)
    assert np.array_equal(u.model_relinearize(orc, key, c01), want)
    assert np.array_equal(u.model_relinearize(orc, key, c01, steps=True), want)
    assert (len(kc.passes(size, u.k, u.nd)) > 1) == (size > FULL_SIZE[name])       # sizes 8 and 13 split into passes


@pytest.mark.parametrize("name", ["A", "B"])
def test_every_lazy_product_and_every_sum_of_family_u_is_at_its_target(name):
    """dbc 60, 20 terms: every product of every (power, i, d, pp, ii, slot) is at or above q_ii, every sum at least terms x q_ii, the folded
    sum at or above q_ii in some slot of every target prime; the crafted sums are larger than any of 10^5 random ones.  0 targets left out"""
    q = PM_BASES[name]
    size = FULL_SIZE[name]
    u = kc.Uniform(q, N, 60, size - 2, pm=True)
    terms = u.k * u.nd * u.npow
    assert not u.zero_digits and u.src == [p - 1 for p in q]
    assert (u.k, u.nd, u.npow, terms) == ((4, 1, 5, 20) if name == "A" else (2, 1, 10, 20)) and kc.gate(u.k, u.nd, u.npow) and not kc.gate(u.k, u.nd, u.npow + 1)
    key = u.key("crafted")
    missed = 0
    for pw in range(u.npow):
        for i in range(u.k):
            for d in range(u.nd):
                for ii in range(u.k):
                    a, m = u.a[i][d][ii], u.mods[ii]
                    assert a == u.src[i] % q[ii] and a != 0
                    for e in set(key[pw, i, d, :, ii].reshape(-1).tolist()):
                        r = mulvv_pm(a, e, m)
                        assert r % m.q == a * e % m.q and 16 * r <= CLASSES[cls_of(m.q)]["RQ"] * m.q
                        missed += r < m.q
    assert missed == 0, "%d lazy products stay below q" % missed
    sums, folded, canon = u.slots(key)
    rng = np.random.default_rng(60)
    print()
    for ii in range(u.k):
        m = u.mods[ii]
        s_min, s_max = int(sums[:, ii].min()), int(sums[:, ii].max())
        assert s_min >= terms * m.q
        above = sum(int(v) >= m.q for v in folded[:, ii].reshape(-1))
        assert above > 0, "no slot of prime %d enters the inverse transform at or above q" % ii
        cnt = N_RANDOM // u.k
        rs = np.zeros(cnt, dtype=np.uint64)
        for _ in range(terms):
            rs += mulvv_np(rng.integers(0, m.q, cnt, dtype=np.uint64), rng.integers(0, m.q, cnt, dtype=np.uint64), m)
        r_max = int(rs.max())
        assert s_max > r_max and s_min > r_max
        print("[keyswitch U %s dbc=60 size=%d] prime %d (%d bits): %d-term sums crafted %.6f .. %.6f q, largest of %d random %.6f q; folded sum >= q in %d of %d slots (%.1f %%)"
              % (name, size, ii, m.b, terms, s_min / m.q, s_max / m.q, cnt, r_max / m.q, above, 2 * N, 100.0 * above / (2 * N)))


@pytest.mark.parametrize("q", PM_BASES["A"] + PM_BASES["B"])
def test_vectorised_product_is_the_scalar_model(q):
    m, rng = Pm(q), random.Random(q)
    a = [q - 1, 1, 0, (1 << (m.b + 1)) - 1] + [rng.randrange(1 << (m.b + 1)) for _ in range(300)]
    b = [q - 1, q - 1, 5, q - 1] + [rng.randrange(q) for _ in range(300)]
    got = mulvv_np(np.array(a, dtype=np.uint64), np.array(b, dtype=np.uint64), m)
    assert [int(x) for x in got] == [mulvv_pm(x, y, m) for x, y in zip(a, b)]
    # the bound the comment at mulvv_pm derives: 2^b + 2 delta^2 for a < 2^(b+1), 2^b + delta^2 for a canonical a
    assert all(int(r) < (1 << m.b) + (2 if x >= q else 1) * m.delta ** 2 for r, x in zip(got, a))


@pytest.mark.parametrize("name", ["A", "B"])
def test_largest_lazy_product_per_prime_is_recorded(name):
    """a record, not a threshold: the largest mulvv_pm(a, e) the search e = t a^-1, t < 2000, finds per (source, target) prime at dbc 60,
    against the documented bound 2^b + 2^(85-b) delta -- and, as a condition, every such search finds a product at or above q"""
    q = PM_BASES[name]
    print()
    for ii, qq in enumerate(q):
        m = Pm(qq)
        bound = (1 << m.b) + (m.delta << (85 - m.b))
        best = 0
        for i, qi in enumerate(q):
            found, (r, e) = kc.qualifying((qi - 1) % qq, m)
            assert found and r < bound
            best = max(best, r)
        rng = np.random.default_rng(ii)
        cnt = 200000
        rnd = mulvv_np(rng.integers(0, qq, cnt, dtype=np.uint64), rng.integers(0, qq, cnt, dtype=np.uint64), m)
        assert max(best, int(rnd.max())) < (1 << m.b) + m.delta ** 2 <= bound          # canonical operands: far inside the documented bound
        print("[keyswitch %s] prime %d = 2^%d - %d: largest crafted product %.6f q, largest of %d random %.6f q (%.3f %% at or above q); bound for canonical operands 2^b + delta^2 = %.6f q, documented bound %.4f q"
              % (name, ii, m.b, m.delta, best / qq, cnt, int(rnd.max()) / qq, 100.0 * float((rnd >= np.uint64(qq)).mean()), ((1 << m.b) + m.delta ** 2) / qq, bound / qq))


@pytest.mark.parametrize("name", list(kc.BASES))
def test_every_digit_pattern_of_family_d_occurs_where_the_rule_says_it_can(name):
    n, q, _, _ = kc.BASES[name]
    widths = sorted({p.bit_length() for p in q})
    rule = kc.dbc_rule(q)
    for b in widths:
        assert {b - 1, b, min(b + 1, 60)} <= set(rule)
    assert {1, 31, 32, 33, 60} <= set(rule)
    if name == "A":
        assert {27, 54, 11, 10} <= set(rule)
    if name == "B":
        assert {6, 5} <= set(rule)
    if name.startswith("P4096"):
        assert 36 in rule
    for dbc in rule:
        nd = kc.digits(q, dbc)
        src, targets = kc.digit_sources(q, n, dbc)
        assert src.shape == (3 + n.bit_length() - 1, len(q), n)
        full = (1 << dbc) - 1
        for i, qi in enumerate(q):
            assert int(src[:, i].max()) < qi
            ndi = -(-qi.bit_length() // dbc)
            col = [int(v) for v in src[0, i]]
            seen = {(d, kc.digit_of(v, dbc, d)) for j, v in enumerate(col[:-1]) for d in [targets[i][j % len(targets[i])][0]]}
            assert set(targets[i]) <= seen and col[-1] == 0
            want = set()
            for d in range(ndi):
                cap = full if d < ndi - 1 else (qi - 1) >> (dbc * d)
                want |= {(d, v) for v in (0, 1, full - 1, full) if v <= cap}
                want |= {(d, qq + s) for qq in q if dbc >= qq.bit_length() for s in (-1, 0, 1) if qq + s <= cap}
            want.add((ndi - 1, (qi - 1) >> (dbc * (ndi - 1))))
            for qq in q:
                if qq.bit_length() < qi.bit_length():
                    above = ((qq - 1) >> (dbc * (ndi - 1))) + 1
                    if above <= (qi - 1) >> (dbc * (ndi - 1)):
                        want.add((ndi - 1, above))
            assert want <= set(targets[i]), (name, dbc, i, sorted(want - set(targets[i])))
            # a prime narrower than the widest: its digits above its own top one are zero in every coefficient
            for d in range(ndi, nd):
                assert not any(kc.digit_of(v, dbc, d) for v in col)
            # the whole-polynomial patterns: all ones below the top digit, or q_i - 1 where that leaves no top digit
            top = int(src[1, i, 0])
            assert top == kc.max_source(qi, dbc) and (top == qi - 1 or all(kc.digit_of(top, dbc, d) == full for d in range(ndi - 1)))
            assert not src[2, i, 1::2].any() and (src[2, i, 0::2] == top).all()
            for b in range(n.bit_length() - 1):
                on = (np.arange(n) >> b) & 1 == 1
                assert (src[3 + b, i][on] == top).all() and not src[3 + b, i][~on].any()
        # the direct Galois form: the kernel's negation gives the pattern back, 0 stays 0
        for g, _, _ in go.elements(n):
            direct = kc.direct_form(src[0], g, q)
            neg = kc.negated_positions(n, g)
            for i, qi in enumerate(q):
                seen_by_kernel = np.where(neg & (direct[i] != 0), np.uint64(qi) - direct[i], direct[i])
                assert np.array_equal(seen_by_kernel, src[0, i]) and neg.any() and int(direct[i].max()) < qi
            assert np.array_equal(go.sigma(go.sigma(src[:2], pow(g, -1, 2 * n), q), g, q), src[:2])


def test_restated_gate_and_pass_grouping_agree_with_the_header_comments():
    """csrc/behz.hip fhe_relinearize_n on the P8192 primes: one pass at dbc 60 up to size 7, two at size 8; all at once for a Cubic's size-4
    result at dbc 30 too, and two passes of two powers at dbc 30 for size 6"""
    q = PM_BASES["A"]
    nd60, nd30 = kc.digits(q, 60), kc.digits(q, 30)
    assert (nd60, nd30) == (1, 2)
    for size in range(3, 8):
        assert kc.passes(size, 4, nd60) == ([(2, size - 1)] if size > 3 else [(2, 2)])
    assert kc.passes(8, 4, nd60) == [(3, 7), (2, 2)]
    assert kc.passes(4, 4, nd30) == [(2, 3)]
    assert kc.passes(6, 4, nd30) == [(4, 5), (2, 3)]
    assert kc.passes(5, 4, nd30) == [(3, 4), (2, 2)]
    assert kc.passes(6, 4, nd30, steps=True) == [(5, 5), (4, 4), (3, 3), (2, 2)] == kc.passes(6, 4, nd30, pm=False)
    qb = PM_BASES["B"]
    assert kc.passes(12, 2, kc.digits(qb, 60)) == [(2, 11)] and kc.passes(13, 2, kc.digits(qb, 60)) == [(3, 12), (2, 2)]
    assert kc.twenty_term_dbc(q) == 11 and kc.twenty_term_dbc(qb) == 6
    # a pass's polynomials partition 2 .. size - 1, from the top
    for size in range(3, 16):
        for nd in (1, 2, 3, 5):
            flat = [p for lo, hi in kc.passes(size, 4, nd) for p in range(hi, lo - 1, -1)]
            assert flat == list(range(size - 1, 1, -1))
            assert all(kc.gate(4, nd, hi - lo + 1) or hi == lo for lo, hi in kc.passes(size, 4, nd))

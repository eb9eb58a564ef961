"""CPU: the specification of the key switch with a special prime (tests/keyswitch_sp_oracle.py) -- its residue form on the oracle's
transforms agrees with its big-integer form on every base the GPU tests use; a toy BFV in Python integers relinearises and rotates
through it, decrypts, and keeps the budget circuits.special_key_switch_budget promises; the crafted operand families reach their targets
in the model of the kernels' arithmetic, and the wrong variants of that arithmetic are caught."""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

import galois_oracle as go
import keyswitch_sp_oracle as ks
import modswitch_oracle as mo
import packed_oracle as po

BASES = mo.bases(1024)                     # Q3 (P4096), Q4 (P8192), Q58, Q61, Q61R, S16K: the last prime of each is the special prime
PM_BASES = ("Q4", "Q58", "S16K")           # the bases whose key switch runs the pseudo-Mersenne kernels
N_SMALL = 64
_orc = {}


def _oracle(om, name, n=N_SMALL):
    if (name, n) not in _orc:
        _orc[(name, n)] = om.Oracle(n, BASES[name], go.T_BATCH)
    return _orc[(name, n)]


def _ternary(rng, q, n):
    v = rng.integers(0, 3, size=n)
    return np.stack([np.where(v == 2, qi - 1, v).astype(np.uint64) for qi in q])


def _random_ct(rng, q, size, n):
    return np.stack([np.stack([rng.integers(0, qi, size=n, dtype=np.uint64) for qi in q]) for _ in range(size)])


# ---- (a) the forms agree ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BASES))
def test_residue_form_equals_the_big_integer_form(oracle_mod, name):
    q, n = BASES[name], N_SMALL
    L = len(q) - 1
    orc = _oracle(oracle_mod, name)
    rng = np.random.default_rng(len(name))
    sk = _ternary(rng, q, n)
    kc = ks.switch_key(orc, sk, ks.secret_powers(orc, sk, 1)[0], seed=3)
    ko = ks.key_to_oracle(orc, kc)
    ct = _random_ct(rng, q[:-1], 3, n)
    ct[2, :, :4] = [[0, 1, qi - 1, qi - 2] for qi in q[:-1]]
    u = ks.key_switch(orc, ct[2], ko)
    assert u.shape == (2, L, n) and np.array_equal(u, ks.key_switch_big(q, ct[2], kc)), name
    got = ks.relinearize_poly(orc, ct, 2, ko)
    want = np.array([[[(int(ct[pp, r, c]) + int(u[pp, r, c])) % q[r] for c in range(n)] for r in range(L)] for pp in range(2)], dtype=np.uint64)
    assert np.array_equal(got, want)
    for g in (3, 2 * n - 1, pow(3, n // 8, 2 * n)):
        target = go.sigma(sk, g, q)
        gc = ks.switch_key(orc, sk, target, seed=g)
        sig = np.array([[ks.sigma_big([int(x) for x in ct[pp, r]], g, q[r]) for r in range(L)] for pp in range(2)], dtype=np.uint64)
        assert np.array_equal(sig, go.sigma(ct[:2], g, q[:-1]))
        ub = ks.key_switch_big(q, sig[1], gc)
        want = np.stack([np.array([[(int(sig[0, r, c]) + int(ub[0, r, c])) % q[r] for c in range(n)] for r in range(L)], dtype=np.uint64), ub[1]])
        assert np.array_equal(ks.apply_galois(orc, ct[:2], g, ks.key_to_oracle(orc, gc)), want), (name, g)


# ---- (b) a toy BFV in Python integers -----------------------------------------------------------------------------------------------------
def _exact_budget(Q, worst):
    return math.log2(Q) - math.log2(worst) - 1 if worst else float("inf")


def _worst(polys, s, Q, t):
    acc = [0] * len(s)
    for c in reversed(polys):
        acc = [(u + v) % Q for u, v in zip(mo.negacyclic_mul(acc, s, Q), c)]
    out, plain = 0, []
    for x in acc:
        m = (t * x + Q // 2) // Q
        out = max(out, abs(t * x - m * Q))
        plain.append(m % t)
    return out, plain


def _centre(v, Q):
    return v - Q if v > Q // 2 else v


def _signed_mul(a, b):
    """the negacyclic product over the integers"""
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            if i + j < n:
                out[i + j] += x * y
            else:
                out[i + j - n] -= x * y
    return out


def _toy_key(rng, q, s, target, B):
    """K [L][2][n] modulo Q p: (-(a s + e) + P_i target, a), P_i = p (Q / q_i) [(Q / q_i)^-1]_(q_i), |e| <= B"""
    n, Qp, p, Q = len(s), mo.prod(q), q[-1], mo.prod(q[:-1])
    K = []
    for i in range(len(q) - 1):
        a = [int.from_bytes(rng.bytes(48), "little") % Qp for _ in range(n)]
        e = [int(v) for v in rng.integers(-B, B + 1, size=n)]
        Pi = p * (Q // q[i]) * pow(Q // q[i], -1, q[i])
        as_ = mo.negacyclic_mul(a, s, Qp)
        K.append([[(-(x + y) + Pi * z) % Qp for x, y, z in zip(as_, e, target)], a])
    return K


def _encrypt(rng, m, s, Q, t, noise=8):
    n = len(s)
    c1 = [int.from_bytes(rng.bytes(48), "little") % Q for _ in range(n)]
    e = [int(v) for v in rng.integers(-noise, noise + 1, size=n)]
    c1s = mo.negacyclic_mul(c1, s, Q)
    return [[(Q // t * mi + ei - x) % Q for mi, ei, x in zip(m, e, c1s)], c1]


@pytest.mark.parametrize("name,t", [("Q3", 65537), ("Q4", 65537), ("Q4", po.T33)])
def test_toy_bfv_relinearises_and_rotates_within_the_noise_bound(fhe, name, t):
    """n = 32, a ternary secret: the product of two encryptions relinearised, and an encryption rotated by three Galois elements, decrypt to
    the expected plaintexts, and the EXACT invariant budget after each key switch is at least special_key_switch_budget of the exact
    budget before (noise_bound=None: the keys' noise is drawn up to the library sampler's own largest value)"""
    B = fhe.package.keys._Sampler.NOISE_MAX
    q, n = BASES[name], 32
    ctx = SimpleNamespace(n=n, t=t, q=q, k=len(q))
    Q = mo.prod(q[:-1])
    rng = np.random.default_rng(t % 1000)
    s = [int(v) - 1 for v in rng.integers(0, 3, size=n)]
    m1, m2 = ([int(v) for v in rng.integers(0, t, size=n)] for _ in range(2))
    a, b = _encrypt(rng, m1, s, Q, t), _encrypt(rng, m2, s, Q, t)
    ac, bc = [[_centre(v, Q) for v in p] for p in a], [[_centre(v, Q) for v in p] for p in b]
    rnd = lambda poly: [((2 * t * v + Q) // (2 * Q)) % Q for v in poly]                                   # round(t v / Q)
    cross = [x + y for x, y in zip(_signed_mul(ac[0], bc[1]), _signed_mul(ac[1], bc[0]))]
    prod3 = [rnd(_signed_mul(ac[0], bc[0])), rnd(cross), rnd(_signed_mul(ac[1], bc[1]))]
    want = mo.negacyclic_mul(m1, m2, t)
    worst, plain = _worst(prod3, s, Q, t)
    assert plain == want
    before = _exact_budget(Q, worst)
    s2 = _signed_mul(s, s)
    K = _toy_key(rng, q, s, s2, B)
    d = [[v % qi for v in prod3[2]] for qi in q[:-1]]
    u = ks.key_switch_composed(q, d, K)
    relin = [[(x + y) % Q for x, y in zip(prod3[pp], u[pp])] for pp in range(2)]
    worst, plain = _worst(relin, s, Q, t)
    after, bound = _exact_budget(Q, worst), fhe.circuits.special_key_switch_budget(ctx, before)
    lines = ["relinearise %.1f -> %.1f bits (bound %.1f)" % (before, after, bound)]
    assert plain == want and after >= bound - 1e-9, lines
    worst, plain = _worst(a, s, Q, t)
    assert plain == m1
    fresh = _exact_budget(Q, worst)
    for g in (3, 2 * n - 1, pow(3, n // 8, 2 * n)):
        sg = [_centre(v, 3) for v in ks.sigma_big([v % 3 for v in s], g, 3)]
        K = _toy_key(rng, q, s, sg, B)
        sig = [ks.sigma_big(p, g, Q) for p in a]
        u = ks.key_switch_composed(q, [[v % qi for v in sig[1]] for qi in q[:-1]], K)
        rot = [[(x + y) % Q for x, y in zip(sig[0], u[0])], u[1]]
        worst, plain = _worst(rot, s, Q, t)
        after, bound = _exact_budget(Q, worst), fhe.circuits.special_key_switch_budget(ctx, fresh)
        lines.append("g=%d %.1f -> %.1f bits (bound %.1f)" % (g, fresh, after, bound))
        assert plain == ks.sigma_big(m1, g, t), g
        assert after >= bound - 1e-9, lines
    print("\n[toy BFV special prime %s t=%d n=%d B=%d] %s" % (name, t, n, B, "; ".join(lines)))


def test_budget_formula(fhe):
    c = fhe.circuits
    B19 = fhe.package.keys._Sampler.NOISE_MAX
    import ctypes as C
    cdt = (C.c_uint64 * 19)()
    fhe._lib.load().fhe_noise_cdt(cdt)
    assert B19 == len(cdt)                                             # both samplers of the library stop at the same magnitude
    for q, n, t in ((BASES["Q4"], 8192, 65537), (BASES["Q3"], 4096, 65537), (BASES["S16K"], 16384, po.T33)):
        ctx = SimpleNamespace(n=n, t=t, q=q)
        p, Q = q[-1], mo.prod(q[:-1])
        for budget in (20, 77.5, 140):
            for B in (None, 3):
                E = Fraction(n * (B19 if B is None else B) * sum(qi - 1 for qi in q[:-1]), p) + Fraction(1 + n, 2)
                want = -math.log2(Fraction(2.0 ** -budget) + 2 * t * E / Q)
                got = c.special_key_switch_budget(ctx, budget, B)
                assert got == pytest.approx(want, abs=1e-6) and got <= budget + 1e-9
        print("[special_key_switch_budget n=%d k=%d] a switch at %d bits keeps %.2f" % (n, len(q), 100, c.special_key_switch_budget(ctx, 100)))
    with pytest.raises(ValueError):
        c.special_key_switch_budget(SimpleNamespace(n=1024, t=65537, q=BASES["Q3"][:1]), 50)


# ---- (c) the crafted families reach their targets in the model ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BASES))
def test_reduction_edges_are_reached(name):
    q, n = BASES[name], 1024
    L = len(q) - 1
    for g in (None, 3, 2 * n - 1, pow(3, n // 8, 2 * n)):
        poly = ks.reduction_poly(q, n, g)
        neg = (np.arange(n, dtype=np.int64) * g % (2 * n)) >= n if g is not None else np.zeros(n, dtype=bool)
        for i in range(L):
            vals = set(ks.reduction_values(q, i))
            assert {0, 1, q[i] - 1} <= vals and all(v < q[i] for v in vals)
            for r, qr in enumerate(q):
                if r != i:
                    assert {v for v in (qr - 1, qr, qr + 1, 2 * qr) if v < q[i]} <= vals
            assert all(int(v) < q[i] for v in poly[i])
            seen = {(ks.load_model(int(poly[i, j]), bool(neg[j]), q[i], q[i]), bool(neg[j])) for j in range(n)}      # the value sigma_g hands on, modulo q_i
            if g is None:
                assert vals <= {v for v, _ in seen}, (name, i)
            else:
                assert vals <= {v for v, ng in seen if ng}, (name, g, i)      # every edge value is produced BY a negation


@pytest.mark.parametrize("name", list(BASES))
def test_drop_edges_are_reached(name):
    """family D: acc_pp is modswitch_oracle.crafted_tile itself; the drop of the special prime sees every prescribed remainder and final
    residue, and the final addends make the last addmod give exactly 0 and q_r - 1"""
    q, n = BASES[name], 1024
    k = len(q)
    tiles = ks.drop_tiles(q, n)
    for pp in range(2):
        crafted = mo.craft(q, k - 1, seed=pp)
        assert len(crafted) <= n
        reached = set()
        for c, (res, what) in enumerate(crafted):
            assert [int(tiles[pp, r, c]) for r in range(k)] == res
            got = [ks.drop_model(res[r], res[-1], q, r) for r in range(k - 1)]
            assert got == mo.switch_big(res, q, k - 1)
            if what[0] == "r":
                _, m, rt, ct = what
                assert m == k - 1 and (res[-1] + q[-1] // 2) % q[-1] == mo._r_value(rt, q[-1])
                assert got == [mo._c_value(ct, q[r]) for r in range(k - 1)]
                reached.add((rt, ct))
        assert reached == {(rt, ct) for rt in mo.R_TARGETS for ct in mo.C_TARGETS}
        u = mo.switch_residues_levels(tiles[pp], q)[k - 1]
        add = ks.final_addends(u, q)
        for r in range(k - 1):
            s = (add[r].astype(object) + u[r].astype(object)) % q[r]
            assert set(s[2::4]) == {0} and set(s[3::4]) == {q[r] - 1} and set(add[r][0::4]) == {0} and set(add[r][1::4]) == {q[r] - 1}


@pytest.mark.parametrize("name", PM_BASES)
def test_lazy_sums_are_above_q_in_every_term(name):
    """family U: every one of the L mulvv_pm terms of every slot is at or above q_r, their integer sum stays in 64 bits and its fold is the
    canonical sum plus at most one q_r"""
    import keyswitch_craft as kc
    from test_pm_arithmetic_model import Pm, fold_pm
    q = BASES[name]
    U = ks.Uniform(q, 1024, pm=True)
    key = U.key()
    for r, qr in enumerate(q):
        m = Pm(qr)
        for pp in range(2):
            for s in range(0, 1024, 37):
                terms = [(U.a[i][r], int(key[i, pp, r, s])) for i in range(U.L)]
                prods = [kc.lazy_product(a, e, m) for a, e in terms]
                assert all(v >= qr for v in prods), (name, r, s)
                total = sum(prods)
                assert total < 1 << 64
                f = fold_pm(total, m)
                assert f % qr == sum(a * e for a, e in terms) % qr and f < 2 * qr


# ---- (d) wrong variants, in the model only ------------------------------------------------------------------------------------------------
def test_wrong_variants_are_caught(oracle_mod):
    """(changed crafted outputs, crafted outputs, changed random outputs, random outputs) per variant:
         gt_final     `>` for `>=` in the last conditional subtraction of the drop: family D's coefficients whose result is 0; random 0
         neg0         the negation of 0 gives q_i: family R's zeros at negated positions; random data holds no zero
         raw_d        [d_i]_(q_r) taken as d_i: family R's values at and above q_r
         p_everywhere P_i T added on every component: any data
         neg_qr       the negation modulo q_r instead of q_i: any data"""
    rng = np.random.default_rng(5)
    report = {}
    # gt_final on the 58-bit pair
    q, n = BASES["Q58"], 1024
    tile = ks.drop_tiles(q, n)[0]
    crafted = [(int(tile[0, c]), int(tile[1, c])) for c in range(n)]
    rand = [(int(rng.integers(0, q[0])), int(rng.integers(0, q[1]))) for _ in range(20000)]
    cnt = lambda ops: sum(ks.drop_model(x, cp, q, 0, "gt_final") != ks.drop_model(x, cp, q, 0) for x, cp in ops)
    report["gt_final"] = (cnt(crafted), len(crafted), cnt(rand), len(rand))
    # neg0 / raw_d / neg_qr on {55-bit, 61-bit} and {61-bit, 55-bit}: a residue reduced to a larger and to a smaller prime
    for variant in ("neg0", "raw_d", "neg_qr"):
        c_bad = c_all = r_bad = r_all = 0
        for name in ("Q61", "Q61R", "Q4"):
            q = BASES[name]
            g = 2 * n - 1
            poly = ks.reduction_poly(q, n, g)
            neg = (np.arange(n, dtype=np.int64) * g % (2 * n)) >= n
            for i in range(len(q) - 1):
                rvals = rng.integers(0, q[i], size=n, dtype=np.uint64)
                for r, qr in enumerate(q):
                    if r == i:
                        continue
                    for j in range(n):
                        c_bad += ks.load_model(int(poly[i, j]), bool(neg[j]), q[i], qr, variant) != ks.load_model(int(poly[i, j]), bool(neg[j]), q[i], qr)
                        r_bad += ks.load_model(int(rvals[j]), bool(neg[j]), q[i], qr, variant) != ks.load_model(int(rvals[j]), bool(neg[j]), q[i], qr)
                    c_all, r_all = c_all + n, r_all + n
        report[variant] = (c_bad, c_all, r_bad, r_all)
    # p_everywhere: the wrong key through the specification itself
    orc = _oracle(oracle_mod, "Q4")
    q = BASES["Q4"]
    sk = _ternary(rng, q, N_SMALL)
    target = ks.secret_powers(orc, sk, 1)[0]
    good, bad = (ks.key_to_oracle(orc, ks.switch_key(orc, sk, target, seed=2, variant=v)) for v in (None, "p_everywhere"))
    d = _random_ct(rng, q[:-1], 1, N_SMALL)[0]
    diff = int((ks.key_switch(orc, d, good) != ks.key_switch(orc, d, bad)).sum())
    report["p_everywhere"] = (None, None, diff, 2 * 3 * N_SMALL)
    print("\n[key switch, special prime: wrong variants] variant: (crafted changed, crafted, random changed, random) = %r" % report)
    assert report["gt_final"][0] > 0 and report["gt_final"][2] == 0
    assert report["neg0"][0] > 0 and report["neg0"][2] == 0
    assert report["raw_d"][0] > 0
    assert report["p_everywhere"][2] > N_SMALL
    assert report["neg_qr"][2] > report["neg_qr"][3] // 2 and report["neg_qr"][0] > 0


# ---- (e) the library ----------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points(fhe):
    lib = fhe._lib.load()
    for name in ("fhe_ksk_sp_words", "fhe_key_switch_sp_scratch_bytes", "fhe_relinearize_sp_poly", "fhe_apply_galois_sp"):
        assert hasattr(lib, name) and name in fhe._lib.SIGNATURES and name in open(fhe.HEADER_PATH).read(), name
    assert lib.fhe_ksk_sp_words(None) == 0 and lib.fhe_key_switch_sp_scratch_bytes(None, 3) == 0
    assert lib.fhe_relinearize_sp_poly(None, None, 0, 2, None, 0, 1, None, None, 0, None) == -1
    assert lib.fhe_apply_galois_sp(None, None, 0, None, 0, 1, 3, None, None, 0, None) == -1

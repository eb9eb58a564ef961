"""CPU: the scalar restatement of the BEHZ product (tests/behz_craft.py) equals the big-integer model and the C oracle, and the
operands crafted with it reach -- in the model, as conditions -- the values they are aimed at.  tests/test_gpu_behz_extremes.py
runs the same operands through the kernels of csrc/behz.hip.

Run with -s for the tables: per base the floor value of the maximal products against B m_sk / 2, and the Shenoy-Kumaresan
correction alpha_sk they need (far above k: alpha_sk ~ -v / B).

The big-integer model and whole-polynomial scalar products are Python loops over n k values, so they run at n = 256 (N_WHOLE):
steps 0, 1, 3 and 4 are per coefficient and do not know n; the auxiliary base stays the one the library picks for the base's own n.
The per-coefficient checks against the C oracle run at the base's own n."""
import math
import random

import numpy as np
import pytest

import behz_craft as bc
from oracle.bigint_model import Model, polymul_negacyclic

N_RANDOM = 10 ** 5
N_WHOLE = 256
# (sa, sb) of the maximal products of test_gpu_behz_extremes.py; sa == sb == 5 is a square
MAGNITUDE_SIZES = {name: [(2, 2), (3, 2), (5, 5)] + ([(12, 12), (13, 13)] if name in ("SMALL", "Q61x5-n1024") else []) for name in bc.BASES}
MAGNITUDE_SIZES["SEAL23_16384"] = [(2, 2)]


class Base:
    def __init__(self, om, name):
        self.name = name
        self.n, self.q, self.t = bc.BASES[name]
        self.k = len(self.q)
        self.aux = bc.library_aux(self.q, self.t, self.n)
        self.sc = bc.Scalar(self.q, self.t, self.aux)
        self.n_cpu = N_WHOLE
        self.orc = om.Oracle(self.n_cpu, self.q, self.t)
        self.model = Model(self.n_cpu, self.q, self.t)
        self.lift = bc.lift_cases(self.q, self.n_cpu)
        self.floor_y = bc.floor_y_cases(self.q, self.t, self.n_cpu)
        self.floor_z = bc.floor_z_cases(self.q, self.t, self.aux, self.n_cpu)
        self.floor_z_extra = bc.floor_z_extra_cases(self.q, self.t, self.aux, self.n_cpu)

    def crafted_coefficients(self, aux=None):
        """(builder's label, residues, c) of every crafted coefficient of polynomial 0"""
        fz = self.floor_z if aux is None else bc.floor_z_cases(self.q, self.t, aux, self.n_cpu)
        extra = self.floor_z_extra if aux is None else bc.floor_z_extra_cases(self.q, self.t, aux, self.n_cpu)
        for (a, labels), c in [(self.lift, 1), (self.floor_y, 1), (fz[:2], fz[2])] + [(x[:2], x[2]) for x in extra[0]]:
            for (poly, pos), label in labels.items():
                if poly == 0:
                    assert np.array_equal(a[0, :, pos], a[1, :, self.n_cpu - 1 - pos])       # polynomial 1 mirrors polynomial 0
                    yield label, [int(x) for x in a[0, :, pos]], c


@pytest.fixture(scope="module")
def bases(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Base(oracle_mod, name)
        return cache[name]
    return get


def test_the_auxiliary_base_is_the_one_fhe_behz_build_picks(oracle_mod):
    """58-bit primes when 57 (k + 1) bits cover bits(q) + bits(t) + log2 n + 12, else 61-bit ones; the boundary base sits exactly on
    the rule at n = 1024 and one past it at n = 2048, where the candidates that ARE its q-primes are skipped (as in the C oracle)"""
    for name, (n, q, t) in bc.BASES.items():
        aux, k = bc.library_aux(q, t, n), len(q)
        assert aux["bits"] == (61 if name == "Q61x5-n2048" else 58), name
        for p in [aux["msk"]] + aux["b"]:
            assert bc.is_prime(p) and p % (1 << 17) == 1 and p.bit_length() == aux["bits"] and p not in q
        assert aux["msk"] > aux["b"][0] and aux["b"] == sorted(aux["b"], reverse=True) and len(aux["b"]) == k
        forced, orc = bc.library_aux(q, t, n, aux61=True), oracle_mod.Oracle(N_WHOLE, q, t)
        assert forced == bc.seal_aux(q) and orc.aux == forced["b"] + [forced["msk"]], name
    n, q, t = bc.BASES["Q61x5-n1024"]
    assert bc.aux_need(q, t, n) == 342 == 57 * 6 and bc.aux_need(q, t, 2048) == 343
    assert all(p.bit_length() == 61 and p % (1 << 17) == 1 for p in q)
    assert max(bc.seal_aux(q)["b"] + [bc.seal_aux(q)["msk"]]) < min(q)          # all five leading candidates were skipped
    assert bc.library_aux(bc.SMALL_Q, t, 1024)["msk"] == bc.primes_below(58, 1)[0] == 0x3FFFFFFFFBE0001
    from test_pm_arithmetic_model import AUX_B, aux_primes                     # the same search, as the range-plan model states it
    assert bc.primes_below(58, 9) == AUX_B and bc.primes_below(61, 3) == aux_primes(3, 61)


def _same(b, x, y):
    """scalar model == big-integer model == C oracle on one product, coefficient for coefficient"""
    want = b.orc.square(x) if y is None else b.orc.multiply(x, y)
    got, _ = b.sc.multiply(x, x if y is None else y)
    mx = b.model.from_rns(x.tolist())
    big = np.array(b.model.to_rns(b.model.multiply(mx, mx if y is None else b.model.from_rns(y.tolist()))), dtype=np.uint64)
    assert np.array_equal(got, want), "scalar model against the C oracle"
    assert np.array_equal(big, want), "big-integer model against the C oracle"


@pytest.mark.parametrize("name", list(bc.BASES))
def test_scalar_model_equals_the_bigint_model_and_the_oracle(bases, name):
    """on every crafted operand.  The scalar model runs on the library's auxiliary base, the C oracle on SEAL's 61-bit one, the
    big-integer model on none: the product does not depend on the base."""
    b = bases(name)
    rnd = b.orc.random_ct(1, seed=97)[0]
    one = bc.constant_ct(b.q, b.n_cpu, 1)
    a, _ = b.lift
    _same(b, a, rnd)
    _same(b, a, None)
    _same(b, b.floor_y[0], one)
    az, _, c, _ = b.floor_z
    _same(b, bc.constant_ct(b.q, b.n_cpu, c), az)
    for ax, _, cx in b.floor_z_extra[0]:
        _same(b, ax, bc.constant_ct(b.q, b.n_cpu, cx))
    lo, hi = bc.magnitude_cases(b.q, b.n_cpu, 3)
    _same(b, lo, hi[:2])
    _same(b, lo[:2], None)


@pytest.mark.parametrize("name", list(bc.BASES))
def test_crafted_coefficients_at_the_base_size_equal_the_oracle(oracle_mod, bases, name):
    """the operands as the GPU test builds them, at the base's own n: the C oracle's product with (c, 0), in both orders, is the
    scalar model's result at every crafted coefficient and at 64 coefficients of the padding"""
    b = bases(name)
    orc = oracle_mod.Oracle(b.n, b.q, b.t)
    fy, fz = bc.floor_y_cases(b.q, b.t, b.n), bc.floor_z_cases(b.q, b.t, b.aux, b.n)
    for (a, labels), c in [(fy, 1), (fz[:2], fz[2])] + [(x[:2], x[2]) for x in bc.floor_z_extra_cases(b.q, b.t, b.aux, b.n)[0]]:
        cc = bc.constant_ct(b.q, b.n, c)
        want = orc.multiply(a, cc)
        assert np.array_equal(want, orc.multiply(cc, a))
        assert not want[2].any()
        for poly, pos in list(labels) + [(p, b.n // 2 + 5 * i) for p in (0, 1) for i in range(32)]:
            _, fl = b.sc.coefficient([int(x) for x in a[poly, :, pos]], c)
            assert [int(x) for x in want[poly, :, pos]] == fl["result"], (name, poly, pos)


def _check_targets(b, aux, wanted_z):
    sc = b.sc if aux is None else bc.Scalar(b.q, b.t, aux)
    hit = set()
    for label, a, c in b.crafted_coefficients(aux):
        lf, fl = sc.coefficient(a, c)
        here = bc.labels_of(lf if label.startswith("lift") else None, fl, sc)
        assert label in here, "%s: the coefficient built for %s reaches only %s" % (b.name, label, sorted(here))
        hit |= here
    z_targets = bc.floor_z_targets(b.q, b.t, aux or b.aux)
    assert len(z_targets) == wanted_z == 12 * b.k
    missed = set(bc.lift_targets(b.k) + bc.floor_y_targets(b.k) + z_targets) - hit
    assert not missed, "%s: targets no coefficient reaches: %s" % (b.name, sorted(missed))


@pytest.mark.parametrize("name", list(bc.BASES))
def test_every_target_is_hit(bases, name):
    """the labels are read off the model's intermediates (behz_craft.labels_of), not taken from the builders: every y_i of both
    stages at 0, 1, q_i - 2, q_i - 1 and on both sides of 2^28 and 2^29, all y_i at q_i - 1 and at 0, the six remainders r, both
    signs of v, and every z_j at 0, 1, b_j - 2, b_j - 1 and on both sides of 2^29 under both signs of v -- 12 k targets on every base.
    On the single 54-bit prime six of the twelve (|v| near b_0) lie outside the sweep of the shared constant 2^s and have a constant
    of their own each (behz_craft.floor_z_extra_cases).  Prints the largest number of model evaluations a z_j target took."""
    b = bases(name)
    _check_targets(b, None, 12 * b.k)
    print("\n[%s] z_j targets: %d with c = 2^%d (at most %d model evaluations each), %d with a constant of their own (at most %d)"
          % (name, len(b.floor_z[1]) // 2, b.floor_z[2].bit_length() - 1, b.floor_z[3], len(b.floor_z_extra[0]), b.floor_z_extra[1]))
    if name in ("SEAL23_4096", "P8192"):                       # FHE_BEHZ_AUX61: the z_j targets rebuilt for the 61-bit base
        _check_targets(b, bc.library_aux(b.q, b.t, b.n, aux61=True), 12 * b.k)


def _alpha_floor(b, s=None):
    """a lower bound of |alpha_sk| in the largest maximal product of the base, from the formats alone: |v| >= s n t q / 8, conv < k B"""
    s = max(min(sa, sb) for sa, sb in MAGNITUDE_SIZES[b.name]) if s is None else s
    return s * b.n * b.t * b.sc.Q // 8 // b.sc.B - b.k


def _maximal_D(b):
    H = b.sc.Q // 2
    return [d for sa, sb in MAGNITUDE_SIZES[b.name] for d in (bc.magnitude_D(H, H, sa, sb, b.n)[min(sa, sb) - 1][i] for i in (0, b.n - 1))]


@pytest.mark.parametrize("name", list(bc.BASES))
def test_wrong_models_change_crafted_results_and_no_random_one(bases, name):
    """each deliberately wrong restatement (behz_craft.Scalar) differs from the right one on at least one crafted coefficient -- the
    crafted operands against (1, 0) or (c, 0), or a coefficient of a maximal product -- and on none of 10^5 seeded random ones (random
    residues against (1, 0) and (c, 0) alternately): what the crafted set sees, this random data does not.  (For alpha_byte that holds
    for scalar operands only -- products of two random ciphertexts have large alpha_sk and do see it; see behz_craft.Scalar.)  A variant of the lift is
    compared through lift() -- floor() is then the same function of the same D -- and a variant of the floor through floor()."""
    b = bases(name)
    wrong = {v: bc.Scalar(b.q, b.t, b.aux, v) for v in bc.VARIANTS
             if not (v == "lift_y_keeps_q" and b.k == 1) and not (v == "alpha_byte" and _alpha_floor(b) < 128)}
    assert len(wrong) >= 3
    crafted = list(b.crafted_coefficients())
    for v, w in wrong.items():
        seen = [label for label, a, c in crafted if w.coefficient(a, c)[1]["result"] != b.sc.coefficient(a, c)[1]["result"]]
        seen += ["maximal D = %d" % d for d in _maximal_D(b) if w.floor(d)["result"] != b.sc.floor(d)["result"]]
        assert seen, "%s: no crafted coefficient tells %s from the right model" % (name, v)
        print("[%s] %s is seen by %d crafted coefficients, the first: %s" % (name, v, len(seen), seen[0][:60]))
    rnd, cz = random.Random(2026), b.floor_z[2]
    for i in range(N_RANDOM):
        a = [rnd.randrange(p) for p in b.q]
        lf = b.sc.lift(a)
        D = lf["value"] * (cz if i & 1 else 1)
        res = b.sc.floor(D)["result"]
        for v, w in wrong.items():
            if v in bc.LIFT_VARIANTS:
                assert w.lift(a)["value"] == lf["value"], (name, v, a)
            else:
                assert w.floor(D)["result"] == res, (name, v, a)


@pytest.mark.parametrize("name", list(bc.BASES))
def test_maximal_products_reach_the_magnitude_bound(bases, name):
    """every coefficient floor(q/2): lift(floor(q/2)) == floor(q/2), so the middle polynomial of an sa x sb product has
    D_(n-1) = + s n H^2 and D_0 = -s (n - 2) H^2 with s = min(sa, sb) terms: |v| is within one bit of s n t q / 4, the value the 58-bit
    against 61-bit rule of fhe_behz_build is derived from.  alpha_sk = (conv - v) / B with 0 <= conv < k B, so it is about -v / B: far
    above k wherever s n t q / 8 exceeds (2 k + 1) B -- every base but SMALL (109 bits of q against 174 of B) and the 2 x 2 product of
    SEAL23_16384.  With the 2^8 sizes the rule allows for, |v| still stays below B m_sk / 2 on the base the rule picks."""
    b = bases(name)
    sc, n = b.sc, b.n
    ones = bc.magnitude_D(1, 1, 5, 3, 64)                     # the closed form itself, against the exact convolution
    assert [p[:2] + p[-1:] for p in ones] == [[t * (2 - 64), t * (4 - 64), t * 64] for t in (1, 2, 3, 3, 3, 2, 1)]
    assert ones[0] == polymul_negacyclic([1] * 64, [1] * 64)
    H = sc.Q // 2
    la = sc.lift([H % p for p in b.q])["value"]
    lb = sc.lift([(H + 1) % p for p in b.q])["value"]
    assert la == H and lb in (H + 1, H + 1 - sc.Q)
    half = sc.B * sc.msk // 2
    print("\n[%s] n = %d, k = %d, auxiliary primes of %d bits; lift(ceil(q/2)) = %s" % (name, n, b.k, b.aux["bits"], "ceil(q/2)" if lb > 0 else "-floor(q/2)"))
    for sa, sb in MAGNITUDE_SIZES[name]:
        s = min(sa, sb)
        D = bc.magnitude_D(la, la, sa, sb, n)[s - 1]
        assert D[n - 1] == s * n * H * H and D[0] == -s * (n - 2) * H * H
        bound = s * n * b.t * sc.Q // 4
        for d in (D[n - 1], D[0]):
            fl = sc.floor(d)
            assert fl["result"] == [fl["v"] % p for p in b.q]
            assert bound // 2 <= abs(fl["v"]) <= bound and abs(fl["v"]) < half
            assert -fl["v"] // sc.B - 1 <= fl["alpha"] <= -fl["v"] // sc.B + b.k + 1
            assert abs(fl["alpha"]) > b.k or _alpha_floor(b, s) <= b.k
            print("  %2d x %2d  v = %s2^%.2f  (bound s n t q / 4 = 2^%.2f)   alpha_sk = %+d   slack to B m_sk / 2 = 2^%.2f: %.2f bits"
                  % (sa, sb, "-" if fl["v"] < 0 else "+", math.log2(abs(fl["v"])), math.log2(bound), fl["alpha"], math.log2(half),
                     math.log2(half) - math.log2(abs(fl["v"]))))
    worst = sc.floor(256 * n * H * H)
    assert abs(worst["v"]) < half and worst["result"] == [worst["v"] % p for p in b.q]
    print("  sizes 2^8: |v| = 2^%.2f, slack %.2f bits, alpha_sk = %+d" % (math.log2(abs(worst["v"])), math.log2(half) - math.log2(abs(worst["v"])), worst["alpha"]))

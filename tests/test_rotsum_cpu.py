"""CPU: the specification of the hoisted special-prime rotations (tests/rotsum_oracle.py) -- its residue form on the oracle's transforms
agrees with its big-integer form (digits sigma_g(d_i) over Z) on every base the GPU tests use; its bits are NOT those of the op-by-op
rotation, and the difference of the accumulators is exactly the stated one; a toy BFV in Python integers decrypts the fused sum to
sum_j w_j rot_j(m) slot by slot, as the op-by-op composition does, and keeps the budget circuits.rotate_sum_budget promises; the wrong
variants of the arithmetic are caught; the refusals that need no device; the plan's host code under the host sanitizers."""
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import galois_oracle as go
import keyswitch_sp_oracle as ks
import modswitch_oracle as mo
import rotsum_oracle as rs
import test_keyswitch_sp_cpu as tk

BASES = mo.bases(1024)
N_SMALL = 64
T = go.T_BATCH
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _taps5(n):
    return [1, 3, 2 * n - 1, pow(3, n // 8, 2 * n), pow(3, -1, 2 * n)]


def _setup(om, name, elts, seed, n=N_SMALL):
    """(oracle, ct [2][L][n], coefficient-form keys, oracle-form keys) with one test key per tap under a random ternary secret"""
    q = BASES[name]
    orc = tk._oracle(om, name, n)
    rng = np.random.default_rng(seed)
    sk = tk._ternary(rng, q, n)
    kc = [None if g == 1 else ks.switch_key(orc, sk, go.sigma(sk, g, q), seed=g) for g in elts]
    ko = [None if k is None else ks.key_to_oracle(orc, k) for k in kc]
    ct = tk._random_ct(rng, q[:-1], 2, n)
    ct[:, :, :4] = [[0, 1, qi - 1, qi - 2] for qi in q[:-1]]
    return orc, ct, kc, ko


# ---- (a) the two restatements agree --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BASES))
def test_residue_form_equals_the_big_integer_form(oracle_mod, name):
    q, n = BASES[name], N_SMALL
    elts = _taps5(n)
    weights = rs.edge_weights(T) + [T - 7]
    orc, ct, kc, ko = _setup(oracle_mod, name, elts, seed=len(name))
    for g in elts:                                                      # pi_g IS the permutation of the transform of sigma_g, on every prime
        if g == 1:
            continue
        for r in range(len(q)):
            a = np.random.default_rng(g + r).integers(0, q[r], size=n, dtype=np.uint64)
            assert np.array_equal(orc.ntt_fwd(a, r)[rs.slot_perm(orc, g, r)], orc.ntt_fwd(go.sigma(a[None], g, [q[r]])[0], r)), (name, g, r)
            assert np.array_equal(rs.slot_perm(orc, g, r), rs.slot_perm(orc, g, 0))          # one table serves every prime
    for sel in ([1], [0, 1], [0, 1, 2, 3, 4]):
        e, w = [elts[j] for j in sel], [weights[j] for j in sel]
        got = rs.rotate_sum(orc, ct, T, e, w, [ko[j] for j in sel])
        assert np.array_equal(got, rs.rotate_sum_big(q, T, ct, e, w, [kc[j] for j in sel])), (name, e)
    each = rs.rotate_each(orc, ct, T, elts, ko)
    assert np.array_equal(each[0], ct)
    for j in range(1, len(elts)):
        assert np.array_equal(each[j], rs.rotate_sum_big(q, T, ct, [elts[j]], [1], [kc[j]])), (name, elts[j])


# ---- (b) the correction: not the bits of the op-by-op rotation -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BASES))
def test_one_tap_differs_from_the_op_by_op_rotation_by_exactly_the_stated_terms(oracle_mod, name):
    """G = 1, w = 1 against keyswitch_sp_oracle.apply_galois on random input: other bits, and the accumulators differ by
    sum_i (q_i mod q_r) M_i (*) K_i, M_i the mask of the negated non-zero coefficients (q_i - x against -x modulo q_r)"""
    q, n = BASES[name], N_SMALL
    for g in (3, 2 * n - 1):
        orc, ct, _, ko = _setup(oracle_mod, name, [g], seed=g)
        hoisted = rs.rotate_sum(orc, ct, T, [g], [1], ko)
        op = ks.apply_galois(orc, ct, g, ko[0])
        assert not np.array_equal(hoisted, op), "hoisting is NOT bit-identical to op-by-op"
        a_h = rs.accumulators(orc, rs.digits(orc, ct[1]), [g], [1], ko)
        a_o = rs.op_by_op_accumulators(orc, ct, g, ko[0])
        diff = rs.accumulator_difference(orc, ct, g, ko[0])
        for r, qr in enumerate(q):
            assert np.array_equal((a_o[:, r].astype(object) - a_h[:, r].astype(object)) % qr, diff[:, r].astype(object)), (name, g, r)
        assert int((diff != 0).sum()) > 0
        print("[rotsum %s g=%d] %d of %d outputs differ from the op-by-op rotation" % (name, g, int((hoisted != op).sum()), hoisted.size))


# ---- (c) decryption and noise on a toy BFV ---------------------------------------------------------------------------------------------------
def _slots_of(plain, n, t):
    return [int(v) for v in go.decode_slots(plain, n, t)]


@pytest.mark.parametrize("name,n", [("Q3", 32), ("Q4", 32), ("Q4", 64)])
def test_toy_bfv_rotate_sum_decrypts_slot_by_slot_within_the_noise_bound(fhe, name, n):
    """the fused sum and the op-by-op composition (rotate, multiply by the constant, add) of one encryption decrypt to
    sum_j w_j rot_j(m) modulo t in every slot; the EXACT budget of the fused result is at or above rotate_sum_budget of the exact budget
    before (keys' noise drawn up to the sampler's largest value); the op-by-op budget is printed beside it"""
    t = T
    B = fhe.package.keys._Sampler.NOISE_MAX
    q = BASES[name]
    ctx = SimpleNamespace(n=n, t=t, q=q, k=len(q))
    Q = mo.prod(q[:-1])
    rng = np.random.default_rng(n + len(name))
    s = [int(v) - 1 for v in rng.integers(0, 3, size=n)]
    slots = [int(v) for v in rng.integers(0, t, size=n)]
    m = [int(v) for v in go.encode_slots(slots, n, t)]
    assert _slots_of(m, n, t) == slots
    a = tk._encrypt(rng, m, s, Q, t)
    worst, plain = tk._worst(a, s, Q, t)
    assert plain == m
    fresh = tk._exact_budget(Q, worst)
    moves = {g: (left, swap) for g, left, swap in go.elements(n)}
    moves[1] = (0, False)
    elts = _taps5(n)
    weights = rs.edge_weights(t) + [t - 7]
    K = []
    for g in elts:
        sg = s if g == 1 else [tk._centre(v, 3) for v in ks.sigma_big([v % 3 for v in s], g, 3)]
        K.append(None if g == 1 else tk._toy_key(rng, q, s, sg, B))
    want = np.zeros(n, dtype=object)
    for g, w in zip(elts, weights):
        want = (want + w * go.permute_slots(np.array(slots, dtype=object), *moves[g])) % t
    fused = rs.rotate_sum_composed(q, t, a, elts, weights, K)
    worst, plain = tk._worst(fused, s, Q, t)
    assert _slots_of(plain, n, t) == [int(v) for v in want]
    after = tk._exact_budget(Q, worst)
    bound = fhe.circuits.rotate_sum_budget(ctx, fresh, weights)
    # op-by-op: keyswitch_sp_oracle's rotation per tap, the centred constant, the sum
    acc = [[0] * n, [0] * n]
    for g, w, Kj in zip(elts, weights, K):
        if g == 1:
            rot = a
        else:
            sig = [ks.sigma_big(p, g, Q) for p in a]
            u = ks.key_switch_composed(q, [[v % qi for v in sig[1]] for qi in q[:-1]], Kj)
            rot = [[(x + y) % Q for x, y in zip(sig[0], u[0])], u[1]]
        acc = [[(x + rs.centred(w, t) * y) % Q for x, y in zip(acc[pp], rot[pp])] for pp in range(2)]
    worst_op, plain_op = tk._worst(acc, s, Q, t)
    assert plain_op == plain, "the fused sum and the op-by-op composition decrypt to the same plaintext"
    assert fused != acc, "and are not the same ciphertext"
    print("\n[toy BFV rotate_sum %s n=%d t=%d taps=%d sum|w'|=%d] fresh %.1f bits -> fused %.1f, op-by-op %.1f (bound %.1f)"
          % (name, n, t, len(elts), sum(abs(rs.centred(w, t)) for w in weights), fresh, after, tk._exact_budget(Q, worst_op), bound))
    assert after >= bound - 1e-9


def test_budget_formula(fhe):
    import math
    from fractions import Fraction
    c = fhe.circuits
    B19 = fhe.package.keys._Sampler.NOISE_MAX
    for q, n, t in ((BASES["Q4"], 8192, 65537), (BASES["Q3"], 4096, 65537)):
        ctx = SimpleNamespace(n=n, t=t, q=q)
        p, Q = q[-1], mo.prod(q[:-1])
        for budget in (40, 77.5):
            for weights in ([1], [1] * 9, [1, 4, 6, 4, 1, t - 2, (t + 1) // 2]):
                W = sum(abs(rs.centred(w, t)) for w in weights)
                E = Fraction(W * n * B19 * sum(qi - 1 for qi in q[:-1]), p) + Fraction(1 + n, 2)
                want = -math.log2(W * Fraction(2.0 ** -budget) + 2 * t * E / Q)
                assert c.rotate_sum_budget(ctx, budget, weights) == pytest.approx(want, abs=1e-6)
            assert c.rotate_sum_budget(ctx, budget, [1]) == pytest.approx(c.special_key_switch_budget(ctx, budget), abs=1e-9)
        print("[rotate_sum_budget n=%d k=%d] a box 3x3 at 100 bits keeps %.2f, nine op-by-op rotations' bound %.2f"
              % (n, len(q), c.rotate_sum_budget(ctx, 100, [1] * 9), -math.log2(9 * 2.0 ** -c.special_key_switch_budget(ctx, 100))))
    with pytest.raises(ValueError):
        c.rotate_sum_budget(SimpleNamespace(n=1024, t=65537, q=BASES["Q3"][:1]), 50, [1])
    with pytest.raises(ValueError):
        c.rotate_sum_budget(SimpleNamespace(n=1024, t=65537, q=BASES["Q3"]), 50, [1, 65537])
    with pytest.raises(ValueError):
        c.rotate_sum_budget(SimpleNamespace(n=1024, t=65537, q=BASES["Q3"]), 50, [])


# ---- (d) wrong variants, in the model only --------------------------------------------------------------------------------------------------
def test_wrong_variants_are_caught(oracle_mod):
    """(changed crafted outputs, crafted outputs, changed random outputs, random outputs) per variant, Q4 at n = 64, taps {1, 3, 2n - 1,
    3^(n/8), 3^-1}.  Crafted: c_0 and c_1 of family R (keyswitch_sp_oracle.reduction_poly: 0, 1, q_i - 1 and the values around the other
    primes) under the edge weights 1, t - 1, (t - 1)/2, (t + 1)/2.
         perm_inv    pi_g replaced by pi_(g^-1): any data
         uncentred   w instead of w - t for a weight above t/2: every output of a sum with such a weight
         no_id_c1    the identity tap's w' c_1 left out: the second polynomial wherever c_1 is non-zero
         neg_q0      sum w' sigma(c_0) negated modulo q_0 where q_r is meant: the negated non-zero positions of the residues r != 0
    Counts of this run: perm_inv 384 of 384 / 384 of 384, uncentred 384 / 384, no_id_c1 168 / 189, neg_q0 94 / 98."""
    name, n = "Q4", N_SMALL
    q = BASES[name]
    elts = _taps5(n)
    weights = rs.edge_weights(T) + [T - 7]
    orc, rand, _, ko = _setup(oracle_mod, name, elts, seed=11)
    crafted = np.stack([ks.reduction_poly(q, n, 3), ks.reduction_poly(q, n, 2 * n - 1)])
    report = {}
    for variant in rs.VARIANTS:
        row = []
        for ct in (crafted, rand):
            good = rs.rotate_sum(orc, ct, T, elts, weights, ko)
            bad = rs.rotate_sum(orc, ct, T, elts, weights, ko, variant=variant)
            row += [int((good != bad).sum()), good.size]
        report[variant] = tuple(row)
    print("\n[rotate_sum: wrong variants] variant: (crafted changed, crafted, random changed, random) = %r" % report)
    for variant, (cb, ca, rb, ra) in report.items():
        assert cb > 0, variant
    assert report["perm_inv"][2] > report["perm_inv"][3] // 2
    assert report["uncentred"][0] > report["uncentred"][1] // 2 and report["uncentred"][2] > report["uncentred"][3] // 2
    assert report["no_id_c1"][2] >= report["no_id_c1"][3] // 2 - 8           # the whole second polynomial of random data
    assert report["neg_q0"][2] > 0
    # uncentred changes nothing when no weight is above t/2
    small = [1, 2, 3, (T - 1) // 2, 5]
    assert np.array_equal(rs.rotate_sum(orc, rand, T, elts, small, ko), rs.rotate_sum(orc, rand, T, elts, small, ko, variant="uncentred"))


@pytest.mark.parametrize("name", ["Q58", "Q4", "S16K"])
def test_the_tap_sum_needs_its_fold_at_64_taps(name):
    """family U of the key switch, extended over taps (rotsum_oracle.TapEdge): every lazy digit product AND every weighted tap term is at
    or above q_r.  With the fold every 32 taps the 64-tap sum stays in 64 bits and folds to the canonical sum plus at most one q_r.

    One fold of the tap sum dropped, in the u64() model: at the bound the kernel's static_assert reasons with (a term below RQ / 16 q, the
    figure the host checks mulvv_pm's result against) 64 terms of 1.5 q wrap on the 58-bit base -- u64() raises -- and 64 terms of 6 q on
    a 55-bit prime only just fit; that is why the kernel folds.  The products themselves cannot get there: for a weight below 2^43 the two
    folds inside mulvv_pm leave tau + q with tau < delta = 2^b - q, so a term is at most 2^b - 1 and 64 of them at most 2^64 - 64.  Measured
    here on Q58 (delta = 28671) with every term crafted above q: the unfolded 64-tap sum reaches 2^64 - 64 delta + sum tau, i.e. more than
    0.99999 * 2^64, and does not wrap; with the fold the largest register is 0.516 * 2^64."""
    from test_pm_arithmetic_model import Pm, cls_of, fold_pm, mulvv_pm
    q = BASES[name]
    E = rs.TapEdge(q, 1024, T)
    for r in range(len(q)):
        m = Pm(q[r])
        terms = E.slot_terms(r, rs.MAX_TAPS, s=3 * r, pp=r & 1)
        lazy = [mulvv_pm(fold_pm(sum(mulvv_pm(a, e, m) for a, e in pairs), m), w, m) for pairs, w in terms]
        assert all(q[r] <= v < 1 << m.b for v in lazy), "a term of the tap sum is not above q"
        assert all(mulvv_pm(a, e, m) >= q[r] for pairs, _ in terms for a, e in pairs[1:]), "a digit product is not above q"
        exact = sum(sum(a * e for a, e in pairs) * w for pairs, w in terms)
        folded, top = rs.tap_sum_model(terms, m)
        assert folded % q[r] == exact % q[r] and folded < 2 * q[r] and top < 1 << 64
        folded2, top2 = rs.tap_sum_model(terms, m, fold_every=None)
        assert folded2 % q[r] == exact % q[r] and top2 >= rs.MAX_TAPS * q[r]
        print("[rotsum tap sum %s prime %d, %d bits] 64 taps, every term above q: largest register %.6f * 2^64 with the fold every %d, %.6f * 2^64 without"
              % (name, r, m.b, top / 2.0 ** 64, rs.FOLD_TAPS, top2 / 2.0 ** 64))
    # the bound the static_assert works with: sixteenths of q per term (ntt_core.h PmA / PmB)
    rq = {"Q58": 24, "Q4": 96, "S16K": 96}[name]
    for qr in q:
        assert rs.tap_sum_bound_model(rs.MAX_TAPS, rq, qr) < 1 << 64
        if name == "Q58":
            with pytest.raises(AssertionError, match="64-bit register overflow"):
                rs.tap_sum_bound_model(rs.MAX_TAPS, rq, qr, fold_every=None)
        else:
            assert rs.tap_sum_bound_model(rs.MAX_TAPS, rq, qr, fold_every=None) < 1 << 64      # class A: 384 q of 512


# ---- (e) refusals that need no device, and the library's entry points ------------------------------------------------------------------------
def test_host_side_refusals(fhe):
    n, t = 1024, T
    level = SimpleNamespace(n=n, t=t, k=3, q=BASES["Q4"][:3], device="cpu")
    parent = SimpleNamespace(n=n, t=t, k=4, q=BASES["Q4"], device="cpu", h=None)
    keys = fhe.SpecialGaloisKeys(parent, {})
    mk = lambda e, w=None, k=keys, **kw: fhe.RotSumPlan(level, k, e, w, **kw)
    for bad, what in (([], "taps"), (list(range(1, 131, 2)), "taps"), ([4], "odd"), ([2 * n + 1], "odd"), ([0], "odd"), ([3, 5, 3], "repeated")):
        with pytest.raises(ValueError, match=what):
            mk(bad)
    with pytest.raises(ValueError, match="0 modulo t"):
        mk([1, 3], [1, 2 * t])
    with pytest.raises(ValueError, match="weights for"):
        mk([1, 3], [1])
    with pytest.raises(ValueError, match="no special Galois key for element 3"):
        mk([1, 3])
    with pytest.raises(ValueError, match="no special Galois key"):
        mk([1], steps=True)                                             # one step to the left is element 3
    with pytest.raises(ValueError, match="SpecialGaloisKeys expected"):
        mk([1], k=fhe.GaloisKeys(parent, 30, {}))
    for elts, weights, why in (([1, 3], [1, 1], None), ([], [], "tap count"), ([3, 3], [1, 1], "repeated"), ([2], [1], "odd"), ([3], [t], "0 modulo t")):
        got = rs.check_taps(n, t, 2, elts, weights)
        assert (got is None) if why is None else (why in got)
    assert rs.check_taps(n, t, 1, [3], [1]) is not None
    elts, ws = fhe.circuits.packed_filter_taps(n, t, 32, [1, 0, t - 1, 2, 5, 2, t, 3, 1], 3, 3)
    assert elts == [e for e, w in zip(rs.filter_elements(n, 32, 3, 3), [1, 0, 1, 1, 1, 1, 0, 1, 1]) if w] and ws == [1, t - 1, 2, 5, 2, 3, 1] and elts[3] == 1
    with pytest.raises(ValueError, match="every weight is zero"):
        fhe.circuits.packed_filter_taps(n, t, 32, [0] * 9, 3, 3)


def test_library_exports_the_entry_points(fhe):
    lib = fhe._lib.load()
    header = open(fhe.HEADER_PATH).read()
    for name in ("fhe_rotsum_plan_create", "fhe_rotsum_plan_destroy", "fhe_rotsum_scratch_bytes", "fhe_rotate_sum_sp", "fhe_rotate_each_sp"):
        assert hasattr(lib, name) and name in fhe._lib.SIGNATURES and name in header, name
    assert lib.fhe_rotsum_scratch_bytes(None, 3, 0) == 0 and lib.fhe_rotsum_plan_destroy(None) == 0
    assert lib.fhe_rotsum_plan_create(None, 1, None, None, None, None) == -1
    assert lib.fhe_rotate_sum_sp(None, None, 0, None, 0, 1, None, 0, None) == -1
    assert lib.fhe_rotate_each_sp(None, None, 0, None, 0, 0, 1, None, 0, None) == -1
    assert "bit-identical to op-by-op" not in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- (f) the plan's host code under the host sanitizers ---------------------------------------------------------------------------------------
def test_plan_host_code_under_address_and_undefined_sanitizers(tmp_path):
    """tools/rotsum_host_check.cpp: a program of its own around csrc/rotsum_host.h (no device, nothing loaded into Python), built with
    -fsanitize=address,undefined and run once"""
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rotsum_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "rotsum_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.stdout[-2000:], out.stderr[-2000:])

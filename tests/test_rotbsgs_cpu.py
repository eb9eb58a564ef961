"""CPU: the specification of the baby-step / giant-step linear maps on encrypted slots (tests/rotbsgs_oracle.py) -- its residue form on the
oracle's transforms agrees with its big-integer form on every base the GPU tests use; with one identity giant step it reproduces
tests/rotdiag_oracle.py bit for bit, with one giant step over the constant 1 tests/rotsum_oracle.py; the wrong variants are caught; a toy
BFV decrypts slot by slot within circuits.rotate_bsgs_budget; the host helpers (bsgs_split, block_matvec_bsgs, block_dct2d_matrix)
against plain numpy; the refusals that need no device; the plan's host code under the host sanitizers."""
import math
import os
import shutil
import subprocess
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

import galois_oracle as go
import keyswitch_sp_oracle as ks
import modswitch_oracle as mo
import rotbsgs_oracle as ro
import rotdiag_oracle as rd
import rotsum_oracle as rs
import test_keyswitch_sp_cpu as tk
import test_rotsum_cpu as tr

BASES = mo.bases(1024)
N_SMALL = 64
T = go.T_BATCH
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lists(n):
    """baby (1 first), giant (1 in the middle); 3 is in both lists"""
    return [1, 3, 2 * n - 1], [pow(3, n // 8, 2 * n), 1, 3]


def _plains(n, G1, G2, seed, absent=((0, 1), (2, 0))):
    """[G2][G1][n]: random dense with the edge coefficients in front, one pair (t - 1) X^(n-1), the pairs in `absent` all zero"""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, T, size=(G2, G1, n), dtype=np.uint64)
    out[:, :, :5] = [0, 1, T - 1, (T - 1) // 2, (T + 1) // 2]
    out[-1, -1] = 0
    out[-1, -1, n - 1] = T - 1
    for i, j in absent:
        if i < G2 and j < G1:
            out[i, j] = 0
    return out


def _setup(om, name, baby, giant, seed):
    """(oracle, ct, coefficient-form and oracle-form keys of both lists) under ONE secret"""
    orc, ct, kc, ko = tr._setup(om, name, list(baby) + list(giant), seed)
    G1 = len(baby)
    return orc, ct, (kc[:G1], kc[G1:]), (ko[:G1], ko[G1:])


# ---- (a) the restatements agree --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BASES))
def test_residue_form_equals_the_big_integer_form(oracle_mod, name):
    q, n = BASES[name], N_SMALL
    baby, giant = _lists(n)
    orc, ct, (kbc, kgc), (kbo, kgo) = _setup(oracle_mod, name, baby, giant, seed=len(name) + 2)
    plains = _plains(n, 3, 3, seed=len(name))
    for bs, gs in (([0, 1, 2], [0, 1, 2]), ([1], [0]), ([0], [1]), ([0, 1], [2, 0])):
        b, g = [baby[j] for j in bs], [giant[i] for i in gs]
        p = np.stack([np.stack([plains[i][j] for j in bs]) for i in gs])
        if ro.check_plan(n, T, len(q), b, g, p) is not None:             # a selection that leaves a row or a column without a pair
            p = _plains(n, len(b), len(g), seed=7, absent=())
        got = ro.rotate_bsgs(orc, ct, T, b, g, p, [kbo[j] for j in bs], [kgo[i] for i in gs])
        big = ro.rotate_bsgs_big(q, T, ct, b, g, p, [kbc[j] for j in bs], [kgc[i] for i in gs])
        assert np.array_equal(got, big), (name, b, g, np.argwhere(got != big)[:4])
        for r in range(len(q) - 1):
            assert int(got[:, r].max()) < q[r]


@pytest.mark.parametrize("name", list(BASES))
def test_identity_giant_reproduces_rotate_diag_sum(oracle_mod, name):
    """G2 = 1, h = {1}: drop(A) is rotdiag_oracle's structured form, the same bytes"""
    n = N_SMALL
    elts = tr._taps5(n)
    orc, ct, _, ko = tr._setup(oracle_mod, name, elts, seed=3)
    plains = _plains(n, len(elts), 1, seed=len(name) + 5, absent=())
    for sel in ([0], [1], [0, 1, 2, 3, 4]):
        e, k = [elts[j] for j in sel], [ko[j] for j in sel]
        p = plains[:, sel]
        assert np.array_equal(ro.rotate_bsgs(orc, ct, T, e, [1], p, k, [None]), rd.rotate_diag_sum(orc, ct, T, e, list(p[0]), k)), (name, e)


@pytest.mark.parametrize("name", list(BASES))
def test_one_giant_over_the_constant_one_reproduces_rotate_sum(oracle_mod, name):
    """G1 = 1, g = {1}, p = 1: A = p ct, v = c_1 exactly, and the giant step is rotsum_oracle's single tap of weight 1"""
    n = N_SMALL
    elts = tr._taps5(n)
    orc, ct, _, ko = tr._setup(oracle_mod, name, elts, seed=4)
    one = rd.constant(n, 1)[None, None]
    for h, key in zip(elts[1:], ko[1:]):
        assert np.array_equal(ro.rotate_bsgs(orc, ct, T, [1], [h], one, [None], [key]), rs.rotate_sum(orc, ct, T, [h], [1], [key])), (name, h)


# ---- (b) wrong variants, in the model only -------------------------------------------------------------------------------------------------
def test_wrong_variants_are_caught(oracle_mod):
    """(changed crafted outputs, crafted outputs, changed random outputs, random outputs) per variant, Q4 at n = 64, baby {1, 3, 2n - 1},
    giant {3^(n/8), 1, 3}, two absent pairs.  Crafted: c_0 and c_1 of family R.
         galois_digit  fhe_apply_galois_sp's digit (negate modulo q_l, then reduce) for v(i)
         a0_dropped    A(i)_0 dropped on its own before the giant step
         a0_no_perm    pi_(h_i) left off A(i)_0
         perm_inv      pi of the inverse element, in both lists
         giant_first   the giant rotation applied before the diagonal
         id_switched   the identity giant's A_1 dropped and key-switched too (with a key from s to s)
    Counts of this run: galois_digit, perm_inv, giant_first and id_switched change 384 of 384 crafted and 384 of 384 random outputs;
    a0_no_perm 189 of 384 each (the first polynomial); a0_dropped 51 of 384 crafted and 72 of 384 random outputs (one more rounding of
    c_0: the outputs whose two roundings do not cancel move by one)."""
    name, n = "Q4", N_SMALL
    q = BASES[name]
    baby, giant = _lists(n)
    orc, rand, _, (kbo, kgo) = _setup(oracle_mod, name, baby, giant, seed=11)
    rng = np.random.default_rng(5)
    sk = tk._ternary(rng, q, n)
    kgo = list(kgo)
    kgo[1] = ks.key_to_oracle(orc, ks.switch_key(orc, sk, sk, seed=9))    # only id_switched reads it
    plains = _plains(n, 3, 3, seed=2)
    crafted = np.stack([ks.reduction_poly(q, n, 3), ks.reduction_poly(q, n, 2 * n - 1)])
    report = {}
    for variant in ro.VARIANTS:
        row = []
        for ct in (crafted, rand):
            good = ro.rotate_bsgs(orc, ct, T, baby, giant, plains, kbo, kgo)
            bad = ro.rotate_bsgs(orc, ct, T, baby, giant, plains, kbo, kgo, variant=variant)
            row += [int((good != bad).sum()), good.size]
        report[variant] = tuple(row)
    print("\n[rotate_bsgs: wrong variants] variant: (crafted changed, crafted, random changed, random) = %r" % report)
    for variant, (cb, ca, rb, ra) in report.items():
        assert cb > 0, variant
        assert rb > 0, variant


# ---- (c) decryption and noise on a toy BFV -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("Q3", 32), ("Q4", 32), ("Q4", 64)])
def test_toy_bfv_decrypts_slot_by_slot_within_the_noise_bound(fhe, name, n):
    """one encryption through the definition in big integers: every slot is sum_i rot_(h_i)(sum_j d_(i,j) (.) rot_(g_j)(m)) modulo t, the
    EXACT budget is at or above rotate_bsgs_budget of the exact budget before"""
    t = T
    B = fhe.package.keys._Sampler.NOISE_MAX
    q = BASES[name]
    ctx = SimpleNamespace(n=n, t=t, q=q, k=len(q))
    Q = mo.prod(q[:-1])
    rng = np.random.default_rng(n + len(name) + 1)
    s = [int(v) - 1 for v in rng.integers(0, 3, size=n)]
    slots = [int(v) for v in rng.integers(0, t, size=n)]
    m = [int(v) for v in go.encode_slots(slots, n, t)]
    a = tk._encrypt(rng, m, s, Q, t)
    worst, plain = tk._worst(a, s, Q, t)
    assert plain == m
    fresh = tk._exact_budget(Q, worst)
    moves = {g: (left, swap) for g, left, swap in go.elements(n)}
    moves[1] = (0, False)
    baby, giant = _lists(n)
    diags = rng.integers(0, 2, size=(3, 3, n))                         # 0/1 masks ...
    diags[0, 2] = rng.integers(0, 4, size=n)                           # ... small weights ...
    diags[0, 1] = 0                                                    # ... and two absent pairs
    diags[2, 0] = 0
    plains = np.array([[[int(v) for v in go.encode_slots([int(x) for x in d], n, t)] for d in row] for row in diags], dtype=np.uint64)
    key = lambda g: None if g == 1 else tk._toy_key(rng, q, s, [tk._centre(v, 3) for v in ks.sigma_big([v % 3 for v in s], g, 3)], B)
    KB, KG = [key(g) for g in baby], [key(h) for h in giant]
    x = np.array(slots, dtype=object)
    want = np.zeros(n, dtype=object)
    for h, row in zip(giant, diags):
        inner = np.zeros(n, dtype=object)
        for g, d in zip(baby, row):
            inner = (inner + d.astype(object) * go.permute_slots(x, *moves[g])) % t
        want = (want + go.permute_slots(inner, *moves[h])) % t
    fused = ro.rotate_bsgs_composed(q, t, a, baby, giant, plains, KB, KG)
    worst, plain = tk._worst(fused, s, Q, t)
    assert tr._slots_of(plain, n, t) == [int(v) for v in want]
    after = tk._exact_budget(Q, worst)
    bound = fhe.circuits.rotate_bsgs_budget(ctx, fresh, plains, baby, giant)
    print("\n[toy BFV rotate_bsgs %s n=%d] fresh %.1f bits -> fused %.1f (bound %.1f)" % (name, n, fresh, after, bound))
    assert after >= bound - 1e-9


def test_budget_formula(fhe):
    c = fhe.circuits
    B19 = fhe.package.keys._Sampler.NOISE_MAX
    q, n, t = BASES["Q4"], 8192, 65537
    ctx = SimpleNamespace(n=n, t=t, q=q)
    p, Q = q[-1], mo.prod(q[:-1])
    S = sum(qi - 1 for qi in q[:-1])
    plains = np.zeros((2, 2, n), dtype=np.uint64)
    plains[0, 0, :3] = [1, t - 1, (t + 1) // 2]
    plains[0, 1, n - 1] = 5
    plains[1, 1, 0] = t - 2
    W = (1 + 1 + (t - 1) // 2 + 5) + 2
    for giant, Gn in (([1, 3], 1), ([5, 3], 2)):
        E = Fraction((W + Gn) * n * B19 * S, p) + Fraction(Gn * n, 2) + Fraction(1 + n, 2)
        for budget in (40, 77.5):
            want = -math.log2(W * Fraction(2.0 ** -budget) + 2 * t * E / Q)
            assert c.rotate_bsgs_budget(ctx, budget, plains, [1, 3], giant) == pytest.approx(want, abs=1e-6)
    one = plains[:1]
    assert c.rotate_bsgs_budget(ctx, 50, one, [1, 3], [1]) == pytest.approx(c.rotate_diag_budget(ctx, 50, one[0]), abs=1e-9)
    with pytest.raises(ValueError):
        c.rotate_bsgs_budget(ctx, 50, np.zeros((1, 1, n), dtype=np.uint64), [1], [1])
    with pytest.raises(ValueError):
        c.rotate_bsgs_budget(ctx, 50, plains, [1, 3], [1])
    with pytest.raises(ValueError):
        c.rotate_bsgs_budget(SimpleNamespace(n=n, t=t, q=q[:1]), 50, plains, [1, 3], [1, 3])


# ---- (d) the host helpers against plain numpy ------------------------------------------------------------------------------------------------
def _apply_bsgs(n, baby, giant, diags, slots, t):
    """sum_i rot_(h_i)(sum_j d_(i,j) (.) rot_(g_j)(slots)) on flat slots from signed STEPS: step s rotates both rows LEFT by s"""
    half = n // 2
    rows = np.asarray(slots, dtype=object).reshape(2, half)
    out = np.zeros((2, half), dtype=object)
    for h, drow in zip(giant, diags):
        inner = np.zeros((2, half), dtype=object)
        for g, d in zip(baby, drow):
            inner = (inner + np.asarray(d, dtype=object).reshape(2, half) * np.roll(rows, -g, axis=1)) % t
        out = (out + np.roll(inner, -h, axis=1)) % t
    return out.reshape(n)


def _blocks(B, x, n, t):
    d = B.shape[0]
    return (np.einsum("ab,gb->ga", B.astype(object), np.asarray(x).reshape(n // d, d).astype(object)) % t).reshape(n)


@pytest.mark.parametrize("n,d,baby", [(1024, 8, 4), (256, 64, 16), (1024, 8, None), (256, 2, 1)])
def test_block_matvec_bsgs_against_numpy(fhe, n, d, baby):
    c = fhe.circuits
    t = T
    rng = np.random.default_rng(d + n)
    B = rng.integers(-300, 300, size=(d, d))
    bs, gs, diags = c.block_matvec_bsgs(n, t, B, baby)
    b = baby if baby else 1 << int(round(math.log2(math.sqrt(2 * d - 1))))
    assert bs == list(range(min(b, 2 * d - 1))) and all(g % b == 0 for g in gs) and gs == sorted(gs) and gs[0] < 0 < gs[-1]
    assert diags.shape == (len(gs), len(bs), n)
    assert len(bs) + len(gs) - 1 - (0 in gs) <= 2 * d - 2                # no more keys than the diagonal method
    if (d, baby) == (64, 16):
        assert (len(bs), len(gs)) == (16, 8) and len(bs) - 1 + len(gs) - 1 == 22
    x = rng.integers(0, t, size=n)
    assert np.array_equal(_apply_bsgs(n, bs, gs, diags, x, t), _blocks(B, x, n, t))
    pr = diags.any(axis=2)                                              # what RotBsgsPlan asks of a plan
    assert pr.any(axis=0).all() and pr.any(axis=1).all()


def test_bsgs_split_negative_wrapping_and_missing_steps(fhe):
    c = fhe.circuits
    n, t = 256, T
    half = n // 2
    rng = np.random.default_rng(3)
    steps = [-9, -1, 0, 2, 7, half - 3, 40, -half + 5]                  # negative, wrapping (half - 3 = -3, -half + 5 = 5), gaps
    d = rng.integers(0, t, size=(len(steps), n), dtype=np.uint64)
    x = rng.integers(0, t, size=n)
    want = np.zeros(n, dtype=object)
    for s, row in zip(steps, d):
        want = (want + (row.astype(object).reshape(2, half) * np.roll(np.asarray(x, dtype=object).reshape(2, half), -s, axis=1)).reshape(n)) % t
    for baby in (None, 1, 4, 8, 64):
        bs, gs, diags = c.bsgs_split(n, steps, d, baby)
        assert int(diags.any(axis=2).sum()) == len(steps)
        assert np.array_equal(_apply_bsgs(n, bs, gs, diags, x, t), want), baby
    bs, gs, _ = c.bsgs_split(n, steps, d, 4)
    assert bs == [0, 1, 2, 3] and gs == sorted(set(4 * (s // 4) for s in steps))
    # a matrix with missing diagonals: lower triangular, and one with a single off-diagonal
    for B in (np.tril(np.ones((8, 8), dtype=np.int64)), np.eye(8, k=5, dtype=np.int64) * 7 + np.eye(8, dtype=np.int64)):
        bs, gs, diags = c.block_matvec_bsgs(n, t, B, 4)
        assert np.array_equal(_apply_bsgs(n, bs, gs, diags, x, t), _blocks(B, x, n, t))
    with pytest.raises(ValueError, match="same rotation"):
        c.bsgs_split(n, [1, 1 + half], d[:2])
    with pytest.raises(ValueError, match="diagonals of shape"):
        c.bsgs_split(n, [1, 2], d[:3])
    with pytest.raises(ValueError, match="baby"):
        c.bsgs_split(n, [1, 2], d[:2], 0)


@pytest.mark.parametrize("bits", [4, 8])
def test_block_dct2d_matrix_is_rows_then_columns(fhe, bits):
    c = fhe.circuits
    D = c.dct8_matrix(bits).astype(object)
    M = c.block_dct2d_matrix(bits)
    assert M.shape == (64, 64) and M.dtype == np.int64
    rng = np.random.default_rng(bits)
    for _ in range(3):
        X = rng.integers(-128, 128, size=(8, 8)).astype(object)
        rows = X.dot(D.T)                                               # the DCT of every row
        want = D.dot(rows)                                              # then of every column
        assert np.array_equal(M.astype(object).dot(X.reshape(64)), want.reshape(64))


# ---- (e) refusals that need no device, and the library's entry points ---------------------------------------------------------------------------
def test_host_side_refusals(fhe):
    n, t = 1024, T
    level = SimpleNamespace(n=n, t=t, k=3, q=BASES["Q4"][:3], device="cpu")
    parent = SimpleNamespace(n=n, t=t, k=4, q=BASES["Q4"], device="cpu", h=None)
    keys = fhe.SpecialGaloisKeys(parent, {})
    ones = lambda G2, G1: np.ones((G2, G1, n), dtype=np.uint64)
    mk = lambda b, g, d=None, k=keys, **kw: fhe.RotBsgsPlan(level, k, b, g, ones(len(g), len(b)) if d is None else d, **kw)
    many = list(range(1, 131, 2))
    for b, g, what in (([], [1], "baby steps"), ([1], [], "giant steps"), (many, [1], "baby steps"), ([1], many, "giant steps"), ([4], [1], "odd"),
                       ([1], [2 * n + 1], "odd"), ([0], [1], "odd"), ([3, 5, 3], [1], "baby Galois element 3 is repeated"), ([1], [5, 5], "giant Galois element 5 is repeated")):
        with pytest.raises(ValueError, match=what):
            mk(b, g)
    with pytest.raises(ValueError, match="diagonals of shape"):
        mk([1, 3], [1], ones(2, 1))
    d = ones(2, 2)
    d[1] = t                                                            # 0 modulo t
    with pytest.raises(ValueError, match="giant step 1 has no present pair"):
        mk([1, 3], [1, 5], d)
    d = ones(2, 2)
    d[:, 0] = 0
    with pytest.raises(ValueError, match="baby step 0 has no present pair"):
        mk([1, 3], [1, 5], d)
    with pytest.raises(ValueError, match="no special Galois key for element 3"):
        mk([1, 3], [1])
    with pytest.raises(ValueError, match="no special Galois key for element 5"):
        mk([1], [1, 5])
    with pytest.raises(ValueError, match="SpecialGaloisKeys expected"):
        mk([1], [1], k=fhe.GaloisKeys(parent, 30, {}))
    one = rd.constant(n, 1)
    zero = np.zeros(n, dtype=np.uint64)
    good = [[one, one], [one, zero]]
    for b, g, p, why in (([1, 3], [1, 5], good, None), ([], [1], [[]], "baby step count"), ([1], [], [], "giant step count"), ([3, 3], [1], good[:1], "repeated"),
                         ([1, 3], [5, 5], good, "repeated"), ([2], [1], [[one]], "odd"), ([1, 3], [1, 5], [[one, zero], [one, zero]], "baby step 1 has no present pair"),
                         ([1, 3], [1, 5], [[one, one], [zero, zero]], "giant step 1 has no present pair"), ([3], [1], [[rd.constant(n, t)]], "not below t"),
                         ([1, 3], [1, 5], good[:1], "expected")):
        got = ro.check_plan(n, t, 2, b, g, p)
        assert (got is None) if why is None else (why in got), (b, g, got)
    assert ro.check_plan(n, t, 1, [3], [1], [[one]]) is not None


def test_library_exports_the_entry_points(fhe):
    lib = fhe._lib.load()
    header = open(fhe.HEADER_PATH).read()
    for name in ("fhe_rotbsgs_plan_create", "fhe_rotbsgs_plan_destroy", "fhe_rotbsgs_scratch_bytes", "fhe_rotate_bsgs_sp"):
        assert hasattr(lib, name) and name in fhe._lib.SIGNATURES and name in header, name
    assert lib.fhe_rotbsgs_scratch_bytes(None, 3) == 0 and lib.fhe_rotbsgs_plan_destroy(None) == 0
    assert lib.fhe_rotbsgs_plan_create(None, 1, None, 1, None, None, None, None, None) == -1
    assert lib.fhe_rotate_bsgs_sp(None, None, 0, None, 0, 1, None, 0, None) == -1
    assert lib.fhe_abi_version() == 4


# ---- (f) the plan's host code under the host sanitizers -------------------------------------------------------------------------------------
def test_plan_host_code_under_address_and_undefined_sanitizers(tmp_path):
    """tools/rotbsgs_host_check.cpp: a program of its own around csrc/rotbsgs_host.h (no device, nothing loaded into Python), built with
    -fsanitize=address,undefined and run once"""
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rotbsgs_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "rotbsgs_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.stdout[-2000:], out.stderr[-2000:])
